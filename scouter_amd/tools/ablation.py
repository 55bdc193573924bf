"""Occlusion maps and Ablation-CAM as rows of the two explanation tools: the single-image tool (scouter_amd/test.py) and the
explanation table over a validation set (tools/explanation_table.py), both with two more families on top of tools/surrogate.py's.

    occlusion    occlusion sensitivity: the mean drop of the class probability over the windows that covered a pixel
                 (tools/attribution.py occlusion)
    ablationcam  Ablation-CAM: the backbone's channels weighted by the relative drop of the class probability when each is zeroed
                 (tools/attribution.py ablationcam)

The tables of the tools are pinned (test.FAMILIES, explanation_table.FAMILIES, surrogate.FAMILIES), so the two rows live here:
FAMILIES is the surrogate tool's families plus these, the parser is that tool's plus their flags and options, and both tools run on
the extended table through their `rows=` / `families=` arguments.  Every flag and option of the three tools keeps its name,
default and meaning.

    --table_images 0 (the default)   the single-image tool: `--occlusion true` / `--ablationcam true` write occlusion_{c}.png /
                                     ablationcam_{c}.png of every class into --vis_dir, and --causal / --infidelity / --sensitivity
                                     print their lines for them
    --table_images N > 0             the explanation table over N validation images: one `table occlusion:` / `table ablationcam:`
                                     line each

occlusion takes --occlusion_window and --occlusion_stride (pixels, the same for rows and columns), --occlusion_fill (the value
that fills the window) and --occlusion_batch (rows per forward, the clean image included); ablationcam takes --ablationcam_batch
(rows per head pass, the clean features included).

    python -m scouter_amd.tools.ablation --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --occlusion true --ablationcam true [--causal true] [--table_images 64 --batch_size 16 --localization true]"""
import argparse

from .. import test as T
from ..train import _flag
from . import explanation_table as E
from . import surrogate as S

_O = T.Option

ABLATIONS = (
    T.Family("occlusion", "occlusion map", maps="occlusion_maps", explain="occlusion", options=(
        _O("window", "window", int, 16, "side of the occluding window in pixels"),
        _O("stride", "stride", int, 8, "step of the window in pixels (at most the window)"),
        _O("fill", "fill", float, 0.0, "the value that fills the window"),
        _O("batch", "batch", int, 250, "rows per forward, the clean image included"))),
    T.Family("ablationcam", "Ablation-CAM heat map", maps="ablationcam_maps", explain="ablationcam", options=(
        _O("batch", "batch", int, 256, "rows per head pass, the clean features included"),)),
)
FAMILIES = S.FAMILIES + ABLATIONS
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_ablation_parser():
    """the surrogate tool's parser (which holds the table tool's and the single-image tool's) plus the flag and the options of
    the two rows; --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("Occlusion maps and Ablation-CAM: one image, or a table over a validation set",
                                     parents=[S.get_surrogate_parser()], add_help=False)
    for row in ABLATIONS:
        parser.add_argument("--" + row.name, default=False, type=_flag,
                            help="true: the %s of every class as %s_{c}.png into --vis_dir, or its row of the table"
                                 % (row.what, row.name))
        for o in row.options:
            parser.add_argument("--%s_%s" % (row.name, o.suffix), default=o.default, type=o.type, choices=o.choices,
                                help="--%s: %s (default: %s)" % (row.name, o.help, o.default))
    parser.set_defaults(table_images=0)
    return parser


def option_kwargs(args, name):
    """the keyword arguments the options of the row `name` of this tool's table give its library functions"""
    return T.option_kwargs(args, name, _ROWS)


def main():
    args = get_ablation_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
