"""Layer IG, layer conductance, HiResCAM and LayerCAM as rows of the two explanation tools: the single-image tool
(scouter_amd/test.py) and the explanation table over a validation set (tools/explanation_table.py), both with four more families on
top of tools/ablation.py's.  All four attribute to the backbone's output, the layer the reference's captum_vis.py attributes to.

    layerig      Layer Integrated Gradients: a straight line in FEATURE space from the baseline image's features to the image's,
                 through the head alone (tools/attribution.py layer_integrated_gradients)
    conductance  Layer Conductance: a straight line in IMAGE space, the gradient at the layer times the layer's step, summed
                 (tools/attribution.py layer_conductance)
    hirescam     HiResCAM: gradient times activation per position, summed over the channels (tools/attribution.py hirescam)
    layercam     LayerCAM: the positive gradient times activation per position, clamped at 0 (tools/attribution.py layercam)

The tables of the tools are pinned (test.FAMILIES, explanation_table.FAMILIES, surrogate.FAMILIES, ablation.FAMILIES), so the four
rows live here: FAMILIES is the ablation tool's families plus these, the parser is that tool's plus their flags and options, and
both tools run on the extended table through their `rows=` / `families=` arguments.  Every flag and option of the four tools keeps
its name, default and meaning.

    --table_images 0 (the default)   the single-image tool: `--layerig true` / `--conductance true` / `--hirescam true` /
                                     `--layercam true` write layerig_{c}.png / conductance_{c}.png / hirescam_{c}.png /
                                     layercam_{c}.png of every class into --vis_dir, and --causal / --infidelity / --sensitivity
                                     print their lines for them
    --table_images N > 0             the explanation table over N validation images: one `table layerig:` / `table conductance:` /
                                     `table hirescam:` / `table layercam:` line each

layerig takes --layerig_steps (Gauss-Legendre steps) and --layerig_batch (path rows per head pass); conductance takes
--conductance_steps (steps of the path) and --conductance_batch (path images per feature pass, at least 2); hirescam and layercam
take no options.

    python -m scouter_amd.tools.layer --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --layerig true --conductance true --hirescam true --layercam true [--causal true] \
        [--table_images 64 --batch_size 16 --localization true]"""
import argparse

from .. import test as T
from ..train import _flag
from . import ablation as A
from . import explanation_table as E

_O = T.Option

LAYERS = (
    T.Family("layerig", "Layer Integrated Gradients heat map", maps="layerig_maps", explain="layer_integrated_gradients", options=(
        _O("steps", "n_steps", int, 50, "Gauss-Legendre steps"),
        _O("batch", "batch", int, 256, "path rows per head pass"))),
    T.Family("conductance", "Layer Conductance heat map", maps="conductance_maps", explain="layer_conductance", options=(
        _O("steps", "n_steps", int, 50, "steps of the path"),
        _O("batch", "batch", int, 50, "path images per feature pass (at least 2)"))),
    T.Family("hirescam", "HiResCAM heat map", maps="hirescam_maps", explain="hirescam"),
    T.Family("layercam", "LayerCAM heat map", maps="layercam_maps", explain="layercam"),
)
FAMILIES = A.FAMILIES + LAYERS
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_layer_parser():
    """the ablation tool's parser (which holds the surrogate tool's, the table tool's and the single-image tool's) plus the flag
    and the options of the four rows; --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("Layer IG, layer conductance, HiResCAM and LayerCAM: one image, or a table over a validation set",
                                     parents=[A.get_ablation_parser()], add_help=False)
    for row in LAYERS:
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
    args = get_layer_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
