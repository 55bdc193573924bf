"""LIME and KernelSHAP as rows of the two explanation tools: the single-image tool (scouter_amd/test.py) and the explanation
table over a validation set (tools/explanation_table.py), both with two more families.

    lime         LIME: a ridge regression of the class probability over superpixels (tools/attribution.py lime)
    shap         KernelSHAP: Shapley values of the superpixels by weighted regression (tools/attribution.py kernelshap)

The tables of those two tools are pinned (test.FAMILIES, explanation_table.FAMILIES), so the two rows live here: FAMILIES is the
explanation table's families plus these, the parser is that tool's plus their flags and options, and both tools run on the
extended table through their `rows=` / `families=` arguments.  Every flag and option of the two tools keeps its name, default and
meaning.

    --table_images 0 (the default)   the single-image tool: `--lime true` / `--shap true` write lime_{c}.png / shap_{c}.png of every
                                     class into --vis_dir, and --causal / --infidelity / --sensitivity print their lines for them
    --table_images N > 0             the explanation table over N validation images: one `table lime:` / `table shap:` line each

Both rows take --<row>_samples (perturbed copies per image), --<row>_batch (copies per forward), --<row>_segments (g: a g x g grid
of superpixels), --<row>_slic_iters, --<row>_compactness and --<row>_ridge; lime also --lime_kernel_width, shap also --shap_hide
(the constant that fills a hidden superpixel; lime fills with the superpixel's mean colour).

    python -m scouter_amd.tools.surrogate --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --lime true --shap true [--causal true] [--table_images 64 --batch_size 16 --localization true]"""
import argparse

from .. import test as T
from ..train import _flag
from . import explanation_table as E

_O = T.Option


def _shared_options(ridge):
    return (_O("samples", "n_samples", int, 1000, "perturbed copies per image"),
            _O("batch", "batch", int, 250, "perturbed copies per forward"),
            _O("segments", "segments", int, 8, "superpixels a side: a g x g grid, g * g <= 128"),
            _O("slic_iters", "slic_iters", int, 10, "iterations of the superpixel loop (0: the plain grid)"),
            _O("compactness", "compactness", float, 1.0, "weight of the distance term of the superpixel loop"),
            _O("ridge", "ridge", float, ridge, "ridge penalty on the coefficients"))


SURROGATES = (
    T.Family("lime", "LIME map", maps="lime_maps", explain="lime", options=_shared_options(1.0) + (
        _O("kernel_width", "kernel_width", float, 0.25, "width of the exponential kernel on the distance to the image"),)),
    T.Family("shap", "KernelSHAP map", maps="kernelshap_maps", explain="kernelshap", options=_shared_options(0.0) + (
        _O("hide", "hide", float, 0.0, "the constant that fills a hidden superpixel"),)),
)
FAMILIES = E.FAMILIES + SURROGATES
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_surrogate_parser():
    """the explanation table's parser (which holds the single-image tool's) plus the flag and the options of the two rows;
    --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("LIME and KernelSHAP: one image, or a table over a validation set",
                                     parents=[E.get_table_parser()], add_help=False)
    for row in SURROGATES:
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
    args = get_surrogate_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
