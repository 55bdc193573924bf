"""GradientSHAP (expected gradients) as rows of the two explanation tools: the single-image tool (scouter_amd/test.py) and the
explanation table over a validation set (tools/explanation_table.py), both with two more families on top of tools/layer.py's.
The reference's captum_vis.py imports captum's GradientShap first; these are the only gradient rows that explain against a
DISTRIBUTION of baselines instead of one black image.

    gradshap       GradientSHAP at the image: every sample walks from its own randomly drawn baseline of a Gaussian bank by its
                   own random fraction, optionally from a noisy copy of the image; the mean of gradient times that sample's own
                   difference (tools/attribution.py gradient_shap).  A full attribution: --infidelity scores it as it does `ig`.
    layergradshap  the same at the backbone's output, the line in FEATURE space from the features of the drawn baseline to the
                   image's, through the head alone (tools/attribution.py layer_gradient_shap)

The tables of the tools are pinned (test.FAMILIES, explanation_table.FAMILIES, surrogate.FAMILIES, ablation.FAMILIES,
layer.FAMILIES), so the two rows live here: FAMILIES is the layer tool's families plus these, the parser is that tool's plus their
flags and options, and both tools run on the extended table through their `rows=` / `families=` arguments.  Every flag and option
of the five tools keeps its name, default and meaning.

    --table_images 0 (the default)   the single-image tool: `--gradshap true` / `--layergradshap true` write gradshap_{c}.png /
                                     layergradshap_{c}.png of every class into --vis_dir, and --causal / --infidelity /
                                     --sensitivity print their lines for them
    --table_images N > 0             the explanation table over N validation images: one `table gradshap:` /
                                     `table layergradshap:` line each

gradshap takes --gradshap_samples, --gradshap_baselines (the size of the Gaussian bank), --gradshap_bank_sigma (its standard
deviation in normalised image space), --gradshap_sigma (the noise added to the image), --gradshap_batch and --gradshap_seed;
layergradshap the same without the image noise.

    python -m scouter_amd.tools.gradshap --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --gradshap true --layergradshap true [--infidelity true] [--table_images 64 --batch_size 16 --localization true]"""
import argparse

from .. import test as T
from ..train import _flag
from . import explanation_table as E
from . import layer as L

_O = T.Option

SHAPS = (
    T.Family("gradshap", "GradientSHAP map", maps="gradient_maps", explain="gradient_shap", reduce=T._channel_mean, options=(
        _O("samples", "n_samples", int, 50, "samples (baseline, fraction and noise drawn per sample)"),
        _O("baselines", "baselines", int, 10, "baselines in the Gaussian bank"),
        _O("bank_sigma", "bank_sigma", float, 1.0, "standard deviation of the bank's baselines"),
        _O("sigma", "sigma", float, 0.0, "standard deviation of the noise added to the image"),
        _O("batch", "batch", int, 50, "samples per forward and backward"),
        _O("seed", "seed", int, 0, "seed of the draws, the bank and the noise"))),
    T.Family("layergradshap", "Layer GradientSHAP heat map", maps="layergradshap_maps", explain="layer_gradient_shap", options=(
        _O("samples", "n_samples", int, 200, "samples (baseline and fraction drawn per sample)"),
        _O("baselines", "baselines", int, 10, "baselines in the Gaussian bank"),
        _O("bank_sigma", "bank_sigma", float, 1.0, "standard deviation of the bank's baseline images"),
        _O("batch", "batch", int, 256, "samples per head pass"),
        _O("seed", "seed", int, 0, "seed of the draws and the bank"))),
)
FAMILIES = L.FAMILIES + SHAPS
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_gradshap_parser():
    """the layer tool's parser (which holds the ablation tool's, the surrogate tool's, the table tool's and the single-image
    tool's) plus the flag and the options of the two rows; --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("GradientSHAP at the image and at the backbone's output: one image, or a table over a "
                                     "validation set", parents=[L.get_layer_parser()], add_help=False)
    for row in SHAPS:
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
    args = get_gradshap_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
