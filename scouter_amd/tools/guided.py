"""Guided backpropagation, the deconvnet rule and Guided Grad-CAM as rows of the two explanation tools: the single-image tool
(scouter_amd/test.py) and the explanation table over a validation set (tools/explanation_table.py), both with three more families
on top of tools/foldgrad.py's.  The reference's captum_vis.py imports captum's GuidedGradCam; these are three of the oldest saliency
baselines, the natural comparison for the slot maps.

    guidedbp    guided backpropagation (Springenberg et al. 2015): every ReLU of the backbone passes what is positive in the
                gradient arriving at it and lies where its output was positive (tools/attribution.py guided_backprop)
    deconvnet   the deconvnet rule (Zeiler & Fergus 2014): every ReLU of the backbone passes the positive part of the gradient
                arriving at it, whatever its output was (tools/attribution.py deconvnet)
    guidedcam   Guided Grad-CAM (Selvaraju et al. 2017): guided backpropagation times the class map of the backbone's output
                brought to the image's size, --guidedcam_interpolate nearest (captum's default) | bilinear
                (tools/attribution.py guided_gradcam)

All three run on SlotModel.image_pass -- ONE forward on the BatchNorm-folded weights for every class, a gradient-only backward
per class in which the rule is a compile-time switch of the four kernels that apply a ReLU mask (fp32 models; there is no
autograd form) -- and are full attributions: --infidelity, --sensitivity and --causal score them as they score `ig`.

The tables of the tools are pinned (test.FAMILIES, explanation_table.FAMILIES, surrogate.FAMILIES, ablation.FAMILIES,
layer.FAMILIES, gradshap.FAMILIES, foldgrad.FAMILIES), so the rows live here: FAMILIES is the foldgrad tool's table plus these,
the parser is that tool's plus their flags and the one option, and both tools run on the extended table through their `rows=` /
`families=` arguments.  Every flag and option of the seven tools keeps its name, default and meaning.

    --table_images 0 (the default)   the single-image tool: `--guidedbp true` / `--deconvnet true` / `--guidedcam true` write
                                     guidedbp_{c}.png / deconvnet_{c}.png / guidedcam_{c}.png of every class into --vis_dir
    --table_images N > 0             the explanation table over N validation images: one `table guidedbp:` / `table deconvnet:` /
                                     `table guidedcam:` line each

    python -m scouter_amd.tools.guided --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --guidedbp true --guidedcam true [--deconvnet true] [--infidelity true] [--table_images 64 --batch_size 16]"""
import argparse

from .. import test as T
from ..train import _flag
from . import explanation_table as E
from . import foldgrad as FG

_O = T.Option

GUIDED = (
    T.Family("guidedbp", "guided backpropagation map", maps="gradient_maps", explain="guided_backprop", reduce=T._channel_mean),
    T.Family("deconvnet", "deconvnet map", maps="gradient_maps", explain="deconvnet", reduce=T._channel_mean),
    T.Family("guidedcam", "Guided Grad-CAM map", maps="gradient_maps", explain="guided_gradcam", reduce=T._channel_mean, options=(
        _O("interpolate", "interpolate", str, "nearest", "how the class map is brought to the image's size",
           ("nearest", "bilinear")),)),
)
FAMILIES = FG.FAMILIES + GUIDED
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_guided_parser():
    """the foldgrad tool's parser (which holds the parsers of the six tools under it) plus the flags of the three rows and the
    one option; --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("guided backpropagation, deconvnet and Guided Grad-CAM on the BatchNorm-folded gradient-only "
                                     "pass: one image, or a table over a validation set", parents=[FG.get_foldgrad_parser()],
                                     add_help=False)
    for row in GUIDED:
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
    args = get_guided_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
