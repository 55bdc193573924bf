"""The image-space gradient rows of the two explanation tools on the BatchNorm-folded gradient-only pass: the single-image tool
(scouter_amd/test.py) and the explanation table over a validation set (tools/explanation_table.py), both on the GradientSHAP
tool's table (tools/gradshap.py) with four rows replaced by copies that carry one more option.

    grad        --grad_route        autograd | folded     tools/attribution.py input_gradients(route=)
    ig          --ig_route          autograd | folded     integrated_gradients_by_route(route=)
    smoothgrad  --smoothgrad_route  autograd | folded     smoothgrad_by_route(route=)
    gradshap    --gradshap_route    autograd | folded     gradient_shap(route=)

`autograd` (the default of all four) is what every other tool runs: the unfolded eval forward and the training backward walked
on to the image, once per class.  `folded` is SlotModel.image_pass: one forward on the folded weights per batch of rows, serving
every class, and a backward that computes input gradients only -- no BatchNorm kernel, no parameter gradient of the backbone
(fp32 models; it does not need --eval_fold).  The two routes agree to rounding, not bit for bit.

The tables of the tools are pinned (test.FAMILIES, explanation_table.FAMILIES, surrogate.FAMILIES, ablation.FAMILIES,
layer.FAMILIES, gradshap.FAMILIES), so the copies live here: FAMILIES is the GradientSHAP tool's table with the four rows
replaced, the parser is that tool's plus the four options, and both tools run on the table through their `rows=` / `families=`
arguments.  Every flag and option of the six tools keeps its name, default and meaning; --infidelity and --sensitivity score
the rows under the route they were drawn with.

    --table_images 0 (the default)   the single-image tool
    --table_images N > 0             the explanation table over N validation images

    python -m scouter_amd.tools.foldgrad --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 \
        --ig true --ig_route folded [--grad true --grad_route folded] [--infidelity true] [--table_images 64 --batch_size 16]"""
import argparse

from .. import test as T
from . import explanation_table as E
from . import gradshap as G

ROUTED = ("grad", "ig", "smoothgrad", "gradshap")
_ROUTE = T.Option("route", "route", str, "autograd",
                  "autograd: the unfolded forward and the training backward per class; folded: one BatchNorm-folded forward for "
                  "every class and a gradient-only backward (SlotModel.image_pass)", ("autograd", "folded"))

# (integrated_gradients and smoothgrad keep the parameter lists their callers know: the option is taken by their *_by_route forms)
_BY_ROUTE = {"ig": "integrated_gradients_by_route", "smoothgrad": "smoothgrad_by_route"}
FAMILIES = tuple(f._replace(options=tuple(f.options) + (_ROUTE,), explain=_BY_ROUTE.get(f.name, f.explain)) if f.name in ROUTED else f
                 for f in G.FAMILIES)
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}


def get_foldgrad_parser():
    """the GradientSHAP tool's parser (which holds the parsers of the five tools under it) plus the four route options;
    --table_images defaults to 0, the single-image mode"""
    parser = argparse.ArgumentParser("image-space gradient explanations on the BatchNorm-folded gradient-only pass: one image, "
                                     "or a table over a validation set", parents=[G.get_gradshap_parser()], add_help=False)
    for name in ROUTED:
        o = _ROUTE
        parser.add_argument("--%s_%s" % (name, o.suffix), default=o.default, type=o.type, choices=o.choices,
                            help="--%s: %s (default: %s)" % (name, o.help, o.default))
    parser.set_defaults(table_images=0)
    return parser


def option_kwargs(args, name):
    """the keyword arguments the options of the row `name` of this tool's table give its library functions"""
    return T.option_kwargs(args, name, _ROWS)


def main():
    args = get_foldgrad_parser().parse_args()
    if args.table_images < 0:
        raise ValueError("--table_images must be at least 0, got %d" % args.table_images)
    if args.table_images > 0:
        return E.run_table(args, FAMILIES, _ROWS)
    return T.single_image(args, FAMILIES, _ROWS)


if __name__ == "__main__":
    main()
