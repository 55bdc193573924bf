"""Single-image inference + slot attention maps -- the `--vis` path of the reference (test.py:18-122 together with
sloter/utils/slot_attention.py:68-85): eval-mode forward of ONE image on the HIP path, per-class uint8 attention
maps written as `<out>/slot_{c}.png`, the input as `<out>/image.png`, and (optionally) the attention-area ratio the
reference prints with --cal_area_size (test.py:40-44).  The jet-colormap overlay of test.py:33-38 is matplotlib
post-processing of these PNGs and is not reproduced.

Every other explanation family is one row of FAMILIES below and follows one pattern: `--<name> true` draws the family's map of
every class for the image with tools/attribution.py, under the options `--<name>_<option>` of its row, and writes the uint8
maps as `<out>/<name>_{c}.png` at the input resolution, floored at --grad_min_level and BatchNorm-folded under --eval_fold.

    slot         the xSlot attention itself (--use_slot true; no flag)
    grad         d log-probability / d image (the reference's train.py --grad / --grad_min_level, captum_vis.py; also for the
                 --use_slot false baseline, the model the reference attributes)
    cam          Grad-CAM at the last backbone stage (captum's LayerGradCam on layer4)
    rise         RISE: random masks through the model (torchray's rise of the reference's torchcam_vis.py)
    scorecam     Score-CAM: one eval forward per channel of the last backbone stage (the gradient-free CAMs of torchcam_vis.py)
    ig           Integrated Gradients: zero baseline, Gauss-Legendre steps (captum's IntegratedGradients of captum_vis.py)
    smoothgrad   SmoothGrad: the mean gradient over noisy copies (captum's NoiseTunnel)
    campp        Grad-CAM++ (torchcam's GradCAMpp of torchcam_vis.py)
    smoothcampp  Smooth Grad-CAM++ (torchcam's SmoothGradCAMpp)
    extremal     Extremal Perturbation: SGD on a smooth mask of a fixed area (torchray's extremal_perturbation)
    iba          information bottleneck at the backbone's output, its feature distribution fitted on --iba_fit images of the
                 validation loader -- synthetic ones under --synthetic_data true (the IBA of torchcam_vis.py)
    igos         I-GOS: a coarse mask moved along integrated gradients (the Integrated_Mask torchcam_vis.py runs first)
    sscam        SS-CAM: Score-CAM over noisy copies of every mask (torchcam's SSCAM)
    iscam        IS-CAM: Score-CAM with every mask at scales along a ramp (torchcam's ISCAM, the ISSCAM torchcam_vis.py lists)

The three scores are the rows of SCORES; each scores the predicted class's explanation of every family drawn in the call, in
the order above.  `--causal true` prints the deletion and insertion scores (tools/attribution.py causal_metrics on the float
maps; the DAUC / IAUC the paper compares explanations with) as `causal <family> class <c>: deletion <d> insertion <i>`;
`--infidelity true` the infidelity (tools/attribution.py infidelity; grad, ig and smoothgrad with their full attribution, the
others with their map) as `infidelity <family> class <c>: raw <r> normalized <n> beta <b>`; `--sensitivity true` the
max-sensitivity (tools/attribution.py sensitivity_max) as `sensitivity <family> class <c>: max <s>` -- the infidelity and
sensitivity columns of the paper, after Yeh et al. 2019.  `--help` lists every option with its default.

    python -m scouter_amd.test --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --vis true --pre_trained false \
        [--checkpoint saved_model/ImageNet_use_slot_checkpoint.pth] [--image some.jpg] --img_size 224 \
        [--grad true --grad_min_level 0.1] [--cam true] [--rise true --rise_masks 4000 --rise_batch 250] \
        [--causal true --causal_step 224] [--infidelity true] [--sensitivity true]"""
import argparse
import collections
import functools
import os

import numpy as np
import torch

from .sloter.slot_model import SlotModel
from .train import _flag, checkpoint_name, get_args_parser


# ------------------------------------------------------------------------------------------------ the table
# One option of a row: `--<row>_<suffix>` of the parser, read with `type` and `default`, handed to the row's library function
# as `keyword` (None: to nothing; the tool reads it itself) after `convert` (None: as it is).
Option = collections.namedtuple("Option", "suffix keyword type default help choices convert", defaults=(None, None))

# One explanation family.  `name` is the flag `--<name>`, the PNG stem and the word of the score lines; `what` the phrase of the
# flag's help.  `maps` and `explain` name functions of tools/attribution.py:
#   explain(model, images, classes=, **options) -> the float explanation, maps [n, K, h, w];
#   maps(model, images, min_level=, **options) -> the uint8 maps [n, K, H, W].
# `reduce` marks the families whose explanation is a full attribution [n, K, C, H, W], the form --infidelity scores: it is the
# step from there to the float map, and `maps` then draws that attribution, maps(attribution, min_level=).  `estimate`: both
# functions also take estimate=iba_fit(args, model).  `flag` False: on by something else than a flag of this parser (main()).
Family = collections.namedtuple("Family", "name what options maps explain reduce estimate flag",
                                defaults=((), None, None, None, False, True))

# One score of the families drawn: the flag `--<name>`, the word that opens its printed lines, the options of its
# tools/attribution.py function.
Score = collections.namedtuple("Score", "name what options")


def _channel_mean(g):
    from . import kernels as K
    return K.channel_mean(g)


_O = Option
FAMILIES = (
    # (its PNGs are written by run(); its float map is the `slot_map` main() captures right after the predicting forward)
    Family("slot", "xSlot attention map", flag=False),
    # (--grad / --grad_min_level belong to train.py's parser; drawn on the host)
    Family("grad", "gradient attribution map", maps="attribution_maps", explain="input_gradients",
           reduce=lambda g: g.mean(dim=2), flag=False),
    Family("cam", "Grad-CAM heat map", maps="gradcam_maps", explain="gradcam"),
    Family("rise", "RISE saliency map", maps="rise_maps", explain="rise", options=(
        _O("masks", "n_masks", int, 4000, "number of random masks"),
        _O("batch", "batch", int, 250, "masked images per forward"))),
    Family("scorecam", "Score-CAM heat map", maps="scorecam_maps", explain="scorecam", options=(
        _O("batch", "batch", int, 250, "masked images per forward"),)),
    Family("ig", "Integrated Gradients map", maps="gradient_maps", explain="integrated_gradients", reduce=_channel_mean, options=(
        _O("steps", "n_steps", int, 50, "Gauss-Legendre steps"),
        _O("batch", "batch", int, 50, "path images per forward and backward"))),
    Family("smoothgrad", "SmoothGrad map", maps="gradient_maps", explain="smoothgrad", reduce=_channel_mean, options=(
        _O("samples", "n_samples", int, 50, "noisy copies per class"),
        _O("sigma", "sigma", float, 1.0, "standard deviation of the noise"),
        _O("batch", "batch", int, 50, "noisy copies per forward and backward"))),
    Family("campp", "Grad-CAM++ heat map", maps="gradcampp_maps", explain="gradcampp"),
    Family("smoothcampp", "Smooth Grad-CAM++ heat map", maps="smooth_gradcampp_maps", explain="smooth_gradcampp", options=(
        _O("samples", "n_samples", int, 4, "noisy copies per class"),
        _O("sigma", "sigma", float, 0.3, "standard deviation of the noise"),
        _O("batch", "batch", int, 4, "noisy copies per feature pass"))),
    Family("extremal", "Extremal Perturbation map", maps="extremal_maps", explain="extremal_saliency", options=(
        _O("area", "areas", float, 0.1, "fraction of the image the mask covers", convert=lambda a: (a,)),
        _O("iters", "n_iters", int, 800, "SGD steps"),
        _O("variant", "variant", str, "preserve", "keep (preserve) or remove (delete) the evidence under the mask",
           choices=("preserve", "delete")),
        _O("batch", "batch", int, 50, "masks per forward and backward"))),
    Family("iba", "information-bottleneck map", maps="iba_maps", explain="information_bottleneck", estimate=True, options=(
        _O("beta", "beta", float, 10.0, "weight of the information term"),
        _O("steps", "steps", int, 10, "Adam steps"),
        _O("samples_per_step", "samples", int, 10, "noisy samples per class and step"),
        _O("sigma", "sigma", float, 1.0, "standard deviation of the smoothing window (0: none)",
           convert=lambda s: s if s > 0.0 else None),
        _O("fit", None, int, 5000, "images the feature distribution is fitted on"),
        _O("batch", "batch", int, 0, "head rows per pass (0: all classes at once)", convert=lambda b: b or None))),
    Family("igos", "I-GOS map", maps="igos_maps", explain="igos_saliency", options=(
        _O("size", "size", int, 8, "cells a side of the mask"),
        _O("iters", "n_iters", int, 15, "iterations"),
        _O("steps", "n_steps", int, 20, "noisy path images per class and iteration"),
        _O("l1", "l1_coeff", float, 1.0, "weight of the L1 term"),
        _O("tv", "tv_coeff", float, 20.0, "weight of the total-variation term"),
        _O("batch", "batch", int, 50, "images per forward (and backward)"))),
    Family("sscam", "SS-CAM heat map", maps="sscam_maps", explain="sscam", options=(
        _O("samples", "n_samples", int, 35, "noisy copies of every channel's mask"),
        _O("sigma", "sigma", float, 2.0, "standard deviation of the noise"),
        _O("batch", "batch", int, 250, "masked images per forward"))),
    Family("iscam", "IS-CAM heat map", maps="iscam_maps", explain="iscam", options=(
        _O("samples", "n_samples", int, 10, "scales of every channel's mask"),
        _O("batch", "batch", int, 250, "masked images per forward"))),
)
SCORES = (
    Score("causal", "deletion / insertion scores of the predicted class's map", (
        _O("step", "step", int, 0, "pixels changed per point (0: --img_size)", convert=lambda s: s or None),)),
    Score("infidelity", "infidelity of the predicted class's explanation", (
        _O("samples", "n_samples", int, 50, "noisy copies"),
        _O("sigma", "sigma", float, 0.003, "standard deviation of the noise"),
        _O("batch", "batch", int, 50, "rows per forward, the clean image included"))),
    Score("sensitivity", "max-sensitivity of the predicted class's map", (
        _O("samples", "n_samples", int, 10, "perturbed copies"),
        _O("radius", "radius", float, 0.02, "half-width of the box"),
        _O("batch", "batch", int, 11, "rows per call of the explanation method, the clean image included"))),
)
_ROWS = {row.name: row for row in FAMILIES + SCORES}


def _row(name, rows=_ROWS):
    """the row `name` of the table `rows` {name: row}: this tool's own, or one that extends it (tools/explanation_table.py)"""
    if name not in rows:
        raise ValueError("unknown explanation family or score %r (known: %s)" % (name, ", ".join(rows)))
    return rows[name]


def _options(args, name, rows=_ROWS):
    """{suffix: value} of every option of the row `name`, read from `args` and converted; a namespace without an option (the
    tests build such) gets the table's default"""
    values = {}
    for o in _row(name, rows).options:
        v = o.type(getattr(args, "%s_%s" % (name, o.suffix), o.default))
        values[o.suffix] = o.convert(v) if o.convert else v
    return values


def option_kwargs(args, name, rows=_ROWS):
    """the keyword arguments the options of the row `name` give its library functions"""
    values = _options(args, name, rows)
    return {o.keyword: values[o.suffix] for o in _row(name, rows).options if o.keyword}


_igos_kwargs = functools.partial(option_kwargs, name="igos")           # (tests/test_igos_cpu.py reads the keywords by this name)


# ------------------------------------------------------------------------------------------------ the image and the prediction
def load_image(path, size, channels):
    """RGB (or grey) image -> normalised float tensor [c, size, size] (dataset/transform_func.py:101-124: resize to
    img_size, ToTensor, ImageNet mean/std)."""
    from PIL import Image
    img = Image.open(path).convert("L" if channels == 1 else "RGB").resize((size, size), Image.BILINEAR)
    a = np.asarray(img, dtype=np.float32) / 255.0
    if channels == 1:
        a = (a[None] - 0.1307) / 0.3081
    else:
        a = (a.transpose(2, 0, 1) - np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]) / \
            np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
    return img, torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@torch.no_grad()
def run(args, model, image, out_dir, label=None):
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    model.eval()
    output = model(image.unsqueeze(0).to(args.device, dtype=torch.float32))
    pred = int(output.argmax(dim=1))
    # [C, h, w] uint8, min-max scaled over the whole map (:74); the FC baseline (--use_slot false) has no slot maps
    maps = model.slot.vis_maps() if model.use_slot else np.zeros((0, 0, 0), dtype=np.uint8)
    for c, m in enumerate(maps):
        Image.fromarray(m, mode="L").save(os.path.join(out_dir, "slot_%d.png" % c))
    ratio = None
    if label is not None and len(maps):
        idx = label if args.loss_status > 0 else min(label + 1, len(maps) - 1)
        ratio = float(maps[idx].astype(np.float64).sum()) / float(maps[idx].size * 255)
    return output[0].cpu(), pred, maps, ratio


# ------------------------------------------------------------------------------------------------ the families
def iba_fit(args, model):
    """the feature distribution --iba needs (tools/attribution.py iba_estimate), fitted once per run on --iba_fit images of the
    validation loader -- seeded synthetic images under --synthetic_data true -- and kept on `args`"""
    est = getattr(args, "_iba_estimate", None)
    if est is None:
        from .tools.attribution import iba_estimate
        from .train import _build_loaders
        args.distributed = bool(getattr(args, "distributed", False))
        _, loader, _ = _build_loaders(args)
        transform = getattr(loader, "gpu_transform", None)

        def batches():
            for batch in loader:
                images = batch["image"]
                raw = not torch.is_tensor(images)
                yield transform(images, args.device) if raw else images.to(args.device, dtype=torch.float32)

        est = args._iba_estimate = iba_estimate(model, batches(), n_samples=_options(args, "iba")["fit"])
    return est


def _call(args, model, x, family, function, **kwargs):
    """function(model, x, **kwargs) of tools/attribution.py under the options of the row `family` (its own: read from the row)"""
    from .tools import attribution
    kwargs.update(option_kwargs(args, family.name, {family.name: family}))
    if family.estimate:
        kwargs["estimate"] = iba_fit(args, model)
    return getattr(attribution, function)(model, x, **kwargs)


def run_family(args, model, image, out_dir, name, rows=_ROWS):
    """`--<name> true`: the maps of every class of the family `name` for the one image -> `<out>/<name>_{c}.png`, uint8 maps at
    the input resolution, floored at --grad_min_level; returns them [C, H, W] (host).  run_grad, run_cam, ... below are this
    function for one name each.  rows: the table the name is looked up in -- this tool's own, or one that extends it."""
    from PIL import Image
    from .tools import attribution
    family = _row(name, rows)
    os.makedirs(out_dir, exist_ok=True)
    x, min_level = image.unsqueeze(0).to(args.device, dtype=torch.float32), float(args.grad_min_level)
    if family.reduce is None:
        maps = _call(args, model, x, family, family.maps, min_level=min_level)[0]
    else:
        maps = getattr(attribution, family.maps)(_call(args, model, x, family, family.explain), min_level=min_level)[0]
    if torch.is_tensor(maps):                                             # (attribution_maps has drawn on the host already)
        maps = maps.cpu().numpy()
    for c, m in enumerate(maps):
        Image.fromarray(m, mode="L").save(os.path.join(out_dir, "%s_%d.png" % (name, c)))
    return maps


# run_<name>(args, model, image, out_dir) of every family the tool draws: run_grad, run_cam, run_rise, ... in table order
globals().update({"run_" + f.name: functools.partial(run_family, name=f.name) for f in FAMILIES if f.maps})


def _family_attribution(args, model, x, pred, family, slot_map=None, full=False, rows=_ROWS):
    """the predicted class's FLOAT explanation of one family for the images x [n, C, H, W] on the device -> [n, 1, h, w]: the
    row's `explain`, brought to a map by its `reduce`; for the row without one (slot) the given `slot_map`, taken right after
    the forward that predicted.  full: the families with a `reduce` keep their attribution [n, 1, C, H, W] instead."""
    row = _row(family, rows)
    if row.explain is None:
        return slot_map
    g = _call(args, model, x, row, row.explain, classes=[pred])
    return g if full or row.reduce is None else row.reduce(g)


# ------------------------------------------------------------------------------------------------ the scores
def run_causal(args, model, image, pred, families, slot_map=None, rows=_ROWS):
    """--causal true: the deletion / insertion scores (tools/attribution.py causal_metrics: --causal_step pixels per point, 0 =
    one image row) of the predicted class's FLOAT map (_family_attribution) of every family in `families`, one printed line
    each; returns {family: (deletion, insertion)}."""
    from .tools.attribution import causal_metrics
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)
    # (the forward batch of the metric is --rise_batch whatever the family: the flag it had when RISE was the one family scored)
    kwargs = dict(option_kwargs(args, "causal"), batch=option_kwargs(args, "rise")["batch"])
    scores = {}
    for family in families:
        maps = _family_attribution(args, model, x, pred, family, slot_map, rows=rows)
        r = causal_metrics(model, x, maps, classes=[pred], **kwargs)
        scores[family] = (float(r.deletion[0, 0]), float(r.insertion[0, 0]))
        print("causal %s class %d: deletion %.6f insertion %.6f" % ((family, pred) + scores[family]))
    return scores


def run_infidelity(args, model, image, pred, families, slot_map=None, rows=_ROWS):
    """--infidelity true: the infidelity (tools/attribution.py infidelity: --infidelity_samples noisy copies at --infidelity_sigma,
    --infidelity_batch rows per forward) of the predicted class's explanation of every family in `families` -- grad, ig and
    smoothgrad with their full [C, H, W] attribution, the other families with their map, which counts for every channel -- one
    printed line each; returns {family: (raw, normalized, beta)}."""
    from .tools.attribution import infidelity
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)
    kwargs = option_kwargs(args, "infidelity")
    scores = {}
    for family in families:
        attr = _family_attribution(args, model, x, pred, family, slot_map, full=True, rows=rows)
        r = infidelity(model, x, attr, classes=[pred], **kwargs)
        scores[family] = (float(r.raw[0, 0]), float(r.normalized[0, 0]), float(r.beta[0, 0]))
        print("infidelity %s class %d: raw %.6e normalized %.6e beta %.6e" % ((family, pred) + scores[family]))
    return scores


def run_sensitivity(args, model, image, pred, families, rows=_ROWS):
    """--sensitivity true: the max-sensitivity (tools/attribution.py sensitivity_max: --sensitivity_samples points of the box of
    half-width --sensitivity_radius, --sensitivity_batch rows per call) of the predicted class's FLOAT map of every family in
    `families`, each family explaining the perturbed images as it explained the image (slot: an eval forward, then
    slot_saliency), one printed line each; returns {family: score}."""
    from .tools.attribution import _eval_mode, sensitivity_max, slot_saliency
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)
    kwargs = option_kwargs(args, "sensitivity")

    def slot_maps(images):
        with _eval_mode(model), torch.no_grad():
            model(images)
        return slot_saliency(model)[:, pred:pred + 1].contiguous()

    scores = {}
    for family in families:
        explain = slot_maps if _row(family, rows).explain is None else \
            functools.partial(_family_attribution, args, model, pred=pred, family=family, rows=rows)
        r = sensitivity_max(explain, x, **kwargs)
        scores[family] = float(r.score[0, 0])
        print("sensitivity %s class %d: max %.6e" % (family, pred, scores[family]))
    return scores


# ------------------------------------------------------------------------------------------------ the command line
def get_test_parser():
    """the training tool's arguments plus this tool's own: a flag and the options of every row of FAMILIES and SCORES"""
    parser = argparse.ArgumentParser("single-image xSlot inference", parents=[get_args_parser()])
    parser.add_argument("--checkpoint", default="", help="checkpoint written by train.py (default: the standard name "
                                                         "under --output_dir, if it exists)")
    parser.add_argument("--image", default="", help="image file; a seeded synthetic image is used when empty")
    parser.add_argument("--label", default=None, type=int)
    parser.add_argument("--vis_dir", default="sloter/vis")
    for row in FAMILIES + SCORES:
        if isinstance(row, Score):
            parser.add_argument("--" + row.name, default=False, type=_flag, help="true: print the %s of every family drawn" % row.what)
        elif row.flag:
            parser.add_argument("--" + row.name, default=False, type=_flag,
                                help="true: write the %s of every class as %s_{c}.png into --vis_dir" % (row.what, row.name))
        for o in row.options:
            parser.add_argument("--%s_%s" % (row.name, o.suffix), default=o.default, type=o.type, choices=o.choices,
                                help="--%s: %s (default: %s)" % (row.name, o.help, o.default))
    return parser


def build_model(args):
    """the model of a parsed command line on --device, folded under --eval_fold, with --checkpoint (or the standard name under
    --output_dir) loaded where it exists -> (model, whether --grad was given); shared with tools/explanation_table.py"""
    for name, typ in (("num_classes", int), ("lambda_value", float), ("power", int), ("slots_per_class", int)):
        setattr(args, name, typ(getattr(args, name)))
    args.vis, args.vis_id = False, 0                  # maps are taken from model.slot.last_attn, image index 0
    # (--grad asks THIS tool for gradient maps; the model is built as for training, so that its checkpoints load)
    want_grad, args.grad = bool(args.grad), False
    model = SlotModel(args).to(args.device)
    model.set_inference_fold(bool(args.eval_fold))
    ckpt = args.checkpoint or os.path.join(args.output_dir, checkpoint_name(args))
    if os.path.exists(ckpt):
        model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=False)["model"], strict=True)
        print("load", ckpt)
    else:
        print("no checkpoint found (%s): random weights" % ckpt)
    return model, want_grad


def single_image(args, families=FAMILIES, rows=_ROWS):
    """what main() does with a parsed command line; families / rows: this tool's table, or one that extends it
    (tools/surrogate.py)"""
    model, want_grad = build_model(args)
    channels, size = (1 if args.dataset == "MNIST" else 3), int(args.img_size)
    if args.image:
        raw, image = load_image(args.image, size, channels)
        os.makedirs(args.vis_dir, exist_ok=True)
        raw.save(os.path.join(args.vis_dir, "image.png"))
    else:
        image = torch.from_numpy(np.random.default_rng(0).standard_normal((channels, size, size), dtype=np.float32))
    out, pred, maps, ratio = run(args, model, image, args.vis_dir, args.label)
    slot_map = None
    if (args.causal or args.infidelity) and model.use_slot:
        from .tools.attribution import slot_saliency
        slot_map = slot_saliency(model)[:, pred:pred + 1].contiguous()       # (before another forward replaces last_attn)
    unflagged = {"slot": model.use_slot, "grad": want_grad}                  # the rows with `flag` False
    drawn = [f for f in families if (getattr(args, f.name) if f.flag else unflagged[f.name])]
    for f in drawn:
        if f.maps:
            run_family(args, model, image, args.vis_dir, f.name, rows)
    names = [f.name for f in drawn]
    if args.causal:
        run_causal(args, model, image, pred, names, slot_map, rows)
    if args.infidelity:
        run_infidelity(args, model, image, pred, names, slot_map, rows)
    if args.sensitivity:
        run_sensitivity(args, model, image, pred, names, rows)
    print(out)
    print(pred)
    if ratio is not None and args.cal_area_size:
        print(f"attention_ratio: {ratio}")


def main():
    single_image(get_test_parser().parse_args())


if __name__ == "__main__":
    main()
