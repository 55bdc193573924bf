"""Single-image inference + slot attention maps -- the `--vis` path of the reference (test.py:18-122 together with
sloter/utils/slot_attention.py:68-85): eval-mode forward of ONE image on the HIP path, per-class uint8 attention
maps written as `<out>/slot_{c}.png`, the input as `<out>/image.png`, and (optionally) the attention-area ratio the
reference prints with --cal_area_size (test.py:40-44).  `--grad true` adds the per-class gradient attribution maps
`<out>/grad_{c}.png` (d log-probability / d image through tools/attribution.py, floored at --grad_min_level; also for the
`--use_slot false` baseline, the model the reference attributes); `--cam true` the per-class Grad-CAM heat maps at the last
backbone stage, `<out>/cam_{c}.png` (tools/attribution.py gradcam_maps: one backbone forward, floored at --grad_min_level,
BatchNorm-folded under --eval_fold; what the reference draws with captum's LayerGradCam on layer4); `--rise true` the per-class
RISE perturbation maps `<out>/rise_{c}.png` (tools/attribution.py rise_maps: --rise_masks random masks through the model in
chunks of --rise_batch, floored at --grad_min_level, BatchNorm-folded under --eval_fold; what the reference's torchcam_vis.py
draws with torchray's rise); `--scorecam true` the per-class Score-CAM heat maps `<out>/scorecam_{c}.png`
(tools/attribution.py scorecam_maps: one eval forward per channel of the last backbone stage, in chunks of --scorecam_batch,
floored at --grad_min_level, BatchNorm-folded under --eval_fold; the gradient-free CAM family of the reference's
torchcam_vis.py); `--ig true` the per-class Integrated Gradients maps `<out>/ig_{c}.png` (tools/attribution.py
integrated_gradients: --ig_steps Gauss-Legendre steps from a zero baseline in chunks of --ig_batch, drawn by gradient_maps,
floored at --grad_min_level; captum's IntegratedGradients of the reference's captum_vis.py); `--smoothgrad true` the per-class
SmoothGrad maps `<out>/smoothgrad_{c}.png` (tools/attribution.py smoothgrad: --smoothgrad_samples noisy copies at
--smoothgrad_sigma in chunks of --smoothgrad_batch; captum's NoiseTunnel); `--campp true` the per-class Grad-CAM++ heat maps
`<out>/campp_{c}.png` (tools/attribution.py gradcampp_maps: one backbone forward, floored at --grad_min_level, BatchNorm-folded
under --eval_fold; torchcam's GradCAMpp of the reference's torchcam_vis.py); `--smoothcampp true` the per-class Smooth Grad-CAM++
heat maps `<out>/smoothcampp_{c}.png` (tools/attribution.py smooth_gradcampp: --smoothcampp_samples noisy copies at
--smoothcampp_sigma in chunks of --smoothcampp_batch; torchcam's SmoothGradCAMpp); `--extremal true` the per-class Extremal
Perturbation maps `<out>/extremal_{c}.png` (tools/attribution.py extremal_maps: --extremal_iters SGD steps on a smooth mask of
--extremal_area of the image, variant --extremal_variant, the classes in groups of --extremal_batch, floored at --grad_min_level;
torchray's extremal_perturbation of the reference's torchcam_vis.py); `--iba true` the per-class information-bottleneck maps
`<out>/iba_{c}.png` (tools/attribution.py iba_maps: --iba_steps Adam steps on a feature-space mask with --iba_samples_per_step noisy
samples each, information weight --iba_beta, window --iba_sigma, the feature distribution fitted on --iba_fit images of the
validation loader -- synthetic ones under --synthetic_data true --, at most --iba_batch head rows per pass, 0 = all; the IBA of
the reference's torchcam_vis.py); `--igos true` the per-class I-GOS maps `<out>/igos_{c}.png` (tools/attribution.py igos_maps:
--igos_iters iterations of --igos_steps noisy path images each on a mask of --igos_size x --igos_size cells, L1 weight --igos_l1,
total-variation weight --igos_tv, at most --igos_batch rows per pass, floored at --grad_min_level; the Integrated_Mask the
reference's torchcam_vis.py runs first); `--sscam true` the per-class SS-CAM heat maps `<out>/sscam_{c}.png` (tools/attribution.py
sscam_maps: --sscam_samples noisy copies of every channel's Score-CAM mask at --sscam_sigma, --sscam_batch masked images per
forward, floored at --grad_min_level, BatchNorm-folded under --eval_fold; torchcam's SSCAM of the reference's torchcam_vis.py);
`--iscam true` the per-class IS-CAM heat maps `<out>/iscam_{c}.png` (tools/attribution.py iscam_maps: every mask at
--iscam_samples scales along a ramp, --iscam_batch masked images per forward; torchcam's ISCAM, the ISSCAM that file lists);
`--causal true` prints, for every family of maps
drawn in the call (slot under --use_slot true, grad, cam, rise, scorecam, ig, smoothgrad, campp, smoothcampp, extremal, iba, igos, sscam, iscam), the deletion and insertion scores of
the predicted class's map (tools/attribution.py causal_metrics on the float maps, --causal_step pixels per point, 0 = one image row; the DAUC / IAUC the paper compares explanations with) as
`causal <family> class <c>: deletion <d> insertion <i>`; `--infidelity true` and `--sensitivity true` print, for the same families,
the infidelity of the predicted class's explanation (tools/attribution.py infidelity: --infidelity_samples noisy copies at
--infidelity_sigma, --infidelity_batch rows per forward; grad, ig and smoothgrad with their full attribution, the others with their
map) as `infidelity <family> class <c>: raw <r> normalized <n> beta <b>` and its max-sensitivity (tools/attribution.py
sensitivity_max: --sensitivity_samples points within --sensitivity_radius, --sensitivity_batch rows per call) as
`sensitivity <family> class <c>: max <s>` -- the infidelity and sensitivity columns of the paper, after Yeh et al. 2019.  The
jet-colormap overlay of test.py:33-38 is matplotlib post-processing of these PNGs and is not reproduced.

    python -m scouter_amd.test --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --vis true --pre_trained false \
        [--checkpoint saved_model/ImageNet_use_slot_checkpoint.pth] [--image some.jpg] --img_size 224 \
        [--grad true --grad_min_level 0.1] [--cam true] [--rise true --rise_masks 4000 --rise_batch 250] \
        [--scorecam true --scorecam_batch 250] [--ig true --ig_steps 50 --ig_batch 50] \
        [--smoothgrad true --smoothgrad_samples 50 --smoothgrad_sigma 1.0 --smoothgrad_batch 50] \
        [--campp true] [--smoothcampp true --smoothcampp_samples 4 --smoothcampp_sigma 0.3 --smoothcampp_batch 4] \
        [--extremal true --extremal_area 0.1 --extremal_iters 800 --extremal_variant preserve --extremal_batch 50] \
        [--iba true --iba_beta 10 --iba_steps 10 --iba_samples_per_step 10 --iba_sigma 1.0 --iba_fit 5000 --iba_batch 0] \
        [--igos true --igos_size 8 --igos_iters 15 --igos_steps 20 --igos_l1 1.0 --igos_tv 20.0 --igos_batch 50] \
        [--sscam true --sscam_samples 35 --sscam_sigma 2.0 --sscam_batch 250] \
        [--iscam true --iscam_samples 10 --iscam_batch 250] \
        [--causal true --causal_step 224] \
        [--infidelity true --infidelity_samples 50 --infidelity_sigma 0.003 --infidelity_batch 50] \
        [--sensitivity true --sensitivity_samples 10 --sensitivity_radius 0.02 --sensitivity_batch 11]"""
import argparse
import functools
import os

import numpy as np
import torch

from .sloter.slot_model import SlotModel
from .train import _flag, checkpoint_name, get_args_parser


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


def run_grad(args, model, image, out_dir):
    """--grad true: the gradient attribution of every class for the one image (reference train.py --grad /
    --grad_min_level, captum_vis.py) -> `<out>/grad_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from PIL import Image
    from .tools.attribution import attribution_maps, input_gradients
    os.makedirs(out_dir, exist_ok=True)
    grads = input_gradients(model, image.unsqueeze(0).to(args.device, dtype=torch.float32))
    maps = attribution_maps(grads, min_level=float(args.grad_min_level))[0]
    for c, m in enumerate(maps):
        Image.fromarray(m, mode="L").save(os.path.join(out_dir, "grad_%d.png" % c))
    return maps


def _run_maps(args, model, image, out_dir, stem, maps_fn):
    """one attribution family for the one image: maps_fn(images [1, C, H, W] on the device, min_level=) -> uint8 maps [1, C, H, W]
    on the device, saved as `<out>/<stem>_{c}.png`; returns them [C, H, W] (host)"""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    maps = maps_fn(image.unsqueeze(0).to(args.device, dtype=torch.float32), min_level=float(args.grad_min_level))[0].cpu().numpy()
    for c, m in enumerate(maps):
        Image.fromarray(m, mode="L").save(os.path.join(out_dir, "%s_%d.png" % (stem, c)))
    return maps


def run_cam(args, model, image, out_dir):
    """--cam true: the Grad-CAM heat map of every class for the one image at the backbone's output (reference captum_vis.py
    LayerGradCam on layer4) -> `<out>/cam_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import gradcam_maps
    return _run_maps(args, model, image, out_dir, "cam", functools.partial(gradcam_maps, model))


def run_rise(args, model, image, out_dir):
    """--rise true: the RISE saliency map of every class for the one image (reference torchcam_vis.py, torchray.attribution.rise)
    -> `<out>/rise_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import rise_maps
    return _run_maps(args, model, image, out_dir, "rise",
                     functools.partial(rise_maps, model, n_masks=int(getattr(args, "rise_masks", 4000)),
                                       batch=int(getattr(args, "rise_batch", 250))))


def run_scorecam(args, model, image, out_dir):
    """--scorecam true: the Score-CAM heat map of every class for the one image at the backbone's output (Wang et al. 2020; the
    gradient-free CAMs of the reference's torchcam_vis.py) -> `<out>/scorecam_{c}.png`, uint8 maps at the input resolution;
    returns them [C, H, W]."""
    from .tools.attribution import scorecam_maps
    return _run_maps(args, model, image, out_dir, "scorecam",
                     functools.partial(scorecam_maps, model, batch=int(getattr(args, "scorecam_batch", 250))))


def _sscam_kwargs(args):
    return dict(n_samples=int(getattr(args, "sscam_samples", 35)), sigma=float(getattr(args, "sscam_sigma", 2.0)),
                batch=int(getattr(args, "sscam_batch", 250)))


def _iscam_kwargs(args):
    return dict(n_samples=int(getattr(args, "iscam_samples", 10)), batch=int(getattr(args, "iscam_batch", 250)))


def run_sscam(args, model, image, out_dir):
    """--sscam true: the SS-CAM heat map of every class for the one image at the backbone's output (torchcam's SSCAM of the
    reference's torchcam_vis.py: --sscam_samples noisy copies of every channel's mask at --sscam_sigma, --sscam_batch masked
    images per forward) -> `<out>/sscam_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import sscam_maps
    return _run_maps(args, model, image, out_dir, "sscam", functools.partial(sscam_maps, model, **_sscam_kwargs(args)))


def run_iscam(args, model, image, out_dir):
    """--iscam true: the IS-CAM heat map of every class for the one image at the backbone's output (torchcam's ISCAM, the ISSCAM
    of the reference's torchcam_vis.py: every channel's mask at --iscam_samples scales along a ramp, --iscam_batch masked images
    per forward) -> `<out>/iscam_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import iscam_maps
    return _run_maps(args, model, image, out_dir, "iscam", functools.partial(iscam_maps, model, **_iscam_kwargs(args)))


def run_campp(args, model, image, out_dir):
    """--campp true: the Grad-CAM++ heat map of every class for the one image at the backbone's output (torchcam's GradCAMpp of
    the reference's torchcam_vis.py) -> `<out>/campp_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import gradcampp_maps
    return _run_maps(args, model, image, out_dir, "campp", functools.partial(gradcampp_maps, model))


def _smoothcampp_kwargs(args):
    return dict(n_samples=int(getattr(args, "smoothcampp_samples", 4)), sigma=float(getattr(args, "smoothcampp_sigma", 0.3)),
                batch=int(getattr(args, "smoothcampp_batch", 4)))


def run_smoothcampp(args, model, image, out_dir):
    """--smoothcampp true: the Smooth Grad-CAM++ heat map of every class for the one image (torchcam's SmoothGradCAMpp:
    --smoothcampp_samples noisy copies at --smoothcampp_sigma in chunks of --smoothcampp_batch) -> `<out>/smoothcampp_{c}.png`,
    uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import smooth_gradcampp_maps
    return _run_maps(args, model, image, out_dir, "smoothcampp",
                     functools.partial(smooth_gradcampp_maps, model, **_smoothcampp_kwargs(args)))


def _extremal_kwargs(args):
    return dict(areas=(float(getattr(args, "extremal_area", 0.1)),), n_iters=int(getattr(args, "extremal_iters", 800)),
                variant=str(getattr(args, "extremal_variant", "preserve")), batch=int(getattr(args, "extremal_batch", 50)))


def run_extremal(args, model, image, out_dir):
    """--extremal true: the Extremal Perturbation map of every class for the one image (torchray's extremal_perturbation of the
    reference's torchcam_vis.py: --extremal_iters steps on a mask of --extremal_area of the image, variant --extremal_variant, the
    classes in groups of --extremal_batch) -> `<out>/extremal_{c}.png`, uint8 maps at the input resolution; returns them
    [C, H, W]."""
    from .tools.attribution import extremal_maps
    return _run_maps(args, model, image, out_dir, "extremal", functools.partial(extremal_maps, model, **_extremal_kwargs(args)))


def _iba_kwargs(args):
    sigma = float(getattr(args, "iba_sigma", 1.0))
    return dict(beta=float(getattr(args, "iba_beta", 10.0)), steps=int(getattr(args, "iba_steps", 10)),
                samples=int(getattr(args, "iba_samples_per_step", 10)), sigma=sigma if sigma > 0.0 else None,
                batch=int(getattr(args, "iba_batch", 0)) or None)


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

        est = args._iba_estimate = iba_estimate(model, batches(), n_samples=int(getattr(args, "iba_fit", 5000)))
    return est


def run_iba(args, model, image, out_dir):
    """--iba true: the information-bottleneck map of every class for the one image (the IBA the reference's torchcam_vis.py attaches
    to layer4: --iba_steps Adam steps, --iba_samples_per_step samples, weight --iba_beta, window --iba_sigma) ->
    `<out>/iba_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import iba_maps
    return _run_maps(args, model, image, out_dir, "iba", functools.partial(iba_maps, model, estimate=iba_fit(args, model),
                                                                          **_iba_kwargs(args)))


def _igos_kwargs(args):
    return dict(size=int(getattr(args, "igos_size", 8)), n_iters=int(getattr(args, "igos_iters", 15)),
                n_steps=int(getattr(args, "igos_steps", 20)), l1_coeff=float(getattr(args, "igos_l1", 1.0)),
                tv_coeff=float(getattr(args, "igos_tv", 20.0)), batch=int(getattr(args, "igos_batch", 50)))


def run_igos(args, model, image, out_dir):
    """--igos true: the I-GOS map of every class for the one image (the Integrated_Mask of the reference's torchcam_vis.py:
    --igos_iters iterations of --igos_steps path images on a mask of --igos_size cells a side, weights --igos_l1 and --igos_tv, at
    most --igos_batch rows per pass) -> `<out>/igos_{c}.png`, uint8 maps at the input resolution; returns them [C, H, W]."""
    from .tools.attribution import igos_maps
    return _run_maps(args, model, image, out_dir, "igos", functools.partial(igos_maps, model, **_igos_kwargs(args)))


def _ig(args, model, x, classes=None):
    from .tools.attribution import integrated_gradients
    return integrated_gradients(model, x, classes=classes, n_steps=int(getattr(args, "ig_steps", 50)),
                                batch=int(getattr(args, "ig_batch", 50)))


def _smoothgrad(args, model, x, classes=None):
    from .tools.attribution import smoothgrad
    return smoothgrad(model, x, classes=classes, n_samples=int(getattr(args, "smoothgrad_samples", 50)),
                      sigma=float(getattr(args, "smoothgrad_sigma", 1.0)), batch=int(getattr(args, "smoothgrad_batch", 50)))


def _run_gradient_family(args, model, image, out_dir, attribute, stem):
    from .tools.attribution import gradient_maps
    return _run_maps(args, model, image, out_dir, stem,
                     lambda x, min_level: gradient_maps(attribute(args, model, x), min_level=min_level))


def run_ig(args, model, image, out_dir):
    """--ig true: the Integrated Gradients attribution of every class for the one image (captum's IntegratedGradients of the
    reference's captum_vis.py: zero baseline, Gauss-Legendre, --ig_steps steps) -> `<out>/ig_{c}.png`, uint8 maps at the input
    resolution drawn on the device (tools/attribution.py gradient_maps, floored at --grad_min_level); returns them [C, H, W]."""
    return _run_gradient_family(args, model, image, out_dir, _ig, "ig")


def run_smoothgrad(args, model, image, out_dir):
    """--smoothgrad true: the SmoothGrad attribution of every class for the one image (captum's NoiseTunnel of the reference's
    captum_vis.py: --smoothgrad_samples noisy copies at --smoothgrad_sigma) -> `<out>/smoothgrad_{c}.png`, drawn like run_ig;
    returns the uint8 maps [C, H, W]."""
    return _run_gradient_family(args, model, image, out_dir, _smoothgrad, "smoothgrad")


def _family_attribution(args, model, x, pred, family, slot_map=None, full=False):
    """the predicted class's FLOAT explanation of one family for the images x [n, C, H, W] on the device -> [n, 1, h, w] (slot: the
    given `slot_map`, taken right after the forward that predicted; grad: the channel mean of input_gradients; cam: gradcam;
    rise: rise; scorecam: scorecam; ig / smoothgrad: kernels.channel_mean of integrated_gradients / smoothgrad; campp: gradcampp;
    smoothcampp: smooth_gradcampp; extremal: extremal_saliency; iba: information_bottleneck; igos: igos_saliency; sscam: sscam;
    iscam: iscam).  full: grad, ig and smoothgrad keep their attribution
    [n, 1, C, H, W] instead."""
    from . import kernels as K
    from .tools.attribution import extremal_saliency, gradcam, gradcampp, information_bottleneck, input_gradients, rise, scorecam
    from .tools.attribution import igos_saliency, iscam, smooth_gradcampp, sscam
    if family == "sscam":
        return sscam(model, x, classes=[pred], **_sscam_kwargs(args))
    if family == "iscam":
        return iscam(model, x, classes=[pred], **_iscam_kwargs(args))
    if family == "slot":
        return slot_map
    if family == "grad":
        g = input_gradients(model, x, classes=[pred])
        return g if full else g.mean(dim=2)
    if family == "cam":
        return gradcam(model, x, classes=[pred])
    if family == "scorecam":
        return scorecam(model, x, classes=[pred], batch=int(getattr(args, "scorecam_batch", 250)))
    if family == "ig":
        g = _ig(args, model, x, classes=[pred])
        return g if full else K.channel_mean(g)
    if family == "smoothgrad":
        g = _smoothgrad(args, model, x, classes=[pred])
        return g if full else K.channel_mean(g)
    if family == "campp":
        return gradcampp(model, x, classes=[pred])
    if family == "smoothcampp":
        return smooth_gradcampp(model, x, classes=[pred], **_smoothcampp_kwargs(args))
    if family == "extremal":
        return extremal_saliency(model, x, classes=[pred], **_extremal_kwargs(args))
    if family == "iba":
        return information_bottleneck(model, x, iba_fit(args, model), classes=[pred], **_iba_kwargs(args))
    if family == "igos":
        return igos_saliency(model, x, classes=[pred], **_igos_kwargs(args))
    return rise(model, x, classes=[pred], n_masks=int(getattr(args, "rise_masks", 4000)),
                batch=int(getattr(args, "rise_batch", 250)))


def run_causal(args, model, image, pred, families, slot_map=None):
    """--causal true: the deletion / insertion scores (tools/attribution.py causal_metrics) of the predicted class's FLOAT map of
    every family in `families` (slot: `slot_map` [1, 1, h, w], taken right after the forward that predicted; grad: the channel
    mean of input_gradients; cam: gradcam; rise: rise; scorecam: scorecam; ig / smoothgrad: kernels.channel_mean of
    integrated_gradients / smoothgrad; campp: gradcampp; smoothcampp: smooth_gradcampp; extremal: extremal_saliency; iba:
    information_bottleneck; igos: igos_saliency; sscam: sscam; iscam: iscam), one printed
    line each; returns {family: (deletion, insertion)}."""
    from .tools.attribution import causal_metrics
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)
    step, batch = int(getattr(args, "causal_step", 0)) or None, int(getattr(args, "rise_batch", 250))
    scores = {}
    for family in families:
        maps = _family_attribution(args, model, x, pred, family, slot_map)
        r = causal_metrics(model, x, maps, classes=[pred], step=step, batch=batch)
        scores[family] = (float(r.deletion[0, 0]), float(r.insertion[0, 0]))
        print("causal %s class %d: deletion %.6f insertion %.6f" % ((family, pred) + scores[family]))
    return scores


def run_infidelity(args, model, image, pred, families, slot_map=None):
    """--infidelity true: the infidelity (tools/attribution.py infidelity: --infidelity_samples noisy copies at --infidelity_sigma,
    --infidelity_batch rows per forward) of the predicted class's explanation of every family in `families` -- grad, ig and
    smoothgrad with their full [C, H, W] attribution, the other families with their map, which counts for every channel -- one
    printed line each; returns {family: (raw, normalized, beta)}."""
    from .tools.attribution import infidelity
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)
    scores = {}
    for family in families:
        attr = _family_attribution(args, model, x, pred, family, slot_map, full=True)
        r = infidelity(model, x, attr, classes=[pred], n_samples=int(getattr(args, "infidelity_samples", 50)),
                       sigma=float(getattr(args, "infidelity_sigma", 0.003)), batch=int(getattr(args, "infidelity_batch", 50)))
        scores[family] = (float(r.raw[0, 0]), float(r.normalized[0, 0]), float(r.beta[0, 0]))
        print("infidelity %s class %d: raw %.6e normalized %.6e beta %.6e" % ((family, pred) + scores[family]))
    return scores


def run_sensitivity(args, model, image, pred, families):
    """--sensitivity true: the max-sensitivity (tools/attribution.py sensitivity_max: --sensitivity_samples points of the box of
    half-width --sensitivity_radius, --sensitivity_batch rows per call) of the predicted class's FLOAT map of every family in
    `families`, each family explaining the perturbed images as it explained the image (slot: an eval forward, then
    slot_saliency), one printed line each; returns {family: score}."""
    from .tools.attribution import _eval_mode, sensitivity_max, slot_saliency
    x = image.unsqueeze(0).to(args.device, dtype=torch.float32)

    def slot_maps(images):
        with _eval_mode(model), torch.no_grad():
            model(images)
        return slot_saliency(model)[:, pred:pred + 1].contiguous()

    scores = {}
    for family in families:
        explain = slot_maps if family == "slot" else functools.partial(_family_attribution, args, model, pred=pred, family=family)
        r = sensitivity_max(explain, x, n_samples=int(getattr(args, "sensitivity_samples", 10)),
                            radius=float(getattr(args, "sensitivity_radius", 0.02)),
                            batch=int(getattr(args, "sensitivity_batch", 11)))
        scores[family] = float(r.score[0, 0])
        print("sensitivity %s class %d: max %.6e" % (family, pred, scores[family]))
    return scores


def get_test_parser():
    """the training tool's arguments plus this tool's own"""
    parser = argparse.ArgumentParser("single-image xSlot inference", parents=[get_args_parser()])
    parser.add_argument("--checkpoint", default="", help="checkpoint written by train.py (default: the standard name "
                                                         "under --output_dir, if it exists)")
    parser.add_argument("--image", default="", help="image file; a seeded synthetic image is used when empty")
    parser.add_argument("--label", default=None, type=int)
    parser.add_argument("--vis_dir", default="sloter/vis")
    parser.add_argument("--cam", default=False, type=_flag,
                        help="true: write the Grad-CAM heat map of every class as cam_{c}.png into --vis_dir")
    parser.add_argument("--rise", default=False, type=_flag,
                        help="true: write the RISE saliency map of every class as rise_{c}.png into --vis_dir")
    parser.add_argument("--rise_masks", default=4000, type=int, help="number of random masks of --rise")
    parser.add_argument("--rise_batch", default=250, type=int, help="masked images per forward of --rise")
    parser.add_argument("--causal", default=False, type=_flag,
                        help="true: print the deletion / insertion scores of the predicted class's map of every family drawn")
    parser.add_argument("--causal_step", default=0, type=int, help="pixels changed per point of --causal (0: --img_size)")
    parser.add_argument("--scorecam", default=False, type=_flag,
                        help="true: write the Score-CAM heat map of every class as scorecam_{c}.png into --vis_dir")
    parser.add_argument("--scorecam_batch", default=250, type=int, help="masked images per forward of --scorecam")
    parser.add_argument("--ig", default=False, type=_flag,
                        help="true: write the Integrated Gradients map of every class as ig_{c}.png into --vis_dir")
    parser.add_argument("--ig_steps", default=50, type=int, help="Gauss-Legendre steps of --ig")
    parser.add_argument("--ig_batch", default=50, type=int, help="path images per forward and backward of --ig")
    parser.add_argument("--smoothgrad", default=False, type=_flag,
                        help="true: write the SmoothGrad map of every class as smoothgrad_{c}.png into --vis_dir")
    parser.add_argument("--smoothgrad_samples", default=50, type=int, help="noisy copies per class of --smoothgrad")
    parser.add_argument("--smoothgrad_sigma", default=1.0, type=float, help="standard deviation of the noise of --smoothgrad")
    parser.add_argument("--smoothgrad_batch", default=50, type=int, help="noisy copies per forward and backward of --smoothgrad")
    parser.add_argument("--campp", default=False, type=_flag,
                        help="true: write the Grad-CAM++ heat map of every class as campp_{c}.png into --vis_dir")
    parser.add_argument("--smoothcampp", default=False, type=_flag,
                        help="true: write the Smooth Grad-CAM++ heat map of every class as smoothcampp_{c}.png into --vis_dir")
    parser.add_argument("--smoothcampp_samples", default=4, type=int, help="noisy copies per class of --smoothcampp")
    parser.add_argument("--smoothcampp_sigma", default=0.3, type=float, help="standard deviation of the noise of --smoothcampp")
    parser.add_argument("--smoothcampp_batch", default=4, type=int, help="noisy copies per feature pass of --smoothcampp")
    parser.add_argument("--extremal", default=False, type=_flag,
                        help="true: write the Extremal Perturbation map of every class as extremal_{c}.png into --vis_dir")
    parser.add_argument("--extremal_area", default=0.1, type=float, help="fraction of the image the mask of --extremal covers")
    parser.add_argument("--extremal_iters", default=800, type=int, help="SGD steps of --extremal")
    parser.add_argument("--extremal_variant", default="preserve", choices=("preserve", "delete"),
                        help="--extremal keeps (preserve) or removes (delete) the evidence under the mask")
    parser.add_argument("--extremal_batch", default=50, type=int, help="masks per forward and backward of --extremal")
    parser.add_argument("--iba", default=False, type=_flag,
                        help="true: write the information-bottleneck map of every class as iba_{c}.png into --vis_dir")
    parser.add_argument("--iba_beta", default=10.0, type=float, help="weight of the information term of --iba")
    parser.add_argument("--iba_steps", default=10, type=int, help="Adam steps of --iba")
    parser.add_argument("--iba_samples_per_step", default=10, type=int, help="noisy samples per class and step of --iba")
    parser.add_argument("--iba_sigma", default=1.0, type=float, help="standard deviation of the smoothing window of --iba (0: none)")
    parser.add_argument("--iba_fit", default=5000, type=int, help="images the feature distribution of --iba is fitted on")
    parser.add_argument("--iba_batch", default=0, type=int, help="head rows per pass of --iba (0: all classes at once)")
    parser.add_argument("--igos", default=False, type=_flag,
                        help="true: write the I-GOS map of every class as igos_{c}.png into --vis_dir")
    parser.add_argument("--igos_size", default=8, type=int, help="cells a side of the mask of --igos")
    parser.add_argument("--igos_iters", default=15, type=int, help="iterations of --igos")
    parser.add_argument("--igos_steps", default=20, type=int, help="noisy path images per class and iteration of --igos")
    parser.add_argument("--igos_l1", default=1.0, type=float, help="weight of the L1 term of --igos")
    parser.add_argument("--igos_tv", default=20.0, type=float, help="weight of the total-variation term of --igos")
    parser.add_argument("--igos_batch", default=50, type=int, help="images per forward (and backward) of --igos")
    parser.add_argument("--sscam", default=False, type=_flag,
                        help="true: write the SS-CAM heat map of every class as sscam_{c}.png into --vis_dir")
    parser.add_argument("--sscam_samples", default=35, type=int, help="noisy copies of every channel's mask of --sscam")
    parser.add_argument("--sscam_sigma", default=2.0, type=float, help="standard deviation of the noise of --sscam")
    parser.add_argument("--sscam_batch", default=250, type=int, help="masked images per forward of --sscam")
    parser.add_argument("--iscam", default=False, type=_flag,
                        help="true: write the IS-CAM heat map of every class as iscam_{c}.png into --vis_dir")
    parser.add_argument("--iscam_samples", default=10, type=int, help="scales of every channel's mask of --iscam")
    parser.add_argument("--iscam_batch", default=250, type=int, help="masked images per forward of --iscam")
    parser.add_argument("--infidelity", default=False, type=_flag,
                        help="true: print the infidelity of the predicted class's explanation of every family drawn")
    parser.add_argument("--infidelity_samples", default=50, type=int, help="noisy copies of --infidelity")
    parser.add_argument("--infidelity_sigma", default=0.003, type=float, help="standard deviation of the noise of --infidelity")
    parser.add_argument("--infidelity_batch", default=50, type=int,
                        help="rows per forward of --infidelity, the clean image included")
    parser.add_argument("--sensitivity", default=False, type=_flag,
                        help="true: print the max-sensitivity of the predicted class's map of every family drawn")
    parser.add_argument("--sensitivity_samples", default=10, type=int, help="perturbed copies of --sensitivity")
    parser.add_argument("--sensitivity_radius", default=0.02, type=float, help="half-width of the box of --sensitivity")
    parser.add_argument("--sensitivity_batch", default=11, type=int,
                        help="rows per call of the explanation method of --sensitivity, the clean image included")
    return parser


def main():
    args = get_test_parser().parse_args()
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
    if want_grad:
        run_grad(args, model, image, args.vis_dir)
    if args.cam:
        run_cam(args, model, image, args.vis_dir)
    if args.rise:
        run_rise(args, model, image, args.vis_dir)
    if args.scorecam:
        run_scorecam(args, model, image, args.vis_dir)
    if args.ig:
        run_ig(args, model, image, args.vis_dir)
    if args.smoothgrad:
        run_smoothgrad(args, model, image, args.vis_dir)
    if args.campp:
        run_campp(args, model, image, args.vis_dir)
    if args.smoothcampp:
        run_smoothcampp(args, model, image, args.vis_dir)
    if args.extremal:
        run_extremal(args, model, image, args.vis_dir)
    if args.iba:
        run_iba(args, model, image, args.vis_dir)
    if args.igos:
        run_igos(args, model, image, args.vis_dir)
    if args.sscam:
        run_sscam(args, model, image, args.vis_dir)
    if args.iscam:
        run_iscam(args, model, image, args.vis_dir)
    families = [f for f, on in (("slot", model.use_slot), ("grad", want_grad), ("cam", args.cam), ("rise", args.rise),
                                ("scorecam", args.scorecam), ("ig", args.ig), ("smoothgrad", args.smoothgrad),
                                ("campp", args.campp), ("smoothcampp", args.smoothcampp), ("extremal", args.extremal),
                                ("iba", args.iba), ("igos", args.igos), ("sscam", args.sscam), ("iscam", args.iscam)) if on]
    if args.causal:
        run_causal(args, model, image, pred, families, slot_map)
    if args.infidelity:
        run_infidelity(args, model, image, pred, families, slot_map)
    if args.sensitivity:
        run_sensitivity(args, model, image, pred, families)
    print(out)
    print(pred)
    if ratio is not None and args.cal_area_size:
        print(f"attention_ratio: {ratio}")


if __name__ == "__main__":
    main()
