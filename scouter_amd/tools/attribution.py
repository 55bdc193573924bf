"""Gradient attribution on the HIP path: d output / d image per class (`input_gradients`) and the post-processing the
reference gives every attribution map before it is drawn (`attribution_maps`; reference captum_vis.py:49-59, train.py
--grad / --grad_min_level).  The gradient comes from SlotModel's own backward, which walks on to the image when the input
requires grad (ResNet.features_bwd need_input_grad, kernels.stem_dgrad); saliency is this gradient as it is, integrated
gradients / SmoothGrad / adversarial perturbations are loops over it.

Class activation maps at the backbone's output (`gradcam`, `gradcam_maps`): what the reference draws for its FC baseline with
captum's LayerGradCam(model, layer=model.layer4) (captum_vis.py, sloter/utils/grad_cam.py) and compares the slot maps with.
One backbone forward per batch (SlotModel.feature_pass), one head backward per class, the channel-mean weighting and the
uint8 heat maps in two HIP kernels (kernels.gradcam, kernels.cam_maps) -- nothing walks into the backbone."""
import numpy as np
import torch

from .. import kernels as K


def input_gradients(model, images, classes=None, of="log_prob", target=None):
    """Gradient of the model output with respect to `images` [B, C, H, W] -> fp32 [B, K, C, H, W] on the images' device.

    of="log_prob": K = len(classes) (None: every class); slice [:, k] is d(sum_b output[b, classes[k]]) / d images -- one
    eval-mode forward + backward per class, with a one-hot gradient on the model output (the log-probabilities).
    of="loss": K = 1, the gradient of the training loss (losses[0]) for the labels `target`.

    The model is put in eval mode (BatchNorm uses its running statistics and no buffer moves) and the caller's mode is
    restored.  Parameters that require grad get their `.grad` overwritten by each backward, as in any backward of the model."""
    if of not in ("log_prob", "loss"):
        raise ValueError("of must be 'log_prob' or 'loss', got %r" % (of,))
    if images.dim() != 4:
        raise ValueError("images must be [B, C, H, W], got shape %s" % (tuple(images.shape),))
    if of == "loss" and target is None:
        raise ValueError("of='loss' needs target= labels")
    was_training = model.training
    model.eval()
    try:
        grads = []
        with torch.enable_grad():
            if of == "loss":
                x = images.detach().float().clone().requires_grad_(True)
                _, losses = model(x, target)
                grads.append(torch.autograd.grad(losses[0], x)[0])
            else:
                seed = None
                for c in (classes if classes is not None else range(_num_classes(model, images))):
                    x = images.detach().float().clone().requires_grad_(True)
                    out = model(x)
                    if not 0 <= int(c) < out.shape[1]:
                        raise IndexError("class %d out of range (the model has %d outputs)" % (int(c), out.shape[1]))
                    if seed is None:
                        seed = torch.zeros_like(out)
                    seed.zero_()
                    seed[:, int(c)] = 1.0
                    grads.append(torch.autograd.grad(out, x, seed)[0])
        return torch.stack(grads, dim=1)
    finally:
        model.train(was_training)


def _num_classes(model, images):
    slot = getattr(model, "slot", None)
    if slot is not None:
        return int(slot.num_classes)
    return int(model.backbone.fc.out_features)


def attribution_maps(grads, min_level=0.0):
    """[B, K, C, H, W] gradients -> uint8 maps [B, K, H, W] (host side, like SlotAttention.vis_maps).  Per map: mean over the
    channels, negative values cut to 0, min-max scaled to [0, 1], raised to at least `min_level`, min-max scaled again,
    times 255.  A map that is constant at either scaling step (no positive gradient, min_level >= 1) is all zeros -- the
    reference divides 0 / 0 there; SlotAttention.vis_maps makes the same choice."""
    g = grads.detach().double().cpu().numpy() if torch.is_tensor(grads) else np.asarray(grads, dtype=np.float64)
    if g.ndim != 5:
        raise ValueError("grads must be [B, K, C, H, W], got shape %s" % (g.shape,))
    m = np.maximum(g.mean(axis=2), 0.0)
    m = _minmax(m)
    m = _minmax(np.maximum(m, float(min_level)))
    return (m * 255.0).astype(np.uint8)


def _minmax(m):
    """each [H, W] map of m [B, K, H, W] scaled to [0, 1]; a constant map becomes zeros"""
    lo = m.min(axis=(2, 3), keepdims=True)
    span = m.max(axis=(2, 3), keepdims=True) - lo
    return np.where(span > 0, (m - lo) / np.where(span > 0, span, 1.0), 0.0)


def gradcam(model, images, classes=None, relu=False):
    """Grad-CAM of `images` [B, C, H, W] at the backbone's output -> fp32 [B, K, h, w] on the images' device:
    cam[b, k, p] = sum_c mean_p'(d out_k / d features[b, p', c]) * features[b, p, c], captum's LayerGradCam with
    relu_attributions=False (`relu`: clamped at 0).

    classes=None: every class, K = the number of outputs; a list of ints: K = len(classes), slice [:, k] belongs to the
    log-probability of classes[k] (one head backward each, with a one-hot column as its seed); a LongTensor [B]: every image
    its own class, one backward, K = 1.  One SlotModel.feature_pass for the batch -- eval mode, the caller's mode restored,
    BatchNorm-folded when the model's inference fold is on; head parameters that require grad get their `.grad` overwritten
    by each backward.  One feature gradient is alive at a time."""
    if images.dim() != 4:
        raise ValueError("images must be [B, C, H, W], got shape %s" % (tuple(images.shape),))
    B, n = images.shape[0], _num_classes(model, images)
    per_image = torch.is_tensor(classes)
    if per_image:
        if classes.dtype != torch.int64 or classes.dim() != 1 or classes.shape[0] != B:
            raise ValueError("a tensor of classes must be a LongTensor [B = %d], got %s %s"
                             % (B, classes.dtype, tuple(classes.shape)))
        cols = classes.detach().cpu().tolist()
    else:
        cols = [int(c) for c in (classes if classes is not None else range(n))]
    for c in cols:
        if not 0 <= c < n:
            raise IndexError("class %d out of range (the model has %d outputs)" % (c, n))
    fp = model.feature_pass(images)
    feat = fp.features
    _, h, w, _ = feat.shape
    seed = torch.zeros_like(fp.log_probs)
    if per_image:
        seed[torch.arange(B, device=seed.device), classes.to(seed.device)] = 1.0
        seeds = [None]
    else:
        seeds = cols
    cam = torch.empty((B, len(seeds), h, w), dtype=torch.float32, device=feat.device)
    for k, c in enumerate(seeds):
        if c is not None:
            seed.zero_()
            seed[:, c] = 1.0
        dfeat = fp.grad(seed)
        K.gradcam(feat, dfeat, cam[:, k], relu=relu)
        del dfeat
    return cam


def gradcam_maps(model, images, classes=None, size=None, min_level=0.0):
    """uint8 Grad-CAM heat maps [B, K, H, W] on the device: `gradcam`, then per map the reference's drawing steps in one
    launch (kernels.cam_maps; captum_vis.py:51-59) -- bilinear resize to `size` = (H, W) (None: the images' H x W), negative
    values cut to 0, min-max scaled, raised to at least `min_level`, min-max scaled again, times 255.  A map that is constant at
    either scaling step is all zeros, like attribution_maps."""
    H, W = (int(v) for v in (size if size is not None else images.shape[-2:]))
    return K.cam_maps(gradcam(model, images, classes), H, W, min_level)
