"""Gradient attribution on the HIP path: d output / d image per class (`input_gradients`) and the post-processing the
reference gives every attribution map before it is drawn (`attribution_maps`; reference captum_vis.py:49-59, train.py
--grad / --grad_min_level).  The gradient comes from SlotModel's own backward, which walks on to the image when the input
requires grad (ResNet.features_bwd need_input_grad, kernels.stem_dgrad); saliency is this gradient as it is, integrated
gradients / SmoothGrad / adversarial perturbations are loops over it."""
import numpy as np
import torch


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
