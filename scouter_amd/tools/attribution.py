"""Gradient attribution on the HIP path: d output / d image per class (`input_gradients`) and the post-processing the
reference gives every attribution map before it is drawn (`attribution_maps`; reference captum_vis.py:49-59, train.py
--grad / --grad_min_level).  The gradient comes from SlotModel's own backward, which walks on to the image when the input
requires grad (ResNet.features_bwd need_input_grad, kernels.stem_dgrad); saliency is this gradient as it is, integrated
gradients / SmoothGrad / adversarial perturbations are loops over it.

Class activation maps at the backbone's output (`gradcam`, `gradcam_maps`): what the reference draws for its FC baseline with
captum's LayerGradCam(model, layer=model.layer4) (captum_vis.py, sloter/utils/grad_cam.py) and compares the slot maps with.
One backbone forward per batch (SlotModel.feature_pass), one head backward per class, the channel-mean weighting and the
uint8 heat maps in two HIP kernels (kernels.gradcam, kernels.cam_maps) -- nothing walks into the backbone.

Perturbation maps (`rise_masks`, `rise`, `rise_maps`): RISE (Petsiuk et al. 2018), what the reference's torchcam_vis.py draws
with torchray.attribution.rise.  The image is multiplied by thousands of smooth random masks, every masked image goes through
the model, and every mask is weighted by the class probabilities it produced.  No gradient and no feature hook: the same call
serves the xSlot model and the FC baseline, and its cost is eval forwards (BatchNorm-folded when the model's inference fold is
on).  The masks exist only as s x s byte grids and shifts; the masked batch, the weighted sum and the heat maps are three HIP
kernels (kernels.rise_mask_images, kernels.rise_accumulate, kernels.heat_maps) and nothing comes to the host in between.

Scores for any of these maps (`causal_metrics`, `slot_saliency`, `gaussian_taps`): the deletion and insertion areas (DAUC / IAUC)
of the RISE paper's section 4.1, which the SCOUTER paper reports next to the area size.  The pixels of a map are ranked, the
image is edited a row's worth of pixels at a time -- deleted to zero, or inserted into a blurred copy -- and every edited
image goes through the model; the score is the area under the class probability.  Like `rise` its cost is eval forwards; the
resize of a coarse map, the ranking, the blur, the edited batch, the curve and its area are HIP kernels (kernels.resize_bilinear,
saliency_ranks, separable_filter, causal_step_images, causal_curve, causal_auc).  The blur is the plain sampled Gaussian with
zero padding, not the kernel the RISE authors' script derives from scipy's reflecting gaussian_filter.

Activation-masked maps (`scorecam`, `scorecam_maps`): Score-CAM (Wang et al., CVPR-W 2020), the method the gradient-free CAMs of
the reference's torchcam_vis.py (SS-CAM, IS-CAM) are loops over.  Every channel of the backbone's output -- the layer `gradcam`
reads -- is resized to the image, min-max scaled to [0, 1] and multiplied onto the image; every masked image goes through the
model, and every channel is weighted by the class probability its mask produced.  No gradient: one feature pass and one eval
forward per channel (512 for resnet18, 2048 for resnest26d / resnest50d; BatchNorm-folded when the model's inference fold is
on).  A mask exists only as its channel's h x w source values and its range; the ranges, the masked batch, the weights and the
weighted sum are four HIP kernels (kernels.scorecam_ranges, kernels.sscam_mask_images, kernels.sscam_weights,
kernels.sscam_contract) and nothing comes to the host in between.  It is the one-sample row of the stream SS-CAM and IS-CAM run
on, below.

Smoothed and integrated Score-CAM (`sscam`, `sscam_maps`, `iscam`, `iscam_maps`, `iscam_ramp`): SS-CAM (Wang et al. 2020) and
IS-CAM (Naidu et al. 2020), the SSCAM and ISSCAM of the reference's torchcam_vis.py.  Every channel's mask goes through the model
N times -- with Gaussian noise added to the mask (SS-CAM, 35 times at torchcam's defaults), or scaled along a ramp (IS-CAM, 10
times) -- and the channel is weighted by the mean, or the sum, of the class probabilities: N C eval forwards per image, 71 680
for SS-CAM on resnest26d.  The N C rows of an image form one flat stream cut into chunks that may straddle a sample boundary;
the masked noisy batch is written straight into one reused buffer (kernels.sscam_mask_images: Score-CAM's mask expression and
the stream of kernels.noise_images, one noise field per sample shared by all channels), the weights of every class are summed
in float64 per (channel, class) from the one stream (kernels.sscam_weights) and contracted with the features once
(kernels.sscam_contract: one fma per live channel in ascending order), and nothing comes to the host in between.  `scorecam` is
the same loop with one sample, no noise and no ramp, so with those arguments both are `scorecam` bit for bit.  The docstrings
of `sscam` and `iscam` are the definition and list what departs from torchcam: our random stream, one noise field for all images
of a batch, every class from one stream, dead channels weighted 0, no final ReLU and no normalisation.

Gradient methods that need many gradients per image (`integrated_gradients`, `smoothgrad`, `gradient_maps`, `ig_quadrature`):
Integrated Gradients (Sundararajan et al. 2017) and SmoothGrad / SmoothGrad-squared / VarGrad (Smilkov et al. 2017), what the
reference's captum_vis.py runs with captum's IntegratedGradients and NoiseTunnel.  The images on the path from a baseline to
the image, or the image plus Gaussian noise, are written straight into one reused batch buffer (kernels.path_images,
kernels.noise_images: Philox4x32-10 and Box-Muller, a value per (seed, sample, element)), the model's own eval forward and
backward give the gradients of a chunk, and they are summed in float64 in sample order (kernels.grad_accumulate), so the
chunking does not change a bit; kernels.attr_finish forms the result and, for Integrated Gradients, its sum for the
completeness check.  kernels.channel_mean and kernels.heat_maps draw the result on the device (`gradient_maps`, the device
counterpart of `attribution_maps`).  Nothing comes to the host in between.  Both work for any module whose eval forward
returns [n, n_outputs].

Second-order class activation maps (`gradcampp`, `gradcampp_maps`, `smooth_gradcampp`, `smooth_gradcampp_maps`): Grad-CAM++
(Chattopadhay et al. 2018) and Smooth Grad-CAM++ (Omeiza et al. 2019), the GradCAMpp and SmoothGradCAMpp the reference's
torchcam_vis.py draws and the SCOUTER paper tabulates beside the slot maps.  They read the layer and the gradient `gradcam` reads
-- one feature pass, one head backward per class, nothing walks into the backbone -- and weight every position of a channel by
alpha = g^2 / (2 g^2 + sum_p g^3 A) before the rectified gradient is summed; the smooth variant averages g^2 and g^3 over noisy
copies of the image (kernels.noise_images, float64 sums in sample order by kernels.grad_powers_accumulate, so the chunking does
not change a bit) and rectifies the last sample's gradient, as the reference does.  The weighting and the contraction are HIP
kernels (kernels.gradcampp, kernels.gradcampp_smooth); alpha is 0 where the reference divides 0 / 0.  Nothing comes to the host
in between.

Two more scores for any of these explanations (`infidelity`, `sensitivity_max`): the infidelity and the max-sensitivity of Yeh et
al. 2019 ("On the (In)fidelity and Sensitivity of Explanations"), the last two columns of the SCOUTER paper's comparison, which its
authors took from captum.  Infidelity adds Gaussian noise to the image and compares the change of the model's output with what
the attribution predicts for that perturbation; max-sensitivity moves the image inside a small box and measures how far the
explanation moves.  Like `causal_metrics` they cost eval forwards (or calls of the explanation method) over a stream of
perturbed copies written straight into one reused batch buffer (kernels.noise_images, kernels.uniform_images), the clean image
riding in row 0 of every batch; the attribution-times-perturbation sums regenerate the noise instead of reading it
(kernels.perturb_dots), and the output differences, the map distances and the final sums are float64 in one fixed order
(kernels.output_deltas, kernels.map_distances, kernels.infidelity_finish, kernels.sensitivity_finish), so the chunking does not
change a bit of the per-sample sums.  No reference program computes either score here: the definitions in the two docstrings
(and include/scouter_hip.h) are the specification.

An optimised mask (`extremal_perturbation`, `extremal_saliency`, `extremal_maps`, `perturbation_pyramid`, `pyramid_pass_plan`,
`extremal_schedule`): Extremal Perturbation (Fong, Patrick, Vedaldi, ICCV 2019), what the reference's torchcam_vis.py runs with
torchray.attribution.extremal_perturbation right after RISE.  Per image, class and area a coarse mask is upsampled by a smooth
maximum, reads a blur pyramid of the image, and is moved by hundreds of SGD steps towards the mask of that area which keeps (or
deletes) the most class probability.  It is the one method here whose cost is not model passes alone: every iteration pushes
the batch of masks through the upsampler, the pyramid blend, an eval forward and input backward, a ranked area penalty, the
upsampler's backward and the update.  The mask side is five HIP kernels and the ranking of `causal_metrics`
(kernels.extremal_mask, extremal_blend, extremal_seed, saliency_ranks, extremal_mask_grad, extremal_step); the seed of the
backward is written on the device from the forward's own output, so nothing comes to the host for the whole run.  No reference
program runs here (torchray is not a dependency): the docstring of `extremal_perturbation` is the specification, and it lists
what departs from TorchRay.

An optimised mask in feature space (`iba_estimate`, `information_bottleneck`, `iba_saliency`, `iba_maps`): information-bottleneck
attribution (Schulz, Sixt, Tombari, Landgraf, ICLR 2020), the IBA the reference's torchcam_vis.py attaches to model.layer4.  Noise
replaces the backbone's output neuron by neuron, as much as a per-class mask allows, and ten Adam steps trade the class
log-probability against the information the mask lets through; the map is that information in bits per cell.  The layer is the
one `gradcam` reads, so the loop never enters the backbone: the samples go through SlotModel.head_pass and its head backward.
The mask side of an iteration is two HIP kernels (kernels.iba_sample, kernels.iba_step: sigmoid, reflecting Gaussian window, noise
from the stream of kernels.noise_images, blend and capacity; then the analytic gradient, the window's adjoint and Adam in place),
the fitted feature distribution comes from a streaming float64 Welford kernel (kernels.iba_estimate), and nothing comes to the
host in between.  The docstring of `information_bottleneck` is the definition and lists what departs from the reference.

A mask found along integrated gradients (`igos`, `igos_saliency`, `igos_maps`, `igos_ladder`): I-GOS (Qi, Khorram, Fuxin, AAAI
2020), the Integrated_Mask the reference's torchcam_vis.py runs first of all.  Per image and class a coarse mask blends the image
with a blurred copy; every iteration sends twenty noisy images on the path from the blurred copy to the masked image through an
eval forward and input backward, contracts their gradients into the mask's descent direction, and chooses the step by a
backtracking line search.  The reference does this one image and one pass at a time, with host noise and a host read per trial
step; here the classes of an image are the rows of one stream, the path images, the contraction, the upsampler's adjoint with
the L1 / total-variation terms and the trial images are HIP kernels (kernels.igos_path_images, igos_accumulate, igos_mask_grad,
igos_trial_images, igos_upsample), every trial step goes through the model in one batch, and the selection itself runs on the
device (kernels.igos_step), so nothing comes to the host for the whole run.  The docstring of `igos` is the specification and
lists what departs from the reference.

The class activation map itself (`fccam`, `fccam_maps`): CAM (Zhou et al. 2016), the first extractor the reference's
torchcam_vis.py builds -- torchcam's CAM(model, 'layer4', 'fc') on the FC baseline (--use_slot false).  The fc weights of a class
are contracted with the features `gradcam` reads: one feature pass and one HIP kernel (kernels.cam_fc) in which the features
cross HBM once, no backward at all.  It exists for the baseline only; a model with a slot head has no fc layer and is refused.

Where a map lies (`localization`, `slot_maps`): the area size and the precision of the SCOUTER paper's comparison and the strict
pointing game, for the uint8 maps every *_maps function draws, against bounding boxes.  One HIP kernel forms the exact integer
sums of a batch of maps (kernels.map_localization: the mass, the mass inside the union of an image's boxes, the largest byte's
position and whether a box holds it) and the ratios are float64 divisions of them on the device; `slot_maps` gives the byte
slot maps of a whole batch, each image scaled as SlotAttention.vis_maps scales one on the host (kernels.group_maps), the maps
the reference's attention_ratio is taken from.  tools/explanation_table.py puts these scores, `causal_metrics` and `infidelity`
into the paper's table: one row per family, every cell a mean over a validation set.

Superpixel surrogates (`superpixels`, `lime_samples`, `kernelshap_samples`, `lime_fit`, `kernelshap_fit`, `lime`, `kernelshap`,
`lime_maps`, `kernelshap_maps`): LIME (Ribeiro et al. 2016) and KernelSHAP (Lundberg & Lee 2017), the two explainers a comparison
table is asked for first.  The image is cut into at most 128 superpixels (a SLIC loop of two HIP kernels, kernels.slic_update and
kernels.slic_assign), a thousand copies with random subsets of them hidden go through the model, and a weighted linear model of
the class probability over the subsets is fitted; its coefficients, painted back onto the segments, are the map.  Like `rise`
both are black-box and cost eval forwards.  The perturbed batch, the float64 moments of the regression (summed in row order, so
the chunking does not change a bit), the Cholesky fit and the painting are four more HIP kernels (kernels.segment_images,
surrogate_accumulate, surrogate_solve, segment_paint) and nothing comes to the host in between.  No reference program runs
either method here (lime, shap and skimage are not dependencies): the docstrings are the specification and say what departs
from those packages.  tools/surrogate.py adds both as rows to the single-image tool and the explanation table.

Occlusion maps (`occlusion_windows`, `occlusion`, `occlusion_maps`): occlusion sensitivity (Zeiler & Fergus 2014; captum's Occlusion,
from the package the reference's captum_vis.py draws its methods from), the first baseline a perturbation method is compared
with.  A window slides over the image, every occluded copy goes through the model, and a pixel's score is the mean drop of the
class probability over the windows that covered it: the deterministic counterpart of `rise`, with no random stream and no
surrogate.  The occluded batch is written straight into one reused buffer with the clean image in row 0 (kernels.occlude_images),
the drops are float64 differences inside one forward (kernels.output_deltas) and the map is their mean over the covering windows
in one fixed order (kernels.occlusion_finish); nothing comes to the host in between.  Like `rise` it is black-box and costs eval
forwards: 729 for a 224 x 224 image at the default window 16 and stride 8.

The gradient-free class activation map (`ablationcam`, `ablationcam_maps`): Ablation-CAM (Desai & Ramaswamy, WACV 2020).  Every
channel of the layer `gradcam` reads is zeroed in turn and weighted by the relative drop of the class probability.  The ablated
copies are rows of one reused feature buffer (kernels.ablate_channels) and go through SlotModel.head_pass alone -- the backbone
runs once per batch, where `scorecam` runs it once per channel -- the drops come from kernels.output_deltas and the weighted sum
from kernels.ablation_contract (the weight rounded from float64 once, one fma per channel in ascending order).  No backward, and
nothing comes to the host in between.  tools/ablation.py adds both methods as rows to the single-image tool and the explanation
table.

Layer Integrated Gradients (`layer_integrated_gradients`, `layerig_maps`): captum's LayerIntegratedGradients at the layer `gradcam`
reads, the layer the reference's captum_vis.py attributes to.  The straight line runs IN FEATURE SPACE from the baseline image's
features to the image's, so a step is a head forward and a head backward and nothing enters the backbone: for a head that is
linear in the features (the FC baseline's logits) it equals the DeepLIFT the reference draws, and for the slot head it is the
quantity DeepLIFT's Rescale rule approximates (Ancona et al. 2018).  The path rows are written by kernels.path_images into one
reused feature buffer, one SlotModel.head_pass per chunk serves every class (one `.grad` each), kernels.grad_accumulate keeps
float64 sums in step order and kernels.layer_attr_finish forms all maps, the attributions and the completeness sums in one launch.

Layer Conductance (`layer_conductance`, `conductance_maps`): Dhamdhere et al. 2018, captum's LayerConductance.  The path runs IN
IMAGE SPACE, n + 1 equidistant images, and the attribution is sum_i g(A(x_i)) * (A(x_{i+1}) - A(x_i)): what flows through every
element of the backbone's output along the way.  One SlotModel.feature_pass per chunk, one `.grad` per class, and
kernels.conductance_accumulate adds the steps in float64; consecutive chunks share a row, so no step is lost between them.  The
sum over positions and channels telescopes to out(x) - out(x') as the steps shrink.

The class maps that keep the gradient per position (`layer_gradxact`, `hirescam`, `layercam` and their `*_maps`): HiResCAM (Draelos
& Carin 2020; captum's LayerGradientXActivation summed over the channels), sum_c g[p, c] A[p, c], and LayerCAM (Jiang et al. 2021),
relu(sum_c relu(g[p, c]) A[p, c]), where `gradcam` pools the gradient over the positions first.  They run on `gradcam`'s loop with
kernels.layer_gxa as its fill.  tools/layer.py adds the four methods as rows to the single-image tool and the explanation table.

GradientSHAP (`gradient_shap`, drawn by `gradient_maps`; `layer_gradient_shap`, `layergradshap_maps`): expected gradients (Lundberg
& Lee 2017; Erion et al. 2019), captum's GradientShap and LayerGradientShap, the first name the reference's captum_vis.py imports.
The one gradient method here that explains against a DISTRIBUTION of baselines: every sample walks from its own randomly drawn
baseline of a bank by its own random fraction, optionally from a noisy copy of the image, and the attribution is the mean of
gradient times that sample's own difference.  The draws are a Philox stream of their own (kernels.gradshap_draws), the rows are
written by kernels.gradshap_images into the reused buffer of `integrated_gradients` (or, for the layer variant, the feature buffer
of `layer_integrated_gradients`, with one SlotModel.head_pass per chunk), and kernels.gradshap_accumulate forms every sample's
difference again from the draws and adds gradient times difference in float64 in sample order: the differences are never
stored.  tools/gradshap.py adds both methods as rows to the single-image tool and the explanation table.

Guided backpropagation, deconvnet and Guided Grad-CAM (`guided_backprop`, `deconvnet`, `guided_gradcam`, drawn by `gradient_maps`):
Springenberg et al. 2015, Zeiler & Fergus 2014 and Selvaraju et al. 2017; captum's GuidedBackprop, Deconvolution and the
GuidedGradCam the reference's captum_vis.py imports.  The backward to the image with another rule at every ReLU of the backbone:
what is positive in the arriving gradient and lies where the output was positive (guided), or the positive part of the arriving
gradient alone (deconvnet).  They run on SlotModel.image_pass only -- the gradient-only backward of the folded path applies every
ReLU mask in four kernels (kernels.relu_bwd, sa_gate_bwd, sa_apply_relu_bwd, maxpool_relu_bwd), whose `rule` is a compile-time
argument -- so one forward serves every class and there is no autograd form.  Guided Grad-CAM multiplies the guided gradient by
the rectified class map of the backbone's output, brought to the image's size inside kernels.guided_cam; one head backward per
class (ImagePass.feature_grad) serves both factors.  The head's own ReLU keeps the plain rule (captum's hooks do not see it in the
reference) and the log-probabilities are differentiated.  tools/guided.py adds the three methods as rows to the single-image tool
and the explanation table."""
import collections
import contextlib
import functools

import numpy as np
import torch

from .. import kernels as K


_ROUTES = ("autograd", "folded")


def _check_route(route, of="log_prob"):
    """the `route` argument of the image-space gradient methods, checked before any launch"""
    if route not in _ROUTES:
        raise ValueError("route must be 'autograd' or 'folded', got %r" % (route,))
    if route == "folded" and of == "loss":
        raise ValueError("route='folded' differentiates the model output; of='loss' needs route='autograd'")
    return route


def _check_device_images(images):
    """route="folded" has no host form: refused before any launch"""
    if not torch.is_tensor(images) or not images.is_cuda:
        raise RuntimeError("route='folded' runs on a HIP device (got %s); there is no CPU fallback"
                           % (images.device if torch.is_tensor(images) else type(images).__name__,))


@contextlib.contextmanager
def _eval_mode_once(model):
    """_eval_mode for the folded route: a model that is in eval mode already is left alone -- SlotModel.eval() / train() mark the
    folded weights stale (the model would fold them again for every call, and an ImagePass taken before would refuse)"""
    if not getattr(model, "training", False):
        yield
    else:
        with _eval_mode(model):
            yield


def _folded_input_gradients(model, images, classes):
    """input_gradients(route="folded"): ONE model.image_pass and one .grad per class column (a LongTensor: one .grad)"""
    _check_device_images(images)
    B = images.shape[0]
    n = _num_classes(model, images)
    per_image, cols = _class_list(classes, B, n)
    _check_class_range(cols, n)
    with _eval_mode_once(model):
        ip = model.image_pass(images)
        seed = torch.zeros_like(ip.log_probs)
        grads = []
        if per_image:
            seed[torch.arange(B, device=seed.device), classes.to(seed.device)] = 1.0
            grads.append(ip.grad(seed))
        else:
            for c in cols:
                seed.zero_()
                seed[:, c] = 1.0
                grads.append(ip.grad(seed))
    if not grads:
        return torch.empty((B, 0) + tuple(images.shape[1:]), dtype=torch.float32, device=images.device)
    return torch.stack(grads, dim=1)


def input_gradients(model, images, classes=None, of="log_prob", target=None, route="autograd"):
    """Gradient of the model output with respect to `images` [B, C, H, W] -> fp32 [B, K, C, H, W] on the images' device.

    of="log_prob": K = len(classes) (None: every class); slice [:, k] is d(sum_b output[b, classes[k]]) / d images -- one
    eval-mode forward + backward per class, with a one-hot gradient on the model output (the log-probabilities).  A LongTensor
    [B] as `classes`: every image its own class, K = 1 and one backward with the seed 1 at (b, classes[b]), the convention of
    `gradcam` and every other method here (any other tensor is a ValueError, a class outside the outputs an IndexError).  Before
    this form existed a tensor was iterated like a list of ints -- K = len(classes) columns for every image; pass
    `classes.tolist()` for that.
    of="loss": K = 1, the gradient of the training loss (losses[0]) for the labels `target`.

    The model is put in eval mode (BatchNorm uses its running statistics and no buffer moves) and the caller's mode is
    restored.  Parameters that require grad get their `.grad` overwritten by each backward, as in any backward of the model.

    route="autograd" (the default) is the path above: the unfolded layer-by-layer forward and the training backward walked on to
    the image, once per class.  route="folded": ONE forward on the BatchNorm-folded weights (model.image_pass) and one
    gradient-only backward per class column -- no BatchNorm kernel, no parameter gradient of the backbone; of="log_prob" only
    (of="loss" is a ValueError), fp32 models only.  The two routes agree to rounding, not bit for bit: the folded weights are
    rounded once more and the ReLU signs are those of the folded forward.  Any other value is a ValueError before any launch."""
    if of not in ("log_prob", "loss"):
        raise ValueError("of must be 'log_prob' or 'loss', got %r" % (of,))
    _check_route(route, of)
    _check_images(images)
    if of == "loss" and target is None:
        raise ValueError("of='loss' needs target= labels")
    if route == "folded":
        return _folded_input_gradients(model, images, classes)
    with _eval_mode(model):
        grads = []
        with torch.enable_grad():
            if of == "loss":
                x = images.detach().float().clone().requires_grad_(True)
                _, losses = model(x, target)
                grads.append(torch.autograd.grad(losses[0], x)[0])
            elif torch.is_tensor(classes):                     # a LongTensor [B]: every image its own class, one backward, K = 1
                _, cols = _class_list(classes, images.shape[0], None)
                x = images.detach().float().clone().requires_grad_(True)
                out = model(x)
                _check_class_range(cols, out.shape[1])
                seed = torch.zeros_like(out)
                seed[torch.arange(out.shape[0], device=out.device), classes.to(out.device)] = 1.0
                grads.append(torch.autograd.grad(out, x, seed)[0])
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


_RULES = ("gradient", "guided", "deconvnet")
_INTERPOLATE = ("nearest", "bilinear")


def _rule_columns(model, images, classes, rule, column):
    """the loop guided_backprop, deconvnet and guided_gradcam share: the refusals that come before any launch, ONE
    model.image_pass, then column(ip, seed, k) -> fp32 [B, C, H, W] per class column (a LongTensor: one column); stacked to
    [B, K, C, H, W]"""
    if rule not in _RULES:
        raise ValueError("rule must be 'gradient', 'guided' or 'deconvnet', got %r" % (rule,))
    _check_images(images)
    _check_device_images(images)
    if getattr(model, "precision", "fp32") == "bf16":
        raise NotImplementedError('the folded pass has no backward under precision "bf16" (fp32 only)')
    B = images.shape[0]
    n = _num_classes(model, images)
    per_image, cols = _class_columns(classes, B, n)
    with _eval_mode_once(model):
        ip = model.image_pass(images)
        seed = torch.zeros_like(ip.log_probs)
        outs = []
        if per_image:
            seed[torch.arange(B, device=seed.device), classes.to(seed.device)] = 1.0
            outs.append(column(ip, seed, 0, 1))
        else:
            for k, c in enumerate(cols):
                seed.zero_()
                seed[:, c] = 1.0
                outs.append(column(ip, seed, k, len(cols)))
    if not outs:
        return torch.empty((B, 0) + tuple(images.shape[1:]), dtype=torch.float32, device=images.device)
    return torch.stack(outs, dim=1)


def guided_backprop(model, images, classes=None, rule="guided"):
    """Guided backpropagation (Springenberg et al. 2015; captum's GuidedBackprop) of `images` [B, C, H, W] on the device -> fp32
    [B, K, C, H, W]: the backward of the class output to the image in which every ReLU OF THE BACKBONE passes only what is
    positive in the gradient arriving at it AND lies where its output was positive.  `classes` as in `input_gradients`: None
    (every class), a list of ints, or a LongTensor [B] (every image its own class, K = 1).

    ONE forward on the BatchNorm-folded weights (model.image_pass) and one gradient-only backward under the rule per class
    column (ImagePass.grad_from(feature_grad(seed), rule)): the rule is a compile-time switch in the four kernels that apply a ReLU mask there, there is no autograd form.  rule="deconvnet" is
    `deconvnet`, rule="gradient" the plain gradient of input_gradients(route="folded"); anything else is a ValueError before
    any launch.  Departures from captum: the output differentiated is the log-probability (as everywhere here), and the head's
    own ReLU behind conv1x1 keeps the plain rule -- it is `torch.relu` in the reference, not a module captum's hooks see.
    fp32 models only (precision "bf16" is a NotImplementedError); the caller's mode is restored, no BatchNorm buffer moves."""
    return _rule_columns(model, images, classes, rule, lambda ip, seed, k, K_: ip.grad_from(ip.feature_grad(seed), rule))


def deconvnet(model, images, classes=None):
    """The deconvnet rule (Zeiler & Fergus 2014; captum's Deconvolution) -> fp32 [B, K, C, H, W]: `guided_backprop` with every
    ReLU of the backbone passing the positive part of the gradient arriving at it, whatever its output was -- the backward
    kernels do not read the activations at all."""
    return guided_backprop(model, images, classes, rule="deconvnet")


def guided_gradcam(model, images, classes=None, interpolate="nearest"):
    """Guided Grad-CAM (Selvaraju et al. 2017; captum's GuidedGradCam) -> fp32 [B, K, C, H, W]:
    guided_backprop(x)[c] * up(relu(gradcam(x)[c])), the class map of the backbone's output (kernels.gradcam with relu=True)
    brought to the image's size.  interpolate="nearest" (captum's default): source index (y h) // H, (x w) // W;
    "bilinear": the resize of kernels.resize_bilinear.  Anything else is a ValueError before any launch.

    ONE model.image_pass; per class column ONE head backward (ImagePass.feature_grad) that serves both factors -- the class map
    and the guided gradient (ImagePass.grad_from) -- and one launch for the product (kernels.guided_cam).  Nothing is read on the
    host.  `classes`, the departures from captum and the refusals are those of `guided_backprop`."""
    if interpolate not in _INTERPOLATE:
        raise ValueError("interpolate must be 'nearest' or 'bilinear', got %r" % (interpolate,))
    state = {}

    def column(ip, seed, k, K_):
        if "cam" not in state:
            B, h, w, _ = ip.features.shape
            state["cam"] = torch.empty((B, K_, h, w), dtype=torch.float32, device=ip.features.device)
        cam = state["cam"]
        dfeat = ip.feature_grad(seed)
        K.gradcam(ip.features, dfeat, cam[:, k], relu=True)
        g = ip.grad_from(dfeat, "guided")
        return K.guided_cam(g, cam[:, k], out=g, mode=interpolate)
    return _rule_columns(model, images, classes, "guided", column)


@contextlib.contextmanager
def _eval_mode(model):
    """the model in eval mode (BatchNorm uses its running statistics and no buffer moves); the caller's mode is restored"""
    was_training = model.training
    model.eval()
    try:
        yield
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


def _gradient_cam(model, images, classes, fill):
    """the loop shared by gradcam and gradcampp: one feature pass, one head backward per column of `classes`, and
    fill(features, feature gradient, cam[:, k]) for each -- one feature gradient alive at a time"""
    B = _check_images(images).shape[0]
    per_image, cols = _class_columns(classes, B, _num_classes(model, images))
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
        fill(feat, dfeat, cam[:, k])
        del dfeat
    return cam


def gradcam(model, images, classes=None, relu=False):
    """Grad-CAM of `images` [B, C, H, W] at the backbone's output -> fp32 [B, K, h, w] on the images' device:
    cam[b, k, p] = sum_c mean_p'(d out_k / d features[b, p', c]) * features[b, p, c], captum's LayerGradCam with
    relu_attributions=False (`relu`: clamped at 0).

    classes=None: every class, K = the number of outputs; a list of ints: K = len(classes), slice [:, k] belongs to the
    log-probability of classes[k] (one head backward each, with a one-hot column as its seed); a LongTensor [B]: every image
    its own class, one backward, K = 1.  One SlotModel.feature_pass for the batch -- eval mode, the caller's mode restored,
    BatchNorm-folded when the model's inference fold is on; head parameters that require grad get their `.grad` overwritten
    by each backward.  One feature gradient is alive at a time."""
    return _gradient_cam(model, images, classes, lambda feat, dfeat, out: K.gradcam(feat, dfeat, out, relu=relu))


def gradcam_maps(model, images, classes=None, size=None, min_level=0.0):
    """uint8 Grad-CAM heat maps [B, K, H, W] on the device: `gradcam`, then per map the reference's drawing steps in one
    launch (kernels.cam_maps; captum_vis.py:51-59) -- bilinear resize to `size` = (H, W) (None: the images' H x W), negative
    values cut to 0, min-max scaled, raised to at least `min_level`, min-max scaled again, times 255.  A map that is constant at
    either scaling step is all zeros, like attribution_maps."""
    H, W = _out_size(size, images)
    return K.cam_maps(gradcam(model, images, classes), H, W, min_level)


def fccam(model, images, classes=None, relu=False):
    """CAM (Zhou et al., CVPR 2016; torchcam's CAM(model, 'layer4', 'fc'), the first extractor of the reference's
    torchcam_vis.py) of `images` [B, C, H, W] for the FC baseline (--use_slot false) -> fp32 [B, K, h, w] on the images' device:
    cam[b, k, p] = sum_c fc.weight[classes[k], c] * features[b, p, c] (`relu`: clamped at 0) -- CAM._get_weights followed by
    compute_cams: no bias and no 1 / (h w), so mean_p cam[b, k] + fc.bias[classes[k]] is the model's logit.

    classes as in `gradcam`: None (every class), a list of K ints, or a LongTensor [B] (every image its own class, K = 1).  One
    SlotModel.feature_pass for the batch -- eval mode, the caller's mode restored, BatchNorm-folded when the model's inference
    fold is on -- and one launch (kernels.cam_fc); there is no backward at all, so no `.grad` appears.  RuntimeError for a model
    with a slot head: it has no fc layer to read."""
    B = _check_images(images).shape[0]
    if getattr(model, "use_slot", True):
        raise RuntimeError("fccam: the model has a slot head and no fc layer to read: CAM belongs to the --use_slot false "
                           "baseline; gradcam is the method for the slot model")
    weight = model.backbone.fc.weight.detach()
    per_image, cols = _class_columns(classes, B, int(weight.shape[0]))
    feat = model.feature_pass(images).features
    _, h, w, _ = feat.shape
    if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.data_ptr() % 16:
        weight = weight.float().contiguous().clone()
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(feat.device)
    cam = torch.empty((B, 1 if per_image else len(cols), h, w), dtype=torch.float32, device=feat.device)
    if cam.numel() == 0:
        return cam
    return K.cam_fc(feat, weight, cols_dev, cam, per_image=per_image, relu=relu)


def fccam_maps(model, images, classes=None, size=None, min_level=0.0):
    """uint8 CAM heat maps [B, K, H, W] on the device: `fccam`, then the drawing steps of `gradcam_maps` (kernels.cam_maps)."""
    H, W = _out_size(size, images)
    return K.cam_maps(fccam(model, images, classes), H, W, min_level)


def gradcampp(model, images, classes=None, relu=True):
    """Grad-CAM++ (Chattopadhay et al., WACV 2018; torchcam's GradCAMpp) of `images` [B, C, H, W] at the backbone's output -> fp32
    [B, K, h, w] on the images' device.  With A = features[b] (NHWC, p over the h w positions) and g = d out_k / d A:
    S[c] = sum_p g[p, c]^3 A[p, c], alpha[p, c] = g[p, c]^2 / (2 g[p, c]^2 + S[c]), w[c] = sum_p alpha[p, c] max(g[p, c], 0),
    cam[b, k, p] = sum_c w[c] A[p, c], clamped at 0 when `relu` is set (torchcam's final _relu; the default).

    g is the gradient `gradcam` uses: out_k is the LOG-PROBABILITY of class k, the model's output, not the raw score the paper
    and torchcam differentiate.  alpha is 0 where its denominator is 0 (a channel whose gradient vanishes): this DEPARTS from
    the reference, which divides 0 / 0 there and whose _CAM.compute_cams then replaces the NaN product by 1, adding a constant
    to the map -- the choice `attribution_maps` makes for its own 0 / 0.

    classes, the feature pass, the head backwards and their side effects as in `gradcam`: None, a list of ints or a LongTensor
    [B]; one SlotModel.feature_pass, one head backward per class, one feature gradient alive at a time; the weighting and the
    contraction are one HIP kernel (kernels.gradcampp) that fills cam[:, k] in place."""
    return _gradient_cam(model, images, classes, lambda feat, dfeat, out: K.gradcampp(feat, dfeat, out, relu=relu))


def gradcampp_maps(model, images, classes=None, size=None, min_level=0.0, relu=True):
    """uint8 Grad-CAM++ heat maps [B, K, H, W] on the device: `gradcampp`, then the drawing steps of `gradcam_maps` in one launch
    (kernels.cam_maps) at `size` = (H, W) (None: the images' H x W).  A map that is constant at either scaling step is all
    zeros."""
    H, W = _out_size(size, images)
    return K.cam_maps(gradcampp(model, images, classes, relu=relu), H, W, min_level)


def smooth_gradcampp(model, images, classes=None, n_samples=4, sigma=0.3, batch=4, seed=0, relu=True):
    """Smooth Grad-CAM++ (Omeiza et al. 2019; torchcam's SmoothGradCAMpp, whose defaults num_samples = 4 and std = 0.3 these are)
    of `images` [B, C, H, W] at the backbone's output -> fp32 [B, K, h, w] on the images' device.  The samples are
    x_j = x_b + sigma z(seed, j), j < n_samples (kernels.noise_images: the noise of `smoothgrad`, added to the normalised model
    input; sigma is absolute), g_j = d out_k / d features at x_j, q = mean_j g_j^2 and t = mean_j g_j^3.  With A the features of
    the CLEAN image: S[c] = sum_p t[p, c] A[p, c], alpha = q / (2 q + S[c]), w[c] = sum_p alpha[p, c] max(g_last[p, c], 0),
    cam[b, k, p] = sum_c w[c] A[p, c], clamped at 0 when `relu` is set.  g_last is the gradient of the LAST sample, j =
    n_samples - 1, alone: that is what the reference rectifies (torchcam/cams/gradcam.py:272), not a mean over the samples.

    As in `gradcampp`, out_k is the log-probability of class k and alpha is 0 where its denominator is 0.  classes as in
    `gradcam`.  Per image: one clean SlotModel.feature_pass for A, then the noisy copies in chunks of `batch` (the last may be
    shorter) written into one reused buffer, one feature pass per chunk and one head backward per class per chunk, whose
    gradients are summed into per-class float64 sums of squares and cubes in sample order (kernels.grad_powers_accumulate), so
    the chunking does not change a bit; kernels.gradcampp_smooth forms S, alpha and w in float64 and the map in fp32.  Eval
    mode, the caller's mode restored, no BatchNorm buffer moves, nothing is copied to the host and nothing synchronises inside
    the loop; head parameters that require grad get their `.grad` overwritten by each backward."""
    x, batch = _check_images_batch(images, batch)
    n_samples, sigma = int(n_samples), float(sigma)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    if not 0.0 <= sigma < float("inf"):
        raise ValueError("sigma must be finite and not negative, got %r" % (sigma,))
    B = x.shape[0]
    n = _num_classes(model, x)
    per_image, cols = _class_columns(classes, B, n)
    Kc = 1 if per_image else len(cols)
    dev = x.device
    rows = min(batch, n_samples)
    buf = torch.empty((rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
    onehot = torch.zeros((rows, n), dtype=torch.float32, device=dev)
    out = acc2 = acc3 = glast = None
    for b in range(B):
        feat = model.feature_pass(x[b:b + 1]).features
        if out is None:
            _, h, w, C = feat.shape
            out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
            acc2 = torch.empty((Kc, 1, h, w, C), dtype=torch.float64, device=dev)
            acc3 = torch.empty_like(acc2)
            glast = torch.empty((Kc, 1, h, w, C), dtype=torch.float32, device=dev)
        if Kc == 0:
            break
        cb = cols[b:b + 1] if per_image else cols
        acc2.zero_()
        acc3.zero_()
        for first in range(0, n_samples, batch):
            m = min(batch, n_samples - first)
            fp = model.feature_pass(K.noise_images(x[b], buf[:m], sigma, seed, first))
            for k, c in enumerate(cb):
                onehot.zero_()
                onehot[:, c] = 1.0
                g = fp.grad(onehot[:m])
                K.grad_powers_accumulate(g, acc2[k, 0], acc3[k, 0])
                if first + m == n_samples:
                    glast[k, 0].copy_(g[m - 1])
                del g
            del fp
        for k in range(Kc):
            K.gradcampp_smooth(feat, acc2[k], acc3[k], glast[k], out[b:b + 1, k], n_samples, relu=relu)
    return out


def smooth_gradcampp_maps(model, images, classes=None, size=None, min_level=0.0, **smooth_kwargs):
    """uint8 Smooth Grad-CAM++ heat maps [B, K, H, W] on the device: `smooth_gradcampp` (its keyword arguments pass through), then
    the drawing steps of `gradcam_maps` in one launch (kernels.cam_maps) at `size` = (H, W) (None: the images' H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(smooth_gradcampp(model, images, classes, **smooth_kwargs), H, W, min_level)


RiseMasks = collections.namedtuple("RiseMasks", "grids shifts s p size cell")
RiseMasks.__doc__ = """The draws of `rise_masks`: grids uint8 [N, s, s] in {0, 1}, shifts int32 [N, 2] = (dy, dx) with
0 <= dy < cell[0], 0 <= dx < cell[1], the grid size s, the keep-probability p, size = (H, W) and cell = (ceil(H / s), ceil(W / s))."""


def rise_masks(n_masks, size, s=7, p=0.5, seed=0, device=None):
    """The N random masks of a RISE run for images of `size` = (H, W), reusable across calls: from a CPU
    torch.Generator().manual_seed(seed), first every grid (torch.rand(N, s, s) < p), then every shift (torch.randint below the
    cell, rows then columns), uploaded once to `device`.  Mask n is the bilinear upsampling (align_corners=False) of grid n to
    (s + 1) * cell per axis, cropped to H x W at its shift; kernels.rise_mask_images / rise_accumulate form it on the fly."""
    H, W = (int(v) for v in size)
    n_masks, s, p = int(n_masks), int(s), float(p)
    if n_masks < 1:
        raise ValueError("n_masks must be at least 1, got %d" % n_masks)
    if not 1 <= s <= 16 or s > min(H, W):
        raise ValueError("the grid size must satisfy 1 <= s <= 16 and s <= min(H, W) = %d, got %d" % (min(H, W), s))
    if not 0.0 < p < 1.0:
        raise ValueError("the keep-probability must satisfy 0 < p < 1, got %r" % (p,))
    cell = (-(-H // s), -(-W // s))
    gen = torch.Generator().manual_seed(int(seed))
    grids = (torch.rand(n_masks, s, s, generator=gen) < p).to(torch.uint8)
    dy = torch.randint(0, cell[0], (n_masks,), generator=gen)
    dx = torch.randint(0, cell[1], (n_masks,), generator=gen)
    shifts = torch.stack([dy, dx], dim=1).to(torch.int32).contiguous()
    if device is not None:
        grids, shifts = grids.to(device), shifts.to(device)
    return RiseMasks(grids, shifts, s, p, (H, W), cell)


def _check_rise_masks(masks, size, device):
    """a caller's RiseMasks record against the images of this call, once and before any launch (the one host read of the
    shifts)"""
    H, W = size
    if tuple(masks.size) != (H, W):
        raise ValueError("the masks were drawn for %s images, these are %d x %d" % (tuple(masks.size), H, W))
    s = int(masks.s)
    if not 1 <= s <= 16 or s > min(H, W) or not 0.0 < float(masks.p) < 1.0:
        raise ValueError("masks: s = %r, p = %r (1 <= s <= 16, s <= min(H, W), 0 < p < 1)" % (masks.s, masks.p))
    g, sh = masks.grids, masks.shifts
    if g.dtype != torch.uint8 or sh.dtype != torch.int32 or g.dim() != 3 or tuple(g.shape[1:]) != (s, s) or g.shape[0] < 1 or \
            tuple(sh.shape) != (g.shape[0], 2):
        raise ValueError("masks: grids must be uint8 [N, %d, %d] and shifts int32 [N, 2] (got %s %s and %s %s)"
                         % (s, s, g.dtype, tuple(g.shape), sh.dtype, tuple(sh.shape)))
    cell = torch.tensor([-(-H // s), -(-W // s)], dtype=torch.int32)
    shc = sh.cpu()
    if bool((shc < 0).any()) or bool((shc >= cell).any()):
        raise ValueError("masks: a shift lies outside [0, cell) = [0, %d) x [0, %d)" % (int(cell[0]), int(cell[1])))
    return g.to(device).contiguous(), sh.to(device).contiguous()


def rise(model, images, classes=None, n_masks=4000, s=7, p=0.5, batch=250, seed=0, masks=None):
    """RISE saliency of `images` [B, C, H, W] -> fp32 [B, K, H, W] on the images' device:
    S[b, k] = 1 / (N p) * sum_n exp(log_prob_n[classes[k]]) * mask_n, log_prob_n the eval-mode output for images[b] * mask_n.

    classes as in `gradcam`: None (every class), a list of ints (K = len), or a LongTensor [B] (each image its own class,
    K = 1).  The N = n_masks masks are `rise_masks(n_masks, (H, W), s, p, seed)` or the record given as `masks` (then n_masks,
    s, p and seed are taken from it), the same for every image of the call.  Per image they go through the model in chunks of
    `batch` (the last may be shorter): kernels.rise_mask_images into one reused buffer, the model under torch.no_grad() in eval
    mode (folded when the model's inference fold is on; the caller's mode is restored), kernels.rise_accumulate onto the
    result in mask order -- the same bits for any two runs.  No BatchNorm buffer moves, no `.grad` appears, nothing is copied
    to the host and nothing synchronises inside the loop."""
    B, C, H, W = _check_images(images).shape
    per_image, cols = _class_columns(classes, B, _num_classes(model, images))
    x, batch = _check_images_batch(images, batch)
    dev = images.device
    if masks is None:
        masks = rise_masks(n_masks, (H, W), s=s, p=p, seed=seed, device=dev)
        grids, shifts = masks.grids, masks.shifts
    else:
        grids, shifts = _check_rise_masks(masks, (H, W), dev)
    N, s = int(grids.shape[0]), int(masks.s)
    scale = 1.0 / (N * float(masks.p))
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    Kc = 1 if per_image else len(cols)
    out = torch.zeros((B, Kc, H, W), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    buf = torch.empty((min(batch, N), C, H, W), dtype=torch.float32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            for n0 in range(0, N, batch):
                g, sh = grids[n0:n0 + batch], shifts[n0:n0 + batch]
                chunk = K.rise_mask_images(x[b], g, sh, buf[:g.shape[0]], s, check_shifts=False)
                logp = model(chunk)
                K.rise_accumulate(logp, cb, g, sh, out[b], s, scale, check_shifts=False)
    return out


def rise_maps(model, images, classes=None, min_level=0.0, **rise_kwargs):
    """uint8 RISE heat maps [B, K, H, W] on the device: `rise`, then per map the drawing steps of `gradcam_maps` at the maps'
    own size (kernels.heat_maps): negative values cut to 0, min-max scaled, raised to at least `min_level`, min-max scaled
    again, times 255.  A map that is constant at either scaling step is all zeros."""
    return K.heat_maps(rise(model, images, classes, **rise_kwargs), min_level)


Superpixels = collections.namedtuple("Superpixels", "labels d means")
Superpixels.__doc__ = """The segmentation of `superpixels`: labels int32 [B, H, W] in [0, d), the number of segments d and
means fp32 [B, d, C], the mean colour of every segment (0 for a segment without a pixel)."""

SurrogateFit = collections.namedtuple("SurrogateFit", "coef intercept labels")
SurrogateFit.__doc__ = """What `lime_fit` / `kernelshap_fit` return: coefficients float64 [B, K, d], one per class and
segment, intercepts float64 [B, K] and the segments' labels int32 [B, H, W]."""

_MAX_SEGMENTS = K.SURROGATE_MAX_D


def _check_segment_count(d):
    if not 1 <= d <= _MAX_SEGMENTS:
        raise ValueError("the number of segments must satisfy 1 <= d <= %d, got %d" % (_MAX_SEGMENTS, d))
    return d


def superpixels(images, segments=(8, 8), iters=10, compactness=1.0, d=None):
    """Superpixels of `images` [B, C, H, W] -> Superpixels(labels int32 [B, H, W], d, means fp32 [B, d, C]) on the images' device.

    segments = (gy, gx) (an int g: (g, g)), 1 <= gy <= H, 1 <= gx <= W, d = gy * gx <= 128.  labels_0 is the grid: pixel (y, x) lies
    in cell (y * gy // H, x * gx // W) and cell (i, j) has label i * gx + j.  For t = 1 .. iters: centres = update(x, labels_{t-1})
    (kernels.slic_update: per segment the mean colour and the mean (y, x), float64 sums rounded once to fp32; an empty segment
    keeps its centre), labels_t = assign(x, centres) (kernels.slic_assign: among the centres of the 3 x 3 cells around the
    pixel's home cell the smallest D^2 = sum_c (x_c - mu_c)^2 + lam ((y - c_y)^2 + (x - c_x)^2), lam = (compactness / S)^2,
    S = sqrt(H W / d); the smallest label among equals).  iters = 0 gives the plain grid.  means are those of the final labels
    (one more update).

    This is SLIC (Achanta et al. 2012) WITHOUT its connectivity pass -- a segment may have stray pixels -- and on the image as
    it is given, the normalised tensor, not Lab: what skimage.segmentation.slic would give differs.  The compactness default
    of 1.0 is untuned.

    segments may instead be an int32 tensor [B, H, W] of labels from elsewhere, passed with d= (every label in [0, d), checked
    once on the host before any launch); then only the means are computed."""
    B, C, H, W = _check_images(images).shape
    if torch.is_tensor(segments):
        if d is None:
            raise ValueError("a tensor of labels needs d=, the number of segments")
        d = _check_segment_count(int(d))
        if segments.dtype != torch.int32 or tuple(segments.shape) != (B, H, W):
            raise ValueError("a tensor of labels must be int32 [%d, %d, %d], got %s %s"
                             % (B, H, W, segments.dtype, tuple(segments.shape)))
        host = segments.detach().cpu()
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= d):
            raise ValueError("a label lies outside [0, d = %d): the labels span [%d, %d]" % (d, int(host.min()), int(host.max())))
        gy, gx, iters, given = 1, d, 0, segments.detach().to(images.device).contiguous()
    else:
        gy, gx = (int(segments),) * 2 if isinstance(segments, int) else (int(v) for v in segments)
        if not (1 <= gy <= H and 1 <= gx <= W):
            raise ValueError("the grid must satisfy 1 <= gy <= H = %d and 1 <= gx <= W = %d, got %d x %d" % (H, W, gy, gx))
        d, given = _check_segment_count(gy * gx), None
        iters = int(iters)
        if iters < 0 or not float(compactness) >= 0.0:
            raise ValueError("iters and compactness must be at least 0, got %r and %r" % (iters, compactness))
    x = images.detach().contiguous()
    x = x.float() if x.dtype != torch.float32 else x
    dev = x.device
    if given is None:
        rows = (torch.arange(H, dtype=torch.int64) * gy) // H
        cells = (torch.arange(W, dtype=torch.int64) * gx) // W
        grid = (rows[:, None] * gx + cells[None, :]).to(torch.int32)
        labels = grid.to(dev).unsqueeze(0).repeat(B, 1, 1)
    else:
        labels = given
    lam = (float(compactness) / (H * W / float(d)) ** 0.5) ** 2
    centres = torch.zeros((B, d, C + 2), dtype=torch.float32, device=dev)
    means = torch.empty((B, d, C), dtype=torch.float32, device=dev)
    for _ in range(iters):
        K.slic_update(x, labels, centres, means, gy, gx)
        K.slic_assign(x, centres, labels, gy, gx, lam)
    K.slic_update(x, labels, centres, means, gy, gx, window=given is None)
    return Superpixels(labels, d, means)


def _check_samples_shape(N, d):
    N, d = int(N), _check_segment_count(int(d))
    if N < 1:
        raise ValueError("the number of samples must be at least 1, got %d" % N)
    return N, d


def lime_samples(N, d, seed=0):
    """The N x d sample matrix of a LIME run, uint8 on the host: from a CPU torch.Generator().manual_seed(seed),
    torch.rand(N, d) < 0.5, then row 0 set to all ones (the image itself), as lime_image draws them."""
    N, d = _check_samples_shape(N, d)
    gen = torch.Generator().manual_seed(int(seed))
    z = (torch.rand(N, d, generator=gen) < 0.5).to(torch.uint8)
    z[0] = 1
    return z


def kernelshap_samples(N, d, seed=0):
    """The N x d sample matrix of a KernelSHAP run, uint8 on the host.  Row 0 is all ones, row 1 all zeros.  From a CPU
    torch.Generator().manual_seed(seed): first the sizes of rows 2 .. N - 1, m in [1, d - 1] with probability proportional to
    (d - 1) / (m (d - m)) (one torch.multinomial with replacement), then torch.rand(N - 2, d), of which row n keeps its m
    smallest entries (the first among equals).  Rows drawn under this size law carry weight 1 in the regression: the Shapley
    kernel by importance sampling.  N >= d + 2; for d = 1 the matrix is rows 0 and 1 alone (N >= 2).  No paired (complement)
    sampling."""
    N, d = _check_samples_shape(N, d)
    if N < (d + 2 if d > 1 else 2):
        raise ValueError("KernelSHAP needs N >= d + 2 = %d samples (2 for d = 1), got %d" % (d + 2, N))
    z = torch.zeros((N if d > 1 else 2, d), dtype=torch.uint8)
    z[0] = 1
    if d > 1 and N > 2:
        gen = torch.Generator().manual_seed(int(seed))
        m = torch.arange(1, d, dtype=torch.float64)
        sizes = torch.multinomial((d - 1) / (m * (d - m)), N - 2, replacement=True, generator=gen) + 1
        order = torch.rand(N - 2, d, generator=gen).argsort(dim=1, stable=True).argsort(dim=1, stable=True)
        z[2:] = (order < sizes[:, None]).to(torch.uint8)
    return z


def _check_sample_matrix(z, d, shap):
    """a caller's sample matrix against the segmentation of this call"""
    if not torch.is_tensor(z) or z.dtype != torch.uint8 or z.dim() != 2 or z.shape[1] != d or z.shape[0] < 1:
        raise ValueError("samples must be uint8 [N, d = %d], got %s" % (d, (z.dtype, tuple(z.shape)) if torch.is_tensor(z) else type(z)))
    if shap:
        head = z[:2].cpu()
        if z.shape[0] < 2 or not bool(head[0].all()) or bool(head[1].any()):
            raise ValueError("KernelSHAP samples: row 0 must be all ones and row 1 all zeros")
    return z


def _surrogate_fit(model, images, classes, seg, z, batch, hide, mode, kernel_width, ridge):
    """the loop LIME and KernelSHAP share: image, then chunk of sample rows; then one fit for all images"""
    B, C, H, W = images.shape
    if isinstance(hide, str) and hide != "mean":
        raise ValueError('hide must be "mean" or a number, got %r' % (hide,))
    if not float(ridge) >= 0.0:
        raise ValueError("ridge must be at least 0, got %r" % (ridge,))
    per_image, cols = _class_columns(classes, B, _num_outputs(model, images))
    x, batch = _check_images_batch(images, batch)
    dev = x.device
    z = z.to(dev).contiguous()
    N, d = z.shape
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    Kc = 1 if per_image else len(cols)
    if Kc == 0:
        return SurrogateFit(torch.empty((B, 0, d), dtype=torch.float64, device=dev),
                            torch.empty((B, 0), dtype=torch.float64, device=dev), seg.labels)
    means = seg.means if hide == "mean" else None
    fill = 0.0 if means is not None else float(hide)
    S = torch.zeros((B, d + 1, d + 1), dtype=torch.float64, device=dev)
    T = torch.zeros((B, d + 1, Kc), dtype=torch.float64, device=dev)
    yref = torch.zeros((B, 2, Kc), dtype=torch.float64, device=dev)
    buf = torch.empty((min(batch, N), C, H, W), dtype=torch.float32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            for n0 in range(0, N, batch):
                zc = z[n0:n0 + batch]
                chunk = K.segment_images(x[b], seg.labels[b], zc, buf[:zc.shape[0]], None if means is None else means[b], fill)
                K.surrogate_accumulate(model(chunk), cb, zc, S[b], T[b], yref[b], n0, mode, kernel_width)
        coef, icpt = K.surrogate_solve(S, T, yref, mode, ridge)
    return SurrogateFit(coef, icpt, seg.labels)


def _segmentation(images, segments, slic_iters, compactness, d):
    return segments if isinstance(segments, Superpixels) else superpixels(images, segments, slic_iters, compactness, d)


def lime_fit(model, images, classes=None, n_samples=1000, segments=(8, 8), batch=250, seed=0, hide="mean", kernel_width=0.25,
             ridge=1.0, slic_iters=10, compactness=1.0, samples=None, d=None):
    """LIME (Ribeiro et al. 2016, lime_image's arithmetic) for `images` [B, C, H, W] -> SurrogateFit(coef float64 [B, K, d],
    intercept float64 [B, K], labels int32 [B, H, W]) on the images' device.

    The segments are `superpixels(images, segments, slic_iters, compactness, d)` (or a Superpixels record given as `segments`),
    the samples z uint8 [N, d] are `lime_samples(n_samples, d, seed)` (or `samples`), the same for every image.  Row n shows the
    image where z[n, segment] is set and `hide` elsewhere: "mean", the segment's mean colour (lime_image's default), or a number,
    a constant fill.  The targets are y[n, k] = exp(log_prob_n[classes[k]]) in float64, the weights pi_n = sqrt(exp(-D_n^2 /
    kernel_width^2)) with D_n = 1 - sqrt(|z_n| / d) (1 for an empty row), and the fit minimises sum_n pi_n (y_n - b - w . z_n)^2 +
    ridge |w|^2 with a free intercept b (sklearn's Ridge(alpha=1) at the default).  LIME's feature selection is left out: every
    segment keeps its coefficient.

    classes as in `gradcam` / `rise`; any module whose eval forward returns [n, n_outputs] works.  Per image the rows go through
    the model in chunks of `batch`: kernels.segment_images into one reused buffer, the model under torch.no_grad() in eval mode
    (folded when the model's inference fold is on; the caller's mode is restored), kernels.surrogate_accumulate onto the float64
    moments in row order -- the same bits for any `batch` -- and one kernels.surrogate_solve at the end.  No BatchNorm buffer
    moves, no `.grad` appears, nothing is copied to the host and nothing synchronises inside the loop."""
    seg = _segmentation(_check_images(images), segments, slic_iters, compactness, d)
    z = lime_samples(n_samples, seg.d, seed) if samples is None else _check_sample_matrix(samples, seg.d, False)
    if not float(kernel_width) > 0.0:
        raise ValueError("kernel_width must be positive, got %r" % (kernel_width,))
    return _surrogate_fit(model, images, classes, seg, z, batch, hide, K.SURROGATE_LIME, float(kernel_width), ridge)


def kernelshap_fit(model, images, classes=None, n_samples=1000, segments=(8, 8), batch=250, seed=0, hide=0.0, ridge=0.0,
                   slic_iters=10, compactness=1.0, samples=None, d=None):
    """KernelSHAP (Lundberg & Lee 2017) for `images` [B, C, H, W] -> SurrogateFit(coef = phi float64 [B, K, d], intercept = y_0
    float64 [B, K], labels int32 [B, H, W]) on the images' device.

    Segments, perturbed rows, targets and the loop are those of `lime_fit`; the samples are `kernelshap_samples(n_samples, d,
    seed)` (row 0 the image, row 1 everything hidden, the rest drawn under the Shapley kernel's size law, so every row weighs 1)
    and `hide` defaults to the constant 0.0, the dataset mean of a normalised image.  The fit minimises sum_n (y_n - y_0 -
    phi . z_n)^2 + ridge |phi|^2 with the intercept fixed at y_0, the target of row 1, and sum(phi) = y_full - y_0 enforced
    exactly by eliminating the last segment.  n_samples >= d + 2.  No paired sampling and no exhaustive enumeration of small
    coalitions (shap's KernelExplainer does both); a singular system (fewer distinct rows than segments) gives NaN."""
    seg = _segmentation(_check_images(images), segments, slic_iters, compactness, d)
    z = kernelshap_samples(n_samples, seg.d, seed) if samples is None else _check_sample_matrix(samples, seg.d, True)
    return _surrogate_fit(model, images, classes, seg, z, batch, hide, K.SURROGATE_SHAP, 1.0, ridge)


def lime(model, images, classes=None, **lime_kwargs):
    """LIME saliency fp32 [B, K, H, W] on the device: `lime_fit`, every pixel painted with its segment's coefficient
    (kernels.segment_paint)."""
    fit = lime_fit(model, images, classes, **lime_kwargs)
    return K.segment_paint(fit.coef, fit.labels)


def kernelshap(model, images, classes=None, **shap_kwargs):
    """KernelSHAP saliency fp32 [B, K, H, W] on the device: `kernelshap_fit`, every pixel painted with its segment's phi
    (kernels.segment_paint)."""
    fit = kernelshap_fit(model, images, classes, **shap_kwargs)
    return K.segment_paint(fit.coef, fit.labels)


def lime_maps(model, images, classes=None, min_level=0.0, **lime_kwargs):
    """uint8 LIME heat maps [B, K, H, W] on the device: `lime`, then the drawing steps of `rise_maps` (kernels.heat_maps), which
    cut negative coefficients to 0 -- lime_image's positive_only."""
    return K.heat_maps(lime(model, images, classes, **lime_kwargs), min_level)


def kernelshap_maps(model, images, classes=None, min_level=0.0, **shap_kwargs):
    """uint8 KernelSHAP heat maps [B, K, H, W] on the device: `kernelshap`, then the drawing steps of `rise_maps`
    (kernels.heat_maps); negative phi are cut to 0."""
    return K.heat_maps(kernelshap(model, images, classes, **shap_kwargs), min_level)


def scorecam(model, images, classes=None, batch=250):
    """Score-CAM of `images` [B, Cin, H, W] at the backbone's output -> fp32 [B, K, h, w] on the images' device:
    S[b, k, p] = sum_c live_c * exp(log_prob_c[classes[k]]) * A[b, p, c], A = model.feature_pass(images).features (NHWC
    [B, h, w, C], the layer `gradcam` reads) and log_prob_c the eval-mode output for images[b] * mask_c.  mask_c is channel c of
    A[b] resized bilinearly to H x W (align_corners=False), minus its minimum lo_c over the H x W pixels, divided by its span
    hi_c - lo_c; a channel whose span is not positive (a constant channel) is dead: its mask is all zeros and its weight 0 -- the
    official implementation's "skip a constant channel", without a host read (its zero image still goes through the model).
    The channels are summed in ascending order.

    The paper's final ReLU is NOT applied: backbone features are post-ReLU and the weights are probabilities, so it changes
    nothing there, and `kernels.cam_maps` cuts negative values as its first drawing step anyway.  The result stays at h x w, like
    `gradcam`: bilinear resizing is linear, so resizing S (what `scorecam_maps` does) equals the official sum of upsampled maps.

    classes as in `gradcam` / `rise`: None (every class), a list of ints (K = len), or a LongTensor [B] (each image its own
    class, K = 1).  It is the one-sample row of the stream `sscam` and `iscam` run on (`_scorecam_stream` with n_samples = 1, no
    noise, no ramp, norm = 1).  Per image: kernels.scorecam_ranges once, then the C masked images go through the model in chunks
    of `batch` (the last may be shorter): kernels.sscam_mask_images into one reused buffer, the model under torch.no_grad() in
    eval mode (folded when the model's inference fold is on; the caller's mode is restored), kernels.sscam_weights (each
    channel's probabilities, held in float64, which holds an fp32 value exactly); kernels.sscam_contract at the end, one fma per
    live channel in ascending order -- the same bits for any two runs.  No BatchNorm buffer moves, no `.grad` appears, nothing is
    copied to the host and nothing synchronises inside the loop."""
    return _scorecam_stream(model, images, classes, 1, 0.0, batch, 0, False, 1.0)


def scorecam_maps(model, images, classes=None, size=None, min_level=0.0, batch=250):
    """uint8 Score-CAM heat maps [B, K, H, W] on the device: `scorecam`, then per map the drawing steps of `gradcam_maps` in one
    launch (kernels.cam_maps) -- bilinear resize to `size` = (H, W) (None: the images' H x W), negative values cut to 0, min-max
    scaled, raised to at least `min_level`, min-max scaled again, times 255.  A map that is constant at either scaling step is
    all zeros."""
    H, W = _out_size(size, images)
    return K.cam_maps(scorecam(model, images, classes, batch=batch), H, W, min_level)


def iscam_ramp(n_samples):
    """The scales of `iscam` as fp32 [n_samples] (host): scale_j = float32((j + 1) (j + 2) / (2 N)), the partial sum of
    (t + 1) / N over t <= j in closed form -- the reference accumulates fmap += (i + 1) / N * input * mask, so the image of step i
    carries that partial sum.  kernels.sscam_mask_images forms the same value on the device."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    j = np.arange(n_samples, dtype=np.float64)
    return ((j + 1.0) * (j + 2.0) / (2.0 * n_samples)).astype(np.float32)


def _scorecam_stream(model, images, classes, n_samples, sigma, batch, seed, ramp, norm):
    """the loop shared by scorecam, sscam and iscam: per image the n_samples * C rows as one flat stream cut into chunks of
    min(batch, C) rows, float64 weight sums per (channel, class), one contraction at the end"""
    B, Cin, H, W = _check_images(images).shape
    per_image, cols = _class_columns(classes, B, _num_classes(model, images))
    x, batch = _check_images_batch(images, batch)
    dev = images.device
    feat = model.feature_pass(x).features.detach()          # (the FeaturePass and its head state are dropped here)
    feat = (feat.float() if feat.dtype != torch.float32 else feat).contiguous()
    _, h, w, C = feat.shape
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    Kc = 1 if per_image else len(cols)
    out = torch.zeros((B, Kc, h, w), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    rows, step = n_samples * C, min(batch, C)
    buf = torch.empty((step, Cin, H, W), dtype=torch.float32, device=dev)
    ranges = torch.empty((C, 2), dtype=torch.float32, device=dev)
    wsum = torch.empty((C, Kc), dtype=torch.float64, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            K.scorecam_ranges(feat[b], H, W, out=ranges)
            wsum.zero_()
            for first in range(0, rows, step):
                chunk = K.sscam_mask_images(x[b], feat[b], ranges, buf[:min(step, rows - first)], first, n_samples, sigma, seed,
                                            ramp)
                K.sscam_weights(model(chunk), cb, wsum, first)
            K.sscam_contract(wsum, feat[b], ranges, out[b], norm)
    return out


def sscam(model, images, classes=None, n_samples=35, sigma=2.0, batch=250, seed=0):
    """SS-CAM (Wang et al. 2020; torchcam's SSCAM, whose defaults these are) of `images` [B, Cin, H, W] at the backbone's output
    -> fp32 [B, K, h, w] on the images' device: `scorecam` with every channel's weight averaged over n_samples noisy copies of its
    mask, S[b, k, p] = sum_c live_c * w[c, k] * A[b, p, c], w[c, k] = (1 / N) sum_j exp(log_prob_{j,c}[classes[k]]), log_prob_{j,c}
    the eval-mode output for images[b] * (mask_c + sigma * z_j).  A, mask_c, live and dead are `scorecam`'s.  z_j is standard
    normal, a function of (seed, j, image element) alone (kernels.noise_images' stream): it has the image's shape [Cin, H, W] and is
    the same for every channel c, as in torchcam, where one draw is broadcast over all masks.  In fp32: sigma * z is one product,
    added to the mask in one sum, times the image.  sigma is absolute (>= 0); sigma = 0 forms no noise.

    The weight sums are float64 per (channel, class) in sample order and are rounded to fp32 once, w32 = float32(sum / N); then
    the live channels are added in ascending order, one fma each, as in `scorecam`.  So sscam(n_samples=1, sigma=0) equals
    `scorecam` bit for bit.

    Per image the N * C rows form one flat stream, row r = sample r // C, channel r % C, cut into chunks of min(batch, C) rows
    that may straddle a sample boundary (no short chunk at the end of every sample) but never hold a channel twice:
    kernels.scorecam_ranges once, then per chunk kernels.sscam_mask_images into one reused buffer, the model under
    torch.no_grad() in eval mode (folded when the model's inference fold is on; the caller's mode is restored) and
    kernels.sscam_weights; kernels.sscam_contract at the end.  The same bits for any two runs.  No BatchNorm buffer moves, no
    `.grad` appears, nothing is copied to the host and nothing synchronises inside the loop.  classes as in `scorecam`.

    What departs from torchcam: the noise comes from our Philox stream, not torch's host generator; one noise field serves all
    images of the batch (sample j of every image); every class is weighted from the ONE stream of forwards, where the reference
    repeats the loop, and redraws the noise, per class; a dead channel is weighted 0, where the reference divides 0 / 0 in
    _normalize; and, as in `scorecam`, there is no final ReLU and no normalisation -- `sscam_maps` / kernels.cam_maps do both."""
    n_samples, sigma = int(n_samples), float(sigma)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    if not 0.0 <= sigma < float("inf"):
        raise ValueError("sigma must be finite and not negative, got %r" % (sigma,))
    return _scorecam_stream(model, images, classes, n_samples, sigma, batch, seed, False, 1.0 / n_samples)


def sscam_maps(model, images, classes=None, size=None, min_level=0.0, n_samples=35, sigma=2.0, batch=250, seed=0):
    """uint8 SS-CAM heat maps [B, K, H, W] on the device: `sscam`, then the drawing steps of `scorecam_maps` in one launch
    (kernels.cam_maps) at `size` = (H, W) (None: the images' H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(sscam(model, images, classes, n_samples=n_samples, sigma=sigma, batch=batch, seed=seed), H, W, min_level)


def iscam(model, images, classes=None, n_samples=10, batch=250):
    """IS-CAM (Naidu et al. 2020; torchcam's ISCAM, whose default this is) of `images` [B, Cin, H, W] at the backbone's output ->
    fp32 [B, K, h, w] on the images' device: `scorecam` with every channel's mask sent through the model n_samples times along
    a ramp, S[b, k, p] = sum_c live_c * w[c, k] * A[b, p, c], w[c, k] = sum_j exp(log_prob_{j,c}[classes[k]]) -- a SUM, with no
    division by N, as in the reference -- and log_prob_{j,c} the eval-mode output for images[b] * (scale_j * mask_c), scale_j =
    `iscam_ramp(n_samples)[j]` (one fp32 product with the mask).  No noise and no seed.

    The float64 weight sums, the flat stream of N * C rows, the kernels and the guarantees are `sscam`'s; iscam(n_samples=1)
    equals `scorecam` bit for bit (scale_0 = 1).  classes as in `scorecam`.

    What departs from torchcam: every class is weighted from the one stream of forwards (the reference repeats the loop per
    class); a dead channel is weighted 0, where the reference divides 0 / 0 in _normalize; no final ReLU and no normalisation
    -- `iscam_maps` / kernels.cam_maps do both.  There is no random stream to differ in, and nothing is shared between the
    images of a batch."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    return _scorecam_stream(model, images, classes, n_samples, 0.0, batch, 0, True, 1.0)


def iscam_maps(model, images, classes=None, size=None, min_level=0.0, n_samples=10, batch=250):
    """uint8 IS-CAM heat maps [B, K, H, W] on the device: `iscam`, then the drawing steps of `scorecam_maps` in one launch
    (kernels.cam_maps) at `size` = (H, W) (None: the images' H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(iscam(model, images, classes, n_samples=n_samples, batch=batch), H, W, min_level)


CausalScores = collections.namedtuple("CausalScores", "deletion insertion deletion_curve insertion_curve step")
CausalScores.__doc__ = """The result of `causal_metrics`: deletion / insertion fp32 [B, K] (the areas under the curves; low deletion
and high insertion mean a good map), deletion_curve / insertion_curve fp32 [B, K, n_points] (the class probability at every
point), all on the images' device, and the `step` (pixels changed per point) that was used."""


def gaussian_taps(klen=11, sigma=5.0):
    """The blur of `causal_metrics` as fp32 taps [klen] (host): w[i] proportional to exp(-(i - klen // 2)^2 / (2 sigma^2)),
    normalised to sum 1 in float64 and rounded to fp32."""
    klen, sigma = int(klen), float(sigma)
    if klen < 1 or klen > 31 or klen % 2 == 0:
        raise ValueError("klen must be odd with 1 <= klen <= 31, got %d" % klen)
    if not sigma > 0.0:
        raise ValueError("sigma must be positive, got %r" % (sigma,))
    i = torch.arange(klen, dtype=torch.float64) - (klen // 2)
    w = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    return (w / w.sum()).to(torch.float32)


def slot_saliency(model):
    """The xSlot attention of the model's last forward as saliency maps, fp32 [B, num_classes, h, w] on the device:
    model.slot.last_attn with the slots of a class summed, as SlotAttention.vis_maps does, WITHOUT its min-max scaling to bytes
    (monotone: the ranks, and so `causal_metrics`, do not change).  RuntimeError when the model has no slot head (--use_slot
    false) or no forward has run yet."""
    slot = getattr(model, "slot", None)
    if slot is None or not getattr(model, "use_slot", True):
        raise RuntimeError("slot_saliency: the model has no slot head (use_slot is false)")
    a = slot.last_attn
    if a is None:
        raise RuntimeError("slot_saliency: no forward has run yet (model.slot.last_attn is None)")
    a = a.detach().float()
    if slot.slots_per_class > 1:
        a = a.reshape(a.shape[0], slot.num_classes, slot.slots_per_class, a.shape[-1]).sum(2)
    side = int(a.size(2) ** 0.5)
    return a.reshape(a.shape[0], a.shape[1], side, side).contiguous()


def slot_maps(model):
    """The uint8 slot maps of EVERY image of the model's last forward, [B, num_classes, h, w] on the device: `slot_saliency`
    with the maps of all classes of an image scaled jointly to bytes (kernels.group_maps: uint8((v - lo) / (hi - lo) * 255) in
    fp32 over the image's num_classes h w values) -- image i holds the bytes SlotAttention.vis_maps draws on the host with
    vis_id = i, the map the reference's attention_ratio (test.py:40-44) is taken from.  A constant image is all zeros."""
    return K.group_maps(slot_saliency(model))


LocalizationScores = collections.namedtuple("LocalizationScores", "area precision hit boxed empty sums")
LocalizationScores.__doc__ = """The result of `localization`, all on the maps' device: area / precision / hit float64 [B, K], boxed
bool [B] (the image has a box), empty bool [B, K] (the map is all zeros) and the integers they come from, sums int64 [B, K, 4] =
(S, S_in, arg, hit) of kernels.map_localization."""


def localization(maps, boxes=None, n_boxes=None):
    """Area size, precision and pointing game of uint8 `maps` [B, K, H, W] (what every *_maps function, kernels.cam_maps and
    kernels.heat_maps produce) against bounding boxes -> LocalizationScores.  The SCOUTER paper names the first two scores and no
    reference program computes precision or pointing, so this docstring is their specification.

    boxes int32 [B, max_boxes, 4] = (x0, y0, x1, y1), half-open pixel ranges of the map's own H x W grid, at most 32 an image;
    n_boxes int32 [B] says how many of an image's boxes count.  Both None: no image has a box.  A pixel is inside when it lies
    in any of its image's boxes -- a union, a pixel under two boxes counts once; boxes are clipped to the map, and a box with
    x1 <= x0 or y1 <= y0 holds nothing.  With S the sum of a map's bytes and S_in the sum of those inside:

    area = S / (255 H W): the reference's attention_ratio (test.py:40-44), for any map.
    precision = S_in / S, and 0 where S == 0 (`empty`): the share of the map's mass inside the boxes, taken on the BYTE map, not
        on the float map it was drawn from.
    hit = 1 when the map's largest byte -- the smallest flat index y W + x among equals -- lies inside, else 0: the STRICT
        pointing game; the customary 15-pixel tolerance is not applied.

    kernels.map_localization forms the integers exactly, one launch; the two ratios are float64 divisions of them on the device.
    An image without a box (`boxed` false) has precision and hit 0: a mean over a data set leaves it out (and the empty maps),
    as tools/explanation_table.py does.  Nothing is read on the host."""
    sums = K.map_localization(maps, boxes, n_boxes)
    H, W = maps.shape[-2:]
    S, S_in = sums[..., 0], sums[..., 1]
    empty = S == 0
    # (a tensor as the divisor: torch multiplies by the reciprocal of a Python scalar on the device, which is one rounding more)
    area = S.double() / torch.full_like(S, 255 * H * W).double()
    precision = torch.where(empty, torch.zeros_like(area), S_in.double() / torch.where(empty, torch.ones_like(S), S).double())
    boxed = (n_boxes > 0) if n_boxes is not None else torch.zeros(maps.shape[0], dtype=torch.bool, device=maps.device)
    return LocalizationScores(area, precision, sums[..., 3].double(), boxed, empty, sums)


def _num_outputs(model, images):
    """the number of model outputs: SlotModel's own count, or -- for any other module (the metric is black-box) -- the width of
    one eval-mode forward of the first image"""
    try:
        return _num_classes(model, images)
    except AttributeError:
        with _eval_mode(model), torch.no_grad():
            return int(model(images[:1].detach().float()).shape[1])


def causal_metrics(model, images, maps, classes=None, step=None, batch=250, klen=11, sigma=5.0):
    """Deletion and insertion scores (DAUC / IAUC; Petsiuk et al. 2018, section 4.1, the causal metrics the SCOUTER paper
    compares explanations with) of saliency `maps` [B, K, h, w] for `images` [B, C, H, W] -> CausalScores.

    Per image, class c and map m: the pixels are ordered by saliency, most salient first (equal values by ascending flat index
    y * W + x, -0.0 equal to +0.0, NaN after every number).  `step` pixels change per point (None: W, what the RISE authors'
    script uses at 224 x 224); a curve has n_points = ceil(H W / step) + 1 points and point j has the min(j step, H W)
    first-ranked pixels changed.  Deletion: the image with the changed pixels set to 0 in all channels.  Insertion: the blurred
    image with the changed pixels taken from the image.  p_j = exp(log_prob_j[c]) from the eval-mode output for point j, and the
    score is the trapezoid area over [0, 1], (p_0 / 2 + p_1 + ... + p_{n-1} + p_n / 2) / n with n = n_points - 1.  Low deletion
    and high insertion mean a good map.

    The blur is the plain sampled Gaussian: a separable filter of `klen` taps w[i] ~ exp(-(i - klen // 2)^2 / (2 sigma^2))
    (`gaussian_taps`: normalised in float64, rounded to fp32) along rows and then columns, zeros outside the image.  This
    DEPARTS from the RISE authors' script, which builds its 11 x 11 kernel by pushing a delta through scipy's reflecting
    gaussian_filter; scipy's border handling is not reproduced.  klen = 11 and sigma = 5 are that script's numbers.

    maps: fp32 or uint8 on the device (uint8 is converted to float; another dtype is a ValueError), resized to H x W with
    kernels.resize_bilinear when (h, w) != (H, W).  classes as in `gradcam` / `rise`: None -- map k belongs to class k and K must
    be the number of outputs; a list of K ints; a LongTensor [B] (each image its own class) with K = 1.

    Per image: kernels.saliency_ranks and kernels.separable_filter once, then the 2 K n_points edited images go through the model
    in chunks of `batch` that may start and end anywhere in the stream (every forward but the last runs at the full batch):
    kernels.causal_step_images into one reused buffer, the model under torch.no_grad() in eval mode (folded when the model's
    inference fold is on; the caller's mode is restored), kernels.causal_curve.  kernels.causal_auc at the end.  No BatchNorm
    buffer moves, no `.grad` appears, nothing is copied to the host and nothing synchronises inside the loop; two calls give
    the same bits."""
    B, C, H, W = _check_images(images).shape
    if not torch.is_tensor(maps) or maps.dim() != 4 or maps.shape[0] != B or maps.shape[1] < 1 or maps[0, 0].numel() < 1:
        raise ValueError("maps must be a tensor [B = %d, K, h, w], got %s"
                         % (B, tuple(maps.shape) if torch.is_tensor(maps) else type(maps).__name__))
    if maps.dtype not in (torch.float32, torch.uint8):
        raise ValueError("maps must be fp32 or uint8, got %s" % maps.dtype)
    Kc = int(maps.shape[1])
    n = _num_outputs(model, images)
    per_image, cols = _class_list(classes, B, n)
    if per_image and Kc != 1:
        raise ValueError("a tensor of classes (each image its own class) needs K = 1 map per image, got K = %d" % Kc)
    if not per_image and len(cols) != Kc:
        raise ValueError("%d maps per image for %d classes%s" % (Kc, len(cols), "" if classes is not None else
                                                               " (classes=None: one map per model output)"))
    _check_class_range(cols, n)
    x, batch = _check_images_batch(images, batch)
    step = W if step is None else int(step)
    if step < 1:
        raise ValueError("step must be at least 1, got %d" % step)
    if H * W > 1 << 20:
        raise ValueError("images of %d x %d pixels: the ranking covers at most 2^20" % (H, W))
    dev = images.device
    taps = gaussian_taps(klen, sigma).to(dev)
    n_points = -(-(H * W) // step) + 1
    total = 2 * Kc * n_points
    m = maps.detach().to(dev)
    m = (m.float() if m.dtype != torch.float32 else m).contiguous()
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    curves = torch.empty((B, Kc, 2, n_points), dtype=torch.float32, device=dev)
    buf = torch.empty((min(batch, total), C, H, W), dtype=torch.float32, device=dev)
    blurred = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    ranks = torch.empty((Kc, H * W), dtype=torch.int32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            mb = m[b] if tuple(m.shape[2:]) == (H, W) else K.resize_bilinear(m[b], H, W)
            K.saliency_ranks(mb.view(Kc, H * W), out=ranks)
            K.separable_filter(x[b], taps, out=blurred)
            for first in range(0, total, batch):
                chunk = K.causal_step_images(x[b], blurred, ranks, buf[:min(batch, total - first)], first, n_points, step)
                K.causal_curve(model(chunk), cb, curves[b], first, n_points)
    scores = K.causal_auc(curves)
    return CausalScores(scores[:, :, 0].contiguous(), scores[:, :, 1].contiguous(), curves[:, :, 0].contiguous(),
                        curves[:, :, 1].contiguous(), step)


def ig_quadrature(n_steps=50, method="gausslegendre"):
    """The nodes and weights of `integrated_gradients` on [0, 1] as fp32 CPU tensors (alphas [n_steps], weights [n_steps]), built
    in float64 and rounded once.  "gausslegendre": numpy.polynomial.legendre.leggauss(n_steps) mapped from [-1, 1] (captum's
    default); "riemann_trapezoid": linspace(0, 1, n_steps) with the end weights 1 / (2 (n - 1)) and the inner weights
    1 / (n - 1), n_steps >= 2."""
    n_steps = int(n_steps)
    if method not in ("gausslegendre", "riemann_trapezoid"):
        raise ValueError("method must be 'gausslegendre' or 'riemann_trapezoid', got %r" % (method,))
    if n_steps < 1 or (method == "riemann_trapezoid" and n_steps < 2):
        raise ValueError("n_steps must be at least %d for %s, got %d" % (2 if method == "riemann_trapezoid" else 1, method, n_steps))
    alphas, weights = _quadrature_fp32(n_steps, method)
    return torch.from_numpy(alphas.copy()), torch.from_numpy(weights.copy())


@functools.lru_cache(maxsize=32)
def _quadrature_fp32(n_steps, method):
    """the float64 tables of ig_quadrature rounded to fp32 (kept: leggauss solves an eigenproblem of size n_steps)"""
    if method == "gausslegendre":
        x, w = np.polynomial.legendre.leggauss(n_steps)
        alphas, weights = 0.5 * (x + 1.0), 0.5 * w
    else:
        alphas = np.linspace(0.0, 1.0, n_steps)
        weights = np.full(n_steps, 1.0 / (n_steps - 1))
        weights[0] = weights[-1] = 0.5 / (n_steps - 1)
    return alphas.astype(np.float32), weights.astype(np.float32)


def _class_list(classes, B, n):
    """the `classes` argument of every method -> (per_image, cols): None (every output), a list of ints, or a LongTensor [B]"""
    per_image = torch.is_tensor(classes)
    if per_image:
        if classes.dtype != torch.int64 or classes.dim() != 1 or classes.shape[0] != B:
            raise ValueError("a tensor of classes must be a LongTensor [B = %d], got %s %s"
                             % (B, classes.dtype, tuple(classes.shape)))
        return True, classes.detach().cpu().tolist()
    return False, [int(c) for c in (classes if classes is not None else range(n))]


def _check_class_range(cols, n):
    for c in cols:
        if not 0 <= c < n:
            raise IndexError("class %d out of range (the model has %d outputs)" % (c, n))


def _class_columns(classes, B, n):
    """_class_list with every column checked against the model's n outputs"""
    per_image, cols = _class_list(classes, B, n)
    _check_class_range(cols, n)
    return per_image, cols


def _chunk_gradient(model, chunk, seed):
    """d sum(out * seed) / d chunk for a batch that lives in the reused buffer: the chunk becomes a leaf (no copy), one eval
    forward, one backward with the leading rows of the one-hot `seed` [batch, n_outputs]"""
    x = chunk.detach().requires_grad_(True)
    g = torch.autograd.grad(model(x), x, seed[:x.shape[0]])[0]
    return g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()


def _path_method(model, images, n, per_image, cols, batch, N, fill, weights, want_sq, finish, totals=None, accumulate=None,
                 route="autograd"):
    """the loop shared by integrated_gradients, smoothgrad and gradient_shap: image, then class, then chunk.  (per_image, cols)
    come from _class_columns for a model of n outputs; fill(b, buf, first) writes the images first .. first + len(buf) - 1 of
    image b's batch of N into buf; finish(b, acc, acc_sq, out, total) forms out[b, k].  accumulate(b, grads, acc, first), when
    given, adds a chunk's gradients in place of kernels.grad_accumulate with `weights`.
    route="folded": the second loop order, image, then chunk, then class -- the rows of a chunk do not depend on the class, so ONE
    fill and ONE model.image_pass serve every class of the chunk; per class one .grad and one accumulate onto that class's own
    float64 sums (acc / acc_sq [K, C, H, W]), `finish` per class at the end.  Per class the chunks still arrive in ascending
    order, so the chunking changes no bit."""
    B, C, H, W = images.shape
    dev = images.device
    Kc = 1 if per_image else len(cols)
    out = torch.empty((B, Kc, C, H, W), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    if route == "folded":
        buf = torch.empty((min(batch, N), C, H, W), dtype=torch.float32, device=dev)
        seed = torch.zeros((min(batch, N), n), dtype=torch.float32, device=dev)
        acc = torch.empty((Kc, C, H, W), dtype=torch.float64, device=dev)
        acc_sq = torch.empty_like(acc) if want_sq else None
        with _eval_mode_once(model), torch.no_grad():
            for b in range(B):
                cb = cols[b:b + 1] if per_image else cols
                acc.zero_()
                if want_sq:
                    acc_sq.zero_()
                for first in range(0, N, batch):
                    chunk = fill(b, buf[:min(batch, N - first)], first)
                    ip = model.image_pass(chunk)
                    rows = seed[:chunk.shape[0]]
                    for k, c in enumerate(cb):
                        rows.zero_()
                        rows[:, c] = 1.0
                        grads = ip.grad(rows)
                        if accumulate is None:
                            K.grad_accumulate(grads, weights, acc[k], None if acc_sq is None else acc_sq[k], first)
                        else:
                            accumulate(b, grads, acc[k], first)
                for k in range(len(cb)):
                    finish(b, acc[k], None if acc_sq is None else acc_sq[k], out[b, k],
                           None if totals is None else totals[b, k:k + 1])
        return out
    buf = torch.empty((min(batch, N), C, H, W), dtype=torch.float32, device=dev)
    seed = torch.zeros((min(batch, N), n), dtype=torch.float32, device=dev)
    acc = torch.empty((C, H, W), dtype=torch.float64, device=dev)
    acc_sq = torch.empty_like(acc) if want_sq else None
    with _eval_mode(model), torch.enable_grad():
        for b in range(B):
            for k, c in enumerate(cols[b:b + 1] if per_image else cols):
                acc.zero_()
                if want_sq:
                    acc_sq.zero_()
                seed.zero_()
                seed[:, c] = 1.0
                for first in range(0, N, batch):
                    chunk = fill(b, buf[:min(batch, N - first)], first)
                    grads = _chunk_gradient(model, chunk, seed)
                    if accumulate is None:
                        K.grad_accumulate(grads, weights, acc, acc_sq, first)
                    else:
                        accumulate(b, grads, acc, first)
                finish(b, acc, acc_sq, out[b, k], None if totals is None else totals[b, k:k + 1])
    return out


def _check_images(images):
    if images.dim() != 4:
        raise ValueError("images must be [B, C, H, W], got shape %s" % (tuple(images.shape),))
    return images


def _out_size(size, images):
    """the `size` = (H, W) argument of the *_maps functions as two ints; None: the images' H x W"""
    H, W = (int(v) for v in (size if size is not None else images.shape[-2:]))
    return H, W


def _check_images_batch(images, batch):
    """images [B, C, H, W] and the chunk length of a batched method -> (the images detached, contiguous and fp32, int(batch))"""
    _check_images(images)
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1, got %d" % batch)
    x = images.detach().contiguous()
    return (x.float() if x.dtype != torch.float32 else x), batch


def integrated_gradients(model, images, classes=None, baseline=None, n_steps=50, method="gausslegendre", batch=50,
                         return_delta=False):
    """Integrated Gradients (Sundararajan et al., ICML 2017; captum's IntegratedGradients) of `images` [B, C, H, W] -> fp32
    [B, K, C, H, W] on the images' device:
    attr[b, k] = (x_b - x'_b) * sum_i w_i * d out[:, c_k] / dx at x'_b + alpha_i (x_b - x'_b),
    out the eval-mode model output as in input_gradients(of="log_prob"), (alpha_i, w_i) = ig_quadrature(n_steps, method) (built
    on the host in float64, rounded to fp32, uploaded once) and x' the `baseline`: None (zeros), [C, H, W] (one for the batch) or
    [B, C, H, W].  classes as in `gradcam` / `rise`: None (every output), a list of ints (K = len), or a LongTensor [B] (each
    image its own class, K = 1).

    Per image and class the n_steps path images go through the model in chunks of `batch` (the last may be shorter):
    kernels.path_images into one reused buffer, which becomes the leaf of an eval-mode forward (the caller's mode is restored)
    and of one backward with a one-hot column, kernels.grad_accumulate onto float64 sums in step order -- the chunking does not
    change a bit -- and kernels.attr_finish at the end of the class.  return_delta=True: also `delta` fp32 [B, K] =
    sum(attr[b, k]) - (out(x_b)[c_k] - out(x'_b)[c_k]), the completeness gap, from the float64 sum of attr_finish and one extra
    no_grad forward of [x'_b, x_b] per image.  No BatchNorm buffer moves, nothing is copied to the host and nothing synchronises
    inside the loop; parameters that require grad get their `.grad` overwritten by each backward, as in `input_gradients`.  Any
    module whose eval forward returns [n, n_outputs] will do.  `integrated_gradients_by_route` is this method with one more
    option, the route its gradients take."""
    return integrated_gradients_by_route(model, images, classes=classes, baseline=baseline, n_steps=n_steps, method=method,
                                         batch=batch, return_delta=return_delta, route="autograd")


def integrated_gradients_by_route(model, images, classes=None, baseline=None, n_steps=50, method="gausslegendre", batch=50,
                                  return_delta=False, route="autograd"):
    """`integrated_gradients` with the option `route` (that function keeps the parameter list its callers know):
    route="autograd" is `integrated_gradients`, the same code and the same bits.  route="folded" (a SlotModel in fp32): the chunks
    go through model.image_pass -- ONE forward of a chunk on the BatchNorm-folded weights serves every class, each class one
    gradient-only backward (the loop order image, chunk, class of _path_method); the chunking still changes no bit, return_delta
    and everything downstream are the same.  Any other value is a ValueError before any launch."""
    _check_route(route)
    x, batch = _check_images_batch(images, batch)
    if route == "folded":
        _check_device_images(x)
    B, C, H, W = x.shape
    alphas, weights = ig_quadrature(n_steps, method)
    dev = x.device
    if baseline is not None:
        if not torch.is_tensor(baseline) or tuple(baseline.shape) not in ((C, H, W), (B, C, H, W)):
            raise ValueError("baseline must be None, [%d, %d, %d] or [%d, %d, %d, %d], got %s"
                             % (C, H, W, B, C, H, W, tuple(baseline.shape) if torch.is_tensor(baseline) else type(baseline).__name__))
        baseline = baseline.detach().to(dev, dtype=torch.float32).contiguous()
    alphas, weights = alphas.to(dev), weights.to(dev)

    def base_of(b):
        return None if baseline is None else baseline if baseline.dim() == 3 else baseline[b]

    def fill(b, buf, first):
        return K.path_images(x[b], base_of(b), alphas, buf, first)

    def finish(b, acc, acc_sq, out, total):
        K.attr_finish(K.ATTR_IG, acc, image=x[b], base=base_of(b), out=out, total=total)

    n = _num_outputs(model, x)
    per_image, cols = _class_columns(classes, B, n)
    Kc = 1 if per_image else len(cols)
    totals = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    attr = _path_method(model, x, n, per_image, cols, batch, int(alphas.shape[0]), fill, weights, False, finish, totals,
                        route=route)
    if not return_delta:
        return attr
    delta = torch.zeros((B, Kc), dtype=torch.float32, device=dev)
    if Kc:
        with _eval_mode(model), torch.no_grad():
            for b in range(B):
                base = base_of(b)
                ends = model(torch.stack([torch.zeros_like(x[b]) if base is None else base, x[b]])).double()
                cb = cols[b:b + 1] if per_image else cols
                delta[b] = (totals[b] - (ends[1, cb] - ends[0, cb])).float()
    return attr, delta


_SMOOTHGRAD_KINDS = {"smoothgrad": K.ATTR_MEAN, "smoothgrad_sq": K.ATTR_MEAN_SQ, "vargrad": K.ATTR_VAR}


def smoothgrad(model, images, classes=None, n_samples=50, sigma=1.0, kind="smoothgrad", batch=50, seed=0):
    """SmoothGrad (Smilkov et al. 2017; captum's NoiseTunnel over Saliency with stdevs = sigma) of `images` [B, C, H, W] -> fp32
    [B, K, C, H, W] on the images' device, from the gradients g_s = d out[:, c_k] / dx at x_b + sigma * z_s, s < n_samples, out
    the eval-mode model output as in input_gradients(of="log_prob"): kind "smoothgrad" is their mean, "smoothgrad_sq" the mean
    of their squares, "vargrad" their biased variance (mean of squares minus squared mean).  z_s is standard normal, a function
    of (seed, s, element) alone (kernels.noise_images): sample s of every image and class uses the same noise, and the same
    seed repeats bit for bit.  sigma is absolute (>= 0), not relative to the image's range.  classes as in `gradcam` / `rise`.

    The loop is that of `integrated_gradients`: kernels.noise_images into one reused buffer in chunks of `batch`, an eval-mode
    forward and one backward with a one-hot column, kernels.grad_accumulate onto float64 sums in sample order,
    kernels.attr_finish at the end of the class, with the same guarantees -- no BatchNorm buffer moves, the caller's mode is
    restored, nothing is copied to the host or synchronises inside the loop, `.grad` of parameters that require grad is
    overwritten.  `smoothgrad_by_route` is this method with one more option, the route its gradients take."""
    return smoothgrad_by_route(model, images, classes=classes, n_samples=n_samples, sigma=sigma, kind=kind, batch=batch, seed=seed,
                               route="autograd")


def smoothgrad_by_route(model, images, classes=None, n_samples=50, sigma=1.0, kind="smoothgrad", batch=50, seed=0, route="autograd"):
    """`smoothgrad` with the option `route` (that function keeps the parameter list its callers know): route="autograd" is
    `smoothgrad`, the same code and the same bits; route="folded": as in `integrated_gradients_by_route` -- one folded forward of
    a chunk for every class.  Any other value is a ValueError before any launch."""
    _check_route(route)
    x, batch = _check_images_batch(images, batch)
    if route == "folded":
        _check_device_images(x)
    n_samples, sigma = int(n_samples), float(sigma)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    if not 0.0 <= sigma < float("inf"):
        raise ValueError("sigma must be finite and not negative, got %r" % (sigma,))
    if kind not in _SMOOTHGRAD_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(_SMOOTHGRAD_KINDS), kind))
    mode = _SMOOTHGRAD_KINDS[kind]

    def fill(b, buf, first):
        return K.noise_images(x[b], buf, sigma, seed, first)

    def finish(b, acc, acc_sq, out, total):
        K.attr_finish(mode, acc, acc_sq, inv_n=1.0 / n_samples, out=out)

    n = _num_outputs(model, x)
    per_image, cols = _class_columns(classes, x.shape[0], n)
    return _path_method(model, x, n, per_image, cols, batch, n_samples, fill, None, mode != K.ATTR_MEAN, finish, route=route)


def gradient_maps(attr, min_level=0.0, absolute=False):
    """[B, K, C, H, W] attributions on the device -> uint8 maps [B, K, H, W] on the device, the device counterpart of
    `attribution_maps`: the mean over the channels (absolute: of the magnitudes; kernels.channel_mean), then the drawing steps of
    kernels.heat_maps -- negative values cut to 0, min-max scaled, raised to at least `min_level`, min-max scaled again, times
    255.  A map that is constant at either scaling step is all zeros."""
    if not torch.is_tensor(attr) or attr.dim() != 5:
        raise ValueError("attr must be a tensor [B, K, C, H, W], got %s"
                         % (tuple(attr.shape) if torch.is_tensor(attr) else type(attr).__name__,))
    return K.heat_maps(K.channel_mean(attr.detach().contiguous(), absolute=absolute), min_level)


InfidelityScores = collections.namedtuple("InfidelityScores", "raw normalized beta dots deltas")
InfidelityScores.__doc__ = """The result of `infidelity`, float64 on the images' device: raw / normalized / beta [B, K] (low
infidelity means a faithful attribution; `normalized` is the one that means something for maps of arbitrary scale, `beta` the
scale it chose), and the per-sample dots / deltas [B, K, N] they were summed from."""

SensitivityScores = collections.namedtuple("SensitivityScores", "score terms")
SensitivityScores.__doc__ = """The result of `sensitivity_max`, float64 on the images' device: score [B, K] (the largest relative
change of the explanation; low means a stable explanation) and the per-sample terms [B, K, N]."""


def _check_samples(n_samples, spread, name, batch):
    n_samples, spread = int(n_samples), float(spread)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    if not 0.0 <= spread < float("inf"):
        raise ValueError("%s must be finite and not negative, got %r" % (name, spread))
    if batch < 2:
        raise ValueError("batch must be at least 2 (the clean image and one sample), got %d" % batch)
    return n_samples, spread


def infidelity(model, images, attributions, classes=None, n_samples=50, sigma=0.003, batch=50, seed=0, of="log_prob"):
    """Infidelity (Yeh et al., NeurIPS 2019; captum.metrics.infidelity with additive Gaussian noise) of `attributions` for
    `images` [B, C, H, W] -> InfidelityScores, float64 on the device.  Per image x, attribution a_k and class c_k, with E = C H W:

    noise        z_j[e], j < N = n_samples: the standard normal of kernels.noise_images for (seed, j, e); the perturbed image
                 x_j = fma(sigma, z_j, x) is written by that kernel.
    perturbation I_j[e] = -sigma z_j[e], the exact product (x - x_j up to the one rounding of the fma, not re-derived from x_j).
    dots         dot[k, j] = sum_e a_k[e] I_j[e] in float64 (kernels.perturb_dots, which regenerates z).
    deltas       delta[k, j] = F(out[0, c_k]) - F(out[1 + i, c_k]) in float64 from the fp32 eval-mode output of the forward that
                 carried sample j in row 1 + i and the clean image in row 0 -- both sides of the difference come from the same
                 kernel instances.  of="log_prob": F is the identity, the quantity `input_gradients` differentiates; of="prob":
                 F = exp.
    scores       raw = mean_j (dot - delta)^2, beta = sum_j dot delta / sum_j dot^2 (0 when the denominator is 0),
                 normalized = mean_j (beta dot - delta)^2 -- captum's normalize=True, the only form that means anything for CAM,
                 RISE and slot maps, whose scale is arbitrary.  Summed in ascending j (kernels.infidelity_finish).

    attributions: [B, K, C, H, W] fp32, the full form (`input_gradients`, `integrated_gradients`, `smoothgrad`), or maps
    [B, K, h, w], fp32 or uint8, that count for every channel (a_k[e] = m_k[e mod H W]); maps are resized with
    kernels.resize_bilinear when (h, w) != (H, W), as in `causal_metrics`.  classes as in `causal_metrics`: None -- attribution k
    belongs to class k and K must be the number of outputs; a list of K ints; a LongTensor [B] (each image its own class) with
    K = 1.  `batch` is the number of rows per forward, the clean row included (at least 2).

    Per image: row 0 of one reused buffer is written once; then chunks of up to batch - 1 samples: kernels.noise_images into the
    rows behind it, the model under torch.no_grad() in eval mode (folded when the model's inference fold is on; the caller's
    mode is restored), kernels.output_deltas and kernels.perturb_dots.  kernels.infidelity_finish once at the end.  No BatchNorm
    buffer moves, no `.grad` appears, nothing is copied to the host and nothing synchronises inside the loop; two calls give the
    same bits, and `dots` has the same bits for every `batch`.  Any module whose eval forward returns [n, n_outputs] will do.

    The defaults n_samples = 50 and sigma = 0.003 are remembered from captum's infidelity tutorial and could not be checked when
    this was written; they are parameters and nothing else depends on them."""
    if of not in ("log_prob", "prob"):
        raise ValueError("of must be 'log_prob' or 'prob', got %r" % (of,))
    B, C, H, W = _check_images(images).shape
    x, batch = _check_images_batch(images, batch)
    N, sigma = _check_samples(n_samples, sigma, "sigma", batch)
    a = attributions
    if not torch.is_tensor(a) or a.dim() not in (4, 5) or a.shape[0] != B or a.shape[1] < 1 or a[0, 0].numel() < 1:
        raise ValueError("attributions must be a tensor [B = %d, K, h, w] or [B, K, %d, %d, %d], got %s"
                         % (B, C, H, W, tuple(a.shape) if torch.is_tensor(a) else type(a).__name__))
    full = a.dim() == 5
    if full and (a.dtype != torch.float32 or tuple(a.shape[2:]) != (C, H, W)):
        raise ValueError("full attributions must be fp32 [B, K, %d, %d, %d], got %s %s" % (C, H, W, a.dtype, tuple(a.shape)))
    if not full and a.dtype not in (torch.float32, torch.uint8):
        raise ValueError("attribution maps must be fp32 or uint8, got %s" % a.dtype)
    Kc = int(a.shape[1])
    n = _num_outputs(model, images)
    per_image, cols = _class_list(classes, B, n)
    if per_image and Kc != 1:
        raise ValueError("a tensor of classes (each image its own class) needs K = 1 attribution per image, got K = %d" % Kc)
    if not per_image and len(cols) != Kc:
        raise ValueError("%d attributions per image for %d classes%s" % (Kc, len(cols), "" if classes is not None else
                                                                       " (classes=None: one attribution per model output)"))
    _check_class_range(cols, n)
    dev = images.device
    a = a.detach().to(dev)
    a = (a.float() if a.dtype != torch.float32 else a).contiguous()
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    dots = torch.empty((B, Kc, N), dtype=torch.float64, device=dev)
    deltas = torch.empty_like(dots)
    buf = torch.empty((min(batch, N + 1), C, H, W), dtype=torch.float32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            ab = a[b] if full or tuple(a.shape[2:]) == (H, W) else K.resize_bilinear(a[b], H, W)
            buf[0].copy_(x[b])
            for first in range(0, N, batch - 1):
                m = min(batch - 1, N - first)
                K.noise_images(x[b], buf[1:1 + m], sigma, seed, first)
                out = model(buf[:1 + m])
                out = out if out.dtype == torch.float32 and out.is_contiguous() else out.float().contiguous()
                K.output_deltas(out, cb, deltas[b], first, of)
                K.perturb_dots(ab, dots[b], sigma, seed, first, m, channels=C)
    raw, normalized, beta = K.infidelity_finish(dots, deltas)
    return InfidelityScores(raw, normalized, beta, dots, deltas)


def sensitivity_max(explain, images, n_samples=10, radius=0.02, batch=11, seed=0):
    """Max-sensitivity (Yeh et al., NeurIPS 2019; captum.metrics.sensitivity_max) of the explanation method `explain` at `images`
    [B, C, H, W] -> SensitivityScores, float64 on the device.  Per image x:

    perturbation d_j[e] = 2 u - 1, j < N = n_samples, uniform on (-1, 1) and never 0, from the Philox stream beside the noise of
                 `smoothgrad` / `infidelity` (kernels.uniform_images: a value per (seed, j, e)); x_j = fma(radius, d_j, x), a point
                 of the box of half-width `radius` around x.
    explanations explain(images [n, C, H, W] on the device) -> an fp32 device tensor [n, K, ...] with M elements per map; every
                 call carries the clean image in row 0 and perturbed samples in the rows behind it.
    terms        term[k, j] = sqrt(sum_m (A_j[k, m] - A_0[k, m])^2 / den_k), den_k = sum_m A_0[k, m]^2, or 1 when that is 0
                 (captum's choice for a zero explanation); float64, A_0 from the same call as A_j (kernels.map_distances).
    score        score[k] = max_j term[k, j], NaN if any term is NaN (kernels.sensitivity_finish).

    `explain` is any callable; for the families of this module, with a class list `cs` (a LongTensor of per-image classes would
    have to follow the batch it is given):
        grad         lambda im: input_gradients(model, im, classes=cs)
        cam          lambda im: gradcam(model, im, classes=cs)
        campp        lambda im: gradcampp(model, im, classes=cs)
        smoothcampp  lambda im: smooth_gradcampp(model, im, classes=cs)
        rise         lambda im: rise(model, im, classes=cs, masks=masks)
        scorecam     lambda im: scorecam(model, im, classes=cs)
        ig           lambda im: integrated_gradients(model, im, classes=cs)
        smoothgrad   lambda im: smoothgrad(model, im, classes=cs)
        iba          lambda im: information_bottleneck(model, im, estimate, classes=cs)
        slot       lambda im: (model(im), slot_saliency(model)[:, cs].contiguous())[1]        (model in eval mode, no_grad)
    `batch` is the number of rows per call, the clean row included (at least 2).  Per image: row 0 of one reused buffer is
    written once, then chunks of up to batch - 1 samples: kernels.uniform_images into the rows behind it, explain, and
    kernels.map_distances.  A result that is not an fp32 device tensor [n, K, ...], or whose shape behind the first dimension
    changes between calls, raises ValueError.  Nothing is copied to the host and nothing synchronises here; what `explain` does
    to the model (its mode, `.grad`) is its own.

    The defaults n_samples = 10 and radius = 0.02 are remembered from captum's sensitivity_max and could not be checked when this
    was written; they are parameters and nothing else depends on them."""
    if not callable(explain):
        raise ValueError("explain must be callable: images [n, C, H, W] -> explanations [n, K, ...]")
    x, batch = _check_images_batch(images, batch)
    B, C, H, W = x.shape
    N, radius = _check_samples(n_samples, radius, "radius", batch)
    dev = x.device
    buf = torch.empty((min(batch, N + 1), C, H, W), dtype=torch.float32, device=dev)
    terms, shape = None, None
    for b in range(B):
        buf[0].copy_(x[b])
        for first in range(0, N, batch - 1):
            m = min(batch - 1, N - first)
            K.uniform_images(x[b], buf[1:1 + m], radius, seed, first)
            maps = explain(buf[:1 + m])
            if not torch.is_tensor(maps) or maps.dtype != torch.float32 or not maps.is_cuda or maps.dim() < 2 or \
                    maps.shape[0] != 1 + m or maps.shape[1] < 1 or maps[0, 0].numel() < 1:
                raise ValueError("explain must return an fp32 device tensor [n = %d, K, ...], got %s"
                                 % (1 + m, "%s %s" % (maps.dtype, tuple(maps.shape)) if torch.is_tensor(maps)
                                    else type(maps).__name__))
            if shape is None:
                shape = tuple(maps.shape[1:])
                terms = torch.empty((B, shape[0], N), dtype=torch.float64, device=dev)
            elif tuple(maps.shape[1:]) != shape:
                raise ValueError("explain returned maps of shape %s after %s: the shape of an explanation must not change"
                                 % (tuple(maps.shape[1:]), shape))
            K.map_distances(maps.detach().contiguous(), terms[b], first)
    return SensitivityScores(K.sensitivity_finish(terms), terms)


ExtremalMasks = collections.namedtuple("ExtremalMasks", "masks pmasks rewards")
ExtremalMasks.__doc__ = """The result of `extremal_perturbation`, fp32 on the images' device: masks [B, K, A, H, W] in [0, 1] (the
smooth-max upsampling of the final coarse masks), pmasks [B, K, A, hm, wm] (the coarse masks themselves) and rewards
[B, K, A, n_iters] (the class probability of the perturbed image at every iteration, before that iteration's update)."""


def pyramid_pass_plan(levels=8, max_blur=20.0):
    """The blur passes of `perturbation_pyramid` (host arithmetic only): a list of levels - 1 entries, entry l for level l, each
    (passes, sd, klen).  Level l has sigma_l = max_blur (1 - l / (levels - 1)) and comes from level l + 1 by the variance
    increment sigma_l^2 - sigma_{l+1}^2, split into passes = ceil(increment / 25) equal Gaussian passes of standard deviation
    sd = sqrt(increment / passes) <= 5 with klen = 2 ceil(3 sd) + 1 <= 31 taps -- 19 passes at the defaults."""
    levels, max_blur = int(levels), float(max_blur)
    if levels < 2:
        raise ValueError("levels must be at least 2, got %d" % levels)
    if not 0.0 < max_blur < float("inf"):
        raise ValueError("max_blur must be positive and finite, got %r" % (max_blur,))
    plan = []
    for l in range(levels - 1):
        hi, lo = max_blur * (1.0 - l / (levels - 1.0)), max_blur * (1.0 - (l + 1) / (levels - 1.0))
        inc = hi * hi - lo * lo
        passes = max(1, int(np.ceil(inc / 25.0)))
        sd = float(np.sqrt(inc / passes))
        plan.append((passes, sd, 2 * int(np.ceil(3.0 * sd)) + 1))
    return plan


def perturbation_pyramid(image, levels=8, max_blur=20.0):
    """The blur pyramid of Extremal Perturbation for ONE `image` [C, H, W] -> fp32 [levels, C, H, W] on its device: level
    levels - 1 is the image and level l the image blurred to sigma_l = max_blur (1 - l / (levels - 1)), so level 0 carries
    max_blur.  Built with kernels.separable_filter alone, downwards: level l is level l + 1 after the passes of
    `pyramid_pass_plan` (variances add), each with the taps of `gaussian_taps(klen, sd)`.  Zeros outside the image, as in
    `causal_metrics`: this DEPARTS from TorchRay, whose Gaussian blur pads by replication, so the borders of the blurred levels
    are darker here."""
    if not torch.is_tensor(image) or image.dim() != 3:
        raise ValueError("image must be a tensor [C, H, W], got %s"
                         % (tuple(image.shape) if torch.is_tensor(image) else type(image).__name__,))
    plan = pyramid_pass_plan(levels, max_blur)
    x = image.detach().contiguous()
    x = x.float() if x.dtype != torch.float32 else x
    L = len(plan) + 1
    pyr = torch.empty((L,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    pyr[L - 1].copy_(x)
    tmp = torch.empty_like(x) if any(p[0] > 1 for p in plan) else None
    for l in range(L - 2, -1, -1):
        passes, sd, klen = plan[l]
        taps = gaussian_taps(klen, sd).to(x.device)
        src = pyr[l + 1]
        for i in range(passes):
            dst = pyr[l] if (passes - 1 - i) % 2 == 0 else tmp            # (the last pass lands in the level)
            K.separable_filter(src, taps, out=dst)
            src = dst
    return pyr


def extremal_schedule(n_iters, area_weight=300.0, area_growth=1.0035):
    """lambda_it = area_weight * area_growth^it for it < n_iters, formed in float64 on the host (a list of floats); each is handed
    to kernels.extremal_mask_grad as an fp32 scalar."""
    return [float(area_weight) * float(area_growth) ** it for it in range(int(n_iters))]


def _extremal_area_pixels(areas, HW):
    """the areas of `extremal_perturbation` as pixel counts A = floor(a H W + 0.5), each inside [1, H W - 1]"""
    try:
        areas = [float(a) for a in areas]
    except TypeError:
        raise ValueError("areas must be a sequence of fractions of the image, got %r" % (areas,))
    if not areas:
        raise ValueError("areas must name at least one area")
    counts = []
    for a in areas:
        A = int(np.floor(a * HW + 0.5)) if a == a and abs(a) < float("inf") else -1
        if not 1 <= A <= HW - 1:
            raise ValueError("area %r of %d pixels is %d pixels: an area must cover between 1 and H W - 1 pixels" % (a, HW, A))
        counts.append(A)
    return counts


def extremal_perturbation(model, images, classes=None, areas=(0.1,), n_iters=800, step=7, sigma=21.0, levels=8, max_blur=20.0,
                          variant="preserve", lr=0.01, momentum=0.9, area_weight=300.0, area_growth=1.0035, jitter=True, batch=50,
                          init=None):
    """Extremal Perturbation (Fong, Patrick, Vedaldi, ICCV 2019; torchray.attribution.extremal_perturbation, which the reference's
    torchcam_vis.py runs after RISE) of `images` [B, C, H, W] -> ExtremalMasks: for every image, class c_k and area a, the smooth
    mask of area a H W whose perturbed image keeps ("preserve") or loses ("delete") the most probability of class c_k, found by
    n_iters steps of SGD.  No reference program runs here; this docstring (and include/scouter_hip.h) is the specification.

    mask         a coarse mask p [hm, wm] in [0, 1], hm = ceil(H / step), wm = ceil(W / step), starts at 0.5 (or `init`) and is
                 upsampled by kernels.extremal_mask: cell (i, j) sits at pixel ((i + 0.5) step - 0.5, (j + 0.5) step - 0.5), a pixel
                 sees the (2 r + 1)^2 cells around its own, r = 1 + ceil(sigma / step), v_c = k(|u - centre_c| / sigma) p_c with
                 k(z) = exp(-2 max(z - 0.5, 0)^2) (0 for a cell outside the grid) and m(u) = sum_c v_c softmax_c(20 v).
    perturbation `perturbation_pyramid(image, levels, max_blur)` P [L, C, H, W]; m' = m ("preserve") or 1 - m ("delete"),
                 t = m' (L - 1), k = min(floor(t), L - 2), w = t - k, x~ = (1 - w) P[k] + w P[k + 1] (kernels.extremal_blend).  With
                 `jitter`, odd iterations hand the model the horizontally mirrored x~ and mirror the gradient back.
    objective    p = exp(log_prob[c_k]) of the eval-mode output for x~ (recorded in `rewards`); loss = -p (preserve) or +p
                 (delete) + lambda_it mean_q (m(q) - tau(q))^2, tau = 1 for the A = floor(a H W + 0.5) pixels
                 kernels.saliency_ranks(m) ranks first (most salient first, ties by ascending index) and 0 for the rest -- the
                 value of TorchRay's |sort(m) - template|^2 whatever the tie order; lambda_it = `extremal_schedule`.
    update       g = d loss / d p (kernels.extremal_mask_grad, kernels.extremal_step); buf = g at the first iteration, then
                 momentum buf + (1 - momentum) g (SGD with dampening = momentum); p = clamp(p - lr buf, 0, 1).

    classes as in `gradcam`: None (every output), a list of ints (K = len), or a LongTensor [B] (each image its own class,
    K = 1).  areas: fractions of the image, each with 1 <= A <= H W - 1.  init: None, fp32 [hm, wm] (every mask) or
    [B, K, A, hm, wm].  Per image the K A masks form one batch, split into groups of at most `batch` rows; masks are independent,
    so the grouping does not change a bit.  Every group runs the whole loop, per iteration: kernels.extremal_mask,
    kernels.extremal_blend into one reused buffer, which becomes the leaf of an eval-mode forward and of one backward whose seed
    kernels.extremal_seed writes from the output itself, kernels.saliency_ranks, kernels.extremal_mask_grad,
    kernels.extremal_step.  The model is in eval mode (no BatchNorm buffer moves; the caller's mode is restored) and runs its
    plain eval backward, as in `integrated_gradients` -- the inference fold is not involved; SlotModel's backward overwrites
    the `.grad` of its parameters that require grad, as in any backward of it, while a plain torch module, differentiated by
    torch.autograd.grad with respect to the input alone, has no `.grad` touched.  Nothing is copied to the host and nothing synchronises inside the loop; two calls give the same
    bits.  Any module whose eval forward returns log-probabilities [n, n_outputs] and is differentiable to its input will do.

    This DEPARTS from TorchRay in what it leaves out -- the `dual` variant, the contrastive reward, the `resize` / `smooth`
    post-processing and the `margin` offset of the upsampler's grid -- in the zero padding of the blur (`perturbation_pyramid`),
    and in the pyramid's piecewise-linear blend being differentiated by its right-hand piece at a knot."""
    if variant not in ("preserve", "delete"):
        raise ValueError("variant must be 'preserve' or 'delete', got %r" % (variant,))
    n_iters, step, levels = int(n_iters), int(step), int(levels)
    if n_iters < 1:
        raise ValueError("n_iters must be at least 1, got %d" % n_iters)
    if step < 1 or not 0.0 < float(sigma) < float("inf"):
        raise ValueError("step must be at least 1 and sigma positive and finite, got %d and %r" % (step, sigma))
    pyramid_pass_plan(levels, max_blur)                                      # (levels < 2: ValueError)
    if not (0.0 <= float(lr) < float("inf") and 0.0 <= float(momentum) <= 1.0):
        raise ValueError("lr must be finite and not negative and 0 <= momentum <= 1, got %r and %r" % (lr, momentum))
    x, batch = _check_images_batch(images, batch)
    B, C, H, W = x.shape
    if H * W > 1 << 20:
        raise ValueError("images of %d x %d pixels: the ranking covers at most 2^20" % (H, W))
    counts = _extremal_area_pixels(areas, H * W)
    hm, wm, _ = K.extremal_grid(H, W, step, sigma)
    if init is not None:
        if not torch.is_tensor(init) or not (tuple(init.shape) == (hm, wm) or
                                             (init.dim() == 5 and tuple(init.shape[3:]) == (hm, wm) and init.shape[0] == B)):
            raise ValueError("init must be None, [%d, %d] or [B = %d, K, A, %d, %d], got %s"
                             % (hm, wm, B, hm, wm, tuple(init.shape) if torch.is_tensor(init) else type(init).__name__))
    lams = extremal_schedule(n_iters, area_weight, area_growth)
    n_out = _num_outputs(model, x)
    per_image, cols = _class_columns(classes, B, n_out)
    Kc, A = (1 if per_image else len(cols)), len(counts)
    if init is not None and init.dim() == 5 and tuple(init.shape[:3]) != (B, Kc, A):
        raise ValueError("init must be None, [%d, %d] or [B = %d, K = %d, A = %d, %d, %d], got %s"
                         % (hm, wm, B, Kc, A, hm, wm, tuple(init.shape)))
    dev = x.device
    pmasks = torch.full((B, Kc * A, hm, wm), 0.5, dtype=torch.float32, device=dev)
    if init is not None:
        pmasks.copy_(init.detach().to(dev, dtype=torch.float32).reshape((-1, Kc * A, hm, wm) if init.dim() == 5 else (1, 1, hm, wm))
                     .expand(B, Kc * A, hm, wm))
    masks = torch.empty((B, Kc * A, H, W), dtype=torch.float32, device=dev)
    rewards = torch.empty((B, Kc * A, n_iters), dtype=torch.float32, device=dev)
    R = Kc * A
    if R == 0:
        return ExtremalMasks(masks.view(B, Kc, A, H, W), pmasks.view(B, Kc, A, hm, wm), rewards.view(B, Kc, A, n_iters))
    rows = min(batch, R)
    buf = torch.empty((rows, C, H, W), dtype=torch.float32, device=dev)
    seed = torch.empty((rows, n_out), dtype=torch.float32, device=dev)
    mask = torch.empty((rows, H, W), dtype=torch.float32, device=dev)
    dmask = torch.empty_like(mask)
    stats = torch.empty((rows, H, W, 2), dtype=torch.float32, device=dev)
    ranks = torch.empty((rows, H * W), dtype=torch.int32, device=dev)
    mom = torch.empty((rows, hm, wm), dtype=torch.float32, device=dev)
    targets_all = torch.tensor(counts * Kc, dtype=torch.int32).to(dev)       # row k A + a: area a
    with _eval_mode(model), torch.enable_grad():
        for b in range(B):
            cb = cols[b:b + 1] if per_image else cols
            cols_all = torch.tensor([c for c in cb for _ in range(A)], dtype=torch.int32).to(dev)
            pyr = perturbation_pyramid(x[b], levels, max_blur)
            for r0 in range(0, R, batch):
                n = min(batch, R - r0)
                pm = pmasks[b, r0:r0 + n]
                cg, tg = cols_all[r0:r0 + n], targets_all[r0:r0 + n]
                mk, dm, st, rk = mask[:n], dmask[:n], stats[:n], ranks[:n]
                rw = torch.empty((n_iters, n), dtype=torch.float32, device=dev)
                for it in range(n_iters):
                    flip = bool(jitter) and it % 2 == 1
                    K.extremal_mask(pm, mk, step, sigma, st)
                    leaf = K.extremal_blend(pyr, mk, buf[:n], variant, flip).detach().requires_grad_(True)
                    out = model(leaf)
                    logp = out.detach()
                    logp = logp if logp.dtype == torch.float32 and logp.is_contiguous() else logp.float().contiguous()
                    K.extremal_seed(logp, cg, seed[:n], rw, it, variant)
                    g = torch.autograd.grad(out, leaf, seed[:n].to(out.dtype))[0]
                    g = g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()
                    K.saliency_ranks(mk.view(n, H * W), out=rk)
                    K.extremal_mask_grad(pyr, mk, g, rk, tg, dm, lams[it], variant, flip)
                    K.extremal_step(pm, mom[:n], mk, dm, st, step, sigma, lr, momentum, it == 0)
                    del out, leaf, g
                K.extremal_mask(pm, masks[b, r0:r0 + n], step, sigma)
                rewards[b, r0:r0 + n].copy_(rw.t())
    return ExtremalMasks(masks.view(B, Kc, A, H, W), pmasks.view(B, Kc, A, hm, wm), rewards.view(B, Kc, A, n_iters))


def extremal_saliency(model, images, classes=None, variant="preserve", **kwargs):
    """The masks of `extremal_perturbation` (its other keyword arguments pass through) as one FLOAT saliency map per class, fp32
    [B, K, H, W] on the device: the mean of the masks over the areas (kernels.channel_mean, the area axis playing the channel),
    and 1 - that mean for variant "delete", whose masks are small where the evidence is."""
    r = extremal_perturbation(model, images, classes, variant=variant, **kwargs)
    m = K.channel_mean(r.masks)
    return 1.0 - m if variant == "delete" else m


def extremal_maps(model, images, classes=None, min_level=0.0, **kwargs):
    """uint8 Extremal Perturbation heat maps [B, K, H, W] on the device: `extremal_saliency` (the mean of the masks over the
    areas; 1 - the mean for "delete"), then the drawing steps of `rise_maps` at the maps' own size (kernels.heat_maps)."""
    return K.heat_maps(extremal_saliency(model, images, classes, **kwargs), min_level)


IbaEstimate = collections.namedtuple("IbaEstimate", "mean std active n")
IbaEstimate.__doc__ = """The fitted feature distribution `information_bottleneck` needs, from `iba_estimate`: fp32 mean, std and 0 / 1
activity [h, w, channel] of the backbone's output (NHWC, on the device) and the number of images n they were fitted on."""


def iba_estimate(model, batches, n_samples=5000, threshold=0.01):
    """Fits the per-neuron distribution of the backbone's output over `batches`, any iterable of image batches [b, C, H, W] (or of
    tuples whose first entry is one, as a data loader yields) -> IbaEstimate.  Each batch takes one SlotModel.feature_pass and one
    kernels.iba_estimate launch (streaming Welford in float64, rows in order, so the batching does not change a bit); whole
    batches are taken until at least `n_samples` images are in.  std = sqrt(M2 / (n - 1)); a neuron is active where it was
    non-zero in more than `threshold` of the images (the reference's TorchWelfordEstimator).  Fewer than 2 images: ValueError."""
    state = None
    for batch in batches:
        if state is not None and state.n >= int(n_samples):
            break
        images = batch[0] if isinstance(batch, (tuple, list)) else batch
        feat = model.feature_pass(_check_images(images)).features
        state = K.iba_estimate(feat, state)
    if state is None or state.n < 2:
        raise ValueError("iba_estimate needs at least 2 images, got %d" % (0 if state is None else state.n))
    mean, std, active = K.iba_estimate_finish(state, threshold)
    return IbaEstimate(mean, std, active, state.n)


def _check_iba(images, estimate, steps, samples, sigma, batch):
    """the refusals of information_bottleneck that need no launch -> (steps, samples, rows per group or None)"""
    steps, samples = int(steps), int(samples)
    if steps < 1 or samples < 1:
        raise ValueError("steps and samples must be at least 1, got %d and %d" % (steps, samples))
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be at least 1, got %d" % int(batch))
    if not isinstance(estimate, IbaEstimate) or not all(torch.is_tensor(v) for v in estimate[:3]):
        raise ValueError("estimate must be an IbaEstimate (from iba_estimate), got %s" % type(estimate).__name__)
    shape = tuple(estimate.mean.shape)
    if len(shape) != 3 or tuple(estimate.std.shape) != shape or tuple(estimate.active.shape) != shape:
        raise ValueError("estimate.mean, .std and .active must share one shape [h, w, channel], got %s, %s and %s"
                         % (shape, tuple(estimate.std.shape), tuple(estimate.active.shape)))
    r = K.iba_radius(sigma)
    if r >= shape[0] or r >= shape[1]:
        raise ValueError("sigma = %r smooths with a window of radius %d: the %d x %d features must exceed it in both directions "
                         "(sigma=None: no smoothing)" % (sigma, r, shape[0], shape[1]))
    _check_images(images)
    if not images.is_cuda or not estimate.mean.is_cuda:
        raise RuntimeError("information_bottleneck runs on a HIP device (images on %s, estimate on %s); there is no CPU fallback"
                           % (images.device, estimate.mean.device))
    return steps, samples, (None if batch is None else int(batch))


def information_bottleneck(model, images, estimate, classes=None, beta=10.0, steps=10, samples=10, sigma=1.0, lr=1.0, min_std=0.01,
                           relu=False, batch=None, seed=0):
    """Information-bottleneck attribution (Schulz, Sixt, Tombari, Landgraf, ICLR 2020, "Restricting the Flow"; the per-sample
    bottleneck of the reference's torchcam/IBA/pytorch.py, which torchcam_vis.py attaches to model.layer4) of `images` [B, C, H, W]
    at the backbone's output -> fp32 [B, K, h, w] on the device, in bits per cell.  This docstring (and include/scouter_hip.h) is the
    definition; tests/test_iba_cpu.py restates it in float64.

    x is one image's feature tensor [h, w, C] (NHWC), m, s, a = `estimate` (`iba_estimate`), alpha [K, h, w, C] one mask per
    explained class, S = samples, E = h w C.
    smoothing G  the depthwise Gaussian window of side 2 round(2 sigma) + 1 (5 at sigma = 1), values exp(-d^2 / (2 sigma^2))
                 normalised to sum 1, over (h, w) with reflection padding that does not repeat the edge (ReflectionPad2d);
                 sigma=None: none.  h and w must both exceed the radius (ValueError; the reference raises from the pad).
    mask         lambda = G(sigmoid(alpha)), kappa = 1 - lambda formed as G(sigmoid(-alpha)).
    noise        eps[j], row j = k S + s, at iteration t: the stream of kernels.noise_images for sample t K S + j under `seed`.
    sample       z[j] = a (lambda_k x + kappa_k (max(s, min_std) eps[j] + m)), clamped at 0 with `relu`.
    capacity     cap_k = -0.5 (1 + 2 ln kappa - r^2 lambda^2 - kappa^2) nats where a = 1, r = (x - m) / max(s, min_std); exactly 0
                 where a = 0.
    loss_k       -mean_s log_probs[k S + s, class_k] + beta mean_{p, c} cap_k; the head runs on z (SlotModel.head_pass).
    update       Adam as torch.optim.Adam (lr, betas (0.9, 0.999), eps 1e-8) on alpha from 5, by the analytic gradient
                 sigmoid'(alpha) G^T(a (sum_s dz (x - (s eps + m)) [z > 0 if relu] + beta / E (1 / kappa + r^2 lambda - kappa))).
    result       sum_c cap / ln 2 of the LAST forward, that is of alpha after steps - 1 updates -- what the reference returns.

    classes as in `gradcam`: None (every output), a list of ints (K = len), or a LongTensor [B] (each image its own class,
    K = 1).  `batch` caps the head rows per pass: the classes of an image run in groups of max(1, batch // samples) whole classes
    (None: all at once); masks are independent and the noise of a row depends on (seed, t, row) alone, so the grouping does not
    change a bit.  One SlotModel.feature_pass for the batch, then per image, group and iteration: kernels.iba_sample,
    model.head_pass, its .grad with a seed of -1 / S built once, kernels.iba_step; the last iteration stops after the sample,
    which writes the capacity, and kernels.iba_bits sums it.  Nothing is copied to the host and nothing synchronises; two calls
    give the same bits.  Head parameters that require grad get their `.grad` overwritten by each backward.

    This DEPARTS from the reference in four ways: kappa avoids the cancellation of fp32 1 - lambda at alpha around 5 to 17; an
    inactive neuron's capacity is selected as 0 where the reference multiplies and drops the NaN with nansum (the same map); the
    noise is the Philox stream, not torch's generator; and alpha past about 88 (never reached from 5 in tens of steps) gives
    kappa = 0 and an infinite capacity."""
    steps, S, batch = _check_iba(images, estimate, steps, samples, sigma, batch)
    x, _ = _check_images_batch(images, 1)
    B = x.shape[0]
    fp = model.feature_pass(x)
    feat, n_out = fp.features, int(fp.log_probs.shape[1])
    del fp
    _, h, w, C = feat.shape
    if tuple(estimate.mean.shape) != (h, w, C):
        raise ValueError("the estimate is for features %s, these images give %s" % (tuple(estimate.mean.shape), (h, w, C)))
    per_image, cols = _class_columns(classes, B, n_out)
    Kc = 1 if per_image else len(cols)
    dev = feat.device
    out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    kg = Kc if batch is None else min(Kc, max(1, batch // S))
    mean, std, active = (v.detach().to(dev, dtype=torch.float32).contiguous() for v in estimate[:3])
    z = torch.empty((kg * S, h, w, C), dtype=torch.float32, device=dev)
    cap = torch.empty((kg, h, w, C), dtype=torch.float32, device=dev)
    alpha, adam_m, adam_v = torch.empty_like(cap), torch.empty_like(cap), torch.empty_like(cap)
    for b in range(B):
        cb = cols[b:b + 1] if per_image else cols
        for k0 in range(0, Kc, kg):
            kn = min(kg, Kc - k0)
            al, am, av = alpha[:kn], adam_m[:kn], adam_v[:kn]
            al.fill_(5.0); am.zero_(); av.zero_()
            hseed = torch.zeros((kn * S, n_out), dtype=torch.float32, device=dev)
            hcols = torch.tensor([c for c in cb[k0:k0 + kn] for _ in range(S)], dtype=torch.int64).to(dev)
            hseed[torch.arange(kn * S, device=dev), hcols] = -1.0 / S
            for t in range(steps):
                last = t == steps - 1
                K.iba_sample(feat[b], mean, std, active, al, z[:kn * S], cap[:kn] if last else None, sigma, seed, t, relu, min_std,
                             row0=k0 * S, rows=Kc * S)
                if last:
                    break
                dz = model.head_pass(z[:kn * S]).grad(hseed)
                K.iba_step(feat[b], mean, std, active, al, dz, am, av, sigma, seed, t, beta, lr, relu, min_std, row0=k0 * S,
                           rows=Kc * S)
                del dz
            K.iba_bits(cap[:kn], out=out[b, k0:k0 + kn])
    return out


def iba_saliency(model, images, estimate, classes=None, size=None, **kwargs):
    """The maps of `information_bottleneck` (its other keyword arguments pass through) brought to the image: fp32 [B, K, H, W] on
    the device, `size` = (H, W) (None: the images' H x W).  The bits of a cell are spread over its pixels -- times h w / (H W) --
    and resized by kernels.resize_bilinear, the clamped half-pixel bilinear.  The reference resizes with skimage's
    resize(order=1), whose reflecting edge mode equals the clamped one when upsampling; skimage was not available to check
    that when this was written."""
    H, W = _out_size(size, images)
    bits = information_bottleneck(model, images, estimate, classes, **kwargs)
    h, w = bits.shape[-2:]
    return K.resize_bilinear(bits * (float(h * w) / float(H * W)), H, W)


def iba_maps(model, images, estimate, classes=None, size=None, min_level=0.0, **kwargs):
    """uint8 information-bottleneck heat maps [B, K, H, W] on the device: `iba_saliency`, then the drawing steps of `rise_maps`
    (kernels.heat_maps)."""
    return K.heat_maps(iba_saliency(model, images, estimate, classes, size, **kwargs), min_level)


IgosMasks = collections.namedtuple("IgosMasks", "masks pmasks curves")
IgosMasks.__doc__ = """The result of `igos`, on the images' device: fp32 masks [B, K, H, W] in [0, 1] (the upsampled final masks, small
where the evidence is), fp32 pmasks [B, K, hm, wm] (the coarse masks themselves) and fp64 curves [B, K, n_iters, 4]: per iteration
the regulariser before the update, the class probability of the masked image before the update, the step size the line search
took and its index in `igos_ladder`."""


def igos_ladder(step0=200.0, shrink=0.2, min_step=1e-5):
    """The step sizes the line search of `igos` tries, as a list of floats (host, float64): [0, step0, step0 shrink, step0 shrink^2,
    ...] up to and including the first value below min_step, each formed from the one before by one multiplication.  Entry 0 is
    the step of size 0 -- the mask as it stands.  The defaults give 12 trial steps, 200 down to 4.096e-6."""
    step0, shrink, min_step = float(step0), float(shrink), float(min_step)
    if not 0.0 < step0 < float("inf") or not 0.0 < shrink < 1.0 or not 0.0 < min_step < float("inf"):
        raise ValueError("igos_ladder: step0 = %r, shrink = %r, min_step = %r (step0 and min_step positive and finite, 0 < shrink < 1)"
                         % (step0, shrink, min_step))
    ladder, s = [0.0, step0], step0
    while s >= min_step:
        s *= shrink
        ladder.append(s)
        if len(ladder) > K.IGOS_MAX_LADDER:
            raise ValueError("igos_ladder: step0 = %r, shrink = %r, min_step = %r give more than %d steps"
                             % (step0, shrink, min_step, K.IGOS_MAX_LADDER - 1))
    return ladder


def _igos_size(size, H, W):
    """the `size` argument of `igos` -> (hm, wm), checked against the image"""
    try:
        hm, wm = (int(size), int(size)) if not isinstance(size, (tuple, list)) else (int(size[0]), int(size[1]))
        ok = not isinstance(size, (tuple, list)) or len(size) == 2
    except (TypeError, ValueError, IndexError):
        ok, hm, wm = False, 0, 0
    if not ok:
        raise ValueError("size must be an int or (hm, wm), got %r" % (size,))
    if H < 2 or W < 2:
        raise ValueError("images of %d x %d pixels: each side must be at least 2" % (H, W))
    if not (2 <= hm <= H and 2 <= wm <= W):
        raise ValueError("a mask of %d x %d cells for images of %d x %d pixels (2 <= hm <= H, 2 <= wm <= W)" % (hm, wm, H, W))
    if hm * wm > K.IGOS_MAX_CELLS:
        raise ValueError("a mask of %d x %d cells: at most %d cells" % (hm, wm, K.IGOS_MAX_CELLS))
    return hm, wm


def igos(model, images, classes=None, size=8, n_iters=15, n_steps=20, l1_coeff=1.0, tv_coeff=20.0, tv_beta=2.0, sigma=0.2,
         baseline=None, blur_klen=31, blur_sigma=30.0, step0=200.0, shrink=0.2, min_step=1e-5, alpha=1e-4, adapt_l1=True, batch=50,
         seed=0, init=None):
    """I-GOS (Qi, Khorram, Fuxin, AAAI 2020; the Integrated_Mask the reference's torchcam_vis.py runs first of all) of `images`
    [B, C, H, W] -> IgosMasks: for every image and class c_k the small, smooth mask whose masked image loses the most probability
    of class c_k, found by n_iters steps along the integrated gradient with a backtracking line search.  The reference program
    cannot run here; this docstring (and include/scouter_hip.h) is the specification.  The defaults are the reference's call.

    mask         a coarse mask p [hm, wm] in [0, 1], (hm, wm) = `size` (an int: both), starts at 1 (or `init`) and is upsampled by
                 U = torch.nn.UpsamplingBilinear2d's rule, align_corners = True (kernels.igos_upsample).  1 keeps the image, 0
                 replaces it: the masked image is x' + U(p) (x - x'), x' the `baseline`: None (the image blurred by
                 kernels.separable_filter with `gaussian_taps(blur_klen, blur_sigma)`), [C, H, W] (one for the batch) or [B, C, H, W].
    regulariser  loss1(p) = l1 mean|1 - p| + tv_coeff (mean|p[i, :] - p[i + 1, :]|^tv_beta + mean|p[:, j] - p[:, j + 1]|^tv_beta); l1
                 starts at l1_coeff and is a per-class state (below).
    direction    at iteration `it` the n_steps = S path points x_j = x' + (j + 1) / S U(p) (x - x') + sigma z_j, z_j the noise of
                 kernels.noise_images for (seed, it S + j, element) -- the same for every class -- go through the model, and
                 g = d (loss1 + (1 / S) sum_j prob_j) / d p, prob = exp(log_prob[c_k]): the input gradients are contracted with
                 (j + 1) / S (x - x') in float64 (kernels.igos_accumulate), pulled back through U and joined by the regulariser's
                 derivative (kernels.igos_mask_grad; the derivative of |.| at 0 is 0).
    line search  the candidates cand_k = clamp(p - steps[k] g, 0, 1) for EVERY k of `igos_ladder(step0, shrink, min_step)` (k = 0:
                 the mask as it stands) form one batched stream (kernels.igos_trial_images) that goes through the model without
                 noise; tot_k = loss1(cand_k) + prob(cand_k); the first k >= 1 with not (tot_k > tot_0 - alpha steps[k] sum g^2) is
                 taken, the last one when none passes (kernels.igos_step), and p = cand_k.
    adapt_l1     (n_iters > 3) after iteration n_iters // 2, l1 /= 10 for a class whose probability has moved by at most 1e-3 since
                 iteration 0; otherwise after iteration int(n_iters / 1.25), l1 /= 5 when it has moved by at most 1e-2.

    classes as in `gradcam` / `extremal_perturbation`: None (every output), a list of ints (K = len), or a LongTensor [B] (each
    image its own class, K = 1).  init: None, fp32 [hm, wm] (every mask) or [B, K, hm, wm].  Per image the K masks are the rows of
    one stream: per iteration the K S path images in chunks of at most `batch` rows -- kernels.igos_path_images into one reused
    buffer, which becomes the leaf of an eval-mode forward and of one backward whose seed kernels.extremal_seed (variant
    "delete") writes from the output itself, kernels.igos_accumulate -- then kernels.igos_mask_grad, the K T1 trial images in
    chunks under no_grad, kernels.igos_step; kernels.igos_upsample at the end.  Rows are independent and every sum has one fixed
    order, so neither `batch` nor the set of classes in the call changes a bit of a class's result, and two calls give the same
    bits.  Nothing is copied to the host and nothing synchronises inside the loop.  The model is in eval mode (no BatchNorm buffer
    moves; the caller's mode is restored) and runs its plain eval backward, as in `extremal_perturbation`: SlotModel's backward
    overwrites the `.grad` of its parameters that require grad, a plain torch module has no `.grad` touched.  Any module whose
    eval forward returns log-probabilities [n, n_outputs] and is differentiable to its input will do.

    This DEPARTS from the reference in: the path term's weight 1 / n_steps (the reference hard-codes / 20, the same at the
    default); the probability, which is exp of the model's log-probability (the reference applies a softmax to its model's
    output); the blur, zero-padded with at most 31 taps (the reference: cv2.GaussianBlur(51, 50), reflecting border); the noise,
    Philox and Box-Muller on the device (the reference: cv2.randn on the host); the per-iteration top-40-pixel curve, left out;
    adapt_l1, which compares with iteration 0 (the reference's curve starts with a doubled entry, so it compares with the
    iteration before); and the line search, which evaluates every candidate in one batch -- more forwards, no host round trip,
    the same choice."""
    n_iters, S = int(n_iters), int(n_steps)
    if n_iters < 1 or S < 1:
        raise ValueError("n_iters and n_steps must be at least 1, got %d and %d" % (n_iters, S))
    if not (0.0 <= float(l1_coeff) < float("inf") and 0.0 <= float(tv_coeff) < float("inf")):
        raise ValueError("l1_coeff and tv_coeff must be finite and not negative, got %r and %r" % (l1_coeff, tv_coeff))
    if not 1.0 <= float(tv_beta) <= 64.0:
        raise ValueError("tv_beta must lie inside [1, 64], got %r" % (tv_beta,))
    if not 0.0 <= float(sigma) < float("inf"):
        raise ValueError("sigma must be finite and not negative, got %r" % (sigma,))
    if not 0.0 <= float(alpha) < float("inf"):
        raise ValueError("alpha must be finite and not negative, got %r" % (alpha,))
    ladder = igos_ladder(step0, shrink, min_step)
    T1 = len(ladder)
    if (n_iters + 1) * S >= 1 << 31:
        raise ValueError("n_iters * n_steps = %d noise samples are past 2^31" % (n_iters * S))
    x, batch = _check_images_batch(images, batch)
    B, C, H, W = x.shape
    hm, wm = _igos_size(size, H, W)
    if baseline is not None:
        if not torch.is_tensor(baseline) or tuple(baseline.shape) not in ((C, H, W), (B, C, H, W)):
            raise ValueError("baseline must be None, [%d, %d, %d] or [%d, %d, %d, %d], got %s"
                             % (C, H, W, B, C, H, W, tuple(baseline.shape) if torch.is_tensor(baseline) else type(baseline).__name__))
    else:
        taps = gaussian_taps(blur_klen, blur_sigma)
    if init is not None:
        if not torch.is_tensor(init) or not (tuple(init.shape) == (hm, wm) or
                                             (init.dim() == 4 and tuple(init.shape[2:]) == (hm, wm) and init.shape[0] == B)):
            raise ValueError("init must be None, [%d, %d] or [B = %d, K, %d, %d], got %s"
                             % (hm, wm, B, hm, wm, tuple(init.shape) if torch.is_tensor(init) else type(init).__name__))
    n_out = _num_outputs(model, x)
    per_image, cols = _class_columns(classes, B, n_out)
    R = 1 if per_image else len(cols)
    if init is not None and init.dim() == 4 and init.shape[1] != R:
        raise ValueError("init must be None, [%d, %d] or [B = %d, K = %d, %d, %d], got %s" % (hm, wm, B, R, hm, wm, tuple(init.shape)))
    dev = x.device
    pmasks = torch.ones((B, R, hm, wm), dtype=torch.float32, device=dev)
    if init is not None:
        pmasks.copy_(init.detach().to(dev, dtype=torch.float32).reshape((B, R, hm, wm) if init.dim() == 4 else (1, 1, hm, wm))
                     .expand(B, R, hm, wm))
    masks = torch.empty((B, R, H, W), dtype=torch.float32, device=dev)
    curves = torch.zeros((B, R, n_iters, 4), dtype=torch.float64, device=dev)
    if R == 0:
        return IgosMasks(masks, pmasks, curves)
    if baseline is not None:
        baseline = baseline.detach().to(dev, dtype=torch.float32).contiguous()
    else:
        taps = taps.to(dev)
    rows = min(batch, R * max(S, T1))
    buf = torch.empty((rows, C, H, W), dtype=torch.float32, device=dev)
    seed_rows = torch.empty((min(rows, R * S), n_out), dtype=torch.float32, device=dev)
    probs = torch.empty((1, seed_rows.shape[0]), dtype=torch.float32, device=dev)     # (extremal_seed's rewards: not kept)
    acc = torch.empty((R, H, W), dtype=torch.float64, device=dev)
    dmask = torch.empty((R, hm, wm), dtype=torch.float32, device=dev)
    stats = torch.empty((R, 2), dtype=torch.float64, device=dev)
    logp_all = torch.empty((R * T1, n_out), dtype=torch.float32, device=dev)
    l1 = torch.empty((R,), dtype=torch.float32, device=dev)
    steps = torch.tensor(ladder, dtype=torch.float64).to(torch.float32).to(dev)
    with _eval_mode(model), torch.enable_grad():
        for b in range(B):
            cb = cols[b:b + 1] if per_image else cols
            cols_rows = torch.tensor(cb, dtype=torch.int32).to(dev)
            cols_path = torch.tensor([c for c in cb for _ in range(S)], dtype=torch.int32).to(dev)
            base = K.separable_filter(x[b], taps) if baseline is None else baseline if baseline.dim() == 3 else baseline[b]
            pm = pmasks[b]
            l1.fill_(float(l1_coeff))
            for it in range(n_iters):
                acc.zero_()
                for first in range(0, R * S, batch):
                    n = min(batch, R * S - first)
                    leaf = K.igos_path_images(x[b], base, pm, buf[:n], first, S, sigma, seed, it * S).detach().requires_grad_(True)
                    out = model(leaf)
                    logp = out.detach()
                    logp = logp if logp.dtype == torch.float32 and logp.is_contiguous() else logp.float().contiguous()
                    K.extremal_seed(logp, cols_path[first:first + n], seed_rows[:n], probs[:, :n], 0, "delete")
                    g = torch.autograd.grad(out, leaf, seed_rows[:n].to(out.dtype))[0]
                    g = g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()
                    K.igos_accumulate(x[b], base, g, acc, first, S)
                    del out, leaf, g
                K.igos_mask_grad(pm, acc, l1, dmask, stats, tv_coeff, tv_beta)
                with torch.no_grad():
                    for first in range(0, R * T1, batch):
                        n = min(batch, R * T1 - first)
                        logp_all[first:first + n].copy_(model(K.igos_trial_images(x[b], base, pm, dmask, steps, buf[:n], first)))
                K.igos_step(pm, dmask, steps, logp_all, cols_rows, stats, l1, curves[b], it, n_iters, alpha, tv_coeff, tv_beta,
                            adapt_l1)
            K.igos_upsample(pm, masks[b])
    return IgosMasks(masks, pmasks, curves)


def igos_saliency(model, images, classes=None, **kwargs):
    """The masks of `igos` (its other keyword arguments pass through) as one FLOAT saliency map per class, fp32 [B, K, H, W] on
    the device: 1 - masks, large where the evidence is.  The reference draws -mask + 2 max(mask), which the min-max scaling of
    the drawing steps reduces to the same map."""
    return 1.0 - igos(model, images, classes, **kwargs).masks


def igos_maps(model, images, classes=None, min_level=0.0, **kwargs):
    """uint8 I-GOS heat maps [B, K, H, W] on the device: `igos_saliency`, then the drawing steps of `rise_maps` at the maps' own
    size (kernels.heat_maps)."""
    return K.heat_maps(igos_saliency(model, images, classes, **kwargs), min_level)


def occlusion_windows(size, window, stride):
    """(ny, nx): the number of windows per axis of an `occlusion` run over images of `size` = (H, W); `window` and `stride` are an
    int or a pair (rows, columns).  Per axis, with 1 <= stride <= window <= size (anything else is a ValueError):
    n = 1 + ceil((size - window) / stride); window i covers [i * stride, min(i * stride + window, size)), so the last one may be
    partial and every pixel is covered; the windows that cover pixel y are i in [max(0, ceil((y - window + 1) / stride)),
    min(n - 1, y // stride)].  Window n = iy * nx + ix.  Host arithmetic only."""
    return K.occlusion_windows(size, window, stride)


def _rows_per_forward(batch):
    if batch < 2:
        raise ValueError("batch must be at least 2 (the clean row and one changed row), got %d" % batch)
    return batch


def occlusion(model, images, classes=None, window=16, stride=8, fill=0.0, batch=250, of="prob"):
    """Occlusion sensitivity (Zeiler & Fergus 2014; captum's Occlusion) of `images` [B, C, H, W] -> fp32 [B, K, H, W] on the images'
    device:  S[b, k, y, x] = the mean, over the windows n that cover (y, x), of F(out_clean[classes[k]]) - F(out_n[classes[k]]),
    out_n the eval-mode output for images[b] with window n set to `fill` in every channel.  of="prob": F = exp, the drop of the
    class probability; of="log_prob": F is the identity (the two modes of kernels.output_deltas, in float64).

    The windows are those of `occlusion_windows((H, W), window, stride)` -- `window` and `stride` an int or a pair (rows, columns),
    1 <= stride <= window <= size per axis; the last window of an axis may be partial; the order is rows of windows, then columns.
    `fill` is one number for every channel: 0.0 is the dataset mean of a normalised image.  classes as in `gradcam` / `rise`: None
    (every class), a list of ints (K = len), or a LongTensor [B] (each image its own class, K = 1).  Any module whose eval forward
    returns log-probabilities [n, n_outputs] will do.

    Per image the N = ny * nx windows go through the model in chunks of batch - 1 occluded rows behind the clean image in row 0
    (batch >= 2; the last chunk may be shorter): kernels.occlude_images into one reused buffer, the model under torch.no_grad() in
    eval mode (folded when the model's inference fold is on; the caller's mode is restored), kernels.output_deltas -- both sides of
    a difference come from the same forward.  kernels.occlusion_finish once per image: the covering windows are added in float64
    in one fixed order, divided by their number and rounded to fp32 once.  The same bits for any two runs.  No BatchNorm buffer
    moves, no `.grad` appears, nothing is copied to the host and nothing synchronises inside the loop.

    What departs from captum's Occlusion: one window for all channels (captum slides over the channel axis too; this is its
    window shape (C, wh, ww)); a scalar baseline; every class is read from the ONE stream of forwards, where captum takes one
    target per call; the clean output is recomputed in every forward, so that both sides of a difference see the same kernels;
    the mean is formed in float64; and the default F is the probability, where captum differences whatever the forward returns
    (of="log_prob" is that).  The window rule -- a stride no larger than the window, a partial last window -- is captum's as far
    as it is remembered here; captum is no dependency and nothing was checked against it."""
    if of not in ("log_prob", "prob"):
        raise ValueError("of must be 'log_prob' or 'prob', got %r" % (of,))
    B, C, H, W = _check_images(images).shape
    ny, nx = occlusion_windows((H, W), window, stride)
    fill = float(fill)
    if fill != fill:
        raise ValueError("fill must be a number, got %r" % (fill,))
    x, batch = _check_images_batch(images, batch)
    batch = _rows_per_forward(batch)
    per_image, cols = _class_columns(classes, B, _num_outputs(model, images))
    dev = images.device
    N = ny * nx
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    Kc = 1 if per_image else len(cols)
    out = torch.empty((B, Kc, H, W), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    deltas = torch.empty((Kc, N), dtype=torch.float64, device=dev)
    buf = torch.empty((min(batch, N + 1), C, H, W), dtype=torch.float32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            for first in range(0, N, batch - 1):
                chunk = K.occlude_images(x[b], buf[:1 + min(batch - 1, N - first)], first, window, stride, fill)
                logp = model(chunk)
                logp = logp if logp.dtype == torch.float32 and logp.is_contiguous() else logp.float().contiguous()
                K.output_deltas(logp, cb, deltas, first, of)
            K.occlusion_finish(deltas, out[b], window, stride)
    return out


def occlusion_maps(model, images, classes=None, min_level=0.0, **kwargs):
    """uint8 occlusion heat maps [B, K, H, W] on the device: `occlusion` (its other keyword arguments pass through), then the
    drawing steps of `rise_maps` at the maps' own size (kernels.heat_maps), which cut the pixels whose occlusion RAISED the class
    to 0."""
    return K.heat_maps(occlusion(model, images, classes, **kwargs), min_level)


def ablationcam(model, images, classes=None, batch=256, relu=True):
    """Ablation-CAM (Desai & Ramaswamy, WACV 2020) of `images` [B, Cin, H, W] at the backbone's output -> fp32 [B, K, h, w] on the
    images' device:  S[b, k, p] = sum_c w[b, k, c] * A[b, p, c], clamped at 0 when `relu`, with A = model.feature_pass(images)
    .features (NHWC [B, h, w, C], the layer `gradcam` reads) and
    w[b, k, c] = float32((P(A[b]) - P(A[b] with channel c zeroed)) / P_clean),  P = exp(log_prob[classes[k]])
    in float64: the relative drop of the class probability when channel c is taken away.  The two P of the numerator come from ONE
    head forward (the clean features ride in row 0 of every chunk); the denominator P_clean is the feature pass's own
    log-probability.  The channels are added in ascending order, one fma each, the weight rounded from float64 once.

    One `feature_pass` for the batch; then per image the C channels go in chunks of batch - 1 ablated rows behind the clean
    features in row 0 (batch >= 2; the last chunk may be shorter): kernels.ablate_channels into one reused buffer,
    model.head_pass(buf).log_probs -- the head alone: the 2048 ablated copies of resnest26d never enter the backbone, where
    `scorecam` pays 2048 whole forwards -- and kernels.output_deltas(of="prob"); kernels.ablation_contract once per image.  No
    backward runs.  The same bits for any two runs.  No BatchNorm buffer moves, no `.grad` appears, nothing is copied to the host
    and nothing synchronises inside the loop.  classes as in `gradcam`; it needs a SlotModel (slot head or FC baseline).

    What departs from the paper: the weights are relative drops of the class PROBABILITY, the quantity `scorecam` weights by,
    where the paper uses the raw class score before the softmax; ablation is to 0, the minimum of post-ReLU features (the paper's
    choice for such layers); a clean probability that underflows to 0 gives the infinity or NaN the division gives."""
    B = _check_images(images).shape[0]
    per_image, cols = _class_columns(classes, B, _num_classes(model, images))
    x, batch = _check_images_batch(images, batch)
    batch = _rows_per_forward(batch)
    dev = images.device
    fp = model.feature_pass(x)
    feat, clean = fp.features.detach(), fp.log_probs.detach()   # (the FeaturePass and its head state are dropped here)
    del fp
    feat = (feat.float() if feat.dtype != torch.float32 else feat).contiguous()
    clean = (clean.float() if clean.dtype != torch.float32 else clean).contiguous()
    _, h, w, C = feat.shape
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(dev)
    Kc = 1 if per_image else len(cols)
    out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
    if Kc == 0:
        return out
    deltas = torch.empty((Kc, C), dtype=torch.float64, device=dev)
    buf = torch.empty((min(batch, C + 1), h, w, C), dtype=torch.float32, device=dev)
    with _eval_mode(model), torch.no_grad():
        for b in range(B):
            cb = cols_dev[b:b + 1] if per_image else cols_dev
            for first in range(0, C, batch - 1):
                chunk = K.ablate_channels(feat[b], buf[:1 + min(batch - 1, C - first)], first)
                logp = model.head_pass(chunk).log_probs
                logp = logp if logp.dtype == torch.float32 and logp.is_contiguous() else logp.float().contiguous()
                K.output_deltas(logp, cb, deltas, first, "prob")
            K.ablation_contract(deltas, clean[b], cb, feat[b], out[b], relu)
    return out


def ablationcam_maps(model, images, classes=None, size=None, min_level=0.0, **kwargs):
    """uint8 Ablation-CAM heat maps [B, K, H, W] on the device: `ablationcam` (its other keyword arguments pass through), then the
    drawing steps of `gradcam_maps` in one launch (kernels.cam_maps) at `size` = (H, W) (None: the images' H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(ablationcam(model, images, classes, **kwargs), H, W, min_level)


def _image_baseline(baseline, x):
    """the `baseline` argument of the path methods, an IMAGE: None (zeros), [C, H, W] (one for the batch) or [B, C, H, W] -> None or
    the tensor on x's device, fp32 and contiguous"""
    B, C, H, W = x.shape
    if baseline is None:
        return None
    if not torch.is_tensor(baseline) or tuple(baseline.shape) not in ((C, H, W), (B, C, H, W)):
        raise ValueError("baseline must be None, [%d, %d, %d] or [%d, %d, %d, %d], got %s"
                         % (C, H, W, B, C, H, W, tuple(baseline.shape) if torch.is_tensor(baseline) else type(baseline).__name__))
    return baseline.detach().to(x.device, dtype=torch.float32).contiguous()


def _fp32_dense(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _one_hot_rows(cols_dev, n):
    """cols int64 [M] on the device -> fp32 [M, n], row j the one-hot seed of class cols[j]"""
    rows = torch.zeros((cols_dev.shape[0], n), dtype=torch.float32, device=cols_dev.device)
    return rows.scatter_(1, cols_dev[:, None], 1.0) if cols_dev.shape[0] else rows


def _layer_results(out, attr, totals, ends, return_attr, return_delta):
    """(maps[, attr][, delta]) of the two layer path methods; delta = the float64 completeness sums minus `ends` [B, K], the
    float64 differences out(x)[c] - out(x')[c]"""
    res = [out]
    if return_attr:
        res.append(attr)
    if return_delta:
        res.append((totals - ends).float())
    return res[0] if len(res) == 1 else tuple(res)


def layer_integrated_gradients(model, images, classes=None, baseline=None, n_steps=50, method="gausslegendre", batch=256,
                               return_attr=False, return_delta=False):
    """Layer Integrated Gradients (captum's LayerIntegratedGradients) of `images` [B, Cin, H, W] at the backbone's output -> fp32
    [B, K, h, w] on the images' device.  With A = the features of images[b] (NHWC [h, w, C], the layer `gradcam` reads), A' = the
    features of the baseline IMAGE x' and g(F) = d out[:, c_k] / dF, the gradient of the head alone at the features F:
    attr[b, k] = (A - A') * sum_i w_i g(A' + alpha_i (A - A')),   map[b, k, p] = sum_c attr[b, k, p, c],
    a straight line IN FEATURE SPACE, (alpha_i, w_i) = ig_quadrature(n_steps, method).  The sum of a map over its positions satisfies
    completeness: it approaches out(x)[c_k] - out(x')[c_k] as n_steps grows.  For a head that is linear in the features (the FC
    baseline's logits) this is DeepLIFT; for the slot head it is what DeepLIFT's Rescale rule approximates.

    `baseline` is an image: None (zeros), [Cin, H, W] (one for the batch) or [B, Cin, H, W], as in `integrated_gradients`.  classes
    as in `gradcam`: None (every class), a list of ints (K = len), or a LongTensor [B] (each image its own class, K = 1); a class
    outside the outputs is an IndexError.  return_attr: also attr fp32 [B, K, h, w, C]; return_delta: also fp32 [B, K], the
    completeness gap sum_p map - (out(x) - out(x')), formed in float64.  The results come in that order.

    One SlotModel.feature_pass of the baseline and image rows gives A' and A (BatchNorm-folded when the model's inference fold is
    on).  Per image the n_steps path rows go through the head in chunks of `batch` (the last may be shorter): kernels.path_images
    into one reused feature buffer, ONE SlotModel.head_pass, and per class one `.grad` with a one-hot column and one
    kernels.grad_accumulate onto that class's float64 sums in step order -- one head forward per chunk, not one per class.  Then
    kernels.layer_attr_finish once for all K classes: maps, attributions and the float64 sum of each map.  The gap compares that sum
    with the two rows of one head_pass([A', A]).  Nothing is copied to the host and nothing synchronises inside the loop; no
    BatchNorm buffer moves and the caller's mode is restored; head parameters that require grad get their `.grad` overwritten by
    each backward, as in `gradcam`, and nothing enters the backbone.  It needs a SlotModel (slot head or FC baseline).

    What departs from captum's LayerIntegratedGradients: `out` is the eval-mode model output, the LOG-PROBABILITIES, as in every
    method here (the reference's captum script targets logits); the float map is the channel SUM, so that completeness holds map by
    map (the reference draws the channel mean; the factor 1 / C disappears in the min-max of the drawing); the quadrature table is
    `ig_quadrature`'s, rounded to fp32; the difference A - A' the path walks is formed in fp32 (kernels.path_images), the one
    that multiplies the sums in float64.  captum is no dependency and nothing was checked against it."""
    x, batch = _check_images_batch(images, batch)
    B = x.shape[0]
    alphas, weights = ig_quadrature(n_steps, method)
    baseline = _image_baseline(baseline, x)
    n = _num_classes(model, x)
    per_image, cols = _class_columns(classes, B, n)
    dev = x.device
    # (every upload comes before the first pass: a copy from the host waits for the work queued ahead of it)
    alphas, weights = alphas.to(dev), weights.to(dev)
    cols_dev = torch.tensor(cols, dtype=torch.int64).to(dev)
    onehots = _one_hot_rows(cols_dev, n)
    base_rows = torch.zeros_like(x[:1]) if baseline is None else baseline if baseline.dim() == 4 else baseline[None]
    nb = int(base_rows.shape[0])
    feats = _fp32_dense(model.feature_pass(torch.cat([base_rows, x])).features)
    _, h, w, C = feats.shape
    Kc = 1 if per_image else len(cols)
    out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
    attr = torch.empty((B, Kc, h, w, C), dtype=torch.float32, device=dev) if return_attr else None
    totals = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    ends = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    if Kc == 0 or B == 0:
        return _layer_results(out, attr, totals, ends, return_attr, return_delta)
    N = int(alphas.shape[0])
    buf = torch.empty((min(batch, N), h, w, C), dtype=torch.float32, device=dev)
    seed = torch.empty((min(batch, N), n), dtype=torch.float32, device=dev)
    acc = torch.empty((Kc, h, w, C), dtype=torch.float64, device=dev)
    with _eval_mode(model):
        for b in range(B):
            A0, A1 = feats[b if nb > 1 else 0], feats[nb + b]
            acc.zero_()
            for first in range(0, N, batch):
                m = min(batch, N - first)
                fp = model.head_pass(K.path_images(A1, A0, alphas, buf[:m], first))
                for k in range(Kc):
                    seed.copy_(onehots[b if per_image else k])  # (one launch: the row of the class, for every path row)
                    K.grad_accumulate(_fp32_dense(fp.grad(seed[:m])), weights, acc[k], None, first)
                del fp
            K.layer_attr_finish(K.LAYER_PATH, acc, out[b], feat=A1, base=A0, attr=None if attr is None else attr[b],
                                total=None if totals is None else totals[b])
            if return_delta:
                logp = model.head_pass(torch.stack([A0, A1])).log_probs.double()
                ends[b] = (logp[1] - logp[0]).index_select(0, cols_dev[b:b + 1] if per_image else cols_dev)
    return _layer_results(out, attr, totals, ends, return_attr, return_delta)


def layer_conductance(model, images, classes=None, baseline=None, n_steps=50, batch=50, return_attr=False, return_delta=False):
    """Layer Conductance (Dhamdhere et al. 2018; captum's LayerConductance) of `images` [B, Cin, H, W] at the backbone's output ->
    fp32 [B, K, h, w] on the images' device.  The path runs IN IMAGE SPACE: x_i = x' + (i / n) (x - x') for i = 0 .. n = n_steps,
    A(x_i) the backbone's output there (NHWC [h, w, C]) and g_i = d out[:, c_k] / dA at A(x_i):
    attr[b, k] = sum_{i < n} g_i * (A(x_{i+1}) - A(x_i)),   map[b, k, p] = sum_c attr[b, k, p, c],
    what flows through every element of the layer along the path.  The sum of a map over its positions approaches
    out(x)[c_k] - out(x')[c_k] as n_steps grows (completeness).

    `baseline`, `classes`, return_attr (fp32 [B, K, h, w, C]) and return_delta (fp32 [B, K]) as in `layer_integrated_gradients`.
    The table alpha_i = i / n is built in float64, rounded to fp32 and uploaded once.  Per image the n + 1 path images go through
    the model in chunks of the steps first .. first + m, at most `batch` rows (batch >= 2), and the next chunk starts at the row
    the last one ended at: kernels.path_images into one reused image buffer, ONE SlotModel.feature_pass per chunk
    (BatchNorm-folded when the model's inference fold is on), and per class one `.grad` with a one-hot column and one
    kernels.conductance_accumulate onto that class's float64 sums -- float64 differences of neighbouring rows, one fma per step in
    step order.  Then kernels.layer_attr_finish (mode LAYER_SUM) once for all K classes.  The gap compares the float64 sum of each
    map with the two ends of the path, out(x_n) and out(x_0), as the feature passes of the first and the last chunk gave them.
    The guarantees are those of `layer_integrated_gradients`: nothing is copied to the host or synchronises inside the loop, no
    BatchNorm buffer moves, the caller's mode is restored, only head parameters get a `.grad`, nothing is differentiated inside
    the backbone.

    What departs from captum's LayerConductance: the LOG-PROBABILITIES are the output, not the logits; the float map is the channel
    SUM, not the mean; the path has n + 1 equidistant points and n forward differences (captum differences the same rows), and
    the differences and sums are float64.  captum is no dependency and nothing was checked against it."""
    x, batch = _check_images_batch(images, batch)
    batch = _rows_per_forward(batch)
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError("n_steps must be at least 1, got %d" % n_steps)
    B = x.shape[0]
    baseline = _image_baseline(baseline, x)
    n = _num_classes(model, x)
    per_image, cols = _class_columns(classes, B, n)
    dev = x.device
    Kc = 1 if per_image else len(cols)
    cols_dev = torch.tensor(cols, dtype=torch.int64).to(dev)
    onehots = _one_hot_rows(cols_dev, n)
    alphas = torch.from_numpy((np.arange(n_steps + 1, dtype=np.float64) / n_steps).astype(np.float32)).to(dev)
    rows = min(batch, n_steps + 1)
    buf = torch.empty((rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
    seed = torch.empty((rows, n), dtype=torch.float32, device=dev)
    out = attr = acc = None
    totals = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    ends = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    with _eval_mode(model):
        for b in range(B if Kc else 0):
            base = None if baseline is None else baseline if baseline.dim() == 3 else baseline[b]
            for first in range(0, n_steps, batch - 1):
                m = min(batch - 1, n_steps - first)             # (steps of the chunk: rows first .. first + m)
                fp = model.feature_pass(K.path_images(x[b], base, alphas, buf[:m + 1], first))
                feats = _fp32_dense(fp.features)
                if acc is None:                                 # (the first pass tells the layer's shape)
                    _, h, w, C = feats.shape
                    out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
                    attr = torch.empty((B, Kc, h, w, C), dtype=torch.float32, device=dev) if return_attr else None
                    acc = torch.empty((Kc, h, w, C), dtype=torch.float64, device=dev)
                if first == 0:
                    acc.zero_()
                    if return_delta:
                        ends[b] = -fp.log_probs[0].double().index_select(0, cols_dev[b:b + 1] if per_image else cols_dev)
                for k in range(Kc):
                    seed.copy_(onehots[b if per_image else k])
                    K.conductance_accumulate(feats, _fp32_dense(fp.grad(seed[:m + 1])), acc[k])
                if return_delta and first + m == n_steps:
                    ends[b] += fp.log_probs[m].double().index_select(0, cols_dev[b:b + 1] if per_image else cols_dev)
                del fp
            K.layer_attr_finish(K.LAYER_SUM, acc, out[b], attr=None if attr is None else attr[b],
                                total=None if totals is None else totals[b])
    if out is None:                                             # (no class or no image: the shape comes from one feature pass)
        _, h, w, C = model.feature_pass(x[:1]).features.shape if B else (0, 0, 0, 0)
        out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
        attr = torch.empty((B, Kc, h, w, C), dtype=torch.float32, device=dev) if return_attr else None
    return _layer_results(out, attr, totals, ends, return_attr, return_delta)


def layer_gradxact(model, images, classes=None, rectify=False, relu=False):
    """Gradient times activation at the backbone's output, summed over the channels, of `images` [B, Cin, H, W] -> fp32 [B, K, h, w]
    on the images' device.  With A = features[b] (NHWC, the layer `gradcam` reads) and g = d out_k / dA:
    map[b, k, p] = sum_c r(g[p, c]) A[p, c],  r = max(., 0) when `rectify` and the identity otherwise, clamped at 0 when `relu`;
    the products and the sum in float64, rounded to fp32 once (kernels.layer_gxa, which fills cam[:, k] in place).  Where
    `gradcam` pools the gradient over the positions before it weights the channels, this keeps the gradient per position.
    rectify = relu = False is HiResCAM (`hirescam`), rectify = relu = True LayerCAM (`layercam`).

    classes, the feature pass, the head backwards and their side effects as in `gradcam`: None, a list of ints or a LongTensor
    [B]; one SlotModel.feature_pass, one head backward per class, one feature gradient alive at a time.  out_k is the
    LOG-PROBABILITY of class k, the model's output, not the raw score the papers and captum's scripts differentiate, and the map
    is the channel SUM."""
    return _gradient_cam(model, images, classes,
                         lambda feat, dfeat, out: K.layer_gxa(feat, dfeat, out, rectify=rectify, relu=relu))


def hirescam(model, images, classes=None):
    """HiResCAM (Draelos & Carin 2020; captum's LayerGradientXActivation at the backbone's output, summed over the channels) ->
    fp32 [B, K, h, w]: map[b, k, p] = sum_c g[p, c] A[p, c], signed.  `layer_gradxact` with rectify = relu = False, which see for
    what departs from captum (log-probabilities, the channel sum)."""
    return layer_gradxact(model, images, classes, rectify=False, relu=False)


def layercam(model, images, classes=None):
    """LayerCAM (Jiang et al. 2021) at the backbone's output -> fp32 [B, K, h, w]:
    map[b, k, p] = max(0, sum_c max(g[p, c], 0) A[p, c]), never negative.  `layer_gradxact` with rectify = relu = True, which see
    for what departs from the paper (log-probabilities)."""
    return layer_gradxact(model, images, classes, rectify=True, relu=True)


def layerig_maps(model, images, classes=None, size=None, min_level=0.0, **kwargs):
    """uint8 Layer Integrated Gradients heat maps [B, K, H, W] on the device: `layer_integrated_gradients` (its other keyword
    arguments pass through), then the drawing steps of `gradcam_maps` in one launch (kernels.cam_maps) at `size` = (H, W) (None:
    the images' H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(layer_integrated_gradients(model, images, classes, **kwargs), H, W, min_level)


def conductance_maps(model, images, classes=None, size=None, min_level=0.0, **kwargs):
    """uint8 Layer Conductance heat maps [B, K, H, W] on the device: `layer_conductance` (its other keyword arguments pass
    through), then the drawing steps of `gradcam_maps` in one launch (kernels.cam_maps) at `size` = (H, W) (None: the images'
    H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(layer_conductance(model, images, classes, **kwargs), H, W, min_level)


def hirescam_maps(model, images, classes=None, size=None, min_level=0.0):
    """uint8 HiResCAM heat maps [B, K, H, W] on the device: `hirescam`, then the drawing steps of `gradcam_maps` (kernels.cam_maps),
    which cut the negative evidence to 0."""
    H, W = _out_size(size, images)
    return K.cam_maps(hirescam(model, images, classes), H, W, min_level)


def layercam_maps(model, images, classes=None, size=None, min_level=0.0):
    """uint8 LayerCAM heat maps [B, K, H, W] on the device: `layercam`, then the drawing steps of `gradcam_maps` (kernels.cam_maps)."""
    H, W = _out_size(size, images)
    return K.cam_maps(layercam(model, images, classes), H, W, min_level)


def _check_gradshap(n_samples, bank_sigma, sigma=0.0):
    n_samples, bank_sigma, sigma = int(n_samples), float(bank_sigma), float(sigma)
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1, got %d" % n_samples)
    for name, v in (("sigma", sigma), ("bank_sigma", bank_sigma)):
        if not 0.0 <= v < float("inf"):
            raise ValueError("%s must be finite and not negative, got %r" % (name, v))
    return n_samples, bank_sigma, sigma


def _gradshap_bank(baselines, bank_sigma, n_samples, seed, x):
    """the `baselines` argument of the GradientSHAP methods -> the bank of baseline IMAGES, fp32 [R, C, H, W] on x's device: a
    tensor of that shape, or an int R >= 1 for the Gaussian bank, rows n_samples .. n_samples + R - 1 of
    kernels.noise_images(zeros, bank_sigma, seed) -- samples the noise of the image never reads"""
    C, H, W = x.shape[1:]
    if torch.is_tensor(baselines):
        if baselines.dim() != 4 or tuple(baselines.shape[1:]) != (C, H, W) or baselines.shape[0] < 1:
            raise ValueError("a tensor of baselines must be [R >= 1, %d, %d, %d], got %s" % (C, H, W, tuple(baselines.shape)))
        return baselines.detach().to(x.device, dtype=torch.float32).contiguous()
    if isinstance(baselines, bool) or not isinstance(baselines, (int, np.integer)):
        raise ValueError("baselines must be a tensor [R, %d, %d, %d] or an int R >= 1, got %s" % (C, H, W, type(baselines).__name__))
    if baselines < 1:
        raise ValueError("baselines must be at least 1, got %d" % baselines)
    bank = torch.empty((int(baselines), C, H, W), dtype=torch.float32, device=x.device)
    if bank.numel():
        K.noise_images(torch.zeros((C, H, W), dtype=torch.float32, device=x.device), bank, bank_sigma, seed, n_samples)
    return bank


def _gradshap_shares(n_samples, R, seed, dev):
    """n_r / n_samples, float64 [R] on the device: the share of the samples that drew baseline r (kernels.gradshap_draws; the
    counts are added on the device, nothing is read on the host)"""
    picks, _ = K.gradshap_draws(n_samples, R, seed, picks=torch.empty((n_samples,), dtype=torch.int32, device=dev))
    counts = torch.zeros((R,), dtype=torch.float64, device=dev)
    counts.index_add_(0, picks.long(), torch.ones((n_samples,), dtype=torch.float64, device=dev))
    return counts / n_samples


def gradient_shap(model, images, classes=None, baselines=10, bank_sigma=1.0, n_samples=50, sigma=0.0, batch=50, seed=0,
                  return_delta=False, route="autograd"):
    """GradientSHAP / expected gradients (Lundberg & Lee 2017; Erion et al. 2019; captum's GradientShap: NoiseTunnel over
    InputBaselineXGradient with multiply_by_inputs) of `images` [B, C, H, W] -> fp32 [B, K, C, H, W] on the images' device.  With
    a bank of R baselines b_r, per sample s < n_samples a baseline pick_s and a fraction alpha_s in (0, 1) drawn from `seed`:
    x~_s = x_b + sigma * z_s (sigma == 0: x_b itself), d_s = x~_s - b_pick_s, row_s = b_pick_s + alpha_s * d_s,
    attr[b, k] = (1 / n_samples) sum_s (d out[:, c_k] / d row at row_s) * d_s,
    out the eval-mode model output as in input_gradients(of="log_prob").  classes as in `gradcam` / `rise`: None (every output),
    a list of ints (K = len), or a LongTensor [B] (each image its own class, K = 1).

    `baselines` is the bank: a tensor [R, C, H, W], or an int R >= 1 for a Gaussian bank built on the device, rows n_samples ..
    n_samples + R - 1 of kernels.noise_images(zeros, bank_sigma, seed) (the noise of the image reads the samples below
    n_samples only).  In normalised image space that is the per-pixel Gaussian with the dataset's own mean and deviation;
    bank_sigma = 0 with R = 1 is the black image.  Anything else is a ValueError.

    The loop is that of `integrated_gradients`: per image and class the samples go through the model in chunks of `batch`
    (the last may be shorter) -- kernels.gradshap_images into one reused buffer, an eval-mode forward and one backward with a
    one-hot column, kernels.gradshap_accumulate (which forms d_s again from the draws; it is never stored) onto float64 sums in
    sample order, kernels.attr_finish at the end of the class -- with the same guarantees: the chunking does not change a bit, no
    BatchNorm buffer moves, the caller's mode is restored, nothing is copied to the host or synchronises inside the loop, `.grad`
    of parameters that require grad is overwritten, and any module whose eval forward returns [n, n_outputs] will do.  The same
    seed repeats bit for bit.

    return_delta=True: also `delta` fp32 [B, K] = sum(attr[b, k]) - (out(x_b)[c_k] - sum_r (n_r / n_samples) out(b_r)[c_k]),
    n_r the number of samples that drew r, formed in float64 from the sum of attr_finish; it costs one extra no_grad forward of
    the bank and the images.  The gap is a MONTE-CARLO quantity: one random point per sample stands for the integral along that
    sample's line, so it shrinks like 1 / sqrt(n_samples), not like a quadrature error; with sigma > 0 it also holds the noise,
    since the lines end at x~_s and the comparison is made at x_b.

    What departs from captum's GradientShap: the random stream is ours (Philox, kernels.gradshap_draws; captum draws from
    torch's generator); `out` is the LOG-PROBABILITIES, as in every method here; ONE draw sequence serves all images and
    classes (sample s of every image and class has the same pick, fraction and noise); sigma is absolute, not relative to the
    image's range.  captum is no dependency and nothing was checked against it.

    route="folded": as in `integrated_gradients_by_route` -- one folded forward of a chunk for every class."""
    _check_route(route)
    x, batch = _check_images_batch(images, batch)
    if route == "folded":
        _check_device_images(x)
    n_samples, bank_sigma, sigma = _check_gradshap(n_samples, bank_sigma, sigma)
    bank = _gradshap_bank(baselines, bank_sigma, n_samples, seed, x)
    B = x.shape[0]
    dev = x.device
    inv_n = 1.0 / n_samples

    def fill(b, buf, first):
        return K.gradshap_images(x[b], bank, buf, sigma, seed, first)

    def accumulate(b, grads, acc, first):
        K.gradshap_accumulate(grads, x[b], bank, acc, sigma, seed, first, inv_n)

    def finish(b, acc, acc_sq, out, total):
        K.attr_finish(K.ATTR_MEAN, acc, inv_n=1.0, out=out, total=total)

    n = _num_outputs(model, x)
    per_image, cols = _class_columns(classes, B, n)
    Kc = 1 if per_image else len(cols)
    totals = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    attr = _path_method(model, x, n, per_image, cols, batch, n_samples, fill, None, False, finish, totals, accumulate,
                        route=route)
    if not return_delta:
        return attr
    delta = torch.zeros((B, Kc), dtype=torch.float32, device=dev)
    if Kc and B:
        R = int(bank.shape[0])
        cols_dev = torch.tensor(cols, dtype=torch.int64).to(dev)
        shares = _gradshap_shares(n_samples, R, seed, dev)
        with _eval_mode(model), torch.no_grad():
            logp = model(torch.cat([bank, x])).double()
        expected = shares @ logp[:R]                            # [n_outputs]: the bank's expected output under the draws
        gaps = logp[R:] - expected[None]
        ends = gaps.gather(1, cols_dev[:, None]) if per_image else gaps.index_select(1, cols_dev)
        delta = (totals - ends).float()
    return attr, delta


def layer_gradient_shap(model, images, classes=None, baselines=10, bank_sigma=1.0, n_samples=200, batch=256, seed=0,
                        return_attr=False, return_delta=False):
    """Layer GradientSHAP (captum's LayerGradientShap) of `images` [B, Cin, H, W] at the backbone's output, the layer `gradcam`
    reads -> fp32 [B, K, h, w] on the images' device.  With A = the features of images[b] (NHWC [h, w, C]), A_r the features of the
    bank's baseline IMAGE b_r, g(F) = d out[:, c_k] / dF the gradient of the head alone, and per sample s < n_samples a pick_s and
    a fraction alpha_s drawn from `seed` as in `gradient_shap`:
    d_s = A - A_pick_s,  attr[b, k] = (1 / n_samples) sum_s g(A_pick_s + alpha_s d_s) * d_s,  map[b, k, p] = sum_c attr[b, k, p, c],
    lines IN FEATURE SPACE.  There is NO noise option: noise on the image would move the end of every line through the backbone,
    one feature pass per sample, and the method would no longer live in the head.

    `baselines` and `bank_sigma` as in `gradient_shap` (a tensor [R, Cin, H, W] of baseline images, or an int R for the Gaussian
    bank); classes as in `gradcam`: None, a list of ints (K = len) or a LongTensor [B] (K = 1).  return_attr: also attr fp32
    [B, K, h, w, C]; return_delta: also fp32 [B, K], sum_p map - (out(A)[c] - sum_r (n_r / n_samples) out(A_r)[c]) in float64, a
    Monte-Carlo gap as in `gradient_shap`.  The results come in that order.

    The loop is that of `layer_integrated_gradients` with the new kernels: ONE SlotModel.feature_pass of the bank and the images
    gives A_r and A; per image the samples go through the head in chunks of `batch` -- kernels.gradshap_images (sigma = 0) into one
    reused feature buffer, ONE SlotModel.head_pass per chunk, per class one `.grad` with a one-hot column and one
    kernels.gradshap_accumulate onto that class's float64 sums in sample order -- then kernels.layer_attr_finish (mode LAYER_SUM)
    once per image for all K classes.  The gap comes from one head_pass of [A_0 .. A_{R-1}, A].  Nothing enters the backbone after
    the feature pass; nothing is copied to the host or synchronises inside the loop; no BatchNorm buffer moves and the caller's
    mode is restored; only head parameters get a `.grad`.  It needs a SlotModel (slot head or FC baseline).

    What departs from captum's LayerGradientShap: our random stream, the LOG-PROBABILITIES as output, one draw sequence for all
    images and classes, the channel SUM as the float map (as in `layer_integrated_gradients`), and no stdevs."""
    x, batch = _check_images_batch(images, batch)
    n_samples, bank_sigma, _ = _check_gradshap(n_samples, bank_sigma)
    bank = _gradshap_bank(baselines, bank_sigma, n_samples, seed, x)
    B, R = x.shape[0], int(bank.shape[0])
    n = _num_classes(model, x)
    per_image, cols = _class_columns(classes, B, n)
    dev = x.device
    inv_n = 1.0 / n_samples
    # (every upload comes before the first pass: a copy from the host waits for the work queued ahead of it)
    cols_dev = torch.tensor(cols, dtype=torch.int64).to(dev)
    onehots = _one_hot_rows(cols_dev, n)
    feats = _fp32_dense(model.feature_pass(torch.cat([bank, x])).features)
    _, h, w, C = feats.shape
    bank_feats = feats[:R]
    Kc = 1 if per_image else len(cols)
    out = torch.empty((B, Kc, h, w), dtype=torch.float32, device=dev)
    attr = torch.empty((B, Kc, h, w, C), dtype=torch.float32, device=dev) if return_attr else None
    totals = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    ends = torch.zeros((B, Kc), dtype=torch.float64, device=dev) if return_delta else None
    if Kc == 0 or B == 0:
        return _layer_results(out, attr, totals, ends, return_attr, return_delta)
    shares = _gradshap_shares(n_samples, R, seed, dev) if return_delta else None
    rows = min(batch, n_samples)
    buf = torch.empty((rows, h, w, C), dtype=torch.float32, device=dev)
    onehot = torch.empty((rows, n), dtype=torch.float32, device=dev)
    acc = torch.empty((Kc, h, w, C), dtype=torch.float64, device=dev)
    with _eval_mode(model):
        for b in range(B):
            A = feats[R + b]
            acc.zero_()
            for first in range(0, n_samples, batch):
                m = min(batch, n_samples - first)
                fp = model.head_pass(K.gradshap_images(A, bank_feats, buf[:m], 0.0, seed, first))
                for k in range(Kc):
                    onehot.copy_(onehots[b if per_image else k])  # (one launch: the row of the class, for every sample)
                    K.gradshap_accumulate(_fp32_dense(fp.grad(onehot[:m])), A, bank_feats, acc[k], 0.0, seed, first, inv_n)
                del fp
            K.layer_attr_finish(K.LAYER_SUM, acc, out[b], attr=None if attr is None else attr[b],
                                total=None if totals is None else totals[b])
            if return_delta:
                logp = model.head_pass(torch.cat([bank_feats, A[None]])).log_probs.double()
                ends[b] = (logp[R] - shares @ logp[:R]).index_select(0, cols_dev[b:b + 1] if per_image else cols_dev)
    return _layer_results(out, attr, totals, ends, return_attr, return_delta)


def layergradshap_maps(model, images, classes=None, size=None, min_level=0.0, **kwargs):
    """uint8 Layer GradientSHAP heat maps [B, K, H, W] on the device: `layer_gradient_shap` (its other keyword arguments pass
    through), then the drawing steps of `gradcam_maps` in one launch (kernels.cam_maps) at `size` = (H, W) (None: the images'
    H x W)."""
    H, W = _out_size(size, images)
    return K.cam_maps(layer_gradient_shap(model, images, classes, **kwargs), H, W, min_level)
