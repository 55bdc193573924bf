"""Grad-CAM at the last backbone stage (-m gpu): the two kernels of csrc/gradcam.hip against fp64 (kernels.gradcam with the
worst-case fp32 bound of any summation order, kernels.cam_maps against a float64 NumPy restatement of the reference's drawing
steps), SlotModel.feature_pass and tools/attribution.py gradcam on whole models against the CPU oracle's head evaluated at the
HIP path's own features, and gradcam_maps / test.py --cam true.

Model gradients are held to the project's per-tensor rule (tests/test_model_gpu.py pinned_gradient_check): the oracle's fp64
and fp32 autograd run under the conv1x1 sign pattern the HIP forward produced, and
|HIP - fp64| <= max(2 x |torch fp32 - fp64|, 1e-3 x max|.|)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import MODEL_CASES, LAMBDA, model_inputs             # noqa: E402


# ------------------------------------------------------------------------------------------------------ 1: K.gradcam
GRADCAM_SHAPES = [(1, 1, 1, 1), (2, 1, 1, 70), (3, 2, 3, 65), (2, 7, 7, 512), (2, 7, 7, 2048), (1, 9, 9, 2048), (2, 3, 3, 130),
                  # the routes of the column sums gradcam shares with gradcampp (MORE_SHAPES of test_gradcampp_gpu.py): at least
                  # as many columns as threads with and without 16-byte loads, and the largest C
                  (1, 4, 4, 4100), (1, 5, 5, 1030), (1, 5, 5, 8192)]
SENTINEL = -777.25


def _gradcam_operands(shape, seed=0):
    gen = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)


def _gradcam_fp64(feat, dfeat, relu):
    """(reference [B, N], bound [B, N]) in fp64: (N + C + 4) 2^-24 sum_c mean_p'|dfeat| |feat|"""
    B, h, w, C = feat.shape
    N = h * w
    f, d = feat.double().reshape(B, N, C), dfeat.double().reshape(B, N, C)
    ref = torch.einsum("bc,bpc->bp", d.mean(dim=1), f)
    if relu:
        ref = ref.clamp_min(0.0)
    bound = (N + C + 4) * 2.0 ** -24 * torch.einsum("bc,bpc->bp", d.abs().mean(dim=1), f.abs())
    return ref, bound


def _check_gradcam(shape, relu, seed=0):
    from scouter_amd import kernels as K
    B, h, w, C = shape
    feat, dfeat = _gradcam_operands(shape, seed)
    ref, bound = _gradcam_fp64(feat, dfeat, relu)
    fd, dd = feat.cuda(), dfeat.cuda()
    full = torch.full((B, 3, h, w), SENTINEL, device="cuda")
    K.gradcam(fd, dd, full[:, 1], relu=relu)
    again = torch.full((B, h * w), SENTINEL, device="cuda")
    K.gradcam(fd, dd, again, relu=relu)
    torch.cuda.synchronize()
    got = full[:, 1].reshape(B, h * w)
    assert torch.equal(got, again)                                      # two calls, two output strides: the same bits
    assert bool((full[:, 0] == SENTINEL).all()) and bool((full[:, 2] == SENTINEL).all())
    assert bool(torch.isfinite(got).all())
    err = (got.cpu().double() - ref).abs()
    print("gradcam", shape, "relu", relu, "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", GRADCAM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_gradcam_kernel_against_fp64(shape, relu):
    _check_gradcam(shape, relu)


# ------------------------------------------------------------------------------------------------------ 2: refusals
@pytest.mark.parametrize("bad", ["c0", "null", "misaligned", "c_too_large"])
def test_gradcam_kernel_refuses_bad_arguments(bad):
    """C = 0, a null pointer, a pointer off its alignment, more channels than the LDS plan holds: the library's error naming
    gradcam, nothing launched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    out = torch.full((2, 9), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="gradcam"):
        if bad == "c0":
            e = torch.empty((2, 3, 3, 0), device="cuda")
            K.gradcam(e, e.clone(), out)
        elif bad == "null":
            f = torch.ones((2, 3, 3, 8), device="cuda")
            _native.check(_native.lib().scouter_gradcam_f32(f.data_ptr(), None, out.data_ptr(), 2, 9, 8, 9, 0, None), "gradcam")
        elif bad == "misaligned":
            big = torch.ones(2 * 9 * 8 + 4, device="cuda")
            K.gradcam(big[1:1 + 144].view(2, 3, 3, 8), torch.ones((2, 3, 3, 8), device="cuda"), out)
        else:
            f = torch.ones((2, 3, 3, 8196), device="cuda")
            K.gradcam(f, f.clone(), out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    _check_gradcam((3, 2, 3, 65), False, seed=1)


# ------------------------------------------------------------------------------------------------------ 3: K.cam_maps
def _axis(n_in, n_out):
    """align_corners=False source positions of one axis: (lower index, upper index, weight of the upper one), float64"""
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum((d + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def _minmax64(a):
    span = a.max() - a.min()
    return (a - a.min()) / span if span > 0 else np.zeros_like(a)


def _cam_maps_restated(cam, H, W, min_level):
    """the six steps, one map at a time, in float64 -> (uint8 maps, per map: is the resized and clamped map non-constant)"""
    cam = np.asarray(cam, dtype=np.float64)
    M, h, w = cam.shape
    y0, y1, ty = _axis(h, H)
    x0, x1, tx = _axis(w, W)
    out = np.zeros((M, H, W), dtype=np.uint8)
    live = []
    for m in range(M):
        a = cam[m]
        # (the interpolation as a0 + t (a1 - a0): a constant map stays constant to the last bit, also in float64)
        top = a[y0][:, x0] + tx[None, :] * (a[y0][:, x1] - a[y0][:, x0])
        bot = a[y1][:, x0] + tx[None, :] * (a[y1][:, x1] - a[y1][:, x0])
        v = np.maximum(top + ty[:, None] * (bot - top), 0.0)
        live.append(bool(v.max() > v.min()) and min_level < 1.0)
        v = _minmax64(v)
        v = _minmax64(np.maximum(v, min_level))
        out[m] = (255.0 * v).astype(np.uint8)
    return out, live


CAM_SIZES = [(1, 1, 5, 7), (2, 3, 33, 47), (7, 7, 224, 224), (9, 9, 260, 260), (9, 9, 5, 7), (7, 7, 7, 7)]


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("min_level", [0.0, 0.3])
@pytest.mark.parametrize("size", CAM_SIZES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_cam_maps_against_numpy(size, min_level, M):
    from scouter_amd import kernels as K
    h, w, H, W = size
    cam = torch.randn((M, h, w), generator=torch.Generator().manual_seed(17 + M))
    got = K.cam_maps(cam.cuda(), H, W, min_level)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (M, H, W) and got.is_cuda
    got = got.cpu().numpy()
    want, live = _cam_maps_restated(cam.numpy(), H, W, min_level)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print("cam_maps", size, min_level, M, "max grey-level difference", int(diff.max()), "pixels off", int((diff > 0).sum()))
    assert diff.max() <= 1                                               # one grey level, the bar of the vis-map tests
    for m in range(M):
        if live[m]:
            assert got[m].max() >= 254 and got[m].min() == 0
        else:
            assert not got[m].any()
    if h * w > 1:
        assert any(live)


def test_cam_maps_edge_cases():
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(23)
    one = -torch.rand((7, 7), generator=gen)
    one[2, 4] = 0.8
    cams = torch.stack([torch.full((7, 7), 0.7), -torch.rand((7, 7), generator=gen) - 0.1, torch.zeros(7, 7), one]).cuda()
    for size in ((224, 224), (5, 3)):
        for min_level in (0.0, 0.3):
            a = K.cam_maps(cams, size[0], size[1], min_level)
            b = K.cam_maps(cams, size[0], size[1], min_level)
            torch.cuda.synchronize()
            assert torch.equal(a, b)
            a = a.cpu().numpy()
            assert not a[0].any() and not a[1].any() and not a[2].any()  # constant, all negative, all zero
            want, live = _cam_maps_restated(cams.cpu().numpy(), size[0], size[1], min_level)
            assert live == [False, False, False, size == (224, 224)]        # (5 x 3 samples step over the one positive pixel)
            assert np.abs(a.astype(np.int64) - want.astype(np.int64)).max() <= 1
            if live[3]:                                                      # one positive pixel: a non-zero map
                assert a[3].any() and a[3].max() >= 254 and a[3].min() == 0
    assert not K.cam_maps(cams, 32, 32, 1.0).cpu().numpy().any()        # min_level 1: constant at the second scaling
    lead = K.cam_maps(cams.view(2, 2, 7, 7), 16, 16, 0.0)                # leading dimensions are kept
    assert tuple(lead.shape) == (2, 2, 16, 16) and torch.equal(lead.view(4, 16, 16), K.cam_maps(cams, 16, 16, 0.0))


# ------------------------------------------------------------------------------------------------------ 4: whole models
def model_args(arch, C, spc, L, ls, power, mnist, use_slot=True):
    return argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=use_slot, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=ls,
                              power=power, to_k_layer=L, lambda_value=LAMBDA)


def build(case):
    """-> (model on the device, parameters, images, oracle head configuration or None for the FC baseline, architecture)"""
    from scouter_amd.sloter.slot_model import SlotModel
    if case == "fc_resnet18_mnist_64":
        spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
        P = O.synth_state(spec, 400)
        m = SlotModel(model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=False))
        m.load_state_dict(P)
        images, _ = O.synth_batch(4, 1, 64, 10, 401)
        return m.cuda(), P, images, None, "resnet18"
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist))
    m.load_state_dict(P)
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=float(LAMBDA))
    return m.cuda(), P, images, cfg, arch


def bn_buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def capture_conv1x1(m):
    """Arms conv1x1 (the head's only ReLU) to record its output; returns the dict it fills"""
    store = {}
    if m.use_slot:
        m.conv1x1._capture = (store, "conv1x1")
    return store


def oracle_head(P, cfg, feat_nhwc, store):
    """The oracle's head at the HIP path's own features, under its conv1x1 sign pattern, in fp64 and fp32:
    -> per dtype (d log_prob_c / d features [K, B, Cin, h, w], Grad-CAM [K, B, h, w])"""
    mask = (store["conv1x1"] > 0).permute(0, 3, 1, 2).cpu() if cfg is not None else None
    O.RELU_HOOK = lambda name, x: x * mask.to(x.dtype) if name == "conv1x1" else torch.relu(x)
    res = []
    try:
        for dtype in (torch.float64, torch.float32):
            Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
            feat = feat_nhwc.permute(0, 3, 1, 2).cpu().to(dtype).contiguous().requires_grad_(True)      # NCHW leaf
            if cfg is not None:
                out = O.head_forward(Pd, feat, None, cfg)
            else:       # the FC baseline after the backbone, as O.fc_model_forward states it
                out = F.log_softmax(F.linear(feat.mean(dim=(2, 3)), Pd["backbone.fc.weight"], Pd["backbone.fc.bias"]), dim=1)
            grads, cams = [], []
            for c in range(out.shape[1]):
                g, = torch.autograd.grad(out[:, c].sum(), feat, retain_graph=True)
                grads.append(g)
                cams.append((g.mean(dim=(2, 3), keepdim=True) * feat.detach()).sum(dim=1))
            res.append((torch.stack(grads), torch.stack(cams)))
    finally:
        O.RELU_HOOK = None
    return res


def check_rule(what, mine, ref64, ref32, kf=2.0, ks=1e-3):
    mine = mine.detach().cpu().double()
    assert mine.shape == ref64.shape, (what, mine.shape, ref64.shape)
    assert bool(torch.isfinite(mine).all())
    scale = float(ref64.abs().max())
    e = float((mine - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    print("%s: |HIP - fp64| = %.3e, |torch fp32 - fp64| = %.3e, max|.| = %.3e" % (what, e, e32, scale))
    assert scale > 0
    assert e <= max(kf * e32, ks * scale) + 1e-12, (what, e, e32, scale)


_FEATURES = {}       # case -> the oracle's eval-mode backbone output in (fp64, fp32): one run per model


def oracle_features(case, P, images, arch):
    if case not in _FEATURES:
        res = []
        with torch.no_grad():
            for dtype in (torch.float64, torch.float32):
                Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
                res.append(O.backbone_features(Pd, images.to(dtype), arch, training=False))
        _FEATURES[case] = tuple(res)
    return _FEATURES[case]


def check_against_oracle(case, m, P, images, cfg, arch, tag):
    """feature_pass (features, every one-hot .grad) and gradcam of every class against the oracle; returns gradcam's result"""
    from scouter_amd.tools.attribution import gradcam
    store = capture_conv1x1(m)
    fp = m.feature_pass(images.cuda())
    torch.cuda.synchronize()
    feat = fp.features
    B, n = images.shape[0], fp.log_probs.shape[1]
    assert feat.dtype == torch.float32 and feat.dim() == 4 and feat.shape[0] == B and feat.shape[3] == O.ARCHS[arch]["channel"]
    f64, f32 = oracle_features(case, P, images, arch)
    check_rule("%s %s features" % (case, tag), feat.permute(0, 3, 1, 2), f64, f32)
    (g64, c64), (g32, c32) = oracle_head(P, cfg, feat, store)
    seed = torch.zeros_like(fp.log_probs)
    for c in range(n):
        seed.zero_()
        seed[:, c] = 1.0
        d = fp.grad(seed)
        assert tuple(d.shape) == tuple(feat.shape) and d.dtype == torch.float32
        check_rule("%s %s .grad(class %d)" % (case, tag, c), d.permute(0, 3, 1, 2), g64[c], g32[c])
    again = fp.grad(seed)                                                # callable any number of times
    assert torch.equal(again, d)
    cam = gradcam(m, images.cuda())
    torch.cuda.synchronize()
    assert tuple(cam.shape) == (B, n) + tuple(feat.shape[1:3]) and cam.dtype == torch.float32 and cam.is_cuda
    for c in range(n):
        check_rule("%s %s gradcam(class %d)" % (case, tag, c), cam[:, c], c64[c], c32[c])
    return cam, (c64, c32)


@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96", "fc_resnet18_mnist_64"])
def test_feature_pass_and_gradcam_against_oracle(case):
    from scouter_amd.tools.attribution import gradcam
    m, P, images, cfg, arch = build(case)
    m.train()
    before = bn_buffers(m)
    cam, (c64, c32) = check_against_oracle(case, m, P, images, cfg, arch, "unfolded")
    assert m.training                                                    # the caller's mode is back
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    # head parameters that require grad got a gradient, the backbone's did not
    named = dict(m.named_parameters())
    head = [k for k in named if (k.startswith("backbone.fc.") if cfg is None else not k.startswith("backbone."))
            and "to_q" not in k]
    assert head and all(named[k].grad is not None for k in head)
    assert all(p.grad is None for k, p in named.items() if k not in head)
    # a list of classes: the same columns, bit for bit
    B, n = cam.shape[:2]
    two = gradcam(m, images.cuda(), classes=[0, 3])
    assert tuple(two.shape) == (B, 2) + tuple(cam.shape[2:]) and torch.equal(two[:, 0], cam[:, 0]) and torch.equal(two[:, 1], cam[:, 3])
    # one class per image: the diagonal entries, to the rule
    cls = (torch.arange(B) * 3 + 1) % n
    own = gradcam(m, images.cuda(), classes=cls)
    assert tuple(own.shape) == (B, 1) + tuple(cam.shape[2:])
    idx = torch.arange(B)
    check_rule(case + " gradcam(per-image classes)", own[:, 0], c64[cls, idx], c32[cls, idx])
    rel = gradcam(m, images.cuda(), classes=[3], relu=True)
    assert torch.equal(rel[:, 0], cam[:, 3].clamp_min(0.0))
    for bad in ([n], [-1], torch.tensor([0] * (B - 1) + [n])):
        with pytest.raises(IndexError):
            gradcam(m, images.cuda(), classes=bad)
    # BatchNorm-folded features: the same oracle gate
    m.eval()
    m.set_inference_fold(True)
    check_against_oracle(case, m, P, images, cfg, arch, "folded")
    assert not m.training
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("case", ["resnet18_mnist_64", "fc_resnet18_mnist_64"])
def test_gradcam_with_nothing_trainable(case):
    from scouter_amd.tools.attribution import gradcam
    m, P, images, cfg, arch = build(case)
    m.requires_grad_(False)
    for fold in (False, True):
        m.set_inference_fold(fold)
        cam = gradcam(m, images.cuda(), classes=[1, 2])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(cam).all()) and float(cam.abs().max()) > 0
        assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------------ 5: maps and the CLI
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_gradcam_maps_and_test_tool(use_slot, tmp_path, monkeypatch):
    """gradcam_maps is K.cam_maps of gradcam, bytewise; scouter_amd.test --cam true writes cam_0.png .. cam_9.png, 64 x 64,
    byte for byte gradcam_maps of the image"""
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools.attribution import gradcam, gradcam_maps
    torch.manual_seed(11)
    args = model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=use_slot)
    args.device, args.grad_min_level = "cuda", 0.2
    model = SlotModel(args).to(args.device)
    image = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))
    vis_dir = str(tmp_path / "vis")
    maps = T.run_cam(args, model, image, vis_dir)
    want = gradcam_maps(model, image[None].cuda(), min_level=0.2)
    assert want.dtype == torch.uint8 and want.is_cuda and tuple(want.shape) == (1, 10, 64, 64)
    assert torch.equal(want, K.cam_maps(gradcam(model, image[None].cuda()), 64, 64, 0.2))
    small = gradcam_maps(model, image[None].cuda(), classes=[2, 5], size=(20, 30))
    assert tuple(small.shape) == (1, 2, 20, 30)
    assert torch.equal(small, K.cam_maps(gradcam(model, image[None].cuda(), classes=[2, 5]), 20, 30, 0.0))
    want = want[0].cpu().numpy()
    assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and np.array_equal(maps, want)
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(vis_dir, "cam_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
    assert not os.path.exists(os.path.join(vis_dir, "cam_10.png"))
    assert any(m.any() for m in want)
    # the command line: the flag writes the same set of files (random weights: no checkpoint under the empty output_dir)
    cli_dir = str(tmp_path / "cli")
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "true" if use_slot else "false", "--pre_trained", "false",
        "--img_size", "64", "--cam", "true", "--grad_min_level", "0.2", "--eval_fold", "true", "--vis_dir", cli_dir,
        "--output_dir", str(tmp_path / "none")])
    T.main()
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(cli_dir, "cam_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8
    assert not os.path.exists(os.path.join(cli_dir, "cam_10.png")) and not os.path.exists(os.path.join(cli_dir, "grad_0.png"))
