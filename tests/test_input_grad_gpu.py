"""Gradient with respect to the input image (-m gpu): the stem input-gradient kernel (and the stem layer's weight gradient)
against fp64, `x.grad` of the whole model against the CPU oracle with `images` as a leaf (train mode, frozen stages, eval mode
with nothing trainable, the FC baseline), and the attribution tools on top of it (tools/attribution.py, test.py --grad true).

Model gradients are held to the project's per-tensor rule (tests/test_model_gpu.py pinned_gradient_check), with x.grad as
one more tensor: the oracle's fp64 and fp32 autograd run under the sign pattern and max-pool windows the HIP forward
produced, and  |HIP - fp64| <= max(2 x |torch fp32 - fp64|, 1e-3 x max|grad|)."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import MODEL_CASES, LAMBDA, model_inputs             # noqa: E402


# ------------------------------------------------------------------------------------------------------ helpers
def model_args(arch, C, spc, L, ls, power, mnist, use_slot=True):
    return argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=use_slot, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=ls,
                              power=power, to_k_layer=L, lambda_value=LAMBDA)


def build(case):
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist))
    m.load_state_dict(P)
    return m.cuda(), P, images, labels


def case_cfg(case):
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    return dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=float(LAMBDA))


def capture_relu_signs(m):
    """Arms every BatchNorm2d(+ReLU) of the HIP model (and conv1x1) to record its output, the backbone to record the stem
    max-pool's window indices; returns the dict (name -> NHWC tensor)."""
    from scouter_amd.nn_hip import BatchNorm2d, Conv2d
    store = {}
    for name, mod in m.named_modules():
        if isinstance(mod, BatchNorm2d) or (isinstance(mod, Conv2d) and name == "conv1x1"):
            mod._capture = (store, name)
    m.backbone._capture = (store, "maxpool")
    return store


def pattern(signs):
    """(ReLU masks {name: bool NCHW}, pool window indices [B, C, Ho, Wo]) on the CPU, from capture_relu_signs' dict"""
    signs = dict(signs)
    pool_arg = signs.pop("maxpool").permute(0, 3, 1, 2).cpu()
    return {k: (v > 0).permute(0, 3, 1, 2).cpu() for k, v in signs.items()}, pool_arg


_ORACLE = {}     # key -> (masks, pool_arg, fp64 gradient, fp32 gradient): one oracle run per (model, mode, objective)


def oracle_input_grad(key, P, images, scalar, masks, pool_arg):
    """d scalar(P, x) / d x at x = images by the oracle's autograd, in fp64 and in fp32, under the given sign pattern and
    pool windows.  `scalar(P, x)` -> 0-dim tensor.  Cached under `key` as long as the pattern is the same."""
    hit = _ORACLE.get(key)
    if hit is not None and hit[0].keys() == masks.keys() and torch.equal(hit[1], pool_arg) and \
            all(torch.equal(hit[0][k], masks[k]) for k in masks):
        return hit[2], hit[3]
    O.MAXPOOL_HOOK = lambda x: O.maxpool_with_indices(x, pool_arg)
    O.RELU_HOOK = lambda name, x: x * masks[name].to(x.dtype) if name in masks else torch.relu(x)
    try:
        grads = []
        for dtype in (torch.float64, torch.float32):
            Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
            x = images.to(dtype).clone().requires_grad_(True)
            scalar(Pd, x).backward()
            grads.append(x.grad.detach())
    finally:
        O.RELU_HOOK = None
        O.MAXPOOL_HOOK = None
    _ORACLE[key] = (masks, pool_arg, grads[0], grads[1])
    return grads[0], grads[1]


def check_input_grad(what, mine, g64, g32, kf=2.0, ks=1e-3):
    mine = mine.detach().cpu().double()
    assert mine.shape == g64.shape, (mine.shape, g64.shape)
    assert bool(torch.isfinite(mine).all())
    scale = float(g64.abs().max())
    e = float((mine - g64).abs().max())
    e32 = float((g32.double() - g64).abs().max())
    print("%s: |HIP - fp64| = %.3e, |torch fp32 - fp64| = %.3e, max|grad| = %.3e" % (what, e, e32, scale))
    assert scale > 0
    assert e <= max(kf * e32, ks * scale) + 1e-12, (what, e, e32, scale)


def loss_scalar(cfg, labels):
    return lambda P, x: O.slot_model_forward(P, x, labels, cfg, training=True)[1][0]


def class_scalar(cfg, cls):
    def f(P, x):
        out = O.slot_model_forward(P, x, None, cfg, training=False)
        return out[torch.arange(out.shape[0]), cls].sum()
    return f


def bn_buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


# ------------------------------------------------------------------------------------------------------ 1: the kernel
STEM_CASES = [  # Cin, Cout, k, stride, pad, B, H, W
    (3, 64, 7, 2, 3, 2, 37, 45), (3, 64, 7, 2, 3, 3, 64, 64), (3, 64, 7, 2, 3, 1, 9, 300),
    (1, 64, 3, 2, 1, 2, 28, 28), (1, 64, 3, 2, 1, 2, 33, 30),
    (3, 32, 3, 2, 1, 2, 96, 96), (3, 32, 3, 2, 1, 1, 35, 41),
]


def _stem_operands(Cin, Cout, k, stride, pad, B, H, W, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn((B, Cout, Ho, Wo), generator=gen)              # NCHW, unit normal
    w = torch.randn((Cout, Cin, k, k), generator=gen)               # OIHW
    return dy, w


@pytest.mark.parametrize("shape", STEM_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_stem_dgrad_against_fp64(shape):
    """dx against torch.nn.grad.conv2d_input on the CPU in fp64; the project's input-gradient tolerance
    (tests/test_kernels_gpu.py: atol 2e-5 sqrt(Cout k k), rtol 1e-5); two calls give the same bits."""
    from scouter_amd import kernels as K
    Cin, Cout, k, stride, pad, B, H, W = shape
    dy, w = _stem_operands(*shape)
    ref = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy.double(), stride=stride, padding=pad)
    dyd = dy.permute(0, 2, 3, 1).contiguous().cuda()                # NHWC
    wd = w.permute(2, 3, 1, 0).contiguous().cuda()                  # HWIO
    a = K.stem_dgrad(dyd, wd, (B, Cin, H, W), k, stride, pad)
    b = K.stem_dgrad(dyd, wd, (B, Cin, H, W), k, stride, pad)
    torch.cuda.synchronize()
    assert a.shape == (B, Cin, H, W) and a.dtype == torch.float32 and a.is_contiguous()
    assert torch.equal(a, b)
    err = (a.cpu().double() - ref).abs()
    atol, rtol = 2e-5 * math.sqrt(Cout * k * k), 1e-5
    print("stem_dgrad", shape, "max err %.3e (atol %.3e)" % (float(err.max()), atol))
    assert bool((err <= atol + rtol * ref.abs()).all()), float(err.max())


@pytest.mark.parametrize("bad", [(32, 64, 3, 2, 1), (3, 64, 3, 3, 1)], ids=["cin32", "stride3"])
def test_stem_dgrad_rejects_unsupported_shapes(bad):
    """Cin = 32 / stride 3: the library's error, nothing launched, and the device goes on working"""
    from scouter_amd import kernels as K
    Cin, Cout, k, stride, pad = bad
    B, H, W = 1, 17, 19
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.ones((B, Ho, Wo, Cout), device="cuda")
    w = torch.ones((k, k, Cin, Cout), device="cuda")
    with pytest.raises(RuntimeError, match="stem_dgrad"):
        K.stem_dgrad(dy, w, (B, Cin, H, W), k, stride, pad)
    torch.cuda.synchronize()
    good = (1, 64, 3, 2, 1, 2, 28, 28)
    dy, w = _stem_operands(*good)
    out = K.stem_dgrad(dy.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(2, 3, 1, 0).contiguous().cuda(),
                       (2, 1, 28, 28), 3, 2, 1)
    ref = torch.nn.grad.conv2d_input((2, 1, 28, 28), w.double(), dy.double(), stride=2, padding=1)
    assert float((out.cpu().double() - ref).abs().max()) <= 2e-5 * math.sqrt(64 * 9) + 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("shape", [(4, 64, 64), (3, 45, 51)])
def test_stem_layer_weight_gradient_against_fp64(shape):
    """nn_hip.StemConv2d (the deep stem's 3 -> 32 layer; the second shape has an odd height and width): the weight gradient
    -- the saved patch rows through the generic weight-gradient kernel -- against fp64 autograd, 2e-5 x max(1, max|g|), and bit
    for bit the same on its side stream and on the compute stream."""
    from scouter_amd import kernels as K
    from scouter_amd import nn_hip
    B, H, W = shape
    torch.manual_seed(11)
    m = nn_hip.StemConv2d(3, 32, 3, 2, 1).cuda()
    x = torch.randn(B, 3, H, W, device="cuda")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Ho, Wo, 32, device="cuda")
    dw = {}
    for side in (True, False):
        m.use_side_stream = side
        m._dw = torch.zeros(3, 3, 3, 32, device="cuda")
        _, ctx = m.fwd(x, True, bn_stats=True)
        assert tuple(ctx.shape) == (B, 3, H, W) and tuple(ctx.x.shape) == (B, Ho, Wo, m.kpad)
        m.bwd(dy, ctx)
        K.join_side_stream(x.device)
        torch.cuda.synchronize()
        dw[side] = m._dw.clone()
    assert torch.equal(dw[True], dw[False])
    wd = m.weight.detach().double().requires_grad_()
    g, = torch.autograd.grad(torch.nn.functional.conv2d(x.double(), wd, None, 2, 1), wd, dy.double().permute(0, 3, 1, 2))
    got = dw[True].double().permute(3, 2, 0, 1)                                           # HWIO -> OIHW
    err = float((got - g).abs().max())
    print("stem layer dW", shape, "max err %.3e (max|g| %.3e)" % (err, float(g.abs().max())))
    assert err <= 2e-5 * max(1.0, float(g.abs().max()))


# ------------------------------------------------------------------------------------------------------ 2: train mode
@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96"])
def test_input_grad_train_mode(case):
    m, P, images, labels = build(case)
    m.train()
    signs = capture_relu_signs(m)
    x = images.cuda().requires_grad_(True)
    out, losses = m(x, labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    masks, pool_arg = pattern(signs)
    arena = m.grad_arena().flat.clone()
    g64, g32 = oracle_input_grad((case, "train"), P, images, loss_scalar(case_cfg(case), labels), masks, pool_arg)
    check_input_grad(case + " train x.grad", x.grad, g64, g32)
    # the parameter gradients do not notice: the same model and inputs without requires_grad on x, same bits
    m.zero_grad(set_to_none=True)
    out2, losses2 = m(images.cuda(), labels.cuda())
    losses2[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    assert torch.equal(m.grad_arena().flat, arena)


# ------------------------------------------------------------------------------------------------------ 3: frozen stages
def test_input_grad_through_frozen_stages():
    case = "resnest26d_96"
    m, P, images, labels = build(case)
    for mod in (m.backbone.conv1, m.backbone.bn1, m.backbone.layer1, m.backbone.layer2):
        mod.requires_grad_(False)
    m.train()
    signs = capture_relu_signs(m)
    x = images.cuda().requires_grad_(True)
    out, losses = m(x, labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    masks, pool_arg = pattern(signs)
    g64, g32 = oracle_input_grad((case, "train"), P, images, loss_scalar(case_cfg(case), labels), masks, pool_arg)
    check_input_grad(case + " frozen stem/layer1/layer2 x.grad", x.grad, g64, g32)      # (does not depend on what trains)
    named = dict(m.named_parameters())
    frozen = [k for k, p in named.items() if not p.requires_grad]
    assert frozen and all(named[k].grad is None for k in frozen)
    got = {k: p.grad.clone() for k, p in named.items() if p.requires_grad and "to_q" not in k}
    assert got and all(k.startswith(("backbone.layer3", "backbone.layer4", "conv1x1", "slot")) for k in got)
    m.zero_grad(set_to_none=True)
    out2, losses2 = m(images.cuda(), labels.cuda())
    losses2[0].backward()
    torch.cuda.synchronize()
    for k, g in got.items():
        assert torch.equal(named[k].grad, g), k
    assert all(named[k].grad is None for k in frozen)


# ------------------------------------------------------------------------------------------------------ 4: eval mode
@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96"])
def test_input_grad_eval_mode_nothing_trainable(case):
    m, P, images, labels = build(case)
    m.requires_grad_(False)
    m.eval()
    B, C = images.shape[0], MODEL_CASES[case][1]
    cls = (torch.arange(B) * 3 + 1) % C
    before = bn_buffers(m)
    signs = capture_relu_signs(m)
    grads = []
    for fold in (False, True):
        m.set_inference_fold(fold)
        x = images.cuda().requires_grad_(True)
        out = m(x)
        out[torch.arange(B, device="cuda"), cls.cuda()].sum().backward()
        torch.cuda.synchronize()
        assert x.grad is not None
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])                  # the input-gradient route ignores the fold
    masks, pool_arg = pattern(signs)
    g64, g32 = oracle_input_grad((case, "eval", tuple(cls.tolist())), P, images, class_scalar(case_cfg(case), cls), masks,
                                 pool_arg)
    check_input_grad(case + " eval x.grad", grads[0], g64, g32)
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------------ 5: FC baseline
def test_input_grad_fc_baseline():
    from scouter_amd.sloter.slot_model import SlotModel
    spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
    P = O.synth_state(spec, 400)
    m = SlotModel(model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=False))
    m.load_state_dict(P)
    m = m.cuda().train()
    images, labels = O.synth_batch(4, 1, 64, 10, 401)
    signs = capture_relu_signs(m)
    x = images.cuda().requires_grad_(True)
    out, losses = m(x, labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    masks, pool_arg = pattern(signs)
    g64, g32 = oracle_input_grad(("fc_resnet18_mnist_64", "train"), P, images,
                                 lambda Q, xx: O.fc_model_forward(Q, xx, labels, "resnet18", training=True)[1][0], masks,
                                 pool_arg)
    check_input_grad("FC baseline x.grad", x.grad, g64, g32)


# ------------------------------------------------------------------------------------------------------ 6: tools
def test_input_gradients_tool():
    from scouter_amd.tools.attribution import input_gradients
    case = "resnet18_mnist_64"
    m, P, images, labels = build(case)
    m.train()
    images = images[:2]
    before = bn_buffers(m)
    signs = capture_relu_signs(m)
    g = input_gradients(m, images.cuda(), classes=[0, 3])
    torch.cuda.synchronize()
    assert m.training                                        # the caller's mode is back
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert tuple(g.shape) == (2, 2, 1, 64, 64) and g.dtype == torch.float32
    masks, pool_arg = pattern(signs)                          # (the same pattern for every class: one eval forward each)
    for j, c in enumerate([0, 3]):
        cls = torch.full((2,), c, dtype=torch.long)
        g64, g32 = oracle_input_grad((case, "eval2", c), P, images, class_scalar(case_cfg(case), cls), masks, pool_arg)
        check_input_grad("input_gradients class %d" % c, g[:, j], g64, g32)
    every = input_gradients(m.eval(), images.cuda())
    assert tuple(every.shape) == (2, 10, 1, 64, 64) and torch.equal(every[:, 3], g[:, 1]) and not m.training
    loss_g = input_gradients(m, images.cuda(), of="loss", target=labels[:2].cuda())
    assert tuple(loss_g.shape) == (2, 1, 1, 64, 64) and bool(torch.isfinite(loss_g).all()) and float(loss_g.abs().max()) > 0


def _maps_restated(g, min_level):
    """float64 NumPy restatement of the attribution post-processing, one map at a time"""
    g = np.asarray(g, dtype=np.float64)
    out = np.zeros(g.shape[:2] + g.shape[3:], dtype=np.float64)
    for b in range(g.shape[0]):
        for k in range(g.shape[1]):
            a = np.maximum(g[b, k].mean(axis=0), 0.0)
            for floor in (None, min_level):
                if floor is not None:
                    a = np.maximum(a, floor)
                a = a - a.min()
                a = a / a.max() if a.max() > 0 else np.zeros_like(a)
            out[b, k] = a * 255.0
    return out


@pytest.mark.parametrize("shape,min_level", [((2, 3, 3, 33, 47), 0.0), ((2, 3, 3, 33, 47), 0.3), ((1, 1, 5, 7), 0.0),
                                             ((1, 1, 5, 7), 0.3), ((1, 2, 1, 64, 64), 0.3)],
                         ids=["3ch_33x47_min0", "3ch_33x47_min0.3", "1x1x5x7_min0", "1x1x5x7_min0.3", "1ch_64_min0.3"])
def test_attribution_maps_against_numpy(shape, min_level):
    from scouter_amd.tools.attribution import attribution_maps
    if len(shape) == 4:                                       # a 1 x 1 x 5 x 7 gradient: one image, one channel, one class
        shape = (1,) + shape
    g = torch.randn(shape, generator=torch.Generator().manual_seed(7))
    maps = attribution_maps(g.cuda(), min_level=min_level)
    assert maps.dtype == np.uint8 and maps.shape == (shape[0], shape[1]) + shape[3:]
    want = _maps_restated(g.numpy(), min_level)
    assert np.abs(maps.astype(np.float64) - want).max() <= 1.0       # one grey level, the bar of the vis-map test
    assert maps.max() >= 254 and maps.min() == 0


def test_attribution_maps_constant_gradient_is_zero():
    from scouter_amd.tools.attribution import attribution_maps
    for value in (0.0, 0.7, -2.0):
        for min_level in (0.0, 0.3):
            with np.errstate(divide="raise", invalid="raise"):                  # no 0 / 0 on the way
                maps = attribution_maps(torch.full((1, 2, 3, 9, 11), value), min_level=min_level)
            assert maps.shape == (1, 2, 9, 11) and maps.dtype == np.uint8 and not maps.any()


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_test_tool_writes_grad_maps(use_slot, tmp_path):
    """scouter_amd.test --grad true: grad_0.png .. grad_9.png, 64 x 64, byte for byte attribution_maps of input_gradients"""
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools.attribution import attribution_maps, input_gradients
    torch.manual_seed(11)
    args = model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=use_slot)
    args.device, args.grad_min_level = "cuda", 0.2
    model = SlotModel(args).to(args.device)
    image = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))
    vis_dir = str(tmp_path / "vis")
    out, pred, slot_maps, ratio = T.run(args, model, image, vis_dir)
    assert out.shape == (10,) and 0 <= pred < 10 and len(slot_maps) == (10 if use_slot else 0)
    maps = T.run_grad(args, model, image, vis_dir)
    want = attribution_maps(input_gradients(model, image[None].cuda()), min_level=0.2)[0]
    assert maps.shape == (10, 64, 64) and np.array_equal(maps, want)
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(vis_dir, "grad_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
    assert not os.path.exists(os.path.join(vis_dir, "grad_10.png"))
    assert any(m.any() for m in want)
