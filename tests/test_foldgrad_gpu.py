"""The gradient-only backward of the BatchNorm-folded eval path (-m gpu): the three kernels of csrc/fold_bwd.hip against the float64
restatements of tests/foldgrad_restatements.py (or, for the pool, against the two kernels it restates, bit for bit), their refusals,
SlotModel.image_pass on whole models against the CPU oracle's fp64 and fp32 eval-mode autograd under the pass's own sign pattern
(the project's rule), the route="folded" of tools/attribution.py against the definition over the pass's own gradients, and
scouter_amd/tools/foldgrad.py in both modes.

Bounds.  EPS = 2^-24.  A fixed-order fp32 sum of n terms whose longest chain of additions has length L, each term one rounding
away from exact (an fma adds none), is within (L + 2) EPS sum|terms| -- the project's form; L is counted from the kernel's layout by
foldgrad_restatements.row_chain / hidden_chain.
sa_gate_bwd     h: the forward's fc1 column, (L_h + 2) EPS (sum|gap w1| + |b1|).  The test's gap, w1 and b1 are multiples of 1 / 8
                of small magnitude, so every pre-activation is exact in fp32 AND in float64: the mask [h > 0] is exact, with
                pre-activations that are exactly 0 and negative ones among them.
                dz = a (da - dot): three roundings in dot (two products, their sum; 3 EPS S, S = |a0 da0| + |a1 da1|), one in the
                difference, one in the product: EPS (3 |a| S + 3 |dz|) to first order (the second 3 rounds 2 up over the higher orders).
                dh = dz . w2^T: (L_2 + 2) EPS sum|dz w2| for its own sum plus sum dz_err |w2| handed down.
                dgap = dh . w1^T: (L_1 + 2) EPS sum|dh w1| plus sum dh_err |w1|: the bound is summed over the two dot products.
sa_apply_relu_bwd   1 / HW rounds once and its product with dgap once; dout a + that rounds at most twice (once under an fma):
                3 EPS (|dout a| + |dgap| / HW), the issue's bound, and an exact +0 under the mask.
maxpool_relu_bwd    selects and sums of the same operands in the same order as maxpool_bwd then relu_bwd: the same bits.
whole models    the project's rule |HIP - fp64| <= max(2 |torch fp32 - fp64|, 1e-3 max|grad|) (tests/test_input_grad_gpu.py).
library         the tools add the pass's fp32 gradients in float64 and round once: 4 EPS of the magnitudes for IG and SmoothGrad
                (tests/test_pathgrad_gpu.py), EPS |ref| + (n + 4) 2^-53 mag for GradientSHAP (tests/test_gradshap_gpu.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import foldgrad_restatements as R                                           # noqa: E402
from oracle import torch_oracle as O                                        # noqa: E402
from test_input_grad_gpu import check_input_grad, class_scalar, oracle_input_grad               # noqa: E402
from test_layer_gpu import SENTINEL, U, bn_buffers, build, dev, one_hot, rand                    # noqa: E402

EPS = 2.0 ** -24
SC_ERR_ARG, SC_ERR_UNSUPPORTED = -1, -3


def KK():
    from scouter_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------------ 1: sa_gate_bwd
def eighths(shape, seed, lim=8):
    """multiples of 1 / 8 in [-lim / 8, lim / 8]: products and sums of a few hundred of them are exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 8.0


def gate_inputs(Cp, A, B, seed=0):
    gap, w1 = eighths((B, Cp), 10 + seed), eighths((Cp, A), 20 + seed)
    b1 = eighths((A,), 30 + seed, 64)
    pre = (gap.double() @ w1.double())                                      # exact
    b1[0] = -float(pre[0, 0])                                               # image 0, column 0: a pre-activation of exactly 0
    b1[1] = -float(pre[0, 1]) - 0.125                                       # ... column 1: exactly -1 / 8
    b1[2] = -float(pre[B - 1, 2]) + 0.125                                   # the last image, column 2: exactly +1 / 8
    w2 = rand((A, 2 * Cp), 40 + seed)
    z = rand((B, 2, Cp), 50 + seed)
    a = torch.softmax(z, dim=1).reshape(B, 2 * Cp).contiguous()
    da = rand((B, 2 * Cp), 60 + seed)
    return gap, w1, b1, w2, a, da


GATE_SHAPES = [(64, 32), (8, 256), (128, 64), (512, 256)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cp,A", GATE_SHAPES, ids=["%dx%d" % s for s in GATE_SHAPES])
def test_sa_gate_bwd_against_fp64(Cp, A, B):
    K = KK()
    gap, w1, b1, w2, a, da = gate_inputs(Cp, A, B)
    ref = R.sa_gate_bwd(gap, w1, b1, w2, a, da)
    assert float(ref["pre"][0, 0]) == 0.0 and float(ref["pre"][0, 1]) == -0.125 and float(ref["pre"][B - 1, 2]) == 0.125
    assert bool((ref["pre"] < 0).any()) and bool((ref["pre"] > 0).any())
    t = {n: dev(v, 0, 0)[0] for n, v in (("gap", gap), ("w1", w1.view(1, 1, Cp, A)), ("b1", b1), ("w2", w2.view(1, 1, A, 2 * Cp)),
                                         ("a", a), ("da", da))}
    dgap, dtail = dev(torch.zeros((B, Cp)), 0, 8)
    h, htail = dev(torch.zeros((B, A)), 0, 8)
    from scouter_amd import _native
    lib = _native.lib()

    def call(dg, hh, nb=B, first=0):
        rows = lambda x, w: x[first:first + nb].data_ptr()
        _native.check(lib.scouter_sa_gate_bwd_f32(rows(t["gap"], Cp), t["w1"].data_ptr(), t["b1"].data_ptr(), t["w2"].data_ptr(),
                                                  rows(t["a"], 2 * Cp), rows(t["da"], 2 * Cp), dg.data_ptr(),
                                                  None if hh is None else hh.data_ptr(), nb, Cp, A, None), "sa_gate_bwd")
    call(dgap, h)
    torch.cuda.synchronize()
    assert bool((dtail == SENTINEL).all()) and bool((htail == SENTINEL).all())          # sentinels behind every output
    # the hidden activation: the forward's column, and here exact
    herr, hbound = (h.cpu().double() - ref["h"]).abs(), (R.hidden_chain(Cp, A) + 2) * EPS * ref["pre_mag"]
    assert bool((herr <= hbound).all())
    assert torch.equal(h.cpu() > 0, ref["pre"] > 0)                                     # the mask is exact
    assert float(h[0, 0]) == 0.0 and float(h[0, 1]) == 0.0 and float(h[B - 1, 2]) == 0.125
    # dgap: its own dot product, and the error of dh -- its own dot product and dz's roundings -- handed down through |w1|
    L2, L1 = R.row_chain(2 * Cp), R.row_chain(A)
    dh_err = ref["dh_in"] + (L2 + 2) * EPS * ref["dh_mag"]
    bound = dh_err @ w1.double().abs().t() + (L1 + 2) * EPS * ref["dgap_mag"]
    err = (dgap.cpu().double() - ref["dgap"]).abs()
    print("sa_gate_bwd Cp %d A %d B %d: chains %d / %d / %d, max err %.3e, max err / bound %.3f"
          % (Cp, A, B, R.hidden_chain(Cp, A), L2, L1, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool(torch.isfinite(dgap).all()) and bool((err <= bound).all())
    assert float(ref["dgap"].abs().max()) > 0
    # the wrapper: the same bits, with and without h; a repeat repeats
    d2, h2 = K.sa_gate_bwd(t["gap"], t["w1"], t["b1"], t["w2"], t["a"], t["da"], want_h=True)
    d3 = K.sa_gate_bwd(t["gap"], t["w1"], t["b1"], t["w2"], t["a"], t["da"])
    assert torch.equal(d2, dgap) and torch.equal(h2, h) and torch.equal(d3, dgap)
    # a row alone is the row of the batch, bit for bit
    for b in range(B):
        one, oh = torch.zeros((1, Cp), device="cuda"), torch.zeros((1, A), device="cuda")
        call(one, oh, 1, b)
        assert torch.equal(one[0], dgap[b]) and torch.equal(oh[0], h[b]), b


def test_sa_gate_bwd_refusals():
    from scouter_amd import _native
    K, lib = KK(), _native.lib()
    gap, w1, b1, w2, a, da = (v.cuda() for v in gate_inputs(64, 32, 2))
    out = torch.full((2, 64), SENTINEL, device="cuda")
    ptrs = [gap, w1, b1, w2, a, da, out]
    for Cp, A in ((40, 32), (1024, 256)):
        rc = lib.scouter_sa_gate_bwd_f32(*[p.data_ptr() for p in ptrs], None, 2, Cp, A, None)
        assert rc == SC_ERR_UNSUPPORTED and b"sa_gate_bwd" in lib.scouter_last_error()
        assert not K.sa_gate_eligible(Cp, A)
    for i in range(len(ptrs)):                                              # every null pointer (h_out alone may be null)
        args = [None if j == i else p.data_ptr() for j, p in enumerate(ptrs)]
        assert lib.scouter_sa_gate_bwd_f32(*args, None, 2, 64, 32, None) == SC_ERR_ARG, i
    for shape in ((0, 64, 32), (2, 0, 32), (2, 64, 0)):
        assert lib.scouter_sa_gate_bwd_f32(*[p.data_ptr() for p in ptrs], None, *shape, None) == SC_ERR_ARG
    assert lib.scouter_sa_gate_bwd_f32(gap.data_ptr(), w1.data_ptr() + 4, *[p.data_ptr() for p in ptrs[2:]], None, 2, 64, 32,
                                       None) == SC_ERR_ARG                  # the weights are read as 16-byte vectors
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                    # nothing was launched
    with pytest.raises(RuntimeError, match="gap"):
        K.sa_gate_bwd(gap.cpu(), w1.view(1, 1, 64, 32), b1, w2.view(1, 1, 32, 128), a, da)
    got = K.sa_gate_bwd(gap, w1.view(1, 1, 64, 32), b1, w2.view(1, 1, 32, 128), a, da)          # and the device goes on working
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ 2: sa_apply_relu_bwd
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 45, 49])
@pytest.mark.parametrize("Cp", [4, 64, 512])
def test_sa_apply_relu_bwd_against_fp64(Cp, HW, B):
    K = KK()
    dout, a, dgap = rand((B, HW, Cp), 1), torch.rand((B, 2 * Cp), generator=torch.Generator().manual_seed(2)), rand((B, Cp), 3)
    x0 = rand((B, HW, 2 * Cp), 4).clamp_min(0.0)                            # a ReLU's output: about half of it +0
    x0.view(-1)[0], x0.view(-1)[1], x0.view(-1)[2] = -0.0, 0.0, 2.0 ** -149  # -0 and +0 mask, the smallest subnormal does not
    x0.view(-1)[3] = -1.0
    ref, mag, keep = R.sa_apply_relu_bwd(dout, a, dgap, x0)
    assert not bool(keep.view(-1)[0]) and not bool(keep.view(-1)[1]) and bool(keep.view(-1)[2]) and not bool(keep.view(-1)[3])
    dd, ad, gd, xd = (dev(v)[0] for v in (dout, a, dgap, x0))
    dx, tail = dev(torch.full((B, HW, 2 * Cp), 5.0), 0, 8)
    from scouter_amd import _native
    _native.check(_native.lib().scouter_sa_apply_relu_bwd_f32(dd.data_ptr(), ad.data_ptr(), gd.data_ptr(), xd.data_ptr(),
                                                              dx.data_ptr(), B, HW, Cp, None), "sa_apply_relu_bwd")
    torch.cuda.synchronize()
    assert bool((tail == SENTINEL).all())
    got = dx.cpu()
    err, bound = (got.double() - ref).abs(), 3 * EPS * mag
    print("sa_apply_relu_bwd Cp %d HW %d B %d: max err %.3e, max err / bound %.3f"
          % (Cp, HW, B, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    masked = got[~keep]
    assert bool((masked == 0).all()) and not bool(torch.signbit(masked).any())          # an exact +0 wherever x0 <= 0
    assert bool(keep.any()) and bool((~keep).any())
    # the wrapper on NHWC tensors gives the same bits; against the two passes it replaces: the same masks, the sum to rounding
    w = K.sa_apply_relu_bwd(dd.view(B, 1, HW, Cp), ad, gd, xd.view(B, 1, HW, 2 * Cp))
    assert torch.equal(w.view(B, HW, 2 * Cp), dx)
    two = K.relu_bwd(K.sa_apply_bwd(dd.view(B, 1, HW, Cp), ad, gd), xd.view(B, 1, HW, 2 * Cp)).view(B, HW, 2 * Cp)
    assert bool(((two.cpu().double() - got.double()).abs() <= 2 * bound).all())         # (each within `bound` of float64)


def test_sa_apply_relu_bwd_refusals():
    from scouter_amd import _native
    K, lib = KK(), _native.lib()
    B, HW, Cp = 2, 5, 8
    ts = [torch.ones((B, HW, Cp), device="cuda"), torch.ones((B, 2 * Cp), device="cuda"), torch.ones((B, Cp), device="cuda"),
          torch.ones((B, HW, 2 * Cp), device="cuda"), torch.full((B, HW, 2 * Cp), SENTINEL, device="cuda")]
    for i in range(5):
        args = [None if j == i else t.data_ptr() for j, t in enumerate(ts)]
        assert lib.scouter_sa_apply_relu_bwd_f32(*args, B, HW, Cp, None) == SC_ERR_ARG, i
    for shape in ((B, HW, 6), (B, HW, 2), (0, HW, Cp), (B, 0, Cp), (B, HW, 0)):       # Cp % 4, empty shapes
        assert lib.scouter_sa_apply_relu_bwd_f32(*[t.data_ptr() for t in ts], *shape, None) == SC_ERR_ARG, shape
    assert b"sa_apply_relu_bwd" in lib.scouter_last_error()
    torch.cuda.synchronize()
    assert bool((ts[4] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="x0"):
        K.sa_apply_relu_bwd(ts[0].view(B, 1, HW, Cp), ts[1], ts[2], ts[3].view(B, 1, HW, 2 * Cp).cpu())


# ------------------------------------------------------------------------------------------------ 3: maxpool_relu_bwd
@pytest.mark.parametrize("shape", [(1, 7, 9, 4), (2, 33, 30, 64), (1, 2, 2, 4), (1, 65537, 3, 4)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_maxpool_relu_bwd_equals_the_two_kernels(shape):
    """the issue's three shapes, and one past B * H = 65535, where maxpool_bwd leaves its rows kernel for the grid-stride one
    (which adds a pixel's windows in the opposite order) and this kernel follows it"""
    K = KK()
    B, H, W, C = shape
    h = rand(shape, 7).clamp_min(0.0)                                       # a ReLU's output: windows with several exact zeros
    h.view(-1)[0] = -0.0
    hd, _ = dev(h)
    p, arg = K.maxpool_fwd(hd, 3, 2, 1, want_argmax=True)
    dy, _ = dev(rand(tuple(p.shape), 8))
    want = K.relu_bwd(K.maxpool_bwd(dy, arg, shape, 3, 2, 1), hd)
    dx, tail = dev(torch.full(shape, 5.0), 0, 8)
    from scouter_amd import _native
    _native.check(_native.lib().scouter_maxpool_relu_bwd_f32(dy.data_ptr(), arg.data_ptr(), hd.data_ptr(), dx.data_ptr(), B, H, W, C,
                                                             3, 2, 1, None), "maxpool_relu_bwd")
    torch.cuda.synchronize()
    assert bool((tail == SENTINEL).all())
    assert torch.equal(dx, want) and torch.equal(dx.view(torch.int32), want.view(torch.int32))          # bit for bit, signs of zero too
    assert torch.equal(K.maxpool_relu_bwd(dy, arg, hd, 3, 2, 1), want)
    assert bool((dx[hd <= 0] == 0).all()) and float(dx.abs().max()) > 0
    # every pooled gradient whose window chose a positive element arrives exactly once: the sums agree in float64
    chosen = p > 0
    assert abs(float(dx.double().sum()) - float(dy.double()[chosen].sum())) <= 4 * EPS * float(dy.double().abs().sum())


def test_maxpool_relu_bwd_refusals():
    from scouter_amd import _native
    K, lib = KK(), _native.lib()
    B, H, W, C = 1, 6, 6, 4
    h = torch.ones((B, H, W, C), device="cuda")
    p, arg = K.maxpool_fwd(h, 3, 2, 1, want_argmax=True)
    dx = torch.full((B, H, W, C), SENTINEL, device="cuda")
    ts = [torch.ones_like(p), arg, h, dx]
    for i in range(4):
        args = [None if j == i else t.data_ptr() for j, t in enumerate(ts)]
        assert lib.scouter_maxpool_relu_bwd_f32(*args, B, H, W, C, 3, 2, 1, None) == SC_ERR_ARG, i
    for geom in ((B, H, W, 6, 3, 2, 1), (B, H, W, C, 16, 2, 1), (B, H, W, C, 3, 0, 1), (0, H, W, C, 3, 2, 1), (B, H, W, C, 3, 2, 3)):
        assert lib.scouter_maxpool_relu_bwd_f32(*[t.data_ptr() for t in ts], *geom, None) == SC_ERR_ARG, geom
    assert b"maxpool_relu_bwd" in lib.scouter_last_error()
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4: whole models
MODELS = ["resnet18_mnist_64", "resnest26d_96", "fc_resnet18_mnist_64"]


def moved_state(P, seed):
    """every BatchNorm of the state off its initial values: running means and biases moved, variances in [0.5, 1.5] (well above
    0), gammas in [0.5, 1.5] with either sign -- the zero-initialised last gammas of the blocks too, without which the fold is
    trivial and only the shortcuts carry gradient"""
    g = torch.Generator().manual_seed(seed)
    Q = {k: v.clone() for k, v in P.items()}
    for k in [k for k in Q if k.endswith("running_var")]:
        stem = k[:-len("running_var")]
        n = Q[k].shape
        Q[k] = 0.5 + torch.rand(n, generator=g)
        Q[stem + "running_mean"] = Q[stem + "running_mean"] + 0.1 * torch.randn(n, generator=g)
        sign = torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0)
        Q[stem + "weight"] = sign * (0.5 + torch.rand(n, generator=g))
        Q[stem + "bias"] = Q[stem + "bias"] + 0.1 * torch.randn(n, generator=g)
    return Q


def scalar_of(cfg, arch, cls):
    if cfg is not None:
        return class_scalar(cfg, cls)

    def f(P, x):
        out = O.fc_model_forward(P, x, None, arch, training=False)
        return out[torch.arange(out.shape[0]), cls].sum()
    return f


def pass_pattern(ip):
    """(ReLU masks {name: bool NCHW}, pool window indices [B, C, Ho, Wo]) on the CPU from ImagePass.relu_outputs"""
    outs = dict(ip.relu_outputs())
    pool_arg = outs.pop("maxpool").permute(0, 3, 1, 2).cpu()
    return {k: (v > 0).permute(0, 3, 1, 2).cpu() for k, v in outs.items()}, pool_arg


def autograd_gradient(m, x, seed):
    xx = x.clone().requires_grad_(True)
    out = m(xx)
    return torch.autograd.grad(out, xx, seed)[0]


@pytest.mark.parametrize("case", MODELS)
def test_image_pass_on_whole_models(case):
    from scouter_amd.nn_hip import BatchNorm2d
    m, P0, images, cfg, arch = build(case)
    P = moved_state(P0, 900)
    m.load_state_dict(P)
    m.eval()
    x = images.cuda()
    B = x.shape[0]
    n = 10
    cls = (torch.arange(B) * 3 + 1) % n
    seed = torch.zeros((B, n), device="cuda")
    seed[torch.arange(B), cls.cuda()] = 1.0
    auto_before = autograd_gradient(m, x, seed)                             # (also leaves a .grad on every parameter)
    backbone_grads = {k: p.grad.clone() for k, p in m.named_parameters()
                      if k.startswith("backbone.") and not k.startswith("backbone.fc.") and p.grad is not None}
    assert backbone_grads
    before = bn_buffers(m)
    # ---- one pass, against the oracle under the pass's own pattern
    ip = m.image_pass(x)
    g = ip.grad(seed)
    torch.cuda.synchronize()
    assert tuple(g.shape) == tuple(x.shape) and g.dtype == torch.float32 and g.is_contiguous()
    assert tuple(ip.log_probs.shape) == (B, n) and ip.features.dim() == 4
    masks, pool_arg = pass_pattern(ip)
    bn_relus = [k for k, mod in m.named_modules() if isinstance(mod, BatchNorm2d) and "downsample" not in k]
    assert set(masks) == set(bn_relus) | ({"conv1x1"} if m.use_slot else set())        # the keys of capture_relu_signs
    g64, g32 = oracle_input_grad((case, "foldgrad"), P, images, scalar_of(cfg, arch, cls), masks, pool_arg)
    check_input_grad(case + " image_pass", g, g64, g32)
    # ---- several seeds from ONE pass equal fresh passes, bit for bit
    seeds = [one_hot((B, n), 0), one_hot((B, n), 7), seed, torch.randn((B, n), generator=torch.Generator().manual_seed(3)).cuda()]
    many = [ip.grad(s) for s in seeds]
    assert torch.equal(many[2], g)
    for s, got in zip(seeds, many):
        assert torch.equal(m.image_pass(x).grad(s), got)
    assert not torch.equal(many[0], many[1])
    # ---- the refusals of FeaturePass.grad
    for bad in (seed[:, :n - 1], seed.double(), seed.cpu(), None):
        with pytest.raises(ValueError, match="seed"):
            ip.grad(bad)
    # ---- a batch row equals that image alone, bit for bit
    for b in (0, B - 1):
        alone = m.image_pass(x[b:b + 1].contiguous())
        assert torch.equal(alone.log_probs[0], ip.log_probs[b])
        assert torch.equal(alone.grad(seed[b:b + 1].contiguous())[0], g[b]), b
    # ---- the switch changes nothing, nothing of the model moved, the autograd route is what it was
    for fold in (True, False):
        m.set_inference_fold(fold)
        ipf = m.image_pass(x)
        assert torch.equal(ipf.log_probs, ip.log_probs) and torch.equal(ipf.grad(seed), g), fold
        if fold:                                                            # the pass's forward IS the folded eval forward
            with torch.no_grad():
                assert torch.equal(m(x), ipf.log_probs)
    assert not m.training
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    named = dict(m.named_parameters())
    assert all(torch.equal(named[k].grad, v) for k, v in backbone_grads.items())       # no backbone .grad was touched
    assert torch.equal(autograd_gradient(m, x, seed), auto_before)
    m.train()                                                               # a caller in training mode gets its mode back
    gt = m.image_pass(x).grad(seed)
    assert m.training and torch.equal(gt, g)
    assert all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    m.eval()
    # ---- a reload of the state dict between passes refolds: the gradient follows the new weights
    P2 = moved_state(P0, 901)
    m.load_state_dict(P2)
    g2 = m.image_pass(x).grad(seed)
    fresh = build(case)[0]
    fresh.load_state_dict(P2)
    fresh.eval()
    assert torch.equal(fresh.image_pass(x).grad(seed), g2) and not torch.equal(g2, g)
    with pytest.raises(RuntimeError, match="image_pass"):
        ip.grad(seed)                                                       # (the old pass's folded weights are gone)


def test_image_pass_refuses_bf16_and_host_tensors():
    m, P, images, cfg, arch = build("resnet18_mnist_64")
    with pytest.raises(RuntimeError, match="HIP device"):
        m.image_pass(images)
    with pytest.raises(ValueError, match="images"):
        m.image_pass(images.cuda()[0])
    m.set_precision("bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        m.image_pass(images.cuda())
    m.set_precision("fp32")
    assert bool(torch.isfinite(m.image_pass(images.cuda()).grad(one_hot((images.shape[0], 10), 1))).all())


# ------------------------------------------------------------------------------------------------ 5: the library
def lib_model(case="resnet18_mnist_64"):
    m, P0, images, cfg, arch = build(case)
    P = moved_state(P0, 902)
    m.load_state_dict(P)
    return m, P, images[:2].contiguous(), cfg, arch


def report(what, err, bound):
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), what


def test_input_gradients_folded_equals_the_pass():
    from scouter_amd.tools.attribution import input_gradients
    m, P, images, cfg, arch = lib_model()
    m.train()
    x = images.cuda()
    before = bn_buffers(m)
    got = input_gradients(m, x, classes=[0, 3], route="folded")
    assert m.training and tuple(got.shape) == (2, 2, 1, 64, 64) and got.dtype == torch.float32
    m.eval()
    ip = m.image_pass(x)
    for j, c in enumerate([0, 3]):
        assert torch.equal(got[:, j], ip.grad(one_hot((2, 10), c))), c
    every = input_gradients(m, x, route="folded")
    assert tuple(every.shape) == (2, 10, 1, 64, 64) and torch.equal(every[:, 3], got[:, 1])
    cls = torch.tensor([7, 2])
    own = input_gradients(m, x, classes=cls, route="folded")
    seed = torch.zeros((2, 10), device="cuda")
    seed[torch.arange(2), cls.cuda()] = 1.0
    assert tuple(own.shape) == (2, 1, 1, 64, 64) and torch.equal(own[:, 0], ip.grad(seed))
    assert torch.equal(own[0, 0], every[0, 7]) and torch.equal(own[1, 0], every[1, 2])
    assert input_gradients(m, x, classes=[], route="folded").shape[:2] == (2, 0)
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            input_gradients(m, x, classes=bad, route="folded")
    assert all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    # the default route, named or not: the same bits (the two routes are two roundings of one gradient: the figure is printed)
    auto = input_gradients(m, x, classes=[0, 3])
    print("input_gradients: max |folded - autograd| = %.3e, max |autograd| = %.3e" % (float((auto - got).abs().max()),
                                                                                  float(auto.abs().max())))
    assert torch.equal(input_gradients(m, x, classes=[0, 3], route="autograd"), auto)


def pass_gradients(m, images, classes, fill, N):
    """float64 [B, K, N, C, H, W] on the CPU: the folded pass's own gradients on the rows fill(b, buf, first) writes (one pass of
    all N rows: a row's gradient does not depend on the rows next to it)"""
    rows = []
    for b in range(images.shape[0]):
        chunk = fill(b, torch.empty((N,) + tuple(images.shape[1:]), device="cuda"), 0)
        ip = m.image_pass(chunk)
        rows.append(torch.stack([ip.grad(one_hot((N, 10), c)).cpu().double() for c in classes]))
    return torch.stack(rows)


_IG_ORACLE = {}


def oracle_ig_gap(P, cfg, x, base, alphas, weights, cols):
    """the fp64 oracle's own completeness gap of the same quadrature for image 0: [K] gaps and out(x) - out(x')"""
    if "gap" not in _IG_ORACLE:
        Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        x, base = x.double(), base.double()
        rows = (base[None] + alphas.double().view(-1, 1, 1, 1) * (x - base)[None]).requires_grad_(True)
        out = O.slot_model_forward(Pd, rows, None, cfg, training=False)
        gaps = []
        with torch.no_grad():
            ends = O.slot_model_forward(Pd, torch.stack([base, x]), None, cfg, training=False)
        for c in cols:
            g, = torch.autograd.grad(out[:, c].sum(), rows, retain_graph=True)
            attr = (x - base) * (weights.double().view(-1, 1, 1, 1) * g).sum(dim=0)
            gaps.append(attr.sum() - (ends[1, c] - ends[0, c]))
        _IG_ORACLE["gap"] = (torch.stack(gaps), torch.stack([ends[1, c] - ends[0, c] for c in cols]))
    return _IG_ORACLE["gap"]


def test_path_methods_folded_on_a_whole_model():
    """resnet18 / MNIST stem / 64^2, two images, 7 steps or samples, classes [0, 3]"""
    K = KK()
    from scouter_amd.tools import attribution as AT
    from test_gradshap_gpu import restated_rows
    m, P, images, cfg, arch = lib_model()
    m.eval()
    x = images.cuda()
    N, classes = 7, [0, 3]
    before = bn_buffers(m)
    # ---- integrated gradients
    baseline = torch.randn((1, 64, 64), generator=torch.Generator().manual_seed(21)).cuda()
    alphas, weights = AT.ig_quadrature(N)
    ad = alphas.cuda()
    g = pass_gradients(m, x, classes, lambda b, buf, first: K.path_images(x[b], baseline, ad, buf, first), N)
    w64 = weights.double().view(1, 1, -1, 1, 1, 1)
    d = (x - baseline[None]).cpu().double()[:, None]
    ref, mag = d * (w64 * g).sum(dim=2), d.abs() * (w64 * g).abs().sum(dim=2)
    kw = dict(classes=classes, baseline=baseline, n_steps=N, route="folded")
    attr, delta = AT.integrated_gradients_by_route(m, x, batch=3, return_delta=True, **kw)
    assert tuple(attr.shape) == (2, 2, 1, 64, 64) and tuple(delta.shape) == (2, 2)
    report("integrated_gradients folded", (attr.cpu().double() - ref).abs(), 4 * EPS * mag)
    for batch in (1, 3, 7):                                                 # the chunking changes no bit
        a2, d2 = AT.integrated_gradients_by_route(m, x, batch=batch, return_delta=True, **kw)
        assert torch.equal(a2, attr) and torch.equal(d2, delta), batch
    gap64, ends64 = oracle_ig_gap(P, cfg, images[0], baseline.cpu(), alphas, weights, classes)
    allowed = 2.0 * gap64.abs() + 1e-3 * ends64.abs()
    print("integrated_gradients folded completeness: gap HIP %s, fp64 oracle %s, out(x) - out(x') %s"
          % (delta[0].cpu().tolist(), gap64.tolist(), ends64.tolist()))
    assert bool((delta[0].cpu().double().abs() <= allowed).all())
    own = AT.integrated_gradients_by_route(m, x, classes=torch.tensor([3, 0]), baseline=baseline, n_steps=N, batch=3, route="folded")
    assert torch.equal(own[0, 0], attr[0, 1]) and torch.equal(own[1, 0], attr[1, 0])
    # ---- SmoothGrad, the three kinds
    sigma, seed = 0.5, 5
    g = pass_gradients(m, x, classes, lambda b, buf, first: K.noise_images(x[b], buf, sigma, seed, first), N)
    mean, mean_abs, mean_sq = g.mean(dim=2), g.abs().mean(dim=2), (g * g).mean(dim=2)
    skw = dict(classes=classes, n_samples=N, sigma=sigma, seed=seed, route="folded")
    got = {kind: AT.smoothgrad_by_route(m, x, kind=kind, batch=3, **skw) for kind in ("smoothgrad", "smoothgrad_sq", "vargrad")}
    report("smoothgrad folded", (got["smoothgrad"].cpu().double() - mean).abs(), 4 * EPS * mean_abs)
    report("smoothgrad_sq folded", (got["smoothgrad_sq"].cpu().double() - mean_sq).abs(), 4 * EPS * mean_sq)
    report("vargrad folded", (got["vargrad"].cpu().double() - (mean_sq - mean * mean)).abs(), 4 * EPS * mean_sq)
    for batch in (1, 3, 7):
        for kind, want in got.items():
            assert torch.equal(AT.smoothgrad_by_route(m, x, kind=kind, batch=batch, **skw), want), (kind, batch)
    # ---- GradientSHAP
    bank = torch.randn((3, 1, 64, 64), generator=torch.Generator().manual_seed(31)).cuda()
    gsigma, gseed = 0.1, 2
    g = pass_gradients(m, x, classes, lambda b, buf, first: K.gradshap_images(x[b], bank, buf, gsigma, gseed, first), N)
    diffs = torch.stack([restated_rows(x[b], bank, gsigma, gseed, 0, N)[1].cpu().double() for b in range(2)])          # [B, N, C, H, W]
    t = g * diffs[:, None] / N
    ref, mag = t.sum(dim=2), t.abs().sum(dim=2)
    gkw = dict(classes=classes, baselines=bank, n_samples=N, sigma=gsigma, seed=gseed, route="folded")
    gs, gs_delta = AT.gradient_shap(m, x, batch=3, return_delta=True, **gkw)
    report("gradient_shap folded", (gs.cpu().double() - ref).abs(), EPS * ref.abs() + (N + 4) * U * mag)
    for batch in (1, 3, 7):
        a2, d2 = AT.gradient_shap(m, x, batch=batch, return_delta=True, **gkw)
        assert torch.equal(a2, gs) and torch.equal(d2, gs_delta), batch
    assert not m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    # ---- the default route is the code it was: route="autograd" named or not, the same bits
    auto = AT.integrated_gradients(m, x, classes=classes, baseline=baseline, n_steps=N, batch=3)
    assert torch.equal(AT.integrated_gradients_by_route(m, x, classes=classes, baseline=baseline, n_steps=N, batch=3, route="autograd"), auto)
    print("integrated_gradients: max |folded - autograd| = %.3e, max |autograd| = %.3e" % (float((auto - attr).abs().max()),
                                                                                       float(auto.abs().max())))


# ------------------------------------------------------------------------------------------------ 6: the tool
TOOL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--ig", "true", "--ig_route", "folded",
        "--ig_steps", "6", "--ig_batch", "4", "--grad_min_level", "0.2", "--use_slot", "true"]


def test_the_tool_on_one_image(tmp_path, monkeypatch, capsys):
    """--table_images 0 writes ig_{c}.png of every class, the bytes of the library's maps under route="folded", and one infidelity
    line per family drawn"""
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.tools import attribution as AT
    from scouter_amd.tools import foldgrad as FG
    vis_dir = str(tmp_path / "vis")
    argv = ["foldgrad.py"] + TOOL + ["--infidelity", "true", "--infidelity_samples", "4", "--infidelity_batch", "5", "--vis_dir", vis_dir,
                                     "--output_dir", str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    FG.main()
    out = capsys.readouterr().out
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("infidelity ")]
    assert [ln[1] for ln in lines] == ["slot", "ig"], lines
    assert all(math.isfinite(float(v)) for ln in lines for v in ln[4:] if v[0].isdigit() or v[0] == "-")
    assert sorted(os.listdir(vis_dir)) == sorted("%s_%d.png" % (nm, c) for nm in ("slot", "ig") for c in range(10))
    args = FG.get_foldgrad_parser().parse_args(argv[1:])
    kw = FG.option_kwargs(args, "ig")
    assert kw == dict(n_steps=6, batch=4, route="folded")
    torch.manual_seed(11)
    model, _ = T.build_model(args)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))[None].cuda()
    maps = AT.gradient_maps(AT.integrated_gradients_by_route(model, x, **kw), min_level=0.2)[0].cpu().numpy()
    assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and any(mp.any() for mp in maps)
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(vis_dir, "ig_%d.png" % c)))
        assert np.array_equal(png, maps[c]), c


def test_the_tool_on_a_table(tmp_path, monkeypatch, capsys):
    """--table_images 2 on synthetic data: one `table ig:` line after the table's own"""
    from scouter_amd.tools import foldgrad as FG
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["foldgrad.py"] + TOOL + ["--synthetic_data", "true", "--num_workers", "0", "--table_images", "2",
                                                              "--batch_size", "2", "--localization", "true", "--output_dir", str(tmp_path / "none")])
    result = FG.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == ["slot:", "ig:", "accuracy"]
    cols = result.rows["ig"]
    assert all(v.dtype == np.float64 and v.shape == (2,) for v in cols.values())
    assert ((cols["area"] >= 0) & (cols["area"] <= 1)).all()
