"""Grad-CAM++ and Smooth Grad-CAM++ (-m gpu): the three kernels of csrc/gradcampp.hip against fp64, their zero-denominator rule
and refusals, tools/attribution.py gradcampp / smooth_gradcampp on whole models, the heat maps and test.py --campp / --smoothcampp.

Operands.  Unlike Grad-CAM the method is ill-conditioned on arbitrary operands (2 g^2 + S can cancel), so they are fixed:
feat = 0.5 |randn| (the layer's output is post-ReLU), dfeat = s[b][c] + 0.5 randn with s = +1 with probability 0.75 and -1
otherwise, drawn per (image, channel).

Bound, per output element, in fp64 from the same operands by first-order propagation, eps = 2^-24, T[c] = sum_p |g3 A|:
    rel_alpha[p][c] = eps (5 + (6 g2 + (N + 5) T[c]) / |den|)
    dw[c]           = sum_p |alpha relu(g)| (rel_alpha + N eps)
    bound[p]        = 2 sum_c (dw[c] + (C + 2) eps |w[c]|) |A[p][c]|
and the condition max_p bound <= 1e-3 max_p |map| per image, so that the bound cannot hide a failure.  On the CPU (PyTorch fp32
restating the kernel's passes, seeds 0 .. 2, both relu settings, all seven shapes) these operands gave max_p bound / max_p |map|
<= 2.7e-4 for Grad-CAM++ and for the smooth kernel's operands (n = 3), and |fp32 - fp64| <= 0.05 bound.  The ratio grows with C
through the (C + 2) eps term: the three further shapes of MORE_SHAPES, chosen for the kernel routes the list leaves out, gave
5.0e-4 (C = 4100), 1.4e-4 (C = 1030) and 9.9e-4 (C = 8192, the largest supported)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gradcam_gpu import bn_buffers, build, model_args                 # noqa: E402

SHAPES = [(1, 1, 1, 1), (2, 1, 1, 70), (3, 2, 3, 65), (2, 7, 7, 512), (2, 7, 7, 2048), (1, 9, 9, 2048), (2, 3, 3, 130)]
# the routes the list above leaves out: float4 columns and single channels with more columns than threads, and the largest C
MORE_SHAPES = [(1, 4, 4, 4100), (1, 5, 5, 1030), (1, 5, 5, 8192)]
SENTINEL = -777.25
EPS = 2.0 ** -24


def shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------------ operands and fp64
def operands(shape, seed=0, n=1):
    """feat [B, h, w, C] and n gradients [n, B, h, w, C] that share the signs s.  For C = N = B = 1 the seed moves on until
    s = +1 and the gradient is positive (a map that is not identically zero)."""
    B, h, w, C = shape
    while True:
        gen = torch.Generator().manual_seed(5000 + seed)
        feat = 0.5 * torch.randn(shape, generator=gen).abs()
        s = (torch.rand((B, 1, 1, C), generator=gen) < 0.75).float() * 2.0 - 1.0
        grads = s + 0.5 * torch.randn((n,) + tuple(shape), generator=gen)
        if B * h * w * C > 1 or (float(s.min()) > 0 and float(grads.min()) > 0):
            return feat, grads
        seed += 1000


def campp_fp64(feat, g2, g3, gr, relu):
    """(map [B, N], bound [B, N]) in fp64 from A = feat, g2, g3 (the second and third powers, or their means) and gr"""
    B, h, w, C = feat.shape
    N = h * w
    A, g2, g3, gr = (t.double().reshape(B, N, C) for t in (feat, g2, g3, gr))
    S = (g3 * A).sum(dim=1, keepdim=True)
    T = (g3 * A).abs().sum(dim=1, keepdim=True)
    den = 2.0 * g2 + S
    live = den != 0
    safe = torch.where(live, den, torch.ones_like(den))
    alpha = torch.where(live, g2 / safe, torch.zeros_like(den))
    term = alpha * gr.clamp_min(0.0)
    wgt = term.sum(dim=1)
    ref = torch.einsum("bc,bpc->bp", wgt, A)
    if relu:
        ref = ref.clamp_min(0.0)
    rel_alpha = torch.where(live, EPS * (5.0 + (6.0 * g2 + (N + 5) * T) / safe.abs()), torch.zeros_like(den))
    dw = (term.abs() * (rel_alpha + N * EPS)).sum(dim=1)
    bound = 2.0 * torch.einsum("bc,bpc->bp", dw + (C + 2) * EPS * wgt.abs(), A.abs())
    return ref, bound


def check_condition(what, ref, bound):
    """max_p bound <= 1e-3 max_p |map| for every image; returns the largest ratio"""
    top, scale = bound.max(dim=1).values, ref.abs().max(dim=1).values
    ratio = float((top / scale.clamp_min(1e-300)).max()) if float(top.max()) > 0 else 0.0
    print("%s: max_p bound / max_p |map| = %.3e" % (what, ratio))
    assert bool((top <= 1e-3 * scale).all()), (what, top.tolist(), scale.tolist())
    return ratio


def check_error(what, got, ref, bound):
    assert bool(torch.isfinite(got).all())
    err = (got.cpu().double() - ref).abs()
    print("%s: max err %.3e, max err / bound %.3e" % (what, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.min()))


def run_strided(fill, B, h, w):
    """fill(out) through two output strides: the same bits, the sentinel columns untouched, finite -> [B, h * w]"""
    full = torch.full((B, 3, h, w), SENTINEL, device="cuda")
    fill(full[:, 1])
    again = torch.full((B, h * w), SENTINEL, device="cuda")
    fill(again)
    torch.cuda.synchronize()
    got = full[:, 1].reshape(B, h * w)
    assert torch.equal(got, again)
    assert bool((full[:, 0] == SENTINEL).all()) and bool((full[:, 2] == SENTINEL).all())
    assert bool(torch.isfinite(got).all())
    return got


def check_gradcampp(shape, relu, seed=0):
    from scouter_amd import kernels as K
    B, h, w, C = shape
    feat, grads = operands(shape, seed)
    g = grads[0]
    ref, bound = campp_fp64(feat, g.double() ** 2, g.double() ** 3, g, relu)
    what = "gradcampp %s relu %s" % (shape, relu)
    check_condition(what, ref, bound)
    fd, gd = feat.cuda(), g.cuda()
    got = run_strided(lambda out: K.gradcampp(fd, gd, out, relu=relu), B, h, w)
    check_error(what, got, ref, bound)


# ------------------------------------------------------------------------------------------------------ 1: K.gradcampp
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=shape_id)
def test_gradcampp_kernel_against_fp64(shape, relu):
    check_gradcampp(shape, relu)


def test_gradcampp_default_is_rectified():
    from scouter_amd import kernels as K
    feat, grads = operands((2, 3, 3, 130), 3)
    fd, gd = feat.cuda(), (-grads[0]).cuda()                            # mostly negative gradients: negative weights appear
    a, b, c = (torch.empty((2, 9), device="cuda") for _ in range(3))
    K.gradcampp(fd, gd, a)
    K.gradcampp(fd, gd, b, relu=True)
    K.gradcampp(fd, gd, c, relu=False)
    assert torch.equal(a, b) and torch.equal(a, c.clamp_min(0.0))


# ------------------------------------------------------------------------------------------------------ 2: zero denominators
@pytest.mark.parametrize("shape", [(2, 3, 3, 130), (2, 7, 7, 512), (1, 4, 4, 4100)], ids=shape_id)
def test_zero_denominators(shape):
    """a channel whose gradient is all zero contributes nothing: the bits of the same call with that channel's features also
    zeroed; an all-zero gradient gives an all-zero map; no NaN or infinity.  For both kernels."""
    from scouter_amd import kernels as K
    B, h, w, C = shape
    feat, grads = operands(shape, 7, n=2)
    dead = [0, C // 2, C - 1]
    grads[:, :, :, :, dead] = 0.0
    cut = feat.clone()
    cut[..., dead] = 0.0
    g = grads[0].cuda()
    acc2 = (grads.double() ** 2).sum(0).cuda()
    acc3 = (grads.double() ** 3).sum(0).cuda()
    last = grads[1].cuda()
    zero32, zero64 = torch.zeros_like(g), torch.zeros_like(acc2)
    for relu in (False, True):
        outs = []
        for f in (feat.cuda(), cut.cuda()):
            a, b, za, zb = (torch.full((B, h * w), SENTINEL, device="cuda") for _ in range(4))
            K.gradcampp(f, g, a, relu=relu)
            K.gradcampp_smooth(f, acc2, acc3, last, b, 2, relu=relu)
            K.gradcampp(f, zero32, za, relu=relu)
            K.gradcampp_smooth(f, zero64, zero64.clone(), last, zb, 2, relu=relu)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
            assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0
            assert not bool(za.any()) and not bool(zb.any())
            outs.append((a, b))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------------ 3: refusals
def _call(kernel, feat, other, out, lib_args=None):
    """one of the two class-map entry points on (feat, a gradient-shaped tensor); lib_args: straight through the C ABI"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    if lib_args is not None:
        fn = getattr(_native.lib(), "scouter_gradcampp_f32" if kernel == "gradcampp" else "scouter_gradcampp_smooth_f32")
        return _native.check(fn(*lib_args), kernel)
    if kernel == "gradcampp":
        return K.gradcampp(feat, other, out)
    acc = torch.ones(feat.shape, dtype=torch.float64, device="cuda")
    return K.gradcampp_smooth(feat, acc, acc.clone(), other, out, 1)


@pytest.mark.parametrize("bad", ["c0", "null", "misaligned", "c_too_large"])
@pytest.mark.parametrize("kernel", ["gradcampp", "gradcampp_smooth"])
def test_class_map_kernels_refuse_bad_arguments(kernel, bad):
    """C = 0, a null pointer, a pointer off its alignment, more channels than the LDS plan holds: the library's error naming the
    kernel, nothing launched, and a valid call afterwards is right"""
    out = torch.full((2, 9), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match=kernel):
        if bad == "c0":
            e = torch.empty((2, 3, 3, 0), device="cuda")
            _call(kernel, e, e.clone(), out)
        elif bad == "null":
            f = torch.ones((2, 3, 3, 8), device="cuda")
            d = torch.ones((2, 3, 3, 8), dtype=torch.float64, device="cuda")
            if kernel == "gradcampp":
                _call(kernel, None, None, None, (f.data_ptr(), None, out.data_ptr(), 2, 9, 8, 9, 0, None))
            else:
                _call(kernel, None, None, None, (f.data_ptr(), d.data_ptr(), None, f.data_ptr(), out.data_ptr(), 1, 2, 9, 8, 9, 0,
                                                 None))
        elif bad == "misaligned":
            big = torch.ones(2 * 9 * 8 + 4, device="cuda")
            _call(kernel, big[1:1 + 144].view(2, 3, 3, 8), torch.ones((2, 3, 3, 8), device="cuda"), out)
        else:
            f = torch.ones((2, 3, 3, 8196), device="cuda")
            _call(kernel, f, f.clone(), out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    if kernel == "gradcampp":
        check_gradcampp((3, 2, 3, 65), True, seed=1)
    else:
        check_smooth((3, 2, 3, 65), True, seed=1)


@pytest.mark.parametrize("bad", ["e0", "null", "misaligned", "same"])
def test_grad_powers_accumulate_refuses_bad_arguments(bad):
    from scouter_amd import _native
    from scouter_amd import kernels as K
    acc2 = torch.full((9,), float(SENTINEL), dtype=torch.float64, device="cuda")
    acc3 = acc2.clone()
    g = torch.ones((2, 9), device="cuda")
    with pytest.raises(RuntimeError, match="grad_powers_accumulate"):
        if bad == "e0":
            K.grad_powers_accumulate(torch.empty((2, 0), device="cuda"), acc2[:0], acc3[:0])
        elif bad == "null":
            _native.check(_native.lib().scouter_grad_powers_accumulate(g.data_ptr(), acc2.data_ptr(), None, 2, 9, None),
                          "grad_powers_accumulate")
        elif bad == "misaligned":
            _native.check(_native.lib().scouter_grad_powers_accumulate(g.data_ptr(), acc2.data_ptr() + 4, acc3.data_ptr(), 2, 8,
                                                                       None), "grad_powers_accumulate")
        else:
            K.grad_powers_accumulate(g, acc2, acc2)
    torch.cuda.synchronize()
    assert bool((acc2 == SENTINEL).all()) and bool((acc3 == SENTINEL).all())
    check_grad_powers(130)


# ------------------------------------------------------------------------------------------------------ 4: grad_powers_accumulate
def check_grad_powers(E, n=5):
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(6000 + E)
    grads = torch.randn((n, E), generator=gen)
    gd = grads.cuda()
    g = grads.double()
    for start2, start3 in ((torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)),
                           (torch.randn(E, generator=gen).double(), torch.randn(E, generator=gen).double())):
        results = []
        for pieces in ([5], [2, 3], [1] * 5):
            a2, a3 = start2.cuda(), start3.cuda()
            j = 0
            for m in pieces:
                K.grad_powers_accumulate(gd[j:j + m], a2, a3)
                j += m
            results.append((a2, a3))
        torch.cuda.synchronize()
        for a2, a3 in results[1:]:
            assert torch.equal(a2, results[0][0]) and torch.equal(a3, results[0][1])
        assert bool(torch.isfinite(results[0][0]).all()) and bool(torch.isfinite(results[0][1]).all())
        if float(start2.abs().max()) > 0:
            continue                                                    # (the bound below is stated for sums that start at 0)
        for name, got, terms in (("acc2", results[0][0], g ** 2), ("acc3", results[0][1], g ** 3)):
            bound = (n + 1) * 2.0 ** -52 * terms.abs().sum(0)
            err = (got.cpu() - terms.sum(0)).abs()
            print("grad_powers_accumulate E %d %s: max err %.3e, max err / bound %.3f"
                  % (E, name, float(err.max()), float((err / bound).max())))
            assert bool((err <= bound).all())


@pytest.mark.parametrize("E", [1, 130, 49 * 512])
def test_grad_powers_accumulate(E):
    """n = 5: one call, a 2 + 3 split and five single calls give the same bits, from zero and from random starting sums;
    from zero against fp64 torch within (n + 1) 2^-52 sum_j |term_j|"""
    check_grad_powers(E)


# ------------------------------------------------------------------------------------------------------ 5: K.gradcampp_smooth
def check_smooth(shape, relu, seed=0, n=3):
    from scouter_amd import kernels as K
    B, h, w, C = shape
    feat, grads = operands(shape, seed, n=n)
    g = grads.double()
    acc2, acc3 = (g ** 2).sum(0), (g ** 3).sum(0)
    ref, bound = campp_fp64(feat, acc2 / n, acc3 / n, grads[n - 1], relu)
    what = "gradcampp_smooth %s relu %s" % (shape, relu)
    check_condition(what, ref, bound)
    fd, a2, a3, last = feat.cuda(), acc2.cuda(), acc3.cuda(), grads[n - 1].cuda()
    got = run_strided(lambda out: K.gradcampp_smooth(fd, a2, a3, last, out, n, relu=relu), B, h, w)
    check_error(what, got, ref, bound)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", SHAPES + MORE_SHAPES, ids=shape_id)
def test_smooth_kernel_against_fp64(shape, relu):
    check_smooth(shape, relu)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_smooth_kernel_with_one_sample_agrees_with_gradcampp(shape):
    """n = 1, acc2 = g^2, acc3 = g^3 (through K.grad_powers_accumulate), glast = g: K.gradcampp within the bound"""
    from scouter_amd import kernels as K
    B, h, w, C = shape
    feat, grads = operands(shape, 2)
    g = grads[0]
    _, bound = campp_fp64(feat, g.double() ** 2, g.double() ** 3, g, True)
    fd, gd = feat.cuda(), g.cuda()
    acc2 = torch.zeros(shape, dtype=torch.float64, device="cuda")
    acc3 = torch.zeros_like(acc2)
    K.grad_powers_accumulate(gd[None], acc2, acc3)
    one, two = torch.empty((B, h * w), device="cuda"), torch.empty((B, h * w), device="cuda")
    K.gradcampp(fd, gd, one)
    K.gradcampp_smooth(fd, acc2, acc3, gd, two, 1)
    torch.cuda.synchronize()
    assert torch.equal(acc2.cpu(), g.double() ** 2)                     # (exact in fp64)
    check_error("smooth n = 1 against gradcampp %s" % (shape,), two, one.cpu().double(), bound)


# ------------------------------------------------------------------------------------------------------ 6: whole models
def by_hand(m, images, seeds, relu=True):
    """K.gradcampp applied to feature_pass(images) and .grad(seed) for every seed -> [B, len(seeds), h, w]"""
    from scouter_amd import kernels as K
    fp = m.feature_pass(images)
    feat = fp.features
    B, h, w, _ = feat.shape
    out = torch.empty((B, len(seeds), h, w), device="cuda")
    for k, seed in enumerate(seeds):
        K.gradcampp(feat, fp.grad(seed), out[:, k], relu=relu)
    return out


def one_hot(B, n, cls):
    seed = torch.zeros((B, n), device="cuda")
    seed[torch.arange(B), torch.as_tensor(cls).expand(B)] = 1.0
    return seed


@pytest.mark.parametrize("case", ["resnet18_mnist_64", "fc_resnet18_mnist_64", "resnest26d_96"])
def test_gradcampp_on_models(case):
    from scouter_amd.tools.attribution import gradcam, gradcampp
    m, P, images, cfg, arch = build(case)
    images = images.cuda()
    m.train()
    before = bn_buffers(m)
    cam_before = gradcam(m, images, classes=[0, 3])
    B = images.shape[0]
    n = m.feature_pass(images).log_probs.shape[1]
    two = gradcampp(m, images, classes=[0, 3])
    assert m.training                                                    # the caller's mode is back
    feat_shape = m.feature_pass(images).features.shape
    assert tuple(two.shape) == (B, 2) + tuple(feat_shape[1:3]) and two.dtype == torch.float32 and two.is_cuda
    assert torch.equal(two, by_hand(m, images, [one_hot(B, n, 0), one_hot(B, n, 3)]))
    assert bool(torch.isfinite(two).all()) and float(two.abs().max()) > 0 and float(two.min()) >= 0
    plain = gradcampp(m, images, classes=[3], relu=False)
    assert torch.equal(plain, by_hand(m, images, [one_hot(B, n, 3)], relu=False))
    assert torch.equal(plain.clamp_min(0.0)[:, 0], two[:, 1])
    every = gradcampp(m, images)
    assert tuple(every.shape) == (B, n) + tuple(feat_shape[1:3])
    assert torch.equal(every, by_hand(m, images, [one_hot(B, n, c) for c in range(n)]))
    cls = (torch.arange(B) * 3 + 1) % n
    own = gradcampp(m, images, classes=cls)
    assert tuple(own.shape) == (B, 1) + tuple(feat_shape[1:3]) and torch.equal(own, by_hand(m, images, [one_hot(B, n, cls)]))
    for bad in ([n], [-1], torch.tensor([0] * (B - 1) + [n])):
        with pytest.raises(IndexError):
            gradcampp(m, images, classes=bad)
    with pytest.raises(ValueError):
        gradcampp(m, images, classes=torch.tensor([0] * (B + 1)))
    assert m.training
    m.eval()
    gradcampp(m, images, classes=[1])
    assert not m.training
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(gradcam(m, images, classes=[0, 3]), cam_before)   # gradcam itself: the bits it gave before


# ------------------------------------------------------------------------------------------------------ 7: smooth_gradcampp
SMOOTH_CASE = "resnet18_mnist_64"


def test_smooth_gradcampp_chunks_and_seeds():
    """n_samples = 4: batch 1, 3 and 4 give the same bits; the same seed repeats, another differs; per-image classes pick
    the matching columns; the caller's mode and the BatchNorm buffers stay"""
    from scouter_amd.tools.attribution import smooth_gradcampp
    m, P, images, cfg, arch = build(SMOOTH_CASE)
    images = images.cuda()[:2]
    m.train()
    before = bn_buffers(m)
    kw = dict(classes=[0, 3], n_samples=4, sigma=0.3, seed=5)
    ref = smooth_gradcampp(m, images, batch=4, **kw)
    assert m.training
    feat_shape = m.feature_pass(images).features.shape
    assert tuple(ref.shape) == (2, 2) + tuple(feat_shape[1:3]) and ref.dtype == torch.float32 and ref.is_cuda
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0 and float(ref.min()) >= 0
    for batch in (1, 3, 4):
        assert torch.equal(smooth_gradcampp(m, images, batch=batch, **kw), ref), batch
    assert not torch.equal(smooth_gradcampp(m, images, batch=4, **{**kw, "seed": 6}), ref)
    own = smooth_gradcampp(m, images, batch=3, **{**kw, "classes": torch.tensor([3, 0])})
    assert tuple(own.shape) == (2, 1) + tuple(ref.shape[2:])
    assert torch.equal(own[0, 0], ref[0, 1]) and torch.equal(own[1, 0], ref[1, 0])
    plain = smooth_gradcampp(m, images, batch=4, relu=False, **kw)
    assert torch.equal(plain.clamp_min(0.0), ref)
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            smooth_gradcampp(m, images, **{**kw, "classes": bad})
    after = bn_buffers(m)
    assert m.training and all(torch.equal(before[k], after[k]) for k in before)


def test_smooth_gradcampp_without_noise_agrees_with_gradcampp():
    """sigma = 0 on the first image of SMOOTH_CASE (resnet18, MNIST stem, 64 x 64, slot head): every sample is the image itself,
    so with chunks of one image the sums hold n g^2 and n g^3 of gradcampp's own gradient and the two differ by the kernels'
    rounding alone -- within the kernel bound at the model's own features and gradient.  The model case is chosen so that the
    1e-3 condition holds there; if it does not, the assertion is skipped with a printed reason."""
    from scouter_amd.tools.attribution import gradcampp, smooth_gradcampp
    m, P, images, cfg, arch = build(SMOOTH_CASE)
    image = images.cuda()[:1]
    classes = [0, 3]
    fp = m.feature_pass(image)
    want = gradcampp(m, image, classes=classes)
    for k, c in enumerate(classes):
        g = fp.grad(one_hot(1, fp.log_probs.shape[1], c)).cpu()
        ref, bound = campp_fp64(fp.features.cpu(), g.double() ** 2, g.double() ** 3, g, True)
        top, scale = float(bound.max()), float(ref.abs().max())
        print("%s class %d: max_p bound / max_p |map| = %.3e" % (SMOOTH_CASE, c, top / max(scale, 1e-300)))
        conditioned = top <= 1e-3 * scale
        for n_samples in (1, 4):
            got = smooth_gradcampp(m, image, classes=[c], n_samples=n_samples, sigma=0.0, batch=1)
            assert bool(torch.isfinite(got).all())
            if conditioned:
                check_error("%s class %d sigma 0, n %d" % (SMOOTH_CASE, c, n_samples), got.reshape(1, -1),
                            want[:, k].reshape(1, -1).cpu().double(), bound)
            else:
                print("NOT ASSERTED: the 1e-3 condition fails for %s class %d" % (SMOOTH_CASE, c))


# ------------------------------------------------------------------------------------------------------ 8: maps and the CLI
def test_maps_and_test_tool(tmp_path, monkeypatch, capsys):
    """gradcampp_maps / smooth_gradcampp_maps are K.cam_maps of the float results; scouter_amd.test --campp true --smoothcampp
    true --causal true writes campp_{c}.png and smoothcampp_{c}.png with those bytes and prints one causal line for each"""
    import re
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools.attribution import gradcampp, gradcampp_maps, smooth_gradcampp, smooth_gradcampp_maps
    cli_dir = str(tmp_path / "cli")
    argv = ["test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
            "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "true", "--pre_trained", "false", "--img_size", "64",
            "--campp", "true", "--smoothcampp", "true", "--smoothcampp_samples", "3", "--smoothcampp_batch", "2", "--causal",
            "true", "--causal_step", "512", "--grad_min_level", "0.2", "--eval_fold", "true", "--vis_dir", cli_dir, "--output_dir",
            str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    T.main()
    printed = capsys.readouterr().out
    # the same model (the same seed) and the same synthetic image, by hand
    args = T.get_test_parser().parse_args(argv[1:])
    for name, typ in (("num_classes", int), ("lambda_value", float), ("power", int), ("slots_per_class", int)):
        setattr(args, name, typ(getattr(args, name)))
    args.vis, args.vis_id, args.grad = False, 0, False
    torch.manual_seed(11)
    model = SlotModel(args).to(args.device)
    model.set_inference_fold(True)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))[None].cuda()
    kw = dict(n_samples=3, sigma=0.3, batch=2)
    wanted = {"campp": gradcampp_maps(model, x, min_level=0.2), "smoothcampp": smooth_gradcampp_maps(model, x, min_level=0.2, **kw)}
    assert torch.equal(wanted["campp"], K.cam_maps(gradcampp(model, x), 64, 64, 0.2))
    assert torch.equal(wanted["smoothcampp"], K.cam_maps(smooth_gradcampp(model, x, **kw), 64, 64, 0.2))
    small = gradcampp_maps(model, x, classes=[2, 5], size=(20, 30), relu=False)
    assert torch.equal(small, K.cam_maps(gradcampp(model, x, classes=[2, 5], relu=False), 20, 30, 0.0))
    small = smooth_gradcampp_maps(model, x, classes=[2], size=(20, 30), **kw)
    assert torch.equal(small, K.cam_maps(smooth_gradcampp(model, x, classes=[2], **kw), 20, 30, 0.0))
    for stem, want in wanted.items():
        assert want.dtype == torch.uint8 and want.is_cuda and tuple(want.shape) == (1, 10, 64, 64)
        want = want[0].cpu().numpy()
        assert any(mp.any() for mp in want)
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(cli_dir, "%s_%d.png" % (stem, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c]), (stem, c)
        assert not os.path.exists(os.path.join(cli_dir, "%s_10.png" % stem))
        lines = re.findall(r"^causal %s class (\d+): deletion (\S+) insertion (\S+)$" % stem, printed, flags=re.M)
        assert len(lines) == 1, printed
        assert all(np.isfinite(float(v)) for v in lines[0][1:])
    assert not os.path.exists(os.path.join(cli_dir, "cam_0.png")) and len(re.findall(r"^causal ", printed, flags=re.M)) == 3
