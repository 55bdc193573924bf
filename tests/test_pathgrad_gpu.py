"""Integrated Gradients / SmoothGrad (-m gpu): the five kernels of csrc/pathgrad.hip against float64, their refusals,
tools/attribution.py integrated_gradients / smoothgrad / gradient_maps on a polynomial black box and on whole models, and
test.py run_ig / run_smoothgrad / run_causal.  No reference program is involved: every expected value is float64 arithmetic
on seeded inputs, and for the whole models the float64 sum over the HIP path's own gradients.

EPS = 2^-24 (half an fp32 ulp, relative).  Every bound is twice a worst case (one is not: see grad_accumulate):

path_images      one fma of the fp32 difference d = fl(x - x'): |out - (x' + a d)| <= EPS |x' + a d|; bound 2 EPS |ref|.
noise_images     assumes at most 4 ulp (8 EPS relative) for logf, sqrtf, sinf and cosf.  rad = sqrtf(-2 logf(u)): 8 EPS from logf,
                 halved by the root, plus 8 EPS of sqrtf: 12 EPS.  The angle fl(c u) moves by EPS * 2 pi <= 6.3 EPS, and sin / cos
                 by as much; sinf / cosf add 8 EPS and the product 1 EPS: |z - z64| <= (12 + 6.3 + 8 + 1) EPS rad < 31 EPS rad;
                 bound 64 EPS rad64.  With an image, the fma adds EPS (|x| + sigma |z|).
grad_accumulate  N additions in fp64, each within 2^-53 of a partial sum that is at most |acc0| + sum_j |w_j g_j| (w g is exact,
                 (w g) g rounds inside the fma that adds it): N 2^-53 (|acc0| + sum_j |w_j g_j|).  The inputs keep |acc0| below
                 sum_j |w_j g_j| (asserted), so the issue's bound N 2^-52 sum_j |w_j g_j| covers it (and the same with g^2); here
                 the factor of two is taken up by the starting value.
attr_finish      float64 arithmetic (errors of order 2^-53, times at most 10 for the variance, whose inputs keep it above a tenth
                 of the mean square) and one rounding to fp32: EPS |ref|; bound 2 EPS |ref|.  The total adds E fp64 terms:
                 E 2^-53 sum |out|; bound E 2^-52 sum |out|.
channel_mean     a float64 sum and quotient, one rounding to fp32: EPS |mean| <= EPS mean|x|; bound 2 EPS mean|x|.
whole models     the tools add the same fp32 gradients in float64 and round once: EPS |x - x'| sum_i |w_i g_i| (and EPS mean|g|,
                 EPS mean g^2); bounds 4 EPS of those, as the issue sets them."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402
from test_pathgrad_cpu import normal_fp64                                   # noqa: E402

SENTINEL = -777.25
EPS = 2.0 ** -24

# ((C, H, W), the buffers written start one element past a 16-byte boundary)
CASES = [((1, 5, 7), False),          # the one-element form, E % 4 = 3
         ((3, 64, 64), False),        # the 16-byte form, more than one workgroup
         ((3, 33, 47), False),        # E = 4653: odd, more than one workgroup
         ((1, 16, 16), True)]         # E a multiple of 4 at a misaligned pointer: the one-element form
CASE_IDS = ["x".join(str(v) for v in s) + ("_off1" if off else "") for s, off in CASES]


def off1(t):
    """the same data on the device at a pointer one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def batch_buffer(n, shape, off):
    """(out [n, *shape] filled with the sentinel, the sentinel image behind it), dense or starting one float off"""
    E = int(np.prod(shape))
    flat = torch.full(((n + 1) * E + 1,), SENTINEL, device="cuda")
    start = 1 if off else 0
    whole = flat[start:start + (n + 1) * E].view((n + 1,) + tuple(shape))
    assert (whole.data_ptr() % 16 != 0) == bool(off)
    return whole[:n], whole[n]


@functools.lru_cache(maxsize=None)
def case_inputs(shape):
    """(image, base, alphas [12] with alphas[8] = 0) on the CPU: computed once, shared, never changed"""
    gen = torch.Generator().manual_seed(9000 + int(np.prod(shape)))
    image, base = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    alphas = torch.rand(12, generator=gen)
    alphas[8] = 0.0
    return image, base, alphas


def report(what, err, bound):
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), (what, float(err.max()), ratio)


# ------------------------------------------------------------------------------------------------ 1: K.path_images
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_path_images_against_fp64(shape, off):
    from scouter_amd import kernels as K
    image, base, alphas = case_inputs(shape)
    N, first, n = 12, 7, 5
    xd, bd, ad = image.cuda(), base.cuda(), alphas.cuda()
    out, behind = batch_buffer(n, shape, off)
    got = K.path_images(xd, bd, ad, out, first)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((behind == SENTINEL).all())        # the image behind the slice is untouched
    d = (image - base).double()                                                          # the fp32 difference, exactly
    ref = base.double()[None] + alphas[first:first + n].double().view(-1, 1, 1, 1) * d[None]
    report("path_images %s" % (shape,), (out.cpu().double() - ref).abs(), 2 * EPS * ref.abs())
    assert torch.equal(out[8 - first].cpu(), base)                                       # alpha = 0: the baseline, bit for bit
    # two consecutive pieces equal one call
    two, _ = batch_buffer(n, shape, off)
    K.path_images(xd, bd, ad, two[:2], first)
    K.path_images(xd, bd, ad, two[2:], first + 2)
    assert torch.equal(two, out)
    # base=None equals a zero tensor bit for bit
    none, _ = batch_buffer(n, shape, off)
    zero, _ = batch_buffer(n, shape, off)
    K.path_images(xd, None, ad, none, first)
    K.path_images(xd, torch.zeros_like(xd), ad, zero, first)
    assert torch.equal(none, zero)
    ref0 = alphas[first:first + n].double().view(-1, 1, 1, 1) * image.double()[None]
    report("path_images %s base=None" % (shape,), (none.cpu().double() - ref0).abs(), 2 * EPS * ref0.abs())
    # the 16-byte form (dense buffers) and the one-element form (the same data at a misaligned pointer): equal bits
    dense, _ = batch_buffer(n, shape, False)
    moved, _ = batch_buffer(n, shape, True)
    K.path_images(xd, bd, ad, dense, first)
    K.path_images(off1(image), off1(base), ad, moved, first)
    assert torch.equal(dense, moved) and torch.equal(dense, out)


# ------------------------------------------------------------------------------------------------ 2: K.noise_images
SEED = 0x9E3779B97F4A7C15                                                                # both key words in use, the high bits set


def z_reference(seed, first, n, shape):
    """float64 (z, rad) [n, *shape] of the samples first .. first + n - 1"""
    E = int(np.prod(shape))
    pairs = [normal_fp64(seed, first + j, E) for j in range(n)]
    z = torch.from_numpy(np.stack([p[0] for p in pairs])).view((n,) + tuple(shape))
    rad = torch.from_numpy(np.stack([p[1] for p in pairs])).view((n,) + tuple(shape))
    return z, rad


@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_noise_images_against_restated_philox(shape, off):
    from scouter_amd import kernels as K
    image, _, _ = case_inputs(shape)
    first, n = 3, 5
    z64, rad64 = z_reference(SEED, first, n, shape)
    zero = torch.zeros(shape, device="cuda")
    out, behind = batch_buffer(n, shape, off)
    K.noise_images(zero, out, 1.0, SEED, first)
    torch.cuda.synchronize()
    assert bool((behind == SENTINEL).all())
    report("noise_images %s image 0 sigma 1" % (shape,), (out.cpu().double() - z64).abs(), 64 * EPS * rad64)
    # pieces equal one call; the two forms give equal bits
    two, _ = batch_buffer(n, shape, off)
    K.noise_images(zero, two[:3], 1.0, SEED, first)
    K.noise_images(zero, two[3:], 1.0, SEED, first + 3)
    assert torch.equal(two, out)
    dense, _ = batch_buffer(n, shape, False)
    moved, _ = batch_buffer(n, shape, True)
    K.noise_images(zero, dense, 1.0, SEED, first)
    K.noise_images(off1(zero), moved, 1.0, SEED, first)
    assert torch.equal(dense, moved) and torch.equal(dense, out)
    # sigma = 0 returns the image bit for bit
    xd = image.cuda()
    same, _ = batch_buffer(n, shape, off)
    K.noise_images(xd, same, 0.0, SEED, first)
    assert all(torch.equal(same[j].cpu(), image) for j in range(n))
    # a non-zero image
    sigma = 0.75
    noisy, _ = batch_buffer(n, shape, off)
    K.noise_images(xd, noisy, sigma, SEED, first)
    ref = image.double()[None] + sigma * z64
    bound = 2 * EPS * (image.double().abs()[None] + sigma * z64.abs()) + sigma * 64 * EPS * rad64
    report("noise_images %s sigma %.2f" % (shape, sigma), (noisy.cpu().double() - ref).abs(), bound)
    # seeds that differ only in the high word differ
    other, _ = batch_buffer(n, shape, off)
    K.noise_images(zero, other, 1.0, SEED ^ (1 << 32), first)
    assert not torch.equal(other, out)
    zo, ro = z_reference(SEED ^ (1 << 32), first, n, shape)
    report("noise_images %s other high word" % (shape,), (other.cpu().double() - zo).abs(), 64 * EPS * ro)


@pytest.mark.parametrize("seed", [0, 1])
def test_noise_images_statistics(seed):
    """8 samples of 3 * 64 * 64 elements: |mean|, |variance - 1| and the correlation of the first and second half of the samples
    within 4 standard errors (1 / sqrt(n), sqrt(2 / n), 1 / sqrt(n / 2)); the float64 restatement alone stays below 1.8"""
    from scouter_amd import kernels as K
    shape, n = (3, 64, 64), 8
    zero = torch.zeros(shape, device="cuda")
    out, _ = batch_buffer(n, shape, False)
    K.noise_images(zero, out, 1.0, seed, 0)
    two, _ = batch_buffer(n, shape, False)
    K.noise_images(zero, two[:3], 1.0, seed, 0)                                           # pieces 0 .. 2 and 3 .. 7
    K.noise_images(zero, two[3:], 1.0, seed, 3)
    assert torch.equal(two, out)
    z = out.cpu().double().numpy().reshape(n, -1)
    z64, rad64 = z_reference(seed, 0, n, shape)
    report("noise_images seed %d" % seed, (out.cpu().double() - z64).abs(), 64 * EPS * rad64)
    a, b = z[:4].ravel(), z[4:].ravel()
    figures = (abs(z.mean()) * np.sqrt(z.size), abs(z.var() - 1.0) * np.sqrt(z.size / 2.0),
               abs(float(np.corrcoef(a, b)[0, 1])) * np.sqrt(a.size))
    print("seed %d: |mean|, |var - 1|, |corr| in standard errors: %.2f %.2f %.2f (bound 4)" % ((seed,) + figures))
    assert all(f <= 4.0 for f in figures)


# ------------------------------------------------------------------------------------------------ 3: K.grad_accumulate
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("squares", [True, False], ids=["sq", "nosq"])
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_grad_accumulate_against_fp64(shape, off, squares, weighted):
    from scouter_amd import kernels as K
    N = 12
    gen = torch.Generator().manual_seed(9100 + int(np.prod(shape)))
    g = torch.randn((N,) + shape, generator=gen)
    w = torch.rand(N, generator=gen) + 0.5 if weighted else None
    acc0 = (torch.rand(shape, generator=gen, dtype=torch.float64) - 0.5)                 # non-zero, |acc0| <= 0.5
    sq0 = torch.rand(shape, generator=gen, dtype=torch.float64) * 0.25 + 0.01
    w64 = w.double() if weighted else torch.ones(N, dtype=torch.float64)
    g64 = g.double()
    ref = acc0 + torch.einsum("j,jchw->chw", w64, g64)
    ref_sq = sq0 + torch.einsum("j,jchw->chw", w64, g64 * g64)
    mag = torch.einsum("j,jchw->chw", w64, g64.abs())
    mag_sq = torch.einsum("j,jchw->chw", w64, g64 * g64)
    assert bool((acc0.abs() <= mag).all()) and bool((sq0 <= mag_sq).all())               # a condition on the inputs (docstring)

    def fresh(t):
        return off1(t) if off else t.cuda()

    gd, wd = (off1(g) if off else g.cuda()), (w.cuda() if weighted else None)
    one, one_sq = fresh(acc0), (fresh(sq0) if squares else None)
    assert K.grad_accumulate(gd, wd, one, one_sq, 0) is one
    pieces, pieces_sq = fresh(acc0), (fresh(sq0) if squares else None)
    for lo, hi in ((0, 5), (5, 10), (10, 12)):                                            # 5 / 5 / 2
        K.grad_accumulate(gd[lo:hi], wd, pieces, pieces_sq, lo)
    torch.cuda.synchronize()
    report("grad_accumulate %s" % (shape,), (one.cpu() - ref).abs(), N * 2.0 ** -52 * mag)
    assert torch.equal(one, pieces)
    assert bool((one.cpu() != acc0).any())
    if squares:
        report("grad_accumulate %s squares" % (shape,), (one_sq.cpu() - ref_sq).abs(), N * 2.0 ** -52 * mag_sq)
        assert torch.equal(one_sq, pieces_sq)
    # the 16-byte form and the one-element form: equal bits
    dense, dense_sq = acc0.cuda(), (sq0.cuda() if squares else None)
    K.grad_accumulate(g.cuda(), wd, dense, dense_sq, 0)
    assert torch.equal(dense, one) and (not squares or torch.equal(dense_sq, one_sq))


# ------------------------------------------------------------------------------------------------ 4: K.attr_finish
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_attr_finish_against_fp64(shape, off):
    from scouter_amd import kernels as K
    n = 7
    gen = torch.Generator().manual_seed(9200 + int(np.prod(shape)))
    g = torch.randn((n,) + shape, generator=gen).double()
    g = g - g.mean(0) + 0.5 * g.std(0, unbiased=False)            # every element: mean = half its deviation, variance = 0.8 mean square
    acc, acc_sq = g.sum(0), (g * g).sum(0)
    image, base, _ = case_inputs(shape)
    inv_n = 1.0 / n
    mean, mean_sq = acc * inv_n, acc_sq * inv_n
    var = mean_sq - mean * mean
    assert bool((var >= 0.1 * mean_sq).all())                                             # the variance is not a small difference
    refs = {K.ATTR_IG: (image - base).double() * acc, K.ATTR_MEAN: mean, K.ATTR_MEAN_SQ: mean_sq, K.ATTR_VAR: var}
    move = off1 if off else (lambda t: t.cuda())
    ad, sd, xd, bd = move(acc), move(acc_sq), move(image), move(base)
    E = acc.numel()
    for mode, ref in refs.items():
        out = move(torch.full(shape, SENTINEL))
        total = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
        args = dict(acc=None if mode == K.ATTR_MEAN_SQ else ad, acc_sq=sd if mode >= K.ATTR_MEAN_SQ else None,
                    image=xd if mode == K.ATTR_IG else None, base=bd if mode == K.ATTR_IG else None, inv_n=inv_n)
        assert K.attr_finish(mode, out=out, total=total, **args) is out
        plain = K.attr_finish(mode, **args)                                               # no total, a new output
        again_total = torch.zeros(1, dtype=torch.float64, device="cuda")
        again = K.attr_finish(mode, total=again_total, **args)
        torch.cuda.synchronize()
        assert plain.dtype == torch.float32 and tuple(plain.shape) == tuple(shape)
        assert torch.equal(plain, out) and torch.equal(again, out)
        report("attr_finish mode %d %s" % (mode, shape), (out.cpu().double() - ref).abs(), 2 * EPS * ref.abs())
        o64 = out.cpu().double()
        terr, tbound = abs(float(total) - float(o64.sum())), E * 2.0 ** -52 * float(o64.abs().sum())
        print("attr_finish mode %d %s total: err %.3e, bound %.3e" % (mode, shape, terr, tbound))
        assert terr <= tbound and torch.equal(total, again_total)
    # the two forms give equal bits; the baseline None is a zero baseline
    dense = K.attr_finish(K.ATTR_IG, acc.cuda(), image=image.cuda(), base=base.cuda())
    assert torch.equal(dense, K.attr_finish(K.ATTR_IG, ad, image=xd, base=bd))
    assert torch.equal(K.attr_finish(K.ATTR_IG, ad, image=xd), K.attr_finish(K.ATTR_IG, ad, image=xd, base=torch.zeros_like(xd)))


# ------------------------------------------------------------------------------------------------ 5: K.channel_mean, gradient_maps
@pytest.mark.parametrize("absolute", [False, True], ids=["signed", "abs"])
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_channel_mean_against_fp64(shape, off, absolute):
    from scouter_amd import kernels as K
    x = torch.randn((2, 3) + shape, generator=torch.Generator().manual_seed(9300 + int(np.prod(shape))))    # [2, 3, C, H, W]
    xd = off1(x) if off else x.cuda()
    got = K.channel_mean(xd, absolute=absolute)
    into = K.channel_mean(xd, absolute=absolute, out=torch.full((2, 3) + shape[1:], SENTINEL, device="cuda"))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3) + shape[1:] and torch.equal(got, into)
    v = x.double().abs() if absolute else x.double()
    report("channel_mean %s" % (shape,), (got.cpu().double() - v.mean(dim=2)).abs(), 2 * EPS * x.double().abs().mean(dim=2))
    assert torch.equal(K.channel_mean(x.cuda(), absolute=absolute), got)                  # the two forms: equal bits


@pytest.mark.parametrize("shape,min_level", [((2, 3, 3, 33, 47), 0.0), ((2, 3, 3, 33, 47), 0.3), ((1, 1, 1, 5, 7), 0.0),
                                             ((1, 1, 1, 5, 7), 0.3), ((1, 2, 1, 64, 64), 0.3)],
                         ids=["3ch_33x47_min0", "3ch_33x47_min0.3", "1x1x5x7_min0", "1x1x5x7_min0.3", "1ch_64_min0.3"])
def test_gradient_maps_against_attribution_maps(shape, min_level):
    """the shapes and seed of test_attribution_maps_against_numpy: bytewise K.heat_maps(K.channel_mean(.)), and within one grey
    level (the bar of the existing map tests) of the host's attribution_maps"""
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import attribution_maps, gradient_maps
    g = torch.randn(shape, generator=torch.Generator().manual_seed(7)).cuda()
    maps = gradient_maps(g, min_level=min_level)
    assert maps.dtype == torch.uint8 and maps.is_cuda and tuple(maps.shape) == shape[:2] + shape[3:]
    assert torch.equal(maps, K.heat_maps(K.channel_mean(g), min_level))
    host = attribution_maps(g, min_level=min_level)
    diff = np.abs(maps.cpu().numpy().astype(np.int64) - host.astype(np.int64)).max()
    print("gradient_maps %s min_level %.1f: max difference from attribution_maps %d grey levels" % (shape, min_level, diff))
    assert diff <= 1 and int(maps.max()) >= 254 and int(maps.min()) == 0
    mag = gradient_maps(g, min_level=min_level, absolute=True)
    assert torch.equal(mag, K.heat_maps(K.channel_mean(g, absolute=True), min_level))
    with pytest.raises(ValueError):
        gradient_maps(g[0])


# ------------------------------------------------------------------------------------------------ 6: refusals
BAD = {"path_images": ["null", "n0", "past_N", "first_low", "out_shape", "base_shape"],
       "noise_images": ["null", "n0", "past_N", "sigma", "out_shape"],
       "grad_accumulate": ["null", "n0", "past_N", "first_low", "out_shape", "same"],
       "attr_finish": ["null", "n0", "mode4", "out_shape", "no_ws"],
       "channel_mean": ["null", "n0", "out_shape", "rank"]}


@pytest.mark.parametrize("call,bad", [(c, b) for c in BAD for b in BAD[c]])
def test_pathgrad_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, a size of 0, a range past N (past 2^31 samples for noise_images, which has no N), a negative first, a wrong
    shape through the wrapper, a negative sigma, acc_sq = acc, mode 4, a total without its workspace: a RuntimeError naming the
    call, the outputs untouched, and a good call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    shape, n, N = (2, 6, 6), 4, 6
    E = int(np.prod(shape))
    image = torch.ones(shape, device="cuda")
    alphas = torch.full((N,), 0.5, device="cuda")
    out = torch.full((n,) + shape, SENTINEL, device="cuda")
    acc = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    acc_sq = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    res = torch.full(shape, SENTINEL, device="cuda")
    total = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
    cm = torch.full((n,) + shape[1:], SENTINEL, device="cuda")
    grads = torch.ones((n,) + shape, device="cuda")
    lib = _native.lib()
    first = {"past_N": N - n + 1, "first_low": -1}.get(bad, 1)
    with pytest.raises(RuntimeError, match=call):
        if call == "path_images":
            if bad == "null":
                _native.check(lib.scouter_path_images_f32(image.data_ptr(), None, None, out.data_ptr(), 1, n, N, E, None), call)
            elif bad == "n0":
                K.path_images(image, None, alphas, out[:0], first)
            elif bad == "out_shape":
                K.path_images(image, None, alphas, out.view(n, shape[0], -1), first)
            elif bad == "base_shape":
                K.path_images(image, image[0], alphas, out, first)
            else:
                K.path_images(image, None, alphas, out, first)
        elif call == "noise_images":
            if bad == "null":
                _native.check(lib.scouter_noise_images_f32(None, out.data_ptr(), 1.0, 0, 0, 0, n, E, None), call)
            elif bad == "n0":
                K.noise_images(image, out[:0], 1.0, 0, 0)
            elif bad == "past_N":
                K.noise_images(image, out, 1.0, 0, 2 ** 31 - n + 1)
            elif bad == "sigma":
                K.noise_images(image, out, -0.5, 0, 0)
            else:
                K.noise_images(image, out.view(n, shape[0], -1), 1.0, 0, 0)
        elif call == "grad_accumulate":
            if bad == "null":
                _native.check(lib.scouter_grad_accumulate_f64(grads.data_ptr(), None, None, None, 0, n, n, E, None), call)
            elif bad == "n0":
                K.grad_accumulate(grads[:0], alphas, acc, acc_sq, first)
            elif bad == "out_shape":
                K.grad_accumulate(grads, alphas, acc.view(shape[0], -1), None, first)
            elif bad == "same":
                K.grad_accumulate(grads, alphas, acc, acc, first)
            else:
                K.grad_accumulate(grads, alphas, acc, acc_sq, first)
        elif call == "attr_finish":
            if bad == "null":
                _native.check(lib.scouter_attr_finish_f32(0, acc.data_ptr(), None, None, None, 1.0, res.data_ptr(), None, E, None, 0,
                                                          None), call)                  # mode 0 without its image
            elif bad == "n0":
                K.attr_finish(K.ATTR_MEAN, acc[:0], out=res[:0])
            elif bad == "mode4":
                K.attr_finish(4, acc, acc_sq, image, out=res, total=total)
            elif bad == "out_shape":
                K.attr_finish(K.ATTR_MEAN, acc, out=res.view(shape[0], -1))
            else:
                _native.check(lib.scouter_attr_finish_f32(1, acc.data_ptr(), None, None, None, 1.0, res.data_ptr(), total.data_ptr(),
                                                          E, None, 0, None), call)
        else:
            if bad == "null":
                _native.check(lib.scouter_channel_mean_f32(grads.data_ptr(), None, n, shape[0], shape[1] * shape[2], 0, None), call)
            elif bad == "n0":
                K.channel_mean(grads[:0], out=cm[:0])
            elif bad == "out_shape":
                K.channel_mean(grads, out=cm.view(n, -1))
            else:
                K.channel_mean(grads[0, 0])
    torch.cuda.synchronize()
    for t in (out, acc, acc_sq, res, total, cm):
        assert bool((t == SENTINEL).all())
    test_path_images_against_fp64(*CASES[0])
    test_attr_finish_against_fp64(*CASES[3])


# ------------------------------------------------------------------------------------------------ 7: a polynomial black box
class Polynomial(torch.nn.Module):
    """out[n, c] = sum_e A[c, e] x[n, e]^p / p: elementwise, then one sum; d out_c / dx = A[c] x^(p - 1)"""

    def __init__(self, A, p):
        super().__init__()
        self.register_buffer("A", A)
        self.p = p

    def forward(self, x):
        return (self.A[None] * x.flatten(1)[:, None, :] ** self.p / self.p).sum(dim=2)


@pytest.mark.parametrize("p,method,n_steps", [(3, "gausslegendre", 2), (2, "riemann_trapezoid", 5)], ids=["cubic_gl2", "square_trap5"])
def test_integrated_gradients_is_exact_on_a_polynomial(p, method, n_steps):
    """the gradient along the path is A (alpha x)^(p - 1), a polynomial of degree p - 1 in alpha that the rule integrates exactly:
    attr = A x^p / p, and completeness holds to rounding.  Positive inputs and coefficients: nothing cancels.  The fp32 path
    rounds alpha x, the power, the product with A, the rounded nodes and weights and the final product: under 12 EPS relative,
    bound 32 EPS |attr|; out(x) is an fp32 sum of 192 positive terms: bound 64 EPS sum |attr| for delta."""
    from scouter_amd.tools.attribution import integrated_gradients
    gen = torch.Generator().manual_seed(9400 + p)
    x = (torch.rand((2, 3, 8, 8), generator=gen) + 0.5)
    A = (torch.rand((4, 3 * 8 * 8), generator=gen) + 0.1)
    model = Polynomial(A, p).cuda()
    model.train()
    attr, delta = integrated_gradients(model, x.cuda(), n_steps=n_steps, method=method, batch=2, return_delta=True)
    torch.cuda.synchronize()
    assert tuple(attr.shape) == (2, 4, 3, 8, 8) and attr.dtype == torch.float32 and tuple(delta.shape) == (2, 4) and model.training
    ref = A.double().view(1, 4, 3, 8, 8) * x.double()[:, None] ** p / p
    report("integrated_gradients x^%d %s" % (p, method), (attr.cpu().double() - ref).abs(), 32 * EPS * ref.abs())
    dbound = 64 * EPS * ref.abs().sum(dim=(2, 3, 4))
    print("delta", delta.cpu().tolist())
    report("integrated_gradients x^%d %s delta" % (p, method), delta.cpu().double().abs(), dbound)
    own = integrated_gradients(model, x.cuda(), classes=torch.tensor([3, 1]), n_steps=n_steps, method=method, batch=50)
    assert torch.equal(own[0, 0], attr[0, 3]) and torch.equal(own[1, 0], attr[1, 1])       # one chunk against chunks of 2


# ------------------------------------------------------------------------------------------------ 8: whole models
def model_args(use_slot):
    return argparse.Namespace(model="resnet18", pre_trained=False, num_classes=10, dataset="MNIST", use_slot=use_slot,
                              use_pre=False, grad=False, channel=O.ARCHS["resnet18"]["channel"], slots_per_class=1, hidden_dim=64,
                              freeze_layers=0, vis=False, vis_id=0, loss_status=1, power=1, to_k_layer=1, lambda_value=LAMBDA)


def build(use_slot, seed=11):
    from scouter_amd.sloter.slot_model import SlotModel
    torch.manual_seed(seed)
    m = SlotModel(model_args(use_slot)).cuda()
    images = torch.randn((2, 1, 64, 64), generator=torch.Generator().manual_seed(seed + 1)).cuda()
    return m, images


def bn_buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def chunk_gradients(m, images, classes, fill, N, batch):
    """float64 [B, K, N, C, H, W] on the CPU: the HIP path's own gradients, input_gradients(m, chunk, classes=[c]) on the chunks
    fill(b, buf, first) writes, at the chunking of the tools"""
    from scouter_amd.tools.attribution import input_gradients
    B = images.shape[0]
    rows = []
    for b in range(B):
        per_class = []
        for c in classes:
            parts = []
            for first in range(0, N, batch):
                n = min(batch, N - first)
                chunk = fill(b, torch.empty((n,) + tuple(images.shape[1:]), device="cuda"), first)
                parts.append(input_gradients(m, chunk, classes=[c])[:, 0].cpu().double())
            per_class.append(torch.cat(parts))
        rows.append(torch.stack(per_class))
    return torch.stack(rows)


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_integrated_gradients_on_whole_models(use_slot):
    """resnet18 / MNIST stem / 64^2 / batch 2; n_steps = 12 in chunks of 5, 5, 2, classes [0, 3], a random [1, 64, 64] baseline"""
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import ig_quadrature, integrated_gradients
    m, images = build(use_slot)
    name = "slot" if use_slot else "fc"
    n_steps, batch, classes = 12, 5, [0, 3]
    baseline = torch.randn((1, 64, 64), generator=torch.Generator().manual_seed(21)).cuda()
    alphas, weights = ig_quadrature(n_steps)
    ad = alphas.cuda()
    m.train()
    g = chunk_gradients(m, images, classes, lambda b, buf, first: K.path_images(images[b], baseline, ad, buf, first), n_steps, batch)
    w64 = weights.double().view(1, 1, -1, 1, 1, 1)
    d = (images - baseline[None]).cpu().double()[:, None]                                  # the fp32 difference, exactly
    ref, mag = d * (w64 * g).sum(dim=2), d.abs() * (w64 * g).abs().sum(dim=2)
    before = bn_buffers(m)
    attr, delta = integrated_gradients(m, images, classes=classes, baseline=baseline, n_steps=n_steps, batch=batch,
                                       return_delta=True)
    torch.cuda.synchronize()
    assert tuple(attr.shape) == (2, 2, 1, 64, 64) and attr.dtype == torch.float32 and attr.is_cuda
    assert tuple(delta.shape) == (2, 2) and delta.dtype == torch.float32
    report("integrated_gradients %s" % name, (attr.cpu().double() - ref).abs(), 4 * EPS * mag)
    assert bool(torch.isfinite(attr).all()) and float(attr.abs().max()) > 0
    assert m.training                                                                     # the caller's mode is restored
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    # a second call: equal bits; without delta: the same attributions
    attr2, delta2 = integrated_gradients(m, images, classes=classes, baseline=baseline, n_steps=n_steps, batch=batch,
                                         return_delta=True)
    assert torch.equal(attr2, attr) and torch.equal(delta2, delta)
    assert torch.equal(integrated_gradients(m, images, classes=classes, baseline=baseline, n_steps=n_steps, batch=batch), attr)
    # a [B, C, H, W] baseline
    assert torch.equal(integrated_gradients(m, images, classes=classes, baseline=baseline[None].expand(2, -1, -1, -1),
                                            n_steps=n_steps, batch=batch), attr)
    # delta against float64 from the returned tensors and the model's own eval outputs
    m.eval()
    with torch.no_grad():
        ends = torch.stack([m(torch.stack([baseline, images[b]])) for b in range(2)]).cpu().double()     # [B, 2, n_outputs]
    m.train()
    want = attr.cpu().double().sum(dim=(2, 3, 4)) - (ends[:, 1, classes] - ends[:, 0, classes])
    E = 64 * 64
    dbound = E * 4 * EPS * attr.cpu().double().abs().amax(dim=(2, 3, 4))
    print("integrated_gradients %s: delta %s, out(x) - out(x') %s" % (name, delta.cpu().tolist(),
                                                                      (ends[:, 1, classes] - ends[:, 0, classes]).tolist()))
    report("integrated_gradients %s delta" % name, (delta.cpu().double() - want).abs(), dbound)
    # the None, list and LongTensor forms of classes agree slice for slice (zero baseline: None equals explicit zeros)
    every = integrated_gradients(m, images, n_steps=n_steps, batch=batch)
    assert tuple(every.shape) == (2, 10, 1, 64, 64)
    two = integrated_gradients(m, images, classes=classes, n_steps=n_steps, batch=batch)
    assert torch.equal(two[:, 0], every[:, 0]) and torch.equal(two[:, 1], every[:, 3])
    own = integrated_gradients(m, images, classes=torch.tensor([7, 2]), n_steps=n_steps, batch=batch)
    assert tuple(own.shape) == (2, 1, 1, 64, 64) and torch.equal(own[0, 0], every[0, 7]) and torch.equal(own[1, 0], every[1, 2])
    zeros = integrated_gradients(m, images, classes=classes, baseline=torch.zeros((1, 64, 64), device="cuda"), n_steps=n_steps,
                                 batch=batch)
    assert torch.equal(zeros, two)
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    # argument errors
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            integrated_gradients(m, images, classes=bad, n_steps=n_steps, batch=batch)
    for kwargs in (dict(classes=torch.tensor([0, 1, 2])), dict(batch=0), dict(n_steps=0), dict(method="simpson"),
                   dict(n_steps=1, method="riemann_trapezoid"), dict(baseline=torch.zeros((64, 64), device="cuda")),
                   dict(baseline=torch.zeros((3, 1, 64, 64), device="cuda"))):
        with pytest.raises(ValueError):
            integrated_gradients(m, images, **{**dict(n_steps=n_steps, batch=batch), **kwargs})
    with pytest.raises(ValueError):
        integrated_gradients(m, images[0], n_steps=n_steps, batch=batch)
    assert m.training


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_smoothgrad_on_whole_models(use_slot):
    """the same models and images; n_samples = 7 in chunks of 3, 3, 1, sigma = 0.5, classes [0, 3]: the three kinds against the
    float64 mean, mean of squares and variance of the HIP path's own gradients on K.noise_images chunks"""
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import smoothgrad
    m, images = build(use_slot)
    name = "slot" if use_slot else "fc"
    n_samples, batch, sigma, classes, seed = 7, 3, 0.5, [0, 3], 5
    m.train()
    g = chunk_gradients(m, images, classes, lambda b, buf, first: K.noise_images(images[b], buf, sigma, seed, first), n_samples,
                        batch)
    mean, mean_abs, mean_sq = g.mean(dim=2), g.abs().mean(dim=2), (g * g).mean(dim=2)
    before = bn_buffers(m)
    kw = dict(classes=classes, n_samples=n_samples, sigma=sigma, batch=batch, seed=seed)
    got = {kind: smoothgrad(m, images, kind=kind, **kw) for kind in ("smoothgrad", "smoothgrad_sq", "vargrad")}
    torch.cuda.synchronize()
    for v in got.values():
        assert tuple(v.shape) == (2, 2, 1, 64, 64) and v.dtype == torch.float32 and v.is_cuda and bool(torch.isfinite(v).all())
    report("smoothgrad %s" % name, (got["smoothgrad"].cpu().double() - mean).abs(), 4 * EPS * mean_abs)
    report("smoothgrad_sq %s" % name, (got["smoothgrad_sq"].cpu().double() - mean_sq).abs(), 4 * EPS * mean_sq)
    report("vargrad %s" % name, (got["vargrad"].cpu().double() - (mean_sq - mean * mean)).abs(), 4 * EPS * mean_sq)
    assert float(got["vargrad"].min()) >= 0.0 and float(got["vargrad"].max()) > 0.0
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    # the same seed repeats bit for bit, two seeds differ, sigma = 0 is the plain gradient
    assert torch.equal(smoothgrad(m, images, **kw), got["smoothgrad"])
    assert not torch.equal(smoothgrad(m, images, **{**kw, "seed": seed + 1}), got["smoothgrad"])
    # the forms of classes agree slice for slice (the noise is common to the classes of a call)
    every = smoothgrad(m, images, **{**kw, "classes": None})
    assert tuple(every.shape) == (2, 10, 1, 64, 64)
    assert torch.equal(every[:, 0], got["smoothgrad"][:, 0]) and torch.equal(every[:, 3], got["smoothgrad"][:, 1])
    own = smoothgrad(m, images, **{**kw, "classes": torch.tensor([7, 2])})
    assert torch.equal(own[0, 0], every[0, 7]) and torch.equal(own[1, 0], every[1, 2])
    for bad in ([10], [-1]):
        with pytest.raises(IndexError):
            smoothgrad(m, images, **{**kw, "classes": bad})
    for kwargs in (dict(batch=0), dict(n_samples=0), dict(sigma=-1.0), dict(kind="smooth"), dict(classes=torch.tensor([1]))):
        with pytest.raises(ValueError):
            smoothgrad(m, images, **{**kw, **kwargs})
    with pytest.raises(ValueError):
        smoothgrad(m, images[0], **kw)
    assert m.training


# ------------------------------------------------------------------------------------------------ 9: the test tool
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_test_tool_writes_ig_and_smoothgrad_maps(use_slot, tmp_path, capsys):
    """scouter_amd.test run_ig / run_smoothgrad: ten 64 x 64 PNGs each, byte for byte gradient_maps of the tool functions;
    run_causal prints one line for the family `ig` and one for `smoothgrad` with finite scores in [0, 1]"""
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.tools.attribution import gradient_maps, integrated_gradients, smoothgrad
    m, images = build(use_slot)
    args = model_args(use_slot)
    args.device, args.grad_min_level, args.causal_step, args.rise_batch = "cuda", 0.2, 256, 96
    args.ig_steps, args.ig_batch = 12, 5
    args.smoothgrad_samples, args.smoothgrad_sigma, args.smoothgrad_batch = 7, 0.5, 3
    image = images[0].cpu()
    vis_dir = str(tmp_path / "vis")
    wanted = {"ig": gradient_maps(integrated_gradients(m, images[:1], n_steps=12, batch=5), min_level=0.2)[0].cpu().numpy(),
              "smoothgrad": gradient_maps(smoothgrad(m, images[:1], n_samples=7, sigma=0.5, batch=3), min_level=0.2)[0].cpu().numpy()}
    for stem, runner in (("ig", T.run_ig), ("smoothgrad", T.run_smoothgrad)):
        got, want = runner(args, m, image, vis_dir), wanted[stem]
        assert got.shape == (10, 64, 64) and got.dtype == np.uint8 and np.array_equal(got, want)
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(vis_dir, "%s_%d.png" % (stem, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
        assert not os.path.exists(os.path.join(vis_dir, "%s_10.png" % stem))
        assert any(w.any() for w in want)
    m.eval()
    with torch.no_grad():
        pred = int(m(images[:1]).argmax(dim=1))
    capsys.readouterr()
    scores = T.run_causal(args, m, image, pred, families=["ig", "smoothgrad"])
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("causal ")]
    assert len(lines) == 2 and list(scores) == ["ig", "smoothgrad"]
    for ln, family in zip(lines, ("ig", "smoothgrad")):
        assert ln[:4] == ["causal", family, "class", "%d:" % pred] and ln[4] == "deletion" and ln[6] == "insertion" and len(ln) == 8
        for v in scores[family] + (float(ln[5]), float(ln[7])):
            assert np.isfinite(v) and 0.0 <= v <= 1.0
