"""Insertion / deletion scores (-m gpu): the six kernels of csrc/causal.hip -- kernels.saliency_ranks and causal_step_images
exactly against CPU restatements (a stable argsort, torch.where), kernels.resize_bilinear against F.interpolate in float64,
kernels.separable_filter against the same fp32 taps applied with F.conv2d in float64, kernels.causal_curve / causal_auc against
exp and the trapezoid in float64 -- their refusals, tools/attribution.py causal_metrics on a stub model whose curves are known in
closed form and on whole models against the definition restated over the HIP path's own log-probabilities, slot_saliency, and
test.py --causal true.  No reference program is involved: the definition (include/scouter_hip.h, causal_metrics) is the
specification.

Bounds (EPS = 2^-24, one fp32 rounding of a value of magnitude 1).
resize_bilinear: a source coordinate is counted with three roundings (the scale in / out and the fma round; d + 0.5 and
  s - floor(s) are exact and stand for the third), each of a number below the source size n, so it is off by at most
  3 n EPS and moves the value by at most 3 n EPS |a1 - a0| <= 6 n EPS A per axis, A = max |source| over the neighbours; the blend is three fmas whose three differences
  and three sums round values of at most 2 A and A: 6 EPS A.  Worst case (6 (h + w) + 6) EPS A; the test allows twice that,
  (12 (h + w) + 12) EPS A.  A is taken over the four neighbours widened by one source pixel each way, because a coordinate that
  is an integer in exact arithmetic may round to either side of it and then blends the neighbouring cell (continuously).
separable_filter: klen fma roundings per pass, two passes and the stored intermediate: (2 klen + 4) EPS (filter applied to |x|).
causal_curve: expf within a few ulp: 4 EPS p.  causal_auc: non-negative terms, one rounding per addition, one per weight and
  the division, on top of the curve's own error: (n_points + 8) EPS ref, and exactly 0 where every p is 0."""
import argparse
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402

SENTINEL = -777.25
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1: K.saliency_ranks
def ranks_cpu(v):
    """[M, HW] fp32 (CPU) -> int64 ranks: the inverse permutation of a stable ascending argsort of canon(-v) -- -0.0 made +0.0,
    NaNs moved behind every number in index order"""
    out = torch.empty(v.shape, dtype=torch.int64)
    for m in range(v.shape[0]):
        nan = torch.isnan(v[m])
        key = -v[m].clone()
        key[key == 0] = 0.0                                                 # -0.0 counts as +0.0
        key[nan] = 0.0
        order = torch.argsort(key, stable=True)
        order = torch.cat([order[~nan[order]], order[nan[order]]])         # a stable partition: numbers, then NaNs by index
        out[m, order] = torch.arange(v.shape[1])
    return out


def rank_contents(M, HW, seed):
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.arange(HW, dtype=torch.float32).repeat(M, 1)
    zeros = torch.where(torch.rand((M, HW), generator=gen) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    zeros[:, ::5] = -torch.rand((M, HW), generator=gen)[:, ::5] - 0.5       # a few negatives
    if HW > 1:
        zeros[:, 1] = -0.0
    zeros[:, 0] = 0.0
    nans = torch.randn((M, HW), generator=gen)
    for m in range(M):
        nans[m, torch.randperm(HW, generator=gen)[:3]] = float("nan")
    nans[0, 0] = -float("nan")                                              # a NaN with the sign bit set is a NaN like any other
    return {
        "normal": torch.randn((M, HW), generator=gen),
        "constant": torch.full((M, HW), 0.37),
        "four_levels": torch.randint(0, 4, (M, HW), generator=gen).to(torch.uint8).float(),
        "signed_zeros": zeros,
        "three_nans": nans,
        "descending": -ramp,
        "ascending": ramp,
    }


RANK_SHAPES = [1, 2, 5 * 7, 33 * 47, 63 * 65, 224 * 224, 260 * 260]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("HW", RANK_SHAPES)
def test_saliency_ranks_exact(HW, M):
    from scouter_amd import kernels as K
    for name, v in rank_contents(M, HW, 7000 + HW + M).items():
        want = ranks_cpu(v)
        out = torch.full((M + 2, HW), -7, dtype=torch.int32, device="cuda")
        got = K.saliency_ranks(v.cuda(), out=out[1:M + 1])
        again = K.saliency_ranks(v.cuda())
        torch.cuda.synchronize()
        assert got.data_ptr() == out[1].data_ptr() and bool((out[0] == -7).all()) and bool((out[M + 1] == -7).all()), name
        assert again.dtype == torch.int32 and tuple(again.shape) == (M, HW) and torch.equal(again, out[1:M + 1]), name
        assert torch.equal(out[1:M + 1].cpu().long(), want), (name, HW, M)
        if name == "constant":
            assert torch.equal(want, torch.arange(HW).repeat(M, 1))
        if name == "ascending":
            assert torch.equal(want, torch.arange(HW - 1, -1, -1).repeat(M, 1))
    v3 = torch.randn((M, 3, max(HW // 3, 1)), generator=torch.Generator().manual_seed(5))      # [M, H, W] keeps its shape
    r3 = K.saliency_ranks(v3.cuda())
    assert tuple(r3.shape) == tuple(v3.shape) and torch.equal(r3.cpu().long().view(M, -1), ranks_cpu(v3.view(M, -1)))


# ------------------------------------------------------------------------------------------------ 2: K.resize_bilinear
def _neighbours(n_in, n_out):
    """the two source indices of every destination index (align_corners=False), from float64 coordinates"""
    s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    return i0, (i0 + 1).clamp_max(n_in - 1)


@pytest.mark.parametrize("case", [((7, 7), (224, 224)), ((9, 9), (260, 260)), ((5, 3), (33, 47)), ((64, 64), (64, 64)),
                                  ((33, 47), (7, 5))], ids=lambda c: "%dx%d_to_%dx%d" % (c[0] + c[1]))
def test_resize_bilinear_against_fp64(case):
    """|got - F.interpolate in float64| <= (12 (h + w) + 12) 2^-24 max|source over the four neighbours, widened by one pixel|:
    twice the derived worst case (6 (h + w) + 6) 2^-24 A (module docstring); the maps' own size is a bit-for-bit copy"""
    from scouter_amd import kernels as K
    (h, w), (H, W) = case
    M = 3
    src = torch.randn((M, h, w), generator=torch.Generator().manual_seed(7100 + h + W))
    got = K.resize_bilinear(src.cuda(), H, W)
    again = K.resize_bilinear(src.cuda().view(1, M, h, w), H, W)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (M, H, W)
    assert tuple(again.shape) == (1, M, H, W) and torch.equal(again[0], got)
    ref = F.interpolate(src.double()[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    wide = F.max_pool2d(src.double().abs()[None], 3, stride=1, padding=1)[0]
    y0, y1 = _neighbours(h, H)
    x0, x1 = _neighbours(w, W)
    A = torch.stack([wide[:, ys][:, :, xs] for ys in (y0, y1) for xs in (x0, x1)]).amax(dim=0)
    bound = (12 * (h + w) + 12) * EPS * A
    err = (got.cpu().double() - ref).abs()
    print("resize_bilinear", case, "max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))
    if (h, w) == (H, W):
        assert torch.equal(got.cpu(), src)


# ------------------------------------------------------------------------------------------------ 3: K.separable_filter
def filter_fp64(x, taps):
    """[C, H, W] float64: the fp32 taps applied in float64 along rows, then along columns, zeros outside"""
    k = taps.double()
    r = k.numel() // 2
    x = x.double()[:, None]
    x = F.conv2d(x, k.view(1, 1, 1, -1), padding=(0, r))
    return F.conv2d(x, k.view(1, 1, -1, 1), padding=(r, 0))[:, 0]


@pytest.mark.parametrize("klen", [1, 3, 11, 31])
def test_separable_filter_against_fp64(klen):
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import gaussian_taps
    taps = gaussian_taps(klen, 5.0)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (klen,) and abs(float(taps.double().sum()) - 1.0) < klen * EPS
    assert torch.equal(taps, taps.flip(0)) and int(taps.argmax()) == klen // 2
    i = torch.arange(klen, dtype=torch.float64) - klen // 2
    w64 = torch.exp(-i * i / 50.0)
    assert torch.equal(taps, (w64 / w64.sum()).float())
    for C, H, W in [(1, 1, 1), (1, 5, 7), (1, 64, 64), (3, 224, 224)]:
        x = torch.randn((C, H, W), generator=torch.Generator().manual_seed(7200 + H))
        out = torch.full((C + 1, H, W), SENTINEL, device="cuda")
        got = K.separable_filter(x.cuda(), taps.cuda(), out=out[:C])
        again = K.separable_filter(x.cuda(), taps.cuda())
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and bool((out[C] == SENTINEL).all()) and torch.equal(again, out[:C])
        ref, mag = filter_fp64(x, taps), filter_fp64(x.abs(), taps)
        bound = (2 * klen + 4) * EPS * mag
        err = (got.cpu().double() - ref).abs()
        print("separable_filter klen %d %s: max err %.3e, max err / bound %.3f" %
              (klen, (C, H, W), float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (klen, (C, H, W), float(err.max()))
        if klen == 1:
            assert torch.equal(got.cpu(), x)


# ------------------------------------------------------------------------------------------------ 4: K.causal_step_images
def stream_cpu(image, blurred, ranks, n_points, step, first, n):
    """[n, C, H, W]: points first .. first + n - 1 of the edit stream, restated with torch.where from CPU ranks [K, HW]"""
    C, H, W = image.shape
    out = []
    for g in range(first, first + n):
        k, mode, j = g // (2 * n_points), (g // n_points) % 2, g % n_points
        changed = (ranks[k] < min(j * step, H * W)).view(1, H, W)
        out.append(torch.where(changed, image, blurred) if mode else torch.where(changed, torch.zeros(()), image))
    return torch.stack(out)


def perm_ranks(Kc, HW, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(HW, generator=gen) for _ in range(Kc)]).to(torch.int32)


@pytest.mark.parametrize("case", [(3, 16, 16, 2, 40, False), (2, 33, 47, 2, 100, False), (3, 16, 16, 2, 40, True),
                                  (1, 64, 64, 3, 64, False)], ids=["vec", "scalar_33x47", "misaligned_out", "step_divides"])
def test_causal_step_images_exact(case):
    """the first chunk, a chunk in the middle that crosses a deletion / insertion boundary and a map boundary, a short last
    chunk; `step` not dividing HW; W % 4 != 0 and an output 4 bytes off a 16-byte boundary (the one-pixel-per-thread path)"""
    from scouter_amd import kernels as K
    C, H, W, Kc, step, shifted = case
    HW = H * W
    n_points = -(-HW // step) + 1
    total = 2 * Kc * n_points
    gen = torch.Generator().manual_seed(7300 + HW)
    image, blurred = torch.randn((C, H, W), generator=gen), torch.randn((C, H, W), generator=gen)
    ranks = perm_ranks(Kc, HW, 7301 + HW)
    idev, bdev, rdev = image.cuda(), blurred.cuda(), ranks.cuda()
    chunks = [(0, 5), (n_points - 2, 2 * n_points + 5), (total - 2, 2), (0, total)]
    for first, n in chunks:
        flat = torch.full(((n + 1) * C * HW + 4,), SENTINEL, device="cuda")
        off = 1 if shifted else 0
        assert flat.data_ptr() % 16 == 0
        out = flat[off:off + (n + 1) * C * HW].view(n + 1, C, H, W)
        got = K.causal_step_images(idev, bdev, rdev, out[:n], first, n_points, step)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and bool((out[n] == SENTINEL).all())     # the extra image keeps the sentinel
        assert bool((flat[:off] == SENTINEL).all()) and bool((flat[off + (n + 1) * C * HW:] == SENTINEL).all())
        assert torch.equal(out[:n].cpu(), stream_cpu(image, blurred, ranks, n_points, step, first, n)), (case, first, n)
        if n == total:
            whole = out[:n].cpu().view(Kc, 2, n_points, C, H, W)
            for k in range(Kc):
                assert torch.equal(whole[k, 0, 0], image) and torch.equal(whole[k, 1, 0], blurred)
                assert not whole[k, 0, -1].any() and torch.equal(whole[k, 1, -1], image)
                changed = (whole[k, 0] == 0).all(dim=1).view(n_points, -1).sum(dim=1)      # (randn: no pixel is zero by chance)
                assert changed.tolist() == [min(j * step, HW) for j in range(n_points)]
    # ranks given as [K, H, W] are the same thing
    out = torch.empty((3, C, H, W), device="cuda")
    K.causal_step_images(idev, bdev, rdev.view(Kc, H, W), out, 1, n_points, step)
    assert torch.equal(out.cpu(), stream_cpu(image, blurred, ranks, n_points, step, 1, 3))


# ------------------------------------------------------------------------------------------------ 5: K.causal_curve / causal_auc
def test_causal_curve_against_fp64():
    from scouter_amd import kernels as K
    n_points, n_classes = 3, 6
    cols = torch.tensor([5, 0, 2, 2], dtype=torch.int32)
    Kc = cols.numel()
    total = 2 * Kc * n_points
    gen = torch.Generator().manual_seed(7400)
    for first, n in [(0, total), (5, 13), (total - 1, 1)]:
        logp = F.log_softmax(3.0 * torch.randn((n, n_classes), generator=gen), dim=1)
        curves = torch.full((Kc, 2, n_points), SENTINEL, device="cuda")
        got = K.causal_curve(logp.cuda(), cols.cuda(), curves, first, n_points)
        torch.cuda.synchronize()
        assert got.data_ptr() == curves.data_ptr()
        flat = curves.cpu().view(-1)
        g = torch.arange(first, first + n)
        ref = logp.double()[torch.arange(n), cols.long()[g // (2 * n_points)]].exp()
        err = (flat[first:first + n].double() - ref).abs()
        print("causal_curve", (first, n), "max err / p %.3e" % float((err / ref).max()))
        assert bool((err <= 4 * EPS * ref).all())
        assert bool((flat[:first] == SENTINEL).all()) and bool((flat[first + n:] == SENTINEL).all())


def trapezoid_fp64(curves):
    c = curves.double()
    return (c[..., 0] / 2 + c[..., 1:-1].sum(dim=-1) + c[..., -1] / 2) / (c.shape[-1] - 1)


@pytest.mark.parametrize("R", [1, 7])
@pytest.mark.parametrize("n_points", [2, 3, 226])
def test_causal_auc_against_fp64(n_points, R):
    from scouter_amd import kernels as K
    curves = torch.rand((R, n_points), generator=torch.Generator().manual_seed(7500 + n_points + R))
    if R > 1:
        curves[R - 1] = 0.0                                                   # a curve of zeros scores exactly 0
    out = torch.full((R + 1,), SENTINEL, device="cuda")
    got = K.causal_auc(curves.cuda(), out=out[:R])
    again = K.causal_auc(curves.cuda())
    torch.cuda.synchronize()
    assert float(out[R]) == SENTINEL and torch.equal(again, out[:R]) and got.dtype == torch.float32
    ref = trapezoid_fp64(curves)
    err = (got.cpu().double() - ref).abs()
    bound = (n_points + 8) * EPS * ref
    print("causal_auc", (R, n_points), "max err %.3e" % float(err.max()))
    assert bool((err <= bound).all()) and bool((ref > 0).any())
    if R > 1:
        assert float(ref[R - 1]) == 0.0 and float(got[R - 1]) == 0.0
    zeros = torch.zeros((R, n_points))
    assert float(trapezoid_fp64(zeros).abs().max()) == 0.0 and not bool(K.causal_auc(zeros.cuda()).any())
    lead = K.causal_auc(curves.cuda().view(1, R, n_points))                  # leading dimensions are kept
    assert tuple(lead.shape) == (1, R) and torch.equal(lead[0], again)


# ------------------------------------------------------------------------------------------------ 6: refusals
REFUSALS = ["resize_null", "resize_count", "ranks_null", "ranks_count", "ranks_too_long", "filter_null", "filter_count",
            "filter_even", "filter_33", "step_null", "step_count", "step_points", "step_step", "step_outside", "curve_null",
            "curve_count", "curve_points", "auc_null", "auc_count", "auc_points"]


@pytest.mark.parametrize("bad", REFUSALS)
def test_causal_kernels_refuse_bad_arguments(bad):
    """a null pointer, a count below 1, klen even or 33, a map above 2^20 elements (sizes only), n_points < 2, a chunk outside the
    stream: an error naming the call, every output untouched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    lib = _native.lib()
    C, H, W, Kc, step = 2, 8, 12, 2, 12
    HW, n_points = H * W, 9
    f = lambda *shape: torch.full(shape, SENTINEL, device="cuda")              # noqa: E731
    x, blurred, out_f = torch.ones((C, H, W), device="cuda"), torch.ones((C, H, W), device="cuda"), f(C, H, W)
    maps, ranks_out = torch.ones((Kc, HW), device="cuda"), torch.full((Kc, HW), -7, dtype=torch.int32, device="cuda")
    ranks = perm_ranks(Kc, HW, 1).cuda()
    taps3, taps4, taps33 = (torch.ones(k, device="cuda") / k for k in (3, 4, 33))
    ws, tmp = torch.empty(16 * Kc * HW, dtype=torch.uint8, device="cuda"), torch.empty((C, H, W), device="cuda")
    small, big = torch.ones((Kc, 3, 3), device="cuda"), f(Kc, H, W)
    imgs = f(4, C, H, W)
    logp, cols = torch.zeros((4, 6), device="cuda"), torch.zeros(Kc, dtype=torch.int32, device="cuda")
    curves, scores = f(Kc, 2, n_points), f(2 * Kc)
    p = lambda t: t.data_ptr()                                                 # noqa: E731
    calls = {
        "resize_null": lambda: lib.scouter_resize_bilinear_f32(None, p(big), Kc, 3, 3, H, W, None),
        "resize_count": lambda: lib.scouter_resize_bilinear_f32(p(small), p(big), Kc, 3, 3, 0, W, None),
        "ranks_null": lambda: lib.scouter_saliency_ranks_i32(p(maps), None, Kc, HW, p(ws), ws.numel(), None),
        "ranks_count": lambda: lib.scouter_saliency_ranks_i32(p(maps), p(ranks_out), 0, HW, p(ws), ws.numel(), None),
        "ranks_too_long": lambda: lib.scouter_saliency_ranks_i32(p(maps), p(ranks_out), 1, (1 << 20) + 1, p(ws), 1 << 40, None),
        "filter_null": lambda: lib.scouter_separable_filter_f32(p(x), None, p(tmp), p(out_f), C, H, W, 3, None),
        "filter_count": lambda: lib.scouter_separable_filter_f32(p(x), p(taps3), p(tmp), p(out_f), 0, H, W, 3, None),
        "filter_even": lambda: K.separable_filter(x, taps4, out=out_f),
        "filter_33": lambda: K.separable_filter(x, taps33, out=out_f),
        "step_null": lambda: lib.scouter_causal_step_images_f32(p(x), None, p(ranks), p(imgs), 0, 4, Kc, n_points, step, C, H, W,
                                                                None),
        "step_count": lambda: lib.scouter_causal_step_images_f32(p(x), p(blurred), p(ranks), p(imgs), 0, 0, Kc, n_points, step,
                                                                 C, H, W, None),
        "step_points": lambda: lib.scouter_causal_step_images_f32(p(x), p(blurred), p(ranks), p(imgs), 0, 4, Kc, 1, HW + 7, C, H, W,
                                                                  None),
        "step_step": lambda: K.causal_step_images(x, blurred, ranks, imgs, 0, n_points, 0),
        "step_outside": lambda: K.causal_step_images(x, blurred, ranks, imgs, 2 * Kc * n_points - 3, n_points, step),
        "curve_null": lambda: lib.scouter_causal_curve_f32(p(logp), None, p(curves), 0, 4, Kc, n_points, 6, None),
        "curve_count": lambda: lib.scouter_causal_curve_f32(p(logp), p(cols), p(curves), 0, 0, Kc, n_points, 6, None),
        "curve_points": lambda: lib.scouter_causal_curve_f32(p(logp), p(cols), p(curves), 0, 4, Kc, 1, 6, None),
        "auc_null": lambda: lib.scouter_causal_auc_f32(p(curves), None, 2 * Kc, n_points, None),
        "auc_count": lambda: lib.scouter_causal_auc_f32(p(curves), p(scores), 0, n_points, None),
        "auc_points": lambda: lib.scouter_causal_auc_f32(p(curves), p(scores), 2 * Kc * n_points, 1, None),
    }
    name = {"resize": "resize_bilinear", "ranks": "saliency_ranks", "filter": "separable_filter", "step": "causal_step_images",
            "curve": "causal_curve", "auc": "causal_auc"}[bad.split("_")[0]]
    with pytest.raises(RuntimeError, match=name):
        rc = calls[bad]()
        if isinstance(rc, int):
            _native.check(rc, name)
    torch.cuda.synchronize()
    for t in (out_f, big, imgs, curves, scores):
        assert bool((t == SENTINEL).all())
    assert bool((ranks_out == -7).all())
    # a valid call afterwards is right
    v = torch.randn((Kc, HW), generator=torch.Generator().manual_seed(3))
    assert torch.equal(K.saliency_ranks(v.cuda()).cpu().long(), ranks_cpu(v))


# ------------------------------------------------------------------------------------------------ 7: closed-form curves
class MeanStub(torch.nn.Module):
    """two outputs, log [m, 1 - m] with m the mean of channel 0 clamped into [1e-6, 1 - 1e-6]"""

    def forward(self, x):
        m = x[:, 0].mean(dim=(1, 2)).clamp(1e-6, 1 - 1e-6)
        return torch.log(torch.stack([m, 1 - m], dim=1))


def test_causal_metrics_closed_form():
    from scouter_amd.tools.attribution import causal_metrics
    stub = MeanStub().cuda()
    ramp = torch.arange(256, dtype=torch.float32).view(1, 1, 16, 16).cuda()
    ones = torch.ones((1, 1, 16, 16), device="cuda")
    j = torch.arange(17, dtype=torch.float64)
    kw = dict(classes=[0], step=16, klen=1, batch=5)
    down = causal_metrics(stub, ones, -ramp, **kw)                          # the most salient pixel first in raster order
    up = causal_metrics(stub, ones, ramp, **kw)
    torch.cuda.synchronize()
    assert down.step == 16 and tuple(down.deletion.shape) == (1, 1) and tuple(down.deletion_curve.shape) == (1, 1, 17)
    for r in (down, up):                                                    # whole rows go, from the top or from the bottom
        assert float((r.deletion_curve[0, 0].cpu().double() - (1 - j / 16).clamp(1e-6, 1 - 1e-6)).abs().max()) <= 1e-5
        assert abs(float(r.deletion[0, 0]) - 0.5) <= 1e-5
        assert float((r.insertion_curve[0, 0].cpu().double() - 1.0).abs().max()) <= 1e-5      # klen 1: the blur is the image
        assert abs(float(r.insertion[0, 0]) - 1.0) <= 1e-5
    assert torch.equal(down.deletion_curve, up.deletion_curve) and torch.equal(down.deletion, up.deletion)
    half = ones.clone()
    half[:, :, 8:] = 0.0
    good = causal_metrics(stub, half, -ramp, **kw)                           # deletes the rows that carry the evidence first
    poor = causal_metrics(stub, half, ramp, **kw)
    assert float(good.deletion[0, 0]) < float(poor.deletion[0, 0])
    assert abs(float(good.deletion[0, 0]) - 0.125) <= 1e-5 and abs(float(poor.deletion[0, 0]) - 0.375) <= 1e-5
    want = torch.cat([(8 - j[:9]) / 16, torch.zeros(8, dtype=torch.float64)]).clamp(1e-6, 1 - 1e-6)
    assert float((good.deletion_curve[0, 0].cpu().double() - want).abs().max()) <= 1e-5
    # class 1 is the complement, and the default step is one row (W)
    other = causal_metrics(stub, half, -ramp, classes=[1], klen=1, batch=5)
    assert other.step == 16 and abs(float(other.deletion[0, 0]) - 0.875) <= 1e-5


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


def expected_scores(m, images, maps, cols, step, batch, taps):
    """(curves fp64 [B, K, 2, n_points], scores fp64 [B, K, 2]): the whole edit stream built on the CPU from CPU ranks and
    torch.where (the insertion side from the GPU's own blurred image, so the stream is bit-identical), pushed through the model in
    the same chunks under eval() and no_grad(), the curves and trapezoids formed in float64"""
    from scouter_amd import kernels as K
    B, C, H, W = images.shape
    Kc = maps.shape[1]
    n_points = -(-(H * W) // step) + 1
    total = 2 * Kc * n_points
    was_training = m.training
    m.eval()
    curves = []
    try:
        with torch.no_grad():
            for b in range(B):
                blurred = K.separable_filter(images[b], taps.cuda()).cpu()
                ref_blur, mag = filter_fp64(images[b].cpu(), taps), filter_fp64(images[b].cpu().abs(), taps)
                assert bool(((blurred.double() - ref_blur).abs() <= (2 * taps.numel() + 4) * EPS * mag).all())
                ranks = ranks_cpu(maps[b].cpu().float().view(Kc, H * W))
                stream = stream_cpu(images[b].cpu(), blurred, ranks, n_points, step, 0, total)
                logp = torch.cat([m(stream[f:f + batch].cuda()).cpu().double() for f in range(0, total, batch)])
                col = torch.tensor(cols).repeat_interleave(2 * n_points)
                curves.append(logp[torch.arange(total), col].exp().view(Kc, 2, n_points))
    finally:
        m.train(was_training)
    curves = torch.stack(curves)
    return curves, trapezoid_fp64(curves)


def check_scores(r, curves, scores, n_points, what):
    got_c = torch.stack([r.deletion_curve, r.insertion_curve], dim=2).cpu().double()
    got_s = torch.stack([r.deletion, r.insertion], dim=2).cpu().double()
    ec, es = (got_c - curves).abs(), (got_s - scores).abs()
    print("%s: curves max err / p %.3e, scores max err / ref %.3e" % (what, float((ec / curves).max()), float((es / scores).max())))
    assert bool((ec <= 4 * EPS * curves).all()) and bool((es <= (n_points + 8) * EPS * scores).all())


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_causal_metrics_on_whole_models(use_slot):
    from scouter_amd.tools.attribution import causal_metrics, gaussian_taps
    m, images = build(use_slot)
    maps = torch.rand((2, 2, 64, 64), generator=torch.Generator().manual_seed(21)).cuda()
    cols, step, batch, n_points = [0, 3], 256, 16, 17
    kw = dict(step=step, batch=batch)
    m.train()
    curves, scores = expected_scores(m, images, maps, cols, step, batch, gaussian_taps(11, 5.0))
    before = bn_buffers(m)
    r = causal_metrics(m, images, maps, classes=cols, **kw)
    torch.cuda.synchronize()
    # ---- the values, the shapes, the state left behind
    for t, shape in ((r.deletion, (2, 2)), (r.insertion, (2, 2)), (r.deletion_curve, (2, 2, 17)), (r.insertion_curve, (2, 2, 17))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_cuda and bool(torch.isfinite(t).all())
    assert r.step == step and isinstance(r.step, int)
    check_scores(r, curves, scores, n_points, "causal_metrics %s" % ("slot" if use_slot else "fc"))
    assert float(r.deletion.min()) >= 0 and float(r.insertion.max()) <= 1
    assert m.training
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in m.parameters())
    m.eval()
    with torch.no_grad():
        plain = m(images)[:, cols].exp()                                    # [B, K]: the untouched images
    m.train()
    assert bool(((r.deletion_curve[:, :, 0] - plain).abs() <= 1e-3 * plain).all())
    assert bool(((r.insertion_curve[:, :, -1] - plain).abs() <= 1e-3 * plain).all())
    # ---- reproducibility, uint8 maps, class selection
    again = causal_metrics(m, images, maps, classes=cols, **kw)
    assert all(torch.equal(a, b) for a, b in zip(r[:4], again[:4]))
    levels = (maps * 255).to(torch.uint8)
    assert all(torch.equal(a, b) for a, b in zip(causal_metrics(m, images, levels, classes=cols, **kw)[:4],
                                                 causal_metrics(m, images, levels.float(), classes=cols, **kw)[:4]))
    own = causal_metrics(m, images, torch.stack([maps[0, :1], maps[1, 1:]]), classes=torch.tensor([0, 3]), **kw)
    assert tuple(own.deletion.shape) == (2, 1) and tuple(own.insertion_curve.shape) == (2, 1, 17)
    # image 0, map 0: the first 32 stream images sit in the same chunks as in the list run -- the same bits there
    assert torch.equal(own.deletion_curve[0, 0], r.deletion_curve[0, 0]) and torch.equal(own.deletion[0, 0], r.deletion[0, 0])
    assert torch.equal(own.insertion_curve[0, 0, :15], r.insertion_curve[0, 0, :15])
    for a, b in ((own.insertion_curve[0, 0], r.insertion_curve[0, 0]), (own.deletion_curve[1, 0], r.deletion_curve[1, 1]),
                 (own.insertion_curve[1, 0], r.insertion_curve[1, 1]), (own.deletion[1, 0], r.deletion[1, 1]),
                 (own.insertion[:, 0], torch.stack([r.insertion[0, 0], r.insertion[1, 1]]))):
        assert bool(((a - b).abs() <= 1e-3 * b.abs()).all())
    for bad in ([10, 0], [-1, 0]):
        with pytest.raises(IndexError):
            causal_metrics(m, images, maps, classes=bad, **kw)
    with pytest.raises(IndexError):
        causal_metrics(m, images, maps[:, :1], classes=torch.tensor([0, 10]), **kw)
    for bad_kw in (dict(classes=torch.tensor([0, 1, 2])), dict(classes=torch.tensor([0, 1])), dict(classes=None),
                   dict(classes=[0]), dict(classes=cols, batch=0), dict(classes=cols, step=0), dict(classes=cols, klen=4),
                   dict(classes=cols, klen=33), dict(classes=cols, sigma=0.0)):
        with pytest.raises(ValueError):
            causal_metrics(m, images, maps, **{**kw, **bad_kw})
    for bad_maps in (maps.double(), maps[:1], maps[0]):
        with pytest.raises(ValueError):
            causal_metrics(m, images, bad_maps, classes=cols, **kw)
    assert m.training and all(p.grad is None for p in m.parameters())
    # ---- coarse maps are resized first: the scores of the resized maps, bit for bit
    from scouter_amd import kernels as K
    coarse = torch.rand((2, 2, 7, 7), generator=torch.Generator().manual_seed(22)).cuda()
    assert all(torch.equal(a, b) for a, b in zip(causal_metrics(m, images, coarse, classes=cols, **kw)[:4],
                                                 causal_metrics(m, images, K.resize_bilinear(coarse, 64, 64), classes=cols,
                                                                **kw)[:4]))
    # ---- BatchNorm-folded forwards: the fold's own forward tolerance
    m.set_inference_fold(True)
    folded = causal_metrics(m, images, maps, classes=cols, **kw)
    m.set_inference_fold(False)
    got, ref = torch.stack([folded.deletion, folded.insertion]), torch.stack([r.deletion, r.insertion])
    diff, top = float((got - ref).abs().max()), float(ref.abs().max())
    print("causal_metrics folded against unfolded: max difference %.3e, max score %.3e, ratio %.3e" % (diff, top, diff / top))
    assert diff <= 1e-3 * top
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 9: slot_saliency and the CLI
def test_slot_saliency():
    from scouter_amd.tools.attribution import slot_saliency
    m, images = build(True)
    with pytest.raises(RuntimeError):
        slot_saliency(m)                                                    # no forward has run yet
    m.eval()
    with torch.no_grad():
        m(images)
    s = slot_saliency(m)
    attn = m.slot.last_attn
    B, S, N = attn.shape
    side = int(N ** 0.5)
    assert tuple(s.shape) == (2, 10, side, side) and s.dtype == torch.float32 and s.is_cuda
    assert torch.equal(s, attn.reshape(B, 10, S // 10, N).sum(2).view(B, 10, side, side))
    vis = m.slot.vis_maps()                                                 # uint8 [10, side, side] of image 0, monotone in s
    for c in range(10):
        assert int(vis[c].reshape(-1)[int(s[0, c].argmax())]) == int(vis[c].max())
    fc, _ = build(False)
    fc.eval()
    with torch.no_grad():
        fc(images)
    with pytest.raises(RuntimeError):
        slot_saliency(fc)


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_causal_test_tool(use_slot, tmp_path, monkeypatch, capsys):
    """test.py --causal true: one `causal <family> class <c>: deletion <d> insertion <i>` line per family drawn in the call"""
    from scouter_amd import test as T
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "true" if use_slot else "false", "--pre_trained", "false",
        "--img_size", "64", "--causal", "true", "--cam", "true", "--rise", "true", "--rise_masks", "32", "--rise_batch", "16",
        "--causal_step", "256", "--vis_dir", str(tmp_path / "vis"), "--output_dir", str(tmp_path / "none")])
    T.main()
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("causal ")]
    assert [ln[1] for ln in lines] == (["slot"] if use_slot else []) + ["cam", "rise"]
    classes = set()
    for ln in lines:
        assert ln[2] == "class" and ln[3].endswith(":") and ln[4] == "deletion" and ln[6] == "insertion" and len(ln) == 8
        classes.add(int(ln[3][:-1]))
        for v in (float(ln[5]), float(ln[7])):
            assert np.isfinite(v) and 0.0 <= v <= 1.0
    assert len(classes) == 1 and 0 <= classes.pop() < 10                    # every family scores the predicted class
