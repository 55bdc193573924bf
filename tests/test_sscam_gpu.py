"""SS-CAM and IS-CAM (-m gpu): the sscam_* kernels of csrc/scorecam.hip against fp64 -- kernels.sscam_mask_images against
channels resized with F.interpolate in float64 plus the noise kernels.noise_images writes (no reference program is involved),
kernels.sscam_weights against the float64 exp, kernels.sscam_contract against the float64 einsum -- their refusals,
tools/attribution.py sscam / iscam on whole models against the fp64 sum over the HIP path's own features, masked images and
log-probabilities, and sscam_maps / iscam_maps / test.py run_sscam / run_iscam / run_causal / run_infidelity.

Inputs are those of test_scorecam_gpu.py (make_features: live channels whose span is their magnitude, one constant and one
all-zero dead channel per case, the input condition M_c / span_c <= 4 asserted on the fp64 reference).

Bounds (EPS = 2^-24).  A masked image element is image * g, g = a + nz, a = scale * m, nz = sigma * z, four fp32 roundings after
the mask value m: the product a (<= EPS scale, m <= 1), the product nz (<= EPS |sigma z|), the sum (<= EPS (scale + |sigma z|))
and the product with the image (<= EPS (scale + |sigma z|) |image|) -- 3 EPS (scale + |sigma z|) |image| in all, which the test
bounds by 4 EPS (scale + |sigma z|) |image|; the mask value itself lies within 4 e_U(c) / span_c + 8 EPS of the float64 one
(test_scorecam_gpu.py), times scale.  z is taken from kernels.noise_images(zeros, sigma = 1), which is exactly z and is tested
against its own definition in test_pathgrad_gpu.py.  A weight term is expf of an fp32 log-probability, accurate to 2 EPS
relative, bounded by 4 EPS; the float64 sum adds nothing visible.  The contraction adds one fma per channel and one rounding of
the weight to fp32: (C + 8) EPS sum_c |w_c A[p, c]|, and exactly nothing where every term is 0."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_scorecam_gpu import (EPS, SENTINEL, bn_buffers, build, check_accumulated, make_features, model_args,   # noqa: E402
                               reference_fp64)

SEED = 0x5EED0123456789


def noise_field(shape, seed, j):
    """z(seed, sample j) for one image's shape, float64 on the host: kernels.noise_images of a zero image at sigma = 1"""
    from scouter_amd import kernels as K
    out = torch.empty((1,) + tuple(shape), device="cuda")
    K.noise_images(torch.zeros(tuple(shape), device="cuda"), out, 1.0, seed, j)
    return out[0].cpu().double()


def ramp_scale(j, n_samples, ramp):
    from scouter_amd.tools.attribution import iscam_ramp
    return float(iscam_ramp(n_samples)[j]) if ramp else 1.0


# (Cin, H, W, h, w, C, first_row, n, n_samples, ramp, sigma)
CASES = [(1, 5, 7, 2, 3, 5, 3, 5, 3, 0, 0.5),             # the one-pixel form, rows straddle a sample boundary, C not a multiple of 4
         (3, 64, 64, 2, 2, 512, 1012, 24, 3, 0, 2.0),     # the boundary between samples 1 and 2 on the vector form
         (3, 224, 224, 7, 7, 64, 77, 6, 2, 0, 2.0),       # real geometry, mid-stream
         (3, 33, 47, 9, 9, 20, 0, 20, 4, 1, 0.0),         # the ramp, non-integer ratios
         (2, 8, 8, 1, 1, 4, 0, 4, 2, 0, 1.0)]             # one source pixel: every channel is dead, every image zero despite the noise
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(image, A, the float64 reference, the dead channels) of a case: computed once, shared by the tests, never changed"""
    Cin, H, W, h, w, C, first_row, n = case[:8]
    image = torch.randn((Cin, H, W), generator=torch.Generator().manual_seed(8000))
    dead = ((first_row + 1) % C, (first_row + n - 1) % C)
    A = make_features(h, w, C, dead, 8100)
    return image, A, reference_fp64(A, H, W), dead


def _check_mask_images(case):
    from scouter_amd import kernels as K
    Cin, H, W, h, w, C, first_row, n, N, ramp, sigma = case
    image, A, (_, lo64, hi64, live64, mask64, M, e_U), dead = case_data(case)
    assert not bool(live64[list(dead)].any()) and int(live64.sum()) == (C - 2 if h * w > 1 else 0)
    Ad = A.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    rows = torch.arange(first_row, first_row + n)
    js, cs = rows // C, rows % C
    z = {j: noise_field((Cin, H, W), SEED, j) for j in sorted(set(js.tolist()))}
    span = torch.where(live64, hi64 - lo64, torch.ones_like(lo64))
    img = image.double()
    ref = torch.zeros((n, Cin, H, W), dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for i in range(n):
        j, c = int(js[i]), int(cs[i])
        if not bool(live64[c]):
            continue
        s = ramp_scale(j, N, ramp)
        nz = sigma * z[j]
        ref[i] = img * (s * mask64[c][None] + nz)
        bound[i] = img.abs() * (s * (4 * float(e_U[c]) / float(span[c]) + 8 * EPS) + 4 * EPS * (s + nz.abs()))
    out = torch.full((n + 1, Cin, H, W), SENTINEL, device="cuda")
    got = K.sscam_mask_images(image.cuda(), Ad, ranges, out[:n], first_row, N, sigma, SEED, bool(ramp))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[n] == SENTINEL).all())            # the row after keeps the sentinel
    res = out[:n].cpu().double()
    err = (res - ref).abs()
    print("sscam_mask_images", case, "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    lv = live64[cs]
    assert bool((res[~lv] == 0).all())                                                      # dead rows: exactly zero
    if h * w == 1:
        assert bool((res == 0).all())
    # ---- a chunk written as two calls split at any row equals one call; so does a second call
    whole = out[:n].clone()
    for cut in range(1, n):
        two = torch.full((n, Cin, H, W), SENTINEL, device="cuda")
        K.sscam_mask_images(image.cuda(), Ad, ranges, two[:cut], first_row, N, sigma, SEED, bool(ramp))
        K.sscam_mask_images(image.cuda(), Ad, ranges, two[cut:], first_row + cut, N, sigma, SEED, bool(ramp))
        assert torch.equal(two, whole), cut
        if H * W > 4096 and cut >= 2:
            break                                                                          # (real geometry: two cuts are enough)
    return whole


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sscam_mask_images_against_fp64(case):
    _check_mask_images(case)


@pytest.mark.parametrize("W", [16, 15], ids=["vector", "one_pixel"])
def test_sscam_noise_is_shared_by_channels_and_differs_by_sample_and_plane(W):
    """two identical feature channels give bit-identical rows within a sample and different rows across samples; with an all-ones
    image and Cin = 3 the three planes differ: the noise belongs to the image element, not to the pixel or the channel"""
    from scouter_amd import kernels as K
    Cin, H, h, w, C, N = 3, 12, 3, 3, 6, 2
    A = make_features(h, w, C, (4, 5), 8200)
    A[:, :, 3] = A[:, :, 2]
    Ad = A.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    assert torch.equal(ranges[2], ranges[3]) and float(ranges[2, 1] - ranges[2, 0]) > 0
    ones = torch.ones((Cin, H, W), device="cuda")
    out = torch.empty((N, C, Cin, H, W), device="cuda")
    for j in range(N):
        K.sscam_mask_images(ones, Ad, ranges, out[j], j * C, N, 0.75, SEED)
    torch.cuda.synchronize()
    assert torch.equal(out[0, 2], out[0, 3]) and torch.equal(out[1, 2], out[1, 3])
    assert not torch.equal(out[0, 2], out[1, 2])
    assert not torch.equal(out[0, 2, 0], out[0, 2, 1]) and not torch.equal(out[0, 2, 1], out[0, 2, 2])
    # the difference of two live rows of a sample is the difference of their masks: the noise cancels up to the sum's rounding
    clean = K.sscam_mask_images(ones, Ad, ranges, torch.empty((C, Cin, H, W), device="cuda"), 0, N)
    d = ((out[0, 0] - out[0, 1]) - (clean[0] - clean[1])).abs().max()
    assert float(d) <= 16 * EPS * float(out[0].abs().max())
    assert bool((out[:, 4:] == 0).all())                                                    # dead rows: zero under noise


@pytest.mark.parametrize("what", ["out", "image"])
def test_sscam_mask_images_one_pixel_form_on_a_4_byte_aligned_view(what):
    """an `out` or `image` view that is only 4-byte aligned takes the one-pixel form and gives the bits of the aligned call"""
    from scouter_amd import kernels as K
    Cin, H, W, h, w, C, N, n = 3, 16, 16, 3, 2, 8, 2, 8
    image = torch.randn((Cin, H, W), generator=torch.Generator().manual_seed(8300)).cuda()
    Ad = make_features(h, w, C, (1, 6), 8301).cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    for sigma, ramp in ((1.5, False), (0.0, True)):
        want = K.sscam_mask_images(image, Ad, ranges, torch.empty((n, Cin, H, W), device="cuda"), 5, N, sigma, SEED, ramp)
        assert want.data_ptr() % 16 == 0 and image.data_ptr() % 16 == 0
        if what == "out":
            store = torch.full((n * Cin * H * W + 2,), SENTINEL, device="cuda")
            view = store[1:-1].view(n, Cin, H, W)
            assert view.data_ptr() % 16 == 4
            got = K.sscam_mask_images(image, Ad, ranges, view, 5, N, sigma, SEED, ramp)
            assert float(store[0]) == SENTINEL and float(store[-1]) == SENTINEL
        else:
            store = torch.zeros((Cin * H * W + 1,), device="cuda")
            store[1:] = image.flatten()
            view = store[1:].view(Cin, H, W)
            assert view.data_ptr() % 16 == 4
            got = K.sscam_mask_images(view, Ad, ranges, torch.empty((n, Cin, H, W), device="cuda"), 5, N, sigma, SEED, ramp)
        assert torch.equal(got, want), (sigma, ramp)


# ------------------------------------------------------------------------------------------------ 2: K.sscam_weights
# (n, n_classes, K, C, the columns or None for 0 .. K - 1)
W_CASES = [(5, 10, 10, 5, None), (12, 200, 3, 512, [150, 7, 150]), (37, 12, 5, 37, [11, 0, 3, 3, 7])]


@pytest.mark.parametrize("case", W_CASES, ids=lambda c: "%drows_%dof%d_c%d" % (c[0], c[2], c[1], c[3]))
def test_sscam_weights_against_fp64(case):
    from scouter_amd import kernels as K
    n, n_classes, Kc, C, cols = case
    cols = torch.tensor(cols if cols is not None else list(range(Kc)), dtype=torch.int32)
    gen = torch.Generator().manual_seed(8400 + C)
    first = C - 2                                                                          # the first chunk wraps a sample boundary
    logp = F.log_softmax(torch.randn((3 * n, n_classes), generator=gen), dim=1)            # three consecutive chunks of the stream
    terms = logp.double().exp()[:, cols.long()]                                            # [3 n, K]
    chan = (first + torch.arange(3 * n)) % C
    ref = torch.zeros((C, Kc), dtype=torch.float64).index_add_(0, chan, terms)
    ld, cd = logp.cuda(), cols.cuda()

    def run(cuts):
        wsum = torch.zeros((C, Kc), dtype=torch.float64, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert K.sscam_weights(ld[a:b], cd, wsum, first + a) is wsum
        return wsum

    one = run([0, n])
    three = run([0, n, 2 * n, 3 * n])
    torch.cuda.synchronize()
    # ---- one chunk: every touched (channel, class) holds its one term, the rest stays 0
    ref1 = torch.zeros((C, Kc), dtype=torch.float64).index_add_(0, chan[:n], terms[:n])
    err1 = (one.cpu() - ref1).abs()
    assert bool((err1 <= 4 * EPS * ref1).all()) and bool((one.cpu()[ref1 == 0] == 0).all())
    assert bool((one.cpu()[chan[:2]] > 0).all()) and bool((one.cpu()[chan[2:n]] > 0).all())  # both sides of the boundary
    # ---- several chunks onto the same sums
    err = (three.cpu() - ref).abs()
    print("sscam_weights", case[:4], "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / (4 * EPS * ref).clamp_min(1e-300)).max())))
    assert bool((err <= 4 * EPS * ref).all())
    assert bool((three.cpu()[ref == 0] == 0).all())
    # ---- a split at any row, and a second run: the same bits
    assert torch.equal(run([0, n, 2 * n, 3 * n]), three)
    for cut in range(1, n):
        assert torch.equal(run([0, cut, n]), one), cut
    assert torch.equal(run(list(range(0, 3 * n, n - 1)) + [3 * n]), three)                 # another chunking of the same stream


# ------------------------------------------------------------------------------------------------ 3: K.sscam_contract
# (K, h, w, C, signed features)
C_CASES = [(10, 7, 7, 64, False), (3, 2, 2, 512, False), (200, 9, 9, 20, False), (1, 1, 1, 4, False), (5, 3, 5, 37, True)]


@pytest.mark.parametrize("case", C_CASES, ids=lambda c: "%d_%dx%d_c%d%s" % (c[:4] + ("_signed" if c[4] else "",)))
def test_sscam_contract_against_fp64(case):
    from scouter_amd import kernels as K
    Kc, h, w, C, signed = case
    H, W = 2 * h + 1, 2 * w + 3
    gen = torch.Generator().manual_seed(8500 + C)
    A = make_features(h, w, C, (1, C - 1), 8600 + C, signed=signed)
    _, _, _, live64, _, _, _ = reference_fp64(A, H, W)
    assert int(live64.sum()) == (C - 2 if h * w > 1 else 0)
    wsum = torch.rand((C, Kc), generator=gen, dtype=torch.float64) * 3.0
    Ad, wd = A.cuda(), wsum.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    assert torch.equal((ranges[:, 1] - ranges[:, 0] > 0).cpu(), live64)
    zero = torch.zeros((Kc, h, w), dtype=torch.float64)
    for norm in (1.0, 1.0 / 3.0):
        wts = wsum * norm * live64[:, None].double()
        ref = torch.einsum("ck,hwc->khw", wts, A.double())
        absref = torch.einsum("ck,hwc->khw", wts, A.double().abs())
        out = torch.full((Kc, h, w), SENTINEL, device="cuda")
        got = K.sscam_contract(wd, Ad, ranges, out, norm)
        again = K.sscam_contract(wd, Ad, ranges, torch.zeros((Kc, h, w), device="cuda"), norm)
        torch.cuda.synchronize()
        assert got is out
        check_accumulated(got, ref, absref, zero, C, "sscam_contract %s norm %.3f" % (case[:4], norm))
        assert torch.equal(got, again)                       # out is overwritten: the sentinel start and the zero start agree
        huge = wd.clone()
        huge[(~live64).nonzero().flatten().cuda()] = 1.0e300                                # dead channels change nothing
        assert torch.equal(K.sscam_contract(huge, Ad, ranges, torch.empty((Kc, h, w), device="cuda"), norm), got)


@pytest.mark.parametrize("case", [(10, 10, 7, 7, 64, None), (3, 200, 2, 2, 512, [150, 7, 150]), (5, 12, 3, 5, 37, [11, 0, 3, 3, 7])],
                         ids=lambda c: "%dof%d_%dx%d_c%d" % c[:5])
def test_sscam_weights_and_contract_after_three_samples_against_fp64(case):
    """three samples through sscam_weights, one call each, and norm = 1 / 3 (one sample and norm = 1: test_scorecam_gpu.py)"""
    from scouter_amd import kernels as K
    Kc, n_classes, h, w, C, cols = case
    H, W = 2 * h + 1, 2 * w + 3
    cols = torch.tensor(cols if cols is not None else list(range(Kc)), dtype=torch.int32)
    gen = torch.Generator().manual_seed(8700 + C)
    logp = F.log_softmax(torch.randn((3 * C, n_classes), generator=gen), dim=1)
    A = make_features(h, w, C, (1, C - 1), 8800 + C)
    _, _, _, live64, _, _, _ = reference_fp64(A, H, W)
    ld, cd, Ad = logp.cuda(), cols.cuda(), A.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    wsum = torch.zeros((C, Kc), dtype=torch.float64, device="cuda")
    K.sscam_weights(ld[:C], cd, wsum, 0)
    K.sscam_weights(ld[C:2 * C], cd, wsum, C)
    K.sscam_weights(ld[2 * C:], cd, wsum, 2 * C)
    mean = K.sscam_contract(wsum, Ad, ranges, torch.full((Kc, h, w), SENTINEL, device="cuda"), 1.0 / 3.0)
    wts = logp.double().exp()[:, cols.long()].view(3, C, Kc).sum(dim=0) / 3.0 * live64[:, None].double()
    ref = torch.einsum("ck,hwc->khw", wts, A.double())
    absref = torch.einsum("ck,hwc->khw", wts, A.double().abs())
    check_accumulated(mean, ref, absref, torch.zeros_like(ref), C, "sscam_contract after three samples %s" % (case[:5],))


# ------------------------------------------------------------------------------------------------ 4: refusals
BAD = {"sscam_mask_images": ["null", "first_low", "rows_high", "n_above_C", "n_samples0", "sigma_neg", "sigma_nan", "sigma_inf",
                             "ranges_shape", "hw_cap", "out_shape", "H0"],
       "sscam_weights": ["null", "first_low", "n_above_C", "K0", "wsum_dtype", "wsum_shape"],
       "sscam_contract": ["null", "ranges_shape", "hw_cap", "out_shape", "K0", "wsum_dtype", "wsum_shape"]}


@pytest.mark.parametrize("call,bad", [(c, b) for c in BAD for b in BAD[c]])
def test_sscam_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, first_row < 0, rows past n_samples C, n > C, n_samples = 0, sigma negative / NaN / infinite, ranges that are
    not [C, 2], h w above 1024, an output of the wrong shape, H = 0, K = 0, wsum that is not float64 [C, K]: an error naming the
    call, every output at its sentinel, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    Cin, H, W, h, w, C, n, Kc, N = 2, 20, 24, 3, 4, 6, 4, 3, 2
    if bad == "hw_cap":
        h, w = 33, 32                                                    # 1056 source positions: above the 1024 a channel may have
    image = torch.ones((Cin, H, W), device="cuda")
    feat = torch.rand((h, w, C), generator=torch.Generator().manual_seed(5)).cuda()
    good_ranges = torch.tensor([[0.0, 1.0]] * C, device="cuda")
    rg = good_ranges[:C - 1] if bad == "ranges_shape" else good_ranges
    rows = C + 1 if bad == "n_above_C" else n
    out = torch.full((rows, Cin, H, W), SENTINEL, device="cuda")
    maps = torch.full((Kc, h, w), SENTINEL, device="cuda")
    wsum = torch.full((C, Kc), SENTINEL, dtype=torch.float64, device="cuda")
    logp = torch.zeros((rows, 6), device="cuda")
    cols = torch.tensor([0, 5, 2], dtype=torch.int32, device="cuda")
    first = {"first_low": -1, "rows_high": N * C - n + 1}.get(bad, 1)
    sigma = {"sigma_neg": -1.0, "sigma_nan": float("nan"), "sigma_inf": float("inf")}.get(bad, 0.5)
    ws = {"wsum_dtype": wsum.float(), "wsum_shape": wsum[:, :Kc - 1].contiguous()}.get(bad, wsum)
    lib = _native.lib()
    with pytest.raises(RuntimeError, match=call):
        if call == "sscam_mask_images":
            if bad == "null":
                _native.check(lib.scouter_sscam_mask_images_f32(image.data_ptr(), None, good_ranges.data_ptr(), out.data_ptr(), first,
                                                                n, N, 0, 0.5, 1, 2, Cin, H, W, h, w, C, None), call)
            elif bad == "out_shape":
                K.sscam_mask_images(image, feat, rg, out.view(rows, Cin, W, H), first, N, sigma, SEED)
            elif bad == "H0":
                K.sscam_mask_images(image[:, :0], feat, rg, out[:, :, :0], first, N, sigma, SEED)
            else:
                K.sscam_mask_images(image, feat, rg, out, first, 0 if bad == "n_samples0" else N, sigma, SEED)
        elif call == "sscam_weights":
            if bad == "null":
                _native.check(lib.scouter_sscam_weights_f64(logp.data_ptr(), cols.data_ptr(), None, first, n, 6, Kc, C, None), call)
            elif bad == "K0":
                K.sscam_weights(logp, cols[:0], wsum[:, :0], first)
            else:
                K.sscam_weights(logp, cols, ws, first)
        else:
            if bad == "null":
                _native.check(lib.scouter_sscam_contract_f32(wsum.data_ptr(), feat.data_ptr(), None, maps.data_ptr(), 1.0, Kc, h, w,
                                                             C, None), call)
            elif bad == "K0":
                K.sscam_contract(wsum[:, :0], feat, rg, maps[:0])
            elif bad == "out_shape":
                K.sscam_contract(wsum, feat, rg, maps.view(Kc, w, h))
            else:
                K.sscam_contract(ws, feat, rg, maps)
    if bad == "K0":                                                      # K = 0 at the library too, with every pointer valid
        with pytest.raises(RuntimeError, match=call):
            if call == "sscam_weights":
                _native.check(lib.scouter_sscam_weights_f64(logp.data_ptr(), cols.data_ptr(), wsum.data_ptr(), first, n, 6, 0, C,
                                                            None), call)
            else:
                _native.check(lib.scouter_sscam_contract_f32(wsum.data_ptr(), feat.data_ptr(), good_ranges.data_ptr(),
                                                             maps.data_ptr(), 1.0, 0, h, w, C, None), call)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((maps == SENTINEL).all()) and bool((wsum == SENTINEL).all())
    _check_mask_images(CASES[0])


# ------------------------------------------------------------------------------------------------ 5: whole models
def expected_stream(m, images, n_samples, sigma, batch, seed, ramp, norm):
    """fp64 (ref, absref) [B, n, h, w]: the definition's sum over the HIP path's own data -- the features of feature_pass, the
    live flags of K.scorecam_ranges, the same chunks built with K.sscam_mask_images and the model in eval mode under no_grad at
    the same batch, the probabilities summed per (channel, class) and contracted in float64"""
    from scouter_amd import kernels as K
    B, Cin, H, W = images.shape
    feat = m.feature_pass(images).features.detach().float().contiguous()
    _, h, w, C = feat.shape
    rows, step = n_samples * C, min(batch, C)
    was_training = m.training
    m.eval()
    ref, absref = [], []
    try:
        with torch.no_grad():
            for b in range(B):
                ranges = K.scorecam_ranges(feat[b], H, W)
                live = (ranges[:, 1] - ranges[:, 0] > 0).cpu().double()
                wsum = None
                for first in range(0, rows, step):
                    n = min(step, rows - first)
                    chunk = K.sscam_mask_images(images[b], feat[b], ranges, torch.empty((n, Cin, H, W), device="cuda"), first,
                                                n_samples, sigma, seed, ramp)
                    p = m(chunk).cpu().double().exp()
                    if wsum is None:
                        wsum = torch.zeros((C, p.shape[1]), dtype=torch.float64)
                    wsum.index_add_(0, (first + torch.arange(n)) % C, p)
                wts = wsum * norm * live[:, None]
                A = feat[b].cpu().double()
                ref.append(torch.einsum("ck,hwc->khw", wts, A))
                absref.append(torch.einsum("ck,hwc->khw", wts, A.abs()))
    finally:
        m.train(was_training)
    return torch.stack(ref), torch.stack(absref), feat


def check_stream(got, ref, absref, C, what):
    """check_accumulated with one more EPS sum |w A| for the weights' rounding from float64 to fp32"""
    check_accumulated(got, ref, absref * (C + 9) / (C + 8), torch.zeros_like(ref), C, what)


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_sscam_and_iscam_on_whole_models(use_slot):
    """resnet18 / MNIST / 64^2 / batch 2: features [2, 2, 2, 512], three samples, batch = 100: 1536 rows = 15 x 100 + 36, so chunks
    straddle the sample boundaries and the stream ends in a short chunk.  Chunks of 512 against chunks of 100: the forwards run at
    other batch sizes; the eval forward of this model is asserted batch-invariant bit for bit at batches 36, 100 and 512 first, so
    the two runs are asserted to give equal bits."""
    from scouter_amd.tools.attribution import iscam, scorecam, sscam
    m, images = build(use_slot)
    batch, C, N, sigma = 100, 512, 3, 0.5
    name = "slot" if use_slot else "fc"
    m.train()
    before = bn_buffers(m)
    runs = {"sscam": (functools.partial(sscam, m, images, n_samples=N, sigma=sigma, seed=SEED), (N, sigma, batch, SEED, False, 1.0 / N)),
            "iscam": (functools.partial(iscam, m, images, n_samples=N), (N, 0.0, batch, 0, True, 1.0))}
    m.eval()
    with torch.no_grad():                                                                 # is the eval forward batch-invariant?
        x512 = torch.randn((512, 1, 64, 64), generator=torch.Generator().manual_seed(13)).cuda()
        l512 = m(x512)
        assert torch.equal(torch.cat([m(x512[i:i + 100]) for i in range(0, 512, 100)]), l512)
        assert torch.equal(m(x512[100:136]), l512[100:136])
    m.train()
    results = {}
    for method, (call, spec) in runs.items():
        ref, absref, feat = expected_stream(m, images, *spec)
        assert tuple(feat.shape) == (2, 2, 2, C)
        S = call(batch=batch)
        torch.cuda.synchronize()
        # ---- the value, the shape, the state left behind
        assert tuple(S.shape) == (2, 10, 2, 2) and S.dtype == torch.float32 and S.is_cuda
        assert bool(torch.isfinite(S).all()) and float(S.max()) > float(S.min())
        check_stream(S, ref, absref, C, "%s %s" % (method, name))
        assert m.training
        after = bn_buffers(m)
        assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
        assert all(p.grad is None for p in m.parameters())
        # ---- reproducibility, the chunking, class selection
        assert torch.equal(call(batch=batch), S)
        whole = call(batch=512)
        print("%s %s: chunks of 512 against chunks of 100: %s" %
              (method, name, "equal bits" if torch.equal(whole, S) else "max difference %.3e" % float((whole - S).abs().max())))
        assert torch.equal(whole, S)
        two = call(classes=[0, 3], batch=batch)
        assert tuple(two.shape) == (2, 2, 2, 2) and torch.equal(two[:, 0], S[:, 0]) and torch.equal(two[:, 1], S[:, 3])
        own = call(classes=torch.tensor([7, 2]), batch=batch)
        assert tuple(own.shape) == (2, 1, 2, 2) and torch.equal(own[0, 0], S[0, 7]) and torch.equal(own[1, 0], S[1, 2])
        results[method] = S
    # ---- the seed
    other = sscam(m, images, n_samples=N, sigma=sigma, batch=batch, seed=SEED + 1)
    assert not torch.equal(other, results["sscam"])
    assert "seed" not in inspect.signature(iscam).parameters and "sigma" not in inspect.signature(iscam).parameters
    with pytest.raises(TypeError):
        iscam(m, images, n_samples=N, batch=batch, seed=1)
    assert not torch.equal(results["sscam"], results["iscam"])
    # ---- one sample, no noise: Score-CAM bit for bit
    plain = scorecam(m, images, batch=batch)
    assert torch.equal(sscam(m, images, n_samples=1, sigma=0.0, batch=batch), plain)
    assert torch.equal(iscam(m, images, n_samples=1, batch=batch), plain)
    # ---- the documented errors
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            sscam(m, images, classes=bad, n_samples=N, batch=batch)
        with pytest.raises(IndexError):
            iscam(m, images, classes=bad, n_samples=N, batch=batch)
    for kwargs in (dict(n_samples=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(batch=0),
                   dict(classes=torch.tensor([0, 1, 2]))):
        with pytest.raises(ValueError):
            sscam(m, images, **{**dict(n_samples=N, batch=batch), **kwargs})
    for kwargs in (dict(n_samples=0), dict(batch=0), dict(classes=torch.tensor([0, 1, 2]))):
        with pytest.raises(ValueError):
            iscam(m, images, **{**dict(n_samples=N, batch=batch), **kwargs})
    with pytest.raises(ValueError):
        sscam(m, images[0], n_samples=N, batch=batch)
    assert m.training and all(p.grad is None for p in m.parameters())
    # ---- BatchNorm-folded forwards
    m.set_inference_fold(True)
    folded = {method: call(batch=batch) for method, (call, _) in runs.items()}
    m.set_inference_fold(False)
    for method, S in results.items():
        diff, top = float((folded[method] - S).abs().max()), float(S.abs().max())
        print("%s folded against unfolded: max difference %.3e, max|S| %.3e, ratio %.3e" % (method, diff, top, diff / top))
        assert diff <= 1e-3 * top
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 6: maps and the test tool
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_sscam_iscam_maps_and_test_tool(use_slot, tmp_path, capsys):
    """sscam_maps / iscam_maps are K.cam_maps of sscam / iscam, bytewise; scouter_amd.test run_sscam / run_iscam write
    sscam_0.png .. sscam_9.png and iscam_0.png .. iscam_9.png, 64 x 64, byte for byte the maps of the image; run_causal and
    run_infidelity score the families `sscam` and `iscam`"""
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.tools.attribution import iscam, iscam_maps, sscam, sscam_maps
    m, images = build(use_slot)
    skw, ikw = dict(n_samples=3, sigma=0.5, batch=100), dict(n_samples=3, batch=100)
    S, Z = sscam(m, images, **skw), iscam(m, images, **ikw)
    for min_level in (0.0, 0.3):
        for maps, flt in ((sscam_maps(m, images, min_level=min_level, **skw), S), (iscam_maps(m, images, min_level=min_level, **ikw), Z)):
            assert maps.dtype == torch.uint8 and maps.is_cuda and tuple(maps.shape) == (2, 10, 64, 64)
            assert torch.equal(maps, K.cam_maps(flt, 64, 64, min_level))
    assert tuple(sscam_maps(m, images, size=(32, 48), **skw).shape) == (2, 10, 32, 48)
    args = model_args(use_slot)
    args.device, args.grad_min_level, args.causal_step = "cuda", 0.2, 256
    args.sscam_samples, args.sscam_sigma, args.sscam_batch, args.iscam_samples, args.iscam_batch = 3, 0.5, 100, 3, 100
    args.infidelity_samples, args.infidelity_batch = 4, 5
    image = images[0].cpu()
    vis_dir = str(tmp_path / "vis")
    for stem, run, want in (("sscam", T.run_sscam, sscam_maps(m, images[:1], min_level=0.2, **skw)),
                            ("iscam", T.run_iscam, iscam_maps(m, images[:1], min_level=0.2, **ikw))):
        want = want[0].cpu().numpy()
        got = run(args, m, image, vis_dir)
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
    first = T.run_causal(args, m, image, pred, families=["sscam", "iscam"])
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("causal ")]
    assert len(lines) == 2 and list(first) == ["sscam", "iscam"]
    for ln, family in zip(lines, ("sscam", "iscam")):
        assert ln[:4] == ["causal", family, "class", "%d:" % pred]
        assert ln[4] == "deletion" and ln[6] == "insertion" and len(ln) == 8
        for v in first[family] + (float(ln[5]), float(ln[7])):
            assert np.isfinite(v) and 0.0 <= v <= 1.0
    assert T.run_causal(args, m, image, pred, families=["sscam", "iscam"]) == first         # two calls agree
    capsys.readouterr()
    scores = T.run_infidelity(args, m, image, pred, families=["sscam", "iscam"])
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("infidelity ")]
    assert len(lines) == 2 and [ln[1] for ln in lines] == ["sscam", "iscam"] and list(scores) == ["sscam", "iscam"]
    assert all(np.isfinite(v) for family in scores for v in scores[family])
