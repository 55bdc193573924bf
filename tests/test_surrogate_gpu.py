"""LIME and KernelSHAP (-m gpu): the six kernels of csrc/surrogate.hip one by one against NumPy float64 restatements written
here (no reference program is involved), their refusals, and tools/attribution.py superpixels / lime / kernelshap on an additive
toy module, whose segment sums both methods must return, and on whole models against a restatement that sends the same chunks
through the model and fits in NumPy.

Bounds.  slic_update sums in float64 and rounds once: within 1 fp32 ulp of the float64 mean rounded to fp32.  slic_assign
evaluates at most five terms in fp32, an error near 1e-6 relative, so its labels must equal the float64 argmin wherever the best
two float64 distances differ by more than 1e-4 relative (100 x); those pixels are at most 1 % of an image, asserted from the
float64 side alone.  segment_images and segment_paint copy values: bit-equal.  The moments are float64 sums of at most 1000
non-negative terms: rtol 1e-12.  The solve is compared with numpy.linalg.solve on the moments the kernel read at rtol 1e-9, after
cond(G) < 1e4 is asserted in NumPy (a float64 Cholesky errs near cond * 1e-16)."""
import argparse
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402

SENTINEL = -777.25
# (C, H, W, gy, gx)
SHAPES = [(3, 13, 17, 3, 4), (1, 33, 47, 5, 7), (3, 64, 64, 8, 8), (3, 224, 224, 8, 16), (1, 5, 7, 1, 1), (3, 5, 7, 5, 7)]
B = 2


def shape_id(s):
    return "x".join(str(v) for v in s)


def images_for(shape, seed=0):
    C, H, W = shape[:3]
    return np.random.default_rng(seed).standard_normal((B, C, H, W)).astype(np.float32)


def grid_labels(H, W, gy, gx):
    rows = (np.arange(H) * gy) // H
    cols = (np.arange(W) * gx) // W
    return (rows[:, None] * gx + cols[None, :]).astype(np.int32)


def slic_lambda(H, W, d, compactness=1.0):
    return (compactness / math.sqrt(H * W / d)) ** 2


def update64(x, labels, d, prev):
    """float64 centres [B, d, C + 2] and means [B, d, C]; a segment without a pixel keeps prev and gets means 0"""
    Bn, C, H, W = x.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    centres = np.array(prev, dtype=np.float64)
    means = np.zeros((Bn, d, C))
    for b in range(Bn):
        for l in range(d):
            m = labels[b] == l
            if m.any():
                means[b, l] = x[b][:, m].astype(np.float64).mean(axis=1)
                centres[b, l, :C] = means[b, l]
                centres[b, l, C] = yy[m].mean()
                centres[b, l, C + 1] = xx[m].mean()
    return centres, means


def within_one_ulp(got, ref64):
    ref32 = ref64.astype(np.float32)
    return np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1: K.slic_update
UPDATE_CASES = [(s, e) for s in SHAPES for e in (False, True) if not (e and s[3] * s[4] == 1)]     # (one segment cannot be empty)


@pytest.mark.parametrize("shape,empty", UPDATE_CASES, ids=["%s-%s" % (shape_id(s), "empty_segment" if e else "grid")
                                                           for s, e in UPDATE_CASES])
def test_slic_update_against_fp64(shape, empty):
    from scouter_amd import kernels as K
    C, H, W, gy, gx = shape
    d = gy * gx
    x = images_for(shape)
    labels = np.stack([grid_labels(H, W, gy, gx)] * B)
    gone = 1
    if empty:
        labels[labels == gone] = 0                                # segment 1 joins its left-hand neighbour
    prev = np.random.default_rng(1).standard_normal((B, d, C + 2)).astype(np.float32)
    want_c, want_m = update64(x, labels, d, prev)
    for window in (True, False):
        centres = torch.from_numpy(prev).cuda()
        means = torch.full((B, d, C), SENTINEL, device="cuda")
        K.slic_update(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), centres, means, gy, gx, window=window)
        torch.cuda.synchronize()
        got_c, got_m = centres.cpu().numpy(), means.cpu().numpy()
        assert within_one_ulp(got_c, want_c).all() and within_one_ulp(got_m, want_m).all()
        if empty:
            assert np.array_equal(got_c[:, gone], prev[:, gone]) and not got_m[:, gone].any()


# ------------------------------------------------------------------------------------------------ 2: K.slic_assign
def assign64(x, centres, gy, gx, lam):
    """float64 D^2 [B, d, H, W] of every pixel to every centre, infinite outside the 3 x 3 cells around the pixel's home cell"""
    Bn, C, H, W = x.shape
    d = gy * gx
    x = x.astype(np.float64)
    c = centres.astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ci, cj = ((np.arange(H) * gy) // H)[:, None], ((np.arange(W) * gx) // W)[None, :]
    D = np.full((Bn, d, H, W), np.inf)
    for l in range(d):
        i, j = divmod(l, gx)
        near = (np.abs(ci - i) <= 1) & (np.abs(cj - j) <= 1)
        for b in range(Bn):
            col = ((x[b] - c[b, l, :C, None, None]) ** 2).sum(axis=0)
            D[b, l] = np.where(near, col + lam * ((yy - c[b, l, C]) ** 2 + (xx - c[b, l, C + 1]) ** 2), np.inf)
    return D


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_slic_assign_against_fp64_argmin(shape):
    from scouter_amd import kernels as K
    C, H, W, gy, gx = shape
    d = gy * gx
    x = images_for(shape)
    grid = np.stack([grid_labels(H, W, gy, gx)] * B)
    centres = update64(x, grid, d, np.zeros((B, d, C + 2)))[0].astype(np.float32)         # grid-mean centres
    lam = np.float32(slic_lambda(H, W, d))
    D = assign64(x, centres, gy, gx, float(lam))
    want = D.argmin(axis=1)                                                               # (the first among equals)
    two = np.sort(D, axis=1)[:, :2] if d > 1 else None
    close = np.zeros((B, H, W), dtype=bool) if d == 1 else \
        np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] <= 1e-4 * two[:, 1])
    share = close.mean()
    print("slic_assign", shape, "pixels whose best two float64 distances lie within 1e-4 relative: %.4f %%" % (100 * share))
    assert share <= 0.01
    labels = torch.full((B, H, W), -5, dtype=torch.int32, device="cuda")
    K.slic_assign(torch.from_numpy(x).cuda(), torch.from_numpy(centres).cuda(), labels, gy, gx, float(lam))
    torch.cuda.synchronize()
    got = labels.cpu().numpy()
    assert got.min() >= 0 and got.max() < d
    off = got != want
    print("slic_assign", shape, "labels off the float64 argmin: %d, of them outside the margin: %d" % (off.sum(), (off & ~close).sum()))
    assert not (off & ~close).any()
    # a pixel's label is one of the 3 x 3 cells around its home cell
    assert (np.abs(got // gx - grid // gx) <= 1).all() and (np.abs(got % gx - grid % gx) <= 1).all()


def test_slic_assign_exact_tie_goes_to_the_smallest_label():
    """a constant image and two centres at x = 2 and x = 6: column 4 is exactly as far from both and lies in the home cell of
    label 1 -- label 0 wins"""
    from scouter_amd import kernels as K
    H, W, gy, gx = 4, 8, 1, 2
    x = torch.zeros((1, 1, H, W), device="cuda")
    centres = torch.tensor([[[0.0, 1.5, 2.0], [0.0, 1.5, 6.0]]], device="cuda")
    labels = torch.full((1, H, W), -5, dtype=torch.int32, device="cuda")
    K.slic_assign(x, centres, labels, gy, gx, 0.25)
    torch.cuda.synchronize()
    want = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1], dtype=torch.int32).expand(H, W)
    assert torch.equal(labels[0].cpu(), want)


# ------------------------------------------------------------------------------------------------ 3: superpixels
@pytest.mark.parametrize("shape", [(3, 13, 17, 3, 4), (3, 64, 64, 8, 8), (1, 5, 7, 1, 1)], ids=shape_id)
def test_superpixels_is_the_loop_of_the_two_kernels(shape):
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import superpixels
    C, H, W, gy, gx = shape
    d = gy * gx
    x = torch.from_numpy(images_for(shape)).cuda()
    grid = torch.from_numpy(np.stack([grid_labels(H, W, gy, gx)] * B)).cuda()
    plain = superpixels(x, (gy, gx), iters=0)
    assert plain.d == d and plain.labels.dtype == torch.int32 and torch.equal(plain.labels, grid)
    assert tuple(plain.means.shape) == (B, d, C) and plain.means.dtype == torch.float32
    iters, compactness = 3, 0.7
    seg = superpixels(x, (gy, gx), iters=iters, compactness=compactness)
    labels = grid.clone()
    centres = torch.zeros((B, d, C + 2), device="cuda")
    means = torch.empty((B, d, C), device="cuda")
    for _ in range(iters):
        K.slic_update(x, labels, centres, means, gy, gx)
        K.slic_assign(x, centres, labels, gy, gx, slic_lambda(H, W, d, compactness))
    K.slic_update(x, labels, centres, means, gy, gx)
    torch.cuda.synchronize()
    assert torch.equal(seg.labels, labels) and torch.equal(seg.means, means)
    assert int(seg.labels.min()) >= 0 and int(seg.labels.max()) < d
    if d > 1 and H > gy:
        assert not torch.equal(seg.labels, grid)                  # the loop moved something
    # labels from elsewhere, passed with d=: the means of those labels, scanned over the whole image
    given = superpixels(x, seg.labels, d=d)
    want = update64(x.cpu().numpy(), seg.labels.cpu().numpy(), d, np.zeros((B, d, C + 2)))[1]
    assert torch.equal(given.labels, seg.labels) and given.d == d and within_one_ulp(given.means.cpu().numpy(), want).all()
    if gy == gx and gy > 1:
        assert torch.equal(superpixels(x, gy, iters=iters, compactness=compactness).labels, seg.labels)    # an int: g x g


# ------------------------------------------------------------------------------------------------ 4: K.segment_images
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("hide", ["mean", 0.0, -1.5])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_segment_images_equal_torch_where(shape, hide, N):
    from scouter_amd import kernels as K
    C, H, W, gy, gx = shape
    d = gy * gx
    gen = torch.Generator().manual_seed(41 + N)
    image = torch.randn((C, H, W), generator=gen)
    labels = torch.randint(0, d, (H, W), generator=gen).to(torch.int32)
    z = (torch.rand((N, d), generator=gen) < 0.5).to(torch.uint8)
    means = torch.randn((d, C), generator=gen)
    keep = z[:, labels.long()].bool()[:, None]                                            # [N, 1, H, W]
    hidden = means[labels.long()].permute(2, 0, 1)[None] if hide == "mean" else torch.full((1, C, H, W), float(hide))
    want = torch.where(keep, image[None], hidden)
    buf = torch.full((N + 2, C, H, W), SENTINEL, device="cuda")                           # the chunk is shorter than the buffer
    got = K.segment_images(image.cuda(), labels.cuda(), z.cuda(), buf[:N], means.cuda() if hide == "mean" else None,
                           0.0 if hide == "mean" else hide)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and bool((buf[N:] == SENTINEL).all())
    assert torch.equal(buf[:N].cpu(), want)
    # labels outside [0, d) are clamped, not followed
    wild = labels.clone()
    wild[0, 0], wild[-1, -1] = -7, d + 1000
    K.segment_images(image.cuda(), wild.cuda(), z.cuda(), buf[:N], means.cuda() if hide == "mean" else None,
                     0.0 if hide == "mean" else hide)
    torch.cuda.synchronize()
    clamped = wild.clamp(0, d - 1).long()
    hidden = means[clamped].permute(2, 0, 1)[None] if hide == "mean" else hidden
    assert torch.equal(buf[:N].cpu(), torch.where(z[:, clamped].bool()[:, None], image[None], hidden))


# ------------------------------------------------------------------------------------------------ 5: K.surrogate_accumulate
def lime_weights64(z, kernel_width=0.25):
    d = z.shape[1]
    cnt = z.sum(axis=1).astype(np.float64)
    dist = np.where(cnt == 0, 1.0, 1.0 - np.sqrt(cnt / d))
    return np.sqrt(np.exp(-dist ** 2 / kernel_width ** 2))


def moments64(z, logp, cols, mode):
    """S [d + 1, d + 1], T [d + 1, K] and the targets y [N, K] in float64"""
    z = (z != 0).astype(np.float64)
    y = np.exp(logp.astype(np.float64))[:, cols]
    pi = lime_weights64(z) if mode == 0 else np.ones(z.shape[0])
    zh = np.concatenate([np.ones((z.shape[0], 1)), z], axis=1)
    return zh.T @ (pi[:, None] * zh), zh.T @ (pi[:, None] * y), y


def moment_inputs(N, d, Kc, seed, n_classes=7):
    gen = torch.Generator().manual_seed(seed)
    z = (torch.rand((N, d), generator=gen) < 0.5).to(torch.uint8)
    z[0], z[1] = 1, 0                                              # the full row and an all-zero row
    logp = F.log_softmax(torch.randn((N, n_classes), generator=gen), dim=1)
    cols = torch.tensor([5, 0, 5][:Kc], dtype=torch.int32)
    return z, logp, cols


def accumulate(z, logp, cols, mode, chunk):
    from scouter_amd import kernels as K
    N, d = z.shape
    Kc = cols.shape[0]
    S = torch.zeros((d + 1, d + 1), dtype=torch.float64, device="cuda")
    T = torch.zeros((d + 1, Kc), dtype=torch.float64, device="cuda")
    yref = torch.full((2, Kc), SENTINEL, dtype=torch.float64, device="cuda")
    zd, ld, cd = z.cuda(), logp.cuda(), cols.cuda()
    for n0 in range(0, N, chunk):
        K.surrogate_accumulate(ld[n0:n0 + chunk], cd, zd[n0:n0 + chunk], S, T, yref, n0, mode, 0.25)
    torch.cuda.synchronize()
    return S, T, yref


@pytest.mark.parametrize("mode", [0, 1], ids=["lime_weights", "unit_weights"])
@pytest.mark.parametrize("case", [(37, 12, 3), (64, 1, 1), (130, 128, 2)], ids=shape_id)
def test_surrogate_accumulate_against_fp64(case, mode):
    N, d, Kc = case
    z, logp, cols = moment_inputs(N, d, Kc, 50 + N)
    S, T, yref = accumulate(z, logp, cols, mode, N)
    wantS, wantT, y = moments64(z.numpy(), logp.numpy(), cols.numpy(), mode)
    np.testing.assert_allclose(S.cpu().numpy(), wantS, rtol=1e-12, atol=0)
    np.testing.assert_allclose(T.cpu().numpy(), wantT, rtol=1e-12, atol=0)
    np.testing.assert_allclose(yref.cpu().numpy(), y[:2], rtol=1e-12, atol=0)
    if mode == 0:
        assert abs(lime_weights64(z.numpy())[1] - math.sqrt(math.exp(-16.0))) < 1e-18       # the all-zero row: D = 1
    if N == 37:
        for chunk in (16, 5, 1):                                   # the rows in chunks: the same bits
            S2, T2, y2 = accumulate(z, logp, cols, mode, chunk)
            assert torch.equal(S2, S) and torch.equal(T2, T) and torch.equal(y2, yref)


# ------------------------------------------------------------------------------------------------ 6: K.surrogate_solve
def lime_system(S, T, alpha):
    s, S00 = S[1:, 0], S[0, 0]
    return S[1:, 1:] - np.outer(s, s) / S00 + alpha * np.eye(S.shape[0] - 1), T[1:] - np.outer(s, T[0]) / S00


def shap_system(S, T, yF, yE, alpha):
    S2, S1, T1 = S[1:, 1:], S[1:, 0], T[1:]
    e = S2.shape[0] - 1
    G = S2[:e, :e] - S2[:e, e:e + 1] - S2[e:e + 1, :e] + S2[e, e] + alpha * np.eye(e)
    R = T1[:e] - T1[e] - np.outer(S1[:e] - S1[e], yE) - np.outer(S2[:e, e] - S2[e, e], yF - yE)
    return G, R


def solve_inputs(N, d, Kc, shap, seed):
    from scouter_amd.tools.attribution import kernelshap_samples, lime_samples
    z = kernelshap_samples(N, d, seed) if shap else lime_samples(N, d, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    logp = torch.log(0.05 + 0.9 * torch.rand((z.shape[0], 7), generator=gen))
    logp[0], logp[1] = math.log(0.9), math.log(0.05)              # Delta = 0.85 in every class
    cols = torch.tensor([5, 0, 5][:Kc], dtype=torch.int32)
    return z, logp, cols


@pytest.mark.parametrize("case", [(64, 12, 3), (1000, 128, 2), (64, 1, 1)], ids=shape_id)
def test_surrogate_solve_lime_against_numpy(case):
    from scouter_amd import kernels as K
    N, d, Kc = case
    z, logp, cols = solve_inputs(N, d, Kc, False, 70 + d)
    S, T, _ = accumulate(z, logp, cols, 0, 250)
    for alpha in (1.0, 0.0):
        coef, icpt = K.surrogate_solve(S[None], T[None], None, K.SURROGATE_LIME, alpha)
        torch.cuda.synchronize()
        Sn, Tn = S.cpu().numpy(), T.cpu().numpy()
        G, R = lime_system(Sn, Tn, alpha)
        cond = np.linalg.cond(G)
        print("surrogate_solve LIME", case, "alpha", alpha, "cond(G) = %.3g" % cond)
        assert cond < 1e4
        w = np.linalg.solve(G, R)                                  # [d, K]
        assert tuple(coef.shape) == (1, Kc, d) and tuple(icpt.shape) == (1, Kc)
        np.testing.assert_allclose(coef[0].cpu().numpy(), w.T, rtol=1e-9, atol=0)
        np.testing.assert_allclose(icpt[0].cpu().numpy(), (Tn[0] - Sn[1:, 0] @ w) / Sn[0, 0], rtol=1e-9, atol=0)


@pytest.mark.parametrize("case", [(64, 12, 3), (1000, 128, 2), (2, 1, 1)], ids=shape_id)
def test_surrogate_solve_kernelshap_against_numpy(case):
    from scouter_amd import kernels as K
    N, d, Kc = case
    z, logp, cols = solve_inputs(N, d, Kc, True, 80 + d)
    S, T, yref = accumulate(z, logp, cols, 1, 250)
    two = 2                                                        # two images with the same moments: one workgroup each
    coef, icpt = K.surrogate_solve(torch.stack([S] * two), torch.stack([T] * two), torch.stack([yref] * two), K.SURROGATE_SHAP, 0.0)
    torch.cuda.synchronize()
    Sn, Tn, yn = S.cpu().numpy(), T.cpu().numpy(), yref.cpu().numpy()
    delta = yn[0] - yn[1]
    assert tuple(coef.shape) == (two, Kc, d) and torch.equal(coef[0], coef[1]) and torch.equal(icpt[0], icpt[1])
    phi = coef[0].cpu().numpy()
    if d > 1:
        G, R = shap_system(Sn, Tn, yn[0], yn[1], 0.0)
        cond = np.linalg.cond(G)
        print("surrogate_solve KernelSHAP", case, "cond(G) = %.3g" % cond)
        assert cond < 1e4
        np.testing.assert_allclose(phi[:, :d - 1], np.linalg.solve(G, R).T, rtol=1e-9, atol=0)
    else:
        assert np.array_equal(phi[:, 0], delta)                    # d = 1: phi_0 = Delta
    sums = np.array([math.fsum(phi[k]) for k in range(Kc)])
    print("surrogate_solve KernelSHAP", case, "efficiency: max |sum(phi) - Delta| / |Delta| = %.3g" % np.abs(sums / delta - 1).max())
    assert (np.abs(sums - delta) <= 1e-12 * np.abs(delta)).all()
    assert np.array_equal(icpt[0].cpu().numpy(), yn[1])


def test_surrogate_solve_rank_deficient_gives_nan_and_returns():
    """every sample row equal and no ridge: the second pivot is exactly 0 -> NaN coefficients, a clean return, and the next
    call is right"""
    from scouter_amd import kernels as K
    N, d, Kc = 64, 12, 2
    z = torch.tensor([1, 0] * (d // 2), dtype=torch.uint8).repeat(N, 1)
    logp = torch.log(0.05 + 0.9 * torch.rand((N, 7), generator=torch.Generator().manual_seed(5)))
    cols = torch.tensor([5, 0], dtype=torch.int32)
    S, T, yref = accumulate(z, logp, cols, 1, N)
    coef, icpt = K.surrogate_solve(S[None], T[None], yref[None], K.SURROGATE_SHAP, 0.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(coef).all()) and torch.equal(icpt[0], yref[1])
    coef, icpt = K.surrogate_solve(S[None], T[None], yref[None], K.SURROGATE_SHAP, 1.0)      # a ridge makes it definite
    torch.cuda.synchronize()
    assert bool(torch.isfinite(coef).all())
    G, R = shap_system(S.cpu().numpy(), T.cpu().numpy(), yref[0].cpu().numpy(), yref[1].cpu().numpy(), 1.0)
    np.testing.assert_allclose(coef[0, :, :d - 1].cpu().numpy(), np.linalg.solve(G, R).T, rtol=1e-9, atol=1e-18)


# ------------------------------------------------------------------------------------------------ 7: K.segment_paint
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_segment_paint_is_an_exact_gather(shape):
    from scouter_amd import kernels as K
    C, H, W, gy, gx = shape
    d, Kc = gy * gx, 3
    gen = torch.Generator().manual_seed(91)
    coef = torch.randn((B, Kc, d), generator=gen, dtype=torch.float64)
    labels = torch.randint(0, d, (B, H, W), generator=gen).to(torch.int32)
    labels[0, 0, 0], labels[1, -1, -1] = -3, d + 9                 # clamped
    got = K.segment_paint(coef.cuda(), labels.cuda())
    torch.cuda.synchronize()
    idx = labels.clamp(0, d - 1).long()[:, None].expand(B, Kc, H, W).reshape(B, Kc, H * W)
    want = torch.gather(coef.float(), 2, idx).reshape(B, Kc, H, W)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ 8: refusals
REFUSALS = [(call, bad) for call, bads in [
    ("slic_update", ["null", "d0", "d129", "grid_above_image"]),
    ("slic_assign", ["null", "d0", "d129", "grid_above_image"]),
    ("segment_images", ["null", "d0", "d129"]),
    ("surrogate_accumulate", ["null", "d0", "d129", "K0"]),
    ("surrogate_solve", ["null", "d0", "d129", "K0"]),
    ("segment_paint", ["null", "d0", "d129", "K0"])] for bad in bads]


@pytest.mark.parametrize("call,bad", REFUSALS, ids=["%s-%s" % r for r in REFUSALS])
def test_surrogate_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, d = 0, d = 129, a grid larger than the image, K = 0: an error naming the call at the library, every output
    untouched"""
    from scouter_amd import _native
    lib = _native.lib()
    Bn, C, H, W, N, Kc, nc = 1, 2, 8, 8, 3, 2, 5
    gy, gx = {"d0": (0, 4), "d129": (3, 43), "grid_above_image": (2, 9)}.get(bad, (2, 4))
    d = gy * gx
    if bad == "K0":
        Kc = 0
    null = bad == "null"
    D = 129                                                        # every buffer holds the largest d tried
    images = torch.ones((Bn, C, H, W), device="cuda")
    labels = torch.full((Bn, H, W), -9, dtype=torch.int32, device="cuda")
    centres = torch.full((Bn, D, C + 2), SENTINEL, device="cuda")
    means = torch.full((Bn, D, C), SENTINEL, device="cuda")
    z = torch.ones((N, D), dtype=torch.uint8, device="cuda")
    out = torch.full((N, C, H, W), SENTINEL, device="cuda")
    logp = torch.zeros((N, nc), device="cuda")
    cols = torch.zeros(2, dtype=torch.int32, device="cuda")
    S = torch.full((Bn, D + 1, D + 1), SENTINEL, dtype=torch.float64, device="cuda")
    T = torch.full((Bn, D + 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    yref = torch.full((Bn, 2, 2), SENTINEL, dtype=torch.float64, device="cuda")
    coef = torch.full((Bn, 2, D), SENTINEL, dtype=torch.float64, device="cuda")
    icpt = torch.full((Bn, 2), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.zeros(8 * D * (D + 2), dtype=torch.uint8, device="cuda")
    paint = torch.full((Bn, 2, H, W), SENTINEL, device="cuda")
    p = lambda t: t.data_ptr()                                     # noqa: E731
    with pytest.raises(RuntimeError, match=call):
        if call == "slic_update":
            rc = lib.scouter_slic_update_f32(p(images), p(labels), None if null else p(centres), p(means), Bn, C, H, W, gy, gx, 1, None)
        elif call == "slic_assign":
            rc = lib.scouter_slic_assign_f32(p(images), None if null else p(centres), p(labels), Bn, C, H, W, gy, gx, 0.1, None)
        elif call == "segment_images":
            rc = lib.scouter_segment_images_f32(p(images), p(labels), None if null else p(z), None, 0.0, p(out), N, d, C, H, W, None)
        elif call == "surrogate_accumulate":
            rc = lib.scouter_surrogate_accumulate_f64(p(logp), p(cols), p(z), None if null else p(S), p(T), p(yref), 0, N, nc, Kc, d,
                                                      0, 0.25, None)
        elif call == "surrogate_solve":
            rc = lib.scouter_surrogate_solve_f64(p(S), p(T), p(yref), None if null else p(coef), p(icpt), Bn, d, Kc, 1, 0.0, p(ws),
                                                 ws.numel(), None)
        else:
            rc = lib.scouter_segment_paint_f32(None if null else p(coef), p(labels), p(paint), Bn, Kc, d, H, W, None)
        assert rc == -1                                            # SC_ERR_ARG
        _native.check(rc, call)
    torch.cuda.synchronize()
    assert bool((labels == -9).all())
    for t in (centres, means, out, S, T, yref, coef, icpt, paint):
        assert bool((t == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 9: an additive toy module
class Additive(torch.nn.Module):
    """two outputs log(c_k + sum_p u_k[p] x[0, p]), kept inside (0, 1) for every subset of a non-negative image; the sum in
    float64, so the fp32 logarithm is the only rounding"""

    def __init__(self, u, c):
        super().__init__()
        self.register_buffer("u", u)
        self.register_buffer("c", c)

    def forward(self, x):
        return torch.log(self.c.double() + x[:, 0].flatten(1).double() @ self.u.double().t()).float().contiguous()


def test_additive_module_gives_back_its_segment_sums():
    from scouter_amd.tools.attribution import kernelshap, kernelshap_fit, lime_fit, superpixels
    H, W, gy, gx = 16, 20, 3, 4
    d = gy * gx
    gen = torch.Generator().manual_seed(3)
    image = torch.rand((1, 1, H, W), generator=gen) + 0.1
    u = torch.rand((2, H * W), generator=gen) + 0.1
    u = 0.5 * u / (u * image.flatten()).sum(dim=1, keepdim=True)   # sum_p u x = 0.5
    c = torch.tensor([0.2, 0.3])
    model = Additive(u, c).cuda()
    x = image.cuda()
    seg = superpixels(x, (gy, gx), iters=4)
    labels = seg.labels[0].cpu().numpy().ravel()
    terms = u.double().numpy() * image.double().numpy().ravel()                           # [2, HW]
    want = np.stack([np.bincount(labels, weights=terms[k], minlength=d) for k in range(2)])
    assert (want > 0).all()
    shap = kernelshap_fit(model, x, n_samples=64, segments=seg, batch=16, hide=0.0)
    lime = lime_fit(model, x, n_samples=64, segments=seg, batch=16, hide=0.0, ridge=0.0)
    torch.cuda.synchronize()
    for name, fit in (("kernelshap", shap), ("lime", lime)):
        got = fit.coef[0].cpu().numpy()
        err = np.abs(got / want - 1).max()
        print("additive module,", name, "max relative error of a segment sum %.3e" % err)
        assert tuple(fit.coef.shape) == (1, 2, d) and fit.coef.dtype == torch.float64 and err <= 1e-5
        np.testing.assert_allclose(fit.intercept[0].cpu().numpy(), c.numpy(), rtol=1e-5)
        assert torch.equal(fit.labels, seg.labels)
    painted = kernelshap(model, x, n_samples=64, segments=seg, batch=16, hide=0.0)
    assert torch.equal(painted[0].cpu(), shap.coef[0].float().cpu()[:, seg.labels[0].cpu().long()])


# ------------------------------------------------------------------------------------------------ 10: whole models
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


def model_targets(m, images, seg, z, batch, hide):
    """float64 [B, N, n]: exp of the HIP path's own log-probabilities -- the same chunks built with K.segment_images, the model
    in eval mode under no_grad at the same batch"""
    from scouter_amd import kernels as K
    Bn, C, H, W = images.shape
    N = z.shape[0]
    zd = z.cuda()
    was_training = m.training
    m.eval()
    ys = []
    try:
        with torch.no_grad():
            for b in range(Bn):
                logp = []
                for n0 in range(0, N, batch):
                    zc = zd[n0:n0 + batch]
                    chunk = K.segment_images(images[b], seg.labels[b], zc, torch.empty((zc.shape[0], C, H, W), device="cuda"),
                                             seg.means[b] if hide == "mean" else None, 0.0 if hide == "mean" else hide)
                    logp.append(m(chunk).cpu().double())
                ys.append(torch.cat(logp).exp())
    finally:
        m.train(was_training)
    return torch.stack(ys).numpy()


def lime_numpy(z, y, alpha):
    """ridge regression with a free, unpenalised intercept on (1, z): the augmented normal equations -> (w [K, d], b [K])"""
    z = z.astype(np.float64)
    pi = lime_weights64(z)
    zh = np.concatenate([np.ones((z.shape[0], 1)), z], axis=1)
    A = zh.T @ (pi[:, None] * zh) + alpha * np.diag([0.0] + [1.0] * z.shape[1])
    sol = np.linalg.solve(A, zh.T @ (pi[:, None] * y))
    return sol[1:].T, sol[0]


def kernelshap_numpy(z, y):
    """least squares with the intercept y[1] and the constraint sum(phi) = y[0] - y[1], by its KKT system -> phi [K, d]"""
    z = z.astype(np.float64)
    d = z.shape[1]
    A = np.zeros((d + 1, d + 1))
    A[:d, :d] = 2 * z.T @ z
    A[:d, d] = A[d, :d] = 1.0
    rhs = np.concatenate([2 * z.T @ (y - y[1]), (y[0] - y[1])[None]], axis=0)
    return np.linalg.solve(A, rhs)[:d].T


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_lime_and_kernelshap_on_whole_models(use_slot):
    from scouter_amd.tools import attribution as A
    m, images = build(use_slot)
    N, batch, segments = 64, 16, (3, 4)
    d = 12
    seg = A.superpixels(images, segments)
    m.train()
    before = bn_buffers(m)
    for name in ("lime", "kernelshap"):
        shap = name == "kernelshap"
        fit_fn, map_fn = (A.kernelshap_fit, A.kernelshap) if shap else (A.lime_fit, A.lime)
        z = A.kernelshap_samples(N, d, 0) if shap else A.lime_samples(N, d, 0)
        hide = 0.0 if shap else "mean"
        y = model_targets(m, images, seg, z, batch, hide)                                 # [B, N, 10]
        fit = fit_fn(m, images, n_samples=N, segments=segments, batch=batch, seed=0)
        maps = map_fn(m, images, n_samples=N, segments=segments, batch=batch, seed=0)
        torch.cuda.synchronize()
        assert torch.equal(fit.labels, seg.labels)
        assert tuple(fit.coef.shape) == (2, 10, d) and fit.coef.dtype == torch.float64 and tuple(fit.intercept.shape) == (2, 10)
        assert tuple(maps.shape) == (2, 10, 64, 64) and maps.dtype == torch.float32 and maps.is_cuda
        labels = seg.labels.cpu().numpy()
        for b in range(2):
            if shap:
                want, want_b = kernelshap_numpy(z.numpy(), y[b]), y[b][1]
            else:
                want, want_b = lime_numpy(z.numpy(), y[b], 1.0)
            got = fit.coef[b].cpu().numpy()
            print(name, "slot" if use_slot else "fc", "image", b, "max |coef| %.3e, max relative error %.3e"
                  % (np.abs(want).max(), np.abs(got / want - 1).max()))
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
            np.testing.assert_allclose(fit.intercept[b].cpu().numpy(), want_b, rtol=1e-9, atol=0)
            np.testing.assert_allclose(maps[b].cpu().numpy(), want[:, labels[b]], rtol=1e-6, atol=0)
        # ---- the state left behind
        assert m.training
        after = bn_buffers(m)
        assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
        assert all(p.grad is None for p in m.parameters())
        # ---- chunking, class selection
        whole = fit_fn(m, images, n_samples=N, segments=segments, batch=64, seed=0)
        assert torch.equal(whole.coef, fit.coef) and torch.equal(whole.intercept, fit.intercept)
        two = fit_fn(m, images, classes=[0, 3], n_samples=N, segments=segments, batch=batch, seed=0)
        assert tuple(two.coef.shape) == (2, 2, d)
        np.testing.assert_allclose(two.coef.cpu().numpy(), fit.coef[:, [0, 3]].cpu().numpy(), rtol=1e-9, atol=0)
        cls = torch.tensor([7, 2])
        own = fit_fn(m, images, classes=cls, n_samples=N, segments=segments, batch=batch, seed=0)
        assert tuple(own.coef.shape) == (2, 1, d)
        np.testing.assert_allclose(own.coef[:, 0].cpu().numpy(), np.stack([fit.coef[0, 7].cpu().numpy(), fit.coef[1, 2].cpu().numpy()]),
                                   rtol=1e-9, atol=0)
        for bad in ([10], [-1], torch.tensor([0, 10])):
            with pytest.raises(IndexError):
                fit_fn(m, images, classes=bad, n_samples=N, segments=segments, batch=batch)
        heat = (A.kernelshap_maps if shap else A.lime_maps)(m, images, classes=[1], min_level=0.2, n_samples=N, segments=segments,
                                                            batch=batch, seed=0)
        from scouter_amd import kernels as K
        assert heat.dtype == torch.uint8 and torch.equal(heat, K.heat_maps(maps[:, 1:2].contiguous(), 0.2))
    assert m.training and all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------ 11: the tool
TOOL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--lime", "true", "--shap", "true",
        "--lime_samples", "32", "--lime_batch", "16", "--lime_segments", "3", "--shap_samples", "32", "--shap_batch", "16",
        "--shap_segments", "3", "--grad_min_level", "0.2", "--eval_fold", "true"]


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_the_tool_on_one_image(use_slot, tmp_path, monkeypatch, capsys):
    """--table_images 0 (the default): lime_{c}.png and shap_{c}.png of every class, 64 x 64 bytes that are lime_maps /
    kernelshap_maps of the image, and one line per row for each of the three scores"""
    import os
    import sys
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools import surrogate as S
    from scouter_amd.tools.attribution import kernelshap_maps, lime_maps
    vis_dir = str(tmp_path / "vis")
    argv = ["surrogate.py"] + TOOL + ["--use_slot", "true" if use_slot else "false", "--causal", "true", "--causal_step", "2048",
                                      "--infidelity", "true", "--infidelity_samples", "3", "--sensitivity", "true",
                                      "--sensitivity_samples", "2", "--sensitivity_batch", "3", "--vis_dir", vis_dir, "--output_dir",
                                      str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    S.main()
    out = capsys.readouterr().out
    names = (["slot"] if use_slot else []) + ["lime", "shap"]
    for score in ("causal", "infidelity", "sensitivity"):
        lines = [ln.split() for ln in out.splitlines() if ln.startswith(score + " ")]
        assert [ln[1] for ln in lines] == names, (score, lines)
        for ln in lines:
            values = [float(w) for w in ln[4:] if w[0].isdigit() or w[0] == "-"]
            assert ln[2] == "class" and ln[3].endswith(":") and len(values) == {"causal": 2, "infidelity": 3, "sensitivity": 1}[score]
            assert all(math.isfinite(v) for v in values), ln
    # the files: 2 x num_classes maps (and the slot maps of the slot model), nothing else of another family
    files = sorted(os.listdir(vis_dir))
    want_files = ["%s_%d.png" % (n, c) for n in names for c in range(10)]
    assert files == sorted(want_files)
    # the bytes: the library's maps of the same image under the same options and the same weights
    args = S.get_surrogate_parser().parse_args(argv[1:])
    torch.manual_seed(11)
    model, _ = T.build_model(args)
    image = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))
    x = image[None].cuda()
    for name, fn in (("lime", lime_maps), ("shap", kernelshap_maps)):
        want = fn(model, x, min_level=0.2, **S.option_kwargs(args, name))[0].cpu().numpy()
        assert want.shape == (10, 64, 64) and want.dtype == np.uint8
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(vis_dir, "%s_%d.png" % (name, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
        assert any(m.any() for m in want)
    assert isinstance(model, SlotModel)


def test_the_tool_on_a_table(tmp_path, monkeypatch, capsys):
    """--table_images 8: the rows `table lime:` and `table shap:` after the table's own, every column filled, area in [0, 1]"""
    import sys
    from scouter_amd.tools import surrogate as S
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["surrogate.py"] + TOOL + [
        "--use_slot", "true", "--synthetic_data", "true", "--num_workers", "0", "--table_images", "8", "--batch_size", "4",
        "--localization", "true", "--causal", "true", "--causal_step", "2048", "--infidelity", "true", "--infidelity_samples", "3",
        "--cam", "true", "--output_dir", str(tmp_path / "none")])
    result = S.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == ["slot:", "cam:", "lime:", "shap:", "accuracy"]
    for ln in lines[2:4]:
        words = ln.split()
        assert words[2:4] == ["images", "8"] and words[4] == "area" and 0.0 <= float(words[5]) <= 1.0
        for column in ("precision", "pointing", "boxed", "empty", "deletion", "insertion", "infidelity"):
            assert column in words and math.isfinite(float(words[words.index(column) + 1])), (column, ln)
    for name in ("lime", "shap"):
        cols = result.rows[name]
        assert all(v.dtype == np.float64 and v.shape == (8,) for v in cols.values())
        assert ((cols["area"] >= 0) & (cols["area"] <= 1)).all() and (cols["boxed"] == 1).all()
