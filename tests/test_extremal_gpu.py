"""Extremal perturbation (-m gpu): the five entry points of csrc/extremal.hip, each alone and on the fp32 inputs of the float64
restatement of tests/test_extremal_cpu.py, then tools/attribution.py extremal_perturbation / extremal_maps on small black boxes
and on a whole model, and test.py --extremal.  No reference program is involved: every expected value is the restated definition
in float64.

EPS = 2^-24 (half an fp32 ulp, relative), U = 2^-53.  sqrtf and the division are correctly rounded, expf is within one ulp
(2 EPS).  D = 2 r + 1, D2 = D^2, BETA = 20.  Every bound is twice a worst case:

k                dy, dx and dy^2 + dx^2 are exact (half-integers); the root and the quotient by sigma round once each, so with
                 d = max(z - 0.5, 0) the error of d is at most EPS (3 d + 1); -2 d^2 then moves by at most EPS (14 d^2 + 4 d) and
                 expf adds 2 EPS: k is within ek = EPS (14 d^2 + 4 d + 2), relative.  v = k p rounds once more: dv = v (ek + EPS).
extremal_mask    the argument BETA (v - vmax) moves by BETA (dv_c + dv_max) <= 2 BETA DV, DV the window's largest dv, and by its two
                 roundings, 2 BETA EPS (|v - vmax| <= 1); expf adds 2 EPS: every e_c is within rho = 2 BETA DV + (2 BETA + 2) EPS,
                 relative.  den adds D2 positive terms (D2 EPS), num likewise by fmas of terms that carry dv_c as well, and the
                 quotient rounds once: |m - ref| <= ref (2 rho + (2 D2 + 1) EPS) + sum_c w_c dv_c =: bm; bound 2 bm.
                 stats: vmax within DV, den within den (rho + D2 EPS); twice each.
extremal_blend   m' = 1 - m and t = m' (L - 1) round once each: dt = 2 EPS t, and w = t - k is exact, so w carries dt; (1 - w), its
                 product with P[k] and the fma round once each: |x - ref| <= dt |P[k + 1] - P[k]| + 2 EPS (1 - w) |P[k]| + EPS |ref|;
                 twice that.  ON a knot (L = 3 and 5: m' = j / (L - 1) is exact in fp32) t, k and w are exact and the result is P[j]
                 bit for bit.
extremal_seed    one expf of an fp32 input: 2 EPS p; bound 4 EPS p.  The zeros are exact.
extremal_mask_grad the difference P[k + 1] - P[k] rounds once and C fmas add the channels: (C + 1) EPS S on the data term,
                 S = (L - 1) sum_c |dx (P[k + 1] - P[k])|; c2 rounds once, m - tau once, their product once, the final fma once:
                 (C + 1) EPS S + 3 EPS |c2 (m - tau)| + EPS |ref|; twice that.
extremal_step    a term dmask k w (1 + BETA (v - m)): w = expf(BETA (v - vmax_u)) / den_u reads the fp32 statistics extremal_mask left
                 (vmax within DV, den within rho + D2 EPS), so w is within om = BETA (dv + DV) + 2 BETA EPS + 2 EPS + rho + D2 EPS + EPS;
                 the factor f = 1 + BETA (v - m) reads the fp32 mask (within bm): df = BETA (dv + bm + EPS) + EPS |f|; three more
                 roundings form the term: |term| (ek + om + 3 EPS) + |dmask k w| df.  A lane adds ceil(side^2 / 64) terms, the
                 butterfly six more: N EPS sum |term|.  Bg = the sum of both.  buf = g (first: Bg) or fma(mu, buf, (1 - mu) g):
                 (1 - mu) Bg + EPS (2 |(1 - mu) g| + |buf|); p' = clamp(fma(-lr, buf, p)): lr dbuf + EPS |p - lr buf| (the clamp does not
                 expand).  Twice each.
trajectories     six iterations of the whole tool against the fp64 restatement, by the project's parity rule: the HIP error is at most
                 1.5 times the error of the same restatement run in torch fp32 on the CPU, or 1e-5 (the floor smoke() uses).  The
                 comparison means something because the fp64 run keeps the A-th and (A + 1)-th largest mask values 1e-4 apart and
                 every t 1e-4 from an interior knot at every iteration (asserted)."""
import argparse
import math
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA, MODEL_CASES, model_inputs             # noqa: E402
from test_extremal_cpu import (BETA, LinearBox, area_template, blend, cell_gradient, fp32, geometry, knots, mask_gradient,   # noqa: E402
                               momentum_step, patch_case, patch_margin, run_patch, run_trajectory, schedule, smooth_mask,
                               trajectory_case, window)

SENTINEL = -777.25
EPS, U = 2.0 ** -24, 2.0 ** -53
SHAPES = [(13, 10, 4, 6.0), (16, 16, 4, 4.0), (9, 7, 7, 21.0)]
SHAPE_IDS = ["13x10_s4_sig6", "16x16_s4_sig4", "9x7_s7_sig21"]


def off1(t):
    """the same data on the device at a pointer one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def place(t, off):
    return off1(t) if off else t.cuda().contiguous()


def sentinel_rows(n, shape, off, dtype=torch.float32):
    """(out [n, *shape] filled with the sentinel, the sentinel row behind it), dense or starting one element off"""
    E = int(np.prod(shape))
    flat = torch.full(((n + 1) * E + 1,), SENTINEL, device="cuda").to(dtype)
    start = 1 if off else 0
    whole = flat[start:start + (n + 1) * E].view((n + 1,) + tuple(shape))
    assert (whole.data_ptr() % 16 != 0) == bool(off)
    return whole[:n], whole[n]


def report(what, err, bound):
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), (what, float(err.max()), ratio)


def coarse_masks(H, W, s, sigma, n, seed):
    """fp32 pmask [n, hm, wm] in [0, 1] on the CPU"""
    hm, wm, _ = geometry(H, W, s, sigma)
    return torch.rand((n, hm, wm), generator=torch.Generator().manual_seed(seed))


def mask_error_model(p, win):
    """the restated mask of p (fp64) and the worst-case error terms of the docstring"""
    kern, _, _ = win
    m, v, w = smooth_mask(p, win)
    D2 = kern.shape[2] * kern.shape[3]
    d = torch.sqrt(-torch.log(kern) / 2.0)
    ek = EPS * (14.0 * d * d + 4.0 * d + 2.0)
    dv = v * (ek + EPS)
    DV = dv.flatten(3).max(3).values
    rho = 2.0 * BETA * DV + (2.0 * BETA + 2.0) * EPS
    bm = m * (2.0 * rho + (2.0 * D2 + 1.0) * EPS) + (w * dv).sum((3, 4))
    vmax = v.flatten(3).max(3).values
    den = torch.exp(BETA * (v - vmax[..., None, None])).sum((3, 4))
    return dict(m=m, v=v, w=w, ek=ek, dv=dv, DV=DV, rho=rho, bm=bm, vmax=vmax, den=den, D2=D2)


def run_mask(p32, H, W, s, sigma, off, want_stats=True):
    from scouter_amd import kernels as K
    n = p32.shape[0]
    pd = place(p32, off)
    out, out_tail = sentinel_rows(n, (H, W), off)
    stats, stats_tail = sentinel_rows(n, (H, W, 2), off) if want_stats else (None, None)
    assert K.extremal_mask(pd, out, s, sigma, stats) is out
    torch.cuda.synchronize()
    assert bool((out_tail == SENTINEL).all()) and torch.equal(pd.cpu(), p32)
    if want_stats:
        assert bool((stats_tail == SENTINEL).all())
    return pd, out, stats


# ------------------------------------------------------------------------------------------------ 1: K.extremal_mask
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W,s,sigma", SHAPES, ids=SHAPE_IDS)
def test_extremal_mask_against_fp64(H, W, s, sigma, n, off):
    from scouter_amd import kernels as K
    p32 = coarse_masks(H, W, s, sigma, n, 100 + H)
    if n == 3:
        p32[1], p32[2, 0, 0] = 0.0, 1.0
    win = window(H, W, s, sigma)
    em = mask_error_model(p32.double(), win)
    pd, out, stats = run_mask(p32, H, W, s, sigma, off)
    what = "extremal_mask %dx%d n %d" % (H, W, n)
    report(what, (out.cpu().double() - em["m"]).abs(), 2 * em["bm"])
    st = stats.cpu().double()
    report(what + " vmax", (st[..., 0] - em["vmax"]).abs(), 2 * em["DV"])
    report(what + " den", (st[..., 1] - em["den"]).abs(), 2 * em["den"] * (em["rho"] + em["D2"] * EPS))
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    if n == 3:
        assert not bool(out[1].any())                                       # an all-zero coarse mask: exactly 0
    # the same bits from a second call, without the statistics, and for a mask on its own (n does not enter)
    _, again, _ = run_mask(p32, H, W, s, sigma, off, want_stats=False)
    assert torch.equal(again, out)
    _, alone, _ = run_mask(p32[n - 1:], H, W, s, sigma, not off)
    assert torch.equal(alone[0], out[n - 1])


def test_extremal_mask_at_the_real_size():
    """(224, 224, 7, 21), n = 2: the 15.5 KB table, 49 workgroups per mask"""
    H, W, s, sigma, n = 224, 224, 7, 21.0, 2
    p32 = coarse_masks(H, W, s, sigma, n, 224)
    em = mask_error_model(p32.double(), window(H, W, s, sigma))
    _, out, stats = run_mask(p32, H, W, s, sigma, False)
    report("extremal_mask 224x224", (out.cpu().double() - em["m"]).abs(), 2 * em["bm"])
    st = stats.cpu().double()
    report("extremal_mask 224x224 vmax", (st[..., 0] - em["vmax"]).abs(), 2 * em["DV"])
    report("extremal_mask 224x224 den", (st[..., 1] - em["den"]).abs(), 2 * em["den"] * (em["rho"] + em["D2"] * EPS))


# ------------------------------------------------------------------------------------------------ 2: K.extremal_blend
def blend_inputs(H, W, L, n, seed):
    """fp32 (P [L, 3, H, W], m [n, H, W]) on the CPU.  L = 3, 5: the first pixels of every mask sit exactly on the knots 0,
    1 / (L - 1), ..., 1; row 1 (n = 3) is nearly constant, so that four neighbours share their piece."""
    gen = torch.Generator().manual_seed(seed)
    P = torch.randn((L, 3, H, W), generator=gen)
    m = torch.rand((n, H, W), generator=gen)
    if n == 3:
        m[1] = 0.3 + 0.01 * m[1]
    on = 0
    if L in (3, 5):
        on = L
        m.view(n, -1)[:, :L] = torch.arange(L, dtype=torch.float32) / (L - 1)
    return P, m, on


def knot_distance(m, L, variant, skip):
    """the least distance of t to an interior integer over the pixels behind the first `skip` of every mask"""
    t = ((1.0 - m if variant == "delete" else m) * (L - 1)).flatten(1)[:, skip:]
    near = torch.round(t)
    return float((t - near).abs()[(near >= 1) & (near <= L - 2)].min()) if L > 2 else 1.0


@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(13, 10), (16, 16), (9, 7)])
def test_extremal_blend_against_fp64(H, W, n, off):
    from scouter_amd import kernels as K
    for L in (3, 5, 8):
        P32, m32, on = blend_inputs(H, W, L, n, 200 + 10 * H + L)
        P, m = P32.double(), m32.double()
        Pd, md = place(P32, off), place(m32, off)
        for variant in ("preserve", "delete"):
            assert knot_distance(m, L, variant, on) >= 1e-4               # a condition on the inputs: every pixel, none left out
            ref, _ = blend(P, m, variant)
            k, w = knots(m, L, variant)
            p0 = torch.gather(P.unsqueeze(0).expand(n, L, 3, H, W), 1, k[:, None, None].expand(n, 1, 3, H, W)).squeeze(1)
            slope = blend(P, m, variant)[1].abs() / (L - 1.0)                # |P[k + 1] - P[k]|
            t = ((1.0 - m if variant == "delete" else m) * (L - 1))[:, None]
            bound = 2 * (2 * EPS * t * slope + 2 * EPS * (1.0 - w[:, None]) * p0.abs() + EPS * ref.abs())
            for flip in (False, True):
                out, tail = sentinel_rows(n, (3, H, W), off)
                assert K.extremal_blend(Pd, md, out, variant, flip) is out
                torch.cuda.synchronize()
                assert bool((tail == SENTINEL).all())
                got = out.cpu().double()
                got = got.flip(-1) if flip else got                          # back to the mask's own pixels
                report("extremal_blend %dx%d L %d %s flip %d" % (H, W, L, variant, flip), (got - ref).abs(), bound)
                if on:                                                       # on a knot: the level itself, bit for bit
                    js = torch.arange(L) if variant == "preserve" else (L - 1) - torch.arange(L)
                    for i in range(L):
                        y, x = divmod(i, W)
                        assert torch.equal(got[:, :, y, x], P[int(js[i])][:, y, x].expand(n, 3)), (L, variant, flip, i)
                # the other form (the same data, moved by one float) gives the same bits
                other, _ = sentinel_rows(n, (3, H, W), not off)
                K.extremal_blend(place(P32, not off), place(m32, not off), other, variant, flip)
                assert torch.equal(other, out)


def test_extremal_blend_at_the_real_size():
    """(224, 224), L = 8, n = 2: t = piece + 0.001 + 0.998 u by construction, so that all 50176 pixels can meet the condition"""
    from scouter_amd import kernels as K
    L, n, H, W = 8, 2, 224, 224
    gen = torch.Generator().manual_seed(2240)
    P32 = torch.randn((L, 3, H, W), generator=gen)
    piece = torch.randint(0, L - 1, (n, H, W), generator=gen).float()
    m32 = (piece + 0.001 + 0.998 * torch.rand((n, H, W), generator=gen)) / (L - 1)
    P, m = P32.double(), m32.double()
    out, tail = sentinel_rows(n, (3, H, W), False)
    for variant, flip in (("preserve", False), ("delete", True)):
        assert knot_distance(m, L, variant, 0) >= 1e-4
        K.extremal_blend(P32.cuda(), m32.cuda(), out, variant, flip)
        ref, slope = blend(P, m, variant)
        k, w = knots(m, L, variant)
        p0 = torch.gather(P.unsqueeze(0).expand(n, L, 3, H, W), 1, k[:, None, None].expand(n, 1, 3, H, W)).squeeze(1)
        t = ((1.0 - m if variant == "delete" else m) * (L - 1))[:, None]
        bound = 2 * (2 * EPS * t * slope.abs() / (L - 1.0) + 2 * EPS * (1.0 - w[:, None]) * p0.abs() + EPS * ref.abs())
        got = out.cpu().double()
        report("extremal_blend 224x224 %s flip %d" % (variant, flip), ((got.flip(-1) if flip else got) - ref).abs(), bound)
    assert bool((tail == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3: K.extremal_seed
@pytest.mark.parametrize("variant", ["preserve", "delete"])
@pytest.mark.parametrize("n,n_out", [(1, 1), (3, 5), (10, 10), (300, 3)])
def test_extremal_seed_against_fp64(n, n_out, variant):
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(300 + n)
    logp = torch.log_softmax(torch.randn((n, n_out), generator=gen) * 3, dim=1)
    cols = torch.randint(0, n_out, (n,), generator=gen).to(torch.int32)
    cols[0] = 0
    n_iters, it = 4, 2
    seed = torch.full((n, n_out), SENTINEL, device="cuda")
    rewards = torch.full((n_iters, n), SENTINEL, device="cuda")
    assert K.extremal_seed(logp.cuda(), cols.cuda(), seed, rewards, it, variant) is seed
    torch.cuda.synchronize()
    p = torch.exp(logp.double()[torch.arange(n), cols.long()])
    want = torch.zeros((n, n_out), dtype=torch.float64)
    want[torch.arange(n), cols.long()] = p if variant == "delete" else -p
    bound = torch.zeros_like(want)
    bound[torch.arange(n), cols.long()] = 4 * EPS * p
    report("extremal_seed n %d %s" % (n, variant), (seed.cpu().double() - want).abs(), bound)
    report("extremal_seed rewards", (rewards[it].cpu().double() - p).abs(), 4 * EPS * p)
    assert bool((rewards[:it] == SENTINEL).all()) and bool((rewards[it + 1:] == SENTINEL).all())
    assert torch.equal(rewards[it], seed.cpu().abs().max(1).values.cuda())   # the reward and the seed are one expf


# ------------------------------------------------------------------------------------------------ 4: K.extremal_mask_grad
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(13, 10), (16, 16), (9, 7)])
def test_extremal_mask_grad_against_fp64(H, W, n, off):
    from scouter_amd import kernels as K
    HW, C = H * W, 3
    lam = fp32(schedule(6)[5])
    for L in (3, 5, 8):
        P32, m32, on = blend_inputs(H, W, L, n, 400 + 10 * H + L)
        if n == 3:
            m32[2] = 0.5                                                    # every pixel ties; L = 3, 5: all of them on a knot
        gen = torch.Generator().manual_seed(401 + L)
        dx32 = torch.randn((n, C, H, W), generator=gen)
        targets = torch.tensor([max(1, (HW * (i + 1)) // 4) for i in range(n)], dtype=torch.int32)
        P, m, dx = P32.double(), m32.double(), dx32.double()
        Pd, md, dxd = place(P32, off), place(m32, off), place(dx32, off)
        ranks = K.saliency_ranks(m32.cuda().view(n, HW))                    # on the same fp32 mask: ties are not at issue
        if n == 3:
            assert torch.equal(ranks[2].cpu(), torch.arange(HW, dtype=torch.int32))       # ties by ascending index
        rk = place(ranks.cpu(), off)
        for variant in ("preserve", "delete"):
            free = m[:2] if n == 3 else m
            assert knot_distance(free, L, variant, on) >= 1e-4
            for flip in (False, True):
                ref = torch.cat([mask_gradient(P, m[i:i + 1], dx[i:i + 1], int(targets[i]), lam, variant, flip) for i in range(n)])
                slope = blend(P, m, variant)[1].abs()                       # (L - 1) |P[k + 1] - P[k]|
                S = (slope * (dx.flip(-1) if flip else dx).abs()).sum(1)
                tau = torch.cat([area_template(m[i:i + 1], int(targets[i])) for i in range(n)])
                bound = 2 * ((C + 1) * EPS * S + 3 * EPS * (2.0 * lam / HW) * (m - tau).abs() + EPS * ref.abs())
                out, tail = sentinel_rows(n, (H, W), off)
                assert K.extremal_mask_grad(Pd, md, dxd, rk, place(targets, off), out, lam, variant, flip) is out
                torch.cuda.synchronize()
                assert bool((tail == SENTINEL).all())
                report("extremal_mask_grad %dx%d L %d %s flip %d" % (H, W, L, variant, flip), (out.cpu().double() - ref).abs(), bound)
                if n == 3:                                                  # the constant mask: tau is 1 on the first A indices
                    area = (2.0 * lam / HW) * (0.5 - (torch.arange(HW) < int(targets[2])).double())
                    data = ref[2].flatten() - (2.0 * lam / HW) * (m[2] - tau[2]).flatten()
                    assert float((out[2].cpu().double().flatten() - data - area).abs().max()) <= float(bound[2].max())
                again, _ = sentinel_rows(n, (H, W), not off)
                K.extremal_mask_grad(place(P32, not off), place(m32, not off), place(dx32, not off), place(ranks.cpu(), not off),
                                     place(targets, not off), again, lam, variant, flip)
                assert torch.equal(again, out)


def test_extremal_mask_grad_at_the_real_size():
    """(224, 224), L = 8, n = 2: 196 tiles per mask, so the grid's second axis and the stride over it are in use; t = piece + 0.001
    + 0.998 u by construction, so that all 50176 pixels meet the knot condition"""
    from scouter_amd import kernels as K
    L, n, H, W, C = 8, 2, 224, 224, 3
    HW = H * W
    gen = torch.Generator().manual_seed(2241)
    P32 = torch.randn((L, C, H, W), generator=gen)
    piece = torch.randint(0, L - 1, (n, H, W), generator=gen).float()
    m32 = (piece + 0.001 + 0.998 * torch.rand((n, H, W), generator=gen)) / (L - 1)
    dx32 = torch.randn((n, C, H, W), generator=gen)
    targets = torch.tensor([int(0.1 * HW + 0.5), HW // 2], dtype=torch.int32)
    lam = fp32(schedule(800)[799])
    P, m, dx = P32.double(), m32.double(), dx32.double()
    Pd, md, dxd, tg = P32.cuda(), m32.cuda(), dx32.cuda(), targets.cuda()
    ranks = K.saliency_ranks(md.view(n, HW))
    tau = torch.cat([area_template(m[i:i + 1], int(targets[i])) for i in range(n)])
    assert torch.equal((ranks.cpu().view(n, H, W) < targets[:, None, None]).double(), tau)       # the ranking is the restatement's
    for variant in ("preserve", "delete"):
        assert knot_distance(m, L, variant, 0) >= 1e-4
        for flip in (False, True):
            ref = torch.cat([mask_gradient(P, m[i:i + 1], dx[i:i + 1], int(targets[i]), lam, variant, flip) for i in range(n)])
            S = (blend(P, m, variant)[1].abs() * (dx.flip(-1) if flip else dx).abs()).sum(1)
            bound = 2 * ((C + 1) * EPS * S + 3 * EPS * (2.0 * lam / HW) * (m - tau).abs() + EPS * ref.abs())
            out, tail = sentinel_rows(n, (H, W), False)
            K.extremal_mask_grad(Pd, md, dxd, ranks, tg, out, lam, variant, flip)
            torch.cuda.synchronize()
            assert bool((tail == SENTINEL).all())
            report("extremal_mask_grad 224x224 %s flip %d" % (variant, flip), (out.cpu().double() - ref).abs(), bound)


# ------------------------------------------------------------------------------------------------ 5: K.extremal_step
def step_case(H, W, s, sigma, n, first, off, seed, lr=0.4, mu=0.9):
    from scouter_amd import kernels as K
    hm, wm, r = geometry(H, W, s, sigma)
    gen = torch.Generator().manual_seed(seed)
    p32 = coarse_masks(H, W, s, sigma, n, seed + 1)
    dm32 = torch.randn((n, H, W), generator=gen)
    mom32 = torch.randn((n, hm, wm), generator=gen) * 4
    win = window(H, W, s, sigma)
    kern, cell, inside = win
    # the mask and its statistics as extremal_mask leaves them for this pmask
    pd, mask, stats = run_mask(p32, H, W, s, sigma, off)
    dmd = place(dm32, off)
    pbuf, ptail = sentinel_rows(n, (hm, wm), off)
    mbuf, mtail = sentinel_rows(n, (hm, wm), off)
    pbuf.copy_(p32)
    if not first:
        mbuf.copy_(mom32)
    keep = (mask.clone(), stats.clone(), dmd.clone())
    assert K.extremal_step(pbuf, mbuf, mask, dmd, stats, s, sigma, lr, mu, first) is pbuf
    torch.cuda.synchronize()
    assert bool((ptail == SENTINEL).all()) and bool((mtail == SENTINEL).all())
    assert torch.equal(mask, keep[0]) and torch.equal(stats, keep[1]) and torch.equal(dmd, keep[2])
    # the restated derivative and the update, in fp64 on the same fp32 inputs
    p, dm, mom = p32.double(), dm32.double(), mom32.double()
    lr64, mu64 = fp32(lr), fp32(mu)
    g = cell_gradient(dm, p, win)
    want_p, want_buf = momentum_step(p, None if first else mom, g, lr64, mu64, first)
    em = mask_error_model(p, win)
    m, v, w, dv = em["m"], em["v"], em["w"], em["dv"]
    up = lambda a: a[..., None, None]                                       # noqa: E731  (a per-pixel array against the window)
    f = 1.0 + BETA * (v - up(m))
    core = (up(dm) * kern * w).abs() * inside
    term = core * f.abs()
    om = BETA * (dv + up(em["DV"])) + 2 * BETA * EPS + 2 * EPS + up(em["rho"]) + em["D2"] * EPS + EPS
    df = BETA * (dv + up(em["bm"]) + EPS) + EPS * f.abs()
    term_err = term * (em["ek"] + om + 3 * EPS) + core * df
    adds = math.ceil(((2 * r + 1) * s) ** 2 / 64) + 6
    zero = torch.zeros((n, hm * wm), dtype=torch.float64)
    Bg = (zero.clone().index_add_(1, cell.flatten(), term_err.flatten(1))
          + adds * EPS * zero.clone().index_add_(1, cell.flatten(), term.flatten(1))).view(n, hm, wm)
    dbuf = Bg if first else (1.0 - mu64) * Bg + EPS * (2 * ((1.0 - mu64) * g).abs() + want_buf.abs())
    dp = lr64 * dbuf + EPS * (p - lr64 * want_buf).abs()
    what = "extremal_step %dx%d n %d first %d" % (H, W, n, first)
    report(what + " momentum", (mbuf.cpu().double() - want_buf).abs(), 2 * dbuf)
    report(what + " pmask", (pbuf.cpu().double() - want_p).abs(), 2 * dp)
    return pbuf, mbuf, want_p


@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W,s,sigma", SHAPES, ids=SHAPE_IDS)
def test_extremal_step_against_the_restated_derivative(H, W, s, sigma, n, first, off):
    pbuf, mbuf, want_p = step_case(H, W, s, sigma, n, first, off, 500 + H)
    got = pbuf.cpu()
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    if (H, W) != (9, 7):                                                    # (two cells only)
        assert bool((want_p == 0).any()) and bool((want_p == 1).any())      # both ends of the clamp are met ...
        agree = ((got == 0) == (want_p == 0)) & ((got == 1) == (want_p == 1))
        print("clamped cells: %d at 0, %d at 1 of %d; %d differ" % (int((got == 0).sum()), int((got == 1).sum()), got.numel(),
                                                                    int((~agree).sum())))
        assert bool((got == 0).any()) and bool((got == 1).any())            # ... and land exactly on them
    again, mom_again, _ = step_case(H, W, s, sigma, n, first, not off, 500 + H)
    assert torch.equal(again, pbuf) and torch.equal(mom_again, mbuf)        # two calls, two placements: the same bits


def test_extremal_step_at_the_real_size():
    step_case(224, 224, 7, 21.0, 2, False, False, 724, lr=0.01)


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_extremal_kernels_refuse_bad_arguments():
    from scouter_amd import kernels as K
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")      # noqa: E731
    p, m, st = z(2, 4, 3), z(2, 13, 10), z(2, 13, 10, 2)
    P, x = z(3, 2, 13, 10), z(2, 2, 13, 10)
    rk, tg = z(2, 130, dtype=torch.int32), z(2, dtype=torch.int32)
    bad = [
        lambda: K.extremal_mask(z(2, 4, 4), m, 4, 6.0),                      # the grid is 4 x 3
        lambda: K.extremal_mask(p, m, 4, 6.0, z(2, 13, 10)),                 # stats without its pair axis
        lambda: K.extremal_mask(p, m.double(), 4, 6.0),
        lambda: K.extremal_mask(p, m[:, :, ::2], 4, 6.0),                    # not contiguous
        lambda: K.extremal_mask(z(1, 14, 14), z(1, 224, 224), 16, 64.0),     # a table of 256 x 121 floats
        lambda: K.extremal_blend(P[:1], m, x),                               # one level
        lambda: K.extremal_blend(P, m, z(2, 3, 13, 10)),
        lambda: K.extremal_blend(P, m[:1], x),
        lambda: K.extremal_seed(z(2, 5), z(2, dtype=torch.int32), z(2, 5), z(4, 2), 4),           # it == n_iters
        lambda: K.extremal_seed(z(2, 5), z(2, dtype=torch.int64), z(2, 5), z(4, 2), 0),
        lambda: K.extremal_seed(z(2, 5), z(3, dtype=torch.int32), z(2, 5), z(4, 2), 0),
        lambda: K.extremal_mask_grad(P, m, x, rk[:, :100], tg, m.clone(), 1.0),
        lambda: K.extremal_mask_grad(P, m, x, rk, tg, m.clone(), -1.0),
        lambda: K.extremal_mask_grad(P, m, x, rk.float(), tg, m.clone(), 1.0),
        lambda: K.extremal_step(p, p.clone(), m, m.clone(), None, 4, 6.0, 0.01, 0.9, True),
        lambda: K.extremal_step(p, z(2, 4, 4), m, m.clone(), st, 4, 6.0, 0.01, 0.9, True),
        lambda: K.extremal_step(p, p.clone(), m, m.clone(), st, 4, 6.0, -0.01, 0.9, True),
        lambda: K.extremal_step(p, p.clone(), m, m.clone(), st, 4, 6.0, 0.01, 1.5, True),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail("call %d was accepted" % i)
    for call in (lambda: K.extremal_blend(P, m, x, "dual"), lambda: K.extremal_mask(p, m, 0, 6.0), lambda: K.extremal_mask(p, m, 4, 0.0)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ 7: the trajectories
@pytest.mark.parametrize("variant", ["preserve", "delete"])
def test_short_trajectories_hold_the_parity_rule(variant):
    from scouter_amd.tools.attribution import extremal_perturbation
    case = trajectory_case(variant)
    t64, r64, gaps, dists = run_trajectory(case, torch.float64)
    t32, r32, _, _ = run_trajectory(case, torch.float32)
    for it in range(case["n_iters"]):                                       # the two conditions, at every iteration
        assert gaps[it] >= 1e-4 and dists[it] >= 1e-4, (it, gaps[it], dists[it])
    box = LinearBox(case["W_box"].float(), case["b_box"].float()).cuda()
    image = case["image"].float().cuda()[None]
    init = case["p0"].float()[None, :, None]                                # [1, K = 2, A = 1, hm, wm]
    kw = dict(classes=case["cols"], areas=(case["area"],), step=case["s"], sigma=case["sigma"], levels=case["L"],
              max_blur=case["max_blur"], variant=variant, init=init)
    err_hip = err_32 = 0.0
    for it in range(1, case["n_iters"] + 1):
        r = extremal_perturbation(box, image, n_iters=it, **kw)
        e_hip = float((r.pmasks[0, :, 0].cpu().double() - t64[it]).abs().max())
        e_32 = float((t32[it].double() - t64[it]).abs().max())
        print("%s after %d iterations: HIP error %.3e, torch fp32 error %.3e" % (variant, it, e_hip, e_32))
        err_hip, err_32 = max(err_hip, e_hip), max(err_32, e_32)
    rew_hip = float((r.rewards[0, :, 0].cpu().double().t() - r64).abs().max())
    rew_32 = float((r32.double() - r64).abs().max())
    print("%s: pmasks HIP %.3e vs fp32 %.3e; rewards HIP %.3e vs fp32 %.3e; rank gap %.3e, knot distance %.3e"
          % (variant, err_hip, err_32, rew_hip, rew_32, min(gaps), min(dists)))
    assert float((t64[-1] - t64[0]).abs().max()) > 0.01
    assert err_hip <= max(1.5 * err_32, 1e-5)
    assert rew_hip <= max(1.5 * rew_32, 1e-5)


# ------------------------------------------------------------------------------------------------ 8: properties of the tool
class NormBox(torch.nn.Module):
    """a box with a BatchNorm in front: its buffers must not move"""

    def __init__(self, C, H, W, n_out, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.bn = torch.nn.BatchNorm2d(C)
        self.fc = torch.nn.Linear(C * H * W, n_out)
        with torch.no_grad():
            self.bn.running_mean.normal_()
            self.bn.running_var.uniform_(0.5, 2.0)
            self.fc.weight.mul_(3.0)

    def forward(self, x):
        # row by row: every row goes through launches of one shape, so its bits do not depend on the batch it came in
        return torch.cat([torch.log_softmax(self.fc(self.bn(x[i:i + 1]).flatten(1)), dim=1) for i in range(x.shape[0])])


SMALL = dict(step=4, sigma=6.0, levels=3, max_blur=3.0, n_iters=4)


def small_setup(B=2):
    box = NormBox(2, 13, 10, 3, 800).cuda().train()
    images = torch.randn((B, 2, 13, 10), generator=torch.Generator().manual_seed(801)).cuda()
    return box, images


def test_the_tool_repeats_and_does_not_depend_on_the_grouping():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import extremal_perturbation
    box, images = small_setup()
    buffers = {k: v.detach().clone() for k, v in box.state_dict().items()}
    kw = dict(classes=[0, 1, 2], areas=(0.2, 0.4), **SMALL)
    a = extremal_perturbation(box, images, **kw)
    torch.cuda.synchronize()
    assert tuple(a.masks.shape) == (2, 3, 2, 13, 10) and tuple(a.pmasks.shape) == (2, 3, 2, 4, 3)
    assert tuple(a.rewards.shape) == (2, 3, 2, 4) and all(t.dtype == torch.float32 and t.is_cuda for t in a)
    assert float(a.masks.min()) >= 0.0 and float(a.masks.max()) <= 1.0 and bool(torch.isfinite(a.rewards).all())
    assert bool((a.pmasks != 0.5).any())
    for batch in (50, 1, 4, 6):                                             # two calls; one row, 4 + 2 rows, all six
        b = extremal_perturbation(box, images, batch=batch, **kw)
        assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in a._fields), batch
    assert box.training and all(torch.equal(buffers[k], v) for k, v in box.state_dict().items())
    # the masks are the upsampling of the coarse masks
    again = torch.empty((12, 13, 10), device="cuda")
    K.extremal_mask(a.pmasks.view(12, 4, 3).contiguous(), again, 4, 6.0)
    assert torch.equal(again.view_as(a.masks), a.masks)
    # lr = 0 leaves the coarse masks where they started
    still = extremal_perturbation(box, images, lr=0.0, **kw)
    assert bool((still.pmasks == 0.5).all())
    box.eval()
    extremal_perturbation(box, images[:1], classes=[0], **SMALL)
    assert not box.training


def test_the_rewards_are_the_models_probabilities():
    from scouter_amd.tools.attribution import extremal_perturbation
    box, images = small_setup(1)
    seen = []
    hook = box.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().clone()))
    try:
        r = extremal_perturbation(box, images, classes=[2, 0], areas=(0.3,), batch=1, **SMALL)
        torch.cuda.synchronize()
    finally:
        hook.remove()
    assert len(seen) == 9 and all(tuple(o.shape) == (1, 3) for o in seen)                   # (one forward counts the outputs first)
    seen = seen[1:]
    for k, c in enumerate((2, 0)):
        for it in range(4):
            p = math.exp(float(seen[4 * k + it][0, c].double()))
            assert abs(float(r.rewards[0, k, 0, it]) - p) <= 4 * EPS * p, (k, it)


def test_the_three_forms_of_classes():
    from scouter_amd.tools.attribution import extremal_maps, extremal_perturbation
    box, images = small_setup()
    every = extremal_perturbation(box, images, **SMALL)
    assert tuple(every.masks.shape) == (2, 3, 1, 13, 10)
    some = extremal_perturbation(box, images, classes=[2, 0], **SMALL)
    assert torch.equal(some.pmasks[:, 0], every.pmasks[:, 2]) and torch.equal(some.pmasks[:, 1], every.pmasks[:, 0])
    own = extremal_perturbation(box, images, classes=torch.tensor([1, 2]), **SMALL)
    assert tuple(own.masks.shape) == (2, 1, 1, 13, 10)
    assert torch.equal(own.pmasks[0, 0], every.pmasks[0, 1]) and torch.equal(own.pmasks[1, 0], every.pmasks[1, 2])
    assert torch.equal(own.rewards[1, 0], every.rewards[1, 2])
    # the maps: the mean over the areas, 1 - the mean for "delete", then heat_maps
    from scouter_amd import kernels as K
    for variant in ("preserve", "delete"):
        kw = dict(classes=[1], areas=(0.2, 0.4), variant=variant, **SMALL)
        r = extremal_perturbation(box, images, **kw)
        mean = K.channel_mean(r.masks)
        want = K.heat_maps(1.0 - mean if variant == "delete" else mean, 0.1)
        maps = extremal_maps(box, images, min_level=0.1, **kw)
        assert maps.dtype == torch.uint8 and tuple(maps.shape) == (2, 1, 13, 10) and torch.equal(maps, want)
        assert float((mean.cpu().double() - r.masks.cpu().double().mean(2)).abs().max()) <= 2 * EPS


def test_a_patch_of_evidence_is_found():
    from scouter_amd.tools.attribution import extremal_perturbation
    case = patch_case()
    masks64, _ = run_patch(case)
    margin64 = patch_margin(masks64, case["inside"])
    assert margin64 >= 0.1
    box = LinearBox(case["W_box"].float(), case["b_box"].float()).cuda()
    r = extremal_perturbation(box, case["image"].float().cuda()[None], classes=[1], areas=(case["area"],), n_iters=case["n_iters"],
                              step=case["s"], sigma=case["sigma"], levels=case["L"], max_blur=case["max_blur"], lr=case["lr"],
                              area_weight=case["area_weight"])
    margin = patch_margin(r.masks[0, 0].cpu().double(), case["inside"])
    print("patch margin: HIP %.4f, fp64 restatement %.4f" % (margin, margin64))
    assert margin >= 0.5 * margin64


# ------------------------------------------------------------------------------------------------ 9: a whole model and the tool
def build_resnet18():
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES["resnet18_mnist_64"]
    _, P, images, _ = model_inputs("resnet18_mnist_64")
    args = argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet", use_slot=True,
                              use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"], slots_per_class=spc, hidden_dim=64,
                              freeze_layers=0, vis=False, vis_id=0, loss_status=ls, power=power, to_k_layer=L, lambda_value=LAMBDA)
    m = SlotModel(args)
    m.load_state_dict(P)
    return m.cuda(), images[:2].cuda()


def test_extremal_perturbation_on_a_whole_model():
    from scouter_amd.tools.attribution import extremal_maps, extremal_perturbation
    m, images = build_resnet18()
    m.train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()
              if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    kw = dict(classes=[0, 3], areas=(0.1, 0.3), n_iters=3, step=8, sigma=16.0, levels=3)
    a = extremal_perturbation(m, images, **kw)
    b = extremal_perturbation(m, images, **kw)
    torch.cuda.synchronize()
    assert tuple(a.masks.shape) == (2, 2, 2, 64, 64) and tuple(a.pmasks.shape) == (2, 2, 2, 8, 8) and tuple(a.rewards.shape) == (2, 2, 2, 3)
    assert all(t.dtype == torch.float32 and t.is_cuda for t in a)
    assert float(a.masks.min()) >= 0.0 and float(a.masks.max()) <= 1.0 and bool(torch.isfinite(a.rewards).all())
    assert bool((a.rewards > 0).all()) and bool((a.rewards <= 1).all()) and bool((a.pmasks != 0.5).any())
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in a._fields)
    assert m.training and all(torch.equal(before[k], v) for k, v in m.state_dict().items() if k in before)
    maps = extremal_maps(m, images[:1], classes=[3], n_iters=2, step=8, sigma=16.0, levels=3)
    assert maps.dtype == torch.uint8 and tuple(maps.shape) == (1, 1, 64, 64)


def test_extremal_test_tool(tmp_path, monkeypatch, capsys):
    """test.py --extremal true writes extremal_{c}.png for every class and, under --causal true, prints one `causal extremal class
    <c>: ...` line"""
    from scouter_amd import test as T
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "false", "--pre_trained", "false", "--img_size", "64",
        "--extremal", "true", "--extremal_iters", "2", "--extremal_area", "0.2", "--extremal_batch", "4", "--causal", "true",
        "--causal_step", "512", "--vis_dir", str(tmp_path / "vis"), "--output_dir", str(tmp_path / "none")])
    T.main()
    text = capsys.readouterr().out.splitlines()
    for c in range(10):
        assert (tmp_path / "vis" / ("extremal_%d.png" % c)).exists()
    lines = [ln.split() for ln in text if ln.startswith("causal ")]
    assert len(lines) == 1 and lines[0][1] == "extremal" and lines[0][2] == "class" and lines[0][4] == "deletion"
    assert all(np.isfinite(float(lines[0][i])) for i in (5, 7))
