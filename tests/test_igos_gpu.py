"""I-GOS (-m gpu): the six entry points of csrc/igos.hip, each alone against the float64 restatement of tests/test_igos_cpu.py, then
tools/attribution.py igos on small black boxes and on a whole model, and test.py --igos.  No reference program is involved: every
expected value is the restated definition in float64.

EPS = 2^-24 (half an fp32 ulp, relative), U = 2^-53.  The source coordinates of the upsampler are fp32 by definition (one product,
one exact difference), so i0, i1 and t are the restatement's own.  M is the largest |cell| of a mask.  Every bound is twice a worst
case:

igos_upsample    top = fma(tx, a1 - a0, a0): the difference rounds once (EPS M), the fma once (EPS M): within 2 EPS M, and bot
                 likewise; bot - top inherits 4 EPS M and rounds once (EPS M), ty <= 1, the last fma rounds once (EPS M) and top
                 brings its own 2 EPS M: |u - ref| <= 8 EPS M; bound 16 EPS M.  A mask of all 0 gives 0 and a mask of all 1 gives 1,
                 exactly (a1 - a0 = 0).
igos_path_images m = a u rounds once and inherits a 8 EPS M: dm = 8 EPS M a + EPS |m|; d = image - base rounds once; x = fma(m, d,
                 base): |d| dm + EPS |m d| + EPS |x|; out = fma(sigma, z, x) with z the device's own value: + EPS |out|.  Twice the sum.
                 a = (float)(j + 1) / (float)S is fp32 by definition.
igos_accumulate  d is the fp32 difference by definition; dx d is exact in fp64 (24 + 24 bits), C fmas, one product w_j s and one fma
                 per row: (C + 2) U on every term and n U on the running sum; bound 2 (C + n + 2) U (|acc| + sum_j w_j sum_c |dx d|).
igos_mask_grad   wy, wx are exact in fp64 (1 - t: t has 24 bits), their product rounds once, a lane adds at most H W terms and the
                 butterfly six more; the regulariser's derivative is a handful of fp64 operations and two pow (a few U each) on at
                 most five terms of magnitude l1 / N + 4 tv beta / min(nr, nc) =: A_reg (|delta| <= 1); one rounding to fp32:
                 |dmask - ref| <= EPS |ref| + (H W + 40) U (U^T|acc| + A_reg); twice that.  stats: loss1 adds at most hm wm + 22 terms
                 per sum in fp64, pow within a few U: 2 (hm wm + 40) U loss1; the sum of squares, of the STORED dmask: the same
                 factor on the sum.
igos_trial_images the candidate fma(-step, dm, p) rounds once (EPS, |cand| <= 1) and the clamp does not expand; U inherits it: du =
                 9 EPS; out = fma(u, d, base): |d| du + EPS |u d| + EPS |out|; twice that.
igos_step        the inputs are built from few mantissa bits (p in 2^-8, dmask in 2^-6, steps powers of two), so every candidate is
                 exact and pmask must come back bit for bit; the logp columns are placed 0.05 from each threshold, so the choice does
                 not hang on a rounding; curves in fp64 as stats (1e-12 absolute covers them at these magnitudes).
trajectories     six iterations of the whole tool against the fp64 restatement, by the project's parity rule: the HIP error is at most
                 1.5 times the error of the same restatement run in torch fp32 on the CPU, or 1e-5 (the floor smoke() uses).  The
                 comparison means something because the fp64 run keeps every |tot_k - thr_k| it compared at least 1e-4 and never
                 reaches the last rung (asserted), so the three runs take the same steps."""
import math
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_extremal_cpu import LinearBox, fp32                                                                      # noqa: E402
from test_extremal_gpu import EPS, SENTINEL, U, NormBox, build_resnet18, place, report, sentinel_rows            # noqa: E402
from test_igos_cpu import (candidates, loss1, loss1_gradient, path_weights, run_trajectory, trajectory_case, upsample,   # noqa: E402
                           upsample_adjoint)

SHAPES = [(13, 10, 3, 5), (16, 16, 4, 4), (9, 7, 2, 2), (12, 8, 12, 8)]
SHAPE_IDS = ["13x10_3x5", "16x16_4x4", "9x7_2x2", "12x8_12x8"]
RC = [(1, 1), (1, 3), (3, 1), (3, 3)]
SEED = 12345


def masks(R, hm, wm, seed):
    """fp32 pmask [R, hm, wm] on the CPU: row 0 random with cells on both clamps, row 1 all 1, row 2 all 0"""
    p = torch.rand((R, hm, wm), generator=torch.Generator().manual_seed(seed))
    p[0, 0, 0], p[0, hm - 1, wm - 1] = 1.0, 0.0
    if R == 3:
        p[1], p[2] = 1.0, 0.0
    return p


def images(C, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((C, H, W), generator=gen), torch.randn((C, H, W), generator=gen)


def device_noise(C, H, W, n, seed=SEED, first=0):
    """z [n, C, H, W] fp32 on the device: kernels.noise_images on a zero image at sigma 1 is the noise itself"""
    from scouter_amd import kernels as K
    out = torch.empty((n, C, H, W), device="cuda")
    return K.noise_images(torch.zeros((C, H, W), device="cuda"), out, 1.0, seed, first)


# ------------------------------------------------------------------------------------------------ 1: K.igos_upsample
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES, ids=SHAPE_IDS)
def test_igos_upsample_against_fp64(H, W, hm, wm, off):
    from scouter_amd import kernels as K
    for R in (1, 3):
        p32 = masks(R, hm, wm, 10 + H)
        pd = place(p32, off)
        out, tail = sentinel_rows(R, (H, W), off)
        assert K.igos_upsample(pd, out) is out
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all()) and torch.equal(pd.cpu(), p32)
        ref = upsample(p32.double(), H, W)
        M = p32.double().abs().amax((1, 2)).view(R, 1, 1)
        report("igos_upsample %dx%d R %d" % (H, W, R), (out.cpu().double() - ref).abs(), (16 * EPS * M).expand_as(ref))
        if R == 3:
            assert bool((out[1] == 1.0).all()) and not bool(out[2].any())
            alone, _ = sentinel_rows(1, (H, W), not off)
            K.igos_upsample(place(p32[:1], not off), alone)
            assert torch.equal(alone[0], out[0])                            # the other path, one row: the same bits
        if (hm, wm) == (H, W):
            assert torch.equal(out.cpu(), p32)                              # a mask of the image's size is itself


# ------------------------------------------------------------------------------------------------ 2: K.igos_path_images
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES, ids=SHAPE_IDS)
def test_igos_path_images_against_fp64(H, W, hm, wm, off):
    from scouter_amd import kernels as K
    S, sigma, sample0 = 3, 0.25, 4
    for R, C in RC:
        p32 = masks(R, hm, wm, 20 + H)
        x32, b32 = images(C, H, W, 21 + H)
        pd, xd, bd = place(p32, off), place(x32, off), place(b32, off)
        out, tail = sentinel_rows(R * S, (C, H, W), off)
        assert K.igos_path_images(xd, bd, pd, out, 0, S, sigma, SEED, sample0) is out
        z = device_noise(C, H, W, S, SEED, sample0)
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all()) and all(torch.equal(a.cpu(), b) for a, b in ((pd, p32), (xd, x32), (bd, b32)))
        a = torch.tensor([float(np.float32(j + 1) / np.float32(S)) for j in range(S)], dtype=torch.float64).view(1, S, 1, 1, 1)
        u = upsample(p32.double(), H, W)[:, None, None]
        d = (x32.double() - b32.double())
        m = a * u
        xx = b32.double() + m * d
        ref = xx + fp32(sigma) * z.cpu().double()[None]
        M = p32.double().abs().amax((1, 2)).view(R, 1, 1, 1, 1)
        bound = 2 * (d.abs() * (8 * EPS * M * a + EPS * m.abs()) + EPS * (m * d).abs() + EPS * xx.abs() + EPS * ref.abs())
        got = out.view(R, S, C, H, W).cpu().double()
        report("igos_path_images %dx%d R %d C %d" % (H, W, R, C), (got - ref).abs(), bound)
        # every mask row saw the same noise, and sigma = 0 forms none: base + a U d by the two fmas of the definition, bit for bit
        plain, _ = sentinel_rows(R * S, (C, H, W), off)
        K.igos_path_images(xd, bd, pd, plain, 0, S, 0.0, SEED, sample0)
        up = torch.empty((R, H, W), device="cuda")
        K.igos_upsample(pd.contiguous(), up)
        a32 = torch.tensor([np.float32(j + 1) / np.float32(S) for j in range(S)], dtype=torch.float32).view(1, S, 1, 1, 1)
        m64 = (a32.double() * up.cpu().double()[:, None, None]).float().double()           # (one rounding: a 24 x 24 bit product)
        b64, q = b32.double().expand(R, S, C, H, W), m64 * (x32 - b32).double()            # (the product is exact in fp64)
        exact = b64 + q
        want = exact.float()                                                               # (fma: one rounding of the exact value)
        # ... except where the fp64 sum was itself rounded (TwoSum's error term is not 0) AND sits midway between two fp32
        # values: there the second rounding may go the other way; those elements are left out
        bb = exact - b64
        inexact = ((b64 - (exact - bb)) + (q - bb)) != 0
        toward = torch.where(exact > want.double(), math.inf, -math.inf).float().expand_as(want)
        tie = inexact & ((exact - want.double()).abs() == (torch.nextafter(want, toward).double() - exact).abs())
        assert int(tie.sum()) <= tie.numel() // 100
        assert torch.equal(plain.view(R, S, C, H, W).cpu()[~tie], want[~tie])
        if R == 3:
            assert torch.equal(plain.view(R, S, C, H, W)[2].cpu(), b32.expand(S, C, H, W))  # a mask of all 0: the baseline


def test_igos_path_images_chunks_are_one_call():
    from scouter_amd import kernels as K
    R, S, C, H, W = 3, 4, 3, 13, 10
    p, (x, b) = masks(R, 3, 5, 30).cuda(), (t.cuda() for t in images(C, H, W, 31))
    whole = torch.empty((R * S, C, H, W), device="cuda")
    K.igos_path_images(x, b, p, whole, 0, S, 0.2, SEED, 8)
    buf = torch.full((7, C, H, W), SENTINEL, device="cuda")
    for first, n in ((0, 2), (2, 5), (7, 5), (11, 1), (3, 1)):
        K.igos_path_images(x, b, p, buf[:n], first, S, 0.2, SEED, 8)
        assert torch.equal(buf[:n], whole[first:first + n]) and bool((buf[n:] == SENTINEL).all()), (first, n)
        buf.fill_(SENTINEL)
    other = torch.empty_like(whole)
    K.igos_path_images(x, b, p, other, 0, S, 0.2, SEED + 1, 8)
    assert not torch.equal(other, whole)
    K.igos_path_images(x, b, p[[0, 2, 1]].contiguous(), other, 0, S, 0.2, SEED, 8)
    assert torch.equal(other[:S], whole[:S]) and torch.equal(other[S:2 * S], whole[2 * S:])   # a row does not see its neighbours


# ------------------------------------------------------------------------------------------------ 3: K.igos_accumulate
def accumulate_reference(x32, b32, dx32, acc0, R, S):
    d = (x32 - b32).double()                                               # the fp32 difference, by definition
    _, w = path_weights(S)
    terms = dx32.double().view(R, S, *x32.shape) * d
    ref = acc0 + (w.view(1, S, 1, 1) * terms.sum(2)).sum(1)
    mag = acc0.abs() + (w.view(1, S, 1, 1) * terms.abs().sum(2)).sum(1)
    return ref, mag


@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES, ids=SHAPE_IDS)
def test_igos_accumulate_against_fp64(H, W, hm, wm, off):
    from scouter_amd import kernels as K
    S = 3
    for R, C in RC:
        gen = torch.Generator().manual_seed(40 + H + R)
        x32, b32 = images(C, H, W, 41 + H)
        dx32 = torch.randn((R * S, C, H, W), generator=gen)
        acc0 = torch.randn((R, H, W), generator=gen, dtype=torch.float64)
        xd, bd, dxd = place(x32, off), place(b32, off), place(dx32, off)
        acc, tail = sentinel_rows(R, (H, W), off, torch.float64)
        acc.copy_(acc0)
        assert K.igos_accumulate(xd, bd, dxd, acc, 0, S) is acc
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all()) and torch.equal(dxd.cpu(), dx32) and torch.equal(xd.cpu(), x32)
        ref, mag = accumulate_reference(x32, b32, dx32, acc0, R, S)
        report("igos_accumulate %dx%d R %d C %d" % (H, W, R, C), (acc.cpu() - ref).abs(), 2 * (C + R * S + 2) * U * mag)


def test_igos_accumulate_chunks_are_one_call():
    """three calls that cut a mask row's path in two and span two rows give the bits of one call, on either path"""
    from scouter_amd import kernels as K
    R, S, C = 3, 4, 3
    for H, W, off in ((13, 10, False), (16, 16, False), (16, 16, True)):
        gen = torch.Generator().manual_seed(50 + H)
        x, b = (place(t, off) for t in images(C, H, W, 51))
        dx = place(torch.randn((R * S, C, H, W), generator=gen), off)
        acc0 = torch.randn((R, H, W), generator=gen, dtype=torch.float64)
        one = place(acc0, off)
        K.igos_accumulate(x, b, dx, one, 0, S)
        three = place(acc0, off)
        for first, n in ((0, 2), (2, 5), (7, 5)):
            K.igos_accumulate(x, b, dx[first:first + n], three, first, S)
        assert torch.equal(one, three), (H, W, off)


# ------------------------------------------------------------------------------------------------ 4: K.igos_mask_grad
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES, ids=SHAPE_IDS)
def test_igos_mask_grad_against_fp64(H, W, hm, wm, off):
    from scouter_amd import kernels as K
    for R in (1, 3):
        for beta in (1.0, 2.0):
            gen = torch.Generator().manual_seed(60 + H + R)
            p32 = masks(R, hm, wm, 61 + H)
            acc64 = torch.randn((R, H, W), generator=gen, dtype=torch.float64)
            l1_32 = torch.rand((R,), generator=gen) + 0.5
            tv = 2.5
            pd, accd, l1d = place(p32, off), place(acc64, off), place(l1_32, off)
            dm, dm_tail = sentinel_rows(R, (hm, wm), off)
            st, st_tail = sentinel_rows(R, (2,), off, torch.float64)
            assert K.igos_mask_grad(pd, accd, l1d, dm, st, tv, beta) is dm
            torch.cuda.synchronize()
            assert bool((dm_tail == SENTINEL).all()) and bool((st_tail == SENTINEL).all())
            assert torch.equal(pd.cpu(), p32) and torch.equal(accd.cpu(), acc64) and torch.equal(l1d.cpu(), l1_32)
            p, l1 = p32.double(), l1_32.double()
            ref = upsample_adjoint(acc64, hm, wm) + loss1_gradient(p, l1, tv, beta)
            a_reg = l1.view(R, 1, 1) / (hm * wm) + 4 * tv * beta / min((hm - 1) * wm, hm * (wm - 1))
            bound = 2 * (EPS * ref.abs() + (H * W + 40) * U * (upsample_adjoint(acc64.abs(), hm, wm) + a_reg))
            what = "igos_mask_grad %dx%d R %d beta %g" % (H, W, R, beta)
            report(what, (dm.cpu().double() - ref).abs(), bound)
            want_loss = loss1(p, l1, tv, beta)
            want_sq = (dm.cpu().double() ** 2).sum((1, 2))
            report(what + " loss1", (st[:, 0].cpu() - want_loss).abs(), 2 * (hm * wm + 40) * U * want_loss)
            report(what + " sum of squares", (st[:, 1].cpu() - want_sq).abs(), 2 * (hm * wm + 40) * U * want_sq)
            if R == 3:                                                      # a row alone, on the other path: the same bits
                dm1, _ = sentinel_rows(1, (hm, wm), not off)
                st1, _ = sentinel_rows(1, (2,), not off, torch.float64)
                K.igos_mask_grad(place(p32[:1], not off), place(acc64[:1], not off), place(l1_32[:1], not off), dm1, st1, tv, beta)
                assert torch.equal(dm1[0], dm[0]) and torch.equal(st1[0], st[0])


def test_igos_mask_grad_at_the_real_size():
    """224 x 224 and the reference's two mask sizes, 8 x 8 (4761-pixel windows) and 112 x 112 (the largest mask: 12544 cells)"""
    from scouter_amd import kernels as K
    H = W = 224
    for hm in (8, 112):
        gen = torch.Generator().manual_seed(hm)
        p32 = torch.rand((2, hm, hm), generator=gen)
        acc64 = torch.randn((2, H, W), generator=gen, dtype=torch.float64)
        l1_32 = torch.tensor([1.0, 0.1])
        dm, st = torch.empty((2, hm, hm), device="cuda"), torch.empty((2, 2), dtype=torch.float64, device="cuda")
        K.igos_mask_grad(p32.cuda(), acc64.cuda(), l1_32.cuda(), dm, st, 20.0, 2.0)
        ref = upsample_adjoint(acc64, hm, hm) + loss1_gradient(p32.double(), l1_32.double(), 20.0, 2.0)
        a_reg = 1.0 / (hm * hm) + 4 * 20.0 * 2.0 / ((hm - 1) * hm)
        bound = 2 * (EPS * ref.abs() + (H * W + 40) * U * (upsample_adjoint(acc64.abs(), hm, hm) + a_reg))
        report("igos_mask_grad 224x224 <- %dx%d" % (hm, hm), (dm.cpu().double() - ref).abs(), bound)
        want = loss1(p32.double(), l1_32.double(), 20.0, 2.0)
        report("igos_mask_grad 224x224 <- %dx%d loss1" % (hm, hm), (st[:, 0].cpu() - want).abs(), 2 * (hm * hm + 40) * U * want)


# ------------------------------------------------------------------------------------------------ 5: K.igos_trial_images
@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES, ids=SHAPE_IDS)
def test_igos_trial_images_against_fp64(H, W, hm, wm, off):
    from scouter_amd import kernels as K
    steps32 = torch.tensor([0.0, 2.0, 0.5, 0.01])
    T1 = 4
    for R, C in RC:
        gen = torch.Generator().manual_seed(70 + H + R)
        p32 = masks(R, hm, wm, 71 + H)
        dm32 = torch.randn((R, hm, wm), generator=gen)
        x32, b32 = images(C, H, W, 72 + H)
        pd, dmd, xd, bd, sd = (place(t, off) for t in (p32, dm32, x32, b32, steps32))
        out, tail = sentinel_rows(R * T1, (C, H, W), off)
        assert K.igos_trial_images(xd, bd, pd, dmd, sd, out, 0) is out
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all()) and torch.equal(pd.cpu(), p32) and torch.equal(dmd.cpu(), dm32)
        cand = candidates(p32.double(), dm32.double(), steps32.double())
        u = upsample(cand, H, W)[:, :, None]
        d = x32.double() - b32.double()
        ref = b32.double() + u * d
        bound = 2 * (d.abs() * 9 * EPS + EPS * (u * d).abs() + EPS * ref.abs())
        got = out.view(R, T1, C, H, W).cpu().double()
        report("igos_trial_images %dx%d R %d C %d" % (H, W, R, C), (got - ref).abs(), bound)
        assert float(cand.min()) == 0.0 and float(cand.max()) == 1.0       # both clamps are met
        # step 0 is the mask as it stands: the noiseless end of the path, bit for bit
        end, _ = sentinel_rows(R, (C, H, W), off)
        K.igos_path_images(xd, bd, pd, end, 0, 1, 0.0, SEED, 0)
        assert torch.equal(out.view(R, T1, C, H, W)[:, 0], end)
        # a chunk in the middle of the stream
        if R == 3:
            part, part_tail = sentinel_rows(5, (C, H, W), off)
            K.igos_trial_images(xd, bd, pd, dmd, sd, part, 3)
            assert torch.equal(part, out[3:8]) and bool((part_tail == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 6: K.igos_step
STEP_LADDER = [0.0, 0.5, 0.25, 0.125]


def step_case(hm, wm, seed, n_out=3):
    """four rows whose hand-built logp make the line search take: the first candidate, a middle one, none (the last step is
    applied), and -- a NaN total -- the first.  Few mantissa bits everywhere: every candidate is exact in fp32."""
    gen = torch.Generator().manual_seed(seed)
    R, T1 = 4, len(STEP_LADDER)
    p = torch.randint(0, 257, (R, hm, wm), generator=gen).float() / 256.0
    dm = torch.randint(-64, 65, (R, hm, wm), generator=gen).float() / 64.0
    steps = torch.tensor(STEP_LADDER)
    l1, tv, beta, alpha = torch.full((R,), 0.125), 0.125, 2.0, 0.25 / (hm * wm)
    cols = torch.tensor([2, 0, 1, 1], dtype=torch.int32)
    cand = candidates(p.double(), dm.double(), steps.double())
    L = loss1(cand, l1.double().view(R, 1), tv, beta)                       # [R, T1]
    sumsq = (dm.double() ** 2).sum((1, 2))
    tot0 = L[:, 0] + 0.5
    thr = tot0[:, None] - alpha * steps.double()[None] * sumsq[:, None]
    accept = torch.tensor([[True, True, True], [False, True, True], [False, False, False], [False, False, False]])
    prob = torch.full((R, T1), 0.5, dtype=torch.float64)
    prob[:, 1:] = thr[:, 1:] - L[:, 1:] + torch.where(accept, -0.05, 0.05)
    assert float(prob.min()) > 0.05
    logp = torch.zeros((R, T1, n_out))                                      # (a wrong column would read probability 1)
    logp[torch.arange(R)[:, None], torch.arange(T1)[None], cols.long()[:, None]] = prob.log().float()
    logp[3, 1, cols[3]] = float("nan")
    want = [1, 2, 3, 1]
    stats = torch.stack([L[:, 0], sumsq], 1)
    return dict(R=R, T1=T1, p=p, dm=dm, steps=steps, l1=l1, tv=tv, beta=beta, alpha=alpha, cols=cols, cand=cand, L=L, logp=logp,
                want=want, stats=stats, n_out=n_out)


def run_step(c, off, it, n_iters, adapt, first_prob=None):
    from scouter_amd import kernels as K
    R = c["R"]
    pd, dmd, sd, ld = place(c["p"], off), place(c["dm"], off), place(c["steps"], off), place(c["logp"].view(-1, c["n_out"]), off)
    cd, std, l1d = c["cols"].cuda(), c["stats"].cuda(), place(c["l1"], off)
    curves, tail = sentinel_rows(R, (n_iters, 4), False, torch.float64)
    curves.zero_()
    if first_prob is not None:
        curves[:, 0, 1] = first_prob.cuda()
    assert K.igos_step(pd, dmd, sd, ld, cd, std, l1d, curves, it, n_iters, c["alpha"], c["tv"], c["beta"], adapt) is pd
    torch.cuda.synchronize()
    assert bool((tail == SENTINEL).all()) and torch.equal(dmd.cpu(), c["dm"]) and torch.equal(sd.cpu(), c["steps"])
    assert torch.equal(cd.cpu(), c["cols"]) and torch.equal(std.cpu(), c["stats"])
    return pd.cpu(), l1d.cpu(), curves.cpu()


@pytest.mark.parametrize("off", [False, True], ids=["dense", "off1"])
@pytest.mark.parametrize("hm,wm", [(3, 5), (4, 4), (2, 2), (12, 8), (40, 37)])
def test_igos_step_selects_as_the_reference_does(hm, wm, off):
    c = step_case(hm, wm, 80 + hm)
    p, l1, curves = run_step(c, off, 1, 5, True, torch.full((4,), 0.25, dtype=torch.float64))
    R = c["R"]
    assert curves[:, 1, 3].tolist() == [float(k) for k in c["want"]]
    assert curves[:, 1, 2].tolist() == [STEP_LADDER[k] for k in c["want"]]
    assert torch.equal(p, c["cand"][torch.arange(R), c["want"]].float())   # the candidate's bits (exact by construction)
    assert float((curves[:, 1, 0] - c["L"][:, 0]).abs().max()) <= 1e-12
    assert float((curves[:, 1, 1] - torch.exp(c["logp"][torch.arange(R), 0, c["cols"].long()].double())).abs().max()) <= 1e-12
    assert torch.equal(l1, c["l1"])                                         # (iteration 1 of 5 is no adjustment point)
    rest = curves.clone()
    rest[:, 1], rest[:, 0, 1] = 0.0, 0.0
    assert not bool(rest.any())                                             # the other iterations' entries are not written


def test_igos_step_adapts_l1_on_either_side_of_both_thresholds():
    c = step_case(3, 5, 90)
    prob0 = torch.exp(c["logp"][torch.arange(4), 0, c["cols"].long()].double())            # what this iteration records: 0.5
    tenth, fifth = c["l1"] / 10.0, c["l1"] / 5.0
    # it = 15 // 2 = 7: |prob - prob(0)| <= 1e-3 divides by 10
    first = prob0 + torch.tensor([5e-4, 2e-3, -9e-4, -1.1e-3], dtype=torch.float64)
    _, l1, _ = run_step(c, False, 7, 15, True, first)
    assert torch.equal(l1, torch.stack([tenth[0], c["l1"][1], tenth[2], c["l1"][3]]))
    # it = int(15 / 1.25) = 12: <= 1e-2 divides by 5
    first = prob0 + torch.tensor([5e-3, 2e-2, -9e-3, -1.1e-2], dtype=torch.float64)
    _, l1, _ = run_step(c, True, 12, 15, True, first)
    assert torch.equal(l1, torch.stack([fifth[0], c["l1"][1], fifth[2], c["l1"][3]]))
    # adapt off, another iteration, and n_iters <= 3 leave l1 alone
    same = prob0.clone()
    for it, n_iters, adapt in ((7, 15, False), (12, 15, False), (8, 15, True), (1, 3, True), (1, 2, True), (0, 1, True)):
        _, l1, _ = run_step(c, False, it, n_iters, adapt, same)
        assert torch.equal(l1, c["l1"]), (it, n_iters, adapt)
    # n_iters = 4: 4 // 2 = 2 and int(4 / 1.25) = 3
    _, l1, _ = run_step(c, False, 2, 4, True, same)
    assert torch.equal(l1, tenth)
    _, l1, _ = run_step(c, False, 3, 4, True, same)
    assert torch.equal(l1, fifth)
    # iteration 0 compares with itself (n_iters = 1 // ... never an adjustment point above 3 iterations): nothing moves
    _, l1, curves = run_step(c, False, 0, 15, True)
    assert torch.equal(l1, c["l1"]) and float((curves[:, 0, 1] - prob0).abs().max()) <= 1e-12


def test_the_wrappers_refuse_bad_shapes():
    from scouter_amd import kernels as K
    z = lambda *s, **k: torch.zeros(s, device="cuda", **k)                  # noqa: E731
    x, p = z(2, 13, 10), z(2, 3, 5)
    f64 = dict(dtype=torch.float64)
    bad_value = [
        lambda: K.igos_upsample(z(2, 1, 5), z(2, 13, 10)), lambda: K.igos_upsample(z(2, 14, 5), z(2, 13, 10)),
        lambda: K.igos_upsample(z(1, 129, 128), z(1, 224, 224)), lambda: K.igos_upsample(z(2, 2, 2), z(2, 1, 10)),
        lambda: K.igos_path_images(x, x, p, z(5, 2, 13, 10), 0, 2, 0.2, 0, 0), lambda: K.igos_path_images(x, x, p, z(2, 2, 13, 10), 3, 2, 0.2, 0, 0),
        lambda: K.igos_path_images(x, x, p, z(2, 2, 13, 10), -1, 2, 0.2, 0, 0), lambda: K.igos_path_images(x, x, p, z(2, 2, 13, 10), 0, 0, 0.2, 0, 0),
        lambda: K.igos_accumulate(x, x, z(5, 2, 13, 10), z(2, 13, 10, **f64), 0, 2),
        lambda: K.igos_trial_images(x, x, p, p.clone(), z(3), z(4, 2, 13, 10), 3),
        lambda: K.igos_trial_images(x, x, p, p.clone(), z(65), z(4, 2, 13, 10), 0),
        lambda: K.igos_step(p, p.clone(), z(3), z(6, 4), z(2, dtype=torch.int32), z(2, 2, **f64), z(2), z(2, 5, 4, **f64), 5, 5, 1e-4, 1.0, 2.0, True)]
    bad_runtime = [
        lambda: K.igos_upsample(p, z(3, 13, 10)), lambda: K.igos_upsample(p.double(), z(2, 13, 10)),
        lambda: K.igos_path_images(x, z(2, 13, 11), p, z(2, 2, 13, 10), 0, 2, 0.2, 0, 0),
        lambda: K.igos_path_images(x, x, p, z(2, 2, 13, 11), 0, 2, 0.2, 0, 0), lambda: K.igos_path_images(x, x, p, z(2, 2, 13, 10), 0, 2, -0.2, 0, 0),
        lambda: K.igos_accumulate(x, x, z(2, 2, 13, 10), z(2, 13, 10), 0, 2), lambda: K.igos_accumulate(x, x, z(2, 2, 13, 10), z(2, 13, 11, **f64), 0, 2),
        lambda: K.igos_mask_grad(p, z(2, 13, 10, **f64), z(3), z(2, 3, 5), z(2, 2, **f64), 1.0, 2.0),
        lambda: K.igos_mask_grad(p, z(2, 13, 10, **f64), z(2), z(2, 3, 5), z(2, 2), 1.0, 2.0),
        lambda: K.igos_mask_grad(p, z(2, 13, 10, **f64), z(2), z(2, 3, 5), z(2, 2, **f64), 1.0, 0.5),
        lambda: K.igos_mask_grad(p, z(2, 13, 10, **f64), z(2), z(2, 3, 5), z(2, 2, **f64), -1.0, 2.0),
        lambda: K.igos_trial_images(x, x, p, z(2, 3, 4), z(3), z(4, 2, 13, 10), 0), lambda: K.igos_trial_images(x, x, p, p.clone(), z(1), z(2, 2, 13, 10), 0),
        lambda: K.igos_step(p, p.clone(), z(3), z(5, 4), z(2, dtype=torch.int32), z(2, 2, **f64), z(2), z(2, 5, 4, **f64), 0, 5, 1e-4, 1.0, 2.0, True),
        lambda: K.igos_step(p, p.clone(), z(3), z(6, 4), z(2), z(2, 2, **f64), z(2), z(2, 5, 4, **f64), 0, 5, 1e-4, 1.0, 2.0, True),
        lambda: K.igos_step(p, p.clone(), z(3), z(6, 4), z(2, dtype=torch.int32), z(2, 2, **f64), z(2), z(2, 5, 4), 0, 5, 1e-4, 1.0, 2.0, True),
        lambda: K.igos_step(p, p.clone(), z(3), z(6, 4), z(2, dtype=torch.int32), z(2, 2, **f64), z(2), z(2, 5, 4, **f64), 0, 5, -1.0, 1.0, 2.0, True)]
    for kind, calls in ((ValueError, bad_value), (RuntimeError, bad_runtime)):
        for i, call in enumerate(calls):
            with pytest.raises(kind):
                call()
                pytest.fail("%s call %d was accepted" % (kind.__name__, i))


# ------------------------------------------------------------------------------------------------ 7: the trajectory
def test_a_short_trajectory_holds_the_parity_rule():
    from scouter_amd.tools.attribution import igos
    case = trajectory_case()
    n_iters, S, T = case["n_iters"], case["S"], len(case["ladder"]) - 1
    noise = device_noise(1, 16, 16, n_iters * S, SEED).view(n_iters, S, 1, 16, 16).cpu().double()
    t64, c64, margin, rungs = run_trajectory(case, noise, torch.float64)
    t32, c32, _, rungs32 = run_trajectory(case, noise, torch.float32)
    print("fp64 trajectory: least margin %.3e, rungs %s" % (margin, rungs))
    assert margin >= 1e-4 and all(k < T for it in rungs for k in it)       # the conditions, at every iteration
    assert rungs32 == rungs
    box = LinearBox(case["W_box"].float(), case["b_box"].float()).cuda()
    r = igos(box, case["image"].float().cuda()[None], classes=case["cols"], size=(case["hm"], case["wm"]), n_iters=n_iters, n_steps=S,
             l1_coeff=case["l1"], tv_coeff=case["tv"], tv_beta=case["beta"], sigma=case["sigma"], baseline=case["base"].float(),
             seed=SEED)
    torch.cuda.synchronize()
    assert r.curves[0, :, :, 3].cpu().tolist() == [[float(k[0]) for k in rungs]]
    assert torch.equal(r.curves[0, :, :, 2].cpu(), c64[:, :, 2])
    err_hip = float((r.pmasks[0].cpu().double() - t64[-1]).abs().max())
    err_32 = float((t32[-1].double() - t64[-1]).abs().max())
    cur_hip = float((r.curves[0, :, :, :2].cpu() - c64[:, :, :2]).abs().max())
    cur_32 = float((c32[:, :, :2].double() - c64[:, :, :2]).abs().max())
    print("igos after %d iterations: pmasks HIP %.3e vs fp32 %.3e; curves HIP %.3e vs fp32 %.3e" % (n_iters, err_hip, err_32, cur_hip, cur_32))
    assert float((t64[-1] - t64[0]).abs().max()) > 0.1
    assert err_hip <= max(1.5 * err_32, 1e-5)
    assert cur_hip <= max(1.5 * cur_32, 1e-5)
    mask = r.masks[0, 0].cpu().double()
    inside, outside = float(mask[case["inside"]].mean()), float(mask[~case["inside"]].mean())
    print("the mask ends at %.3f inside the patch and %.3f outside" % (inside, outside))
    assert inside < outside - 0.1


# ------------------------------------------------------------------------------------------------ 8: properties of the tool
SMALL = dict(size=(3, 4), n_iters=4, n_steps=3, l1_coeff=0.05, tv_coeff=0.5, blur_klen=5, blur_sigma=2.0)


def small_setup(B=2):
    box = NormBox(2, 13, 10, 3, 900).cuda().train()
    imgs = torch.randn((B, 2, 13, 10), generator=torch.Generator().manual_seed(901)).cuda()
    return box, imgs


def test_the_tool_repeats_and_depends_on_neither_batch_nor_classes():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import igos, igos_maps, igos_saliency
    box, imgs = small_setup()
    buffers = {k: v.detach().clone() for k, v in box.state_dict().items()}
    a = igos(box, imgs, classes=[2, 0], **SMALL)
    torch.cuda.synchronize()
    assert tuple(a.masks.shape) == (2, 2, 13, 10) and tuple(a.pmasks.shape) == (2, 2, 3, 4) and tuple(a.curves.shape) == (2, 2, 4, 4)
    assert a.masks.dtype == a.pmasks.dtype == torch.float32 and a.curves.dtype == torch.float64 and all(t.is_cuda for t in a)
    assert float(a.masks.min()) >= 0.0 and float(a.masks.max()) <= 1.0 and bool(torch.isfinite(a.curves).all())
    assert bool((a.pmasks != 1.0).any())
    for batch in (50, 1, 7):                                                # two calls; one row per pass; 7 cuts rows and rungs
        b = igos(box, imgs, classes=[2, 0], batch=batch, **SMALL)
        assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in a._fields), batch
    for k, c in enumerate((2, 0)):                                          # a class alone
        b = igos(box, imgs, classes=[c], **SMALL)
        assert all(torch.equal(getattr(a, f)[:, k], getattr(b, f)[:, 0]) for f in a._fields), c
    own = igos(box, imgs, classes=torch.tensor([0, 2]), **SMALL)
    assert torch.equal(own.pmasks[0, 0], a.pmasks[0, 1]) and torch.equal(own.pmasks[1, 0], a.pmasks[1, 0])
    every = igos(box, imgs[:1], **SMALL)
    assert tuple(every.masks.shape) == (1, 3, 13, 10) and torch.equal(every.pmasks[0, 2], a.pmasks[0, 0])
    assert box.training and all(torch.equal(buffers[k], v) for k, v in box.state_dict().items())
    assert all(q.grad is None for q in box.parameters())                    # a plain torch module: no .grad is touched
    # the masks are the upsampling of the coarse masks; the maps are 1 - masks through heat_maps
    again = torch.empty((4, 13, 10), device="cuda")
    K.igos_upsample(a.pmasks.view(4, 3, 4), again)
    assert torch.equal(again.view_as(a.masks), a.masks)
    assert torch.equal(igos_saliency(box, imgs, classes=[2, 0], **SMALL), 1.0 - a.masks)
    maps = igos_maps(box, imgs, classes=[2, 0], min_level=0.1, **SMALL)
    assert maps.dtype == torch.uint8 and torch.equal(maps, K.heat_maps(1.0 - a.masks, 0.1))
    # the documented columns: the regulariser of the mask before the update (0 for a mask of all 1 with no variation), the
    # probability, a step of the ladder and its index
    from scouter_amd.tools.attribution import igos_ladder
    ladder = torch.tensor(igos_ladder(), dtype=torch.float64).float().double()
    assert bool((a.curves[..., 0, 0] == 0.0).all()) and bool((a.curves[..., 1] > 0).all()) and bool((a.curves[..., 1] <= 1).all())
    k = a.curves[..., 3].cpu().long()
    assert bool((k >= 1).all()) and bool((k <= 12).all()) and torch.equal(a.curves[..., 2].cpu(), ladder[k])
    # init, and a mask that cannot move
    start = torch.rand((3, 4), generator=torch.Generator().manual_seed(5))
    still = igos(box, imgs, classes=[1], init=start, step0=1e-30, min_step=1e-31, **SMALL)
    assert float((still.pmasks.cpu() - start).abs().max()) <= 1e-6
    box.eval()
    igos(box, imgs[:1], classes=[0], **SMALL)
    assert not box.training


def test_igos_on_a_whole_model():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import igos
    m, imgs = build_resnet18()
    m.train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()
              if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    kw = dict(classes=[0, 3], size=8, n_iters=2, n_steps=3)
    a = igos(m, imgs[:1], **kw)
    b = igos(m, imgs[:1], **kw)
    torch.cuda.synchronize()
    assert tuple(a.masks.shape) == (1, 2, 64, 64) and tuple(a.pmasks.shape) == (1, 2, 8, 8) and tuple(a.curves.shape) == (1, 2, 2, 4)
    assert all(bool(torch.isfinite(t).all()) for t in a) and float(a.masks.min()) >= 0.0 and float(a.masks.max()) <= 1.0
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in a._fields)
    again = torch.empty((2, 64, 64), device="cuda")
    K.igos_upsample(a.pmasks[0], again)
    assert torch.equal(again, a.masks[0])
    assert bool((a.curves[..., 1] > 0).all()) and bool((a.curves[..., 1] <= 1).all())
    k = a.curves[..., 3]
    assert bool((k >= 1).all()) and bool((k <= 12).all()) and bool((k == k.round()).all()) and bool((a.curves[..., 2] > 0).all())
    assert bool((a.curves[:, :, 0, 0] == 0.0).all())                        # the regulariser of the initial mask of all 1
    assert m.training and all(torch.equal(before[k], v) for k, v in m.state_dict().items() if k in before)


def test_igos_test_tool(tmp_path, monkeypatch, capsys):
    """test.py --igos true writes igos_{c}.png for every class at the image size and, under --causal true, prints one `causal igos
    class <c>: ...` line"""
    from PIL import Image
    from scouter_amd import test as T
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "false", "--pre_trained", "false", "--img_size", "64",
        "--igos", "true", "--igos_iters", "1", "--igos_steps", "2", "--igos_size", "8", "--causal", "true",
        "--causal_step", "512", "--vis_dir", str(tmp_path / "vis"), "--output_dir", str(tmp_path / "none")])
    T.main()
    text = capsys.readouterr().out.splitlines()
    for c in range(10):
        assert Image.open(tmp_path / "vis" / ("igos_%d.png" % c)).size == (64, 64)
    lines = [ln.split() for ln in text if ln.startswith("causal ")]
    assert len(lines) == 1 and lines[0][1] == "igos" and lines[0][2] == "class" and lines[0][4] == "deletion"
    assert all(math.isfinite(float(lines[0][i])) for i in (5, 7))
