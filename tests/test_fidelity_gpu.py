"""Infidelity / max-sensitivity (-m gpu): the six entry points of csrc/fidelity.hip against float64, their refusals,
tools/attribution.py infidelity / sensitivity_max on a linear black box, on stub explainers and on whole models, and test.py
--infidelity / --sensitivity.  No reference program is involved: every expected value is float64 (or 80-bit) arithmetic on seeded
inputs, or the definition restated over the HIP path's own outputs (the bits of kernels.noise_images / kernels.uniform_images, the
model outputs and explanations recorded while the tool ran, the per-sample arrays the tool returns).

EPS = 2^-24 (half an fp32 ulp, relative), U = 2^-53 (the same for fp64).  Every bound is twice a worst case:

perturb_dots     p = -sigma z is exact in fp64 (24 x 24 bits); every term enters by one fma, and the at most E additions of one
                 sum (in a thread, across a wave, the waves, the workgroups) each round a partial sum that is at most
                 S = sum_e |a sigma z|: E U S; bound 2 E U S.  The reference sum is 80-bit.  Against the
                 restated normal_fp64 the z bits differ by at most noise_images' own bound 64 EPS rad (tests/test_pathgrad_gpu.py),
                 which the sum carries as sum_e |a| sigma 64 EPS rad.
uniform_images   d = fma(2, u, -1) and, with image 0 and radius 1, fma(1, d, 0) are exact: equal bits.  With an image, one fma:
                 |out - (x + r d)| <= EPS |x + r d|; bound 2 EPS |ref|.  |out - x| <= r |d| + EPS |ref| <= r + EPS (|x| + r);
                 bound r (1 + 2 EPS) + 2 EPS |x|: twice the rounding part, the box itself as it is.  Every case runs with
                 n = 1, inside one tile of 8 samples, one past it and into the second tile, cut at and beside the tile's edge.
output_deltas    log_prob: the difference of two fp32 values in fp64 rounds once: U |ref|; bound 2 U |ref|.  prob: exp in fp64
                 within 1 ulp (2 U relative) on the device and in the reference each, then the difference:
                 4 U (e^a + e^b) + U |ref|; twice that.
map_distances    d = (double)A_j - (double)A_0 rounds once (U, so 2 U on d^2), the M non-negative terms of num and of den enter by
                 one fma each ((M + 1) U relative), the quotient adds U: (2 M + 5) U on the radicand, halved by the root, which
                 adds U: (M + 3.5) U |term|; bound (2 M + 8) U |term|.  A zero term is exact.
infidelity_finish raw and normalized are sums of N non-negative fmas of a gap that rounds once: (N + 3) U relative.  beta: the
                 numerator within (N + 1) U sum |dot delta|, the denominator within (N + 1) U relative, the quotient U:
                 db = (N + 1) U sum |dot delta| / sum dot^2 + (N + 2) U |beta|.  The gap of normalized then moves by at most
                 t_j = db |dot_j| + U |gap_j| and its square by t_j (2 |gap_j| + t_j) -- not linearised: for N = 1 the gap itself is
                 rounding -- so normalized moves by m = mean_j t_j (2 |gap_j| + t_j), plus (N + 3) U (normalized + m).  Twice each.
sensitivity_finish a maximum: exact.
the linear box   out = fl32(W x + b) with the sum in fp64: |out - (W x + b)| <= EPS |out| + (E + 1) U (|W| |x| + |b|); x_j is one
                 fma: |x_j - (x + sigma z)| <= EPS |x_j|.  With a = W: dot - delta = sum_e W (x_j - x - sigma z) + the two output
                 roundings, so |dot_j - delta_j| <= g_j = (EPS + U) (|out_0| + |out_j|) + EPS |W| |x_j|
                 + 2 (E + 1) U (|W| (|x| + |x_j|) + |b|) + the dot's own E U S (bound: 2 g).  raw <= mean g^2 (bound: twice),
                 |beta - 1| <= sum |dot| g / sum dot^2 (bound: twice, plus the finish kernel's db), normalized <= raw (1 + (2 N + 8) U)
                 because beta minimises it (bound: (4 N + 16) U)."""
import argparse
import functools
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402
from test_fidelity_cpu import uniform_fp64                                  # noqa: E402
from test_pathgrad_cpu import normal_fp64                                   # noqa: E402

SENTINEL = -777.25
EPS, U = 2.0 ** -24, 2.0 ** -53
SEED = 0x9E3779B97F4A7C15                                                   # both key words in use, the high bits set
KT, JT = 4, 4                                                               # the register tiles of perturb_dots (asserted below)
IT = 8                                                                      # the samples a thread of uniform_images writes (too)

# ((C, H, W), the buffers start one element past a 16-byte boundary)
CASES = [((1, 5, 7), False),          # the one-element form, E % 4 = 3
         ((3, 8, 8), False),          # the 16-byte form
         ((1, 5, 7), True),
         ((3, 8, 8), True),           # E a multiple of 4 at a misaligned pointer: the one-element form
         ((3, 224, 224), False),      # 147 workgroups
         ((3, 300, 300), False)]      # 264 workgroups' worth of groups on a grid of 256: the threads stride, the last round partial
CASE_IDS = ["x".join(str(v) for v in s) + ("_off1" if off else "") for s, off in CASES]
KN = [(1, 1), (1, JT + 1), (KT, 1), (KT, JT + 1), (KT + 1, 1), (KT + 1, JT + 1)]


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


def per_sample(K, N):
    return torch.full((K, N), SENTINEL, dtype=torch.float64, device="cuda")


def untouched(t, first, n):
    """the columns of a per-sample array outside [first, first + n) still hold the sentinel"""
    return bool((t[:, :first] == SENTINEL).all()) and bool((t[:, first + n:] == SENTINEL).all())


def report(what, err, bound):
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max err %.3e, max err / bound %.3f" % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), (what, float(err.max()), ratio)


def noise_bits(shape, first, n, seed=SEED):
    """float64 [n, E] on the CPU: the exact z bits of kernels.noise_images(zeros, sigma = 1) for the samples first .. first + n - 1"""
    from scouter_amd import kernels as K
    out = torch.empty((n,) + tuple(shape), device="cuda")
    K.noise_images(torch.zeros(shape, device="cuda"), out, 1.0, seed, first)
    return out.cpu().double().view(n, -1).numpy()


def dots_reference(attrs, z, sigma):
    """(ref, S) float64 [K, n]: sum_e a (-sigma z) summed in 80 bits and S = sum_e |a sigma z|, for attrs [K, E], z [n, E]"""
    p = -(float(np.float32(sigma)) * z)                                      # exact: 24 x 24 bits
    a = attrs.astype(np.longdouble)
    ref = np.einsum("ke,je->kj", a, p.astype(np.longdouble))
    mag = np.einsum("ke,je->kj", np.abs(a), np.abs(p).astype(np.longdouble))
    return torch.from_numpy(ref.astype(np.float64)), torch.from_numpy(mag.astype(np.float64))


@functools.lru_cache(maxsize=None)
def attributions(shape, K):
    """fp32 (full [K, C, H, W], maps [K, H, W]) on the CPU: computed once, shared, never changed"""
    gen = torch.Generator().manual_seed(9500 + int(np.prod(shape)) + K)
    return torch.randn((K,) + tuple(shape), generator=gen), torch.randn((K,) + tuple(shape[1:]), generator=gen)


def test_the_tiles_are_the_librarys():
    from scouter_amd import kernels as K
    assert (K.PERTURB_DOTS_CLASS_TILE, K.PERTURB_DOTS_SAMPLE_TILE) == (KT, JT) and K.UNIFORM_IMAGES_SAMPLE_TILE == IT


# ------------------------------------------------------------------------------------------------ 1: K.perturb_dots
@pytest.mark.parametrize("Kc,n", KN, ids=["K%d_n%d" % kn for kn in KN])
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_perturb_dots_against_fp64(shape, off, Kc, n):
    from scouter_amd import kernels as K
    full, maps = attributions(shape, Kc)
    E, C = int(np.prod(shape)), shape[0]
    first, sigma = 3, 0.37
    N = first + n + 2
    move = off1 if off else (lambda t: t.cuda())
    fd, md = move(full), move(maps)
    z = noise_bits(shape, first, n)
    dots = per_sample(Kc, N)
    assert K.perturb_dots(fd, dots, sigma, SEED, first, n) is dots
    torch.cuda.synchronize()
    assert untouched(dots, first, n)
    ref, mag = dots_reference(full.view(Kc, E).numpy(), z, sigma)
    report("perturb_dots %s K %d n %d" % (shape, Kc, n), (dots[:, first:first + n].cpu() - ref).abs(), 2 * E * U * mag)
    assert bool((dots[:, first:first + n] != 0).all())
    # two chunks (which move the samples to other places of the sample tile) give the bits of one call
    two = per_sample(Kc, N)
    cut = min(2, n - 1)
    if cut:
        K.perturb_dots(fd, two, sigma, SEED, first, cut)
    K.perturb_dots(fd, two, sigma, SEED, first + cut, n - cut)
    assert torch.equal(two, dots)
    # the 16-byte form (dense) and the one-element form (the same data at a misaligned pointer): equal bits
    dense, moved = per_sample(Kc, N), per_sample(Kc, N)
    K.perturb_dots(full.cuda(), dense, sigma, SEED, first, n)
    K.perturb_dots(off1(full), moved, sigma, SEED, first, n)
    assert torch.equal(dense, moved) and torch.equal(dense, dots)
    # a map counts for every channel: the bits of the full form fed the map repeated over the channels
    as_map, as_full = per_sample(Kc, N), per_sample(Kc, N)
    K.perturb_dots(md, as_map, sigma, SEED, first, n, channels=C)
    K.perturb_dots(move(maps[:, None].expand((Kc,) + tuple(shape)).contiguous()), as_full, sigma, SEED, first, n)
    torch.cuda.synchronize()
    assert torch.equal(as_map, as_full) and untouched(as_map, first, n)
    mref, mmag = dots_reference(maps[:, None].expand((Kc,) + tuple(shape)).reshape(Kc, E).numpy(), z, sigma)
    report("perturb_dots %s K %d n %d map form" % (shape, Kc, n), (as_map[:, first:first + n].cpu() - mref).abs(), 2 * E * U * mmag)
    # sigma = 0: exact zeros
    zero = per_sample(Kc, N)
    K.perturb_dots(fd, zero, 0.0, SEED, first, n)
    assert bool((zero[:, first:first + n] == 0).all()) and untouched(zero, first, n)


@pytest.mark.parametrize("shape,off", [CASES[0], CASES[1]], ids=CASE_IDS[:2])
def test_perturb_dots_against_restated_philox(shape, off):
    """once against the float64 restatement of the noise itself: noise_images' bound 64 EPS rad carried through the sum"""
    from scouter_amd import kernels as K
    Kc, n, first, sigma = KT + 1, JT + 1, 3, 0.37
    full, _ = attributions(shape, Kc)
    E = int(np.prod(shape))
    pairs = [normal_fp64(SEED, first + j, E) for j in range(n)]
    z64, rad64 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    a = full.view(Kc, E).numpy()
    ref, mag = dots_reference(a, z64, sigma)
    carried = torch.from_numpy(np.einsum("ke,je->kj", np.abs(a).astype(np.float64), rad64)) * float(np.float32(sigma)) * 64 * EPS
    dots = per_sample(Kc, first + n)
    K.perturb_dots(full.cuda(), dots, sigma, SEED, first, n)
    report("perturb_dots %s against normal_fp64" % (shape,), (dots[:, first:].cpu() - ref).abs(), carried + 2 * E * U * mag)
    other = per_sample(Kc, first + n)
    K.perturb_dots(full.cuda(), other, sigma, SEED ^ (1 << 32), first, n)               # the high seed word matters
    assert not torch.equal(other, dots)


# ------------------------------------------------------------------------------------------------ 2: K.uniform_images
def d_reference(seed, first, n, shape):
    E = int(np.prod(shape))
    return torch.from_numpy(np.stack([uniform_fp64(seed, first + j, E) for j in range(n)])).view((n,) + tuple(shape))


@functools.lru_cache(maxsize=None)
def case_image(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(9600 + int(np.prod(shape))))


# n -> where a call is cut in two: inside the first sample tile, at the tile's edge, inside the second tile
UNIFORM_CUTS = {1: [], 5: [3], IT + 1: [IT], IT + 4: [IT, IT + 2]}


@pytest.mark.parametrize("n", sorted(UNIFORM_CUTS), ids=["n%d" % n for n in sorted(UNIFORM_CUTS)])
@pytest.mark.parametrize("shape,off", CASES, ids=CASE_IDS)
def test_uniform_images_against_restated_philox(shape, off, n):
    from scouter_amd import kernels as K
    image = case_image(shape)
    first = 3
    d64 = d_reference(SEED, first, n, shape)
    zero = torch.zeros(shape, device="cuda")
    out, behind = batch_buffer(n, shape, off)
    assert K.uniform_images(zero, out, 1.0, SEED, first).data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((behind == SENTINEL).all())
    assert torch.equal(out.cpu().double(), d64)                                          # 2 u - 1 and fma(1, d, 0) are exact
    assert float(out.abs().max()) < 1.0 and float(out.abs().min()) > 0.0
    # pieces equal one call; the two forms give equal bits
    for cut in UNIFORM_CUTS[n]:
        two, behind_two = batch_buffer(n, shape, off)
        K.uniform_images(zero, two[:cut], 1.0, SEED, first)
        K.uniform_images(zero, two[cut:], 1.0, SEED, first + cut)
        assert torch.equal(two, out) and bool((behind_two == SENTINEL).all())
    dense, _ = batch_buffer(n, shape, False)
    moved, _ = batch_buffer(n, shape, True)
    K.uniform_images(zero, dense, 1.0, SEED, first)
    K.uniform_images(off1(zero), moved, 1.0, SEED, first)
    assert torch.equal(dense, moved) and torch.equal(dense, out)
    # radius = 0 returns the image bit for bit
    xd = off1(image) if off else image.cuda()
    same, _ = batch_buffer(n, shape, off)
    K.uniform_images(xd, same, 0.0, SEED, first)
    assert all(torch.equal(same[j].cpu(), image) for j in range(n))
    # a non-zero image
    radius = float(np.float32(0.37))
    moved_x, behind = batch_buffer(n, shape, off)
    K.uniform_images(xd, moved_x, radius, SEED, first)
    torch.cuda.synchronize()
    assert bool((behind == SENTINEL).all())
    x64 = image.double()[None]
    ref = x64 + radius * d64
    got = moved_x.cpu().double()
    report("uniform_images %s radius %.2f" % (shape, radius), (got - ref).abs(), 2 * EPS * ref.abs())
    report("uniform_images %s stays in the box" % (shape,), (got - x64).abs(), radius * (1 + 2 * EPS) + 2 * EPS * x64.abs())
    # seeds that differ only in the high word differ; the noise stream of the same seed is another stream
    other, _ = batch_buffer(n, shape, off)
    K.uniform_images(zero, other, 1.0, SEED ^ (1 << 32), first)
    assert not torch.equal(other, out) and torch.equal(other.cpu().double(), d_reference(SEED ^ (1 << 32), first, n, shape))
    noise, _ = batch_buffer(n, shape, off)
    K.noise_images(zero, noise, 1.0, SEED, first)
    assert float((noise == out).float().mean()) < 0.01


# ------------------------------------------------------------------------------------------------ 3: K.output_deltas
@pytest.mark.parametrize("of", ["log_prob", "prob"])
@pytest.mark.parametrize("Kc,n,n_classes", [(1, 1, 5), (3, 5, 5), (10, 50, 10), (2, 300, 3)],
                         ids=["K1_n1", "K3_n5", "K10_n50", "K2_n300"])
def test_output_deltas_against_fp64(Kc, n, n_classes, of):
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(9700 + Kc + n)
    out = torch.log_softmax(3.0 * torch.randn((1 + n, n_classes), generator=gen), dim=1)
    cols = torch.randperm(n_classes, generator=gen)[:Kc]
    first = 2
    N = first + n + 3
    deltas = per_sample(Kc, N)
    assert K.output_deltas(out.cuda(), cols.to(torch.int32).cuda(), deltas, first, of) is deltas
    torch.cuda.synchronize()
    assert untouched(deltas, first, n)
    o = out.double()[:, cols]                                                            # [1 + n, K]
    if of == "log_prob":
        ref = (o[:1] - o[1:]).t()
        bound = 2 * U * ref.abs()
    else:
        e = torch.exp(o)
        ref = (e[:1] - e[1:]).t()
        bound = 2 * (4 * U * (e[:1] + e[1:]).t() + U * ref.abs())
    report("output_deltas %s K %d n %d" % (of, Kc, n), (deltas[:, first:first + n].cpu() - ref).abs(), bound)
    if of == "log_prob":
        assert torch.equal(deltas[:, first:first + n].cpu(), ref)                       # (the fp64 difference rounds the same way)
    again = per_sample(Kc, N)
    K.output_deltas(out.cuda(), cols.to(torch.int32).cuda(), again, first, of=of)
    assert torch.equal(again, deltas)


# ------------------------------------------------------------------------------------------------ 4: K.map_distances
def terms_reference(maps):
    """(terms, den) float64 [K, n] / [K] from maps [1 + n, K, M] (any float tensor on the CPU): the definition in 80 bits"""
    a = maps.double().numpy().astype(np.longdouble)
    a = a.reshape(a.shape[0], a.shape[1], -1)
    den = (a[0] * a[0]).sum(axis=1)
    den_used = np.where(den == 0, np.longdouble(1), den)
    num = ((a[1:] - a[:1]) ** 2).sum(axis=2)                                             # [n, K]
    return torch.from_numpy(np.sqrt(num / den_used[None]).astype(np.float64)).t().contiguous(), torch.from_numpy(den.astype(np.float64))


@pytest.mark.parametrize("Kc,n,item", [(1, 1, (7,)), (3, 5, (7, 7)), (2, 4, (3, 10, 10)), (1, 2, (3, 224, 224))],
                         ids=["K1_n1_M7", "K3_n5_M49", "K2_n4_M300", "K1_n2_M150528"])
def test_map_distances_against_fp64(Kc, n, item):
    from scouter_amd import kernels as K
    M = int(np.prod(item))
    gen = torch.Generator().manual_seed(9800 + M + Kc)
    maps = torch.randn((1 + n, Kc) + item, generator=gen)
    maps[1:] = maps[:1] + 0.1 * maps[1:]                                                 # near the clean explanation
    first = 2
    N = first + n + 1
    terms = per_sample(Kc, N)
    assert K.map_distances(maps.cuda(), terms, first) is terms
    torch.cuda.synchronize()
    assert untouched(terms, first, n)
    ref, _ = terms_reference(maps)
    report("map_distances K %d n %d M %d" % (Kc, n, M), (terms[:, first:first + n].cpu() - ref).abs(), (2 * M + 8) * U * ref.abs())
    assert bool((terms[:, first:first + n] > 0).all())
    # one sample at a time: the bits of one call (den comes from row 0 of each call, in the same order)
    one = per_sample(Kc, N)
    for j in range(n):
        K.map_distances(torch.cat([maps[:1], maps[1 + j:2 + j]]).cuda(), one, first + j)
    assert torch.equal(one, terms)
    assert torch.equal(K.map_distances(off1(maps), per_sample(Kc, N), first), terms)    # any 4-byte aligned pointer


def test_map_distances_edges():
    """den = 0 -> the sum of squares itself; a map equal to the clean one -> exactly 0; a NaN or an infinity in one sample -> that
    term alone is NaN / infinite; a NaN in the clean map -> every term of its class is NaN"""
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(9850)
    maps = torch.randn((5, 3, 6, 6), generator=gen)
    maps[0, 0] = 0.0                                                                     # class 0: a zero explanation, den = 1
    maps[2] = maps[0]                                                                    # sample 1 equals the clean row
    maps[3, 1, 2, 2] = float("nan")
    maps[4, 1, 0, 0] = float("inf")
    terms = per_sample(3, 4)
    K.map_distances(maps.cuda(), terms, 0)
    t = terms.cpu()
    ref, den = terms_reference(torch.nan_to_num(maps, nan=0.0, posinf=0.0))
    assert float(den[0]) == 0.0
    want0 = torch.sqrt((maps[1:, 0].double() ** 2).sum(dim=(1, 2)))
    report("map_distances den = 0", (t[0] - want0).abs(), (2 * 36 + 8) * U * want0)
    assert bool((t[:, 1] == 0).all())
    assert bool(torch.isnan(t[1, 2])) and float(t[1, 3]) == float("inf") and bool(torch.isfinite(t[1, :2]).all())
    report("map_distances class 2", (t[2] - ref[2]).abs(), (2 * 36 + 8) * U * ref[2])
    maps[0, 2, 1, 1] = float("nan")
    K.map_distances(maps.cuda(), terms, 0)
    assert bool(torch.isnan(terms[2]).all()) and bool(torch.isfinite(terms[0]).all())
    score = K.sensitivity_finish(terms)
    assert bool(torch.isnan(score[1:]).all()) and float(score[0]) == float(terms[0].max())


# ------------------------------------------------------------------------------------------------ 5: the finish kernels
def finish_reference(dots, deltas):
    """float64 (raw, normalized, beta, their three bounds) from float64 dots / deltas [..., N] on the CPU, the sums in 80 bits"""
    d, y = dots.numpy().astype(np.longdouble), deltas.numpy().astype(np.longdouble)
    N = d.shape[-1]
    raw = ((d - y) ** 2).sum(-1) / N
    sdd, sdy, sady = (d * d).sum(-1), (d * y).sum(-1), np.abs(d * y).sum(-1)
    safe = np.where(sdd == 0, np.longdouble(1), sdd)
    beta = np.where(sdd == 0, np.longdouble(0), sdy / safe)
    gap = beta[..., None] * d - y
    norm = (gap ** 2).sum(-1) / N
    db = np.where(sdd == 0, np.longdouble(0), (N + 1) * U * sady / safe + (N + 2) * U * np.abs(beta))
    dgap = (db[..., None] * np.abs(d) + U * np.abs(gap)) * (1 + 2 * U)
    moved = (dgap * (2 * np.abs(gap) + dgap)).sum(-1) / N
    dnorm = moved + (N + 3) * U * (norm + moved)
    f = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))                      # noqa: E731
    return f(raw), f(norm), f(beta), 2 * (N + 3) * U * f(raw), 2 * f(dnorm), 2 * f(db)


def check_finish(what, dots, deltas, raw, normalized, beta):
    """the three scores against the definition restated in float64 over the given per-sample arrays"""
    rr, rn, rb, br, bn, bb = finish_reference(dots.cpu(), deltas.cpu())
    report(what + " raw", (raw.cpu() - rr).abs(), br)
    report(what + " normalized", (normalized.cpu() - rn).abs(), bn)
    report(what + " beta", (beta.cpu() - rb).abs(), bb)


@pytest.mark.parametrize("lead,N", [((1,), 1), ((2, 3), 7), ((5,), 50), ((300,), 3)], ids=["R1_N1", "R2x3_N7", "R5_N50", "R300_N3"])
def test_infidelity_finish_against_fp64(lead, N):
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(9900 + N)
    dots = torch.randn(lead + (N,), generator=gen, dtype=torch.float64)
    deltas = 0.7 * dots + 0.2 * torch.randn(lead + (N,), generator=gen, dtype=torch.float64)
    if len(lead) == 2:
        dots[1, 2] = 0.0                                                                 # sum dot^2 = 0: beta = 0, normalized = raw
    raw, normalized, beta = K.infidelity_finish(dots.cuda(), deltas.cuda())
    torch.cuda.synchronize()
    assert all(t.dtype == torch.float64 and tuple(t.shape) == lead and t.is_cuda for t in (raw, normalized, beta))
    check_finish("infidelity_finish %s N %d" % (lead, N), dots, deltas, raw, normalized, beta)
    assert bool((normalized <= raw * (1 + (4 * N + 16) * U)).all())
    if len(lead) == 2:
        assert float(beta[1, 2]) == 0.0 and float(normalized[1, 2]) == float(raw[1, 2])
        report("zero dots: raw = mean delta^2", (raw[1, 2].cpu() - (deltas[1, 2] ** 2).mean()).abs(), 2 * (N + 3) * U * raw[1, 2].cpu())
    longer = [torch.full((lead[0] + 1,) + lead[1:], SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3)]
    outs = tuple(t[:lead[0]] for t in longer)                                            # leading slices: a row of sentinels behind each
    got = K.infidelity_finish(dots.cuda(), deltas.cuda(), out=outs)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, outs)) and all(bool((t[lead[0]:] == SENTINEL).all()) for t in longer)
    assert torch.equal(outs[0], raw) and torch.equal(outs[1], normalized) and torch.equal(outs[2], beta)


@pytest.mark.parametrize("lead,N", [((1,), 1), ((2, 3), 7), ((300,), 3)], ids=["R1_N1", "R2x3_N7", "R300_N3"])
def test_sensitivity_finish_is_the_maximum(lead, N):
    from scouter_amd import kernels as K
    terms = torch.rand(lead + (N,), generator=torch.Generator().manual_seed(9950 + N), dtype=torch.float64)
    if len(lead) == 2:
        terms[0, 1, N - 1] = float("nan")                                                # the last term
        terms[1, 0, 0] = float("nan")                                                    # the first
        terms[1, 1, 3] = float("inf")
    score = K.sensitivity_finish(terms.cuda())
    longer = torch.full((lead[0] + 1,) + lead[1:], SENTINEL, dtype=torch.float64, device="cuda")
    into = K.sensitivity_finish(terms.cuda(), out=longer[:lead[0]])
    torch.cuda.synchronize()
    assert bool((longer[lead[0]:] == SENTINEL).all())
    want = terms.max(dim=-1).values                                                      # (torch's max propagates NaN)
    assert score.dtype == torch.float64 and tuple(score.shape) == lead
    assert torch.equal(torch.nan_to_num(score.cpu(), nan=-1.0), torch.nan_to_num(want, nan=-1.0)) and torch.equal(
        torch.isnan(score.cpu()), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(into, nan=-1.0), torch.nan_to_num(score, nan=-1.0))
    if len(lead) == 2:
        assert bool(torch.isnan(score[0, 1])) and bool(torch.isnan(score[1, 0])) and float(score[1, 1]) == float("inf")


# ------------------------------------------------------------------------------------------------ 6: refusals
BAD = {"perturb_dots": ["null", "n0", "past_N", "first_low", "misaligned", "small_ws", "sigma", "form", "attr_rank", "dots_shape"],
       "uniform_images": ["null", "n0", "past_N", "misaligned", "radius", "out_shape", "grid"],
       "output_deltas": ["null", "n0", "past_N", "misaligned", "of", "deltas_shape"],
       "map_distances": ["null", "n0", "past_N", "misaligned", "terms_shape"],
       "infidelity_finish": ["null", "n0", "misaligned", "shape"],
       "sensitivity_finish": ["null", "n0", "misaligned", "out_shape"]}


@pytest.mark.parametrize("call,bad", [(c, b) for c in BAD for b in BAD[c]])
def test_fidelity_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, n = 0, a chunk past N (past 2^31 samples for uniform_images, which has no N), a negative first, a
    misaligned pointer, a workspace that is too small, a negative sigma / radius, more samples than a grid holds, attributions
    that are neither the image's size nor a divisor of it, a wrong shape through the wrapper, of = 2: a RuntimeError naming the
    call, the outputs untouched, and a good call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    shape, n, N, Kc = (2, 6, 6), 4, 6, 2
    E = int(np.prod(shape))
    image = torch.ones(shape, device="cuda")
    attrs = torch.ones((Kc,) + shape, device="cuda")
    out = torch.full((n,) + shape, SENTINEL, device="cuda")
    dots, other = per_sample(Kc, N), per_sample(Kc, N)
    logp = torch.zeros((1 + n, 5), device="cuda")
    cols = torch.zeros(Kc, dtype=torch.int32, device="cuda")
    maps = torch.ones((1 + n, Kc, 3, 3), device="cuda")
    res = [torch.full((Kc,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    lib = _native.lib()
    first = {"past_N": N - n + 1, "first_low": -1}.get(bad, 1)
    with pytest.raises(RuntimeError, match=call):
        if call == "perturb_dots":
            good = [attrs.data_ptr(), dots.data_ptr(), 1.0, 0, 0, 1, n, N, Kc, E, E, ws.data_ptr(), ws.numel(), None]
            if bad == "null":
                _native.check(lib.scouter_perturb_dots_f64(*(good[:1] + [None] + good[2:])), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_perturb_dots_f64(*(good[:1] + [dots.data_ptr() + 4] + good[2:])), call)
            elif bad == "small_ws":
                assert lib.scouter_perturb_dots_workspace_bytes(n, Kc, E) == 8 * n * Kc
                _native.check(lib.scouter_perturb_dots_f64(*(good[:12] + [8 * n * Kc - 1, None])), call)
            elif bad == "form":
                _native.check(lib.scouter_perturb_dots_f64(*(good[:10] + [E - 1] + good[11:])), call)          # 71 does not divide 72
            elif bad == "n0":
                K.perturb_dots(attrs, dots, 1.0, 0, first, 0)
            elif bad == "sigma":
                K.perturb_dots(attrs, dots, -0.5, 0, first, n)
            elif bad == "attr_rank":
                K.perturb_dots(attrs[:, 0].contiguous(), dots, 1.0, 0, first, n)                               # maps without channels=
            elif bad == "dots_shape":
                K.perturb_dots(attrs, dots[:1], 1.0, 0, first, n)
            else:
                K.perturb_dots(attrs, dots, 1.0, 0, first, n)
        elif call == "uniform_images":
            if bad == "null":
                _native.check(lib.scouter_uniform_images_f32(None, out.data_ptr(), 1.0, 0, 0, 0, n, E, None), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_uniform_images_f32(image.data_ptr(), out.data_ptr() + 2, 1.0, 0, 0, 0, n, E, None), call)
            elif bad == "n0":
                K.uniform_images(image, out[:0], 1.0, 0, 0)
            elif bad == "past_N":
                K.uniform_images(image, out, 1.0, 0, 2 ** 31 - n + 1)
            elif bad == "radius":
                K.uniform_images(image, out, -0.5, 0, 0)
            elif bad == "grid":                                                          # one sample tile more than a grid holds
                many = torch.full((65535 * IT + 1, 1), SENTINEL, device="cuda")
                try:
                    K.uniform_images(image.view(-1)[:1], many, 1.0, 0, 0)
                finally:
                    assert bool((many == SENTINEL).all())
            else:
                K.uniform_images(image, out.view(n, shape[0], -1), 1.0, 0, 0)
        elif call == "output_deltas":
            good = [logp.data_ptr(), cols.data_ptr(), dots.data_ptr(), 1, n, N, Kc, 5, 0, None]
            if bad == "null":
                _native.check(lib.scouter_output_deltas_f64(*(good[:1] + [None] + good[2:])), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_output_deltas_f64(*(good[:2] + [dots.data_ptr() + 4] + good[3:])), call)
            elif bad == "of":
                _native.check(lib.scouter_output_deltas_f64(*(good[:8] + [2, None])), call)
            elif bad == "n0":
                K.output_deltas(logp[:1], cols, dots, first)
            elif bad == "deltas_shape":
                K.output_deltas(logp, cols, dots[:1], first)
            else:
                K.output_deltas(logp, cols, dots, first)
        elif call == "map_distances":
            if bad == "null":
                _native.check(lib.scouter_map_distances_f64(maps.data_ptr(), None, 1, n, N, Kc, 9, None), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_map_distances_f64(maps.data_ptr() + 2, dots.data_ptr(), 1, n, N, Kc, 9, None), call)
            elif bad == "n0":
                K.map_distances(maps[:1], dots, first)
            elif bad == "terms_shape":
                K.map_distances(maps, dots[:1], first)
            else:
                K.map_distances(maps, dots, first)
        elif call == "infidelity_finish":
            if bad == "null":
                _native.check(lib.scouter_infidelity_finish_f64(dots.data_ptr(), other.data_ptr(), res[0].data_ptr(), None,
                                                                res[2].data_ptr(), Kc, N, None), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_infidelity_finish_f64(dots.data_ptr(), other.data_ptr() + 4, res[0].data_ptr(),
                                                                res[1].data_ptr(), res[2].data_ptr(), Kc, N, None), call)
            elif bad == "n0":
                K.infidelity_finish(dots[:, :0], other[:, :0], out=tuple(res))
            else:
                K.infidelity_finish(dots, other[:, :3], out=tuple(res))
        else:
            if bad == "null":
                _native.check(lib.scouter_sensitivity_finish_f64(None, res[0].data_ptr(), Kc, N, None), call)
            elif bad == "misaligned":
                _native.check(lib.scouter_sensitivity_finish_f64(dots.data_ptr() + 4, res[0].data_ptr(), Kc, N, None), call)
            elif bad == "n0":
                K.sensitivity_finish(dots[:, :0], out=res[0])
            else:
                K.sensitivity_finish(dots, out=res[1][:1])
    torch.cuda.synchronize()
    for t in [out, dots, other] + res:
        assert bool((t == SENTINEL).all())
    test_perturb_dots_against_fp64(CASES[0][0], CASES[0][1], KT + 1, JT + 1)
    test_map_distances_against_fp64(3, 5, (7, 7))


def test_output_deltas_refuses_a_bad_of_through_the_wrapper():
    from scouter_amd import kernels as K
    with pytest.raises(ValueError, match="of must be"):
        K.output_deltas(torch.zeros((3, 5), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), per_sample(1, 2), 0, "logit")


# ------------------------------------------------------------------------------------------------ 7: a linear black box
class Linear(torch.nn.Module):
    """out[n, c] = fl32(sum_e W[c, e] x[n, e] + b[c]) with the sum in float64, one row at a time (so a row's bits do not depend on
    the batch it rides in); records every batch it is given and what it answered"""

    def __init__(self, W, b):
        super().__init__()
        self.Wt = torch.nn.Parameter(W.double().t().contiguous())                        # (a parameter: no .grad may appear)
        self.register_buffer("b", b.double())
        self.seen = []

    def forward(self, x):
        rows = x.detach().flatten(1).double()
        out = torch.stack([(r[:, None] * self.Wt).sum(dim=0) + self.b for r in rows]).float()
        self.seen.append((x.detach().clone(), out.clone()))
        return out


SHAPE, NCLS = (3, 8, 8), 5


@functools.lru_cache(maxsize=None)
def linear_inputs():
    gen = torch.Generator().manual_seed(9990)
    E = int(np.prod(SHAPE))
    x = torch.randn((2,) + SHAPE, generator=gen)
    W = torch.randn((NCLS, E), generator=gen)
    Wm = torch.randn((NCLS,) + SHAPE[1:], generator=gen)                                 # a W that is constant over the channels
    b = torch.randn(NCLS, generator=gen)
    return x, W, Wm, b


def run_linear(W, b, attributions, classes, **kw):
    """(scores, the recorded (batch, output) pairs of the stream, the model): the probe that counts the outputs is dropped"""
    from scouter_amd.tools.attribution import infidelity
    x = linear_inputs()[0].cuda()
    model = Linear(W, b).cuda()
    model.train()
    r = infidelity(model, x, attributions, classes=classes, **kw)
    torch.cuda.synchronize()
    assert model.training and all(p.grad is None for p in model.parameters()) and x.grad is None
    assert tuple(model.seen[0][0].shape) == (1,) + SHAPE                                 # the probe: one image, before the stream
    return r, model.seen[1:], model


def restate_linear(r, seen, full_attrs, cols, N, sigma, seed, batch, of="log_prob"):
    """every field of InfidelityScores against the definition restated in float64 over the recorded outputs and the noise_images
    bits; returns (dots, deltas, |W| |x_j| per sample) references for the caller's own bounds.  full_attrs [B, K, E] on the CPU"""
    x = linear_inputs()[0]
    B, Kc = full_attrs.shape[:2]
    E = int(np.prod(SHAPE))
    z = noise_bits(SHAPE, 0, N, seed)
    seen = list(seen)
    for b in range(B):
        ref, mag = dots_reference(full_attrs[b].numpy(), z, sigma)
        report("infidelity dots image %d" % b, (r.dots[b].cpu() - ref).abs(), 2 * E * U * mag)
        for first in range(0, N, batch - 1):
            m = min(batch - 1, N - first)
            xin, out = seen.pop(0)
            assert tuple(xin.shape) == (1 + m,) + SHAPE and torch.equal(xin[0].cpu(), x[b])      # the clean image rides in row 0
            want = torch.from_numpy(z[first:first + m]).view((m,) + SHAPE)
            got = xin[1:].cpu().double()
            ref_x = x[b].double()[None] + float(np.float32(sigma)) * want
            report("the perturbed rows", (got - ref_x).abs(), 2 * EPS * ref_x.abs())
            o = out.cpu().double()[:, cols]
            if of == "prob":
                o = torch.exp(o)
                bound = 2 * (4 * U * (o[:1] + o[1:]).t() + U * (o[:1] - o[1:]).t().abs())
            else:
                bound = 2 * U * (o[:1] - o[1:]).t().abs()
            report("infidelity deltas image %d chunk %d" % (b, first), (r.deltas[b, :, first:first + m].cpu() - (o[:1] - o[1:]).t()).abs(),
                   bound)
    assert not seen
    check_finish("infidelity", r.dots, r.deltas, r.raw, r.normalized, r.beta)
    for t in (r.raw, r.normalized, r.beta):
        assert t.dtype == torch.float64 and tuple(t.shape) == (B, Kc) and t.is_cuda
    assert tuple(r.dots.shape) == (B, Kc, N) and tuple(r.deltas.shape) == (B, Kc, N)
    return z


def test_infidelity_on_a_linear_black_box():
    from scouter_amd.tools.attribution import infidelity
    x, W, Wm, b = linear_inputs()
    E, N, sigma, seed, batch = int(np.prod(SHAPE)), 50, 0.05, 7, 51
    cols = [0, 3, 4]
    kw = dict(n_samples=N, sigma=sigma, seed=seed, batch=batch)
    a = W[cols].view((1, len(cols)) + SHAPE).expand((2, len(cols)) + SHAPE).contiguous()
    # ---- a = W: the attribution of a linear model is its weights
    r, seen, model = run_linear(W, b, a.cuda(), cols, **kw)
    z = restate_linear(r, seen, a.view(2, len(cols), E), cols, N, sigma, seed, batch)
    s32 = float(np.float32(sigma))
    W64, absW = W.double()[cols], W.double()[cols].abs()
    for bi in range(2):
        xj = seen[bi][0].cpu().double().view(1 + N, E)                                   # (batch 51: one forward per image)
        out = seen[bi][1].cpu().double()[:, cols]
        S = absW @ (s32 * torch.from_numpy(np.abs(z))).t()                               # [K, N]
        g = (EPS + U) * (out[:1].abs().t() + out[1:].abs().t()) + EPS * (absW @ xj[1:].abs().t()) \
            + 2 * (E + 1) * U * (absW @ (xj[:1].abs() + xj[1:].abs()).t() + b.double()[cols].abs()[:, None]) + E * U * S
        dots, deltas = r.dots[bi].cpu(), r.deltas[bi].cpu()
        report("a = W image %d: |dot - delta|" % bi, (dots - deltas).abs(), 2 * g)
        print("a = W image %d: raw %s, bound %s" % (bi, r.raw[bi].tolist(), (2 * (g * g).mean(dim=1)).tolist()))
        assert bool((r.raw[bi].cpu() <= 2 * (g * g).mean(dim=1)).all())
        db = 2 * ((dots.abs() * g).sum(dim=1) / (dots * dots).sum(dim=1)) + finish_reference(dots, deltas)[5]
        report("a = W image %d: |beta - 1|" % bi, (r.beta[bi].cpu() - 1.0).abs(), db)
        assert bool((r.normalized[bi] <= r.raw[bi] * (1 + (4 * N + 16) * U)).all())
    # ---- a = 2 W: beta halves, normalized does not move, raw is the mean of delta^2 up to the same roundings
    r2, seen2, _ = run_linear(W, b, (2 * a).cuda(), cols, **kw)
    restate_linear(r2, seen2, (2 * a).view(2, len(cols), E), cols, N, sigma, seed, batch)
    assert torch.equal(r2.deltas, r.deltas) and torch.equal(r2.dots, 2 * r.dots)         # powers of two move no bit
    assert torch.equal(r2.beta, r.beta / 2) and torch.equal(r2.normalized, r.normalized)
    for bi in range(2):
        deltas = r.deltas[bi].cpu()
        gap = (r.dots[bi].cpu() - deltas).abs()                                          # (|dot - delta| <= g, shown above)
        mean_sq = (deltas * deltas).mean(dim=1)
        report("a = 2 W image %d: raw against mean delta^2" % bi, (r2.raw[bi].cpu() - mean_sq).abs(),
               2 * ((4 * deltas.abs() * gap + 4 * gap * gap).mean(dim=1) + (N + 3) * U * mean_sq))
    # ---- a = 0
    r0, seen0, _ = run_linear(W, b, torch.zeros_like(a).cuda(), cols, **kw)
    restate_linear(r0, seen0, torch.zeros_like(a).view(2, len(cols), E), cols, N, sigma, seed, batch)
    mean_sq = (r0.deltas.cpu() ** 2).mean(dim=2)
    assert bool((r0.dots == 0).all()) and bool((r0.beta == 0).all()) and torch.equal(r0.raw, r0.normalized)
    assert torch.equal(r0.deltas, r.deltas)
    report("a = 0: raw against mean delta^2", (r0.raw.cpu() - mean_sq).abs(), 2 * (N + 3) * U * mean_sq)
    # ---- the chunking moves no bit of dots; for this row-independent box no bit of anything
    r4, seen4, _ = run_linear(W, b, a.cuda(), cols, **{**kw, "batch": 4})
    restate_linear(r4, seen4, a.view(2, len(cols), E), cols, N, sigma, seed, 4)
    assert len(seen4) == 2 * 17 and tuple(seen4[16][0].shape) == (3,) + SHAPE            # 16 chunks of 3 samples and one of 2
    for f in r._fields:
        assert torch.equal(getattr(r4, f), getattr(r, f)), f
    # ---- two calls give the same bits; another seed gives other noise; per-image classes are the list's columns
    again, _, _ = run_linear(W, b, a.cuda(), cols, **kw)
    assert all(torch.equal(getattr(again, f), getattr(r, f)) for f in r._fields)
    other, _, _ = run_linear(W, b, a.cuda(), cols, **{**kw, "seed": seed + 1})
    assert not torch.equal(other.dots, r.dots)
    own, seen_own, _ = run_linear(W, b, torch.stack([a[0, 2:3], a[1, 0:1]]).cuda(), torch.tensor([4, 0]), **kw)
    assert torch.equal(own.dots[0, 0], r.dots[0, 2]) and torch.equal(own.dots[1, 0], r.dots[1, 0])
    assert torch.equal(own.deltas[0, 0], r.deltas[0, 2]) and torch.equal(own.raw[1, 0], r.raw[1, 0])
    # ---- classes=None: one attribution per output
    every = W.view((1, NCLS) + SHAPE).expand((2, NCLS) + SHAPE).contiguous()
    rn, _, _ = run_linear(W, b, every.cuda(), None, **kw)
    assert torch.equal(rn.dots[:, cols], r.dots) and torch.equal(rn.beta[:, cols], r.beta)
    # ---- of = "prob"
    rp, seenp, _ = run_linear(W, b, a.cuda(), cols, **{**kw, "of": "prob"})
    restate_linear(rp, seenp, a.view(2, len(cols), E), cols, N, sigma, seed, batch, of="prob")
    assert torch.equal(rp.dots, r.dots) and not torch.equal(rp.deltas, r.deltas)
    # ---- argument errors
    xd = x.cuda()
    for bad in ([NCLS], [-1], torch.tensor([0, NCLS])):
        with pytest.raises(IndexError):
            infidelity(model, xd, a[:, :1].cuda(), classes=bad, **kw)
    for kwargs in (dict(batch=1), dict(of="logit"), dict(n_samples=0), dict(sigma=-1.0), dict(classes=[0, 1]), dict(classes=None),
                   dict(classes=torch.tensor([0, 1]))):
        with pytest.raises(ValueError):
            infidelity(model, xd, a.cuda(), **{**dict(classes=cols), **kw, **kwargs})
    assert model.training


def test_infidelity_map_form_on_a_linear_black_box():
    """a W that is constant over the channels: its [h, w] map scores as the full attribution does, bit for bit; a coarse map is
    resized by kernels.resize_bilinear first; uint8 maps count as their float values"""
    from scouter_amd import kernels as K
    x, _, Wm, b = linear_inputs()
    E, N, sigma, seed, batch = int(np.prod(SHAPE)), 9, 0.05, 3, 4
    cols = [1, 2]
    kw = dict(n_samples=N, sigma=sigma, seed=seed, batch=batch)
    Wfull = Wm[:, None].expand((NCLS,) + SHAPE).reshape(NCLS, E).contiguous()
    maps = Wm[cols][None].expand((2, 2) + SHAPE[1:]).contiguous()
    full = maps[:, :, None].expand((2, 2) + SHAPE).contiguous()
    rm, seenm, _ = run_linear(Wfull, b, maps.cuda(), cols, **kw)
    rf, _, _ = run_linear(Wfull, b, full.cuda(), cols, **kw)
    restate_linear(rm, seenm, full.view(2, 2, E), cols, N, sigma, seed, batch)
    for f in rm._fields:
        assert torch.equal(getattr(rm, f), getattr(rf, f)), f
    # a coarse map: the definition over the resized map
    coarse = torch.randn((2, 2, 4, 4), generator=torch.Generator().manual_seed(5))
    rc, seenc, _ = run_linear(Wfull, b, coarse.cuda(), cols, **kw)
    resized = K.resize_bilinear(coarse.cuda(), SHAPE[1], SHAPE[2]).cpu()
    restate_linear(rc, seenc, resized[:, :, None].expand((2, 2) + SHAPE).reshape(2, 2, E), cols, N, sigma, seed, batch)
    # uint8 maps
    bytes_ = (torch.rand((2, 2) + SHAPE[1:], generator=torch.Generator().manual_seed(6)) * 255).to(torch.uint8)
    ru, _, _ = run_linear(Wfull, b, bytes_.cuda(), cols, **kw)
    rff, _, _ = run_linear(Wfull, b, bytes_.float().cuda(), cols, **kw)
    assert all(torch.equal(getattr(ru, f), getattr(rff, f)) for f in ru._fields)


# ------------------------------------------------------------------------------------------------ 8: stub explainers
def uniform_bits(image, N, radius, seed):
    from scouter_amd import kernels as K
    out = torch.empty((N,) + tuple(image.shape), device="cuda")
    K.uniform_images(image, out, radius, seed, 0)
    return out


def test_sensitivity_max_on_stub_explainers():
    from scouter_amd.tools.attribution import sensitivity_max
    x = linear_inputs()[0].cuda()
    E, N, radius, seed, s = int(np.prod(SHAPE)), 7, 0.1, 11, 2.0
    seen = []

    def scaled(im):
        seen.append(im.detach().clone())
        return (im * s)[:, None]

    r = sensitivity_max(scaled, x, n_samples=N, radius=radius, batch=4, seed=seed)
    torch.cuda.synchronize()
    assert r.score.dtype == torch.float64 and tuple(r.score.shape) == (2, 1) and tuple(r.terms.shape) == (2, 1, N) and r.score.is_cuda
    assert [tuple(t.shape) for t in seen] == [(4,) + SHAPE, (4,) + SHAPE, (2,) + SHAPE] * 2          # 3, 3 and 1 samples behind row 0
    for b in range(2):
        xj = uniform_bits(x[b], N, radius, seed).cpu().double().view(N, E)                           # uniform_images' own output
        x64 = x[b].cpu().double().view(1, E)
        rows = torch.cat([t[1:] for t in seen[3 * b:3 * b + 3]]).cpu().double().view(N, E)
        assert torch.equal(rows, xj) and all(torch.equal(t[0], x[b]) for t in seen[3 * b:3 * b + 3])
        want = torch.sqrt(((s * xj - s * x64) ** 2).sum(dim=1) / ((s * x64) ** 2).sum())             # s = 2: the products are exact
        report("sensitivity terms image %d" % b, (r.terms[b, 0].cpu() - want).abs(), (2 * E + 8) * U * want)
        assert float(r.score[b, 0]) == float(r.terms[b, 0].max())
        # ... which is radius |d_j| / |x| up to the rounding of x_j = fma(radius, d_j, x)
        d = torch.from_numpy(np.stack([uniform_fp64(seed, j, E) for j in range(N)]))
        ideal = float(np.float32(radius)) * torch.sqrt((d * d).sum(dim=1)) / torch.sqrt((x64 * x64).sum())
        slack = 2 * EPS * torch.sqrt((xj * xj).sum(dim=1)) / torch.sqrt((x64 * x64).sum()) + (2 * E + 8) * U * want
        report("sensitivity terms image %d against radius |d| / |x|" % b, (r.terms[b, 0].cpu() - ideal).abs(), slack)
    # the chunking moves no bit (the explainer treats every row alone); two calls agree; another seed does not
    wide = sensitivity_max(lambda im: (im * s)[:, None], x, n_samples=N, radius=radius, batch=11, seed=seed)
    assert torch.equal(wide.terms, r.terms) and torch.equal(wide.score, r.score)
    assert not torch.equal(sensitivity_max(lambda im: (im * s)[:, None], x, n_samples=N, radius=radius, batch=11, seed=seed + 1).terms,
                           r.terms)
    # a constant explanation does not move; a zero one scores 0 through den = 1
    const = sensitivity_max(lambda im: torch.ones((im.shape[0], 2, 3, 3), device="cuda"), x, n_samples=N, batch=3)
    assert tuple(const.score.shape) == (2, 2) and bool((const.score == 0).all()) and bool((const.terms == 0).all())
    zero = sensitivity_max(lambda im: torch.zeros((im.shape[0], 2, 3, 3), device="cuda"), x, n_samples=N, batch=3)
    assert bool((zero.score == 0).all())
    # ... and den = 1 shows when only the clean image's explanation is zero: sqrt(9 * 1 / 1)
    def clean_zero(im):
        a = torch.ones((im.shape[0], 2, 3, 3), device="cuda")
        a[0] = 0.0
        return a
    assert bool((sensitivity_max(clean_zero, x, n_samples=N, batch=3).terms == 3.0).all())
    # a NaN for one sample
    def one_nan(im):
        a = (im * s)[:, None].clone()
        if a.shape[0] == 4:
            a[2, 0, 1, 2, 3] = float("nan")
        return a
    nan = sensitivity_max(one_nan, x, n_samples=N, radius=radius, batch=4, seed=seed)
    assert bool(torch.isnan(nan.score).all()) and int(torch.isnan(nan.terms).sum()) == 2 * 2        # sample 1 of each full chunk
    assert torch.equal(torch.nan_to_num(nan.terms, nan=0.0)[:, :, [0, 2, 3, 5, 6]], r.terms[:, :, [0, 2, 3, 5, 6]])
    # a shape that changes between calls, a result that is not fp32, not on the device or of the wrong length
    calls = []
    def changing(im):
        calls.append(1)
        return torch.ones((im.shape[0], 1, 3, 3 + (len(calls) > 1)), device="cuda")
    with pytest.raises(ValueError, match="shape"):
        sensitivity_max(changing, x, n_samples=N, batch=3)
    for bad in (lambda im: torch.ones((im.shape[0], 1, 3), dtype=torch.float64, device="cuda"),
                lambda im: torch.ones((im.shape[0], 1, 3)), lambda im: torch.ones((im.shape[0] - 1, 1, 3), device="cuda"),
                lambda im: torch.ones((im.shape[0],), device="cuda"), lambda im: None):
        with pytest.raises(ValueError):
            sensitivity_max(bad, x, n_samples=N, batch=3)
    for kwargs in (dict(batch=1), dict(n_samples=0), dict(radius=-1.0)):
        with pytest.raises(ValueError):
            sensitivity_max(lambda im: (im * s)[:, None], x, **kwargs)


# ------------------------------------------------------------------------------------------------ 9: whole models
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


def restate_model(r, seen, full_attrs, images, cols, N, sigma, seed, batch):
    """InfidelityScores of a whole model against the definition over the path's own recorded outputs: full_attrs [B, K, E] (CPU)"""
    shape = tuple(images.shape[1:])
    E = int(np.prod(shape))
    z = noise_bits(shape, 0, N, seed)
    seen = list(seen)
    for b in range(images.shape[0]):
        ref, mag = dots_reference(full_attrs[b].numpy(), z, sigma)
        report("model dots image %d" % b, (r.dots[b].cpu() - ref).abs(), 2 * E * U * mag)
        for first in range(0, N, batch - 1):
            m = min(batch - 1, N - first)
            xin, out = seen.pop(0)
            assert tuple(xin.shape) == (1 + m,) + shape and torch.equal(xin[0], images[b])
            o = out.cpu().double()[:, cols]
            want = (o[:1] - o[1:]).t()
            report("model deltas image %d chunk %d" % (b, first), (r.deltas[b, :, first:first + m].cpu() - want).abs(), 2 * U * want.abs())
    assert not seen
    check_finish("model infidelity", r.dots, r.deltas, r.raw, r.normalized, r.beta)
    assert bool(torch.isfinite(r.raw).all()) and bool(torch.isfinite(r.normalized).all()) and bool(torch.isfinite(r.beta).all())
    assert bool((r.deltas != 0).any()) and bool((r.normalized <= r.raw * (1 + (4 * N + 16) * U)).all())


@pytest.mark.parametrize("fold", [False, True], ids=["unfolded", "folded"])
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_infidelity_and_sensitivity_on_whole_models(use_slot, fold):
    """resnet18 / MNIST stem / 64^2 / batch 2, classes [0, 3]: infidelity (5 samples in chunks of 2, 2, 1) of the gradcam map and of
    the input_gradients attribution, sensitivity_max (4 samples in chunks of 2) of gradcam, against the definitions restated over
    the outputs and maps recorded while the tools ran"""
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import gradcam, infidelity, input_gradients, sensitivity_max
    m, images = build(use_slot)
    m.set_inference_fold(fold)
    cols, N, sigma, seed, batch = [0, 3], 5, 0.05, 5, 3
    E = 64 * 64
    m.train()
    cam = gradcam(m, images, classes=cols)
    grads = input_gradients(m, images, classes=cols)
    before = bn_buffers(m)
    seen = []
    hook = m.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].detach().clone(), out.detach().clone())))
    try:
        rc = infidelity(m, images, cam, classes=cols, n_samples=N, sigma=sigma, batch=batch, seed=seed)
        torch.cuda.synchronize()
        seen_cam, seen[:] = list(seen), []
        rg = infidelity(m, images, grads, classes=cols, n_samples=N, sigma=sigma, batch=batch, seed=seed)
        torch.cuda.synchronize()
        seen_grad, seen[:] = list(seen), []
    finally:
        hook.remove()
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    resized = K.resize_bilinear(cam, 64, 64).cpu()                                       # the path's own resized map; C = 1
    restate_model(rc, seen_cam, resized.view(2, 2, E), images, cols, N, sigma, seed, batch)
    restate_model(rg, seen_grad, grads.cpu().view(2, 2, E), images, cols, N, sigma, seed, batch)
    assert torch.equal(rc.deltas, rg.deltas)                                             # the same forwards: the same bits
    print("infidelity %s fold %s: cam raw %s normalized %s; grad raw %s normalized %s beta %s" % (
        "slot" if use_slot else "fc", fold, rc.raw.tolist(), rc.normalized.tolist(), rg.raw.tolist(), rg.normalized.tolist(),
        rg.beta.tolist()))
    again = infidelity(m, images, cam, classes=cols, n_samples=N, sigma=sigma, batch=batch, seed=seed)
    assert all(torch.equal(getattr(again, f), getattr(rc, f)) for f in rc._fields)
    wide = infidelity(m, images, cam, classes=cols, n_samples=N, sigma=sigma, batch=N + 1, seed=seed)
    assert torch.equal(wide.dots, rc.dots)                                               # the chunking moves no bit of dots
    # ---- sensitivity_max of gradcam
    maps = []

    def explain(im):
        a = gradcam(m, im, classes=cols)
        maps.append(a.detach().clone())
        return a

    Ns, radius = 4, 0.02
    rs = sensitivity_max(explain, images, n_samples=Ns, radius=radius, batch=3, seed=seed)
    torch.cuda.synchronize()
    assert tuple(rs.score.shape) == (2, 2) and tuple(rs.terms.shape) == (2, 2, Ns) and len(maps) == 4
    M = int(maps[0][0, 0].numel())
    for b in range(2):
        for i, first in enumerate((0, 2)):
            ref, _ = terms_reference(maps[2 * b + i].cpu())
            report("model sensitivity image %d chunk %d" % (b, first), (rs.terms[b, :, first:first + 2].cpu() - ref).abs(),
                   (2 * M + 8) * U * ref.abs())
    assert torch.equal(rs.score, rs.terms.max(dim=2).values) and bool(torch.isfinite(rs.score).all()) and bool((rs.score > 0).all())
    print("sensitivity_max gradcam %s fold %s: %s" % ("slot" if use_slot else "fc", fold, rs.score.tolist()))
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())
    m.set_inference_fold(False)


# ------------------------------------------------------------------------------------------------ 10: the test tool
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_fidelity_test_tool(use_slot, tmp_path, monkeypatch, capsys):
    """test.py --infidelity true --sensitivity true: one `infidelity <family> class <c>: raw <r> normalized <n> beta <b>` and one
    `sensitivity <family> class <c>: max <s>` line per family drawn in the call, every value finite"""
    from scouter_amd import test as T
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "true" if use_slot else "false", "--pre_trained", "false",
        "--img_size", "64", "--cam", "true", "--grad", "true", "--infidelity", "true", "--infidelity_samples", "5",
        "--infidelity_batch", "3", "--infidelity_sigma", "0.01", "--sensitivity", "true", "--sensitivity_samples", "3",
        "--sensitivity_batch", "3", "--vis_dir", str(tmp_path / "vis"), "--output_dir", str(tmp_path / "none")])
    T.main()
    text = capsys.readouterr().out.splitlines()
    families = (["slot"] if use_slot else []) + ["grad", "cam"]
    inf = [ln.split() for ln in text if ln.startswith("infidelity ")]
    sens = [ln.split() for ln in text if ln.startswith("sensitivity ")]
    assert [ln[1] for ln in inf] == families and [ln[1] for ln in sens] == families
    assert not [ln for ln in text if ln.startswith("causal ")]                          # --causal was not asked for
    classes = set()
    for ln in inf:
        assert ln[2] == "class" and ln[3].endswith(":") and (ln[4], ln[6], ln[8]) == ("raw", "normalized", "beta") and len(ln) == 10
        classes.add(int(ln[3][:-1]))
        raw, normalized, beta = float(ln[5]), float(ln[7]), float(ln[9])
        assert all(np.isfinite(v) for v in (raw, normalized, beta)) and 0.0 <= normalized <= raw * (1 + 1e-5)     # (six printed digits)
    for ln in sens:
        assert ln[2] == "class" and ln[3].endswith(":") and ln[4] == "max" and len(ln) == 6
        classes.add(int(ln[3][:-1]))
        assert np.isfinite(float(ln[5])) and float(ln[5]) >= 0.0
    assert len(classes) == 1 and 0 <= classes.pop() < 10                                # every family scores the predicted class
