"""GradientSHAP at the image and at the backbone's output (-m gpu): the three kernels of csrc/gradshap.hip -- the draws against the
NumPy restatement bit for bit, the rows against the two existing kernels they restate (noise_images, path_images) bit for bit, the
float64 sums against the restatement of tests/gradshap_restatements.py with a derived bound -- their refusals, the two methods of
tools/attribution.py on whole models -- against the definition over the HIP path's own gradients (the kernels' bounds), against the
CPU oracle under fp64 and fp32 autograd fed the same draws (the project's rule, tests/test_layer_gpu.py check_rule), the completeness
gap against its definition -- and scouter_amd/tools/gradshap.py in both modes.

Bounds.  u = 2^-53.  gradshap_accumulate adds n terms t inv_n, t an exact product, with one rounding per fma, onto acc0: within
(n + 2) u (|acc0| + sum|t inv_n|).  attr_finish rounds the sum to fp32 once: 2^-24 |ref| more.  The layer maps add a position's C
channels in float64 (csrc/layerattr.hip): (C + 2) u sum|terms| and one rounding to fp32, as tests/test_layer_gpu.py check_own has it.
The gap is formed in float64 from sums of fp32-rounded values and rounded to fp32 once: recomputed from the returned fp32
attribution it is within E 4 2^-24 max|attr| (the margin tests/test_pathgrad_gpu.py gives integrated_gradients' delta) plus
2^-23 |gap| for its own rounding."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gradshap_restatements as R                                           # noqa: E402
from test_layer_gpu import SENTINEL, U, bn_buffers, build, check_own, check_rule, dev, one_hot, oracle_parts, rand   # noqa: E402
from oracle import torch_oracle as O                                        # noqa: E402

EPS = 2.0 ** -24
BIG_SEED = 2 ** 40 + 7
GROUP = 256 * 4                             # the elements one workgroup covers (csrc/gradshap.hip GS_THREADS x 4)
SIZES = [1, 4, 5, 105, GROUP - 1, GROUP + 1, 2048, 5184]
CASES = [(E, off) for E in SIZES for off in (0, 1)]
CASE_IDS = ["E%d%s" % (E, "_off1" if off else "") for E, off in CASES]
REAL = [(7 * 7 * 2048, 0), (3 * 224 * 224, 0)]
# (n, R, first, seed, sigma): every value of the issue's lists, in both noise modes
COMBOS = [(1, 1, 0, 0, 0.0), (3, 3, 5, BIG_SEED, 0.5), (8, 10, 0, BIG_SEED, 0.0), (8, 3, 5, 0, 0.5), (3, 10, 0, 0, 0.5),
          (1, 3, 5, BIG_SEED, 0.0), (8, 1, 0, 0, 0.5)]
# gradshap_images tiles the rows by 8 (blockIdx.y) and gradshap_accumulate walks them in rounds of 64 samples, 8 rows at a time and
# a tail: n on both sides of either boundary, a second tile / round that is full and one that is not
LONG_COMBOS = [(9, 3, 0, 0, 0.5), (11, 3, 5, BIG_SEED, 0.0), (11, 10, 5, 0, 0.5), (65, 10, 5, BIG_SEED, 0.0), (70, 10, 5, 0, 0.0),
               (70, 3, 5, BIG_SEED, 0.5), (200, 10, 5, BIG_SEED, 0.5), (200, 3, 0, 0, 0.0)]
LONG_CASES = [(E, off) for E in (5, GROUP + 1, 2048) for off in (0, 1)]
LONG_IDS = ["E%d%s" % (E, "_off1" if off else "") for E, off in LONG_CASES]


def splits(n):
    """where a call is cut in two: the ends, the middle, and either side of the tile of 8 and of the round of 64"""
    return sorted({1, n // 2, n - 1, 8, 9, 64, 65} & set(range(1, n)))


def restated_rows(image, bank, sigma, seed, first, n):
    """the rows first .. first + n - 1 by the two EXISTING kernels, and their differences: x~_j = noise_images(image, sigma, seed,
    first + j) (sigma == 0: the image itself), row_j = path_images(x~_j, bank[pick_j], [alpha_j]), d_j = x~_j - bank[pick_j] in fp32
    -> (rows [n, E], diffs [n, E], picks) on the device"""
    from scouter_amd import kernels as K
    picks, alphas = R.draws(seed, first, n, bank.shape[0])
    ad = torch.from_numpy(alphas).cuda()
    rows, diffs = torch.empty((n,) + tuple(image.shape), device="cuda"), torch.empty((n,) + tuple(image.shape), device="cuda")
    for j in range(n):
        xt = image.clone()
        if sigma > 0:
            K.noise_images(image.clone(), xt[None], sigma, seed, first + j)
        b = bank[int(picks[j])].clone()
        K.path_images(xt, b, ad, rows[j:j + 1], j)
        diffs[j] = xt - b                                                   # one fp32 subtraction, IEEE: the kernel's
    return rows, diffs, picks


# ------------------------------------------------------------------------------------------------ 1: the draws
@pytest.mark.parametrize("seed", [0, BIG_SEED, 2 ** 64 - 1])
@pytest.mark.parametrize("Rn", [1, 3, 10, 2 ** 31 - 1])
def test_the_draws_equal_the_restatement(seed, Rn):
    from scouter_amd import _native
    from scouter_amd import kernels as K
    for n, first in ((1, 0), (3, 5), (8, 0), (300, 5)):                     # (300: more than one workgroup)
        want_p, want_a = R.draws(seed, first, n, Rn)
        pbuf = torch.full((1 + n + 4,), -5, dtype=torch.int32, device="cuda")
        picks, ptail = pbuf[1:1 + n], pbuf[1 + n:]
        alphas, atail = dev(torch.zeros(n), 1, 4)
        got_p, got_a = K.gradshap_draws(n, Rn, seed, first, picks=picks, alphas=alphas)
        torch.cuda.synchronize()
        assert got_p is picks and got_a is alphas and bool((atail == SENTINEL).all()) and bool((ptail == -5).all()) and int(pbuf[0]) == -5
        assert np.array_equal(picks.cpu().numpy(), want_p)
        assert np.array_equal(alphas.cpu().numpy().view(np.uint32), want_a.view(np.uint32))
        new_p, new_a = K.gradshap_draws(n, Rn, seed, first)                 # tensors of its own
        assert torch.equal(new_p, picks) and torch.equal(new_a, alphas)
        for m in {0, 1, n // 2, n}:                                         # a call split at `first + m` equals one call
            sp, sa = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda")
            K.gradshap_draws(m, Rn, seed, first, picks=sp[:m], alphas=sa[:m])
            K.gradshap_draws(n - m, Rn, seed, first + m, picks=sp[m:], alphas=sa[m:])
            assert torch.equal(sp, picks) and torch.equal(sa, alphas)
        # either output may be null
        lo, hi = K._seed_words(seed)
        only_p = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda")
        only_a = torch.full((n + 2,), SENTINEL, device="cuda")
        _native.check(_native.lib().scouter_gradshap_draws(only_p.data_ptr(), None, lo, hi, first, n, Rn, None), "gradshap_draws")
        _native.check(_native.lib().scouter_gradshap_draws(None, only_a.data_ptr(), lo, hi, first, n, Rn, None), "gradshap_draws")
        _native.check(_native.lib().scouter_gradshap_draws(None, None, lo, hi, first, n, Rn, None), "gradshap_draws")
        torch.cuda.synchronize()
        assert torch.equal(only_p[:n], picks) and torch.equal(only_a[:n], alphas)
        assert bool((only_p[n:] == -5).all()) and bool((only_a[n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 2: gradshap_images
def check_images(E, off, combos):
    from scouter_amd import kernels as K
    for n, Rn, first, seed, sigma in combos:
        image, bank = rand((E,), 10 + n), rand((Rn, E), 20 + Rn)
        image[0] = -0.0
        bank[0, -1] = -0.0
        xd, _ = dev(image, off)
        bd, _ = dev(bank, off)
        out, tail = dev(torch.zeros((n, E)), off, 8)
        assert (xd.data_ptr() % 16 != 0) == bool(off) and (out.data_ptr() % 16 != 0) == bool(off)
        assert K.gradshap_images(xd, bd, out, sigma, seed, first) is out
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all())
        want, _, _ = restated_rows(xd, bd, sigma, seed, first, n)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (E, off, n, Rn, first, seed, sigma)
        assert bool(torch.isfinite(out).all())
        # chunks written by separate calls equal one call, whatever the alignment of the chunk
        for m in splits(n):
            parts, ptail = dev(torch.zeros((n, E)), off, 8)
            K.gradshap_images(xd, bd, parts[:m], sigma, seed, first)
            K.gradshap_images(xd, bd, parts[m:], sigma, seed, first + m)
            assert torch.equal(parts.view(torch.int32), out.view(torch.int32)) and bool((ptail == SENTINEL).all())
        if sigma == 0.0 and Rn == 1:
            # no noise is drawn at sigma = 0: where the image IS the one baseline, d = +0.0 exactly and every row is b + alpha 0 = b
            # (b + 0.0 in IEEE terms: the -0.0 element comes out +0.0, as path_images gives it)
            same = bank.clone()
            same[0, :] = image
            sd, _ = dev(same, off)
            flat = K.gradshap_images(xd, sd, torch.empty_like(out), 0.0, seed, first)
            assert torch.equal(flat.view(torch.int32), (xd + 0.0)[None].expand(n, -1).contiguous().view(torch.int32))

@pytest.mark.parametrize("E,off", CASES, ids=CASE_IDS)
def test_gradshap_images_equal_the_two_kernels_they_restate(E, off):
    check_images(E, off, COMBOS)


@pytest.mark.parametrize("E,off", LONG_CASES, ids=LONG_IDS)
def test_gradshap_images_past_a_tile_of_rows(E, off):
    check_images(E, off, LONG_COMBOS)


@pytest.mark.parametrize("E,off", REAL, ids=["7x7x2048", "3x224x224"])
def test_gradshap_images_at_the_real_shapes(E, off):
    check_images(E, off, [(8, 10, 5, BIG_SEED, 0.5), (3, 3, 0, 0, 0.0), (70, 10, 5, 0, 0.5)])


# ------------------------------------------------------------------------------------------------ 3: gradshap_accumulate
def check_accumulate(E, off, combos, N=7):
    """inv_n = 1 / N, no power of two"""
    from scouter_amd import kernels as K
    inv_n = 1.0 / N
    for n, Rn, first, seed, sigma in combos:
        image, bank = rand((E,), 30 + n), rand((Rn, E), 40 + Rn)
        grads, acc0 = rand((n, E), 50 + n), rand((E,), 60 + n, torch.float64)
        if sigma == 0.0:                                                    # a -0.0 survives: -0.0 - (+0.0) = -0.0, times a positive
            image[0], bank[:, 0], grads[:, 0], acc0[0] = -0.0, 0.0, 1.0, -0.0   # gradient -0.0, added to -0.0
        xd, _ = dev(image, off)
        bd, _ = dev(bank, off)
        gd, _ = dev(grads, off)
        acc, tail = dev(acc0, off, 8)
        assert (gd.data_ptr() % 16 != 0) == bool(off) and (acc.data_ptr() % 16 != 0) == bool(off)
        _, diffs, _ = restated_rows(xd, bd, sigma, seed, first, n)
        ref, mag = R.accumulate(grads, diffs.cpu(), acc0, inv_n)
        assert K.gradshap_accumulate(gd, xd, bd, acc, sigma, seed, first, inv_n) is acc
        torch.cuda.synchronize()
        assert bool((tail == SENTINEL).all())
        got = acc.cpu()
        assert bool(torch.isfinite(got).all())
        err, bound = (got - ref).abs(), (n + 2) * U * mag
        print("gradshap_accumulate E %d off %d" % (E, off), (n, Rn, first, seed, sigma), "max err %.3e, max err / bound %.3f"
              % (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all())
        if sigma == 0.0:
            assert float(got[0]) == 0.0 and math.copysign(1.0, float(got[0])) == -1.0
        # a repeat, and calls over consecutive pieces: the same bits
        again, _ = dev(acc0, off)
        K.gradshap_accumulate(gd, xd, bd, again, sigma, seed, first, inv_n)
        assert torch.equal(again.view(torch.int64), acc.view(torch.int64))
        for m in splits(n):
            split, stail = dev(acc0, off, 8)
            K.gradshap_accumulate(gd[:m], xd, bd, split, sigma, seed, first, inv_n)
            K.gradshap_accumulate(gd[m:], xd, bd, split, sigma, seed, first + m, inv_n)
            assert torch.equal(split.view(torch.int64), acc.view(torch.int64)) and bool((stail == SENTINEL).all()), (E, off, n, m)
        # a NaN in a gradient row poisons exactly its own elements
        hit = sorted({0, E // 2, E - 1})
        bad = grads.clone()
        bad[n // 2, hit] = float("nan")
        bgd, _ = dev(bad, off)
        poisoned, _ = dev(acc0, off)
        K.gradshap_accumulate(bgd, xd, bd, poisoned, sigma, seed, first, inv_n)
        mask = torch.zeros(E, dtype=torch.bool)
        mask[hit] = True
        assert torch.equal(torch.isnan(poisoned).cpu(), mask)
        assert torch.equal(poisoned.cpu()[~mask], got[~mask])


@pytest.mark.parametrize("E,off", CASES, ids=CASE_IDS)
def test_gradshap_accumulate_against_fp64(E, off):
    check_accumulate(E, off, COMBOS)


@pytest.mark.parametrize("E,off", LONG_CASES, ids=LONG_IDS)
def test_gradshap_accumulate_past_a_round_of_samples(E, off):
    check_accumulate(E, off, LONG_COMBOS, N=200)


@pytest.mark.parametrize("E,off", REAL, ids=["7x7x2048", "3x224x224"])
def test_gradshap_accumulate_at_the_real_shapes(E, off):
    check_accumulate(E, off, [(8, 10, 5, BIG_SEED, 0.5), (3, 3, 0, 0, 0.0), (70, 10, 5, 0, 0.5)])


# ------------------------------------------------------------------------------------------------ 4: refusals
BADS = ["r0", "n_negative", "first_negative", "past_2_31", "sigma_negative", "sigma_inf", "sigma_nan", "inv_n_inf", "inv_n_nan", "null"]
REFUSALS = [(call, bad) for call in ("gradshap_draws", "gradshap_images", "gradshap_accumulate") for bad in BADS
            if not (call == "gradshap_draws" and (bad.startswith(("sigma", "inv_n")) or bad == "null"))
            and not (call == "gradshap_images" and bad.startswith("inv_n"))]


@pytest.mark.parametrize("call,bad", REFUSALS, ids=["%s-%s" % r for r in REFUSALS])
def test_the_kernels_refuse_bad_arguments(call, bad):
    """error returns with nothing launched: an error that names the call, from the library itself and through the wrapper where a
    wrapper can pass the value on, the sentinel-filled outputs untouched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    lib = _native.lib()
    n, Rn, E = 3, 2, 8
    image, bank, grads = torch.ones(E, device="cuda"), torch.ones((Rn, E), device="cuda"), torch.ones((n, E), device="cuda")
    out = torch.full((n, E), SENTINEL, device="cuda")
    acc = torch.full((E,), SENTINEL, dtype=torch.float64, device="cuda")
    picks = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    alphas = torch.full((n,), SENTINEL, device="cuda")
    R_ = 0 if bad == "r0" else Rn
    n_ = -1 if bad == "n_negative" else n
    first = -1 if bad == "first_negative" else 2 ** 31 - 1 - n + 1 if bad == "past_2_31" else 0
    sigma = {"sigma_negative": -0.5, "sigma_inf": float("inf"), "sigma_nan": float("nan")}.get(bad, 0.5)
    inv_n = {"inv_n_inf": float("inf"), "inv_n_nan": float("nan")}.get(bad, 0.25)
    null = bad == "null"

    def direct():
        if call == "gradshap_draws":
            return lib.scouter_gradshap_draws(picks.data_ptr(), alphas.data_ptr(), 0, 0, first, n_, R_, None)
        if call == "gradshap_images":
            return lib.scouter_gradshap_images_f32(image.data_ptr(), None if null else bank.data_ptr(), out.data_ptr(), sigma, 0, 0, first,
                                                   n_, R_, E, None)
        return lib.scouter_gradshap_accumulate_f64(grads.data_ptr(), image.data_ptr(), bank.data_ptr(), None if null else acc.data_ptr(),
                                                   sigma, inv_n, 0, 0, first, n_, R_, E, None)

    def wrapped():
        if call == "gradshap_draws":
            return K.gradshap_draws(n_, R_, 0, first, picks=picks if n_ >= 0 else None, alphas=alphas if n_ >= 0 else None)
        if call == "gradshap_images":
            return K.gradshap_images(image, bank[:R_], out, sigma, 0, first)
        return K.gradshap_accumulate(grads, image, bank[:R_], acc, sigma, 0, first, inv_n)

    with pytest.raises(RuntimeError, match=call):
        _native.check(direct(), call)
    if bad not in ("null", "n_negative") or call == "gradshap_draws":       # (a tensor has a pointer and no negative length)
        with pytest.raises(RuntimeError, match=call):
            wrapped()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((acc == SENTINEL).all()) and bool((alphas == SENTINEL).all()) and bool((picks == -5).all())
    # n == 0 and E == 0 are no error and no launch
    assert lib.scouter_gradshap_draws(picks.data_ptr(), alphas.data_ptr(), 0, 0, 5, 0, Rn, None) == 0
    assert lib.scouter_gradshap_images_f32(image.data_ptr(), bank.data_ptr(), out.data_ptr(), 0.5, 0, 0, 5, 0, Rn, E, None) == 0
    assert lib.scouter_gradshap_images_f32(image.data_ptr(), bank.data_ptr(), out.data_ptr(), 0.5, 0, 0, 5, n, Rn, 0, None) == 0
    assert lib.scouter_gradshap_accumulate_f64(grads.data_ptr(), image.data_ptr(), bank.data_ptr(), acc.data_ptr(), 0.5, 0.25, 0, 0, 5, 0,
                                               Rn, E, None) == 0
    assert lib.scouter_gradshap_accumulate_f64(grads.data_ptr(), image.data_ptr(), bank.data_ptr(), acc.data_ptr(), 0.5, 0.25, 0, 0, 5, n,
                                               Rn, 0, None) == 0
    assert tuple(K.gradshap_images(image, bank, out[:0], 0.5, 0, 5).shape) == (0, E)
    assert tuple(K.gradshap_images(image, bank, torch.empty((0, E), device="cuda"), 0.5, 0, 5).shape) == (0, E)   # (no storage at all)
    K.gradshap_accumulate(torch.empty((0, E), device="cuda"), image, bank, acc, 0.5, 0, 5, 0.25)
    # ... but the scalar arguments of an empty chunk are checked all the same, through the wrappers too
    for sg, fr in ((-0.5, 0), (float("inf"), 0), (float("nan"), 0), (0.5, -1)):
        with pytest.raises(RuntimeError, match="gradshap_images"):
            K.gradshap_images(image, bank, out[:0], sg, 0, fr)
        with pytest.raises(RuntimeError, match="gradshap_accumulate"):
            K.gradshap_accumulate(grads[:0], image, bank, acc, sg, 0, fr, 0.25)
    for bad_inv in (float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="gradshap_accumulate"):
            K.gradshap_accumulate(grads[:0], image, bank, acc, 0.5, 0, 0, bad_inv)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((acc == SENTINEL).all()) and bool((alphas == SENTINEL).all()) and bool((picks == -5).all())
    check_images(5, 1, COMBOS[1:2])
    check_accumulate(5, 1, COMBOS[1:2])


def test_the_wrappers_refuse_wrong_tensors():
    from scouter_amd import kernels as K
    n, Rn, E = 3, 2, 8
    image, bank, grads = torch.ones((2, 4), device="cuda"), torch.ones((Rn, 2, 4), device="cuda"), torch.ones((n, 2, 4), device="cuda")
    out, acc = torch.empty((n, 2, 4), device="cuda"), torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    for kwargs in (dict(bank=bank.view(Rn, E)), dict(bank=bank[0]), dict(bank=bank[:0]), dict(out=out.view(n, E)), dict(image=image.double()),
                   dict(bank=bank.double()), dict(out=out.double()), dict(out=torch.empty((n, 2, 8), device="cuda")[:, :, ::2]),
                   dict(bank=bank.cpu())):
        with pytest.raises(RuntimeError, match="gradshap_images"):
            K.gradshap_images(**{**dict(image=image, bank=bank, out=out, sigma=0.0, seed=0, first=0), **kwargs})
    for kwargs in (dict(bank=bank.view(Rn, E)), dict(grads=grads.view(n, E)), dict(acc=acc.float()), dict(acc=acc.view(E)),
                   dict(grads=grads.double()), dict(acc=acc.cpu())):
        with pytest.raises(RuntimeError, match="gradshap_accumulate"):
            K.gradshap_accumulate(**{**dict(grads=grads, image=image, bank=bank, acc=acc, sigma=0.0, seed=0, first=0), **kwargs})
    for kwargs in (dict(picks=torch.zeros(n, device="cuda")), dict(alphas=torch.zeros(n, dtype=torch.float64, device="cuda")),
                   dict(picks=torch.zeros(n + 1, dtype=torch.int32, device="cuda"))):
        with pytest.raises(RuntimeError, match="gradshap_draws"):
            K.gradshap_draws(n, Rn, 0, **kwargs)
    # a dense leading slice of a longer buffer is fine
    longer = torch.empty((n + 2, 2, 4), device="cuda")
    assert torch.equal(K.gradshap_images(image, bank, longer[:n], 0.0, 0, 0), K.gradshap_images(image, bank, out, 0.0, 0, 0))


# ------------------------------------------------------------------------------------------------ 5: whole models
MODELS = ["resnet18_mnist_64", "resnest26d_96", "fc_resnet18_mnist_64"]
N_SAMPLES, BANK, SEED = 8, 3, 5


def oracle_full(P, cfg, arch, dtype):
    """images [n, Cin, H, W] -> log-probabilities, the oracle in `dtype`, differentiable through the backbone"""
    _, head = oracle_parts(P, cfg, arch, dtype)
    Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    return lambda x: head(O.backbone_features(Pd, x.to(dtype), arch, training=False).permute(0, 2, 3, 1))


_ORACLE = {}         # case -> the oracle's results in (fp64, fp32): one run per model, shared and left unchanged


def oracle_results(case, P, images, bank, cfg, arch, cols):
    """per dtype a dict: gs / gs_gap for image 0 (the image method, sigma = 0), lgs / lgs_gap for every image (the layer method),
    fed the draws of the restatement"""
    if case not in _ORACLE:
        picks, alphas = R.draws(SEED, 0, N_SAMPLES, bank.shape[0])
        res = []
        for dtype in (torch.float64, torch.float32):
            backbone, head = oracle_parts(P, cfg, arch, dtype)
            x0 = images[0].to(dtype)
            gs, gs_gap = R.gradient_shap(oracle_full(P, cfg, arch, dtype), x0[None].repeat(N_SAMPLES, 1, 1, 1), bank, picks, alphas, cols)
            feats = backbone(torch.cat([bank, images]))
            bank_feats, A = feats[:bank.shape[0]], feats[bank.shape[0]:]
            lgs = [R.gradient_shap(head, A[b][None].repeat(N_SAMPLES, 1, 1, 1), bank_feats, picks, alphas, cols) for b in range(images.shape[0])]
            res.append(dict(gs=gs, gs_gap=gs_gap, lgs=torch.stack([a.sum(dim=3) for a, _ in lgs]), lgs_gap=torch.stack([g for _, g in lgs])))
        _ORACLE[case] = tuple(res)
    return _ORACLE[case]


def own_gradient_shap(m, x, bank, cols, sigma, batch, n_samples=N_SAMPLES):
    """the definition over the HIP path's own gradients at the chunking of the method, summed in float64 on the host:
    (terms [B, K, C, H, W], their magnitudes)"""
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as AT
    res = []
    with AT._eval_mode(m), torch.enable_grad():
        n = int(m(x[:1]).shape[1])
        for b in range(x.shape[0]):
            _, diffs, _ = restated_rows(x[b], bank, sigma, SEED, 0, n_samples)
            per_class = []
            for c in cols:
                seed = one_hot((batch, n), c)
                parts = []
                for first in range(0, n_samples, batch):
                    k = min(batch, n_samples - first)
                    chunk = K.gradshap_images(x[b], bank, torch.empty((k,) + tuple(x[b].shape), device="cuda"), sigma, SEED, first)
                    parts.append(AT._chunk_gradient(m, chunk, seed).cpu().double())
                t = torch.cat(parts) * diffs.cpu().double() / n_samples
                per_class.append((t.sum(dim=0), t.abs().sum(dim=0)))
            res.append((torch.stack([t for t, _ in per_class]), torch.stack([a for _, a in per_class])))
    return torch.stack([t for t, _ in res]), torch.stack([a for _, a in res])


def own_layer_gradient_shap(m, x, bank, cols, batch, n_samples=N_SAMPLES):
    """per image (terms [K, h, w, C], their magnitudes): the definition over the HIP path's own head gradients"""
    from scouter_amd import kernels as K
    Rn = bank.shape[0]
    feats = m.feature_pass(torch.cat([bank, x])).features
    bank_feats = feats[:Rn]
    res = []
    for b in range(x.shape[0]):
        A = feats[Rn + b]
        _, diffs, _ = restated_rows(A, bank_feats, 0.0, SEED, 0, n_samples)
        parts = []
        for first in range(0, n_samples, batch):
            k = min(batch, n_samples - first)
            fp = m.head_pass(K.gradshap_images(A, bank_feats, torch.empty((k,) + tuple(A.shape), device="cuda"), 0.0, SEED, first))
            parts.append(torch.stack([fp.grad(one_hot(fp.log_probs.shape, c)) for c in cols]).cpu().double())
        terms = torch.cat(parts, dim=1) * diffs.cpu().double()[None] / n_samples                  # [K, n, h, w, C]
        res.append((terms.sum(dim=1), terms.abs().sum(dim=1)))
    return res


@pytest.mark.parametrize("case", MODELS)
def test_the_two_methods_on_whole_models(case):
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as AT
    m, P, images, cfg, arch = build(case)
    images = images[:2].contiguous()
    bank = (0.5 * rand((BANK,) + tuple(images.shape[1:]), 77)).contiguous()
    x, bd = images.cuda(), bank.cuda()
    B, cols = 2, [1, 4]
    E = images[0].numel()
    m.train()
    before = bn_buffers(m)
    kw = dict(classes=cols, baselines=bd, n_samples=N_SAMPLES, seed=SEED)
    gs, gs_delta = AT.gradient_shap(m, x, batch=3, return_delta=True, **kw)
    gsn, gsn_delta = AT.gradient_shap(m, x, batch=3, sigma=0.5, return_delta=True, **kw)
    lgs, lgs_attr, lgs_delta = AT.layer_gradient_shap(m, x, batch=5, return_attr=True, return_delta=True, **kw)
    torch.cuda.synchronize()
    assert m.training                                                       # the caller's mode is back
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    h, w, C = lgs_attr.shape[2:]
    assert tuple(gs.shape) == (B, 2) + tuple(images.shape[1:]) and gs.dtype == torch.float32 and gs.is_cuda
    assert tuple(lgs.shape) == (B, 2, h, w) and tuple(lgs_attr.shape) == (B, 2, h, w, C) and lgs.dtype == torch.float32
    for d in (gs_delta, gsn_delta, lgs_delta):
        assert tuple(d.shape) == (B, 2) and d.dtype == torch.float32
    assert bool(torch.isfinite(gs).all()) and float(gs.abs().max()) > 0

    # ---- the definition over the HIP path's own gradients, the same chunks: the kernels' bounds
    for name, got, sigma in (("gradshap", gs, 0.0), ("gradshap sigma 0.5", gsn, 0.5)):
        ref, mag = own_gradient_shap(m, x, bd, cols, sigma, 3)
        err, bound = (got.cpu().double() - ref).abs(), EPS * ref.abs() + (N_SAMPLES + 4) * U * mag
        print("%s %s: max err %.3e, max err / bound %.3f" % (case, name, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (case, name)
    own_lgs = own_layer_gradient_shap(m, x, bd, cols, 5)
    check_own(case + " layergradshap", lgs, lgs_attr, None, own_lgs, N_SAMPLES)
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())

    # ---- chunks longer than a tile of 8 rows and than a round of 64 samples, as the defaults run them: the same definition
    lkw = dict(classes=cols, baselines=bd, seed=SEED)
    for n_long, batch in ((70, 70), (70, 256), (70, 66), (11, 11)):
        got = AT.layer_gradient_shap(m, x, n_samples=n_long, batch=batch, return_attr=True, **lkw)
        check_own("%s layergradshap, %d samples in chunks of %d" % (case, n_long, batch), got[0], got[1], None,
                  own_layer_gradient_shap(m, x, bd, cols, batch, n_long), n_long)
    got = AT.gradient_shap(m, x[:1], n_samples=11, batch=11, sigma=0.5, **lkw)
    ref, mag = own_gradient_shap(m, x[:1], bd, cols, 0.5, 11, 11)
    err, bound = (got.cpu().double() - ref).abs(), EPS * ref.abs() + (11 + 4) * U * mag
    print("%s gradshap, 11 samples in one chunk: max err / bound %.3f" % (case, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), case

    # ---- the CPU oracle under fp64 and fp32 autograd, fed the same draws: the project's rule
    o64, o32 = oracle_results(case, P, images, bank, cfg, arch, cols)
    for k, c in enumerate(cols):
        check_rule("%s gradshap(class %d)" % (case, c), gs[0, k], o64["gs"][k], o32["gs"][k])
        check_rule("%s layergradshap(class %d)" % (case, c), lgs[:, k], o64["lgs"][:, k], o32["lgs"][:, k])

    # ---- return_delta: its definition, in float64 from the returned attribution and the model's own outputs
    picks, _ = R.draws(SEED, 0, N_SAMPLES, BANK)
    share = R.shares(picks, BANK)
    m.eval()
    with torch.no_grad():
        logp = m(torch.cat([bd, x])).cpu().double()
    m.train()
    feats = m.feature_pass(torch.cat([bd, x])).features
    heads = [m.head_pass(torch.cat([feats[:BANK], feats[BANK + b][None]])).log_probs.detach().cpu().double() for b in range(B)]
    ends = (logp[BANK:] - (share @ logp[:BANK])[None])[:, cols]
    want = gs.cpu().double().sum(dim=(2, 3, 4)) - ends
    err, bound = (gs_delta.cpu().double() - want).abs(), E * 4 * EPS * gs.cpu().double().abs().amax(dim=(2, 3, 4)) + 2 * EPS * want.abs()
    print("%s gradshap delta %s, out(x) - E out(b) %s, err / bound %.3f" % (case, gs_delta.cpu().tolist(), ends.tolist(), float((err / bound).max())))
    assert bool((err <= bound).all())
    # (with sigma > 0 the gap also holds the noise: the same definition, at the clean image)
    want = gsn.cpu().double().sum(dim=(2, 3, 4)) - ends
    err, bound = (gsn_delta.cpu().double() - want).abs(), E * 4 * EPS * gsn.cpu().double().abs().amax(dim=(2, 3, 4)) + 2 * EPS * want.abs()
    assert bool((err <= bound).all())
    lends = torch.stack([(lp[BANK] - share @ lp[:BANK])[cols] for lp in heads])
    want = lgs_attr.cpu().double().sum(dim=(2, 3, 4)) - lends
    err = (lgs_delta.cpu().double() - want).abs()
    bound = h * w * C * 4 * EPS * lgs_attr.cpu().double().abs().amax(dim=(2, 3, 4)) + 2 * EPS * want.abs()
    print("%s layergradshap delta %s, out(A) - E out(A_r) %s, err / bound %.3f" % (case, lgs_delta.cpu().tolist(), lends.tolist(),
                                                                                  float((err / bound).max())))
    assert bool((err <= bound).all())

    # ---- the same seed gives the same bits, another seed does not; without delta and attr: the same maps
    assert torch.equal(AT.gradient_shap(m, x, batch=3, **kw), gs) and torch.equal(AT.gradient_shap(m, x, batch=3, sigma=0.5, **kw), gsn)
    assert torch.equal(AT.layer_gradient_shap(m, x, batch=5, **kw), lgs)
    assert not torch.equal(AT.gradient_shap(m, x, batch=3, **{**kw, "seed": SEED + 1}), gs)
    assert not torch.equal(AT.layer_gradient_shap(m, x, batch=5, **{**kw, "seed": SEED + 1}), lgs)
    assert not torch.equal(gsn, gs)

    # ---- the int bank is the explicit bank of noise_images rows n_samples .. n_samples + R - 1
    zeros = torch.zeros_like(x[0])
    explicit = K.noise_images(zeros, torch.empty((BANK,) + tuple(zeros.shape), device="cuda"), 0.7, SEED, N_SAMPLES)
    ikw = dict(classes=cols[:1], n_samples=N_SAMPLES, seed=SEED)
    assert torch.equal(AT.gradient_shap(m, x, baselines=BANK, bank_sigma=0.7, batch=8, **ikw), AT.gradient_shap(m, x, baselines=explicit, batch=8, **ikw))
    assert torch.equal(AT.layer_gradient_shap(m, x, baselines=BANK, bank_sigma=0.7, **ikw), AT.layer_gradient_shap(m, x, baselines=explicit, **ikw))
    black = AT.gradient_shap(m, x, baselines=1, bank_sigma=0.0, batch=8, **ikw)                        # the black image
    assert torch.equal(black, AT.gradient_shap(m, x, baselines=zeros[None], batch=8, **ikw))

    # ---- classes: None is every output, a LongTensor the diagonal; a class outside the outputs is refused
    n = int(logp.shape[1])
    cls = (torch.arange(B) * 3 + 1) % n
    diag = AT.layer_gradient_shap(m, x, classes=cls, baselines=bd, n_samples=N_SAMPLES, seed=SEED, batch=5, return_delta=True)
    every = AT.layer_gradient_shap(m, x, baselines=bd, n_samples=N_SAMPLES, seed=SEED, batch=5, return_delta=True)
    assert tuple(every[0].shape) == (B, n, h, w) and tuple(diag[0].shape) == (B, 1, h, w)
    assert torch.equal(every[0][:, cols], lgs) and torch.equal(every[1][:, cols], lgs_delta)
    assert all(torch.equal(diag[0][b, 0], every[0][b, cls[b]]) and torch.equal(diag[1][b, 0], every[1][b, cls[b]]) for b in range(B))
    own, own_delta = AT.gradient_shap(m, x, classes=torch.tensor([4, 1]), baselines=bd, n_samples=N_SAMPLES, seed=SEED, batch=3, return_delta=True)
    assert torch.equal(own[0, 0], gs[0, 1]) and torch.equal(own[1, 0], gs[1, 0])
    assert torch.equal(own_delta[0, 0], gs_delta[0, 1]) and torch.equal(own_delta[1, 0], gs_delta[1, 0])
    for fn in (AT.gradient_shap, AT.layer_gradient_shap):
        for bad in ([n], [-1]):
            with pytest.raises(IndexError):
                fn(m, x, classes=bad, baselines=bd, n_samples=2)
        assert fn(m, x, classes=[], baselines=bd, n_samples=2).shape[:2] == (B, 0)
        with pytest.raises(ValueError, match="baselines"):
            fn(m, x, baselines=bd[:, :, 1:])

    # ---- the maps, and the two scores that take an explanation
    H, W = images.shape[2:]
    assert torch.equal(AT.layergradshap_maps(m, x, min_level=0.2, batch=5, **kw), K.cam_maps(lgs, H, W, 0.2))
    assert torch.equal(AT.layergradshap_maps(m, x, size=(20, 30), batch=5, **kw), K.cam_maps(lgs, 20, 30, 0.0))
    maps = AT.gradient_maps(gs, min_level=0.2)
    assert tuple(maps.shape) == (B, 2, H, W) and maps.dtype == torch.uint8 and bool(maps.any())
    inf = AT.infidelity(m, x, gs, classes=cols, n_samples=4, batch=5)
    sens = AT.sensitivity_max(lambda im: AT.gradient_shap(m, im, batch=8, **kw), x[:1], n_samples=2, batch=3)
    torch.cuda.synchronize()
    assert tuple(inf.raw.shape) == (B, 2) and bool(torch.isfinite(inf.normalized).all())
    assert tuple(sens.score.shape) == (1, 2) and bool(torch.isfinite(sens.score).all()) and bool((sens.score > 0).all())
    assert m.training and all(torch.equal(before[k], v) for k, v in bn_buffers(m).items())


# ------------------------------------------------------------------------------------------------ 6: the tool
TOOL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--gradshap", "true", "--layergradshap", "true",
        "--gradshap_samples", "6", "--gradshap_baselines", "3", "--gradshap_batch", "4", "--gradshap_sigma", "0.1", "--gradshap_seed", "2",
        "--layergradshap_samples", "9", "--layergradshap_baselines", "2", "--layergradshap_batch", "5", "--grad_min_level", "0.2",
        "--eval_fold", "true"]
NAMES = ["gradshap", "layergradshap"]


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_the_tool_on_one_image(use_slot, tmp_path, monkeypatch, capsys):
    """--table_images 0 (the default) writes the two PNG sets of every class, the bytes of the library's maps, no other family's
    files, and one causal and one infidelity line per row"""
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.tools import attribution as AT
    from scouter_amd.tools import gradshap as G
    vis_dir = str(tmp_path / "vis")
    argv = ["gradshap.py"] + TOOL + ["--use_slot", "true" if use_slot else "false", "--causal", "true", "--causal_step", "2048",
                                     "--infidelity", "true", "--infidelity_samples", "4", "--infidelity_batch", "5",
                                     "--vis_dir", vis_dir, "--output_dir", str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    G.main()
    out = capsys.readouterr().out
    names = (["slot"] if use_slot else []) + NAMES
    for score, count in (("causal", 2), ("infidelity", 3)):
        lines = [ln.split() for ln in out.splitlines() if ln.startswith(score + " ")]
        assert [ln[1] for ln in lines] == names, lines
        for ln in lines:
            values = [float(v) for v in ln[4:] if v[0].isdigit() or v[0] == "-"]
            assert len(values) == count and all(math.isfinite(v) for v in values), ln
    assert sorted(os.listdir(vis_dir)) == sorted("%s_%d.png" % (n, c) for n in names for c in range(10))
    args = G.get_gradshap_parser().parse_args(argv[1:])
    gkw, lkw = G.option_kwargs(args, "gradshap"), G.option_kwargs(args, "layergradshap")
    assert gkw == dict(n_samples=6, baselines=3, bank_sigma=1.0, sigma=0.1, batch=4, seed=2)
    assert lkw == dict(n_samples=9, baselines=2, bank_sigma=1.0, batch=5, seed=0)
    torch.manual_seed(11)
    model, _ = T.build_model(args)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))[None].cuda()
    want = {"gradshap": AT.gradient_maps(AT.gradient_shap(model, x, **gkw), min_level=0.2),
            "layergradshap": AT.layergradshap_maps(model, x, min_level=0.2, **lkw)}
    for name, maps in want.items():
        maps = maps[0].cpu().numpy()
        assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and any(m.any() for m in maps)
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(vis_dir, "%s_%d.png" % (name, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, maps[c]), (name, c)


def test_the_tool_on_a_table(tmp_path, monkeypatch, capsys):
    """--table_images 2 on synthetic data: one `table <family>:` line for each of the two rows after the table's own"""
    from scouter_amd.tools import gradshap as G
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["gradshap.py"] + TOOL + [
        "--use_slot", "true", "--synthetic_data", "true", "--num_workers", "0", "--table_images", "2", "--batch_size", "2",
        "--localization", "true", "--output_dir", str(tmp_path / "none")])
    result = G.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == ["slot:"] + [n + ":" for n in NAMES] + ["accuracy"]
    for ln in lines[1:3]:
        words = ln.split()
        assert words[2:4] == ["images", "2"] and words[4] == "area" and 0.0 <= float(words[5]) <= 1.0
    for name in NAMES:
        cols = result.rows[name]
        assert all(v.dtype == np.float64 and v.shape == (2,) for v in cols.values())
        assert ((cols["area"] >= 0) & (cols["area"] <= 1)).all()
