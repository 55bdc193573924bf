"""Score-CAM (-m gpu): the kernels of csrc/scorecam.hip as Score-CAM runs them -- one sample, no noise, no ramp -- against fp64:
kernels.scorecam_ranges and kernels.sscam_mask_images against channels resized with F.interpolate in float64 (no reference
program is involved), kernels.sscam_weights followed by kernels.sscam_contract against the float64 einsum -- the refusals of
scorecam_ranges (those of the sscam_* calls: test_sscam_gpu.py), tools/attribution.py scorecam on whole models against the same
fp64 sum over the HIP path's own features and log-probabilities, and scorecam_maps / test.py run_scorecam / run_causal.

Inputs.  Features are relu(randn) from a seeded CPU generator.  Every channel meant to be live gets its maximum at [0, 0] and a 0
at [h - 1, w - 1]; the clamped interpolation reproduces the corners exactly when H >= h and W >= w, so the span of the resized
channel is M_c = max_p |A[p, c]|.  The tests assert M_c / span_c <= 4 on the float64 reference for every live channel.  Every case
also carries one constant non-zero channel (0.7) and one all-zero channel; both are dead.

Bounds (EPS = 2^-24), each twice the worst case.  The source coordinate carries one rounding of the scale and one of the fma,
<= 1.5 in EPS; it moves the value by at most that times the source range <= 2 M_c.  The three interpolation fmas add
<= 6 EPS M_c.  So e_U(c) = (6 (h + w) + 12) EPS M_c bounds |U - U64|, and with it |lo - lo64| and |hi - hi64|.  A mask value
(U - lo) / span then lies within 4 e_U(c) / span_c + 8 EPS of the float64 one, times |image value| for the masked image.  The
accumulation adds one fma per channel: (C + 8) EPS sum_c |w_c A[p, c]|, and exactly nothing where every term is 0."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402

SENTINEL = -777.25
EPS = 2.0 ** -24


def make_features(h, w, C, dead, seed, signed=False):
    """fp32 [h, w, C]: relu(randn) (signed: randn), the live channels with their maximum at [0, 0] and 0 at [h - 1, w - 1], channel
    dead[0] constant 0.7 and channel dead[1] all zero"""
    A = torch.randn((h, w, C), generator=torch.Generator().manual_seed(seed))
    if not signed:
        A = A.relu()
    if h * w > 1:
        mx = A.abs().amax(dim=(0, 1))
        A[0, 0] = torch.where(mx > 0, mx, torch.ones_like(mx))
        A[h - 1, w - 1] = 0.0
    A[:, :, dead[0]] = 0.7
    A[:, :, dead[1]] = 0.0
    return A.contiguous()


def reference_fp64(A, H, W):
    """the definition in float64 -> (U [C, H, W], lo [C], hi [C], live [C], mask [C, H, W], M [C], e_U [C])"""
    h, w, C = A.shape
    U = F.interpolate(A.permute(2, 0, 1)[None].double(), size=(H, W), mode="bilinear", align_corners=False)[0]
    lo, hi = U.amin(dim=(1, 2)), U.amax(dim=(1, 2))
    M = A.double().abs().amax(dim=(0, 1))
    # (F.interpolate blends w0 a + w1 b: a constant channel comes back with float64 rounding noise of order 2^-52 M, so the
    # reference calls a channel live when its float64 span exceeds 2^-30 M; the live channels' spans are at least M / 4, below)
    live = hi - lo > 2.0 ** -30 * M
    span = torch.where(live, hi - lo, torch.ones_like(lo))
    mask = torch.where(live[:, None, None], (U - lo[:, None, None]) / span[:, None, None], torch.zeros_like(U))
    # a condition on the inputs: the span of a live channel is not small against its magnitude
    assert bool((M[live] / (hi - lo)[live] <= 4).all())
    return U, lo, hi, live, mask, M, (6 * (h + w) + 12) * EPS * M


# (Cin, H, W, h, w, C, first, n)
CASES = [(1, 5, 7, 2, 3, 5, 0, 5),            # the one-pixel path, C not a multiple of 4
         (3, 64, 64, 2, 2, 512, 500, 12),     # the tail of the whole-model stream
         (3, 224, 224, 7, 7, 64, 13, 6),      # real geometry, the four-pixel path, a mid-stream chunk
         (3, 33, 47, 9, 9, 20, 0, 20),        # non-integer ratios
         (1, 16, 16, 16, 16, 8, 0, 8),        # H = h: the mask is the normalised source
         (2, 8, 8, 1, 1, 4, 0, 4)]            # one source pixel: every channel is dead and every image zero
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def case_data(case, seed=0):
    """(image, A, the float64 reference) of a case: computed once, shared by the tests, never changed"""
    Cin, H, W, h, w, C, first, n = case
    image = torch.randn((Cin, H, W), generator=torch.Generator().manual_seed(7000 + seed))
    A = make_features(h, w, C, (first + 1, first + n - 1), 7100 + seed)
    return image, A, reference_fp64(A, H, W)


# ------------------------------------------------------------------------------------------------ 1: K.scorecam_ranges
def _check_ranges(case, seed=0):
    from scouter_amd import kernels as K
    Cin, H, W, h, w, C, first, n = case
    _, A, (_, lo64, hi64, live64, _, M, e_U) = case_data(case, seed)
    Ad = A.cuda()
    got = K.scorecam_ranges(Ad, H, W)
    again = K.scorecam_ranges(Ad, H, W, out=torch.full((C, 2), SENTINEL, device="cuda"))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (C, 2) and got.is_cuda
    assert torch.equal(got, again)                                                         # a second call: the same bits
    g = got.cpu().double()
    err = torch.maximum((g[:, 0] - lo64).abs(), (g[:, 1] - hi64).abs())
    ratio = (err / e_U.clamp_min(1e-300))[M > 0]
    print("scorecam_ranges", case, "max err %.3e, max err / bound %.3f, %d live of %d channels" %
          (float(err.max()), float(ratio.max()) if ratio.numel() else 0.0, int(live64.sum()), C))
    assert bool((err <= e_U).all())
    assert bool((g[~live64, 0] == g[~live64, 1]).all())                                     # dead channels: lo == hi exactly
    assert bool((g[live64, 1] > g[live64, 0]).all())
    dead = [first + 1, first + n - 1]
    assert not bool(live64[dead].any())
    assert int(live64.sum()) == (C - 2 if h * w > 1 else 0)
    return got


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_scorecam_ranges_against_fp64(case):
    _check_ranges(case)


@pytest.mark.parametrize("case", [CASES[3], CASES[0]], ids=[CASE_IDS[3], CASE_IDS[0]])
def test_scorecam_ranges_are_the_extrema_of_resize_bilinear(case):
    """ranges[c] = (min, max) of the resized channel, bit for bit: the range kernel and kernels.resize_bilinear form the resized
    value with the same expression.  randn features: finite, no constant channel, so no +0 / -0 tie enters."""
    from scouter_amd import kernels as K
    _, H, W, h, w, C, _, _ = case
    A = torch.randn((h, w, C), generator=torch.Generator().manual_seed(7300)).cuda()
    assert bool(torch.isfinite(A).all()) and bool((A.amax(dim=(0, 1)) > A.amin(dim=(0, 1))).all())
    U = K.resize_bilinear(A.permute(2, 0, 1).contiguous(), H, W)                            # [C, H, W]
    got = K.scorecam_ranges(A, H, W)
    torch.cuda.synchronize()
    assert torch.equal(got[:, 0], U.amin(dim=(1, 2))) and torch.equal(got[:, 1], U.amax(dim=(1, 2)))


# ------------------------------------------------------------------------------------------------ 2: K.sscam_mask_images, one sample
def _check_mask_images(case, seed=0):
    from scouter_amd import kernels as K
    Cin, H, W, h, w, C, first, n = case
    image, A, (_, lo64, hi64, live64, mask64, M, e_U) = case_data(case, seed)
    Ad = A.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    sl = slice(first, first + n)
    ref = image.double()[None] * mask64[sl][:, None]                                        # [n, Cin, H, W]
    span = torch.where(live64, hi64 - lo64, torch.ones_like(lo64))
    coef = (4 * e_U / span + 8 * EPS)[sl]
    bound = coef[:, None, None, None] * image.double().abs()[None]
    out = torch.full((n + 1, Cin, H, W), SENTINEL, device="cuda")
    got = K.sscam_mask_images(image.cuda(), Ad, ranges, out[:n], first, 1)
    ones = K.sscam_mask_images(torch.ones((Cin, H, W), device="cuda"), Ad, ranges, torch.empty((n, Cin, H, W), device="cuda"),
                               first, 1)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[n] == SENTINEL).all())            # the extra image keeps the sentinel
    res = out[:n].cpu().double()
    err = (res - ref).abs()
    print("sscam_mask_images, one sample", case, "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    lv = live64[sl]
    assert bool((res[~lv] == 0).all())                                                      # dead channels: exactly zero
    ones = ones.cpu()
    assert bool((ones[~lv] == 0).all())
    if bool(lv.any()):                                                                      # live: exactly 0 and exactly 1 attained
        flat = ones[lv].flatten(1)
        assert bool((flat.amin(dim=1) == 0).all()) and bool((flat.amax(dim=1) == 1).all())
        assert bool((ones[lv][:, 0] == ones[lv][:, -1]).all())                              # one mask for every image channel


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_scorecam_masked_images_against_fp64(case):
    _check_mask_images(case)


# ------------------------------------------------------------------------------------------------ 3: K.sscam_weights, K.sscam_contract
# (K, n_classes, h, w, C, the columns or None for 0 .. K - 1, signed features)
ACC_CASES = [(10, 10, 7, 7, 64, None, False), (3, 200, 2, 2, 512, [150, 7, 150], False),
             (200, 200, 9, 9, 20, None, False), (1, 1, 1, 1, 4, None, False),
             (5, 12, 3, 5, 37, [11, 0, 3, 3, 7], True)]


def check_accumulated(got, ref, absref, start, C, what):
    """|got - ref| <= (C + 8) 2^-24 sum_c |w_c A[p, c]|, and exactly the starting value where every term is 0"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = (C + 8) * EPS * absref
    zero = absref == 0
    print("%s: max err %.3e, max err / bound %.3f, %d elements whose terms are all zero" %
          (what, float(err.max()), float((err / bound.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.0,
           int(zero.sum())))
    assert bool((got[zero] == start[zero]).all())
    assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound.clamp_min(1e-300))[~zero].max()))


@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: "%dof%d_%dx%d_c%d%s" % (c[:5] + ("_signed" if c[6] else "",)))
def test_scorecam_weights_and_contract_against_fp64(case):
    """one sample: kernels.sscam_weights (one call, and a call cut at C // 3) followed by kernels.sscam_contract(norm = 1)"""
    from scouter_amd import kernels as K
    Kc, n_classes, h, w, C, cols, signed = case
    H, W = 2 * h + 1, 2 * w + 3
    cols = torch.tensor(cols if cols is not None else list(range(Kc)), dtype=torch.int32)
    gen = torch.Generator().manual_seed(7200 + C)
    logp = F.log_softmax(torch.randn((C, n_classes), generator=gen), dim=1)
    dead = (1, C - 1)
    A = make_features(h, w, C, dead, 7300 + C, signed=signed)
    _, _, _, live64, _, _, _ = reference_fp64(A, H, W)
    assert int(live64.sum()) == (C - 2 if h * w > 1 else 0)
    wts = logp.double().exp()[:, cols.long()] * live64[:, None].double()                  # [C, K]
    ref = torch.einsum("ck,hwc->khw", wts, A.double())
    absref = torch.einsum("ck,hwc->khw", wts, A.double().abs())
    ld, cd, Ad = logp.cuda(), cols.cuda(), A.cuda()
    ranges = K.scorecam_ranges(Ad, H, W)
    assert torch.equal((ranges[:, 1] - ranges[:, 0] > 0).cpu(), live64)

    def run(lp, cuts):
        wsum = torch.zeros((C, Kc), dtype=torch.float64, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            K.sscam_weights(lp[a:b], cd, wsum, a)
        return K.sscam_contract(wsum, Ad, ranges, torch.full((Kc, h, w), SENTINEL, device="cuda"), 1.0)

    one = run(ld, [0, C])
    two = run(ld, [0, C // 3, C])
    again = run(ld, [0, C])
    torch.cuda.synchronize()
    check_accumulated(one, ref, absref, torch.zeros_like(ref), C, "sscam_weights, sscam_contract %s" % (case[:5],))
    assert torch.equal(one, two) and torch.equal(one, again)      # split at any point, and a second call: the same bits
    # dead channels given a huge log-probability change nothing
    huge = ld.clone()
    huge[(~live64).nonzero().flatten().cuda()] = 1.0e4
    assert torch.equal(run(huge, [0, C]), one)


# ------------------------------------------------------------------------------------------------ 4: refusals
BAD = {"scorecam_ranges": ["null", "hw_cap", "H0", "W0", "out_shape"]}


@pytest.mark.parametrize("call,bad", [(c, b) for c in BAD for b in BAD[c]])
def test_scorecam_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, h w above 1024, H or W below 1, an output of the wrong shape: an error naming the call, the output
    untouched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    H, W, h, w, C = 20, 24, 3, 4, 6
    if bad == "hw_cap":
        h, w = 33, 32                                                    # 1056 source positions: above the 1024 a channel may have
    feat = torch.rand((h, w, C), generator=torch.Generator().manual_seed(5)).cuda()
    ranges = torch.full((C, 2), SENTINEL, device="cuda")
    lib = _native.lib()
    with pytest.raises(RuntimeError, match=call):
        if bad == "null":
            _native.check(lib.scouter_scorecam_ranges_f32(feat.data_ptr(), None, h, w, C, H, W, None), call)
        elif bad == "out_shape":
            K.scorecam_ranges(feat, H, W, out=ranges[:C - 1])
        else:
            K.scorecam_ranges(feat, 0 if bad == "H0" else H, 0 if bad == "W0" else W, out=ranges)
    torch.cuda.synchronize()
    assert bool((ranges == SENTINEL).all())
    _check_ranges(CASES[0])
    _check_mask_images(CASES[3])


# ------------------------------------------------------------------------------------------------ 5: whole models
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


def expected_scorecam(m, images, batch):
    """fp64 (ref, absref) [B, n, h, w]: the definition's sum over the HIP path's own data -- the features of feature_pass, the
    live flags of K.scorecam_ranges (checked against fp64 above), the same chunks built with K.sscam_mask_images (one sample)
    and the model in eval mode under no_grad at the same batch"""
    from scouter_amd import kernels as K
    B, Cin, H, W = images.shape
    feat = m.feature_pass(images).features.detach().float().contiguous()
    _, h, w, C = feat.shape
    was_training = m.training
    m.eval()
    ref, absref = [], []
    try:
        with torch.no_grad():
            for b in range(B):
                ranges = K.scorecam_ranges(feat[b], H, W)
                live = (ranges[:, 1] - ranges[:, 0] > 0).cpu().double()
                logp = []
                for first in range(0, C, batch):
                    n = min(batch, C - first)
                    chunk = K.sscam_mask_images(images[b], feat[b], ranges, torch.empty((n, Cin, H, W), device="cuda"), first, 1)
                    logp.append(m(chunk).cpu().double())
                wts = torch.cat(logp).exp() * live[:, None]
                A = feat[b].cpu().double()
                ref.append(torch.einsum("ck,hwc->khw", wts, A))
                absref.append(torch.einsum("ck,hwc->khw", wts, A.abs()))
    finally:
        m.train(was_training)
    return torch.stack(ref), torch.stack(absref), feat


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_scorecam_on_whole_models(use_slot):
    """resnet18 / MNIST / 64^2 / batch 2: features [2, 2, 2, 512], batch = 96 so that 512 = 5 x 96 + 32 ends in a short chunk.
    One chunk of 512 against chunks of 96: the forwards run at another batch size; the eval forward of this model is
    batch-invariant bit for bit at these shapes (every image's log-probabilities are the same at batch 32, 96 and 512, asserted
    here first), so the two runs are asserted to give equal bits."""
    from scouter_amd.tools.attribution import scorecam
    m, images = build(use_slot)
    batch, C = 96, 512
    m.train()
    ref, absref, feat = expected_scorecam(m, images, batch)
    assert tuple(feat.shape) == (2, 2, 2, C)
    before = bn_buffers(m)
    S = scorecam(m, images, batch=batch)
    torch.cuda.synchronize()
    # ---- the value, the shape, the state left behind
    assert tuple(S.shape) == (2, 10, 2, 2) and S.dtype == torch.float32 and S.is_cuda
    assert bool(torch.isfinite(S).all()) and float(S.max()) > float(S.min())
    name = "slot" if use_slot else "fc"
    check_accumulated(S, ref, absref, torch.zeros_like(ref), C, "scorecam %s" % name)
    assert m.training
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in m.parameters())
    # ---- reproducibility and class selection
    assert torch.equal(scorecam(m, images, batch=batch), S)
    two = scorecam(m, images, classes=[0, 3], batch=batch)
    assert tuple(two.shape) == (2, 2, 2, 2) and torch.equal(two[:, 0], S[:, 0]) and torch.equal(two[:, 1], S[:, 3])
    own = scorecam(m, images, classes=torch.tensor([7, 2]), batch=batch)
    assert tuple(own.shape) == (2, 1, 2, 2) and torch.equal(own[0, 0], S[0, 7]) and torch.equal(own[1, 0], S[1, 2])
    m.eval()
    with torch.no_grad():                                                                 # is the eval forward batch-invariant?
        x512 = torch.randn((512, 1, 64, 64), generator=torch.Generator().manual_seed(13)).cuda()
        l512 = m(x512)
        assert torch.equal(torch.cat([m(x512[i:i + 96]) for i in range(0, 512, 96)]), l512)
    m.train()
    whole = scorecam(m, images, batch=512)                                                # one chunk
    print("scorecam %s: one chunk of 512 against chunks of 96: %s" %
          (name, "equal bits" if torch.equal(whole, S) else "max difference %.3e" % float((whole - S).abs().max())))
    assert torch.equal(whole, S)
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            scorecam(m, images, classes=bad, batch=batch)
    with pytest.raises(ValueError):
        scorecam(m, images, classes=torch.tensor([0, 1, 2]), batch=batch)
    with pytest.raises(ValueError):
        scorecam(m, images, batch=0)
    with pytest.raises(ValueError):
        scorecam(m, images[0], batch=batch)
    assert m.training and all(p.grad is None for p in m.parameters())
    # ---- BatchNorm-folded forwards
    m.set_inference_fold(True)
    folded = scorecam(m, images, batch=batch)
    m.set_inference_fold(False)
    diff, top = float((folded - S).abs().max()), float(S.abs().max())
    print("scorecam folded against unfolded: max difference %.3e, max|S| %.3e, ratio %.3e" % (diff, top, diff / top))
    assert diff <= 1e-3 * top
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 6: maps and the test tool
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_scorecam_maps_and_test_tool(use_slot, tmp_path, capsys):
    """scorecam_maps is K.cam_maps of scorecam, bytewise; scouter_amd.test run_scorecam writes scorecam_0.png .. scorecam_9.png,
    64 x 64, byte for byte scorecam_maps of the image; run_causal scores the family `scorecam`"""
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.tools.attribution import scorecam, scorecam_maps
    m, images = build(use_slot)
    S = scorecam(m, images, batch=96)
    for min_level in (0.0, 0.3):
        maps = scorecam_maps(m, images, min_level=min_level, batch=96)
        assert maps.dtype == torch.uint8 and maps.is_cuda and tuple(maps.shape) == (2, 10, 64, 64)
        assert torch.equal(maps, K.cam_maps(S, 64, 64, min_level))
    args = model_args(use_slot)
    args.device, args.grad_min_level, args.scorecam_batch, args.causal_step = "cuda", 0.2, 96, 256
    image = images[0].cpu()
    vis_dir = str(tmp_path / "vis")
    got = T.run_scorecam(args, m, image, vis_dir)
    want = scorecam_maps(m, images[:1], min_level=0.2, batch=96)[0].cpu().numpy()
    assert got.shape == (10, 64, 64) and got.dtype == np.uint8 and np.array_equal(got, want)
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(vis_dir, "scorecam_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
    assert not os.path.exists(os.path.join(vis_dir, "scorecam_10.png"))
    assert any(w.any() for w in want)
    m.eval()
    with torch.no_grad():
        pred = int(m(images[:1]).argmax(dim=1))
    capsys.readouterr()
    first = T.run_causal(args, m, image, pred, families=["scorecam"])
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln.startswith("causal ")]
    assert len(lines) == 1 and lines[0][:4] == ["causal", "scorecam", "class", "%d:" % pred]
    assert lines[0][4] == "deletion" and lines[0][6] == "insertion" and len(lines[0]) == 8
    assert list(first) == ["scorecam"]
    for v in first["scorecam"] + (float(lines[0][5]), float(lines[0][7])):
        assert np.isfinite(v) and 0.0 <= v <= 1.0
    assert T.run_causal(args, m, image, pred, families=["scorecam"]) == first                # two calls agree
