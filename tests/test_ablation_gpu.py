"""Occlusion maps and Ablation-CAM (-m gpu): the four kernels of csrc/occlusion.hip and csrc/ablation.hip against restatements in
torch / NumPy float64 written here (no reference program is involved), their refusals, tools/attribution.py occlusion and
ablationcam on whole models against the float64 definitions over the HIP path's own outputs, the two *_maps functions and
tools/ablation.py in both modes.

Bounds.  The two batch writers select: bit equality.  occlusion_finish adds T covering windows in float64, divides and rounds to
fp32 once: |got - ref| <= 2^-24 |ref| + (T + 2) 2^-53 sum|terms| / count.  ablation_contract rounds a weight once and adds C fmas:
|got - ref| <= (C + 2) 2^-24 sum_c |w_c A[p, c]|, and exactly 0 where every term is 0.

Whole models.  With of="log_prob" the terms of `occlusion` are differences of two fp32 numbers, exact in float64, so the reference
is formed on the host alone.  With of="prob" a term is exp(a) - exp(b) in float64 and no two libraries promise the same last bit of
exp, while the bound above is relative to the MEAN of terms that largely cancel; so there the terms are those kernels.output_deltas
forms from the same outputs (the definition, F evaluated by the library's own float64 exp), the bound is unchanged, and the terms
themselves are checked against the host's float64 exp to 2 ulp of each exponential (one for either library), 2^-51 (exp(a) +
exp(b)).  The bound of
`ablationcam` is relative to the sum of |terms|, which 2^-52 cannot reach, so its reference is formed on the host alone."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import LAMBDA                                        # noqa: E402

SENTINEL = -777.25
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def case_id(c):
    return "x".join(str(v) for v in c)


def bits(t):
    return t.contiguous().view(torch.int32)


def counts(H, W, wh, ww, sy, sx):
    """(ny, nx) of the definition: 1 + ceil((size - window) / stride) per axis"""
    return 1 + -(-(H - wh) // sy), 1 + -(-(W - ww) // sx)


def window_box(n, H, W, wh, ww, sy, sx):
    nx = counts(H, W, wh, ww, sy, sx)[1]
    iy, ix = divmod(n, nx)
    return iy * sy, min(iy * sy + wh, H), ix * sx, min(ix * sx + ww, W)


# ------------------------------------------------------------------------------------------------ 1: K.occlude_images
# (C, H, W, wh, ww, sy, sx); the last: W a multiple of 4 and windows whose left edges 3, 6, 9 are no multiple of 4
OCC_CASES = [(1, 5, 7, 2, 3, 1, 2), (3, 33, 47, 16, 16, 8, 8), (3, 64, 64, 16, 16, 8, 8), (1, 16, 16, 16, 16, 16, 16),
             (2, 11, 9, 4, 4, 3, 4), (1, 8, 12, 3, 5, 2, 3)]


def occlusion_image(case, seed=0):
    """a random image with a -0.0 and a NaN of its own payload in it (a copy must keep both); the first case sits one float off a
    16-byte boundary"""
    C, H, W = case[:3]
    base = torch.randn(C * H * W + 1, generator=torch.Generator().manual_seed(7000 + seed)).cuda()
    image = base[1:] if case == OCC_CASES[0] else base[:-1].clone()
    image = image.view(C, H, W)
    if image.numel() > 2:
        image.view(-1)[1] = -0.0
        image.view(-1).view(torch.int32)[2] = 0x7FC12345
    return image


def occluded(image, first, n, geometry, fill):
    """the copy-and-fill: [1 + n, C, H, W], row 0 the image, row 1 + j window first + j filled"""
    ref = image[None].repeat(1 + n, 1, 1, 1)
    for j in range(n):
        y0, y1, x0, x1 = window_box(first + j, image.shape[1], image.shape[2], *geometry)
        ref[1 + j, :, y0:y1, x0:x1] = fill
    return ref


def check_occlude(case, fill, seed=0):
    from scouter_amd import kernels as K
    C, H, W = case[:3]
    g = case[3:]
    ny, nx = counts(H, W, *g)
    N = ny * nx
    assert K.occlusion_windows((H, W), g[:2], g[2:]) == (ny, nx)
    image = occlusion_image(case, seed)
    for first, n in [(0, N)] + ([(N // 2, N - N // 2), (N - 1, 1)] if N > 1 else []):
        out = torch.full((n + 2, C, H, W), SENTINEL, device="cuda")
        got = K.occlude_images(image, out[:1 + n], first, g[:2], g[2:], fill)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and bool((out[1 + n] == SENTINEL).all())   # the row behind keeps the sentinel
        assert torch.equal(bits(out[:1 + n]), bits(occluded(image, first, n, g, fill))), (case, first, n)


@pytest.mark.parametrize("fill", [0.0, -1.5])
@pytest.mark.parametrize("case", OCC_CASES, ids=case_id)
def test_occlude_images_equal_copy_and_fill(case, fill):
    check_occlude(case, fill)


def test_occlude_images_window_may_be_an_int():
    from scouter_amd import kernels as K
    image = occlusion_image((3, 64, 64))
    a = K.occlude_images(image, torch.empty((50, 3, 64, 64), device="cuda"), 0, 16, 8, 0.5)
    b = K.occlude_images(image, torch.empty((50, 3, 64, 64), device="cuda"), 0, (16, 16), [8, 8], 0.5)
    assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 2: K.ablate_channels
# (h, w, C, first, n); n None: all C channels in one call, and split
ABL_CASES = [(1, 1, 1, 0, None), (2, 3, 5, 0, None), (7, 7, 512, 0, None), (9, 9, 64, 0, None), (7, 7, 2048, 2040, 8)]


def ablation_features(h, w, C, seed=0, unaligned=False):
    base = torch.randn(h * w * C + 1, generator=torch.Generator().manual_seed(7100 + seed)).cuda()
    feat = (base[1:] if unaligned else base[:-1].clone()).view(h, w, C)
    if feat.numel() > 2:
        feat.view(-1)[1] = -0.0
        feat.view(-1).view(torch.int32)[2] = 0x7FC12345
    return feat


def ablated(feat, first, n):
    ref = feat[None].repeat(1 + n, 1, 1, 1)
    ref[torch.arange(1, 1 + n), :, :, torch.arange(first, first + n)] = 0.0
    return ref


def check_ablate(case, seed=0, unaligned=False):
    from scouter_amd import kernels as K
    h, w, C, first, n = case
    feat = ablation_features(h, w, C, seed, unaligned)
    calls = [(first, n)] if n is not None else [(0, C)] + ([(C // 2, C - C // 2), (C - 1, 1)] if C > 1 else [])
    for f, m in calls:
        out = torch.full((m + 2, h, w, C), SENTINEL, device="cuda")
        got = K.ablate_channels(feat, out[:1 + m], f)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and bool((out[1 + m] == SENTINEL).all())
        assert torch.equal(bits(out[:1 + m]), bits(ablated(feat, f, m))), (case, f, m)
        zeroed = out[torch.arange(1, 1 + m), :, :, torch.arange(f, f + m)]
        assert bool((bits(zeroed) == 0).all())                                  # +0.0, whatever stood there


@pytest.mark.parametrize("case", ABL_CASES, ids=case_id)
def test_ablate_channels_equal_copy_and_zero(case):
    check_ablate(case)


def test_ablate_channels_off_a_16_byte_boundary():
    """C a multiple of 4 but the features one float off: the one-element path, the same bits"""
    check_ablate((9, 9, 64, 0, None), unaligned=True)


# ------------------------------------------------------------------------------------------------ 3: K.occlusion_finish
def finish64(deltas, H, W, geometry):
    """(the mean over the covering windows, sum|terms| / count, the number of covering windows T) in float64: every window adds
    its delta to the pixels it covers, windows in ascending order -- per pixel iy ascending, then ix ascending"""
    Kc, N = deltas.shape
    acc, mag, cnt = np.zeros((Kc, H, W)), np.zeros((Kc, H, W)), np.zeros((H, W))
    for n in range(N):
        y0, y1, x0, x1 = window_box(n, H, W, *geometry)
        acc[:, y0:y1, x0:x1] += deltas[:, n, None, None]
        mag[:, y0:y1, x0:x1] += np.abs(deltas[:, n, None, None])
        cnt[y0:y1, x0:x1] += 1
    assert cnt.min() >= 1
    return acc / cnt, mag / cnt, cnt


def finish_bound(ref, mag, cnt):
    return EPS32 * np.abs(ref) + (cnt + 2) * EPS64 * mag


def check_finish(case, Kc, seed=0):
    from scouter_amd import kernels as K
    _, H, W = case[:3]
    g = case[3:]
    ny, nx = counts(H, W, *g)
    deltas = np.random.default_rng(7200 + seed).standard_normal((Kc, ny * nx))
    ref, mag, cnt = finish64(deltas, H, W, g)
    d = torch.from_numpy(deltas).cuda()
    out = torch.full((Kc + 1, H, W), SENTINEL, device="cuda")
    got = K.occlusion_finish(d, out[:Kc], g[:2], g[2:])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[Kc] == SENTINEL).all())
    err, bound = np.abs(out[:Kc].cpu().double().numpy() - ref), finish_bound(ref, mag, cnt)
    print("occlusion_finish", case, Kc, "max err %.3e, max err / bound %.3f" % (err.max(), (err / bound).max()))
    assert (err <= bound).all(), (err.max(), (err / bound).max())
    again = K.occlusion_finish(d, torch.full((Kc, H, W), 3.0, device="cuda"), g[:2], g[2:])          # overwritten, the same bits
    assert torch.equal(bits(again), bits(out[:Kc]))


@pytest.mark.parametrize("Kc", [1, 3])
@pytest.mark.parametrize("case", OCC_CASES, ids=case_id)
def test_occlusion_finish_against_fp64(case, Kc):
    check_finish(case, Kc)


# ------------------------------------------------------------------------------------------------ 4: K.ablation_contract
# (K, h, w, C): the issue's four, then two class tiles with a ragged last piece of channels, and two blocks of positions
CONTRACT_CASES = [(1, 1, 1, 1), (3, 2, 2, 5), (10, 7, 7, 512), (2, 9, 9, 2048), (20, 2, 2, 40), (2, 15, 20, 8)]


def check_contract(case, relu, seed=0):
    from scouter_amd import kernels as K
    Kc, h, w, C = case
    P, n_classes = h * w, 12
    gen = torch.Generator().manual_seed(7300 + seed)
    deltas = 0.1 * torch.randn((Kc, C), generator=gen, dtype=torch.float64)
    clean = torch.log_softmax(torch.randn(n_classes, generator=gen), dim=0)
    cols = torch.randint(0, n_classes, (Kc,), generator=gen).to(torch.int32)
    feat = torch.randn((h, w, C), generator=gen).clamp_min(0.0)              # post-ReLU features: about half the values are 0
    if P > 1:
        feat[0, 0] = 0.0                                                    # a position where every term is 0
    w64 = deltas / clean.double()[cols.long()].exp()[:, None]
    terms = w64[:, None, :] * feat.double().view(1, P, C)
    ref, mag = terms.sum(dim=2), terms.abs().sum(dim=2)
    if relu:
        ref = ref.clamp_min(0.0)                                            # (the clamp moves no two numbers apart)
    bound = (C + 2) * EPS32 * mag
    out = torch.full((Kc + 1, h, w), SENTINEL, device="cuda")
    args = (deltas.cuda(), clean.cuda(), cols.cuda(), feat.cuda())
    got = K.ablation_contract(*args, out[:Kc], relu)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[Kc] == SENTINEL).all())
    res = out[:Kc].cpu().double().view(Kc, P)
    err = (res - ref).abs()
    print("ablation_contract", case, relu, "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    assert bool((res[mag == 0] == 0).all()) and (P == 1 or bool((mag[:, 0] == 0).all()))
    if relu:
        assert float(res.min()) >= 0.0
    elif C > 1:
        assert float(res.min()) < 0.0
    again = K.ablation_contract(*args, torch.full((Kc, h, w), 3.0, device="cuda"), relu)             # overwritten, the same bits
    assert torch.equal(bits(again), bits(out[:Kc]))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "signed"])
@pytest.mark.parametrize("case", CONTRACT_CASES, ids=case_id)
def test_ablation_contract_against_fp64(case, relu):
    check_contract(case, relu)


# ------------------------------------------------------------------------------------------------ 5: refusals
REFUSALS = [(call, bad) for call, bads in [
    ("occlude_images", ["null", "misaligned", "n0", "past_end", "negative_first", "stride_above_window", "window_above_size",
                        "stride0", "nan_fill"]),
    ("occlusion_finish", ["null", "misaligned", "k0", "stride_above_window", "window_above_size", "stride0", "wrong_n"]),
    ("ablate_channels", ["null", "misaligned", "n0", "past_end", "negative_first"]),
    ("ablation_contract", ["null", "misaligned", "k0", "no_classes", "wrong_c"])] for bad in bads]


@pytest.mark.parametrize("call,bad", REFUSALS, ids=["%s-%s" % r for r in REFUSALS])
def test_the_kernels_refuse_bad_arguments(call, bad):
    """error returns with nothing launched: an error that names the call from the library itself and from the wrapper, the
    sentinel-filled output untouched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    lib = _native.lib()
    C, H, W, h, w, Cf, Kc, n_classes = 2, 20, 24, 3, 3, 8, 2, 5
    wh, ww, sy, sx = {"stride_above_window": (4, 4, 5, 2), "window_above_size": (21, 4, 2, 2), "stride0": (4, 4, 2, 0)}.get(
        bad, (4, 4, 2, 2))
    geometry_ok = bad not in ("stride_above_window", "window_above_size", "stride0")
    ny, nx = counts(H, W, 4, 4, 2, 2)
    N = ny * nx
    image = torch.ones((C, H, W), device="cuda")
    feat = torch.ones((h, w, Cf), device="cuda")
    batch = torch.full((4, C, H, W), SENTINEL, device="cuda")
    rows = torch.full((4, h, w, Cf), SENTINEL, device="cuda")
    deltas = torch.zeros((Kc, N), dtype=torch.float64, device="cuda")
    fdeltas = torch.zeros((Kc, Cf), dtype=torch.float64, device="cuda")
    smap = torch.full((Kc, H, W), SENTINEL, device="cuda")
    cam = torch.full((Kc, h, w), SENTINEL, device="cuda")
    clean = torch.zeros(n_classes, device="cuda")
    cols = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    first, n = {"past_end": (N - 2, 3), "negative_first": (-1, 3), "n0": (0, 0)}.get(bad, (0, 3))
    ffirst = Cf - 2 if bad == "past_end" else first
    odd = 2 if bad == "misaligned" else 0

    def ptr(t, null=False):
        return None if null and bad == "null" else t.data_ptr()

    def direct():
        if call == "occlude_images":
            return lib.scouter_occlude_images_f32(ptr(image), ptr(batch, True) and ptr(batch) + odd, first, n, C, H, W, wh, ww, sy, sx,
                                                  float("nan") if bad == "nan_fill" else 0.0, None)
        if call == "occlusion_finish":
            return lib.scouter_occlusion_finish_f32(ptr(deltas, True) and ptr(deltas) + 2 * odd, ptr(smap), 0 if bad == "k0" else Kc, H, W,
                                                    wh, ww, sy, sx, None)
        if call == "ablate_channels":
            return lib.scouter_ablate_channels_f32(ptr(feat, True) and ptr(feat) + odd, ptr(rows), ffirst, n, h * w, Cf, None)
        return lib.scouter_ablation_contract_f32(ptr(fdeltas), ptr(clean), ptr(cols, True) and ptr(cols) + odd, ptr(feat), ptr(cam),
                                                 0 if bad == "k0" else Kc, 0 if bad == "no_classes" else n_classes, h * w, Cf, 1, None)

    def wrapped():
        if call == "occlude_images":
            return K.occlude_images(image, batch[:1 + n], first, (wh, ww), (sy, sx), float("nan") if bad == "nan_fill" else 0.0)
        if call == "occlusion_finish":
            k = 0 if bad == "k0" else Kc
            return K.occlusion_finish(deltas[:k, :N - 1] if bad == "wrong_n" else deltas[:k], smap[:k], (wh, ww), (sy, sx))
        if call == "ablate_channels":
            return K.ablate_channels(feat, rows[:1 + n], ffirst)
        k = 0 if bad == "k0" else Kc
        return K.ablation_contract(fdeltas[:k, :Cf - 1].contiguous() if bad == "wrong_c" else fdeltas[:k],
                                   clean[:0] if bad == "no_classes" else clean, cols[:k], feat, cam[:k])

    if bad not in ("wrong_n", "wrong_c"):                                  # (shapes: the wrapper's business alone)
        assert geometry_ok or call in ("occlude_images", "occlusion_finish")
        with pytest.raises(RuntimeError, match=call):
            _native.check(direct(), call)
    if bad not in ("null", "misaligned"):                                   # (a tensor has a pointer, and torch aligns it)
        with pytest.raises((RuntimeError, ValueError), match=call):
            wrapped()
    torch.cuda.synchronize()
    for t in (batch, rows, smap, cam):
        assert bool((t == SENTINEL).all())
    check_occlude(OCC_CASES[4], -1.5, seed=1)
    check_ablate(ABL_CASES[1], seed=1)
    check_finish(OCC_CASES[4], 3, seed=1)
    check_contract(CONTRACT_CASES[1], True, seed=1)


# ------------------------------------------------------------------------------------------------ 6: whole models
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


def state_is_untouched(m, before):
    after = bn_buffers(m)
    return m.training and before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before) and \
        all(p.grad is None for p in m.parameters())


OCC = dict(window=16, stride=8, batch=20)                                   # 7 x 7 = 49 windows: chunks of 19, 19 and 11
GEOMETRY = (16, 16, 8, 8)


def occlusion_outputs(m, images, fill=0.0):
    """[B][chunk] the model's own fp32 outputs [1 + n, classes] (on the device) for the chunks `occlusion` forms"""
    from scouter_amd import kernels as K
    B, C, H, W = images.shape
    N, step = 49, OCC["batch"] - 1
    was_training = m.training
    m.eval()
    try:
        with torch.no_grad():
            return [[m(K.occlude_images(images[b], torch.empty((1 + min(step, N - f), C, H, W), device="cuda"), f, 16, 8, fill))
                     .float().contiguous() for f in range(0, N, step)] for b in range(B)]
    finally:
        m.train(was_training)


def occlusion_terms(outs, of, on_device):
    """float64 [B, classes, N]: F(out[0]) - F(out[1 + j]) per chunk, on the host or by kernels.output_deltas"""
    from scouter_amd import kernels as K
    terms = []
    for chunks in outs:
        if on_device:
            n_out = chunks[0].shape[1]
            d = torch.zeros((n_out, 49), dtype=torch.float64, device="cuda")
            first = 0
            for o in chunks:
                K.output_deltas(o, torch.arange(n_out, dtype=torch.int32, device="cuda"), d, first, of)
                first += o.shape[0] - 1
            terms.append(d.cpu())
        else:
            f = [o.double().cpu().exp() if of == "prob" else o.double().cpu() for o in chunks]
            terms.append(torch.cat([(o[:1] - o[1:]).T for o in f], dim=1))
    return torch.stack(terms).numpy()


def check_occlusion_maps(S, terms, what):
    for b in range(S.shape[0]):
        ref, mag, cnt = finish64(terms[b], 64, 64, GEOMETRY)
        err, bound = np.abs(S[b].cpu().double().numpy() - ref), finish_bound(ref, mag, cnt)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)        # (every term 0: the bound is 0, and so is err)
        print("%s image %d: max err %.3e, max err / bound %.3f, terms that are exactly 0: %d of %d" %
              (what, b, err.max(), ratio.max(), int((terms[b] == 0).sum()), terms[b].size))
        assert (err <= bound).all(), (what, b, err.max(), ratio.max())


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_occlusion_on_whole_models(use_slot):
    from scouter_amd.tools.attribution import occlusion, occlusion_windows
    m, images = build(use_slot)
    assert occlusion_windows((64, 64), 16, 8) == (7, 7)
    m.train()
    outs = occlusion_outputs(m, images)
    assert [o.shape[0] for o in outs[0]] == [20, 20, 12]
    before = bn_buffers(m)
    S = occlusion(m, images, **OCC)
    torch.cuda.synchronize()
    # ---- the value, the shape, the state left behind
    assert tuple(S.shape) == (2, 10, 64, 64) and S.dtype == torch.float32 and S.is_cuda
    assert bool(torch.isfinite(S).all()) and float(S.max()) > 0 > float(S.min())
    terms = occlusion_terms(outs, "prob", True)
    host = occlusion_terms(outs, "prob", False)
    p = torch.stack([torch.cat([(o[:1].double().exp() + o[1:].double().exp()).T for o in chunks], dim=1) for chunks in outs])
    gap = np.abs(terms - host) / p.cpu().numpy()
    print("output_deltas against the host's float64 exp: max |difference| / (exp(a) + exp(b)) = %.3e" % gap.max())
    assert gap.max() <= 2.0 ** -51
    check_occlusion_maps(S, terms, "occlusion prob %s" % ("slot" if use_slot else "fc"))
    err_host = max(np.abs(S[b].cpu().double().numpy() - finish64(host[b], 64, 64, GEOMETRY)[0]).max() for b in range(2))
    print("against the terms formed on the host: max err %.3e" % err_host)
    assert state_is_untouched(m, before)
    # ---- the log-probability: exact terms, the reference formed on the host alone
    L = occlusion(m, images, of="log_prob", **OCC)
    check_occlusion_maps(L, occlusion_terms(outs, "log_prob", False), "occlusion log_prob %s" % ("slot" if use_slot else "fc"))
    assert not torch.equal(L, S)
    # ---- reproducibility and class selection
    assert torch.equal(bits(occlusion(m, images, **OCC)), bits(S))
    two = occlusion(m, images, classes=[0, 3], **OCC)
    assert tuple(two.shape) == (2, 2, 64, 64) and torch.equal(two[:, 0], S[:, 0]) and torch.equal(two[:, 1], S[:, 3])
    own = occlusion(m, images, classes=torch.tensor([7, 2]), **OCC)
    assert tuple(own.shape) == (2, 1, 64, 64) and torch.equal(own[0, 0], S[0, 7]) and torch.equal(own[1, 0], S[1, 2])
    pair = occlusion(m, images, classes=[1], window=(16, 16), stride=(8, 8), batch=20)
    assert torch.equal(pair[:, 0], S[:, 1])
    filled = occlusion(m, images, classes=[1], fill=-1.5, **OCC)
    assert bool(torch.isfinite(filled).all()) and not torch.equal(filled[:, 0], S[:, 1])
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            occlusion(m, images, classes=bad, **OCC)
    with pytest.raises(ValueError):
        occlusion(m, images, classes=torch.tensor([0, 1, 2]), **OCC)
    with pytest.raises(ValueError, match="batch"):
        occlusion(m, images, window=16, stride=8, batch=1)
    for window, stride in ((16, 17), (65, 8), (16, 0), ((16, 65), 8), (16, (8, 17))):
        with pytest.raises(ValueError, match="stride"):
            occlusion(m, images, window=window, stride=stride)
    with pytest.raises(ValueError, match="of"):
        occlusion(m, images, of="logit", **OCC)
    assert state_is_untouched(m, before)
    # ---- BatchNorm-folded forwards: a map value is a mean of differences of two probabilities, each within e of the unfolded one
    m.set_inference_fold(True)
    folded = occlusion(m, images, **OCC)
    outs_folded = occlusion_outputs(m, images)
    m.set_inference_fold(False)
    e = max(float((a.double().exp() - b.double().exp()).abs().max()) for ca, cb in zip(outs, outs_folded) for a, b in zip(ca, cb))
    diff, top = float((folded - S).abs().max()), float(S.abs().max())
    print("occlusion folded against unfolded: max difference %.3e, e %.3e, max|S| %.3e" % (diff, e, top))
    assert diff <= 2 * e + 2.0 ** -23 * top
    assert state_is_untouched(m, before)


ABL_BATCH = 128                                                             # C = 512: chunks of 127, 127, 127, 127 and 4


def ablation_reference(m, images, relu):
    """(float64 [B, classes, P] the definition, its bound): one feature pass, the ablated chunks through head_pass, the weights
    and the sum over the channels in float64 on the host -- all over the HIP path's own features and outputs"""
    from scouter_amd import kernels as K
    fp = m.feature_pass(images)
    feat, clean = fp.features.detach().contiguous(), fp.log_probs.detach().double().cpu()
    B, h, w, C = feat.shape
    step, refs, bounds, chunks = ABL_BATCH - 1, [], [], 0
    for b in range(B):
        drops = []
        for f in range(0, C, step):
            chunk = K.ablate_channels(feat[b], torch.empty((1 + min(step, C - f), h, w, C), device="cuda"), f)
            p = m.head_pass(chunk).log_probs.double().cpu().exp()
            drops.append((p[:1] - p[1:]).T)
            chunks += 1
        w64 = torch.cat(drops, dim=1) / clean[b].exp()[:, None]               # [classes, C]
        terms = w64[:, None, :] * feat[b].double().cpu().view(1, h * w, C)
        ref = terms.sum(dim=2)
        refs.append(ref.clamp_min(0.0) if relu else ref)
        bounds.append((C + 2) * EPS32 * terms.abs().sum(dim=2))
    assert (C, chunks) == (512, 5 * B)
    return torch.stack(refs), torch.stack(bounds), (h, w)


def check_ablationcam(m, images, relu, what):
    from scouter_amd.tools.attribution import ablationcam
    ref, bound, (h, w) = ablation_reference(m, images, relu)
    S = ablationcam(m, images, batch=ABL_BATCH, relu=relu)
    torch.cuda.synchronize()
    assert tuple(S.shape) == (2, 10, h, w) and S.dtype == torch.float32 and S.is_cuda and bool(torch.isfinite(S).all())
    err = (S.cpu().double().view(2, 10, h * w) - ref).abs()
    print("%s: max err %.3e, max err / bound %.3f, max|S| %.3e" %
          (what, float(err.max()), float((err / bound.clamp_min(1e-300)).max()), float(S.abs().max())))
    assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    return S


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_ablationcam_on_whole_models(use_slot):
    from scouter_amd.tools.attribution import ablationcam
    m, images = build(use_slot)
    name = "slot" if use_slot else "fc"
    m.train()
    before = bn_buffers(m)
    S = check_ablationcam(m, images, True, "ablationcam %s" % name)
    assert float(S.min()) >= 0.0 and float(S.max()) > 0.0
    assert state_is_untouched(m, before)
    signed = check_ablationcam(m, images, False, "ablationcam %s, no relu" % name)
    assert torch.equal(signed.clamp_min(0.0), S)
    # ---- reproducibility and class selection
    assert torch.equal(bits(ablationcam(m, images, batch=ABL_BATCH)), bits(S))
    two = ablationcam(m, images, classes=[0, 3], batch=ABL_BATCH)
    assert tuple(two.shape) == (2, 2) + tuple(S.shape[2:]) and torch.equal(two[:, 0], S[:, 0]) and torch.equal(two[:, 1], S[:, 3])
    own = ablationcam(m, images, classes=torch.tensor([7, 2]), batch=ABL_BATCH)
    assert tuple(own.shape) == (2, 1) + tuple(S.shape[2:]) and torch.equal(own[0, 0], S[0, 7]) and torch.equal(own[1, 0], S[1, 2])
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            ablationcam(m, images, classes=bad, batch=ABL_BATCH)
    with pytest.raises(ValueError):
        ablationcam(m, images, classes=torch.tensor([0, 1, 2]), batch=ABL_BATCH)
    with pytest.raises(ValueError, match="batch"):
        ablationcam(m, images, batch=1)
    assert state_is_untouched(m, before)
    # ---- BatchNorm-folded: the same test against the folded feature pass's own features
    m.set_inference_fold(True)
    try:
        folded = check_ablationcam(m, images, True, "ablationcam %s, folded" % name)
    finally:
        m.set_inference_fold(False)
    assert tuple(folded.shape) == tuple(S.shape)
    assert state_is_untouched(m, before)


# ------------------------------------------------------------------------------------------------ 7: maps and the tool
TOOL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--occlusion", "true", "--ablationcam",
        "true", "--occlusion_batch", "20", "--ablationcam_batch", "128", "--grad_min_level", "0.2", "--eval_fold", "true"]


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_the_maps_and_the_tool_on_one_image(use_slot, tmp_path, monkeypatch, capsys):
    """occlusion_maps / ablationcam_maps are K.heat_maps / K.cam_maps of the float results, bytewise; --table_images 0 (the
    default) writes occlusion_{c}.png and ablationcam_{c}.png of every class, those bytes, no other family's files, and one causal
    line per row"""
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.tools import ablation as A
    from scouter_amd.tools.attribution import ablationcam, ablationcam_maps, occlusion, occlusion_maps
    vis_dir = str(tmp_path / "vis")
    argv = ["ablation.py"] + TOOL + ["--use_slot", "true" if use_slot else "false", "--causal", "true", "--causal_step", "2048",
                                     "--vis_dir", vis_dir, "--output_dir", str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    A.main()
    out = capsys.readouterr().out
    names = (["slot"] if use_slot else []) + ["occlusion", "ablationcam"]
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("causal ")]
    assert [ln[1] for ln in lines] == names, lines
    for ln in lines:
        values = [float(v) for v in ln[4:] if v[0].isdigit() or v[0] == "-"]
        assert len(values) == 2 and all(math.isfinite(v) for v in values), ln
    assert sorted(os.listdir(vis_dir)) == sorted("%s_%d.png" % (n, c) for n in names for c in range(10))
    # the bytes: the library's maps of the same image under the same options and the same weights
    args = A.get_ablation_parser().parse_args(argv[1:])
    assert A.option_kwargs(args, "occlusion") == dict(window=16, stride=8, fill=0.0, batch=20)
    assert A.option_kwargs(args, "ablationcam") == dict(batch=128)
    torch.manual_seed(11)
    model, _ = T.build_model(args)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))[None].cuda()
    want = {"occlusion": occlusion_maps(model, x, min_level=0.2, **A.option_kwargs(args, "occlusion")),
            "ablationcam": ablationcam_maps(model, x, min_level=0.2, **A.option_kwargs(args, "ablationcam"))}
    assert torch.equal(want["occlusion"], K.heat_maps(occlusion(model, x, **OCC), 0.2))
    assert torch.equal(want["ablationcam"], K.cam_maps(ablationcam(model, x, batch=128), 64, 64, 0.2))
    assert torch.equal(ablationcam_maps(model, x, classes=[2, 5], size=(32, 48), batch=128),
                       K.cam_maps(ablationcam(model, x, classes=[2, 5], batch=128), 32, 48, 0.0))
    assert torch.equal(occlusion_maps(model, x, classes=[2, 5], **OCC), K.heat_maps(occlusion(model, x, classes=[2, 5], **OCC), 0.0))
    for name, maps in want.items():
        maps = maps[0].cpu().numpy()
        assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and any(m.any() for m in maps)
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(vis_dir, "%s_%d.png" % (name, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, maps[c]), (name, c)


def test_the_tool_on_a_table(tmp_path, monkeypatch, capsys):
    """--table_images 2 on synthetic data: the rows `table occlusion:` and `table ablationcam:` after the table's own"""
    from scouter_amd.tools import ablation as A
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["ablation.py"] + TOOL + [
        "--use_slot", "true", "--synthetic_data", "true", "--num_workers", "0", "--table_images", "2", "--batch_size", "2",
        "--localization", "true", "--output_dir", str(tmp_path / "none")])
    result = A.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == ["slot:", "occlusion:", "ablationcam:", "accuracy"]
    for ln in lines[1:3]:
        words = ln.split()
        assert words[2:4] == ["images", "2"] and words[4] == "area" and 0.0 <= float(words[5]) <= 1.0
    for name in ("occlusion", "ablationcam"):
        cols = result.rows[name]
        assert all(v.dtype == np.float64 and v.shape == (2,) for v in cols.values())
        assert ((cols["area"] >= 0) & (cols["area"] <= 1)).all()
