"""RISE (-m gpu): the three kernels of csrc/rise.hip against fp64 -- kernels.rise_mask_images and kernels.rise_accumulate against
masks stated with F.interpolate in float64 (no reference program is involved), kernels.heat_maps against a float64 NumPy
restatement of the drawing steps and against kernels.cam_maps at the map's own size -- their refusals, tools/attribution.py
rise on whole models against the same fp64 sum over the HIP path's own log-probabilities, and rise_maps / test.py --rise true.

Bounds.  A mask value is one rounding of the scale, one fma per coordinate, three interpolation roundings; with the final
product the worst case is (4 s + 7) 2^-24 of the image value, and the tests allow twice that, (8 s + 8) 2^-24 |image value|
(bilinear interpolation is continuous across cell borders, so a coordinate that rounds to the other side of an integer stays
inside it).  The accumulation adds N non-negative terms, so its bound is relative: (N + 8 s + 16) 2^-24 ref, and exactly 0
where ref is exactly 0."""
import argparse
import os
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


def cells(H, W, s):
    return -(-H // s), -(-W // s)


def draws(N, H, W, s, seed, p=0.5):
    """grids uint8 [N, s, s] and shifts int32 [N, 2] in the order rise_masks draws them; the two extreme shifts are forced into
    the first two masks (N >= 2)"""
    ch, cw = cells(H, W, s)
    gen = torch.Generator().manual_seed(seed)
    grids = (torch.rand(N, s, s, generator=gen) < p).to(torch.uint8)
    shifts = torch.stack([torch.randint(0, ch, (N,), generator=gen), torch.randint(0, cw, (N,), generator=gen)], dim=1)
    shifts = shifts.to(torch.int32)
    shifts[0] = torch.tensor([0, 0], dtype=torch.int32)
    shifts[1] = torch.tensor([ch - 1, cw - 1], dtype=torch.int32)
    return grids, shifts


def masks_fp64(grids, shifts, H, W):
    """[N, H, W] float64: the definition, one F.interpolate per mask"""
    N, s, _ = grids.shape
    ch, cw = cells(H, W, s)
    out = torch.empty((N, H, W), dtype=torch.float64)
    for n in range(N):
        up = F.interpolate(grids[n][None, None].double(), size=((s + 1) * ch, (s + 1) * cw), mode="bilinear", align_corners=False)
        dy, dx = int(shifts[n, 0]), int(shifts[n, 1])
        out[n] = up[0, 0, dy:dy + H, dx:dx + W]
    return out


# ------------------------------------------------------------------------------------------------ 1: K.rise_mask_images
MASK_CASES = [(1, 5, 7, 2, 3), (3, 33, 47, 7, 5), (1, 64, 64, 7, 64), (3, 224, 224, 7, 2), (2, 9, 9, 1, 4), (1, 16, 16, 16, 3)]


def _check_mask_images(case, seed=0):
    from scouter_amd import kernels as K
    C, H, W, s, N = case
    image = torch.randn((C, H, W), generator=torch.Generator().manual_seed(6000 + seed))
    grids, shifts = draws(N, H, W, s, 6100 + seed)
    ref = image.double()[None] * masks_fp64(grids, shifts, H, W)[:, None]
    bound = (8 * s + 8) * EPS * image.double().abs()[None].expand_as(ref)
    out = torch.full((N + 1, C, H, W), SENTINEL, device="cuda")
    got = K.rise_mask_images(image.cuda(), grids.cuda(), shifts.cuda(), out[:N], s)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and bool((out[N] == SENTINEL).all())           # the extra image keeps the sentinel
    err = (out[:N].cpu().double() - ref).abs()
    print("rise_mask_images", case, "max err %.3e, max err / bound %.3f" %
          (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_rise_mask_images_against_fp64(case):
    _check_mask_images(case)


# ------------------------------------------------------------------------------------------------ 2: K.rise_accumulate
# (K, n_classes, H, W, s, N, the columns or None for 0 .. K - 1, acc starts from seeded non-zero values)
ACC_CASES = [(10, 10, 33, 47, 7, 70, None, True), (3, 200, 16, 16, 4, 300, [150, 7, 150], False),
             (200, 200, 8, 8, 2, 5, None, False), (1, 1, 224, 224, 7, 8, None, False)]


def check_accumulated(got, ref, N, s, what):
    """|got - ref| <= (N + 8 s + 16) 2^-24 ref, and exactly 0 where ref is exactly 0"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = (N + 8 * s + 16) * EPS * ref
    zero = ref == 0
    print("%s: max err %.3e, max err / bound %.3f, %d elements with an exactly zero reference" %
          (what, float(err.max()), float((err / bound.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.0,
           int(zero.sum())))
    assert bool((ref >= 0).all())
    assert bool((got[zero] == 0).all())
    assert bool((err <= bound).all()), (what, float(err.max()))


@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: "%dof%d_%dx%d_s%d_n%d" % c[:6])
def test_rise_accumulate_against_fp64(case):
    from scouter_amd import kernels as K
    Kc, n_classes, H, W, s, N, cols, seeded = case
    cols = torch.tensor(cols if cols is not None else list(range(Kc)), dtype=torch.int32)
    gen = torch.Generator().manual_seed(6200 + N)
    logp = F.log_softmax(torch.randn((N, n_classes), generator=gen), dim=1)
    grids, shifts = draws(N, H, W, s, 6300 + N)
    acc0 = torch.rand((Kc, H, W), generator=gen) + 0.25 if seeded else torch.zeros((Kc, H, W))
    scale = 1.0 / (N * 0.5)
    w = scale * logp.double().exp()[:, cols.long()]                                  # [N, K]
    ref = acc0.double() + torch.einsum("nk,nhw->khw", w, masks_fp64(grids, shifts, H, W))
    ld, cd, gd, sd = logp.cuda(), cols.cuda(), grids.cuda(), shifts.cuda()
    one = K.rise_accumulate(ld, cd, gd, sd, acc0.cuda(), s, scale)
    cut = N // 3
    two = acc0.cuda()
    K.rise_accumulate(ld[:cut], cd, gd[:cut], sd[:cut], two, s, scale)
    K.rise_accumulate(ld[cut:], cd, gd[cut:], sd[cut:], two, s, scale)
    again = K.rise_accumulate(ld, cd, gd, sd, acc0.cuda(), s, scale)
    torch.cuda.synchronize()
    check_accumulated(one, ref, N, s, "rise_accumulate %s" % (case[:6],))
    assert torch.equal(one, two) and torch.equal(one, again)      # split at any point, and a second call: the same bits
    if seeded:
        assert float((one.cpu() - acc0).min()) >= 0 and float((one.cpu() - acc0).max()) > 0
    # masks whose grids are all zero add exactly nothing
    same = K.rise_accumulate(ld, cd, torch.zeros_like(gd), sd, one.clone(), s, scale)
    assert torch.equal(same, one)


# ------------------------------------------------------------------------------------------------ 3: K.heat_maps
def _minmax64(a):
    span = a.max() - a.min()
    return (a - a.min()) / span if span > 0 else np.zeros_like(a)


def _heat_maps_restated(maps, min_level):
    """the five steps (cam_maps' six minus the resize), one map at a time, in float64 -> (uint8 maps, per map: is it live)"""
    maps = np.asarray(maps, dtype=np.float64)
    out = np.zeros(maps.shape, dtype=np.uint8)
    live = []
    for m in range(maps.shape[0]):
        v = np.maximum(maps[m], 0.0)
        live.append(bool(v.max() > v.min()) and min_level < 1.0)
        v = _minmax64(v)
        v = _minmax64(np.maximum(v, min_level))
        out[m] = (255.0 * v).astype(np.uint8)
    return out, live


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("min_level", [0.0, 0.3])
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (33, 47), (224, 224), (260, 260)], ids=lambda s: "%dx%d" % s)
def test_heat_maps_against_numpy(size, min_level, M):
    from scouter_amd import kernels as K
    H, W = size
    maps = torch.randn((M, H, W), generator=torch.Generator().manual_seed(29 + M))
    got = K.heat_maps(maps.cuda(), min_level)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (M, H, W) and got.is_cuda
    got = got.cpu().numpy()
    want, live = _heat_maps_restated(maps.numpy(), min_level)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print("heat_maps", size, min_level, M, "max grey-level difference", int(diff.max()), "pixels off", int((diff > 0).sum()))
    assert diff.max() <= 1
    for m in range(M):
        if live[m]:
            assert got[m].max() >= 254 and got[m].min() == 0
        else:
            assert not got[m].any()
    if H * W > 1 and M > 1:
        assert any(live)


@pytest.mark.parametrize("size", [(7, 7), (33, 47), (128, 128)], ids=lambda s: "%dx%d" % s)
def test_heat_maps_equal_cam_maps_at_the_maps_own_size(size):
    from scouter_amd import kernels as K
    h, w = size
    x = torch.randn((4, h, w), generator=torch.Generator().manual_seed(31)).cuda()
    for min_level in (0.0, 0.3):
        assert torch.equal(K.heat_maps(x, min_level), K.cam_maps(x, h, w, min_level))


@pytest.mark.parametrize("size", [(5, 3, 33, 47), (7, 7, 224, 224), (9, 9, 5, 7)], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_cam_maps_equal_heat_maps_of_the_resized_maps(size):
    """cam_maps never stores the resized map; resize_bilinear stores it.  Both form it with the same expression, so drawing the
    stored one gives cam_maps' bytes."""
    from scouter_amd import kernels as K
    h, w, H, W = size
    x = torch.randn((3, h, w), generator=torch.Generator().manual_seed(37)).cuda()
    assert bool(torch.isfinite(x).all()) and bool((x > 0).any()) and bool((x < 0).any())
    resized = K.resize_bilinear(x, H, W)
    for min_level in (0.0, 0.3):
        assert torch.equal(K.cam_maps(x, H, W, min_level), K.heat_maps(resized, min_level))


def test_heat_maps_edge_cases():
    from scouter_amd import kernels as K
    gen = torch.Generator().manual_seed(23)
    one = -torch.rand((7, 7), generator=gen)
    one[2, 4] = 0.8
    maps = torch.stack([torch.full((7, 7), 0.7), -torch.rand((7, 7), generator=gen) - 0.1, torch.zeros(7, 7), one]).cuda()
    for min_level in (0.0, 0.3):
        a, b = K.heat_maps(maps, min_level), K.heat_maps(maps, min_level)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        a = a.cpu().numpy()
        assert not a[0].any() and not a[1].any() and not a[2].any()      # constant, all negative, all zero
        want, live = _heat_maps_restated(maps.cpu().numpy(), min_level)
        assert live == [False, False, False, True]
        assert np.abs(a.astype(np.int64) - want.astype(np.int64)).max() <= 1
        assert a[3].any() and a[3].max() >= 254 and a[3].min() == 0      # one positive pixel: a non-zero map
    assert not K.heat_maps(maps, 1.0).cpu().numpy().any()                # min_level 1: constant at the second scaling
    lead = K.heat_maps(maps.view(2, 2, 7, 7), 0.0)                       # leading dimensions are kept
    assert tuple(lead.shape) == (2, 2, 7, 7) and torch.equal(lead.view(4, 7, 7), K.heat_maps(maps, 0.0))


# ------------------------------------------------------------------------------------------------ 4: refusals
@pytest.mark.parametrize("bad", ["null", "s0", "s17", "s_above_size", "shift_low", "shift_high"])
@pytest.mark.parametrize("call", ["rise_mask_images", "rise_accumulate"])
def test_rise_kernels_refuse_bad_arguments(call, bad):
    """a null pointer, s = 0, s = 17, s > min(H, W), a shift outside [0, cell): an error naming the call, the output untouched,
    and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    N, C, H, W, s = 3, 2, 20, 24, {"s0": 0, "s17": 17}.get(bad, 7)
    if bad == "s_above_size":
        H = 5
    image = torch.ones((C, H, W), device="cuda")
    grids = torch.ones((N, s, s), dtype=torch.uint8, device="cuda")
    shifts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    if bad == "shift_low":
        shifts[1, 1] = -1
    if bad == "shift_high":
        shifts[2, 0] = -(-H // s)                                        # = cell_h: one past the last shift
    out = torch.full((N, C, H, W), SENTINEL, device="cuda")
    acc = torch.full((4, H, W), SENTINEL, device="cuda")
    logp = torch.zeros((N, 6), device="cuda")
    cols = torch.tensor([0, 5, 2, 2], dtype=torch.int32, device="cuda")
    lib = _native.lib()
    with pytest.raises(RuntimeError, match=call):
        if call == "rise_mask_images":
            if bad == "null":
                _native.check(lib.scouter_rise_mask_images_f32(image.data_ptr(), None, shifts.data_ptr(), out.data_ptr(), N, C, H,
                                                               W, s, None), call)
            else:
                K.rise_mask_images(image, grids, shifts, out, s)
        else:
            if bad == "null":
                _native.check(lib.scouter_rise_accumulate_f32(logp.data_ptr(), cols.data_ptr(), grids.data_ptr(),
                                                              shifts.data_ptr(), None, N, 6, 4, H, W, s, 1.0, None), call)
            else:
                K.rise_accumulate(logp, cols, grids, shifts, acc, s, 1.0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((acc == SENTINEL).all())
    _check_mask_images((3, 33, 47, 7, 5), seed=1)


def test_rise_accumulate_refuses_no_classes_and_heat_maps_a_null_pointer():
    from scouter_amd import _native
    from scouter_amd import kernels as K
    lib = _native.lib()
    N, H, W, s = 3, 20, 24, 7
    grids = torch.ones((N, s, s), dtype=torch.uint8, device="cuda")
    shifts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    logp = torch.zeros((N, 6), device="cuda")
    cols = torch.zeros(4, dtype=torch.int32, device="cuda")
    acc = torch.full((4, H, W), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="rise_accumulate"):           # K = 0 at the library, with every pointer valid
        _native.check(lib.scouter_rise_accumulate_f32(logp.data_ptr(), cols.data_ptr(), grids.data_ptr(), shifts.data_ptr(),
                                                      acc.data_ptr(), N, 6, 0, H, W, s, 1.0, None), "rise_accumulate")
    with pytest.raises(RuntimeError, match="rise_accumulate"):           # and through the wrapper
        K.rise_accumulate(logp, cols[:0], grids, shifts, acc[:0], s, 1.0)
    maps = torch.ones((2, H, W), device="cuda")
    out = torch.full((2, H, W), 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="heat_maps"):
        _native.check(lib.scouter_heat_maps_u8(None, out.data_ptr(), 2, H, W, 0.0, None), "heat_maps")
    with pytest.raises(RuntimeError, match="heat_maps"):
        _native.check(lib.scouter_heat_maps_u8(maps.data_ptr(), out.data_ptr(), 0, H, W, 0.0, None), "heat_maps")
    with pytest.raises(RuntimeError, match="heat_maps"):
        K.heat_maps(torch.ones(5, device="cuda"))
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all()) and bool((out == 77).all())
    _check_mask_images((1, 5, 7, 2, 3), seed=2)


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


def expected_rise(m, images, masks, batch):
    """fp64 [B, n, H, W]: the definition's sum over the HIP path's own log-probabilities -- the same chunks built with
    K.rise_mask_images, the model in eval mode under no_grad at the same batch, F.interpolate masks in float64"""
    from scouter_amd import kernels as K
    B, C, H, W = images.shape
    N = masks.grids.shape[0]
    m64 = masks_fp64(masks.grids.cpu(), masks.shifts.cpu(), H, W)
    was_training = m.training
    m.eval()
    ref = []
    try:
        with torch.no_grad():
            for b in range(B):
                logp = []
                for n0 in range(0, N, batch):
                    g, sh = masks.grids[n0:n0 + batch], masks.shifts[n0:n0 + batch]
                    chunk = K.rise_mask_images(images[b], g, sh, torch.empty((g.shape[0], C, H, W), device="cuda"), masks.s)
                    logp.append(m(chunk).cpu().double())
                ref.append(torch.einsum("nk,nhw->khw", torch.cat(logp).exp(), m64) / (N * masks.p))
    finally:
        m.train(was_training)
    return torch.stack(ref)


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_rise_on_whole_models(use_slot):
    from scouter_amd.tools.attribution import rise, rise_masks
    m, images = build(use_slot)
    N, s, batch = 64, 7, 32
    masks = rise_masks(N, (64, 64), s=s, p=0.5, seed=0, device="cuda")
    assert masks.grids.dtype == torch.uint8 and tuple(masks.grids.shape) == (N, s, s) and int(masks.grids.max()) == 1
    assert masks.shifts.dtype == torch.int32 and tuple(masks.shifts.shape) == (N, 2)
    assert (masks.s, masks.p, tuple(masks.size), tuple(masks.cell)) == (s, 0.5, (64, 64), (10, 10))
    assert int(masks.shifts.min()) >= 0 and int(masks.shifts.max()) < 10
    m.train()
    ref = expected_rise(m, images, masks, batch)
    before = bn_buffers(m)
    S = rise(m, images, n_masks=N, s=s, batch=batch, seed=0)
    torch.cuda.synchronize()
    # ---- the value, the shape, the state left behind
    assert tuple(S.shape) == (2, 10, 64, 64) and S.dtype == torch.float32 and S.is_cuda
    assert bool(torch.isfinite(S).all()) and float(S.max()) > float(S.min())
    check_accumulated(S, ref, N, s, "rise %s" % ("slot" if use_slot else "fc"))
    assert m.training
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in m.parameters())
    # ---- reproducibility and class selection
    assert torch.equal(rise(m, images, n_masks=N, s=s, batch=batch, seed=0), S)
    assert not torch.equal(rise(m, images, n_masks=N, s=s, batch=batch, seed=1), S)
    assert torch.equal(rise(m, images, batch=batch, masks=masks), S)
    two = rise(m, images, classes=[0, 3], n_masks=N, s=s, batch=batch, seed=0)
    assert tuple(two.shape) == (2, 2, 64, 64) and torch.equal(two[:, 0], S[:, 0]) and torch.equal(two[:, 1], S[:, 3])
    cls = torch.tensor([7, 2])
    own = rise(m, images, classes=cls, n_masks=N, s=s, batch=batch, seed=0)
    assert tuple(own.shape) == (2, 1, 64, 64) and torch.equal(own[0, 0], S[0, 7]) and torch.equal(own[1, 0], S[1, 2])
    short = rise(m, images, classes=[1], n_masks=48, s=s, batch=batch, seed=0)           # a short last chunk
    assert tuple(short.shape) == (2, 1, 64, 64) and bool(torch.isfinite(short).all()) and float(short.max()) > 0
    for bad in ([10], [-1], torch.tensor([0, 10])):
        with pytest.raises(IndexError):
            rise(m, images, classes=bad, n_masks=N, s=s, batch=batch)
    with pytest.raises(ValueError):
        rise(m, images, classes=torch.tensor([0, 1, 2]), n_masks=N, s=s, batch=batch)
    assert m.training and all(p.grad is None for p in m.parameters())
    # ---- BatchNorm-folded forwards: the fold's forward tolerance carried through a convex combination of masks
    m.set_inference_fold(True)
    folded = rise(m, images, n_masks=N, s=s, batch=batch, seed=0)
    m.set_inference_fold(False)
    diff, top = float((folded - S).abs().max()), float(S.abs().max())
    print("rise folded against unfolded: max difference %.3e, max|S| %.3e, ratio %.3e" % (diff, top, diff / top))
    assert diff <= 1e-3 * top
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 6: maps and the CLI
@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_rise_maps_and_test_tool(use_slot, tmp_path, monkeypatch):
    """rise_maps is K.heat_maps of rise, bytewise; scouter_amd.test run_rise / --rise true write rise_0.png .. rise_9.png,
    64 x 64, byte for byte rise_maps of the image"""
    from PIL import Image
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools.attribution import rise, rise_maps
    torch.manual_seed(11)
    args = model_args(use_slot)
    args.device, args.grad_min_level, args.rise_masks, args.rise_batch = "cuda", 0.2, 64, 32
    model = SlotModel(args).to(args.device)
    image = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))
    vis_dir = str(tmp_path / "vis")
    maps = T.run_rise(args, model, image, vis_dir)
    want = rise_maps(model, image[None].cuda(), min_level=0.2, n_masks=64, batch=32)
    assert want.dtype == torch.uint8 and want.is_cuda and tuple(want.shape) == (1, 10, 64, 64)
    assert torch.equal(want, K.heat_maps(rise(model, image[None].cuda(), n_masks=64, batch=32), 0.2))
    some = rise_maps(model, image[None].cuda(), classes=[2, 5], n_masks=64, batch=32)
    assert torch.equal(some, K.heat_maps(rise(model, image[None].cuda(), classes=[2, 5], n_masks=64, batch=32), 0.0))
    want = want[0].cpu().numpy()
    assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and np.array_equal(maps, want)
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(vis_dir, "rise_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, want[c])
    assert not os.path.exists(os.path.join(vis_dir, "rise_10.png"))
    assert any(m.any() for m in want)
    # the command line: the flag writes the same set of files (random weights: no checkpoint under the empty output_dir)
    cli_dir = str(tmp_path / "cli")
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class",
        "1", "--to_k_layer", "1", "--power", "1", "--use_slot", "true" if use_slot else "false", "--pre_trained", "false",
        "--img_size", "64", "--rise", "true", "--rise_masks", "32", "--rise_batch", "16", "--grad_min_level", "0.2",
        "--eval_fold", "true", "--vis_dir", cli_dir, "--output_dir", str(tmp_path / "none")])
    T.main()
    for c in range(10):
        png = np.asarray(Image.open(os.path.join(cli_dir, "rise_%d.png" % c)))
        assert png.shape == (64, 64) and png.dtype == np.uint8
    assert not os.path.exists(os.path.join(cli_dir, "rise_10.png"))
    assert not os.path.exists(os.path.join(cli_dir, "cam_0.png")) and not os.path.exists(os.path.join(cli_dir, "grad_0.png"))
