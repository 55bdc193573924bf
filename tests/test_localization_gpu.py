"""Localisation scores and the batch's byte slot maps (-m gpu): kernels.map_localization against NumPy with == on all four
integers, tools/attribution.py localization's float64 ratios against NumPy's division of the same integers, kernels.group_maps
against the fp32 NumPy restatement of SlotAttention.vis_maps' expression with ==, and slot_maps(model) against vis_maps itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gradcam_gpu import build                                          # noqa: E402

# one pixel; a 7 x 7 grid of several maps; one and several strides of the 1024 threads; H W off and on a multiple of 4 (the
# byte and the 4-byte route)
SIZES = [(1, 1, 1, 1), (2, 3, 7, 7), (1, 1, 64, 64), (2, 1, 223, 225), (1, 2, 224, 224)]


def _mask(boxes, n_boxes, B, H, W):
    """bool [B, H, W]: the union of each image's first n_boxes boxes, clipped to the map"""
    mask = np.zeros((B, H, W), dtype=bool)
    if boxes is None:
        return mask
    for b in range(B):
        for x0, y0, x1, y1 in boxes[b, :n_boxes[b]]:
            x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), W), min(int(y1), H)
            if x1 > x0 and y1 > y0:
                mask[b, y0:y1, x0:x1] = True
    return mask


def _numpy_sums(maps, boxes, n_boxes):
    B, K, H, W = maps.shape
    mask = _mask(boxes, n_boxes, B, H, W)
    m = maps.astype(np.int64)
    arg = maps.reshape(B, K, H * W).argmax(axis=2)                           # (NumPy's argmax: the first among equals)
    hit = np.stack([mask[b].reshape(-1)[arg[b]] for b in range(B)]).astype(np.int64)
    return np.stack([m.sum(axis=(2, 3)), (m * mask[:, None]).sum(axis=(2, 3)), arg.astype(np.int64), hit], axis=2)


def _run(maps, boxes=None, n_boxes=None):
    from scouter_amd import kernels as K
    got = K.map_localization(torch.from_numpy(maps).cuda(), None if boxes is None else torch.from_numpy(boxes).cuda(),
                             None if n_boxes is None else torch.from_numpy(n_boxes).cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and tuple(got.shape) == maps.shape[:2] + (4,)
    return got.cpu().numpy()


def _boxes_cases(B, H, W, rng):
    """name -> (boxes int32 [B, nb, 4], n_boxes int32 [B])"""
    def same(rows, n=None):
        a = np.array(rows, dtype=np.int32)[None].repeat(B, axis=0)
        return np.ascontiguousarray(a), np.full(B, len(rows) if n is None else n, dtype=np.int32)
    cx, cy = W // 2, H // 2
    many = np.stack([rng.integers(-3, W + 3, (B, 32)), rng.integers(-3, H + 3, (B, 32)), rng.integers(-3, W + 3, (B, 32)),
                     rng.integers(-3, H + 3, (B, 32))], axis=2).astype(np.int32)
    return {
        "n_boxes 0": same([[0, 0, W, H]], 0),
        "whole map": same([[0, 0, W, H]]),
        "one pixel": same([[cx, cy, cx + 1, cy + 1]]),
        "over every edge": same([[-5, -7, W + 9, H + 2]]),
        "past the end": same([[W, H, W + 4, H + 4], [-9, -9, 0, 0]]),
        "inverted": same([[cx + 1, 0, cx, H], [0, cy + 1, W, cy]]),
        "two overlapping": same([[0, 0, cx + 1, cy + 1], [cx // 2, cy // 2, W, H]]),
        "second box not counted": same([[0, 0, 1, 1], [0, 0, W, H]], 1),
        "32 boxes": (many, rng.integers(0, 33, B).astype(np.int32)),
    }


# ------------------------------------------------------------------------------------------------------ 1: map_localization
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(str(v) for v in s))
def test_map_localization_equals_numpy(size):
    B, K, H, W = size
    rng = np.random.default_rng(sum(size))
    maps = rng.integers(0, 256, size, dtype=np.uint8)
    assert np.array_equal(_run(maps), _numpy_sums(maps, None, None))         # no boxes at all: null pointers
    for name, (boxes, n_boxes) in _boxes_cases(B, H, W, rng).items():
        want = _numpy_sums(maps, boxes, n_boxes)
        assert np.array_equal(_run(maps, boxes, n_boxes), want), name
        if name == "two overlapping" and H * W > 1:                          # the union, not the sum of the two boxes
            each = sum(_numpy_sums(maps, np.ascontiguousarray(boxes[:, j:j + 1]), np.ones(B, np.int32))[..., 1] for j in (0, 1))
            assert (want[..., 1] < each).all()
        if name == "whole map":
            assert np.array_equal(want[..., 0], want[..., 1]) and (want[..., 3] == 1).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(str(v) for v in s))
def test_map_localization_special_maps(size):
    B, K, H, W = size
    whole = (np.array([[[0, 0, W, H]]] * B, dtype=np.int32), np.ones(B, dtype=np.int32))
    zero = _run(np.zeros(size, dtype=np.uint8), *whole)
    assert (zero[..., :3] == 0).all() and (zero[..., 3] == 1).all()         # all equal: index 0, which the box holds
    full = _run(np.full(size, 255, dtype=np.uint8), *whole)
    assert (full[..., 0] == 255 * H * W).all() and (full[..., 2] == 0).all()
    if H * W >= 3:                                                           # the maximum twice: the smaller index wins
        rng = np.random.default_rng(5)
        maps = rng.integers(0, 200, size, dtype=np.uint8)
        first, second = (H * W) // 3, H * W - 1
        maps.reshape(B, K, -1)[:, :, [first, second]] = 230
        got = _run(maps)
        assert (got[..., 2] == first).all() and np.array_equal(got, _numpy_sums(maps, None, None))
        maps.reshape(B, K, -1)[:, :, first] = 229                            # and alone at the very end
        assert (_run(maps)[..., 2] == second).all()


def test_map_localization_an_odd_base_address_takes_the_byte_route():
    rng = np.random.default_rng(11)
    flat = torch.from_numpy(rng.integers(0, 256, 1 + 2 * 8 * 8, dtype=np.uint8)).cuda()
    from scouter_amd import kernels as K
    maps = flat[1:].view(1, 2, 8, 8)
    assert maps.data_ptr() % 4 == 1 and maps.is_contiguous()
    got = K.map_localization(maps).cpu().numpy()
    assert np.array_equal(got, _numpy_sums(maps.cpu().numpy(), None, None))


def test_map_localization_refusals():
    from scouter_amd import kernels as K
    maps = torch.zeros((2, 1, 4, 4), dtype=torch.uint8, device="cuda")
    n = torch.ones(2, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="map_localization.*33"):
        K.map_localization(maps, torch.zeros((2, 33, 4), dtype=torch.int32, device="cuda"), n)
    for bad in ((maps, torch.zeros((2, 1, 4), dtype=torch.int32, device="cuda"), None),
                (maps.float(), None, None), (maps[0], None, None),
                (maps, torch.zeros((2, 1, 4), dtype=torch.int64, device="cuda"), n),
                (maps, torch.zeros((3, 1, 4), dtype=torch.int32, device="cuda"), n)):
        with pytest.raises(RuntimeError):
            K.map_localization(*bad)
    ok = K.map_localization(maps, torch.zeros((2, 32, 4), dtype=torch.int32, device="cuda"), n)
    assert not ok.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------ 2: localization
def test_localization_ratios_are_numpys():
    from scouter_amd.tools.attribution import localization
    rng = np.random.default_rng(3)
    B, K, H, W = 3, 2, 9, 13
    maps = rng.integers(0, 256, (B, K, H, W), dtype=np.uint8)
    maps[1, 0] = 0                                                           # an empty map
    boxes = np.array([[[2, 1, 9, 6], [4, 3, 13, 9]], [[0, 0, 13, 9], [0, 0, 0, 0]], [[1, 1, 2, 2], [0, 0, 0, 0]]], dtype=np.int32)
    n_boxes = np.array([2, 1, 0], dtype=np.int32)
    r = localization(torch.from_numpy(maps).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(n_boxes).cuda())
    for t, dtype in ((r.area, torch.float64), (r.precision, torch.float64), (r.hit, torch.float64), (r.boxed, torch.bool),
                     (r.empty, torch.bool), (r.sums, torch.int64)):
        assert t.is_cuda and t.dtype == dtype
    want = _numpy_sums(maps, boxes, n_boxes)
    assert np.array_equal(r.sums.cpu().numpy(), want)
    S, S_in = want[..., 0], want[..., 1]
    assert np.array_equal(r.area.cpu().numpy(), S / (255 * H * W))
    precision = np.zeros((B, K))
    np.divide(S_in, S, out=precision, where=S != 0)
    assert np.array_equal(r.precision.cpu().numpy(), precision)
    assert r.precision[1, 0] == 0.0 and bool(r.empty[1, 0]) and int(r.empty.sum()) == 1
    assert np.array_equal(r.hit.cpu().numpy(), want[..., 3].astype(np.float64))
    assert r.boxed.cpu().tolist() == [True, True, False]
    assert (r.precision[2] == 0).all() and (r.hit[2] == 0).all()             # no box: nothing inside
    assert (r.precision[1, 1] == 1.0) and (r.hit[1] == 1).all()              # the whole map as the box
    none = localization(torch.from_numpy(maps).cuda())
    assert not bool(none.boxed.any()) and torch.equal(none.area, r.area) and not bool(none.precision.any())


# ------------------------------------------------------------------------------------------------------ 3: group_maps
def _group_maps_numpy(a):
    """SlotAttention.vis_maps' expression per group in fp32 NumPy: ((v - lo) / span * 255) truncated; a constant group is zeros"""
    out = np.zeros(a.shape, dtype=np.uint8)
    for m in range(a.shape[0]):
        lo, hi = a[m].min(), a[m].max()
        span = np.float32(hi - lo)
        if span > 0:
            out[m] = ((a[m] - lo) / span * np.float32(255.0)).astype(np.uint8)
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 49), (1, 200, 81), (70, 10, 49)], ids=lambda s: "x".join(str(v) for v in s))
def test_group_maps_equals_the_fp32_restatement(shape):
    from scouter_amd import kernels as K
    a = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)
    assert a.dtype == np.float32
    if shape[0] > 1:
        a[1] = 0.375                                                         # one constant group among varying ones
    got = K.group_maps(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    got, want = got.cpu().numpy(), _group_maps_numpy(a)
    print("group_maps", shape, "bytes off", int((got != want).sum()))
    assert np.array_equal(got, want)
    if shape[0] > 1:
        assert not got[1].any() and got[0].max() == 255 and got[0].min() == 0
    if shape == (1, 1, 1):
        assert not got.any()
    side = K.group_maps(torch.from_numpy(a).cuda().view(shape[0], shape[1], 1, shape[2]))       # trailing dimensions are kept
    assert tuple(side.shape) == (shape[0], shape[1], 1, shape[2]) and np.array_equal(side.cpu().numpy().reshape(shape), want)


def test_slot_maps_are_vis_maps_of_every_image():
    """resnet18_mnist_64: slots_per_class is 1, so no slot sum is involved"""
    from scouter_amd.tools.attribution import localization, slot_maps
    m, P, images, cfg, arch = build("resnet18_mnist_64")
    m.eval()
    with torch.no_grad():
        m(images.cuda())
    maps = slot_maps(m)
    torch.cuda.synchronize()
    B = images.shape[0]
    assert maps.dtype == torch.uint8 and maps.is_cuda and maps.dim() == 4 and tuple(maps.shape[:2]) == (B, 10)
    try:
        for i in range(B):
            m.slot.vis_id = i
            want = m.slot.vis_maps()
            assert want.any() and np.array_equal(maps[i].cpu().numpy(), want), i
            # the reference's attention_ratio (test.py:40-44) of every class's map is localization's area
            ratio = want.astype(np.float64).sum(axis=(1, 2)) / float(want[0].size * 255)
            assert np.array_equal(localization(maps).area[i].cpu().numpy(), ratio)
    finally:
        m.slot.vis_id = 0
