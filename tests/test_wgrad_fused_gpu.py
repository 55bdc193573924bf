"""The tap-fused, register-split and plane weight-gradient kernels at every instance and plan edge, against fp64 (-m gpu).

These are the weight gradients of the default step and of config 5 that tests/test_wgrad_plans_gpu.py (the per-tap kernels)
does not launch:
    wgrad_taps_kernel<32|64>      csrc/conv_wgrad_taps.h           kernels.conv2d_wgrad, plan -1, switch xwt=0
    xwgrad_taps_kernel<32|64>     csrc/conv_wgrad_taps_x3.h        kernels.conv2d_wgrad, plan -1, switch xwt=1
    bwgrad_taps_kernel<32|64>     csrc/conv_wgrad_taps_bf16.h      kernels.conv2d_wgrad, precision "bf16", plan -1, switch bwt=1
    xwgrad_kernel                 csrc/conv_x3.hip                 kernels.conv2d_wgrad_x3(plan=p)
    pwgrad_kernel<BM, BN, NP, 3>  csrc/conv_planes.hip             kernels.conv2d_wgrad_planes, plans -1 .. 51
    pwgrad_taps_kernel<NP, 1>     csrc/conv_planes_wgrad_taps.h    kernels.conv2d_wgrad_planes, plans 64 .. 67
The route is FORCED (kernels._tile_cache[key] = plan, the switches, BF16_MIN_PIXELS = 1) and the tables below name, per case, the
smallest shape that still reaches a path: the shortest map each kernel's rule admits at widths around the 32- / 64-pixel chunk,
every column tile and group count, pixel counts on either side of the first split, last splits with odd and even chunk counts,
chunks that end inside a row and span images, splits past the floor of 256 pixels (only there does `pix_per_split` differ from
256, and the register-split kernel's odd-to-even rounding act), more than 128 splits.  tests/test_wgrad_fused_cpu.py asks the
library (scouter_conv2d_wgrad_plan / _x3_plan / _planes_plan: integers only, no device) what each case reaches and asserts that
the tables cover all of it.

Per case, exactly as tests/test_wgrad_plans_gpu.py does for the per-tap kernels (its _data / _check, so the same bound):
dw is prefilled with NaN; the split-K workspace is a fresh one of exactly the bytes the library's workspace query names for the
case, filled with 0xFF (NaN in every slab element no workgroup writes); every element must be finite and
    |dw - ref64| <= _k_for(M) * sqrt(sum_m t_m^2) + 1e-12
with ref64 the fp64 weight gradient on the CPU of what the kernel multiplies (bf16 kernels and the one-plane plane kernel: of
the RNE-rounded operands; the three-plane split is exact: of the fp32 operands); the profile rows must be the announced kernel
plus slab_reduce exactly when the queried plan has more than one split (a silent fall-back to the per-tap kernel fails on the
name); a second launch on a re-poisoned workspace must give the same bits.  Inputs are standard normal: one dropped or doubled
pixel moves an element by about 1 / sqrt(M) of its magnitude, orders above the bound."""
import collections

import pytest
import torch

from test_wgrad_plans_gpu import Case, _check, _data, K                   # noqa: E402
from test_size_thresholds_gpu import _profiled                           # noqa: E402

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------------------
# tap-fused kernels: 3x3 / stride 1 / pad 1, 32 input channels per group.  ng: output channels per group
# kind: "taps" -- wgrad_taps_kernel; "xwt" -- xwgrad_taps_kernel; "bwt" -- bwgrad_taps_kernel;
# "wide-xwt" / "wide-bwt" -- a map 113 wide under switch xwt / bwt: wgrad_taps_kernel / the per-tap wgrad_bf16_kernel must run
Taps = collections.namedtuple("Taps", "kind B H W ng groups")
TAPS_KINDS = ("taps", "xwt", "bwt")
RULE_CHUNK = {"taps": 32, "xwt": 32, "bwt": 64}          # the chunk of the kernel's map rule: chunk / W + 1 < H
WIDTHS = (3, 31, 32, 33, 63, 64, 65, 111, 112)
# (ng, groups): 32 / 64 -- one column tile; 96 -- three 32-column tiles; 128 -- two 64-column tiles
COMBOS = [(32, 1), (64, 2), (96, 3), (128, 1), (32, 3), (64, 1), (96, 2), (128, 2), (32, 2), (64, 3), (96, 1), (128, 3)]
# (B, H, W) by pixel count, for the kernels of the 32-pixel rule / of the 64-pixel rule
PIXELS = {
    "M256": ((4, 4, 16), (2, 8, 16)),                    # one split, filled to its last pixel
    "M257": ((1, 257, 1), (1, 257, 1)),                  # a second split of one pixel; B = 1; width 1
    "M343/385": ((7, 7, 7), (5, 11, 7)),                 # last split of 87 / 129 pixels: 3 chunks of 32, 2 of 64 / 3 of 64, the last
                                                         # chunk ends inside a row; the split boundary lies inside a row
    "M306/356": ((3, 6, 17), (2, 89, 2)),                # last split of 50 / 100 pixels: 2 chunks of 32, 1 of 64 / 2 of 64
    "M320": ((4, 5, 16), None),                          # the split boundary lies inside an image at the start of a row (64-pixel
                                                         # rule: the maps 64 and 32 wide above)
}
PAST_FLOOR = {"taps": (4, 98, 112), "xwt": (1, 100, 111), "bwt": (2, 100, 112)}     # three groups of 32 -> 128: six tiles
MANY_SPLITS = (5, 59, 112)                                # 32 -> 32, M = 33 040: 130 splits of 256 pixels


def _taps_cases():
    out = []
    for kind in TAPS_KINDS:
        ch = RULE_CHUNK[kind]
        for i, W in enumerate(WIDTHS):                    # the shortest map the rule admits at each width
            out.append(Taps(kind, 7 if W == 3 else 3, ch // W + 2, W, *COMBOS[i]))
        for ng, groups in COMBOS[len(WIDTHS):-1]:         # the column tiles x group counts that neither the widths nor the
            out.append(Taps(kind, 2, ch // 9 + 2, 9, ng, groups))       # case past the floor (128 x 3, below) take
        if kind == "xwt":
            out.append(Taps(kind, 1, 8, 5, 32, 1))        # M = 40: less than the kernel's 64-pixel chunk (the 32-pixel rule admits it)
        for name, (g32, g64) in PIXELS.items():
            if (g64 if ch == 64 else g32) is not None:
                out.append(Taps(kind, *(g64 if ch == 64 else g32), 32, 1))
        out.append(Taps(kind, *PAST_FLOOR[kind], 128, 3))
        if kind != "bwt":
            out.append(Taps(kind, *MANY_SPLITS, 32, 1))
    out.append(Taps("wide-xwt", 2, 2, 113, 64, 1))
    out.append(Taps("wide-bwt", 2, 2, 113, 64, 1))
    return out


TAPS_CASES = _taps_cases()


def taps_id(c):
    return "%s-%dx%dx%d-32to%dg%d" % (c.kind, c.B, c.H, c.W, c.ng, c.groups)


def taps_shape(c):
    return (c.B, c.H, c.W, 32 * c.groups, c.ng * c.groups, 3, 3, 1, 1, c.groups)


def taps_code(kk, kind):
    return {"taps": kk.WGRAD_TAPS, "xwt": kk.WGRAD_XWT, "bwt": kk.WGRAD_BWT, "wide-xwt": kk.WGRAD_TAPS, "wide-bwt": kk.WGRAD_BF16}[kind]


TAPS_PLAN_FIELDS = ("bm", "bn", "splits", "pix_per_split", "chunk")      # ("chunk": the addressing mode for "wide-bwt")


def taps_plan(kk, c):
    """what the library launches for the case: scouter_conv2d_wgrad_plan of its kernel (no device)"""
    return {f: kk.ask("wgrad_plan", *taps_shape(c), taps_code(kk, c.kind), -1, i) for i, f in enumerate(TAPS_PLAN_FIELDS)}


TAPS_NAME = {"taps": "wgrad_taps", "xwt": "xwgrad_taps<bf16x3>", "bwt": "bwgrad_taps<bf16>", "wide-xwt": "wgrad_taps", "wide-bwt": "wgrad_bf16"}

# ------------------------------------------------------------------------------------------------------------------------------
# register-split pointwise kernel: 128-multiples of channels; every shape runs all of kernels._X3_WGRAD_PLANS
X3 = collections.namedtuple("X3", "B H W cin cout")
X3_PLANS = (-1, 0, 1, 2, 3)
X3_CASES = [
    X3(1, 3, 3, 128, 128),          # M = 9: less than one chunk, no multiple of 4
    X3(1, 16, 16, 128, 128),        # M = 256: one full split
    X3(1, 257, 1, 128, 128),        # M = 257: a second split of one pixel
    X3(2, 20, 15, 128, 128),        # M = 600: three splits, the last of 88 pixels -- 3 chunks, the third ragged
    X3(5, 9, 7, 256, 128),          # M = 315 = 4 * 78 + 3: the ci tile of the block index
    X3(5, 9, 7, 128, 384),          # the co tile
    X3(8, 12, 12, 1024, 1024),      # M = 1152, 64 tiles: plans -1 / 0 give 9 chunks per split (288 pixels), plans 1-3 the floor
    X3(3, 10, 10, 2048, 2176),      # 272 tiles, more than the budget of plans -1 / 0: one split of 10 chunks each
]
X3_PLAN_FIELDS = ("ci_tiles", "co_tiles", "splits", "pix_per_split")


def x3_id(c):
    return "x3-%dx%dx%d-%dto%d" % c


def x3_plan(kk, c, plan):
    return {f: kk.ask("wgrad_x3_plan", *c, plan, i) for i, f in enumerate(X3_PLAN_FIELDS)}


# ------------------------------------------------------------------------------------------------------------------------------
# plane kernels: same-size k x k layers (pad = k // 2), 64-multiples of channels per group; every case runs with 1 and 3 planes
Planes = collections.namedtuple("Planes", "B H W cin cout k groups plan")
PLANES_CASES = [
    # pwgrad_kernel<BM, BN>: widths 1, 5, 31, 32, 33, 63 at H = 32 // W + 2
    Planes(2, 34, 1, 128, 128, 3, 1, -1),       # 128 x 128; width 1
    Planes(3, 8, 5, 128, 128, 3, 1, 32),        # 128 x 64 by plan bit 32
    Planes(3, 3, 31, 128, 128, 1, 1, 16),       # 64 x 128 by plan bit 16; 1x1; M = 279: a ragged second split
    Planes(2, 3, 32, 64, 128, 5, 1, -1),        # 64 x 128 by the channels; 5x5; width of the chunk
    Planes(2, 2, 33, 128, 64, 3, 1, 0),         # 128 x 64 by the channels; width one past the chunk
    Planes(3, 2, 63, 192, 192, 3, 1, -1),       # 192 channels: three 64-wide tiles each way; two splits
    Planes(2, 8, 5, 128, 256, 3, 2, -1),        # two groups of 64 -> 128
    Planes(5, 8, 5, 384, 128, 1, 2, 48),        # two groups of 192 -> 64; 1x1 (plan bits on 64-wide tiles change nothing)
    Planes(4, 9, 9, 128, 128, 5, 2, -1),        # 5x5 in two groups; M = 324: last split of 68 pixels = 3 chunks
    Planes(4, 4, 16, 64, 64, 3, 1, 1),          # M = 256: one full split
    Planes(1, 257, 1, 64, 64, 3, 1, 2),         # M = 257: a second split of one pixel; B = 1
    Planes(2, 2, 64, 128, 128, 3, 1, 48),       # 64 x 64 by both plan bits; width 64 (no tap-fused plan there)
    # pwgrad_taps_kernel (plans 64 - 67, 3x3): 64 x 64 tiles carrying all nine taps
    Planes(2, 2, 63, 64, 64, 3, 1, 64),         # the widest map, as short as it may be
    Planes(2, 3, 62, 128, 64, 3, 1, 65),        # width 62; two ci tiles
    Planes(9, 12, 3, 64, 128, 3, 1, 66),        # 36-pixel images: a chunk spans two; two co tiles; two splits
    Planes(20, 12, 3, 128, 128, 3, 2, 67),      # two groups; M = 720: three splits -- ring units before pixel 0 and after a split
    Planes(3, 8, 5, 192, 192, 3, 1, 64),        # three tiles each way
]
PLANES_REFUSED = [
    Planes(2, 2, 64, 64, 64, 3, 1, 64),         # width 64: plans >= 64 are refused
    Planes(2, 2, 64, 64, 64, 3, 1, 67),
]
PLANES_PLAN_FIELDS = ("bm", "bn", "splits", "pix_per_split", "fused")


def planes_id(c):
    return "planes-%dx%dx%d-%dto%dg%d-k%d-plan%d" % (c.B, c.H, c.W, c.cin, c.cout, c.groups, c.k, c.plan)


def planes_args(c, nplanes):
    return (c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.k // 2, c.groups, nplanes)


def planes_plan(kk, c, nplanes):
    return {f: kk.ask("wgrad_planes_plan", *planes_args(c, nplanes), c.plan, i) for i, f in enumerate(PLANES_PLAN_FIELDS)}


# ------------------------------------------------------------------------------------------------------------------------------
WGRAD_ROWS = ("wgrad", "xwgrad", "bwgrad", "pwgrad", "slab_reduce")


def _canon(B, H, W, cin, cout, k, groups):
    """the case as tests/test_wgrad_plans_gpu.py names a layer (its _data and _check take it)"""
    return Case("", B, H, W, cin, cout, k, 1, k // 2, groups, 0, 0)


def _twice(kk, name, launch, ws_bytes, kernel, splits, shape, dtype=torch.float32):
    """two launches -> dw of the first.  Each on a workspace of exactly `ws_bytes` filled with 0xFF and a NaN-filled dw; asserts
    the profile rows (`kernel`, then slab_reduce exactly when splits > 1; nothing else that computes a weight gradient) and that
    the second launch gives the same bits"""
    want = [kernel] + ["slab_reduce"] * (splits > 1)
    key = ("cuda", torch.cuda.current_device(), kk._stream())
    kk._ws.pop(key, None)                                # (a workspace of THIS case's size, not one an earlier case grew)
    ws = kk._ws[key] = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device="cuda")
    dws = []
    try:
        for _ in range(2):
            dw = torch.full(shape, float("nan"), device="cuda", dtype=dtype)
            ws.fill_(0xFF)
            _, names = _profiled(lambda: launch(dw))
            assert kk._ws.get(key) is ws, "%s: the wrapper asked for more workspace than the query's %d bytes" % (name, ws_bytes)
            rows = [n for n in names if n.startswith(WGRAD_ROWS)]
            assert rows == want, (name, names, want)
            dws.append(dw)
    finally:
        kk._ws.pop(key, None)
    assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32)), "%s: two launches differ" % name
    return dws[0]


class _forced:
    """kernels._tile_cache[key] = plan for the duration of a with-block"""

    def __init__(self, kk, key, plan):
        self.kk, self.key, self.plan = kk, key, plan

    def __enter__(self):
        self.saved = self.kk._tile_cache.get(self.key)
        self.kk._tile_cache[self.key] = self.plan

    def __exit__(self, *exc):
        if self.saved is None:
            self.kk._tile_cache.pop(self.key, None)
        else:
            self.kk._tile_cache[self.key] = self.saved
        return False


@pytest.mark.parametrize("c", [c for c in TAPS_CASES if c.kind in ("taps", "xwt", "wide-xwt")], ids=taps_id)
def test_fp32_tap_fused_kernels(c):
    """wgrad_taps_kernel (xwt=0) and xwgrad_taps_kernel (xwt=1): all elements against fp64 of the fp32 operands.  The map 113
    wide is past the register-split kernel's rows: under xwt=1 wgrad_taps_kernel must run."""
    kk = K()
    shape = taps_shape(c)
    if c.kind == "wide-xwt":
        assert kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_XWT) == 0 and kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_TAPS) == 1
    pl = taps_plan(kk, c)
    assert pl["splits"] >= 1, (taps_id(c), pl)
    cc = _canon(c.B, c.H, c.W, shape[3], shape[4], 3, c.groups)
    x, dy, ref, mag = _data(cc, False)
    with _forced(kk, ("wgrad", False, *shape), -1), kk.switches(xwt=0 if c.kind == "taps" else 1, bwt=0):
        dw = _twice(kk, taps_id(c), lambda dw: kk.conv2d_wgrad(x, dy, dw, 1, 1, c.groups), kk.ask("wgrad_workspace_bytes", *shape, -1),
                    TAPS_NAME[c.kind], pl["splits"], (3, 3, 32, shape[4]))
    _check(cc, dw, ref, mag, " [%s]" % taps_id(c))


@pytest.mark.parametrize("c", [c for c in TAPS_CASES if c.kind in ("bwt", "wide-bwt")], ids=taps_id)
def test_bf16_tap_fused_kernel_in_every_storage(c, monkeypatch):
    """bwgrad_taps_kernel (precision "bf16", bwt=1) with x / dy stored as fp32 or bf16: the RNE-rounded operands in each of the
    four storages against the fp64 gradient of those operands, all four the same bits.  The map 113 wide is past its rows: the
    per-tap wgrad_bf16_kernel must run."""
    kk = K()
    monkeypatch.setattr(kk, "BF16_MIN_PIXELS", 1)        # (the model keeps layers under 1024 pixels on the fp32 kernels)
    shape = taps_shape(c)
    if c.kind == "wide-bwt":
        assert kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_BWT) == 0 and kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_BF16) == 1
    pl = taps_plan(kk, c)
    assert pl["splits"] >= 1, (taps_id(c), pl)
    cc = _canon(c.B, c.H, c.W, shape[3], shape[4], 3, c.groups)
    x, dy, ref, mag = _data(cc, True)
    xh, dh = x.bfloat16(), dy.bfloat16()
    first = None
    with _forced(kk, ("wgrad", True, *shape), -1), kk.switches(xwt=0, bwt=1):
        for storage in range(4):
            xs, ds = xh if storage & 1 else xh.float(), dh if storage & 2 else dh.float()
            name = "%s-st%d" % (taps_id(c), storage)
            dw = _twice(kk, name, lambda dw: kk.conv2d_wgrad(xs, ds, dw, 1, 1, c.groups, precision="bf16"),
                        kk.ask("wgrad_workspace_bytes", *shape, -1), TAPS_NAME[c.kind], pl["splits"], (3, 3, 32, shape[4]))
            if first is None:
                first = dw
                _check(cc, dw, ref, mag, " [%s]" % name)
            else:
                assert torch.equal(dw.view(torch.int32), first.view(torch.int32)), "%s differs from storage 0" % name


@pytest.mark.parametrize("c", X3_CASES, ids=x3_id)
def test_register_split_pointwise_kernel_at_every_plan(c):
    """xwgrad_kernel: every plan of kernels._X3_WGRAD_PLANS, all elements against fp64 of the fp32 operands"""
    kk = K()
    assert kk._X3_WGRAD_PLANS == X3_PLANS
    cc = _canon(c.B, c.H, c.W, c.cin, c.cout, 1, 1)
    x, dy, ref, mag = _data(cc, False)
    for plan in X3_PLANS:
        pl = x3_plan(kk, c, plan)
        assert pl["splits"] >= 1, (x3_id(c), plan, pl)
        name = "%s-plan%d" % (x3_id(c), plan)
        dw = _twice(kk, name, lambda dw: kk.conv2d_wgrad_x3(x, dy, dw, plan=plan), kk.ask("wgrad_x3_workspace_bytes", *c, plan),
                    "xwgrad<bf16x3>", pl["splits"], (1, 1, c.cin, c.cout))
        _check(cc, dw, ref, mag, " [%s]" % name)


@pytest.mark.parametrize("nplanes", (1, 3))
@pytest.mark.parametrize("c", PLANES_CASES, ids=planes_id)
def test_plane_kernels_with_one_and_three_planes(c, nplanes):
    """pwgrad_kernel / pwgrad_taps_kernel: three planes (the split is exact) against fp64 of the fp32 operands, one plane against
    fp64 of the RNE-rounded operands"""
    kk = K()
    pl = planes_plan(kk, c, nplanes)
    assert pl["splits"] >= 1, (planes_id(c), pl)
    cc = _canon(c.B, c.H, c.W, c.cin, c.cout, c.k, c.groups)
    x, dy, ref, mag = _data(cc, nplanes == 1)
    xp, dyp = kk.planes_split(x, nplanes), kk.planes_split(dy, nplanes)
    if nplanes == 1:
        assert torch.equal(xp[0], x.bfloat16()) and torch.equal(dyp[0], dy.bfloat16())      # (one plane is the RNE rounding)
    name = "%s-np%d" % (planes_id(c), nplanes)
    ws_bytes = kk.ask("wgrad_planes_workspace_bytes", c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.groups, c.plan)
    with _forced(kk, ("pwgrad", nplanes, c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.k // 2, c.groups), c.plan):
        dw = _twice(kk, name, lambda dw: kk.conv2d_wgrad_planes(xp, dyp, dw, c.k // 2, c.groups), ws_bytes,
                    "pwgrad<bf16x3>" if nplanes == 3 else "pwgrad<bf16>", pl["splits"], (c.k, c.k, c.cin // c.groups, c.cout))
    _check(cc, dw, ref, mag, " [%s]" % name)


@pytest.mark.parametrize("nplanes", (1, 3))
@pytest.mark.parametrize("c", PLANES_REFUSED, ids=planes_id)
def test_tap_fused_plane_plans_are_refused_on_a_map_64_wide(c, nplanes):
    kk = K()
    assert kk.ask("wgrad_planes_plan_ok", *planes_args(c, nplanes), c.plan) == 0
    assert kk.ask("wgrad_planes_plan_ok", *planes_args(c, nplanes), c.plan & 63) == 1
    x = torch.zeros(c.B, c.H, c.W, c.cin, device="cuda")
    dy = torch.zeros(c.B, c.H, c.W, c.cout, device="cuda")
    dw = torch.zeros(c.k, c.k, c.cin // c.groups, c.cout, device="cuda")
    with _forced(kk, ("pwgrad", nplanes, c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.k // 2, c.groups), c.plan):
        with pytest.raises(RuntimeError):
            kk.conv2d_wgrad_planes(kk.planes_split(x, nplanes), kk.planes_split(dy, nplanes), dw, c.k // 2, c.groups)
