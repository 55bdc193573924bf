"""The per-tap weight-gradient kernels at every tile, addressing mode and (tile, split-K) plan, against fp64 (-m gpu).

csrc/conv_igemm.hip wgrad_kernel<BM, BN, .., MODE> (9 tile pairs x 3 modes) and csrc/conv_wgrad_bf16.h wgrad_bf16_kernel<BM, BN, ..,
MODE, A_BF16, B_BF16> (4 tile pairs x 2 modes x 4 storages) take every layer the tap-fused, plane and register-split weight
gradients do not.  Which instance runs depends on the plan kernels.conv2d_wgrad takes from the tuning table, so the shape alone
reaches few of them; here the plan is FORCED (kernels._tile_cache[key] = plan, as tests/test_storage_gpu.py does) and CASES below
lists, per case, the smallest shape that still reaches a path: ragged last chunks and last splits, image boundaries inside a
chunk, maps one chunk wide, 32- / 96-channel groups on 64-wide bf16 tiles, and the split counts on either side of the loop bounds
of slab_reduce_kernel.  tests/test_wgrad_plans_cpu.py asks the library (scouter_conv2d_wgrad_plan, no device) what each case
reaches and asserts that the table covers all of it.

Per case: dw is prefilled with NaN, every element must be finite and within the project's bound of the fp64 weight gradient on
the CPU (torch.nn.grad.conv2d_weight on doubles; x^T dy for pointwise layers; bf16 cases: of the RNE-rounded operands),
    |err| <= _k_for(M) * sqrt(sum_m t_m^2) + 1e-12        (_k_for: tests/test_size_thresholds_gpu.py; t_m: the terms of the sum)
the library profiler must name the kernel the query announced (wgrad<BMxBN> / wgrad_bf16, and slab_reduce exactly when the plan
has more than one split), and a second launch must give the same bits.  The split-K workspace is a fresh one of the size the
library's workspace query names for the plan, filled with NaN bit patterns: a slab element no workgroup writes, or a slab index
the sum reads past the last split, shows.  Inputs are standard normal: one dropped or doubled pixel
moves an element by about 1 / sqrt(M) of its magnitude, orders above the bound."""
import collections
import functools
import zlib

import pytest
import torch

from test_size_thresholds_gpu import _k_for, _profiled                   # noqa: E402
from test_table_entries_gpu import _opnd                                  # noqa: E402

pytestmark = pytest.mark.gpu

# kind: "fp32" -- precision "fp32"; "bf16" -- precision "bf16" on the bf16 kernel, `storage` bit 0: x stored as bf16, bit 1: dy;
# "refused" -- precision "bf16" on a shape the bf16 kernel refuses: the fp32 kernel must run
Case = collections.namedtuple("Case", "kind B H W cin cout k stride pad groups plan storage")
ALL_PLANS = (-1,) + tuple(t | b for t in (0, 16, 32, 48) for b in (0, 1, 2, 3))
EDGES = (128, 64, 32)

# (B, H, W, k, stride, pad)
F32_EVERY_TILE = [
    (3, 7, 5, 1, 1, 0),         # MODE 2, M = 105: ragged last chunk
    (5, 9, 13, 1, 1, 0),        # MODE 2, M = 585: three splits, the last one with 3 chunks
    (3, 8, 5, 3, 1, 1),         # MODE 1, M = 120: the shortest map MODE 1 accepts at width 5
    (3, 7, 5, 3, 1, 1),         # MODE 0, M = 105: the same layer one row shorter
    (4, 11, 17, 3, 1, 1),       # MODE 1, M = 748: three splits, images ending inside chunks
    (3, 9, 11, 3, 2, 1),        # MODE 0: strided 3x3
    (3, 9, 11, 1, 2, 0),        # MODE 0: strided 1x1 downsample
]
F32_TWO_TILES = [
    (1, 3, 3, 1, 1, 0),         # M = 9: less than one chunk
    (2, 6, 32, 3, 1, 1),        # width equal to the chunk
    (2, 6, 33, 3, 1, 1),        # width one past the chunk
    (2, 34, 1, 3, 1, 1),        # width 1
    (2, 9, 9, 5, 1, 2),         # 5x5 taps
    (2, 9, 7, 3, 1, 0),         # shrinking 3x3
    (37, 2, 2, 3, 1, 1),        # 2 x 2 map
    (40, 1, 1, 3, 1, 1),        # 1 x 1 map
]
F32_BUDGET = (5, 20, 20, 96, 96, 3, 1, 1, 1)            # (B, H, W, cin, cout, k, stride, pad, groups): over ALL_PLANS
SLAB_M = (256, 257, 8192, 8193, 24576, 24577, 32768, 32769, 57601, 66000)       # pointwise 32 -> 32 on (M, 1, 1) maps, plan -1
BF16_GEOMS = [
    (5, 15, 14, 1, 1, 0),       # MODE 2, M = 1050: last split of 26 pixels
    (4, 17, 16, 3, 1, 1),       # MODE 1
    (2, 9, 64, 3, 1, 1),        # MODE 1, width 64
    (2, 8, 65, 3, 1, 1),        # MODE 1, width 65
    (2, 9, 63, 3, 1, 1),        # MODE 1, width 63
    (14, 6, 13, 3, 1, 1),       # MODE 1: the shortest map MODE 1 accepts at width 13
]
# (cin, cout, groups, plans): 128 -> 128 reaches the four tiles through the plan bits; both tile axes ragged; 32-channel groups
# (the tile reads the neighbouring pixel's / group's channels and drops them); 32 -> 32
BF16_CHANNELS = [(128, 128, 1, (0, 16, 32, 48)), (96, 160, 1, (-1,)), (64, 64, 2, (1,)), (96, 96, 3, (-1,)), (32, 32, 1, (2,))]
BF16_BUDGET = (8, 17, 18, 96, 160, 3, 1, 1, 1)
REFUSED = (17, 5, 13, 64, 128, 3, 1, 1, 1)              # 64 / 13 + 1 = 5 rows: the bf16 kernel's pixel walk needs more


def _axis(edge, by_plan_bit):
    """-> (channels per group, plan bit needed) that give tile edge `edge`: by the channel count alone, or halved by the plan"""
    if edge == 128:
        return 128, False
    if edge == 64:
        return (128, True) if by_plan_bit else (64, False)
    return (64, True) if by_plan_bit else (96, False)


def _cases():
    out = []
    for gi, (B, H, W, k, s, p) in enumerate(F32_EVERY_TILE):
        for bm in EDGES:
            for bn in EDGES:
                (cg, bit_m), (ng, bit_n) = _axis(bm, gi & 1), _axis(bn, gi & 1)
                plan = (16 * bit_m) | (32 * bit_n) | (gi % 4) if gi & 1 else -1
                out.append(Case("fp32", B, H, W, cg, ng, k, s, p, 1, plan, 0))
    for gi, (B, H, W, k, s, p) in enumerate(F32_TWO_TILES):
        out.append(Case("fp32", B, H, W, 96, 96, k, s, p, 1, -1, 0))
        out.append(Case("fp32", B, H, W, 128, 128, k, s, p, 1, gi % 4, 0))
    # groups (32 input channels per group on a same-size 3x3 layer: an explicit plan, the library's own is a tap-fused kernel)
    out.append(Case("fp32", 4, 11, 17, 64, 64, 3, 1, 1, 2, 0, 0))
    out.append(Case("fp32", 4, 11, 17, 128, 64, 3, 1, 1, 2, -1, 0))
    out.append(Case("fp32", 3, 9, 11, 96, 192, 3, 2, 1, 3, 1, 0))
    out.append(Case("fp32", 5, 9, 13, 192, 96, 1, 1, 0, 3, 18, 0))
    out += [Case("fp32", *F32_BUDGET, plan, 0) for plan in ALL_PLANS]
    out += [Case("fp32", m, 1, 1, 32, 32, 1, 1, 0, 1, -1, 0) for m in SLAB_M]
    for (B, H, W, k, s, p) in BF16_GEOMS:
        for cin, cout, groups, plans in BF16_CHANNELS:
            out += [Case("bf16", B, H, W, cin, cout, k, s, p, groups, plan, st) for plan in plans for st in range(4)]
    out += [Case("bf16", *BF16_BUDGET, plan, st) for plan in ALL_PLANS for st in range(4)]
    out.append(Case("refused", *REFUSED, -1, 0))
    return out


CASES = _cases()


def case_id(c):
    return "%s-%dx%dx%d-%dto%dg%d-k%ds%dp%d-plan%d%s" % (c.kind, c.B, c.H, c.W, c.cin, c.cout, c.groups, c.k, c.stride, c.pad,
                                                         c.plan, "-st%d" % c.storage if c.kind == "bf16" else "")


def shape_of(c):
    return (c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, c.groups)


def plan_of(kk, c):
    """what the library will launch for the case: {bm, bn, splits, pix_per_split, mode} of scouter_conv2d_wgrad_plan (no device)"""
    kernel = kk.WGRAD_BF16 if c.kind == "bf16" else kk.WGRAD_F32
    return {f: kk.ask("wgrad_plan", *shape_of(c), kernel, c.plan, i) for i, f in enumerate(kk.WGRAD_PLAN_FIELDS)}


def out_pixels(c):
    return c.B * ((c.H + 2 * c.pad - c.k) // c.stride + 1) * ((c.W + 2 * c.pad - c.k) // c.stride + 1)


FP32_CASES = [c for c in CASES if c.kind != "bf16"]
BF16_GROUPS = [[c._replace(storage=st) for st in range(4)] for c in CASES if c.kind == "bf16" and c.storage == 0]


def K():
    from scouter_amd import kernels
    return kernels


def _wgrad64(x, dy, c):
    """the weight gradient [k][k][cin / groups][cout] of fp64 NHWC operands on the CPU"""
    cg, ng = c.cin // c.groups, c.cout // c.groups
    if c.k == 1 and c.stride == 1 and c.pad == 0:
        xm, dm = x.reshape(-1, c.cin), dy.reshape(-1, c.cout)
        return torch.cat([xm[:, g * cg:(g + 1) * cg].t() @ dm[:, g * ng:(g + 1) * ng] for g in range(c.groups)], 1).view(1, 1, cg, c.cout)
    w = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (c.cout, cg, c.k, c.k), dy.permute(0, 3, 1, 2), c.stride, c.pad, 1, c.groups)
    return w.permute(2, 3, 1, 0).contiguous()


@functools.lru_cache(maxsize=2)
def _data(c, bf16):
    """-> x, dy (fp32, on the device), the fp64 weight gradient of what the kernel multiplies and sqrt(sum of its squared terms):
    computed once per shape and shared by the plans and storages listed for it (consecutive in CASES)"""
    gen = torch.Generator().manual_seed(zlib.crc32(repr((shape_of(c), bf16)).encode()))
    Ho, Wo = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    x = torch.randn(c.B, c.H, c.W, c.cin, generator=gen)
    dy = torch.randn(c.B, Ho, Wo, c.cout, generator=gen)
    xd, dd = _opnd(x, bf16), _opnd(dy, bf16)
    ref = _wgrad64(xd, dd, c)
    mag = _wgrad64(xd * xd, dd * dd, c).sqrt()
    return x.cuda(), dy.cuda(), ref, mag


def _launch_twice(kk, c, x, dy):
    """two launches of the case's plan -> dw of the first; asserts the profile rows and that the second gives the same bits"""
    bf16 = c.kind == "bf16"
    key = ("wgrad", bf16, *shape_of(c))
    pl = plan_of(kk, c)
    want = ["wgrad_bf16" if bf16 else "wgrad<%dx%d>" % (pl["bm"], pl["bn"])] + ["slab_reduce"] * (pl["splits"] > 1)
    # a workspace of the size the library asks for THIS plan, not one an earlier case grew
    kk._ws.pop((x.device.type, x.device.index, kk._stream()), None)
    ws = kk.workspace(kk.ask("wgrad_workspace_bytes", *shape_of(c), c.plan), x.device)
    saved = kk._tile_cache.get(key)
    kk._tile_cache[key] = c.plan
    try:
        with kk.switches(xwt=0, bwt=0):                  # (else the 32-channel-group 3x3 layers run the tap-fused kernels at plan -1)
            dws = []
            for _ in range(2):
                dw = torch.full((c.k, c.k, c.cin // c.groups, c.cout), float("nan"), device="cuda")
                ws.fill_(0xFF)                           # (NaN in every slab element no workgroup writes)
                _, names = _profiled(lambda: kk.conv2d_wgrad(x, dy, dw, c.stride, c.pad, c.groups,
                                                             precision="fp32" if c.kind == "fp32" else "bf16"))
                assert names == want, (case_id(c), names, want, pl)
                dws.append(dw)
    finally:
        if saved is None:
            del kk._tile_cache[key]
        else:
            kk._tile_cache[key] = saved
    assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32)), "%s: two launches differ" % case_id(c)
    return dws[0]


def _check(c, dw, ref, mag, what=""):
    got = dw.cpu().double()
    name = case_id(c) + what
    assert bool(torch.isfinite(got).all()), "%s: %d elements not written or not finite" % (name, int((~torch.isfinite(got)).sum()))
    tol = _k_for(out_pixels(c)) * mag + 1e-12
    ratio = (got - ref).abs() / tol
    worst = int(ratio.argmax())
    print("%s: worst |err| / bound = %.3g" % (name, float(ratio.view(-1)[worst])))
    bad = int((ratio > 1).sum())
    assert bad == 0, "%s: %d of %d elements off, worst %.3g x its bound at [r][s][ci][co] = %s (got %.9g, fp64 %.9g)" % (
        name, bad, got.numel(), float(ratio.view(-1)[worst]), tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), got.shape)),
        float(got.view(-1)[worst]), float(ref.view(-1)[worst]))


@pytest.mark.parametrize("c", FP32_CASES, ids=case_id)
def test_fp32_kernel_at_every_tile_mode_and_plan(c):
    """wgrad_kernel: all elements against fp64, the profile row of the announced tile, two launches the same bits.  The "refused"
    case asks for precision "bf16" on a map too short for the bf16 kernel's pixel walk: the fp32 kernel takes it, unrounded."""
    kk = K()
    if c.kind == "refused":
        assert out_pixels(c) >= kk.BF16_MIN_PIXELS and not kk.ask("wgrad_kernel_ok", *shape_of(c), kk.WGRAD_BF16)
    x, dy, ref, mag = _data(c._replace(kind="", plan=0, storage=0), False)
    _check(c, _launch_twice(kk, c, x, dy), ref, mag)


@pytest.mark.parametrize("group", BF16_GROUPS, ids=lambda g: case_id(g[0])[:-4])
def test_bf16_kernel_at_every_tile_mode_plan_and_storage(group):
    """wgrad_bf16_kernel with x / dy stored as fp32 or bf16: each of the four storages of the RNE-rounded operands against the
    fp64 gradient of those operands, all four the same bits; and the unrounded fp32 operands (the kernel's own rounding) within
    the same bound of it."""
    kk = K()
    c0 = group[0]
    assert out_pixels(c0) >= kk.BF16_MIN_PIXELS
    x, dy, ref, mag = _data(c0._replace(kind="", plan=0, storage=0), True)
    xh, dh = x.bfloat16(), dy.bfloat16()
    first = None
    for c in group:
        dw = _launch_twice(kk, c, xh if c.storage & 1 else xh.float(), dh if c.storage & 2 else dh.float())
        if first is None:
            first = dw
            _check(c, dw, ref, mag)
        else:
            assert torch.equal(dw.view(torch.int32), first.view(torch.int32)), "%s differs from storage 0" % case_id(c)
    _check(c0, _launch_twice(kk, c0, x, dy), ref, mag, " (unrounded fp32 operands)")
