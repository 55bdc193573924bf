"""The plane, register-split and resident-rows convolution kernels at every named tile, against fp64, on ragged shapes (-m gpu).

csrc/conv_planes.hip (pconv_kernel, phalo_kernel = plane tile 5, ppersist_kernel = plane tile 6; one or three bf16 planes),
csrc/conv_x3.hip (xgemm_kernel, tiles 0-6, pointwise and CONV instantiations) and csrc/conv_xhalo.hip (xhalo_kernel<12 | 16>, tile 7
of the register-split entry points) run the convolutions tests/test_conv_tiles_gpu.py leaves out.  Here the C ABI is called
directly (scouter_conv2d_fwd_planes_io, scouter_conv2d_dgrad_planes_bnbwd, scouter_conv2d_fwd_x3, scouter_conv2d_dgrad_x3_bnbwd)
with the tile as the tile argument, on the smallest shapes that reach each path; the operands come from the library's own split
(kernels.planes_split / planes_split_weight, whose exactness tests/test_planes_gpu.py checks).  tests/test_split_tiles_cpu.py asks
the queries without a device and counts that the table reaches all 62 kernel instances.

GEOMETRIES (B, H, W, kh, kw, stride, pad) -- B, H, W the layer's INPUT map:
  same-size, both families, both passes: (3, 7, 5, 3, 3, 1, 1) M = 105; (5, 9, 13, 3, 3, 1, 1) M = 585 = 2 * 256 + 73 = 4 * 128 + 73 =
    9 * 64 + 9; (5, 34, 1, 3, 3, 1, 1) width 1; (40, 1, 1, 3, 3, 1, 1) 1 x 1 maps; (2, 9, 9, 5, 5, 1, 2) 25 taps
  pointwise, both families: (3, 7, 5), (5, 9, 13), (1, 1, 1) M = 1, (1, 3, 43) M = 129, (1, 1, 257) one row in the second 256-row tile
  plane forward only: (2, 9, 7, 3, 3, 1, 0) shrinking, (2, 9, 9, 3, 3, 1, 2) growing, (2, 8, 9, 1, 3, 1, 1) / (2, 8, 9, 3, 1, 1, 1)
    rectangular, (3, 9, 11, 3, 3, 2, 1) / (3, 10, 12, 3, 3, 2, 1) / (3, 9, 11, 1, 1, 2, 0) stride 2; the plane input gradient takes
    the shrinking and the growing one and refuses the strided ones (rc -3, query 0)
  plane tile 5 (3x3 same, W <= 63): (1, 5, 63), (3, 1, 9) height 1, the width-1 and 1 x 1 geometries; width 64: the query answers 0
  tile 7 (3x3 same, 32 columns per group): widths 1, 7, 63, 64 (sc_launch_xhalo's AG 12 / 16 switch), 126 at heights 5 and 1; width
    127 is refused by query and call
  persistent kernels (plane tile 6, tile 7): a batch of 15 x 17 maps with CU count + 2 M tiles of 256 rows, the last one ragged
    ((259, 15, 17) on 256 CUs: 258 tiles, 253 rows in the last): a second round of the tile walk.  GEMM-K 32 -> 64 columns on
    the plane kernels, 64 -> 32 columns on tile 7 (which has 32 columns per group).
CHANNELS: GEMM-K per group cycles 32, 96, 128 (64 where a pointwise layer needs two K tiles); columns per group 256, 128, 64 on
both families, 96 and 32 on the register-split one; groups 2 and 3 with 32 and 64 channels per group on tiles with one and with
two column tiles per group; tile 7: K per group 16, 32, 48, 64 in 1, 2 and 3 groups.
TILES: on the two ragged geometries every plane tile 0-6 at three planes, 0 / 1 / 5 / 6 at one plane (2 / 3 / 4 are hints that
fall back: their query answers 0, asserted), every register-split tile 0-6 pointwise and CONV; every other geometry on one 256-row
tile and one tile of another height.
EPILOGUES: forward on the two ragged geometries on every tile: none, bias, addend, ReLU, bias + addend + ReLU, statistics,
statistics + bias, less what a rule refuses (tile 7: bias, addend; plane tile 6: statistics with bias / addend, bf16 output --
each refusal asserted through query and call); plane forward with a bf16-stored output on tiles 0-5; input gradient:
plain, addend, one fused BatchNorm backward with the ReLU mask, one without, two with mask and addend, on every tile.

Per case the output lies inside a larger buffer prefilled with a NaN bit pattern, 128 guard rows in front and behind:
  1. the *_tile_ok query answers 1 for the named tile, epilogue and storage (the launch is no re-route);
  2. the library profiler names the family's kernel, once;
  3. every output element is finite, the guard rows keep their bits;
  4. every element is within  |err| <= _k_for(Cg * kh * kw) * V + 1e-12,  V = sqrt(sum of squared terms), of the fp64 convolution
     of the CPU (three planes and register split: of the fp32 operands; one plane: of the RNE-rounded ones; a bf16-stored output
     adds 2^-8 |ref|);
  5. a second launch gives the same bits;
  6. register-split tiles 0-6 give equal bits, plane tiles 0 / 1 / 2 / 3 / 4 / 6 give equal bits, and where the plane family takes
     the shape the register-split result equals the three-plane result on the pre-split operand; tiles 5 and 7 sum K in
     another order and get only the fp64 bound;
  7. statistics: the rows the family's row query names plus an untouched sentinel row, column sums equal to fp64 sums of the
     kernel's own output (rtol 1e-10, atol 1e-8), y bit-equal to the launch without statistics;
  8. fused BatchNorm backward: exactly 0 where the mask bit is clear, within the bound of ref (+ addend) elsewhere; partial rows
     as the row query says plus a sentinel row; summed they equal fp64 sums over the stored gradient (sum g: rtol 1e-9, atol
     1e-6; sum g * xhat: rtol 1e-6, atol 1e-4 -- the bounds of tests/test_xhalo_gpu.py).

FOUND by this file: tile 7 advertises 16-multiples of K per group (sc_xhalo_ok), but both entry points and queries refused 16 and
48 through the channel rule of tiles 0-6 (32-multiples) before tile 7 was looked at; the rule now applies to tiles 0-6 only and
tile 7 runs under its own.  And the three-plane forward took io = Y (query 1, rc 0) although only the one-plane instantiations
had the typed epilogue: it wrote fp32 rows over a bf16 buffer of half the size (the guard rows behind the output caught it).
The bf16-storing three-plane forward is now an instantiation of its own with the typed epilogue (pconv_kernel / phalo_kernel
<.., Y16>); the fp32-storing instantiations compile to the same code as before.  No model routes either shape.

MEASURED on an MI355X (992 cases in 344 groups, 367 tests, 6.0 s), worst |err| / bound per family and pass, fp32-stored outputs:
three planes forward 0.111, input gradient 0.150; one plane 0.106 / 0.106; register split tiles 0-6 0.098 / 0.102; tile 7 0.082 /
0.106.  A bf16-stored plane output: 0.993 (three planes), 0.992 (one): the rounding of the store is the 2^-8 |ref| term itself."""
import collections
import functools
import itertools
import zlib

import pytest
import torch

from test_conv_tiles_gpu import ADDEND, BIAS, GUARD, RELU, STATS, Y, _conv64, _guarded, _refusal, out_map      # noqa: E402
from test_size_thresholds_gpu import _check, _free, _k_for, _profiled                                             # noqa: E402
from test_table_entries_gpu import _opnd                                                                         # noqa: E402

pytestmark = pytest.mark.gpu

BN_BWD, BN_BWD2 = 16, 32                            # SCOUTER_EPI_BN_BWD / _BWD2
FUSE_BITS = {"": 0, "bn": BN_BWD, "bn-nomask": BN_BWD, "bn2": BN_BWD | BN_BWD2}
PLANE_BM = (128, 128, 128, 64, 256, 256, 256)       # rows of plane tile 0-6
X3_BM = (256, 128, 128, 64, 256, 256, 128, 256)     # rows of register-split tile 0-6 and of tile 7
X3_BN = (128, 128, 64, 64, 64, 32, 32, 32)
SAME_BITS = {"planes": (0, 1, 2, 3, 4, 6), "x3": (0, 1, 2, 3, 4, 5, 6)}     # tiles that promise equal bits

# family: "planes" | "x3" (tile 7: csrc/conv_xhalo.hip); nplanes: 1 | 3 (planes; 3 for x3); B, H, W: the layer's input map; cin,
# cout: the layer's channels (all groups); epi: SCOUTER_EPI_* bits of bias / addend / ReLU / statistics; io: Y = the plane
# forward stores bf16; fuse: the fused BatchNorm-backward mode of an input gradient ("", "bn", "bn-nomask", "bn2")
Case = collections.namedtuple("Case", "family dgrad nplanes B H W cin cout kh kw stride pad groups tile epi io fuse")

SAME = [(3, 7, 5, 3, 3, 1, 1), (5, 9, 13, 3, 3, 1, 1), (5, 34, 1, 3, 3, 1, 1), (40, 1, 1, 3, 3, 1, 1), (2, 9, 9, 5, 5, 1, 2)]
POINTWISE = [(3, 7, 5, 1, 1, 1, 0), (5, 9, 13, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 0), (1, 3, 43, 1, 1, 1, 0), (1, 1, 257, 1, 1, 1, 0)]
SHRINK_GROW = [(2, 9, 7, 3, 3, 1, 0), (2, 9, 9, 3, 3, 1, 2)]
RECT = [(2, 8, 9, 1, 3, 1, 1), (2, 8, 9, 3, 1, 1, 1)]
STRIDED = [(3, 9, 11, 3, 3, 2, 1), (3, 10, 12, 3, 3, 2, 1), (3, 9, 11, 1, 1, 2, 0)]
BOTH = SAME + POINTWISE                                         # both families, both passes
PLANE_FWD = BOTH + SHRINK_GROW + RECT + STRIDED
PLANE_DGRAD = BOTH + SHRINK_GROW
TILE5 = [(1, 5, 63, 3, 3, 1, 1), (3, 1, 9, 3, 3, 1, 1), SAME[2], SAME[3]]
TILE7_WIDTHS, TILE7_HEIGHTS = (1, 7, 63, 64, 126), (5, 1)
TILE7 = [(2, h, w, 3, 3, 1, 1) for h in TILE7_HEIGHTS for w in TILE7_WIDTHS]
RAGGED_SAME, RAGGED_PW = SAME[1], POINTWISE[1]
FWD_EPILOGUES = (0, BIAS, ADDEND, RELU, BIAS | ADDEND | RELU, STATS, STATS | BIAS)
DGRAD_MODES = ((0, ""), (ADDEND, ""), (0, "bn"), (0, "bn-nomask"), (ADDEND, "bn2"))         # (epi, fuse)
K_CYCLE = (32, 96, 128)
TILE7_K = (16, 32, 48, 64)


def _case(family, dgrad, nplanes, geom, kg, ncol, groups, tile, epi=0, io=0, fuse=""):
    """kg: GEMM-K channels per group, ncol: GEMM columns per group (the forward: input / output channels; the input gradient:
    output / input channels of the layer)"""
    cin, cout = (ncol * groups, kg * groups) if dgrad else (kg * groups, ncol * groups)
    B, H, W, kh, kw, stride, pad = geom
    return Case(family, dgrad, nplanes, B, H, W, cin, cout, kh, kw, stride, pad, groups, tile, epi, io, fuse)


def geom_of(c):
    return (c.B, c.H, c.W, c.kh, c.kw, c.stride, c.pad)


def shape_of(c):
    return (c.B, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.groups)


def gemm_of(c):
    """(M, GEMM-K per group, GEMM columns per group) of the case's launch"""
    Ho, Wo = out_map(c)
    if c.dgrad:
        return c.B * c.H * c.W, c.cout // c.groups, c.cin // c.groups
    return c.B * Ho * Wo, c.cin // c.groups, c.cout // c.groups


def tile_rows(c):
    return PLANE_BM[c.tile] if c.family == "planes" else X3_BM[c.tile]


def ragged(c):
    """more than one M tile, the last one partly filled"""
    M = gemm_of(c)[0]
    return M > tile_rows(c) and M % tile_rows(c) != 0


def epi_bits(c):
    return c.epi | FUSE_BITS[c.fuse]


def query_of(c):
    """(name, arguments) of the *_tile_ok query that says naming c.tile runs its kernel"""
    if c.family == "planes":
        if c.dgrad:
            return "dgrad_planes_tile_ok", (*shape_of(c), c.nplanes, c.tile, epi_bits(c))
        return "fwd_planes_tile_ok", (*shape_of(c), c.nplanes, c.tile, epi_bits(c), c.io)
    return ("dgrad_x3_tile_ok" if c.dgrad else "fwd_x3_tile_ok"), (*shape_of(c), c.tile, epi_bits(c))


def legal(c):
    """the rules of the three families, restated (csrc/conv_planes.hip pconv_channels_ok / pconv_named_tile_ok / phalo_ok /
    ppersist_ok, csrc/conv_x3.hip x3_filter_ok / x3_channels_ok / x3_tile_ok, csrc/conv_xhalo.hip sc_xhalo_ok) for shapes far
    from the byte guards: what the table below leaves out.  tests/test_split_tiles_cpu.py holds it against the queries."""
    M, kg, ncol = gemm_of(c)
    taps = c.kh * c.kw
    same3 = (c.kh, c.kw, c.stride, c.pad) == (3, 3, 1, 1)
    if c.family == "planes":
        if kg % 32 or ncol % 64 or (c.dgrad and c.stride != 1):
            return False
        t = c.tile
        return {0: ncol % 128 == 0, 1: True, 2: c.nplanes == 3, 3: c.nplanes == 3, 4: c.nplanes == 3 and ncol % 128 == 0,
                5: same3 and c.W <= 63,
                6: taps * (kg // 32) >= 2 and not (c.epi & STATS and c.epi & (BIAS | ADDEND)) and not c.io & Y}[t]
    if c.io or c.nplanes != 3 or c.stride != 1 or c.kh != c.kw or not c.kh & 1 or c.kh > 5 or 2 * c.pad != c.kh - 1:
        return False
    if c.tile == 7:
        return same3 and c.W <= 126 and ncol == 32 and kg % 16 == 0 and (c.dgrad or not c.epi & (BIAS | ADDEND))
    return kg % 32 == 0 and taps * (kg // 32) >= 2 and ncol % X3_BN[c.tile] == 0


def _cases():
    out = []

    def add(*a, **k):
        c = _case(*a, **k)
        if legal(c):
            out.append(c)

    fams = (("planes", 3), ("planes", 1), ("x3", 3))
    # ---- every geometry on one 256-row tile and on one tile of another height
    for family, np_ in fams:
        for dgrad in (False, True):
            geoms = BOTH if family == "x3" else PLANE_DGRAD if dgrad else PLANE_FWD
            for gi, geom in enumerate(geoms):
                kg = K_CYCLE[gi % 3]
                if geom[3] * geom[4] == 1 and kg == 32:
                    kg = 64                                         # (a pointwise layer needs two K tiles: x3, plane tile 6)
                if family == "x3":
                    ncol = (256, 128, 64, 96, 32)[gi % 5]
                    tiles = {256: (0, 1), 128: (4, 2), 64: (4, 3), 96: (5, 6), 32: (5, 6)}[ncol]
                elif np_ == 3:
                    ncol = (256, 128, 64)[gi % 3]
                    tiles = {256: (4, 0), 128: (4, 2), 64: (6, 3)}[ncol]
                else:
                    ncol = (128, 64, 256)[gi % 3]
                    tiles = (6, 0 if ncol % 128 == 0 else 1)
                for tile in tiles:
                    add(family, dgrad, np_, geom, kg, ncol, 1, tile)
    # ---- every tile on the two ragged geometries: K 32 (pointwise: 64), 96, 128; 256 columns (BN = 128 instances of plane tiles
    # 5 / 6) and 64 (their BN = 64 instances); 96 columns on the register-split tiles 5 / 6
    for family, np_ in fams:
        for dgrad in (False, True):
            for geom, kg in ((RAGGED_SAME, 32), (RAGGED_PW, 64), (RAGGED_SAME, 96), (RAGGED_PW, 128)):
                for tile in range(7):
                    add(family, dgrad, np_, geom, kg, 256, 1, tile)
                    add(family, dgrad, np_, geom, kg, 64, 1, tile)
                if family == "x3":
                    for tile in (5, 6):
                        add(family, dgrad, np_, geom, kg, 96, 1, tile)
    # ---- forward epilogues on every tile (the queries refuse: tile 7 bias / addend, plane tile 6 statistics + bias)
    for family, np_ in fams:
        for geom in (RAGGED_SAME, RAGGED_PW):
            for epi in FWD_EPILOGUES:
                for tile in range(7):
                    add(family, False, np_, geom, 64, 256, 1, tile, epi=epi)
    for epi in FWD_EPILOGUES:
        add("x3", False, 3, RAGGED_SAME, 64, 32, 1, 7, epi=epi)
    # ---- the plane forward with a bf16-stored output (tiles 0-5; tile 6 is refused)
    for np_ in (3, 1):
        for geom in (RAGGED_SAME, RAGGED_PW):
            for epi in (0, BIAS | ADDEND | RELU):
                for tile in range(7):
                    add("planes", False, np_, geom, 64, 256, 1, tile, epi=epi, io=Y)
    # ---- input gradient: plain, addend, fused BatchNorm backward (mask, no mask, two BatchNorms + addend), on every tile
    for epi, fuse in DGRAD_MODES:
        for family, np_ in fams:
            for geom in (RAGGED_SAME, RAGGED_PW):
                for tile in range(7):
                    add(family, True, np_, geom, 64, 256, 1, tile, epi=epi, fuse=fuse)
        for kg in (64, 48):
            add("x3", True, 3, RAGGED_SAME, kg, 32, 1, 7, epi=epi, fuse=fuse)
    # ---- groups 2 and 3 with 32 and 64 channels per group, one column tile per group and two
    for geom in (RAGGED_SAME, RAGGED_PW):
        pw = geom[3] * geom[4] == 1
        for dgrad in (False, True):
            for groups, kg, ncol, tiles in ((2, 32, 128, (0, 2)), (3, 64, 128, (4, 3)), (2, 64, 64, (6, 5))):
                for tile in tiles:
                    add("planes", dgrad, 3, geom, kg, ncol, groups, tile)
            for groups, kg, ncol, tiles in ((2, 32, 128, (0, 1)), (3, 64, 128, (6, 1)), (2, 64, 64, (5, 1))):
                for tile in tiles:
                    add("planes", dgrad, 1, geom, kg, ncol, groups, tile)
            for groups, kg, ncol, tiles in ((2, 32, 64, (2, 6)), (3, 64, 128, (0, 3)), (3, 32, 32, (5,)), (2, 64, 64, (4, 5))):
                for tile in tiles:
                    add("x3", dgrad, 3, geom, 64 if pw and kg == 32 else kg, ncol, groups, tile)
    # ---- plane tile 5: the width limit, height 1, width 1, 1 x 1 maps (with tile 0 / 1 next to it)
    for np_ in (3, 1):
        for dgrad in (False, True):
            for gi, geom in enumerate(TILE5):
                ncol = (128, 64)[gi & 1]
                for tile in (5, 0 if ncol == 128 else 1):
                    add("planes", dgrad, np_, geom, K_CYCLE[gi % 3], ncol, 1, tile)
    # ---- tile 7: K per group 16, 32, 48, 64 in 1, 2 and 3 groups; its widths and heights; the same-size geometries
    for dgrad in (False, True):
        for kg in TILE7_K:
            for groups in (1, 2, 3):
                add("x3", dgrad, 3, RAGGED_SAME, kg, 32, groups, 7)
        for gi, geom in enumerate(TILE7 + SAME[:4]):
            add("x3", dgrad, 3, geom, TILE7_K[gi % 4], 32, (1, 2, 3)[gi % 3], 7)
            add("x3", dgrad, 3, geom, TILE7_K[(gi + 1) % 4], 32, 1, 7, epi=0 if dgrad else STATS, fuse="bn" if dgrad else "")
    return list(dict.fromkeys(out))                # (the sweeps overlap in a few cases: each once)


CASES = _cases()

# hints that fall back (conv_planes.hip dispatch_pconv maps them to tile 0 / 1): the query answers 0; no cases
ONE_PLANE_FALLBACKS = [_case("planes", dgrad, 1, RAGGED_SAME, 64, 256, 1, tile) for dgrad in (False, True) for tile in (2, 3, 4)]
# refusals the GPU file asserts through query and call: (case, text of the error)
REFUSALS = (
    [(_case("x3", False, 3, RAGGED_SAME, 64, 32, 1, 7, epi=epi), "tile 7") for epi in (BIAS, ADDEND)] +
    [(_case("planes", False, np_, RAGGED_SAME, 64, 256, 1, 6, epi=STATS | e), "tile 6") for np_ in (3, 1) for e in (BIAS, ADDEND)] +
    [(_case("planes", False, np_, RAGGED_SAME, 64, 256, 1, 6, io=Y), "tile 6") for np_ in (3, 1)] +
    [(_case("planes", True, np_, geom, 64, 128, 1, 1), "stride") for np_ in (3, 1) for geom in STRIDED] +
    [(_case("x3", dgrad, 3, (2, 5, 127, 3, 3, 1, 1), 32, 32, 1, 7), "tile 7") for dgrad in (False, True)])
# query only (the entry re-routes the hint by design): plane tile 5 at width 64
TILE5_TOO_WIDE = [_case("planes", dgrad, np_, (1, 5, 64, 3, 3, 1, 1), 32, 64, 1, 5) for np_ in (3, 1) for dgrad in (False, True)]


def case_id(c, tile=True):
    s = "%s%d-%s-%dx%dx%d-%dto%dg%d-k%dx%ds%dp%d-e%d-io%d%s" % (
        c.family, c.nplanes, "dgrad" if c.dgrad else "fwd", c.B, c.H, c.W, c.cin, c.cout, c.groups, c.kh, c.kw, c.stride, c.pad, c.epi,
        c.io, "-" + c.fuse if c.fuse else "")
    return s + "-t%d" % c.tile if tile else s


def kernel_name(c):
    if c.family == "planes":
        return "pconv_%s<%s>" % ("dgrad" if c.dgrad else "fwd", "bf16x3" if c.nplanes == 3 else "bf16")
    stem = "xhalo" if c.tile == 7 else "xconv3" if c.kh > 1 or c.groups > 1 else "xconv"
    return "%s_%s%s<bf16x3>" % (stem, "dgrad" if c.dgrad else "fwd", "+bn_bwd" if c.fuse else "")


def instance_of(c):
    """the template instance the case runs (dispatch_pconv, dispatch_x3, sc_launch_xhalo restated)"""
    ncol = gemm_of(c)[2]
    if c.family == "planes":
        bn = 128 if ncol % 128 == 0 else 64
        if c.tile == 6:
            return ("ppersist", bn, c.nplanes, c.dgrad)
        if c.tile == 5:
            return ("phalo", bn, c.nplanes, c.dgrad)
        inst = {(3, 0): (128, 128, 3, 3), (3, 1): (128, 64, 3, 3), (3, 2): (128, 64, 3, 2), (3, 3): (64, 64, 3, 2),
                (3, 4): (256, 128, 3, 2), (1, 0): (128, 128, 1, 3), (1, 1): (128, 64, 1, 3)}[(c.nplanes, c.tile)]
        return ("pconv",) + inst + (c.dgrad,)
    if c.tile == 7:
        return ("xhalo", 12 if 256 + 2 * c.W + 2 <= 12 * 32 else 16, c.dgrad)
    return ("xgemm", c.tile, c.dgrad, c.kh > 1 or c.groups > 1)


def data_key(c):
    return (c.dgrad,) + shape_of(c)


# groups of cases that differ in the tile only: one reference, and the bit comparison across tiles; ordered so that the groups
# of one shape (both families, every epilogue) follow each other and share the operands and the fp64 result
_tileless = lambda c: (data_key(c), c._replace(tile=0))
GROUPS = [list(g) for _, g in itertools.groupby(sorted(CASES, key=_tileless), key=_tileless)]


def K():
    from scouter_amd import kernels
    return kernels


@functools.lru_cache(maxsize=2)
def _data(key):
    """key: data_key of a case -> operands on the device (fp32), made once per shape and shared by the families, tiles, epilogues
    and storages listed for it; the fp64 results are added by _ref, the BatchNorm operands by _bn"""
    dgrad, B, H, W, cin, cout, kh, kw, stride, pad, groups = key
    c = Case("planes", dgrad, 3, B, H, W, cin, cout, kh, kw, stride, pad, groups, 0, 0, 0, "")
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    Ho, Wo = out_map(c)
    M, kg, ncol = gemm_of(c)
    a = torch.randn((B, Ho, Wo, cout) if dgrad else (B, H, W, cin), generator=gen)
    w = torch.randn(kh, kw, cin // groups, cout, generator=gen) / (kg * kh * kw) ** 0.5
    n = ncol * groups
    oshape = (B, H, W, n) if dgrad else (B, Ho, Wo, n)
    bias = torch.randn(n, generator=gen)
    addend = torch.randn(oshape, generator=gen)
    xbn = [torch.randn(oshape, generator=gen) * 1.3 + 0.2 for _ in range(2)] if dgrad else []
    return dict(c=c, a=a.cuda(), w=w.cuda(), a_cpu=a, w_cpu=w, bias=bias.cuda(), addend=addend.cuda(), xbn=xbn, oshape=oshape)


def _ref(d, bf16):
    """-> (fp64 result of what the kernels multiply, sum of its squared terms), on the CPU, once per shape and operand rounding"""
    if ("ref", bf16) not in d:
        c = d["c"]
        a64, w64 = _opnd(d["a_cpu"], bf16), _opnd(d["w_cpu"], bf16)
        d["ref", bf16] = (_conv64(a64, w64, c, c.dgrad), _conv64(a64 * a64, w64 * w64, c, c.dgrad))
    return d["ref", bf16]


def _bn(d):
    """the BatchNorm operands of the fused backward: [(x, saved block [4][C], ReLU mask words, mask as booleans)] of two BatchNorms
    over the gradient's tensor, from kernels.bn_fwd(..., want_mask=True)"""
    if "bn" not in d:
        kk = K()
        C = d["oshape"][-1]
        one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        d["bn"] = []
        for x in d["xbn"]:
            x = x.cuda()
            y, saved, mask = kk.bn_fwd(x, one, zero, zero.clone(), one.clone(), True, True, want_mask=True)
            d["bn"].append((x, saved, mask, (y > 0).cpu()))
    return d["bn"]


def _operands(kk, c, d):
    """-> (A operand, weight operand) as the family's entry point takes them: planes of the library's own split, or fp32"""
    key = ("opnd", c.family, c.nplanes)
    if key not in d:
        wf, wd = kk.planes_split_weight(d["w"], c.groups, c.nplanes, fwd=not c.dgrad, dgrad=c.dgrad)
        d[key] = (kk.planes_split(d["a"], c.nplanes) if c.family == "planes" else d["a"], wd if c.dgrad else wf)
    return d[key]


def partial_rows(kk, c):
    """rows of statistics / fused BatchNorm-backward partials the case's kernel writes"""
    M, kg, ncol = gemm_of(c)
    if c.family == "planes":
        return kk.ask("planes_partial_rows", M, c.tile)
    return kk.ask("x3_halo_partial_rows", c.groups) if c.tile == 7 else kk.ask("x3_partial_rows", M, ncol, c.tile)


SENTINEL = -777.25


def _partials(rows, N):
    part = torch.full((rows + 1, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    part[rows] = SENTINEL
    return part


def _launch(kk, c, d):
    """one launch of the case -> (rc, profiled kernel names, y [M][N], its guarded buffer as integers, partial rows or None)"""
    from scouter_amd import _native
    L, p, st = _native.lib(), kk._p, kk._stream()
    M, kg, ncol = gemm_of(c)
    N = ncol * c.groups
    a, w = _operands(kk, c, d)
    buf, y = _guarded(M, N, torch.bfloat16 if c.io & Y else torch.float32)
    addend = d["addend"] if c.epi & ADDEND else None
    bias = d["bias"] if c.epi & BIAS else None
    relu = int(bool(c.epi & RELU))
    s = shape_of(c)
    parts = None
    if c.epi & STATS:
        parts = [_partials(partial_rows(kk, c), N)]
    fuse = (None,) * 7
    if c.fuse:
        bn = _bn(d)
        parts = [_partials(partial_rows(kk, c), N) for _ in range(2 if c.fuse == "bn2" else 1)]
        (x1, s1, m1, _), (x2, s2, _, _) = bn
        fuse = (None if c.fuse == "bn-nomask" else p(m1), p(x1), p(s1), p(parts[0])) + \
               ((p(x2), p(s2), p(parts[1])) if c.fuse == "bn2" else (None, None, None))
    if c.family == "planes" and not c.dgrad:
        fn = lambda: L.scouter_conv2d_fwd_planes_io(p(a), p(w), p(bias), p(addend), p(y), p(parts[0]) if parts else None, *s, relu,
                                                    c.nplanes, c.tile, c.io, st)
    elif c.family == "planes":
        fn = lambda: L.scouter_conv2d_dgrad_planes_bnbwd(p(a), p(w), p(addend), p(y), *s, c.nplanes, c.tile, *fuse, st)
    elif not c.dgrad:
        fn = lambda: L.scouter_conv2d_fwd_x3(p(a), p(w), p(bias), p(addend), p(y), p(parts[0]) if parts else None, *s[:7], c.pad,
                                             c.groups, relu, c.tile, st)
    else:
        fn = lambda: L.scouter_conv2d_dgrad_x3_bnbwd(p(a), p(w), p(addend), p(y), *s[:7], c.pad, c.groups, c.tile, *fuse, st)
    rc, names = _profiled(fn)
    return rc, names, y.view(M, N), buf, parts


def _expected(c, d):
    """-> fp64 reference and V of the case's epilogue and storage (before the ReLU mask of a fused BatchNorm backward)"""
    ref, sq = _ref(d, c.nplanes == 1)
    if c.epi & BIAS:
        b = d["bias"].double().cpu()
        ref, sq = ref + b, sq + b * b
    if c.epi & ADDEND:
        ad = d["addend"].double().cpu()
        ref, sq = ref + ad, sq + ad * ad
    if c.epi & RELU:
        ref = ref.clamp_min(0)
    return ref, sq.sqrt()


WORST = collections.defaultdict(float)              # (family, pass) -> worst |err| / bound of this run (printed per test)


def _run_checked(kk, c, d):
    """checks 1-5, 7 and 8 of the module docstring on one case -> the output's bits"""
    from scouter_amd import _native
    name = case_id(c)
    M, kg, ncol = gemm_of(c)
    N = ncol * c.groups
    qname, qargs = query_of(c)
    assert kk.ask(qname, *qargs) == 1, "%s: %s%r answers 0" % (name, qname, qargs)
    outs = []
    for _ in range(2):
        rc, names, y, buf, parts = _launch(kk, c, d)
        _native.check(rc, name)                                   # (a generated case the library refuses is a failure)
        assert names == [kernel_name(c)], (name, names)
        pat = buf[0].clone()
        assert bool((buf[:GUARD * N] == pat).all()) and bool((buf[(GUARD + M) * N:] == pat).all()), "%s: guard rows written" % name
        outs.append((y, buf, parts))
    (y, buf, parts), (_, buf2, parts2) = outs
    assert torch.equal(buf, buf2), "%s: two launches differ" % name
    got = y.double().cpu().view(d["oshape"])
    assert bool(torch.isfinite(got).all()), "%s: %d elements not written or not finite" % (name, int((~torch.isfinite(got)).sum()))
    ref, mag = _expected(c, d)
    live = None
    if c.fuse and c.fuse != "bn-nomask":
        live = _bn(d)[0][3]
        assert bool((got[~live] == 0).all()), "%s: %d masked elements are not exactly 0" % (name, int((got[~live] != 0).sum()))
        assert 0.2 < float(live.float().mean()) < 0.8
        ref = torch.where(live, ref, torch.zeros_like(ref))
    k = _k_for(kg * c.kh * c.kw)
    if y.dtype == torch.bfloat16:
        mag = mag + ref.abs() * 2.0 ** -8 / k
    worst = float(((got - ref).abs() / (k * mag + 1e-12)).max())
    fam = "%s%s %s" % ("tile 7" if c.tile == 7 else c.family, "" if c.family == "x3" else " %d" % c.nplanes, "dgrad" if c.dgrad else "fwd")
    WORST[fam] = max(WORST[fam], worst)
    print("%s: worst |err| / bound = %.3g (%s so far %.3g)" % (name, worst, fam, WORST[fam]))
    _check(name, got, ref, mag, k)
    if parts is None:
        return buf
    rows = parts[0].shape[0] - 1
    for part, part2 in zip(parts, parts2):
        assert bool((part[rows] == SENTINEL).all()), "%s: the sentinel row of the partials was written" % name
        assert bool(torch.isfinite(part[:rows]).all()), "%s: partial rows not written" % name
        assert torch.equal(part, part2), "%s: partials of two launches differ" % name
    y64 = y.double().cpu()
    if c.epi & STATS:
        sums = parts[0][:rows].sum(0).cpu()
        for j, want in enumerate((y64.sum(0), (y64 * y64).sum(0))):
            err = (sums[:, j] - want).abs()
            assert bool((err <= 1e-8 + 1e-10 * want.abs()).all()), "%s: statistics column %d off by %.3g" % (name, j, float(err.max()))
        plain = _launch(kk, c._replace(epi=c.epi & ~STATS), d)
        assert plain[0] == 0 and torch.equal(plain[3], buf), "%s: y differs from the launch without statistics" % name
    else:
        gsum = y64.sum(0)
        for part, (x, saved, _, _) in zip(parts, _bn(d)):
            s = part[:rows].sum(0).cpu()
            xh = ((x - saved[0]) * saved[1]).double().cpu().view(M, N)
            torch.testing.assert_close(s[:, 0], gsum, rtol=1e-9, atol=1e-6, msg=lambda m: "%s: sum g: %s" % (name, m))
            torch.testing.assert_close(s[:, 1], (y64 * xh).sum(0), rtol=1e-6, atol=1e-4, msg=lambda m: "%s: sum g xhat: %s" % (name, m))
    return buf


def _group_id(g):
    return case_id(g[0], tile=False) + "-t" + ".".join(str(c.tile) for c in g)


@pytest.mark.parametrize("group", GROUPS, ids=_group_id)
def test_named_tiles_against_fp64_and_against_each_other(group):
    kk = K()
    c0 = group[0]
    d = _data(data_key(c0))
    bits = {c.tile: _run_checked(kk, c, d) for c in group}
    same = [t for t in bits if t in SAME_BITS[c0.family]]
    for t in same[1:]:
        assert torch.equal(bits[t], bits[same[0]]), "%s: tiles %d and %d differ in their bits" % (case_id(c0, tile=False), same[0], t)
    # where the plane family takes the shape, the register-split result equals the three-plane result on the pre-split operand
    twin = c0._replace(family="planes", tile=1)
    if c0.family == "x3" and same and kk.ask(*_flat(query_of(twin))) == 1:
        rc, names, _, buf, _ = _launch(kk, twin, d)
        assert rc == 0 and names == [kernel_name(twin)], (case_id(twin), rc, names)
        assert torch.equal(buf, bits[same[0]]), "%s: the register-split and the plane result differ in their bits" % case_id(c0, tile=False)


def _flat(q):
    return (q[0],) + tuple(q[1])


def persistent_batch(cus):
    """B of 15 x 17 maps with cus + 2 M tiles of 256 rows, the last one ragged"""
    B = ((cus + 1) * 256) // 255 + 1
    assert -(-B * 255 // 256) == cus + 2 and B * 255 % 256 != 0, (cus, B)
    return B


PERSISTENT = [("planes", 3, False, 6), ("planes", 3, True, 6), ("planes", 1, False, 6), ("planes", 1, True, 6), ("x3", 3, False, 7),
              ("x3", 3, True, 7)]


def persistent_case(family, nplanes, dgrad, tile, cus):
    kg, ncol = (64, 32) if tile == 7 else (32, 64)
    return _case(family, dgrad, nplanes, (persistent_batch(cus), 15, 17, 3, 3, 1, 1), kg, ncol, 1, tile, epi=0 if dgrad else STATS,
                 fuse="bn" if dgrad else "")


@pytest.mark.parametrize("family,nplanes,dgrad,tile", PERSISTENT, ids=lambda v: str(v))
def test_persistent_kernels_walk_a_second_round_of_tiles(family, nplanes, dgrad, tile):
    """more 256-row M tiles than workgroups (CU count + 2, the last one ragged): the second round of the tile walk of plane
    tile 6 and tile 7, the forward with statistics, the input gradient with the fused BatchNorm backward (both are summed over
    all tiles of a workgroup)"""
    kk = K()
    c = persistent_case(family, nplanes, dgrad, tile, torch.cuda.get_device_properties(0).multi_processor_count)
    d = _data(data_key(c))
    _run_checked(kk, c, d)
    _run_checked(kk, c._replace(epi=0, fuse=""), d)
    _data.cache_clear()
    _free()


def _raw_call(kk, c):
    """the case's entry point on zero operands (refusals: nothing may be launched or written) -> (rc, message, names, output)"""
    from scouter_amd import _native
    L, p, st = _native.lib(), kk._p, kk._stream()
    Ho, Wo = out_map(c)
    M, kg, ncol = gemm_of(c)
    N = ncol * c.groups
    np_ = c.nplanes if c.family == "planes" else 1
    a = torch.zeros((np_, c.B, Ho, Wo, c.cout) if c.dgrad else (np_, c.B, c.H, c.W, c.cin), device="cuda",
                    dtype=torch.bfloat16 if c.family == "planes" else torch.float32)
    w = torch.zeros(3 * c.kh * c.kw * (c.cin // c.groups) * c.cout, device="cuda", dtype=torch.bfloat16)
    buf, y = _guarded(M, N, torch.bfloat16 if c.io & Y else torch.float32)
    vec = torch.zeros(N, device="cuda")
    full = torch.zeros(M, N, device="cuda")
    bias, addend = (vec if c.epi & BIAS else None), (full if c.epi & ADDEND else None)
    part = _partials(4 * (M // 256 + 1), N) if c.epi & STATS else None
    s = shape_of(c)
    if c.family == "planes" and not c.dgrad:
        fn = lambda: L.scouter_conv2d_fwd_planes_io(p(a), p(w), p(bias), p(addend), p(y), p(part), *s, 0, c.nplanes, c.tile, c.io, st)
    elif c.family == "planes":
        fn = lambda: L.scouter_conv2d_dgrad_planes_bnbwd(p(a), p(w), p(addend), p(y), *s, c.nplanes, c.tile, *(None,) * 7, st)
    elif not c.dgrad:
        fn = lambda: L.scouter_conv2d_fwd_x3(p(a), p(w), p(bias), p(addend), p(y), p(part), *s[:7], c.pad, c.groups, 0, c.tile, st)
    else:
        fn = lambda: L.scouter_conv2d_dgrad_x3_bnbwd(p(a), p(w), p(addend), p(y), *s[:7], c.pad, c.groups, c.tile, *(None,) * 7, st)
    rc, msg, names = _refusal(fn)
    return rc, msg, names, buf


@pytest.mark.parametrize("case,text", REFUSALS, ids=lambda v: case_id(v) if isinstance(v, Case) else None)
def test_what_a_rule_refuses_is_refused_by_query_and_call(case, text):
    """rc -3 (SC_ERR_UNSUPPORTED), the output untouched, and the query answers 0.  (Plane tile 6 refuses inside the profiler scope
    of its entry point, which then reports the scope's name without a kernel: the untouched output is the proof here.)"""
    kk = K()
    assert kk.ask(*_flat(query_of(case))) == 0, case_id(case)
    rc, msg, names, buf = _raw_call(kk, case)
    assert rc == -3 and text in msg, (case_id(case), rc, msg, names)
    assert names == [] or "tile 6" in text, (case_id(case), names)
    assert bool((buf == buf[0]).all()), "a refused call wrote its output"


def test_hints_that_fall_back_answer_zero():
    """plane tiles 2 / 3 / 4 at one plane and plane tile 5 on a map 64 wide are hints the entry re-routes by design: the query says
    so, and next to each the tile that does run answers 1"""
    kk = K()
    for c in ONE_PLANE_FALLBACKS + TILE5_TOO_WIDE:
        assert kk.ask(*_flat(query_of(c))) == 0, case_id(c)
        assert kk.ask(*_flat(query_of(c._replace(tile=1)))) == 1, case_id(c)
    for c in TILE5_TOO_WIDE:
        assert kk.ask(*_flat(query_of(c._replace(W=63)))) == 1, case_id(c)
