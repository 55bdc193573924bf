"""The forward and input-gradient implicit-GEMM kernels at every named tile, against fp64, on ragged shapes (-m gpu).

csrc/conv_igemm.hip igemm_kernel<BM, BN, WM, WN, DGRAD, STRIDED, PW, FUSE> and csrc/conv_bf16.hip igemm_bf16_kernel<BM, BN, WM, WN,
KT, DGRAD, A_BF16> run every convolution the plane and register-split kernels do not take.  Here the C ABI is called directly
(scouter_conv2d_fwd_f32, scouter_conv2d_dgrad_f32, scouter_conv2d_fwd_bf16_io, scouter_conv2d_dgrad_bnbwd_bf16_io) with the tile as
tile_hint, on the smallest shapes that reach each path.  tests/test_conv_tiles_cpu.py asks the library's queries (no device) that
every case names a tile the entry point runs, and counts that the table reaches every kernel instance.

GEOMETRIES (B, H, W, kh, kw, stride, pad) -- B, H, W the layer's INPUT map; the GEMM rows M are the forward's output pixels, the
input gradient's input pixels:
  general addressing (block-relative buffer offsets + one tap-mask word per row)
    (3, 7, 5, 3, 3, 1, 1)     M = 105: less than one tile, three images inside it
    (5, 9, 13, 3, 3, 1, 1)    M = 585: a ragged last tile for BM = 128 (73 rows) and BM = 64 (9 rows), images ending inside tiles
    (5, 34, 1, 3, 3, 1, 1)    width 1: every row of a tile carries into the next map row
    (40, 1, 1, 3, 3, 1, 1)    1 x 1 maps: every row carries into the next image, only the centre tap is valid
    (2, 9, 7, 3, 3, 1, 0)     shrinking (pad 0): the output map is smaller than the input map
    (2, 9, 9, 3, 3, 1, 2)     growing (pad 2): border outputs with no valid tap at all
    (2, 9, 9, 5, 5, 1, 2)     25 taps: the highest bits of the tap mask the models use
    (2, 8, 9, 1, 3, 1, 1), (2, 8, 9, 3, 1, 1, 1)    rectangular filters: the r * S + q tap index
  strided (the forward: the general kernel with stride 2; the input gradient: the STRIDED instantiation, per-tap divisibility)
    (3, 9, 11, 3, 3, 2, 1)    odd sizes
    (3, 10, 12, 3, 3, 2, 1)   even sizes: the last input row and column miss taps (iy < H)
    (3, 9, 11, 1, 1, 2, 0)    the downsample: the input gradient writes zeros at odd coordinates
  pointwise (the PW instantiation of the fp32 kernel: no pixel walk, the A descriptor ends at the block's valid rows; the bf16
  kernel has no such instantiation and walks these like any other)
    (3, 7, 5, 1, 1, 1, 0) M = 105, (5, 9, 13, 1, 1, 1, 0) M = 585, (1, 1, 1, 1, 1, 1, 0) M = 1, (1, 3, 43, 1, 1, 1, 0) M = 129: a
    second tile of one row
CHANNELS: GEMM columns per group 256 (tile 0: two column tiles; all four tiles legal), 128 (tiles 1 / 2: two column tiles), 96
(tile 3 only: three column tiles); GEMM-K per group 32 (one K chunk per tap; pointwise: ONE K tile, no pipeline), 96 (three chunks;
the bf16 kernel's KT = 32 path), 128 (its KT = 64 path); groups 2 and 3 with 32 and 64 channels per group, one of them with two
column tiles per group (the grp / nt_id / mt_id split of the block index on all three factors).
EPILOGUES: the forward on the two M = 585 geometries on every tile: none, bias, addend, ReLU, bias + addend + ReLU, BatchNorm
statistics, statistics + bias; the input gradient: plain and addend.  bf16 storage: forward io 0 / X / Y / X|Y, input gradient io 0 /
8 (dy) / 4 (addend), without the fused BatchNorm-backward epilogue (which keeps its own test); the strided input gradient on the
bf16 entry is refused.  The bf16 kernel's one-stage / two-stage switch (ONE_STAGE_MAX = 32 K tiles, input gradients only): 3x3 with
192 GEMM-K channels (27 tiles), 1x1 with 2048 (32), 3x3 with 256 (36); forwards with one K tile and with two.

Per case the output lies inside a larger buffer prefilled with NaN bit patterns, 128 guard rows in front of it and behind it:
  * the library profiler names exactly the kernel asked for (switch bhalo is off for the launch: the resident-rows kernel, which
    the library runs BEHIND bf16 tiles 1 / 3 on 3x3 layers with 32 channels per group, would report its own name and fail this);
  * every element is finite and within the project's bound of the fp64 result on the CPU (F.conv2d / torch.nn.grad.conv2d_input on
    doubles; bf16 cases: of the RNE-rounded operands),
        |err| <= _k_for(Cg * kh * kw) * V + 1e-12,   V = sqrt(sum of squared terms)    (tests/test_size_thresholds_gpu.py)
    V by the same operators on the squares (plus the squares of bias and addend); a bf16-stored output adds 2^-8 |ref|;
  * the guard rows keep their bits; a second launch gives the same bits;
  * forward: every legal tile 0-3 of the case's shape gives the same bits (the promise kernels._pick_tile states and
    tests/test_model_gpu.py relies on); input gradient: whether they do is printed, not asserted;
  * forward with statistics: bn_partial has the rows the *_bn_partial_rows* query names plus one sentinel row; the column sums equal
    the fp64 sums of the kernel's own output (rtol 1e-10, atol 1e-8: the bound of test_conv_fused_bn_statistics), y is bit-equal to
    the launch without statistics, the sentinel row is untouched.
Inputs are standard normal from seeded generators, weights scaled by 1 / sqrt(Cg * kh * kw): one dropped or doubled tap or pixel
moves an element by orders more than the bound.

THE TWO LIMITS of the shared block prologue (csrc/conv_common.h sc_tap_mask_ok, sc_pixel_walk_ok; proved in
tests/test_conv_tiles_cpu.py): a 7x7 layer is refused (rc -3, nothing launched) by all four entry points, and a 3x3 forward runs at
the largest map the pixel-walk rule admits at width 255 and is refused one map row later."""
import collections
import functools
import itertools
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_size_thresholds_gpu import _check, _k_for, _no_lost_tail, _pick, _profiled, _sample_fwd, _free, _gen     # noqa: E402
from test_table_entries_gpu import _opnd                                                                           # noqa: E402

pytestmark = pytest.mark.gpu

BIAS, ADDEND, RELU, STATS = 1, 2, 4, 8              # SCOUTER_EPI_*
X, Y = 1, 2                                         # SCOUTER_IO_X_BF16 / _Y_BF16 (forward)
ADD, DY = 4, 8                                      # SCOUTER_DGRAD_IO_* (input gradient): the addend / dy is stored as bf16
TILE_NAME = ("128x128", "128x64", "64x64", "128x32")
TILE_BM = (128, 128, 64, 128)
TILE_BN = (128, 64, 64, 32)
GUARD = 128                                         # sentinel rows on either side of the output
ONE_STAGE_MAX = 32                                  # csrc/conv_bf16.hip launch_bf16

# kind: "fp32" | "bf16" (the entry point); dgrad: the input gradient; B, H, W: the layer's input map; cin, cout: the layer's
# channels (all groups); tile: tile_hint; epi: SCOUTER_EPI_* bits; io: storage bits of the bf16 entry points
Case = collections.namedtuple("Case", "kind dgrad B H W cin cout kh kw stride pad groups tile epi io")

GENERAL = [(3, 7, 5, 3, 3, 1, 1), (5, 9, 13, 3, 3, 1, 1), (5, 34, 1, 3, 3, 1, 1), (40, 1, 1, 3, 3, 1, 1), (2, 9, 7, 3, 3, 1, 0),
           (2, 9, 9, 3, 3, 1, 2), (2, 9, 9, 5, 5, 1, 2), (2, 8, 9, 1, 3, 1, 1), (2, 8, 9, 3, 1, 1, 1)]
STRIDED = [(3, 9, 11, 3, 3, 2, 1), (3, 10, 12, 3, 3, 2, 1), (3, 9, 11, 1, 1, 2, 0)]
POINTWISE = [(3, 7, 5, 1, 1, 1, 0), (5, 9, 13, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 0), (1, 3, 43, 1, 1, 1, 0)]
GEOMETRIES = GENERAL + STRIDED + POINTWISE
RAGGED_GEN, RAGGED_STR, RAGGED_PW = GENERAL[1], STRIDED[0], POINTWISE[1]
FWD_EPILOGUES = (0, BIAS, ADDEND, RELU, BIAS | ADDEND | RELU, STATS, STATS | BIAS)
K_CYCLE = (32, 96, 128)                             # GEMM-K per group
BIG_TILE = (0, 1, 3)                                # the BM = 128 tiles; tile 2 is the BM = 64 one
COLS = {0: 256, 1: 128, 3: 96}                      # GEMM columns per group for a group of cases led by this BM = 128 tile


def _case(kind, dgrad, geom, kg, ncol, groups, tile, epi=0, io=0):
    """kg: GEMM-K channels per group, ncol: GEMM columns per group (the forward: input / output channels; the input gradient:
    output / input channels of the layer)"""
    cin, cout = (ncol * groups, kg * groups) if dgrad else (kg * groups, ncol * groups)
    B, H, W, kh, kw, stride, pad = geom
    return Case(kind, dgrad, B, H, W, cin, cout, kh, kw, stride, pad, groups, tile, epi, io)


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    for kind in ("fp32", "bf16"):
        # every geometry on tile 2 (BM = 64) and on a BM = 128 tile; the bf16 entry: the A operand's storage alternates
        for gi, geom in enumerate(GEOMETRIES):
            for dgrad in (False, True):
                if kind == "bf16" and dgrad and geom[5] != 1:
                    continue                                       # (refused: test_bf16_entry_refuses_the_strided_input_gradient)
                big = BIG_TILE[gi % 3]
                io = 0 if kind == "fp32" or not gi & 1 else (DY if dgrad else X)
                for tile in ((big,) if big == 3 else (big, 2)):
                    add(kind, dgrad, geom, K_CYCLE[gi % 3], COLS[big], 1, tile, io=io)
                if big == 3:
                    add(kind, dgrad, geom, K_CYCLE[gi % 3], 128, 1, 2, io=io)
        # every tile on the ragged geometries of each addressing mode (fp32: every instance of igemm_kernel)
        for geom, kg in ((RAGGED_PW, 32), (RAGGED_GEN, 32), (RAGGED_STR, 32), (RAGGED_PW, 96), (RAGGED_PW, 128)):
            for dgrad in (False, True):
                if kind == "bf16" and dgrad and geom[5] != 1:
                    continue
                for tile in range(4):
                    add(kind, dgrad, geom, kg, 256, 1, tile)
                add(kind, dgrad, geom, kg, 96, 1, 3)
        # forward epilogues on every tile
        for geom, kg in ((RAGGED_GEN, 64), (RAGGED_PW, 32)):
            for epi in FWD_EPILOGUES:
                for tile in range(4):
                    add(kind, False, geom, kg, 256, 1, tile, epi=epi)
        # the input gradient's addend
        for geom in (RAGGED_GEN, RAGGED_PW, RAGGED_STR):
            if kind == "bf16" and geom[5] != 1:
                continue
            for tile in range(4):
                add(kind, True, geom, 64, 256, 1, tile, epi=ADDEND)
        # groups: 2 x (32 -> 64) on tile 2 (one column tile per group) and tile 3 (two); 3 x (64 -> 128) on tiles 0 (one) and 2 (two);
        # 3 x (32 -> 32) on tile 3
        for geom in (RAGGED_GEN, RAGGED_STR, RAGGED_PW):
            for dgrad in (False, True):
                if kind == "bf16" and dgrad and geom[5] != 1:
                    continue
                for groups, kg, ncol, tiles in ((2, 32, 64, (2, 3)), (3, 64, 128, (0, 2)), (3, 32, 32, (3,))):
                    for tile in tiles:
                        add(kind, dgrad, geom, kg, ncol, groups, tile)
    # bf16: every (tile, pass, KT, storage of the A operand) instance of igemm_bf16_kernel, on ragged M
    for dgrad in (False, True):
        for kg in (96, 128):
            for a16 in (0, 1):
                for tile in range(4):
                    add("bf16", dgrad, RAGGED_GEN if kg == 96 else RAGGED_PW, kg, 256, 1, tile, io=(DY if dgrad else X) * a16)
    # bf16 storage: the forward's output (Y, X|Y; 0 and X are above), the input gradient's addend (4; 0 and 8 are above)
    for tile in range(4):
        for io in (Y, X | Y):
            add("bf16", False, RAGGED_GEN, 96, 256, 1, tile, io=io)
        add("bf16", True, RAGGED_GEN, 96, 256, 1, tile, epi=ADDEND, io=ADD)
        add("bf16", True, RAGGED_PW, 128, 256, 1, tile, epi=ADDEND, io=ADD | DY)
    # the bf16 kernel's stage switch (input gradients up to ONE_STAGE_MAX K tiles run one LDS stage): 27, 32 and 36 K tiles
    for geom, kg in ((RAGGED_GEN, 192), (RAGGED_PW, 2048), (RAGGED_GEN, 256)):
        for tile in (1, 2):
            add("bf16", True, geom, kg, 128, 1, tile, io=DY if kg == 2048 else 0)
    return list(dict.fromkeys(out))                # (the sweeps overlap in a few cases: each once)


CASES = _cases()


def case_id(c, tile=True):
    s = "%s-%s-%dx%dx%d-%dto%dg%d-k%dx%ds%dp%d-e%d-io%d" % (c.kind, "dgrad" if c.dgrad else "fwd", c.B, c.H, c.W, c.cin, c.cout,
                                                          c.groups, c.kh, c.kw, c.stride, c.pad, c.epi, c.io)
    return s + "-t%d" % c.tile if tile else s


def shape_of(c):
    return (c.B, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.groups)


def out_map(c):
    """(Ho, Wo) of the layer"""
    return (c.H + 2 * c.pad - c.kh) // c.stride + 1, (c.W + 2 * c.pad - c.kw) // c.stride + 1


def gemm_of(c):
    """(M, GEMM-K per group, GEMM columns per group) of the case's launch"""
    Ho, Wo = out_map(c)
    if c.dgrad:
        return c.B * c.H * c.W, c.cout // c.groups, c.cin // c.groups
    return c.B * Ho * Wo, c.cin // c.groups, c.cout // c.groups


def legal_tiles(c):
    """tiles 0-3 that divide the case's GEMM columns per group (csrc/conv_common.h sc_igemm_tile_ok)"""
    n = gemm_of(c)[2]
    return tuple(t for t in range(4) if (t == 0 and n % 128 == 0) or (t in (1, 2) and n % 64 == 0) or t == 3)


def kernel_name(c):
    return "igemm_%s%s<%s>" % ("dgrad" if c.dgrad else "fwd", "_bf16" if c.kind == "bf16" else "", TILE_NAME[c.tile])


def query_of(c):
    """(name, arguments) of the *_tile_ok query that says naming c.tile runs its kernel"""
    name = ("dgrad" if c.dgrad else "fwd") + ("_bf16" if c.kind == "bf16" else "") + "_tile_ok"
    return name, (*shape_of(c), c.tile, c.epi) + ((c.io, 0) if c.kind == "bf16" else ())


def instance_of(c):
    """the template instance the case runs: fp32 (tile, DGRAD, addressing), bf16 (tile, DGRAD, KT, A stored as bf16)"""
    if c.kind == "fp32":
        pw = (c.kh, c.kw, c.stride, c.pad) == (1, 1, 1, 0)
        return (c.tile, c.dgrad, "pw" if pw else "strided" if c.dgrad and c.stride != 1 else "general")     # (launch_igemm)
    return (c.tile, c.dgrad, 64 if gemm_of(c)[1] % 64 == 0 else 32, bool(c.io & (DY if c.dgrad else X)))


def ragged(c):
    """more than one M tile, the last one partly filled"""
    M = gemm_of(c)[0]
    return M > TILE_BM[c.tile] and M % TILE_BM[c.tile] != 0


def bf16_k_tiles(c):
    M, kg, _ = gemm_of(c)
    return c.kh * c.kw * (kg // (64 if kg % 64 == 0 else 32))


# groups of cases that differ in the tile only: one reference, and the bit comparison across tiles
GROUPS = [list(g) for _, g in itertools.groupby(sorted(CASES, key=lambda c: c._replace(tile=0)), key=lambda c: c._replace(tile=0))]


def K():
    from scouter_amd import kernels
    return kernels


def _conv64(a, w, c, dgrad):
    """fp64 NHWC result of the layer's forward (a = x) or input gradient (a = dy), HWIO weights, on the CPU"""
    a, w = a.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1)             # NCHW, OIHW
    if dgrad:
        r = torch.nn.grad.conv2d_input((c.B, c.cin, c.H, c.W), w, a, c.stride, c.pad, 1, c.groups)
    else:
        r = F.conv2d(a, w, None, c.stride, c.pad, 1, c.groups)
    return r.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=3)
def _data(c):
    """c: a case with tile = epi = io = 0 -> operands on the device (fp32), the fp64 result of what the kernel multiplies and the
    sum of its squared terms: computed once per shape, shared by the epilogues, storages and tiles listed for it"""
    bf16 = c.kind == "bf16"
    gen = torch.Generator().manual_seed(zlib.crc32(repr(c).encode()))
    Ho, Wo = out_map(c)
    M, kg, ncol = gemm_of(c)
    a = torch.randn((c.B, Ho, Wo, c.cout) if c.dgrad else (c.B, c.H, c.W, c.cin), generator=gen)
    w = torch.randn(c.kh, c.kw, c.cin // c.groups, c.cout, generator=gen) / (kg * c.kh * c.kw) ** 0.5
    n = ncol * c.groups
    bias = torch.randn(n, generator=gen)
    addend = torch.randn((c.B, c.H, c.W, n) if c.dgrad else (c.B, Ho, Wo, n), generator=gen)
    a64, w64 = _opnd(a, bf16), _opnd(w, bf16)
    ref = _conv64(a64, w64, c, c.dgrad)
    sq = _conv64(a64 * a64, w64 * w64, c, c.dgrad)
    return dict(a=a.cuda(), w=w.cuda(), bias=bias.cuda(), addend=addend.cuda(), ref=ref, sq=sq)


def _expected(c, d):
    """-> fp64 reference and V of the case's epilogue and storage"""
    ref, sq = d["ref"], d["sq"]
    if c.epi & BIAS:
        b = d["bias"].double().cpu()
        ref, sq = ref + b, sq + b * b
    if c.epi & ADDEND:
        ad = d["addend"]
        ad = (ad.bfloat16() if c.dgrad and c.io & ADD else ad).double().cpu()
        ref, sq = ref + ad, sq + ad * ad
    if c.epi & RELU:
        ref = ref.clamp_min(0)
    return ref, sq.sqrt()


def _guarded(M, N, dtype):
    """a buffer of GUARD + M + GUARD rows of N elements, every bit pattern a NaN -> (buffer as integers, the M rows in the middle)"""
    ity, pat = (torch.int16, 0x7FC1) if dtype == torch.bfloat16 else (torch.int32, 0x7FC0DEAD)
    buf = torch.full(((2 * GUARD + M) * N,), pat, dtype=ity, device="cuda")
    return buf, buf[GUARD * N:(GUARD + M) * N].view(dtype)


def _launch(kk, c, d, wt):
    """one launch of the case -> (rc, profiled kernel names, y [M][N], its guarded buffer as integers, bn_partial or None)"""
    from scouter_amd import _native
    L, p, st = _native.lib(), kk._p, kk._stream()
    M, kg, ncol = gemm_of(c)
    N = ncol * c.groups
    bf16 = c.kind == "bf16"
    a_bit = (DY if c.dgrad else X) if bf16 else 0
    a = d["a"].bfloat16() if c.io & a_bit else d["a"]
    out16 = bf16 and not c.dgrad and c.io & Y
    buf, y = _guarded(M, N, torch.bfloat16 if out16 else torch.float32)
    addend = d["addend"] if c.epi & ADDEND else None
    if addend is not None and c.dgrad and c.io & ADD:
        addend = addend.bfloat16()
    bias = d["bias"] if c.epi & BIAS else None
    part = None
    if c.epi & STATS:
        rows = kk.ask("fwd_bn_partial_rows_bf16" if bf16 else "fwd_bn_partial_rows", *shape_of(c), c.tile)
        assert rows == -(-M // TILE_BM[c.tile]), (case_id(c), rows)
        part = torch.full((rows + 1, N, 2), float("nan"), dtype=torch.float64, device="cuda")
        part[rows] = -777.25
    s = shape_of(c)
    if not c.dgrad and not bf16:
        fn = lambda: L.scouter_conv2d_fwd_f32(p(a), p(d["w"]), p(bias), p(addend), p(y), p(part), *s, int(bool(c.epi & RELU)), c.tile, st)
    elif not c.dgrad:
        fn = lambda: L.scouter_conv2d_fwd_bf16_io(p(a), p(wt), p(bias), p(addend), p(y), p(part), *s, int(bool(c.epi & RELU)), c.tile,
                                                  c.io, st)
    elif not bf16:
        fn = lambda: L.scouter_conv2d_dgrad_f32(p(a), p(d["w"]), p(addend), p(y), *s, c.tile, st)
    else:
        fn = lambda: L.scouter_conv2d_dgrad_bnbwd_bf16_io(p(a), p(d["w"]), p(addend), p(y), *s, c.tile, None, None, None, None, None,
                                                          None, None, c.io, st)
    with kk.switches(bhalo=0):
        rc, names = _profiled(fn)
    return rc, names, y.view(M, N), buf, part


def _run_checked(kk, c, d, wt, full=True):
    """launches the case twice: kernel name, guard rows, repeatability; full: every element against fp64, the statistics rows.
    -> the output's bits"""
    from scouter_amd import _native
    name = case_id(c)
    M, kg, ncol = gemm_of(c)
    N = ncol * c.groups
    outs = []
    for _ in range(2):
        rc, names, y, buf, part = _launch(kk, c, d, wt)
        _native.check(rc, name)                                   # (a generated case the library refuses is a failure)
        assert names == [kernel_name(c)], (name, names)
        pat = buf[0].clone()
        assert bool((buf[:GUARD * N] == pat).all()) and bool((buf[(GUARD + M) * N:] == pat).all()), "%s: guard rows written" % name
        outs.append((y, buf, part))
    (y, buf, part), (_, buf2, part2) = outs
    assert torch.equal(buf, buf2), "%s: two launches differ" % name
    if not full:
        return buf
    got = y.double().cpu().view(d["ref"].shape)
    assert bool(torch.isfinite(got).all()), "%s: %d elements not written or not finite" % (name, int((~torch.isfinite(got)).sum()))
    ref, mag = _expected(c, d)
    k = _k_for(kg * c.kh * c.kw)
    if y.dtype == torch.bfloat16:
        mag = mag + ref.abs() * 2.0 ** -8 / k
    print("%s: worst |err| / bound = %.3g" % (name, float(((got - ref).abs() / (k * mag + 1e-12)).max())))
    _check(name, got, ref, mag, k)
    if part is not None:
        rows = part.shape[0] - 1
        assert bool((part[rows] == -777.25).all()), "%s: the sentinel row of bn_partial was written" % name
        assert bool(torch.isfinite(part[:rows]).all()), "%s: statistics rows not written" % name
        assert torch.equal(part, part2), "%s: statistics of two launches differ" % name
        sums = part[:rows].sum(0).cpu()
        y64 = y.double().cpu()
        for j, want in enumerate((y64.sum(0), (y64 * y64).sum(0))):
            err = (sums[:, j] - want).abs()
            assert bool((err <= 1e-8 + 1e-10 * want.abs()).all()), "%s: statistics column %d off by %.3g" % (name, j, float(err.max()))
        # the same launch without statistics: the same y
        plain = _launch(kk, c._replace(epi=c.epi & ~STATS), d, wt)
        assert plain[0] == 0 and torch.equal(plain[3], buf), "%s: y differs from the launch without statistics" % name
    return buf


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: case_id(g[0], tile=False) + "-t" + ".".join(str(c.tile) for c in g))
def test_named_tiles_against_fp64_and_against_each_other(group):
    kk = K()
    c0 = group[0]
    d = _data(c0._replace(tile=0, epi=0, io=0))
    wt = kk.weight_bf16t(d["w"], c0.groups) if c0.kind == "bf16" and not c0.dgrad else None
    bits = {c.tile: _run_checked(kk, c, d, wt) for c in group}
    # every other legal tile of the shape: its name, its guard rows, repeatability -- and its bits
    for t in legal_tiles(c0):
        if t not in bits:
            bits[t] = _run_checked(kk, c0._replace(tile=t), d, wt, full=False)
    first = bits[min(bits)]
    same = {t: torch.equal(b, first) for t, b in bits.items()}
    print("%s: tiles %s give %s" % (case_id(c0, tile=False), sorted(bits), "the same bits" if all(same.values()) else "different bits: %s" % same))
    if not c0.dgrad:
        assert all(same.values()), "%s: forward tiles differ in their bits: %s" % (case_id(c0, tile=False), same)


def _refusal(fn):
    """-> (rc, error text, profiled kernel names) of a raw call"""
    from scouter_amd import _native
    rc, names = _profiled(fn)
    msg = _native.lib().scouter_last_error()
    return rc, msg.decode() if msg else "", names


def test_bf16_entry_refuses_the_strided_input_gradient():
    """scouter_conv2d_dgrad_bnbwd_bf16_io has no strided instantiation: rc -3 (SC_ERR_UNSUPPORTED) before any launch, for every tile"""
    kk = K()
    for geom in STRIDED:
        c = _case("bf16", True, geom, 64, 128, 1, 0)
        Ho, Wo = out_map(c)
        dy = torch.zeros(c.B, Ho, Wo, c.cout, device="cuda")
        w = torch.zeros(c.kh, c.kw, c.cin, c.cout, device="cuda")
        dx = torch.zeros(c.B, c.H, c.W, c.cin, device="cuda")
        assert kk.ask("dgrad_bf16_tile_ok", *shape_of(c), 1, 0, 0, 0) == 0
        for tile in range(4):
            rc, msg, names = _refusal(lambda: _launch_dgrad_bf16(kk, dy, w, dx, c, tile))
            assert rc == -3 and names == [] and "strided" in msg, (geom, tile, rc, msg, names)
        assert not bool(dx.any())


def _launch_dgrad_bf16(kk, dy, w, dx, c, tile):
    from scouter_amd import _native
    p = kk._p
    return _native.lib().scouter_conv2d_dgrad_bnbwd_bf16_io(p(dy), p(w), None, p(dx), *shape_of(c), tile, None, None, None, None, None,
                                                            None, None, 0, kk._stream())


@pytest.mark.parametrize("kind,dgrad", [("fp32", False), ("fp32", True), ("bf16", False), ("bf16", True)],
                         ids=["fwd_f32", "dgrad_f32", "fwd_bf16", "dgrad_bf16"])
def test_a_filter_of_more_than_32_taps_is_refused(kind, dgrad):
    """A 7x7, 32 -> 32 layer on an 8 x 8 map: the tap mask of a row holds 32 bits, so every entry point answers rc -3 with nothing
    launched (and the output untouched); the 5x5 layer next to it runs."""
    from scouter_amd import _native
    kk = K()
    L, p, st = _native.lib(), kk._p, kk._stream()
    for k, ok in ((5, True), (6, False), (7, False)):
        pad = k // 2
        c = Case(kind, dgrad, 2, 8, 8, 32, 32, k, k, 1, pad, 1, 3, 0, 0)
        Ho, Wo = out_map(c)
        a = torch.randn((2, Ho, Wo, 32) if dgrad else (2, 8, 8, 32), device="cuda", generator=_gen(k))
        w = torch.randn(k, k, 32, 32, device="cuda", generator=_gen(k + 1)) / (32 * k * k) ** 0.5
        wt = kk.weight_bf16t(w) if kind == "bf16" and not dgrad else None
        M = gemm_of(c)[0]
        buf, y = _guarded(M, 32, torch.float32)
        s = shape_of(c)
        fn = {("fp32", False): lambda: L.scouter_conv2d_fwd_f32(p(a), p(w), None, None, p(y), None, *s, 0, 3, st),
              ("fp32", True): lambda: L.scouter_conv2d_dgrad_f32(p(a), p(w), None, p(y), *s, 3, st),
              ("bf16", False): lambda: L.scouter_conv2d_fwd_bf16_io(p(a), p(wt), None, None, p(y), None, *s, 0, 3, 0, st),
              ("bf16", True): lambda: L.scouter_conv2d_dgrad_bnbwd_bf16_io(p(a), p(w), None, p(y), *s, 3, None, None, None, None, None,
                                                                           None, None, 0, st)}[(kind, dgrad)]
        assert kk.ask(*_flat(query_of(c))) == int(ok), (k, query_of(c))
        rc, msg, names = _refusal(fn)
        if ok:
            assert rc == 0 and names == [kernel_name(c)], (k, rc, msg, names)
            assert bool(torch.isfinite(y).all())
        else:
            assert rc == -3 and names == [] and "32 taps" in msg, (k, rc, msg, names)
            assert bool((buf == buf[0]).all()), "a refused call wrote its output"


def _flat(q):
    return (q[0],) + tuple(q[1])


WALK_MAX, WALK_ROWS = 1 << 22, 256                  # csrc/conv_common.h SC_WALK_MAX, SC_WALK_ROWS
LARGE_W = 255
LARGE_H = (WALK_MAX - WALK_ROWS) // LARGE_W         # 16 447 rows: 4 193 985 pixels


def test_forward_at_the_largest_map_the_pixel_walk_admits_and_the_refusal_one_row_later():
    """3x3 / pad 1, 32 -> 32, one image of 16 447 x 255 pixels: the largest map at this width with Ho * Wo + 256 <= 2^22, the domain
    on which the kernels' fp32 pixel unflattening (fast_div) is exact; igemm_fwd<128x32> there against sampled fp64, the sample
    forced onto the first pixel of each of the last 64 128-row blocks (block starts are what the prologue unflattens) and onto the
    last pixels.  One map row more (4 194 240 pixels) is refused with rc -3 and nothing launched -- before the fix that shape ran,
    and from 4 275 584 pixels on block starts got the tap mask of a neighbouring column.  Peak 1.2 GB measured (x and y of 537 MB
    each, the refused call's buffers are the same ones)."""
    from scouter_amd import _native
    kk = K()
    L, p, st = _native.lib(), kk._p, kk._stream()
    H, W = LARGE_H + 1, LARGE_W
    assert LARGE_H * W + WALK_ROWS <= WALK_MAX < H * W + WALK_ROWS
    gen = _gen(H)
    x = torch.randn(1, H, W, 32, device="cuda", generator=gen)                  # (sized for the refused shape: one row more)
    w = torch.randn(3, 3, 32, 32, device="cuda", generator=gen) / 288 ** 0.5
    y = torch.full((1, H, W, 32), float("nan"), device="cuda")
    assert kk.ask("fwd_tile_ok", 1, H, W, 32, 32, 3, 3, 1, 1, 1, 3, 0) == 0
    rc, msg, names = _refusal(lambda: L.scouter_conv2d_fwd_f32(p(x), p(w), None, None, p(y), None, 1, H, W, 32, 32, 3, 3, 1, 1, 1, 0, 3, st))
    assert rc == -3 and names == [] and "2^22" in msg, (rc, msg, names)
    assert bool(torch.isnan(y[0, -1]).all())
    H = LARGE_H
    ybuf = y
    x, y = x[:, :H], y[:, :H]
    assert kk.ask("fwd_tile_ok", 1, H, W, 32, 32, 3, 3, 1, 1, 1, 3, 0) == 1
    rc, msg, names = _refusal(lambda: L.scouter_conv2d_fwd_f32(p(x), p(w), None, None, p(y), None, 1, H, W, 32, 32, 3, 3, 1, 1, 1, 0, 3, st))
    assert rc == 0 and names == ["igemm_fwd<128x32>"], (rc, msg, names)
    b, yy, xx, cc, nt = _pick(2048, 1, H, W, 32, gen)
    starts = (torch.arange(64, device="cuda") + (H * W // 128 - 63)) * 128      # the first pixel of the last 64 blocks
    yy[:64], xx[:64] = starts // W, starts % W
    idx = (b, yy, xx, cc, nt)
    ref, mag = _sample_fwd(x, w, idx)
    got = y[b, yy, xx, cc]
    _check("forward at %d x %d" % (H, W), got, ref, mag, _k_for(288))
    _no_lost_tail(got[-nt:], ref[-nt:], "tail")
    _no_lost_tail(got[:64], ref[:64], "block starts")
    assert bool(torch.isnan(ybuf[0, -1]).all()), "the map row behind the output was written"
    del x, y, ybuf, w
    _free()
