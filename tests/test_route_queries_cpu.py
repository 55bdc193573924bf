"""The route queries of include/scouter_hip.h (scouter_conv2d_*_tile_ok / *_ok), asked on the CPU: integers only.

Every fast convolution kernel's acceptance rule -- a shape condition plus 31 / 32-bit byte guards -- is ONE host predicate in
csrc/, which its entry point rejects through and its query answers with; scouter_amd.kernels routes on the queries.  Here:
  * every convolution row of the THRESHOLDS table of tests/test_size_thresholds_gpu.py flips its query exactly between the
    listed "below" and "above" shapes (those tests launch the kernels there; this one needs no device);
  * the shape edges of the rules: map width and height, GEMM-K, column multiples, each epilogue / storage bit a rule reads;
  * every non-weight-gradient entry of the committed tuning table names a tile its query accepts for that key's shape."""
import json

import pytest


@pytest.fixture(scope="module")
def kk():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


BIAS, ADDEND, RELU, STATS, BWD, BWD2 = 1, 2, 4, 8, 16, 32
X, Y = 1, 2                                    # SCOUTER_IO_X_BF16 / _Y_BF16
X1, X2, ADD, DY, DX = 1, 2, 4, 8, 16           # SCOUTER_DGRAD_IO_*
PW = (1, 1, 1, 0, 1)                           # kh, kw, stride, pad, groups of a pointwise layer
C3 = (3, 3, 1, 1, 1)                           # ... of a same-size 3x3 layer


def test_queries_answer_one_or_zero_and_refuse_bad_arguments(kk):
    q = kk.ask
    assert q("fwd_tile_ok", 2, 8, 8, 64, 128, *PW, 4, 0) == 1 and q("fwd_tile_ok", 2, 8, 8, 96, 128, *PW, 4, 0) == 0
    for bad in ((0, 8, 8, 64, 128, 1, 1, 1, 0, 1), (2, 8, 8, 64, 128, 1, 1, 0, 0, 1), (2, 8, 8, 64, 128, 1, 1, 1, 0, 0),
                (2, 8, 8, 64, 128, 1, 1, 1, 0, 3), (2, 2, 2, 64, 128, 5, 5, 1, 0, 1), (2, 8, 8, 64, 128, 1, 1, 1, -1, 1)):
        for name, tail in (("fwd_tile_ok", (3, 0)), ("dgrad_tile_ok", (3, 0)), ("fwd_bf16_tile_ok", (3, 0, 0, 0)),
                           ("dgrad_bf16_tile_ok", (3, 0, 0, 0)), ("fwd_x3_tile_ok", (-1, 0)), ("dgrad_x3_tile_ok", (-1, 0)),
                           ("fwd_planes_tile_ok", (3, 1, 0, 0)), ("dgrad_planes_tile_ok", (3, 1, 0)), ("wgrad_kernel_ok", (0,))):
            assert q(name, *bad, *tail) == 0, (name, bad)
    # sizes no tensor has answer 0 (before any product of a rule can overflow)
    big = 2 ** 31 - 1
    for huge in ((big, big, big, 64, 128, 1, 1, 1, 0, 1), (2, 8, 8, big - 31, big - 31, 1, 1, 1, 0, 1), (2, 8, 8, 1 << 20, 1 << 20, 1, 1, 1, 0, 1),
                 (2, 8, 8, 64, 128, 3, 3, 1, big // 2, 1), (1 << 20, 1 << 10, 1 << 10, 64, 128, 1, 1, 1, 0, 1)):
        for name, tail in (("fwd_tile_ok", (3, 0)), ("dgrad_tile_ok", (3, 0)), ("fwd_x3_tile_ok", (-1, 0)), ("fwd_planes_tile_ok", (3, 1, 0, 0)),
                           ("wgrad_kernel_ok", (0,))):
            assert q(name, *huge, *tail) == 0, (name, huge)
    assert not kk.x3_halo_fits(2 ** 31 + 64, 32, 32) and not kk.x3_halo_fits(2 ** 32 + 64, 32, 32)       # (no wrap to a small count)
    # the memo: one library call per argument tuple
    n = len(kk._asked)
    q("fwd_tile_ok", 2, 8, 8, 64, 128, *PW, 4, 0)
    assert len(kk._asked) == n


# ---- the THRESHOLDS rows (tests/test_size_thresholds_gpu.py): (query, arguments with the batch left out, below, above)
def _threshold_rows(kk):
    return [
        # persistent pointwise tile 4: 4*M*max(K, N) < 2^31; 64 <-> 256 channels at 56 x 56
        ("fwd_tile_ok", (56, 56, 64, 256, *PW, 4, 0), 668, 669),
        ("fwd_tile_ok", (56, 56, 256, 64, *PW, 4, STATS), 668, 669),
        ("dgrad_tile_ok", (56, 56, 64, 256, *PW, 4, 0), 668, 669),
        ("dgrad_tile_ok", (56, 56, 256, 64, *PW, 4, ADDEND | BWD), 668, 669),
        # tile 7 of the register-split family: 4*M*max(Cin, Cout) < 2^31 on 64 x 64 maps
        ("fwd_x3_tile_ok", (64, 64, 32, 32, *C3, 7, 0), 4095, 4096),
        ("dgrad_x3_tile_ok", (64, 64, 32, 32, *C3, 7, 0), 4095, 4096),
        ("dgrad_x3_tile_ok", (64, 64, 32, 64, *C3, 7, BWD), 2047, 2048),
        # bf16 resident-rows input gradient behind tile 3, dy stored as bf16: (M + 512)*Cout*2 < 2^31
        ("dgrad_bf16_tile_ok", (64, 64, 32, 64, *C3, 3, 0, DY, 1), 4095, 4096),
        # tap-fused plane weight gradient (plan bit 6): 2*M*max(Cin, Cout) < 2^31; one plane, 128 -> 256 in two groups
        ("wgrad_planes_plan_ok", (56, 56, 128, 256, 3, 3, 1, 2, 1, 64), 1337, 1338),
        ("wgrad_planes_plan_ok", (56, 56, 128, 256, 3, 3, 1, 2, 1, 67), 1337, 1338),
        # plane forward / input gradient: nplanes*B*H*W*C*2 < 2^31 + H*W*C*2; one plane, 64 channels, 32 x 32
        ("fwd_planes_tile_ok", (32, 32, 64, 64, *C3, 1, 1, 0, 0), 16384, 16385),
        ("fwd_planes_tile_ok", (32, 32, 64, 64, *C3, 1, 6, STATS, 0), 16384, 16385),
        ("dgrad_planes_tile_ok", (32, 32, 64, 64, *C3, 1, 1, 0), 16384, 16385),
    ]


def test_every_threshold_row_flips_between_its_two_shapes(kk):
    for name, args, below, above in _threshold_rows(kk):
        assert kk.ask(name, below, *args) == 1, (name, below, args)
        assert kk.ask(name, above, *args) == 0, (name, above, args)
        assert kk.ask(name, 2, *args) == 1, (name, args)
    # the per-tap plans of the plane weight gradient stay legal past the tap-fused plans' guard
    assert kk.ask("wgrad_planes_plan_ok", 1338, 56, 56, 128, 256, 3, 3, 1, 2, 1, 3) == 1
    # (a named tile of the wrappers goes with its query: kernels.x3_halo_fits / _pw_persist_legal are one-line calls of them)
    assert kk.x3_halo_fits(4095 * 64 * 64, 32, 32) and not kk.x3_halo_fits(4096 * 64 * 64, 32, 32)
    assert kk._pw_persist_legal(668 * 56 * 56, 64, 256, 1, 1, 1, 0, 1, True)
    assert not kk._pw_persist_legal(669 * 56 * 56, 64, 256, 1, 1, 1, 0, 1, True)


def test_the_two_policy_margins_sit_below_the_library_guards(kk):
    """fp32-stored operands are rounded for the resident-rows input gradient / the tap-fused bf16 weight gradient only below
    2^31 - 2^20 bytes (kernels.PREROUND_MAX_BYTES: policy); the kernels themselves take two more images."""
    shape = (64, 64, 32, 64, *C3)
    for helper, query in ((kk.dgrad_prerounds, ("dgrad_bf16_tile_ok", (3, 0, DY, 1))),
                          (kk.wgrad_prerounds, ("wgrad_kernel_ok", (kk.WGRAD_BWT,)))):
        assert helper(4093, *shape) and not helper(4094, *shape)
        assert kk.ask(query[0], 4094, *shape, *query[1]) == 1 and kk.ask(query[0], 4095, *shape, *query[1]) == 1
        assert kk.ask(query[0], 4096, *shape, *query[1]) == 0
        assert not helper(2, 64, 64, 64, 64, *C3)              # (64 input channels per group: not the kernels' shape)
    assert kk.PREROUND_MAX_BYTES == 2 ** 31 - 2 ** 20


def test_map_width_and_height_edges(kk):
    q = kk.ask
    for W, ok in ((63, 1), (64, 0)):                        # plane halo tile 5 and the tap-fused plane weight gradient
        assert q("fwd_planes_tile_ok", 2, 16, W, 64, 64, *C3, 3, 5, 0, 0) == ok
        assert q("dgrad_planes_tile_ok", 2, 16, W, 64, 64, *C3, 1, 5, 0) == ok
        assert q("wgrad_planes_plan_ok", 2, 16, W, 64, 64, 3, 3, 1, 1, 3, 64) == ok
        assert q("wgrad_planes_plan_ok", 2, 16, W, 64, 64, 3, 3, 1, 1, 3, 1) == 1
        assert kk._halo_ok(3, 3, 1, 1, 16, W, 1) == bool(ok and kk.HALO_TILE & 1)
    for W, ok in ((112, 1), (113, 0)):                      # bf16 resident rows (both passes), xwt, bwt
        assert q("fwd_bf16_tile_ok", 2, 16, W, 32, 64, *C3, 1, 0, X, 1) == ok
        assert q("fwd_bf16_tile_ok", 2, 16, W, 32, 32, *C3, 3, 0, X, 1) == ok
        assert q("dgrad_bf16_tile_ok", 2, 16, W, 32, 64, *C3, 3, 0, DY, 1) == ok
        assert q("wgrad_kernel_ok", 2, 16, W, 32, 64, *C3, kk.WGRAD_XWT) == ok
        assert q("wgrad_kernel_ok", 2, 16, W, 32, 64, *C3, kk.WGRAD_BWT) == ok
        assert q("wgrad_kernel_ok", 2, 16, W, 32, 64, *C3, kk.WGRAD_TAPS) == 1       # (the fp32 tap-fused kernel: any width)
    # the layers whose weight-gradient plan the wrappers leave to the library under switch xwt: the shape XWT and BWT share, on
    # maps too small for the tap-fused kernels (32 / W + 1 >= H) too -- as before the queries existed
    for H, W, rows32, xwt in ((16, 16, 1, 1), (4, 4, 1, 0), (2, 32, 1, 0), (16, 113, 0, 0), (1, 16, 0, 0)):
        assert q("wgrad_kernel_ok", 2, H, W, 32, 64, *C3, kk.WGRAD_ROWS32) == rows32, (H, W)
        assert q("wgrad_kernel_ok", 2, H, W, 32, 64, *C3, kk.WGRAD_XWT) == xwt, (H, W)
    assert q("wgrad_kernel_ok", 2, 16, 16, 64, 64, *C3, kk.WGRAD_ROWS32) == 0 and q("wgrad_kernel_ok", 2, 16, 16, 32, 64, *PW, kk.WGRAD_ROWS32) == 0
    for W, ok in ((126, 1), (127, 0)):                      # tile 7
        assert q("fwd_x3_tile_ok", 2, 16, W, 32, 32, *C3, 7, 0) == ok
        assert q("dgrad_x3_tile_ok", 2, 16, W, 32, 64, *C3, 7, 0) == ok
        assert kk.x3_halo_ok(True, 2, 16, W, 32, 64) == bool(ok)
    for H, ok in ((2, 1), (1, 0)):                          # bf16 resident rows need two map rows
        assert q("fwd_bf16_tile_ok", 64, H, 64, 32, 64, *C3, 1, 0, X, 1) == ok
        assert q("dgrad_bf16_tile_ok", 64, H, 64, 32, 64, *C3, 3, 0, DY, 1) == ok
    # the resident-rows kernels run behind ONE tile: 1 for 64 columns per group, 3 for 32; two fused BatchNorms: the tile kernel
    assert q("fwd_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 3, 0, X, 1) == 0 and q("fwd_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 3, 0, X, 0) == 1
    assert q("fwd_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 1, 0, 0, 1) == 0          # (x stored as fp32)
    assert q("dgrad_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 3, BWD, DY, 1) == 1
    assert q("dgrad_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 3, BWD | BWD2, DY, 1) == 0
    assert q("dgrad_bf16_tile_ok", 2, 16, 16, 32, 64, *C3, 3, 0, 0, 1) == 0        # (dy stored as fp32)
    assert q("dgrad_bf16_tile_ok", 2, 16, 16, 64, 64, *C3, 3, 0, DY, 1) == 0       # (64 input channels per group)


def test_gemm_k_and_column_multiples(kk):
    q = kk.ask
    ALL_IO = DY | DX | X1
    for k in (64, 96, 128, 256, 512, 1024):
        assert q("fwd_tile_ok", 2, 8, 8, k, 128, *PW, 4, 0) == (k in (64, 128, 256))                # pwp
        assert q("dgrad_tile_ok", 2, 8, 8, 128, k, *PW, 4, 0) == (k in (64, 128, 256))
        assert q("fwd_tile_ok", 2, 8, 8, k, 128, *PW, 5, 0) == (k in (64, 128, 256))                # xpw
        assert q("dgrad_tile_ok", 2, 8, 8, 128, k, *PW, 5, BWD) == (k in (64, 128, 256))
        assert kk.xpw_fwd_eligible(k, 128, 1, 1, 1, 0, 1, False) == (k in (64, 128, 256))
        assert q("fwd_bf16_tile_ok", 2, 8, 8, k, 128, *PW, 4, 0, X, 0) == (k in (64, 128, 256, 512))  # pwb forward
        assert q("dgrad_bf16_tile_ok", 2, 8, 8, 128, k, *PW, 4, BWD, ALL_IO, 0) == (k in (64, 128, 256, 512))
        assert q("dgrad_bf16_tile_ok", 2, 8, 8, 128, k, *PW, 4, 0, DY, 0) == (k != 96)             # plain pwb: up to 1024
    for n, tiles in ((32, (3,)), (64, (1, 2, 3)), (128, (0, 1, 2, 3))):
        for t in range(4):
            ok = int(t in tiles)
            assert q("fwd_tile_ok", 2, 8, 8, 64, n, *PW, t, 0) == ok and q("dgrad_tile_ok", 2, 8, 8, n, 64, *PW, t, 0) == ok
            assert q("fwd_bf16_tile_ok", 2, 8, 8, 64, n, *PW, t, 0, 0, 0) == ok
            assert q("dgrad_bf16_tile_ok", 2, 8, 8, n, 64, *PW, t, 0, 0, 0) == ok
            assert kk._tile_legal(n, t) == bool(ok)
        assert q("fwd_tile_ok", 2, 8, 8, 64, n, *PW, 4, 0) == (n % 64 == 0)
        assert q("fwd_tile_ok", 2, 8, 8, 64, n, *PW, 5, 0) == (n % 64 == 0)
        assert q("fwd_bf16_tile_ok", 2, 8, 8, 64, n, *PW, 4, 0, X, 0) == (n % 128 == 0)
        assert q("dgrad_bf16_tile_ok", 2, 8, 8, n, 64, *PW, 4, BWD, ALL_IO, 0) == (n % 128 == 0)
        assert q("dgrad_bf16_tile_ok", 2, 8, 8, n, 64, *PW, 4, 0, DY, 0) == (n % 64 == 0)
        x3 = {32: (5, 6), 64: (2, 3, 4, 5, 6), 128: (0, 1, 2, 3, 4, 5, 6)}[n]
        for t in range(8):
            assert q("fwd_x3_tile_ok", 2, 8, 8, 64, n, *C3, t, 0) == int(t in x3 or (t == 7 and n == 32)), (n, t)
            assert q("dgrad_x3_tile_ok", 2, 8, 8, n, 64, *C3, t, 0) == int(t in x3 or (t == 7 and n == 32)), (n, t)
            assert kk._x3_tile_ok(t, n) == (t in x3 or (t == 7 and n == 32))
        assert q("fwd_x3_tile_ok", 2, 8, 8, 64, n, *C3, -1, 0) == 1
        p3 = {32: (), 64: (1, 2, 3, 5, 6), 128: (0, 1, 2, 3, 4, 5, 6)}[n]
        p1 = {32: (), 64: (1, 5, 6), 128: (0, 1, 5, 6)}[n]
        for t in range(8):
            assert q("fwd_planes_tile_ok", 2, 8, 8, 64, n, *C3, 3, t, 0, 0) == int(t in p3), (n, t)
            assert q("fwd_planes_tile_ok", 2, 8, 8, 64, n, *C3, 1, t, 0, 0) == int(t in p1), (n, t)
            assert q("dgrad_planes_tile_ok", 2, 8, 8, n, 64, *C3, 3, t, 0) == int(t in p3), (n, t)
    assert kk._plane_tiles(128) == (0, 2, 3, 4, 6) and kk._plane_tiles(64, 3, True) == (2, 3, 5, 6)
    assert kk._plane_tiles(128, 1) == (0, 1, 6) and kk._plane_tiles(64, 1, True) == (1, 5, 6)
    # the register-split entry points: 32-multiples per group, two K-tiles, odd same-size filters up to 5 x 5, stride 1
    assert q("fwd_x3_tile_ok", 2, 8, 8, 32, 64, *PW, -1, 0) == 0 and q("fwd_x3_tile_ok", 2, 8, 8, 64, 64, *PW, -1, 0) == 1
    assert q("fwd_x3_tile_ok", 2, 8, 8, 32, 64, 5, 5, 1, 2, 1, -1, 0) == 1 and q("fwd_x3_tile_ok", 2, 8, 8, 32, 64, 7, 7, 1, 3, 1, -1, 0) == 0
    assert q("fwd_x3_tile_ok", 2, 8, 8, 32, 64, 3, 3, 2, 1, 1, -1, 0) == 0 and q("fwd_x3_tile_ok", 2, 8, 8, 32, 64, 3, 3, 1, 0, 1, -1, 0) == 0
    assert kk.x3_fwd_abi_ok(32, 64, 3, 1, 1, 1) and not kk.x3_fwd_abi_ok(32, 64, 3, 2, 1, 1) and not kk.x3_fwd_abi_ok(48, 64, 3, 1, 1, 1)
    assert kk.x3_fwd_fits(70, 56, 56, 64, 256, 1, 1) and not kk.x3_fwd_fits(1, 2048, 2048, 64, 64, 1, 1)     # (H*W*Cin = 2^28)
    assert kk.x3_wgrad_ok(128, 256) and not kk.x3_wgrad_ok(64, 256) and not kk.x3_wgrad_ok(128, 192)
    assert q("wgrad_x3_ok", 1 << 15, 256, 256, 128, 128) == 0                                               # (2^31 pixels)
    # persistent kernels and the resident-rows kernels are pointwise / 3x3 stride-1 group rules
    for bad in ((3, 3, 1, 1, 1), (1, 1, 2, 0, 1), (1, 1, 1, 0, 2)):
        assert q("fwd_tile_ok", 2, 8, 8, 64, 128, *bad, 4, 0) == 0 and q("fwd_tile_ok", 2, 8, 8, 64, 128, *bad, 5, 0) == 0
        assert q("fwd_bf16_tile_ok", 2, 8, 8, 64, 128, *bad, 4, 0, X, 0) == 0
    # the plane weight gradient: same-size filters, 64-multiples per group
    assert q("wgrad_planes_plan_ok", 2, 8, 8, 64, 64, 3, 3, 1, 1, 3, -1) == 1 and q("wgrad_planes_plan_ok", 2, 8, 8, 32, 64, 3, 3, 1, 1, 3, -1) == 0
    assert q("wgrad_planes_plan_ok", 2, 8, 8, 64, 64, 3, 3, 0, 1, 3, -1) == 0 and q("wgrad_planes_plan_ok", 2, 8, 8, 64, 64, 1, 1, 0, 1, 3, 64) == 0
    # the weight-gradient kernels: 32-multiples per group; bf16: same-size stride-1 layers; tap-fused: 32 input channels per group
    assert q("wgrad_kernel_ok", 2, 8, 8, 32, 64, *C3, kk.WGRAD_F32) == 1 and q("wgrad_kernel_ok", 2, 8, 8, 48, 64, *C3, kk.WGRAD_F32) == 0
    assert q("wgrad_kernel_ok", 2, 16, 16, 64, 64, *C3, kk.WGRAD_BF16) == 1 and q("wgrad_kernel_ok", 2, 16, 16, 64, 64, 3, 3, 2, 1, 1, kk.WGRAD_BF16) == 0
    assert q("wgrad_kernel_ok", 2, 8, 8, 64, 64, *C3, kk.WGRAD_BF16) == 0 and q("wgrad_kernel_ok", 2, 8, 8, 64, 64, *PW, kk.WGRAD_BF16) == 1   # (64 / W + 1 < H)
    assert q("wgrad_kernel_ok", 2, 8, 8, 64, 64, *C3, kk.WGRAD_XWT) == 0 and q("wgrad_kernel_ok", 2, 8, 8, 64, 128, 3, 3, 1, 1, 2, kk.WGRAD_XWT) == 1


def test_each_epilogue_and_storage_bit_a_rule_reads(kk):
    q = kk.ask
    fwd = (2, 8, 8, 64, 128, *PW)
    for tile in (4, 5):                                     # fp32 persistent forward: BatchNorm statistics only
        assert q("fwd_tile_ok", *fwd, tile, STATS) == 1
        for bit in (BIAS, ADDEND, RELU):
            assert q("fwd_tile_ok", *fwd, tile, bit) == 0, (tile, bit)
    dg = (2, 8, 8, 128, 64, *PW)
    assert q("dgrad_tile_ok", *dg, 4, ADDEND) == 1 and q("dgrad_tile_ok", *dg, 4, ADDEND | BWD | BWD2) == 1
    assert q("dgrad_tile_ok", *dg, 5, 0) == 0 and q("dgrad_tile_ok", *dg, 5, ADDEND) == 0     # tile 5: the fused epilogue only
    assert q("dgrad_tile_ok", *dg, 5, BWD) == 1 and q("dgrad_tile_ok", *dg, 5, ADDEND | BWD | BWD2) == 1
    # typed forward tile 4: plain epilogue, x stored as bf16, y either way
    assert q("fwd_bf16_tile_ok", *fwd, 4, STATS, X, 0) == 1 and q("fwd_bf16_tile_ok", *fwd, 4, 0, X | Y, 0) == 1
    assert q("fwd_bf16_tile_ok", *fwd, 4, 0, 0, 0) == 0 and q("fwd_bf16_tile_ok", *fwd, 4, 0, Y, 0) == 0
    for bit in (BIAS, ADDEND, RELU):
        assert q("fwd_bf16_tile_ok", *fwd, 4, bit, X, 0) == 0
    # typed fused input gradient tile 4: every tensor the launch touches stored as bf16
    full = DY | DX | X1
    assert q("dgrad_bf16_tile_ok", *dg, 4, BWD, full, 0) == 1
    for missing in (DY, DX, X1):
        assert q("dgrad_bf16_tile_ok", *dg, 4, BWD, full & ~missing, 0) == 0, missing
    assert q("dgrad_bf16_tile_ok", *dg, 4, BWD | ADDEND, full, 0) == 0 and q("dgrad_bf16_tile_ok", *dg, 4, BWD | ADDEND, full | ADD, 0) == 1
    assert q("dgrad_bf16_tile_ok", *dg, 4, BWD | BWD2, full, 0) == 0 and q("dgrad_bf16_tile_ok", *dg, 4, BWD | BWD2, full | X2, 0) == 1
    # ... and the plain one: dy stored as bf16, dx as fp32, the addend either way
    assert q("dgrad_bf16_tile_ok", *dg, 4, 0, DY, 0) == 1 and q("dgrad_bf16_tile_ok", *dg, 4, ADDEND, DY | ADD, 0) == 1
    assert q("dgrad_bf16_tile_ok", *dg, 4, ADDEND, DY, 0) == 1
    assert q("dgrad_bf16_tile_ok", *dg, 4, 0, 0, 0) == 0 and q("dgrad_bf16_tile_ok", *dg, 4, 0, DY | DX, 0) == 0
    # tile 7 forward: no bias / addend
    x7 = (2, 8, 8, 32, 32, *C3)
    assert q("fwd_x3_tile_ok", *x7, 7, RELU | STATS) == 1 and q("fwd_x3_tile_ok", *x7, 7, BIAS) == 0 and q("fwd_x3_tile_ok", *x7, 7, ADDEND) == 0
    assert q("dgrad_x3_tile_ok", *x7, 7, ADDEND | BWD | BWD2) == 1
    # plane tile 6: fp32 output, statistics of the raw accumulators only, two K-tiles
    p6 = (2, 8, 8, 64, 64, *C3, 3, 6)
    assert q("fwd_planes_tile_ok", *p6, STATS, 0) == 1 and q("fwd_planes_tile_ok", *p6, BIAS | ADDEND | RELU, 0) == 1
    assert q("fwd_planes_tile_ok", *p6, STATS | BIAS, 0) == 0 and q("fwd_planes_tile_ok", *p6, STATS | ADDEND, 0) == 0
    assert q("fwd_planes_tile_ok", *p6, 0, Y) == 0 and q("fwd_planes_tile_ok", 2, 8, 8, 64, 64, *C3, 3, 4 - 2, 0, Y) == 1
    assert q("fwd_planes_tile_ok", 2, 8, 8, 32, 64, *PW, 3, 6, 0, 0) == 0 and q("fwd_planes_tile_ok", 2, 8, 8, 64, 64, *PW, 3, 6, 0, 0) == 1
    assert q("dgrad_planes_tile_ok", 2, 8, 8, 64, 32, *PW, 3, 6, 0) == 0 and q("dgrad_planes_tile_ok", 2, 8, 8, 64, 64, *PW, 3, 6, 0) == 1
    # partial rows of the plane tiles
    M = 70 * 56 * 56
    for t, rows in enumerate((128, 128, 128, 64, 256, 256)):
        assert q("planes_partial_rows", M, t) == -(-M // rows)
    assert q("planes_partial_rows", M, 6) == -(-M // 256) * 4 and q("planes_partial_rows", 1, 6) == 4


def test_every_tuning_table_entry_names_a_tile_its_query_accepts(kk):
    with open(kk.TUNE_TABLE_PATH) as f:
        choices = json.load(f)["choices"]
    seen = {}
    for key, tile in choices.items():
        p = key.split("|")
        kind, v = p[0], [int(s) for s in p[1:]]
        if kind in ("wgrad", "pwgrad", "xwgrad"):
            continue
        if kind in ("fwd", "dgrad"):
            bf16, shape = v[0], v[1:]
            ok = kk.ask(kind + ("_bf16_tile_ok" if bf16 else "_tile_ok"), *shape, tile, 0, *((0, 0) if bf16 else ()))
        elif kind == "dgrad+bn":
            n, addend, bf16, shape = v[0], v[1], v[2], v[3:]
            epi = BWD | (BWD2 if n > 1 else 0) | (ADDEND if addend else 0)
            io = DY | DX | X1 | (X2 if n > 1 else 0) | (ADD if addend else 0)         # (the typed tile 4: all tensors stored as bf16)
            ok = kk.ask("dgrad_bf16_tile_ok", *shape, tile, epi, io, 0) if bf16 else kk.ask("dgrad_tile_ok", *shape, tile, epi)
        elif kind in ("pfwd", "pdgrad"):
            ok = kk.ask("fwd_planes_tile_ok", *v[1:], v[0], tile, 0, 0) if kind == "pfwd" else kk.ask("dgrad_planes_tile_ok", *v[1:], v[0], tile, 0)
        elif kind == "pdgrad+bn":
            n, addend, nplanes, shape = v[0], v[1], v[2], v[3:]
            ok = kk.ask("dgrad_planes_tile_ok", *shape, nplanes, tile, BWD | (BWD2 if n > 1 else 0) | (ADDEND if addend else 0))
        else:
            assert kind in ("xfwd", "xdgrad", "xdgrad+bn"), key
            s = v[1:] if kind != "xdgrad+bn" else v[3:]
            kh, groups = (s[5], s[6]) if len(s) > 5 else (1, 1)
            shape = (*s[:5], kh, kh, 1, (kh - 1) // 2, groups)
            epi = 0 if kind != "xdgrad+bn" else BWD | (BWD2 if v[0] > 1 else 0) | (ADDEND if v[1] else 0)
            ok = kk.ask("fwd_x3_tile_ok" if kind == "xfwd" else "dgrad_x3_tile_ok", *shape, tile, epi)
        assert ok == 1, (key, tile)
        seen[kind] = seen.get(kind, 0) + 1
    assert sum(seen.values()) == 779 and set(seen) == {"fwd", "dgrad", "dgrad+bn", "xfwd", "xdgrad", "xdgrad+bn", "pfwd", "pdgrad",
                                                       "pdgrad+bn"}, seen
