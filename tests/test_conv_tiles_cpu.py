"""What tests/test_conv_tiles_gpu.py reaches, and the two limits of the block prologue every pixel-walking convolution kernel
shares, asked and proved on the CPU: integers and numpy float32 only, no device.

  * NAMED TILES: for every case of the GPU table the matching *_tile_ok query (include/scouter_hip.h) answers 1 for the named tile,
    epilogue and storage -- the GPU run cannot be a re-route -- and the table reaches every instance of igemm_kernel<.., DGRAD,
    STRIDED, PW> and igemm_bf16_kernel<.., KT, DGRAD, A_BF16> on a ragged M, every geometry on two tiles of different height,
    every epilogue and storage, and both sides of the bf16 kernel's stage switch: a later edit of the table cannot drop one quietly.
  * TAP MASK (csrc/conv_common.h sc_tap_mask_ok): the validity of a row's taps is one 32-bit word, bit r * S + q.  Every family
    that keeps one answers 0 to 6x6 and 7x7 filters and 1 to 5x5 where it takes 5x5 at all.  (The entry points' refusal itself is
    asserted on the device, tests/test_conv_tiles_gpu.py.)
  * PIXEL WALK (sc_pixel_walk_ok): the kernels unflatten a pixel index with fast_div(n, 1.0f / d) = (int)(((float)n + 0.5f) * inv)
    (csrc/conv_common.h).  Restated here in numpy float32 -- the same two roundings, inv = float32(1) / float32(d); no fast-math
    flag is in scouter_amd/_build.py -- it is exact for EVERY divisor d >= 1 and EVERY 0 <= n < 2^22, by enumeration: the expression
    is monotone in n (a conversion, an addition and a multiplication by a positive constant, each rounded monotonically, then a
    truncation) and floor(n / d) steps only at multiples of d, so checking n = k * d - 1 (must give k - 1) and n = k * d (must give
    k) for every k covers every n between them; divisors above n give (n + 0.5) * inv < 1 through the k = 1 pair.  Past 2^22 it is
    wrong (first at n = 4 201 469, d = 4095).  What the prologues hand it: blk_rem < Ho * Wo with d = Wo; blk_x + rowoff < Wo + 256
    with d = Wo; blk_y + qx < Ho + 256 with d = Ho (rowoff, and so the carry qx, below the tallest block tile: 256 rows) -- all below
    Ho * Wo + 256, which the rule keeps at or below 2^22.  Every family's query is then asked at the largest map the rule admits
    at a few widths (inside the proven domain) and one map row later (refused)."""
import collections

import numpy as np
import pytest

from test_conv_tiles_gpu import (ADD, ADDEND, BIAS, CASES, DY, FWD_EPILOGUES, GEOMETRIES, GROUPS, ONE_STAGE_MAX, RELU, STATS,     # noqa: E402
                                 STRIDED, TILE_BM, TILE_BN, X, Y, bf16_k_tiles, case_id, gemm_of, instance_of, legal_tiles, query_of, ragged)

F32 = np.float32
WALK_MAX, WALK_ROWS = 1 << 22, 256             # csrc/conv_common.h SC_WALK_MAX, SC_WALK_ROWS
MAX_PIXELS = WALK_MAX - WALK_ROWS              # the most pixels of one image a pixel-walking kernel takes


@pytest.fixture(scope="module")
def kk():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


# ---- the case table of the GPU test
def test_every_case_names_a_tile_its_query_accepts(kk):
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        name, args = query_of(c)
        assert kk.ask(name, *args) == 1, (case_id(c), name, args)
        assert c.tile in legal_tiles(c), case_id(c)
    # the tiles the GPU test launches besides the listed ones, for the bit comparison
    for g in GROUPS:
        for t in legal_tiles(g[0]):
            name, args = query_of(g[0]._replace(tile=t))
            assert kk.ask(name, *args) == 1, (case_id(g[0]), t)
    # ... and a strided input gradient is no case of the bf16 entry point: its query answers 0
    assert not [c for c in CASES if c.kind == "bf16" and c.dgrad and c.stride != 1]
    for geom in STRIDED:
        B, H, W, kh, kw, s, p = geom
        assert kk.ask("dgrad_bf16_tile_ok", B, H, W, 128, 64, kh, kw, s, p, 1, 1, 0, 0, 0) == 0
        assert kk.ask("dgrad_tile_ok", B, H, W, 128, 64, kh, kw, s, p, 1, 1, 0) == 1


def test_the_cases_reach_every_kernel_instance_on_a_ragged_m():
    on_ragged = collections.defaultdict(set)
    for c in CASES:
        if ragged(c):
            on_ragged[c.kind].add(instance_of(c))
    # (STRIDED is an instantiation of the input gradient only: a strided forward runs the general kernel)
    want = {(t, d, a) for t in range(4) for d in (False, True) for a in ("pw", "general", "strided") if d or a != "strided"}
    assert on_ragged["fp32"] >= want, "no ragged fp32 case runs (tile, DGRAD, addressing) %s" % sorted(want - on_ragged["fp32"])
    want = {(t, d, kt, a16) for t in range(4) for d in (False, True) for kt in (32, 64) for a16 in (False, True)}
    assert on_ragged["bf16"] >= want, "no ragged bf16 case runs (tile, DGRAD, KT, A_BF16) %s" % sorted(want - on_ragged["bf16"])


def test_every_geometry_runs_on_two_tile_heights_in_both_passes():
    for kind in ("fp32", "bf16"):
        for geom in GEOMETRIES:
            for dgrad in (False, True):
                if kind == "bf16" and dgrad and geom[5] != 1:
                    continue
                bms = {TILE_BM[c.tile] for c in CASES
                       if (c.kind, c.dgrad, c.B, c.H, c.W, c.kh, c.kw, c.stride, c.pad) == (kind, dgrad, *geom)}
                assert bms == {64, 128}, (kind, geom, dgrad, bms)


def test_the_cases_reach_the_channel_counts_groups_epilogues_and_storages():
    for kind in ("fp32", "bf16"):
        cs = [c for c in CASES if c.kind == kind]
        assert {32, 96, 128} <= {gemm_of(c)[1] for c in cs}
        # two column tiles at least once per tile; tile 3 on 96 columns (three)
        for t, bn in enumerate(TILE_BN):
            assert any(c.tile == t and gemm_of(c)[2] // bn >= 2 for c in cs), (kind, t)
        assert any(c.tile == 3 and gemm_of(c)[2] == 96 for c in cs)
        for dgrad in (False, True):
            grouped = {(c.groups, gemm_of(c)[1]) for c in cs if c.dgrad == dgrad and c.groups > 1}
            assert {g for g, _ in grouped} == {2, 3} and {k for _, k in grouped} == {32, 64}, (kind, dgrad, grouped)
            # all three factors of the block index: groups, column tiles per group and M tiles above one
            assert any(c.groups > 1 and gemm_of(c)[2] // TILE_BN[c.tile] > 1 and ragged(c) for c in cs if c.dgrad == dgrad)
        for geom in ((5, 9, 13, 3, 3, 1, 1), (5, 9, 13, 1, 1, 1, 0)):
            for t in range(4):
                epis = {c.epi for c in cs if not c.dgrad and c.tile == t and (c.B, c.H, c.W, c.kh, c.kw, c.stride, c.pad) == geom}
                assert epis >= set(FWD_EPILOGUES), (kind, geom, t, epis)
        assert set(FWD_EPILOGUES) == {0, BIAS, ADDEND, RELU, BIAS | ADDEND | RELU, STATS, STATS | BIAS}
        for t in range(4):
            assert {c.epi for c in cs if c.dgrad and c.tile == t and ragged(c)} == {0, ADDEND}, (kind, t)
    bf = [c for c in CASES if c.kind == "bf16" and ragged(c)]
    for t in range(4):
        assert {c.io for c in bf if not c.dgrad and c.tile == t} == {0, X, Y, X | Y}, t
        assert {c.io for c in bf if c.dgrad and c.tile == t} >= {0, DY, ADD}, t
    assert all(c.io == 0 for c in CASES if c.kind == "fp32")
    assert all(c.epi & ADDEND for c in CASES if c.dgrad and c.io & ADD)
    # the bf16 kernel's stage switch: input gradients of 27, 32 and 36 K tiles; forwards of one and of two
    kt = {bf16_k_tiles(c) for c in bf if c.dgrad}
    assert {27, ONE_STAGE_MAX, 36} <= kt and ONE_STAGE_MAX == 32, sorted(kt)
    assert {1, 2} <= {bf16_k_tiles(c) for c in bf if not c.dgrad}


# ---- the tap mask
FAMILIES = {  # query -> arguments after (B, H, W, Cin, Cout, kh, kw, stride, pad, groups)
    "fwd_tile_ok": (3, 0), "dgrad_tile_ok": (3, 0), "fwd_bf16_tile_ok": (3, 0, 0, 0), "dgrad_bf16_tile_ok": (3, 0, 0, 0),
    "fwd_planes_tile_ok": (3, 1, 0, 0), "dgrad_planes_tile_ok": (3, 1, 0),
}


def test_filters_of_more_than_32_taps_are_refused_by_every_family_with_a_tap_mask(kk):
    for name, tail in FAMILIES.items():
        for k, ok in ((5, 1), (6, 0), (7, 0)):
            assert kk.ask(name, 2, 8, 8, 64, 64, k, k, 1, k // 2, 1, *tail) == ok, (name, k)
        # rectangular: 4 x 8 = 32 taps fit, 3 x 11 and 11 x 3 = 33 do not (the fp32 / bf16-input kernels take any filter shape)
        if "planes" not in name:
            assert kk.ask(name, 2, 16, 16, 64, 64, 4, 8, 1, 0, 1, *tail) == 1, name
            assert kk.ask(name, 2, 16, 16, 64, 64, 3, 11, 1, 0, 1, *tail) == 0 and kk.ask(name, 2, 16, 16, 64, 64, 11, 3, 1, 0, 1, *tail) == 0, name
    # the register-split family bounds its filters itself (odd same-size filters up to 5 x 5)
    for name in ("fwd_x3_tile_ok", "dgrad_x3_tile_ok"):
        assert kk.ask(name, 2, 8, 8, 64, 64, 5, 5, 1, 2, 1, -1, 0) == 1 and kk.ask(name, 2, 8, 8, 64, 64, 7, 7, 1, 3, 1, -1, 0) == 0
    # a pointwise layer has one tap whatever else is large
    assert kk.ask("fwd_tile_ok", 2, 8, 8, 64, 64, 1, 1, 1, 0, 1, 3, 0) == 1


# ---- the pixel walk
def fast_div(n, d):
    """csrc/conv_common.h fast_div(n, 1.0f / (float)d) on arrays: fp32 reciprocal, fp32 n + 0.5, fp32 product, truncation"""
    inv = F32(1) / d.astype(F32)
    return ((n.astype(F32) + F32(0.5)) * inv).astype(np.int64)


def _wrong(limit):
    """-> (count, smallest n) of the pairs n in {k * d - 1, k * d}, n < limit, d >= 1, on which fast_div is not floor(n / d);
    the divisors an octave at a time"""
    bad, first, j = 0, None, 0
    while (1 << j) < limit:
        d = np.arange(1 << j, min(2 << j, limit), dtype=np.int64)[:, None]
        k = np.arange(1, limit // (1 << j) + 1, dtype=np.int64)[None, :]
        n = k * d
        for nn, want in ((n - 1, k - 1), (n, k)):
            m = (nn < limit) & (fast_div(nn, d) != want)
            if m.any():
                bad += int(m.sum())
                first = int(nn[m].min()) if first is None else min(first, int(nn[m].min()))
        j += 1
    return bad, first


def test_fast_div_is_exact_on_the_whole_guarded_domain():
    """Every divisor, every n < 2^22 (see the module docstring for why the two n per multiple suffice): the block starts blk_rem,
    and the per-row arguments blk_x + rowoff and blk_y + qx, which the rule keeps below Ho * Wo + 256 <= 2^22."""
    assert _wrong(WALK_MAX) == (0, None)
    assert MAX_PIXELS + WALK_ROWS == WALK_MAX
    # the largest arguments of each kind at the extreme maps the rule admits: one row of 2^22 - 256 pixels, one column of them
    for ho, wo in ((1, MAX_PIXELS), (MAX_PIXELS, 1), (16447, 255)):
        assert ho * wo <= MAX_PIXELS
        assert max(ho * wo - 1, wo - 1 + WALK_ROWS - 1, ho - 1 + WALK_ROWS - 1) < WALK_MAX


def test_fast_div_is_wrong_past_the_domain_so_the_guard_is_what_protects_the_kernels():
    """If someone "fixes" this restatement instead of the guard, these constants show it: the first failure past 2^22, the block
    start the issue was found at (Wo = 255, n = 4 275 584 = 128 * 33 403: row 16 767 for 16 766), and the widths of the models."""
    bad, first = _wrong(WALK_MAX + (1 << 13))
    assert first == 4201469 and bad > 0
    one = lambda n, d: int(fast_div(np.array([n]), np.array([d]))[0])
    assert one(4201469, 4095) == 4201469 // 4095 + 1
    assert 4275584 % 128 == 0 and 4275584 // 255 == 16766 and one(4275584, 255) == 16767
    for w in (56, 112, 224):
        n = np.arange(WALK_MAX, 6291488, dtype=np.int64)
        wrong = n[fast_div(n, np.full_like(n, w)) != n // w]
        assert wrong.size and int(wrong[0]) == 6291487, (w, wrong[:3])


def _largest_h(ask, w):
    """the tallest map of width w the query takes, by bisection (the rules are monotone in H up to their other guards)"""
    lo, hi = 128, 1 << 23
    assert ask(lo, w) and not ask(hi, w)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ask(mid, w) else (lo, mid)
    return lo


def _walkers(kk):
    """every family that unflattens pixels with fast_div: name -> ask(H, W) at one image, few channels (its other guards far away),
    and the GEMM-row map (rows, columns) of an H x W input"""
    q = kk.ask
    same = lambda h, w: (h, w)
    return {
        "fp32 forward 3x3": (lambda h, w: q("fwd_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, 3, 0), same),
        "fp32 input gradient 3x3": (lambda h, w: q("dgrad_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, 3, 0), same),
        "fp32 input gradient 3x3 / stride 2": (lambda h, w: q("dgrad_tile_ok", 1, h, w, 32, 32, 3, 3, 2, 1, 1, 3, 0), same),
        "bf16 forward 3x3": (lambda h, w: q("fwd_bf16_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, 3, 0, 0, 0), same),
        "bf16 forward 1x1": (lambda h, w: q("fwd_bf16_tile_ok", 1, h, w, 32, 32, 1, 1, 1, 0, 1, 3, 0, 0, 0), same),
        "bf16 input gradient 3x3": (lambda h, w: q("dgrad_bf16_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, 3, 0, 0, 0), same),
        "register-split forward 3x3": (lambda h, w: q("fwd_x3_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, -1, 0), same),
        "register-split input gradient 3x3": (lambda h, w: q("dgrad_x3_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, -1, 0), same),
        "resident-rows tile 7": (lambda h, w: q("fwd_x3_tile_ok", 1, h, w, 32, 32, 3, 3, 1, 1, 1, 7, 0), same),
        "plane forward 3x3": (lambda h, w: q("fwd_planes_tile_ok", 1, h, w, 32, 64, 3, 3, 1, 1, 1, 1, 1, 0, 0), same),
        "plane forward 1x1": (lambda h, w: q("fwd_planes_tile_ok", 1, h, w, 32, 64, 1, 1, 1, 0, 1, 1, 1, 0, 0), same),
        "plane input gradient 3x3": (lambda h, w: q("dgrad_planes_tile_ok", 1, h, w, 64, 32, 3, 3, 1, 1, 1, 1, 1, 0), same),
        "plane weight gradient 3x3": (lambda h, w: q("wgrad_planes_plan_ok", 1, h, w, 64, 64, 3, 3, 1, 1, 1, 1), same),
        "fp32 weight gradient 3x3 (64 channels)": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 64, 64, 3, 3, 1, 1, 1, kk.WGRAD_F32), same),
        "fp32 weight gradient 3x3 / stride 2": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 64, 64, 3, 3, 2, 1, 1, kk.WGRAD_F32),
                                               lambda h, w: ((h - 1) // 2 + 1, (w - 1) // 2 + 1)),
        "tap-fused fp32 weight gradient": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 32, 64, 3, 3, 1, 1, 1, kk.WGRAD_TAPS), same),
        "bf16 weight gradient 3x3": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 64, 64, 3, 3, 1, 1, 1, kk.WGRAD_BF16), same),
        "tap-fused plane weight gradient": (lambda h, w: q("wgrad_planes_plan_ok", 1, h, w, 64, 64, 3, 3, 1, 1, 1, 64), same),
        "register-split weight gradient": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 32, 64, 3, 3, 1, 1, 1, kk.WGRAD_XWT), same),
        "tap-fused bf16 weight gradient": (lambda h, w: q("wgrad_kernel_ok", 1, h, w, 32, 64, 3, 3, 1, 1, 1, kk.WGRAD_BWT), same),
    }


# the widest map of the families that keep rows resident
NARROW = {"resident-rows tile 7": 126, "tap-fused plane weight gradient": 63, "register-split weight gradient": 112,
          "tap-fused bf16 weight gradient": 112}


WIDTHS = (1, 56, 255, 4095)


def test_every_pixel_walking_family_stops_inside_the_proven_domain(kk):
    for name, (ask, rows_of) in _walkers(kk).items():
        for w in WIDTHS:
            if not ask(128, w):
                assert w > NARROW[name], (name, w)                 # (a width the family does not take at all)
                continue
            h = _largest_h(ask, w)
            ho, wo = rows_of(h, w)
            # the largest Ho * Wo admitted lies inside the domain, with room for the per-row arguments ...
            assert ho * wo + WALK_ROWS <= WALK_MAX, (name, w, h)
            # ... it IS this rule that stops the family there (the most rows of width wo the rule admits), and one GEMM row more
            # is refused
            assert ho == MAX_PIXELS // wo, (name, w, h, ho, MAX_PIXELS // wo)
            h1 = next(hh for hh in range(h + 1, h + 4) if rows_of(hh, w)[0] > ho)
            assert not ask(h1, w), (name, w, h1)
    # the kernels that walk no pixels keep their old limits: pointwise layers of the fp32 kernel, the register-split pointwise
    # kernel and the pointwise weight gradients take an image of 2^22 pixels and more
    h = (1 << 23) // 256 - 1                     # (just inside the fp32 kernel's image guard, H * W * C < 2^28)
    assert h * 256 > WALK_MAX
    assert kk.ask("fwd_tile_ok", 1, h, 256, 32, 32, 1, 1, 1, 0, 1, 3, 0) == 1 and kk.ask("dgrad_tile_ok", 1, h, 256, 32, 32, 1, 1, 1, 0, 1, 3, 0) == 1
    # (the register-split pointwise kernel needs 64 channels and H * W * Cin < 2^28: just short of 2^22 pixels, past 2^22 - 256)
    assert kk.ask("fwd_x3_tile_ok", 1, WALK_MAX - 1, 1, 64, 64, 1, 1, 1, 0, 1, -1, 0) == 1
    assert kk.ask("fwd_x3_tile_ok", 1, WALK_MAX - 1, 1, 32, 64, 3, 3, 1, 1, 1, -1, 0) == 0
    assert kk.ask("wgrad_kernel_ok", 1, h, 256, 32, 32, 1, 1, 1, 0, 1, kk.WGRAD_F32) == 1
    assert kk.ask("wgrad_kernel_ok", 1, h, 256, 32, 32, 1, 1, 1, 0, 1, kk.WGRAD_BF16) == 1
    # many images of an admitted map are as before: the bound is per image
    assert kk.ask("fwd_tile_ok", 64, 1024, 1024, 32, 32, 3, 3, 1, 1, 1, 3, 0) == 1
    assert kk.ask("fwd_tile_ok", 1, 2048, 2048, 32, 32, 3, 3, 1, 1, 1, 3, 0) == 0           # (2^22 pixels: 256 too many)
