"""What tests/test_split_tiles_gpu.py reaches, asked on the CPU: integers only, no device.

  * QUERIES: for every case of the GPU table the matching *_tile_ok query (include/scouter_hip.h) answers 1 for the named tile,
    epilogue and storage -- the GPU run cannot be a re-route -- and 0 for every refusal and every falling-back hint the GPU file
    asserts; the GPU file's restatement of the rules (legal) agrees with the queries on every case and refusal.
  * INSTANCES: instance_of restates dispatch_pconv (csrc/conv_planes.hip), dispatch_x3 (csrc/conv_x3.hip) and sc_launch_xhalo
    (csrc/conv_xhalo.hip); the table reaches each of the 62 kernel instances on a ragged M.
  * TABLE: per family and pass every geometry on two tile heights, K per group 32 / 96 / 128, groups 2 and 3, every forward
    epilogue and every fused mode on every tile, tile 7's K per group 16 / 32 / 48 / 64 and its widths on both sides of 63 / 64: a
    later edit of the table cannot drop one quietly.
  * TILE 7's channel rule: 16-multiples of K per group run under sc_xhalo_ok; tiles 0-6 and the library's own choice keep
    32-multiples (both sides of the rule this file's GPU twin found too narrow)."""
import pytest

from test_split_tiles_gpu import (ADDEND, BIAS, BOTH, CASES, DGRAD_MODES, FWD_EPILOGUES, ONE_PLANE_FALLBACKS, PERSISTENT, PLANE_DGRAD,    # noqa: E402
                                  PLANE_FWD, RAGGED_PW, RAGGED_SAME, REFUSALS, RELU, STATS, STRIDED, TILE5, TILE5_TOO_WIDE, TILE7, TILE7_K,
                                  TILE7_WIDTHS, Y, case_id, gemm_of, geom_of, instance_of, legal, persistent_batch, persistent_case,
                                  query_of, ragged, tile_rows)


@pytest.fixture(scope="module")
def kk():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


def _ask(kk, c):
    name, args = query_of(c)
    return kk.ask(name, *args)


def _of(family, nplanes, dgrad):
    return [c for c in CASES if (c.family, c.nplanes, c.dgrad) == (family, nplanes, dgrad) and c.tile != 7]


FAMILIES = [("planes", 3), ("planes", 1), ("x3", 3)]


# ---- the queries
def test_every_case_names_a_tile_its_query_accepts(kk):
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert _ask(kk, c) == 1, (case_id(c), query_of(c))
        assert legal(c), case_id(c)
    # the persistent batches, as built for 256 CUs and for a few other CU counts
    for cus in (256, 304, 64, 8):
        B = persistent_batch(cus)
        assert -(-B * 255 // 256) == cus + 2 and B * 255 % 256
        for p in PERSISTENT:
            c = persistent_case(*p, cus)
            assert _ask(kk, c) == 1 and _ask(kk, c._replace(epi=0, fuse="")) == 1 and ragged(c), case_id(c)
    assert persistent_batch(256) == 259 and 259 * 255 - 257 * 256 == 253


def test_every_refusal_and_every_fallback_answers_zero(kk):
    for c, _ in REFUSALS:
        assert _ask(kk, c) == 0 and not legal(c), case_id(c)
    for c in ONE_PLANE_FALLBACKS + TILE5_TOO_WIDE:
        assert _ask(kk, c) == 0 and not legal(c), case_id(c)
        assert _ask(kk, c._replace(tile=1)) == 1, case_id(c)
    for c in TILE5_TOO_WIDE:
        assert _ask(kk, c._replace(W=63)) == 1
    # next to each refusal, what the rule does take
    t7 = REFUSALS[0][0]
    assert _ask(kk, t7._replace(epi=0)) == 1 and _ask(kk, t7._replace(epi=STATS)) == 1
    for c, text in REFUSALS:
        if c.family == "planes" and c.tile == 6:
            assert _ask(kk, c._replace(epi=c.epi & STATS, io=0)) == 1, case_id(c)
            assert _ask(kk, c._replace(tile=1)) == 1, case_id(c)              # (the LDS-staged tiles take both)
        if text == "stride":
            assert _ask(kk, c._replace(dgrad=False, cin=c.cout, cout=c.cin)) == 1, case_id(c)     # (the forward runs strided)
        if c.W == 127:
            assert _ask(kk, c._replace(W=126)) == 1, case_id(c)
    assert {c.W for c, _ in REFUSALS if c.tile == 7 and c.epi == 0} == {127}
    assert {geom_of(c) for c, t in REFUSALS if t == "stride"} == set(STRIDED)


def test_tile_7_has_its_own_channel_rule(kk):
    """sc_xhalo_ok: 16-multiples of K per group, 32 columns per group; x3_channels_ok (tiles 0-6 and the library's own choice):
    32-multiples and two K tiles"""
    for q, swap in (("fwd_x3_tile_ok", False), ("dgrad_x3_tile_ok", True)):
        def ask(kg, ncol, tile, groups=1, k=3):
            cin, cout = (ncol, kg) if swap else (kg, ncol)
            return kk.ask(q, 2, 9, 13, cin * groups, cout * groups, k, k, 1, k // 2, groups, tile, 0)
        for kg in range(8, 81, 8):
            for groups in (1, 2, 3):
                assert ask(kg, 32, 7, groups) == int(kg % 16 == 0), (q, kg, groups)
                for tile in (-1, 5, 6):
                    assert ask(kg, 32, tile, groups) == int(kg % 32 == 0), (q, kg, groups, tile)
        assert ask(32, 64, 7) == 0 and ask(16, 64, 7) == 0           # (32 columns per group, no more)
        assert ask(16, 32, 7, k=1) == 0 and ask(16, 32, 7, k=5) == 0   # (3x3 only)
        assert ask(32, 32, 6, k=1) == 0 and ask(64, 32, 6, k=1) == 1   # (two K tiles)


# ---- the instances
def test_the_cases_reach_all_62_kernel_instances_on_a_ragged_m():
    reached = {instance_of(c) for c in CASES if ragged(c)}
    tf = (False, True)
    pconv = {("pconv",) + i + (d,) for d in tf for i in ((128, 128, 3, 3), (128, 64, 3, 3), (128, 64, 3, 2), (64, 64, 3, 2),
                                                          (256, 128, 3, 2), (128, 128, 1, 3), (128, 64, 1, 3))}
    ppersist = {("ppersist", bn, np_, d) for bn in (128, 64) for np_ in (3, 1) for d in tf}
    phalo = {("phalo", bn, np_, d) for bn in (128, 64) for np_ in (3, 1) for d in tf}
    xgemm = {("xgemm", t, d, conv) for t in range(7) for d in tf for conv in tf}
    xhalo = {("xhalo", ag, d) for ag in (12, 16) for d in tf}
    assert (len(pconv), len(ppersist), len(phalo), len(xgemm), len(xhalo)) == (14, 8, 8, 28, 4)
    want = pconv | ppersist | phalo | xgemm | xhalo
    assert len(want) == 62
    assert reached >= want, "no ragged case runs %s" % sorted(want - reached, key=str)
    assert reached == want, "instance_of names an instance the dispatchers do not have: %s" % sorted(reached - want, key=str)


# ---- the table
def test_every_geometry_runs_on_two_tile_heights_in_both_passes():
    for family, np_ in FAMILIES:
        for dgrad in (False, True):
            geoms = BOTH if family == "x3" else PLANE_DGRAD if dgrad else PLANE_FWD
            cs = _of(family, np_, dgrad)
            for geom in geoms:
                heights = {tile_rows(c) for c in cs if geom_of(c) == geom}
                assert 256 in heights and heights - {256}, (family, np_, dgrad, geom, heights)
            assert {geom_of(c) for c in cs} - set(TILE5) == set(geoms) - set(TILE5), (family, np_, dgrad)
    # plane tile 5 and tile 7 on their own geometries
    for np_ in (3, 1):
        for dgrad in (False, True):
            assert {geom_of(c) for c in _of("planes", np_, dgrad) if c.tile == 5} >= set(TILE5) | {RAGGED_SAME}
    for dgrad in (False, True):
        t7 = [c for c in CASES if c.tile == 7 and c.dgrad == dgrad]
        assert {geom_of(c) for c in t7} >= set(TILE7) | {RAGGED_SAME}
        assert {(c.H, c.W) for c in t7 if geom_of(c) in TILE7} == {(h, w) for h in (5, 1) for w in TILE7_WIDTHS}
        assert {63, 64} <= set(TILE7_WIDTHS) and max(TILE7_WIDTHS) == 126
        assert {(gemm_of(c)[1], c.groups) for c in t7} >= {(k, g) for k in TILE7_K for g in (1, 2, 3)}
        assert all(gemm_of(c)[2] == 32 for c in t7)
        # both sides of the AG 12 / 16 switch with an odd count of 16-channel chunks
        assert {instance_of(c)[1] for c in t7 if gemm_of(c)[1] // 16 % 2} == {12, 16}


def test_the_cases_reach_the_channel_counts_groups_epilogues_and_modes():
    for family, np_ in FAMILIES:
        ntiles = (0, 1, 2, 3, 4, 5, 6) if np_ == 3 else (0, 1, 5, 6)
        for dgrad in (False, True):
            cs = _of(family, np_, dgrad)
            assert {32, 96, 128} <= {gemm_of(c)[1] for c in cs}, (family, np_, dgrad)
            assert {256, 128, 64} <= {gemm_of(c)[2] for c in cs}
            if family == "x3":
                assert {96, 32} <= {gemm_of(c)[2] for c in cs}
            grouped = {(c.groups, gemm_of(c)[1]) for c in cs if c.groups > 1}
            assert {g for g, _ in grouped} == {2, 3} and {k for _, k in grouped} >= {32, 64}, (family, np_, dgrad, grouped)
            # one column tile per group and two, on a ragged M
            bn = lambda c: instance_of(c)[2] if family == "planes" and c.tile < 5 else instance_of(c)[1] if family == "planes" else \
                (128, 128, 64, 64, 64, 32, 32)[c.tile]
            per_group = {gemm_of(c)[2] // bn(c) for c in cs if c.groups > 1 and ragged(c)}
            assert {1, 2} <= per_group, (family, np_, dgrad, per_group)
            for geom in (RAGGED_SAME, RAGGED_PW):
                tiles = [t for t in ntiles if not (t == 5 and family == "planes" and geom == RAGGED_PW)]
                on = [c for c in cs if geom_of(c) == geom]
                assert {c.tile for c in on} == set(tiles), (family, np_, dgrad, geom)
                for t in tiles:
                    mine = [c for c in on if c.tile == t]
                    if dgrad:
                        assert {(c.epi, c.fuse) for c in mine} == set(DGRAD_MODES), (family, np_, geom, t)
                    else:
                        epis = {c.epi for c in mine if not c.io}
                        refused = {STATS | BIAS} if family == "planes" and t == 6 else set()
                        assert epis == set(FWD_EPILOGUES) - refused, (family, np_, geom, t, epis)
                        if family == "planes":
                            assert {c.epi for c in mine if c.io & Y} == (set() if t == 6 else {0, BIAS | ADDEND | RELU})
    assert set(FWD_EPILOGUES) == {0, BIAS, ADDEND, RELU, BIAS | ADDEND | RELU, STATS, STATS | BIAS}
    assert {f for _, f in DGRAD_MODES} == {"", "bn", "bn-nomask", "bn2"} and (ADDEND, "bn2") in DGRAD_MODES and (ADDEND, "") in DGRAD_MODES
    # tile 7: the epilogues its rule takes, every fused mode
    t7 = [c for c in CASES if c.tile == 7 and geom_of(c) == RAGGED_SAME]
    assert {c.epi for c in t7 if not c.dgrad} == {0, RELU, STATS}
    assert {(c.epi, c.fuse) for c in t7 if c.dgrad} == set(DGRAD_MODES)
    assert all(c.io == 0 for c in CASES if c.family == "x3" or c.dgrad)

