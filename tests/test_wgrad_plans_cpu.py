"""What the case table of tests/test_wgrad_plans_gpu.py reaches, asked of the library on the CPU: integers only, no device.

scouter_conv2d_wgrad_plan (include/scouter_hip.h; kernels.ask("wgrad_plan", ...)) answers with the launchers' own wgrad_plan() and
wgrad_same_mode(): block tile, split count, pixels per split and addressing mode of the per-tap weight-gradient launch for a shape
and plan.  Here the GPU test's CASES must, between them, reach every instance of wgrad_kernel and wgrad_bf16_kernel, the chunk
counts around the two-fold unrolled software pipeline, budget bits that change the split, and the split counts around the loop
bounds of slab_reduce_kernel -- and tests/golden/wgrad_plan_cases.json records the answer for every case, so a case that is
deleted, or a wgrad_plan() that sends a listed case elsewhere, is a red test that names it.  (After a deliberate change of either:
`python tests/test_wgrad_plans_cpu.py` rewrites the record; the coverage assertions below are what has to hold then.)
Also here: every weight-gradient entry of the committed tuning table names a plan its wrapper offers."""
import json
import os
import sys

import pytest

from test_wgrad_plans_gpu import ALL_PLANS, BF16_BUDGET, CASES, F32_BUDGET, case_id, out_pixels, plan_of, shape_of     # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan_cases.json")
FIELDS = ("bm", "bn", "splits", "pix_per_split", "mode")


def _kernels():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def kk():
    return _kernels()


@pytest.fixture(scope="module")
def plans(kk):
    return [(c, plan_of(kk, c)) for c in CASES]


def _chunk_counts(c, pl, chunk):
    """chunks of `chunk` pixels the workgroups of the case walk: a full split's and the last split's"""
    M, pps = out_pixels(c), pl["pix_per_split"]
    last = M - (pl["splits"] - 1) * pps
    return ({-(-pps // chunk)} if pl["splits"] > 1 else set()) | {-(-last // chunk)}


def test_the_query_answers_the_fields_and_refuses_what_the_entry_points_refuse(kk):
    q = kk.ask
    assert kk.WGRAD_PLAN_FIELDS == FIELDS
    pw = (5, 9, 13, 128, 64, 1, 1, 1, 0, 1)
    assert [q("wgrad_plan", *pw, kk.WGRAD_F32, -1, f) for f in range(5)] == [128, 64, 3, 256, 2]
    assert [q("wgrad_plan", *pw, kk.WGRAD_F32, 48, f) for f in range(5)] == [64, 32, 3, 256, 2]
    assert q("wgrad_plan", *pw, kk.WGRAD_BF16, 48, 0) == 64 and q("wgrad_plan", *pw, kk.WGRAD_BF16, 48, 1) == 64      # (no 32-wide tiles)
    # the mode switch of a same-size 3x3 layer on a 5-wide map: 32 / 5 + 1 = 7 rows are too few for the pixel walk
    assert q("wgrad_plan", 3, 8, 5, 64, 64, 3, 3, 1, 1, 1, kk.WGRAD_F32, -1, 4) == 1
    assert q("wgrad_plan", 3, 7, 5, 64, 64, 3, 3, 1, 1, 1, kk.WGRAD_F32, -1, 4) == 0
    assert q("wgrad_plan", 3, 9, 11, 64, 64, 3, 3, 2, 1, 1, kk.WGRAD_F32, -1, 4) == 0
    # refused exactly where scouter_conv2d_wgrad_kernel_ok says the entry point refuses
    for shape in ((3, 8, 5, 48, 64, 3, 3, 1, 1, 1), (3, 8, 5, 64, 64, 3, 3, 1, 1, 3), (0, 8, 5, 64, 64, 3, 3, 1, 1, 1),
                  (3, 8, 5, 64, 64, 3, 3, 0, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 64, 64, 1, 1, 1, 0, 1)):
        for kernel in (kk.WGRAD_F32, kk.WGRAD_BF16):
            assert q("wgrad_kernel_ok", *shape, kernel) == 0
            assert all(q("wgrad_plan", *shape, kernel, plan, f) == -1 for plan in (-1, 0, 51) for f in range(5)), shape
    for shape in ((17, 5, 13, 64, 128, 3, 3, 1, 1, 1), (3, 9, 11, 64, 64, 3, 3, 2, 1, 1), (2, 9, 7, 64, 64, 3, 3, 1, 0, 1)):
        assert q("wgrad_kernel_ok", *shape, kk.WGRAD_F32) == 1 and q("wgrad_kernel_ok", *shape, kk.WGRAD_BF16) == 0
        assert q("wgrad_plan", *shape, kk.WGRAD_F32, -1, 0) == 64 and q("wgrad_plan", *shape, kk.WGRAD_BF16, -1, 0) == -1
    assert q("wgrad_plan", *pw, 2, -1, 0) == -1 and q("wgrad_plan", *pw, kk.WGRAD_F32, -1, 5) == -1 and q("wgrad_plan", *pw, -1, -1, 0) == -1


def test_every_case_is_one_the_per_tap_kernels_run(kk, plans):
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c, pl in plans:
        assert min(pl.values()) >= 0 and pl["splits"] >= 1, (case_id(c), pl)
        assert c.plan in ALL_PLANS and c.plan in kk._WGRAD_PLANS, case_id(c)
        assert pl["splits"] == -(-out_pixels(c) // pl["pix_per_split"]), (case_id(c), pl)
        # the workspace the wrapper is told to bring holds the slabs of this plan (the entry point returns an error if not)
        slabs = pl["splits"] * c.k * c.k * (c.cin // c.groups) * c.cout * 4 if pl["splits"] > 1 else 0
        assert kk.ask("wgrad_workspace_bytes", *shape_of(c), c.plan) >= slabs, (case_id(c), pl, slabs)
        if c.kind == "bf16":
            assert out_pixels(c) >= kk.BF16_MIN_PIXELS and pl["mode"] in (1, 2) and pl["pix_per_split"] % 64 == 0, (case_id(c), pl)
        elif c.plan < 0:
            # the fp32 entry point's own plan is a tap-fused kernel on these shapes, whatever the switches say
            assert not kk.ask("wgrad_kernel_ok", *shape_of(c), kk.WGRAD_TAPS), case_id(c)
        if c.kind == "refused":
            assert out_pixels(c) >= kk.BF16_MIN_PIXELS and not kk.ask("wgrad_kernel_ok", *shape_of(c), kk.WGRAD_BF16)


def test_the_cases_reach_every_kernel_instance(plans):
    f32 = {(pl["bm"], pl["bn"], pl["mode"]) for c, pl in plans if c.kind != "bf16"}
    want = {(bm, bn, mode) for bm in (128, 64, 32) for bn in (128, 64, 32) for mode in (0, 1, 2)}
    assert f32 == want, "no case runs wgrad_kernel<BM, BN, .., MODE> for (BM, BN, MODE) in %s" % sorted(want - f32)
    bf16 = {}
    for c, pl in plans:
        if c.kind == "bf16":
            bf16.setdefault((pl["bm"], pl["bn"], pl["mode"]), set()).add(c.storage)
    want = {(bm, bn, mode): {0, 1, 2, 3} for bm in (128, 64) for bn in (128, 64) for mode in (1, 2)}
    missing = sorted((k, st) for k, sts in want.items() for st in sts - bf16.get(k, set()))
    assert not missing and set(bf16) == set(want), "no case runs wgrad_bf16_kernel for ((BM, BN, MODE), storage) in %s" % missing


def test_the_cases_reach_the_chunk_counts_around_the_pipeline(plans):
    f32 = [(c, pl) for c, pl in plans if c.kind != "bf16"]
    kts = set().union(*(_chunk_counts(c, pl, 32) for c, pl in f32))
    missing = [k for k in (1, 2, 3) if k not in kts] + ([] if any(k >= 9 and k & 1 for k in kts) else ["an odd count >= 9"])
    assert not missing, "no fp32 case has a split of %s 32-pixel chunks (has %s)" % (missing, sorted(kts))
    assert any(out_pixels(c) % pl["pix_per_split"] % 32 for c, pl in f32), "no fp32 case ends in a chunk of fewer than 32 pixels"
    assert any(out_pixels(c) < 32 for c, pl in f32), "no fp32 case is smaller than one chunk"
    kts = set().union(*(_chunk_counts(c, pl, 64) for c, pl in plans if c.kind == "bf16"))
    assert {1, 4, 5} <= kts, "bf16 cases: splits of %s 64-pixel chunks" % sorted(kts)        # (a short last split, even, odd)
    assert any(out_pixels(c) % pl["pix_per_split"] % 64 for c, pl in plans if c.kind == "bf16")


def test_the_budget_bits_change_the_split_on_one_geometry_of_each_kernel(plans):
    """All 17 plans are listed for one fp32 and one bf16 geometry on which the budget bits give different pixel counts per split,
    one of them an odd count of chunks.  (wgrad_plan rounds the bf16 kernel's splits to whole 64-pixel chunks, so there the odd
    count is a pixel count that is no multiple of 128; the fp32 kernel's is no multiple of 64.)"""
    for kind, budget, odd in (("fp32", F32_BUDGET, 64), ("bf16", BF16_BUDGET, 128)):
        b = budget[:5] + (budget[5],) + budget[5:]
        by_plan = {c.plan: pl["pix_per_split"] for c, pl in plans if c.kind == kind and shape_of(c) == b}
        assert set(by_plan) == set(ALL_PLANS), (kind, sorted(by_plan))
        for tile_bits in (0, 16, 32, 48):
            pps = {by_plan[tile_bits | bits] for bits in range(4)}
            assert len(pps) >= 2, (kind, tile_bits, by_plan)
        assert any(v % odd for v in by_plan.values()), (kind, by_plan)
        if kind == "bf16":
            storages = {c.storage for c, pl in plans if c.kind == kind and shape_of(c) == b}
            assert storages == {0, 1, 2, 3}


def test_the_cases_reach_the_split_counts_around_the_slab_sum_loop(plans):
    """slab_reduce_kernel: 32 split lanes, each adding four slabs per turn of `k + 96 < splits` and the rest one by one"""
    splits = sorted(pl["splits"] for c, pl in plans if c.kind == "fp32" and c.plan < 0 and (c.cin, c.cout, c.k, c.H, c.W) == (32, 32, 1, 1, 1))
    missing = [s for s in (1, 2, 32, 33, 96, 97, 128, 129) if s not in splits]
    assert not missing and len([s for s in splits if s > 224]) >= 2, "pointwise 32 -> 32 cases: no split count %s (has %s)" % (missing, splits)


def test_the_recorded_answer_of_every_case(plans):
    with open(GOLDEN) as f:
        rec = json.load(f)
    now = {case_id(c): [pl[f] for f in FIELDS] for c, pl in plans}
    assert sorted(set(rec) - set(now)) == [], "cases deleted from tests/test_wgrad_plans_gpu.py"
    assert sorted(set(now) - set(rec)) == [], "cases without a record (see this file's docstring)"
    changed = {k: (rec[k], v) for k, v in now.items() if rec[k] != v}
    assert not changed, "(bm, bn, splits, pix_per_split, mode) recorded / now: %s" % changed


def test_every_weight_gradient_entry_of_the_tuning_table_names_an_offered_plan(kk):
    with open(kk.TUNE_TABLE_PATH) as f:
        choices = json.load(f)["choices"]
    offered = {"wgrad": (-1,) + tuple(t | b for t in (0, 16, 32, 48) for b in range(4))}
    offered["pwgrad"] = offered["wgrad"] + (64, 65, 66, 67)
    offered["xwgrad"] = (-1, 0, 1, 2, 3)
    assert (kk._WGRAD_PLANS, kk._PWGRAD_PLANS, kk._X3_WGRAD_PLANS) == (offered["wgrad"], offered["pwgrad"], offered["xwgrad"])
    seen = {}
    for key, plan in choices.items():
        p = key.split("|")
        kind, v = p[0], [int(s) for s in p[1:]]
        if kind not in offered:
            continue
        assert plan in offered[kind], (key, plan)
        if kind == "wgrad":
            # ... and is a plan of a kernel that takes the key's shape
            bf16, shape = v[0], v[1:]
            kernel = kk.WGRAD_BF16 if bf16 else kk.WGRAD_F32
            assert kk.ask("wgrad_kernel_ok", *shape, kernel) == 1 and kk.ask("wgrad_plan", *shape, kernel, plan, 2) >= 1, (key, plan)
        elif kind == "pwgrad":
            nplanes, B, H, W, Cin, Cout, kh, kw, pad, groups = v
            assert kk.ask("wgrad_planes_plan_ok", B, H, W, Cin, Cout, kh, kw, pad, groups, nplanes, plan) == 1, (key, plan)
        seen[kind] = seen.get(kind, 0) + 1
    assert seen == {"wgrad": 264, "pwgrad": 54}, seen


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    k_ = _kernels()
    with open(GOLDEN, "w") as f_:
        json.dump({case_id(c): [plan_of(k_, c)[f] for f in FIELDS] for c in CASES}, f_, indent=0)
        f_.write("\n")
    print("wrote %d cases to %s" % (len(CASES), GOLDEN))
