"""What the case tables of tests/test_wgrad_fused_gpu.py reach, asked of the library on the CPU: integers only, no device.

scouter_conv2d_wgrad_plan (kernels 2 - 4: the tap-fused launches, by the launchers' own wgrad_taps_plan()),
scouter_conv2d_wgrad_x3_plan (xw_plan()) and scouter_conv2d_wgrad_planes_plan (pwg_plan()) answer the column tile, split count and
pixels per split of a launch.  Here the GPU test's tables must, between them, reach every instance of the tap-fused, register-split
and plane weight-gradient kernels, every width class of the map rules, the pixel counts around the first split, odd and even last
splits, a `pix_per_split` past the floor of 256 for each tap-fused kernel (the register-split one rounded up from an odd chunk
count), split counts 1, 2 and > 128, the `want = 1` clamp, and the refusals -- and tests/golden/wgrad_fused_cases.json records
the answer for every case, so a case that is deleted, or a plan function that sends a listed case elsewhere, is a red test that
names it.  (After a deliberate change of either: `python tests/test_wgrad_fused_cpu.py` rewrites the record; the coverage
assertions below are what has to hold then.)  No case may be idle: each reaches something no other case of its table does."""
import json
import os
import sys

import pytest

import test_wgrad_fused_gpu as T                                           # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_fused_cases.json")


def _kernels():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def kk():
    return _kernels()


def _answers(kk):
    """{case id: the plan fields the library answers}, every table"""
    out = {}
    for c in T.TAPS_CASES:
        out[T.taps_id(c)] = [T.taps_plan(kk, c)[f] for f in T.TAPS_PLAN_FIELDS]
    for c in T.X3_CASES:
        for plan in T.X3_PLANS:
            out["%s-plan%d" % (T.x3_id(c), plan)] = [T.x3_plan(kk, c, plan)[f] for f in T.X3_PLAN_FIELDS]
    for c in T.PLANES_CASES + T.PLANES_REFUSED:
        for nplanes in (1, 3):
            out["%s-np%d" % (T.planes_id(c), nplanes)] = [T.planes_plan(kk, c, nplanes)[f] for f in T.PLANES_PLAN_FIELDS]
    return out


def _last(M, pl, chunk):
    """chunks of the last split, and whether its last chunk is ragged"""
    last = M - (pl["splits"] - 1) * pl["pix_per_split"]
    return -(-last // chunk), bool(last % chunk)


def _splits_class(n):
    return n if n <= 2 else "3..128" if n <= 128 else ">128"


def _idle(features):
    """ids whose feature set is covered by the union of the others'"""
    out = []
    for name, f in features.items():
        others = set().union(*(g for n, g in features.items() if n != name))
        if f <= others:
            out.append(name)
    return out


# ---------------------------------------------------------------------------------------------------------------- the queries
def test_the_queries_answer_with_the_launchers_plans_and_refuse_what_the_entry_points_refuse(kk):
    q = kk.ask
    assert (kk.WGRAD_TAPS_PLAN_FIELDS, kk.WGRAD_X3_PLAN_FIELDS, kk.WGRAD_PLANES_PLAN_FIELDS) == (
        T.TAPS_PLAN_FIELDS, T.X3_PLAN_FIELDS, T.PLANES_PLAN_FIELDS)
    s = (2, 2, 33, 96, 384, 3, 3, 1, 1, 3)                  # three groups of 32 -> 128
    assert [q("wgrad_plan", *s, kk.WGRAD_TAPS, -1, f) for f in range(5)] == [32, 64, 1, 256, 32]
    assert [q("wgrad_plan", *s, kk.WGRAD_XWT, -1, f) for f in range(5)] == [32, 64, 1, 256, 64]
    assert q("wgrad_plan", *s, kk.WGRAD_BWT, -1, 0) == -1 and q("wgrad_kernel_ok", *s, kk.WGRAD_BWT) == 0      # 64 / 33 + 1 = 2 rows: it needs three
    s = (2, 4, 33, 64, 192, 3, 3, 1, 1, 2)
    assert [q("wgrad_plan", *s, kk.WGRAD_BWT, -1, f) for f in range(5)] == [32, 32, 2, 256, 64]
    assert q("wgrad_plan", *s, kk.WGRAD_BWT, 17, 3) == 256 and q("wgrad_plan", *s, kk.WGRAD_TAPS, -1, 5) == -1
    # past the floor: ceil(chunks / want) chunks per split -- 1372 / 170 -> 9; 347 / 42 -> 9, rounded to 10; 350 / 85 -> 5
    big = (96, 384, 3, 3, 1, 1, 3)
    assert [q("wgrad_plan", 4, 98, 112, *big, kk.WGRAD_TAPS, -1, f) for f in (2, 3)] == [153, 288]
    assert [q("wgrad_plan", 1, 100, 111, *big, kk.WGRAD_XWT, -1, f) for f in (2, 3)] == [35, 320]
    assert [q("wgrad_plan", 1, 100, 111, *big, kk.WGRAD_TAPS, -1, f) for f in (2, 3)] == [44, 256]
    assert [q("wgrad_plan", 2, 100, 112, *big, kk.WGRAD_BWT, -1, f) for f in (2, 3)] == [70, 320]
    # every tap-fused code answers -1 exactly where scouter_conv2d_wgrad_kernel_ok answers 0
    for shape in ((2, 3, 33, 96, 384, 3, 3, 1, 1, 3), (2, 2, 113, 32, 64, 3, 3, 1, 1, 1), (2, 2, 33, 32, 64, 3, 3, 1, 1, 1),
                  (2, 9, 9, 64, 64, 3, 3, 1, 1, 1), (2, 9, 9, 32, 48, 3, 3, 1, 1, 1), (2, 9, 9, 32, 32, 3, 3, 2, 1, 1),
                  (2, 9, 9, 32, 32, 1, 1, 1, 0, 1), (2, 9, 9, 32, 32, 5, 5, 1, 2, 1), (0, 9, 9, 32, 32, 3, 3, 1, 1, 1)):
        for code in (kk.WGRAD_TAPS, kk.WGRAD_XWT, kk.WGRAD_BWT):
            ok = q("wgrad_kernel_ok", *shape, code)
            assert all((q("wgrad_plan", *shape, code, -1, f) == -1) == (ok == 0) for f in range(5)), (shape, code)
    assert q("wgrad_plan", 2, 9, 9, 32, 32, 3, 3, 1, 1, 1, kk.WGRAD_ROWS32, -1, 0) == -1        # (5 is a shape class, not a kernel)

    assert [q("wgrad_x3_plan", 11, 10, 10, 1024, 1024, -1, f) for f in range(4)] == [8, 8, 4, 288]
    assert [q("wgrad_x3_plan", 11, 10, 10, 1024, 1024, 3, f) for f in range(4)] == [8, 8, 5, 256]
    assert q("wgrad_x3_plan", 11, 10, 10, 1024, 1024, 3, 4) == -1
    for shape in ((1, 3, 3, 64, 128), (1, 3, 3, 128, 192), (0, 3, 3, 128, 128), (2 ** 16, 2 ** 8, 2 ** 8, 128, 128)):
        assert q("wgrad_x3_ok", *shape) == 0 and all(q("wgrad_x3_plan", *shape, p, f) == -1 for p in T.X3_PLANS for f in range(4))

    a = (3, 8, 5, 128, 128, 3, 3, 1, 1)
    assert [q("wgrad_planes_plan", *a, 1, -1, f) for f in range(5)] == [128, 128, 1, 256, 0]
    assert [q("wgrad_planes_plan", *a, 3, 48, f) for f in range(5)] == [64, 64, 1, 256, 0]
    assert [q("wgrad_planes_plan", *a, 3, 64, f) for f in range(5)] == [64, 64, 1, 256, 1]
    assert q("wgrad_planes_plan", *a, 3, 64, 5) == -1 and q("wgrad_planes_plan", *a, 2, -1, 0) == -1
    assert q("wgrad_planes_plan", 3, 8, 5, 128, 128, 5, 5, 2, 1, 3, 64, 4) == -1                # (tap-fused plans: 3x3 only)
    # the map rule 32 / W + 1 < H, one row short
    for B, H, W in ((3, 7, 5), (2, 33, 1), (2, 2, 32), (2, 2, 31), (2, 1, 63)):
        assert q("wgrad_planes_plan_ok", B, H, W, 64, 64, 3, 3, 1, 1, 3, -1) == 0
        assert q("wgrad_planes_plan", B, H, W, 64, 64, 3, 3, 1, 1, 3, -1, 0) == -1
        assert q("wgrad_planes_plan_ok", B, H + 1, W, 64, 64, 3, 3, 1, 1, 3, -1) == 1


# ------------------------------------------------------------------------------------------------------------- tap-fused
@pytest.fixture(scope="module")
def taps(kk):
    return [(c, T.taps_plan(kk, c)) for c in T.TAPS_CASES]


def _taps_features(kk, c, pl):
    M = c.B * c.H * c.W
    img = c.H * c.W
    f = {("tile", c.kind, pl["bn"], c.ng // pl["bn"], c.groups), ("width", c.kind, c.W), ("pps", c.kind, pl["pix_per_split"]),
         ("splits", c.kind, _splits_class(pl["splits"])), ("M", c.kind, M if M in (256, 257) else 0)}
    if c.kind in T.TAPS_KINDS:
        if M < pl["chunk"]:
            f.add(("below one chunk", c.kind))
        f.add(("images a chunk spans", c.kind, min(c.B, -(-(pl["chunk"] - 1) // img) + 1)))
        if pl["splits"] > 128:
            f.add(("more than 128 slabs of 9 x 32 x", c.kind, c.ng * c.groups))
        if pl["splits"] > 1:
            n, ragged = _last(M, pl, pl["chunk"])
            f.add(("last split", c.kind, min(n, 4) if n <= 4 else 4 + n % 2, ragged))
            at = pl["pix_per_split"] % img
            f.add(("first boundary", c.kind, "image" if at == 0 else "row" if at % c.W == 0 else "inside a row"))
    return f


def test_tap_fused_cases_run_the_kernel_they_name_with_the_workspace_they_are_given(kk, taps):
    ids = [T.taps_id(c) for c, _ in taps]
    assert len(set(ids)) == len(ids)
    for c, pl in taps:
        shape, M = T.taps_shape(c), c.B * c.H * c.W
        assert min(pl.values()) >= 0 and pl["splits"] == -(-M // pl["pix_per_split"]), (T.taps_id(c), pl)
        # the workspace the wrapper is told to bring holds the slabs of the plan that will run: with less, the launchers fall
        # back to the per-tap kernel without a word
        slabs = pl["splits"] * 9 * 32 * shape[4] * 4 if pl["splits"] > 1 else 0
        assert kk.ask("wgrad_workspace_bytes", *shape, -1) >= slabs, (T.taps_id(c), pl, slabs)
        if c.kind in T.TAPS_KINDS:
            assert pl["bm"] == 32 and pl["chunk"] == (32 if c.kind == "taps" else 64) and pl["pix_per_split"] % pl["chunk"] == 0
            assert c.H >= T.RULE_CHUNK[c.kind] // c.W + 2 and kk.ask("wgrad_kernel_ok", *shape, T.taps_code(kk, c.kind)) == 1
            # (what kernels.conv2d_wgrad asks before it rounds fp32-stored operands for the one-plane kernel)
            assert c.kind != "bwt" or kk.wgrad_prerounds(*shape), T.taps_id(c)
            # one row shorter and the kernel refuses the map
            short = (c.B, c.H - 1) + shape[2:]
            if c.H == T.RULE_CHUNK[c.kind] // c.W + 2:
                assert kk.ask("wgrad_kernel_ok", *short, T.taps_code(kk, c.kind)) == 0, T.taps_id(c)
        else:
            # width 113: past the rows of the register-split and the one-plane kernel
            assert c.W == 113 and kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_XWT) == 0 and kk.ask("wgrad_kernel_ok", *shape, kk.WGRAD_BWT) == 0
            assert kk.ask("wgrad_kernel_ok", *(shape[:2] + (112,) + shape[3:]), kk.WGRAD_XWT) == 1
            assert kk.ask("wgrad_kernel_ok", *(shape[:2] + (112,) + shape[3:]), kk.WGRAD_BWT) == 1
            assert kk.ask("wgrad_kernel_ok", *shape, T.taps_code(kk, c.kind)) == 1


def test_tap_fused_cases_reach_every_instance_width_and_split_edge(taps):
    for kind in T.TAPS_KINDS:
        mine = [(c, pl) for c, pl in taps if c.kind == kind]
        chunk = 32 if kind == "taps" else 64
        tiles = {(pl["bn"], c.ng // pl["bn"]) for c, pl in mine}
        assert tiles == {(32, 1), (64, 1), (32, 3), (64, 2)}, (kind, tiles)                      # 32, 64, 96, 128 per group
        assert {(c.ng, c.groups) for c, pl in mine} >= {(n, g) for n in (32, 64, 96, 128) for g in (1, 2, 3)}, kind
        # every width class at the shortest map the rule admits
        short = {c.W for c, pl in mine if c.H == T.RULE_CHUNK[kind] // c.W + 2}
        assert short >= set(T.WIDTHS), (kind, sorted(set(T.WIDTHS) - short))
        Ms = {c.B * c.H * c.W for c, pl in mine}
        assert {256, 257} <= Ms and any(c.B == 1 for c, pl in mine), kind
        assert {pl["splits"] for c, pl in mine if c.B * c.H * c.W in (256, 257)} == {1, 2}, kind
        # M below one chunk: only the register-split kernel has a chunk (64) longer than its map rule's (32) -- elsewhere
        # W * (chunk / W + 2) > chunk pixels are the smallest image
        assert any(c.B * c.H * c.W < chunk for c, pl in mine) == (kind == "xwt"), kind
        lasts = [_last(c.B * c.H * c.W, pl, chunk) for c, pl in mine if pl["splits"] > 1]
        assert any(n & 1 and n > 1 for n, _ in lasts) and any(not n & 1 for n, _ in lasts), (kind, lasts)
        assert any(r for _, r in lasts), kind
        # a ragged last chunk that begins inside a row (the tensor ends with a row, so it ends with one); split boundaries
        # inside a row, and inside an image at the start of a row
        assert any(pl["splits"] > 1 and M % chunk and (M - M % chunk) % c.W for c, pl in mine for M in [c.B * c.H * c.W]), kind
        bounds = {("row" if pl["pix_per_split"] % (c.H * c.W) % c.W == 0 else "inside") for c, pl in mine
                  if pl["splits"] > 1 and pl["pix_per_split"] % (c.H * c.W)}
        assert bounds == {"row", "inside"}, (kind, bounds)
        # a chunk that spans three images (64-pixel chunks on the 36-pixel images of the 32-pixel rule)
        if kind == "xwt":
            assert any(c.W == 3 and c.H * c.W + 2 <= chunk and c.B * c.H * c.W >= 2 * chunk for c, pl in mine)
        # past the floor: ceil(chunks / want) chunks per split, more than the floor's 256 pixels
        past = [(c, pl) for c, pl in mine if pl["pix_per_split"] > 256]
        assert past, "no %s case has more than 256 pixels per split" % kind
        if kind == "xwt":
            # ... of which one was rounded up from an odd count of 32-pixel chunks
            def odd_quotient(c, pl):
                want = max(1, 256 // (c.ng // pl["bn"] * c.groups))
                return (-(-(-(-c.B * c.H * c.W // 32)) // want)) & 1
            assert any(odd_quotient(c, pl) for c, pl in past), "no xwt case rounds an odd chunk count up"
    assert {_splits_class(pl["splits"]) for c, pl in taps} >= {1, 2, "3..128", ">128"}
    assert any(pl["splits"] > 128 and c.ng * c.groups == 32 for c, pl in taps)          # (the slab sum's four-loads loop on 9 * 32 * 32)
    assert {c.kind for c, pl in taps} == set(T.TAPS_KINDS) | {"wide-xwt", "wide-bwt"}


def test_no_tap_fused_case_is_idle(kk, taps):
    idle = _idle({T.taps_id(c): _taps_features(kk, c, pl) for c, pl in taps})
    assert not idle, "cases that reach nothing the others do not: %s" % idle


# ---------------------------------------------------------------------------------------------------- register-split pointwise
def _x3_features(c, plans):
    M = c.B * c.H * c.W
    f = {("tiles", min(plans[-1]["ci_tiles"], 2), min(plans[-1]["co_tiles"], 2)), ("M % 4", M % 4), ("M", M if M in (256, 257) else 0)}
    for p, pl in plans.items():
        n, ragged = _last(M, pl, 32)
        f |= {("splits", _splits_class(pl["splits"])), ("pps", pl["pix_per_split"]), ("last split", pl["splits"] > 1, min(n, 4), ragged)}
    f.add(("the plan matters", len({pl["pix_per_split"] for pl in plans.values()}) > 1))
    f.add(("want clamped to 1", plans[-1]["ci_tiles"] * plans[-1]["co_tiles"] > 256))
    return f


def test_register_split_cases_reach_the_plan_edges(kk):
    assert kk._X3_WGRAD_PLANS == T.X3_PLANS
    feats = {}
    for c in T.X3_CASES:
        M = c.B * c.H * c.W
        plans = {p: T.x3_plan(kk, c, p) for p in T.X3_PLANS}
        for p, pl in plans.items():
            assert min(pl.values()) >= 1 and pl["splits"] == -(-M // pl["pix_per_split"]), (T.x3_id(c), p, pl)
            assert (pl["ci_tiles"], pl["co_tiles"]) == (c.cin // 128, c.cout // 128)
            slabs = pl["splits"] * c.cin * c.cout * 4 if pl["splits"] > 1 else 0
            assert kk.ask("wgrad_x3_workspace_bytes", *c, p) >= slabs, (T.x3_id(c), p)
        feats[T.x3_id(c)] = _x3_features(c, plans)
    every = set().union(*feats.values())
    want = {("M", 256), ("M", 257), ("tiles", 1, 1), ("tiles", 2, 1), ("tiles", 1, 2), ("tiles", 2, 2), ("the plan matters", True),
            ("want clamped to 1", True), ("pps", 256), ("pps", 288), ("pps", 320), ("splits", 1), ("splits", 2), ("splits", "3..128"),
            ("last split", True, 3, True), ("last split", True, 1, True), ("last split", False, 1, True), ("M % 4", 1), ("M % 4", 3)}
    assert want <= every, sorted(want - every, key=repr)
    idle = _idle(feats)
    assert not idle, "shapes that reach nothing the others do not: %s" % idle


# ----------------------------------------------------------------------------------------------------------------- planes
def _planes_features(c, nplanes, pl):
    M = c.B * c.H * c.W
    f = {("instance", pl["bm"], pl["bn"], nplanes, pl["fused"]), ("width", c.W, pl["fused"]), ("k", c.k),
         ("channels", c.cin // c.groups, c.cout // c.groups, c.groups, pl["fused"]), ("plan", c.plan),
         ("splits", _splits_class(pl["splits"]), pl["fused"]), ("M", M if M in (256, 257) else 0)}
    if pl["splits"] > 1:
        n, ragged = _last(M, pl, 32)
        f.add(("last split", min(n, 4), ragged, pl["fused"]))
    return f


def test_plane_cases_reach_every_instance_and_edge(kk):
    feats, every = {}, set()
    for c in T.PLANES_CASES:
        both = set()
        for nplanes in (1, 3):
            pl = T.planes_plan(kk, c, nplanes)
            M = c.B * c.H * c.W
            assert min(pl.values()) >= 0 and pl["splits"] == -(-M // pl["pix_per_split"]), (T.planes_id(c), pl)
            assert c.plan in kk._PWGRAD_PLANS and pl["fused"] == (c.plan >= 64) and c.H >= 32 // c.W + 2, T.planes_id(c)
            slabs = pl["splits"] * c.k * c.k * (c.cin // c.groups) * c.cout * 4 if pl["splits"] > 1 else 0
            assert kk.ask("wgrad_planes_workspace_bytes", c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.groups, c.plan) >= slabs, T.planes_id(c)
            both |= _planes_features(c, nplanes, pl)
        feats[T.planes_id(c)] = both
        every |= both
    want = {("instance", bm, bn, np_, 0) for bm in (64, 128) for bn in (64, 128) for np_ in (1, 3)}
    want |= {("instance", 64, 64, 1, 1), ("instance", 64, 64, 3, 1)}
    want |= {("width", w, 0) for w in (1, 5, 31, 32, 33, 63, 64)} | {("width", w, 1) for w in (3, 62, 63)}
    want |= {("k", 1), ("k", 3), ("k", 5)} | {("plan", p) for p in (-1, 16, 32, 48, 64, 65, 66, 67)}
    want |= {("splits", 1, 0), ("splits", 2, 0), ("splits", 1, 1), ("splits", 2, 1), ("splits", "3..128", 1), ("M", 256), ("M", 257)}
    assert want <= every, sorted(want - every, key=repr)
    assert {f[1:3] for f in every if f[0] == "channels"} >= {(64, 64), (128, 128), (192, 192), (64, 128), (128, 64)}
    assert {f[3] for f in every if f[0] == "channels" and not f[4]} == {1, 2} == {f[3] for f in every if f[0] == "channels" and f[4]}
    assert any(f[0] == "last split" and f[2] for f in every)                                   # a ragged last chunk
    # plan bits 16 / 32 halve an axis of 128 channels
    assert any(c.plan >= 0 and c.plan & 16 and c.plan < 64 and (c.cin // c.groups) % 128 == 0 for c in T.PLANES_CASES)
    assert any(c.plan >= 0 and c.plan & 32 and c.plan < 64 and (c.cout // c.groups) % 128 == 0 for c in T.PLANES_CASES)
    # tap-fused plans: a 32-pixel chunk that spans two images, the shortest maps at the widest widths
    assert any(c.plan >= 64 and c.H * c.W < 64 and c.B > 2 for c in T.PLANES_CASES)
    assert any(c.plan >= 64 and c.W == 63 and c.H == 2 for c in T.PLANES_CASES)
    idle = _idle(feats)
    assert not idle, "cases that reach nothing the others do not: %s" % idle


def test_the_refused_plane_cases_are_refused_by_the_queries(kk):
    assert T.PLANES_REFUSED
    for c in T.PLANES_REFUSED:
        for nplanes in (1, 3):
            assert c.W == 64 and c.plan >= 64
            assert kk.ask("wgrad_planes_plan_ok", *T.planes_args(c, nplanes), c.plan) == 0
            assert set(T.planes_plan(kk, c, nplanes).values()) == {-1}
            assert kk.ask("wgrad_planes_plan_ok", *T.planes_args(c._replace(W=63), nplanes), c.plan) == 1


# ----------------------------------------------------------------------------------------------------------------- the record
def test_the_recorded_answer_of_every_case(kk):
    with open(GOLDEN) as f:
        rec = json.load(f)
    now = _answers(kk)
    assert sorted(set(rec) - set(now)) == [], "cases deleted from tests/test_wgrad_fused_gpu.py"
    assert sorted(set(now) - set(rec)) == [], "cases without a record (see this file's docstring)"
    changed = {k: (rec[k], v) for k, v in now.items() if rec[k] != v}
    assert not changed, "plan fields recorded / now: %s" % changed


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ans = _answers(_kernels())
    with open(GOLDEN, "w") as f_:
        json.dump(ans, f_, indent=0)
        f_.write("\n")
    print("wrote %d cases to %s" % (len(ans), GOLDEN))
