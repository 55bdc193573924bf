"""The fused xSlot head's kernel instances, counted on the CPU (no device), and the fp64 restatement the GPU tests compare with.

  * tests/xslot_restatements.py -- every row the kernels store -- against fp64 autograd of oracle.torch_oracle.xslot_forward;
  * scouter_xslot_instance (include/scouter_hip.h, HEAD INSTANCES; the rule both entry points launch through) asked for every
    case of tests/xslot_cases.py: the set of instances reached EQUALS the inventory written out below, no case is idle (taking
    any one case out of the table loses an inventory entry or a required shape), and every boundary of the rule is bisected;
  * the backward's workspace figure covers what the selected instance addresses (the layouts of csrc/xslot_bwd.hip's comments);
  * the inputs of every case leave the reference inside the conditions the GPU bounds assume."""
import os

import pytest
import torch

from oracle import torch_oracle as O

import xslot_cases as XC
import xslot_restatements as R


@pytest.fixture(scope="module")
def kk():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import kernels
    return kernels


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,N,T,L,spc,ls", [(2, 6, 9, 3, 2, 3, -1), (3, 5, 7, 1, 1, 1, 1), (2, 8, 12, 2, 3, 2, 1)])
def test_restatement_matches_fp64_autograd(B, S, N, T, L, spc, ls):
    c = XC.Case(B, S, N, T, L, spc, ls, False)
    P, X, PE, dl, _ = XC._draw(c, 5 + S)
    t = R.head(P, X, PE, spc, T, ls, dl, XC.G_AREA)
    Q = {"slot.initial_slots": P["slots0"][None], "slot.gru.weight_ih_l0": P["w_ih"], "slot.gru.weight_hh_l0": P["w_hh"],
         "slot.gru.bias_ih_l0": P["b_ih"], "slot.gru.bias_hh_l0": P["b_hh"]}
    for l in range(L):
        Q["slot.to_k.%d.weight" % (2 * l)], Q["slot.to_k.%d.bias" % (2 * l)] = P["tok_w"][l], P["tok_b"][l]
    Q = {k: v.double().clone().requires_grad_(True) for k, v in Q.items()}
    x = X.double().clone().requires_grad_(True)
    aux = {}
    lg, _ = O.xslot_forward(Q, x + PE.double(), x, S // spc, spc, ls, 1, iters=T, aux=aux)
    ((lg * dl.double()).sum() + XC.G_AREA * aux["attn"].sum()).backward()

    def chk(a, b, name):
        torch.testing.assert_close(a, b.detach(), rtol=1e-9, atol=1e-12, msg=lambda m: name + ": " + m)
    chk(t["logits"], lg, "logits")
    chk(t["attn"], aux["attn"], "attn")
    chk(t["area_part"], aux["attn"].sum((1, 2)), "area_part")
    chk(t["K"], aux["k"], "K")
    assert len(t["states"]) == T - 1 and len(t["dgi"]) == len(t["dgh"]) == len(t["U"]) == T - 1
    for k in range(T - 1):
        chk(t["states"][k], aux["slot_states"][k + 1], "states[%d]" % k)
    chk(t["dX"], x.grad, "dX")
    g = R.param_grads(t, P["slots0"], t["H"], t["states"])
    chk(g["slots0"], Q["slot.initial_slots"].grad[0], "slots0")
    for name, key in (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0")):
        ref = Q["slot.gru." + key].grad
        chk(g[name], torch.zeros_like(g[name]) if ref is None else ref, name)            # (T = 1: the GRU is never called)
    for l in range(L):
        chk(g["tok_w%d" % l], Q["slot.to_k.%d.weight" % (2 * l)].grad, "tok_w%d" % l)
        chk(g["tok_b%d" % l], Q["slot.to_k.%d.bias" % (2 * l)].grad, "tok_b%d" % l)


def test_inputs_of_every_case_leave_the_reference_well_conditioned():
    """xslot_cases.inputs_and_truth asserts conditions (a) - (d) as it makes a case's inputs; (d) once more, in the open"""
    for c in XC.CASES:
        P, X, PE, dl, ga, t64, t32 = XC.inputs_and_truth(c)
        assert X.shape == (c.B, c.N, XC.D) and P["slots0"].shape == (c.S, XC.D) and len(P["tok_w"]) == c.L
        assert t32["dX"].dtype == torch.float32 and t64["dX"].dtype == torch.float64
        assert (ga == 0.0) == c.null_area
        A = t64["attn"]
        assert 0.0 < float(A.min()) and float(A.max()) < 1.0 and float(((A * (1 - A)) > 1e-2).double().mean()) >= 0.5, XC.case_id(c)
        for rows in (t64["dgi"], t64["dgh"], t64["dZ"], [t64["ds0"]]):
            assert all(float(x.abs().max()) >= 1e-3 for x in rows), XC.case_id(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# THE INVENTORY.  Forward: 16 tile instantiations, each in both attn store forms, and the two small kernels.
FWD = {("tile", njt, gx, tpw, form) for njt, gx in ((1, 4), (2, 8), (3, 11), (3, 12)) for tpw in (1, 2, 3, 4)
       for form in ("vec4", "scalar")} | {("small", 1), ("small", 2)}
# Backward.  Tile kernels <1>, <2>: (family, NJT, ntiles % 4, fewer than four tiles, live half tiles) -- every remainder walked
# whole (halves off, or nothing to halve: nhalf = 0) and as halves: one or two live halves of ONE leftover tile, three or four of
# TWO, each with no whole tile in front (nfull = 0) and behind whole rounds.
BWD = {("small", 1), ("small", 2)}
for njt in (1, 2):
    BWD |= {("tile", njt, 0, False, 0), ("tile", njt, 3, True, 0), ("tile", njt, 3, False, 0)}
    BWD |= {("tile", njt, rem, few, 0) for rem in (1, 2) for few in (True, False)}
    BWD |= {("tile", njt, 1, few, nh) for few in (True, False) for nh in (1, 2)}
    BWD |= {("tile", njt, 2, few, nh) for few in (True, False) for nh in (3, 4)}
# <3, true> and the scratch kernel: every remainder, with fewer than four tiles (waves that own none) and with four or more
for fam in ("tile_wg", "scratch"):
    BWD |= {(fam, 3, 0, False, 0)} | {(fam, 3, rem, few, 0) for rem in (1, 2, 3) for few in (True, False)}
# Shapes the issue of this file names, beyond the instances: every one must be some case's
SHAPES = ({("N", n) for n in (1, 20, 32, 33, 49, 64, 65, 81, 88, 89, 96)} |
          {("S", s, njt) for s in (16, 17, 33, 128, 129, 256, 257, 384, 385, 512) for njt in (1, 2, 3)} | {("S,N", 300, 81)} |
          {("T = 1", njt) for njt in (1, 2, 3)} |
          {("one live slot in the last tile, ntiles % 4 =", r) for r in (0, 1, 2, 3)} |
          {("T", t) for t in (1, 2, 3, 8)} | {("L", l) for l in (1, 2, 3, 8)} | {("spc", k) for k in (1, 2, 3)} |
          {("B", b) for b in (1, 2, 3)} | {("loss_status", s) for s in (1, -1)} |
          {("null g_area_sum", fam) for fam in ("tile", "tile_wg", "scratch", "small")})


def _reached(kk, cases):
    fwd, bwd, shapes = set(), set(), set()
    for c in cases:
        shapes |= {("N", c.N), ("S", c.S, (c.N + 31) // 32), ("S,N", c.S, c.N), ("T", c.T), ("L", c.L), ("spc", c.spc),
                   ("B", c.B), ("loss_status", c.ls)}
        if c.T == 1:
            shapes.add(("T = 1", (c.N + 31) // 32))
        if c.S % 32 == 1:
            shapes.add(("one live slot in the last tile, ntiles % 4 =", ((c.S + 31) // 32) % 4))
        for _, sw in XC.variants(c):
            with kk.switches(**sw):
                fwd |= XC.fwd_keys(kk, c)
                b = XC.bwd_key(kk, c)
            bwd.add(b)
            if c.null_area:
                shapes.add(("null g_area_sum", b[0]))
    return fwd, bwd, shapes & SHAPES


def test_the_case_table_reaches_every_instance_and_no_case_is_idle(kk):
    assert len(FWD) == 34 and len(BWD) == 2 + 2 * 15 + 2 * 7
    fwd, bwd, shapes = _reached(kk, XC.CASES)
    assert fwd == FWD, ("without a case: %s; not in the inventory: %s" % (sorted(FWD - fwd), sorted(fwd - FWD)))
    assert bwd == BWD, ("without a case: %s; not in the inventory: %s" % (sorted(BWD - bwd), sorted(bwd - BWD)))
    assert shapes == SHAPES, sorted(SHAPES - shapes, key=str)
    assert len(set(XC.CASES)) == len(XC.CASES)
    for k, c in enumerate(XC.CASES):              # take any one case out: something above is lost
        assert _reached(kk, XC.CASES[:k] + XC.CASES[k + 1:]) != (fwd, bwd, shapes), "idle case " + XC.case_id(c)


def test_every_boundary_of_the_rule(kk):
    q = kk.xslot_instance
    # refusals: one past every limit, and sizes no head has
    assert q(96, 512, 8, 8) is not None
    for bad in ((97, 512, 8, 8), (96, 513, 8, 8), (96, 512, 9, 8), (96, 512, 8, 9), (0, 5, 3, 1), (5, 0, 3, 1), (5, 5, 0, 1),
                (5, 5, 3, 0), (-1, 5, 3, 1)):
        assert q(*bad) is None, bad
    # N: token tiles, the GX = 11 window, the backward family
    for n, njt, gx, fam in ((32, 1, 4, "tile"), (33, 2, 8, "tile"), (64, 2, 8, "tile"), (65, 3, 11, "tile_wg"),
                            (88, 3, 11, "tile_wg"), (89, 3, 12, "tile_wg"), (96, 3, 12, "tile_wg")):
        i = q(n, 100)
        assert (i["NJT"], i["GX"], i["bwd"], i["small"]) == (njt, gx, fam, 0), n
    with kk.switches(xslot_bwd_scratch=1):
        assert [q(n, 100)["bwd"] for n in (64, 65, 96)] == ["tile", "scratch", "scratch"]
        assert q(65, 100)["bwd_lds_bytes"] != q(64, 100)["bwd_lds_bytes"]
    # S: slot tiles per wave of the forward
    for s, tpw in ((17, 1), (128, 1), (129, 2), (256, 2), (257, 3), (384, 3), (385, 4), (512, 4)):
        assert q(49, s)["TPW"] == tpw and q(49, s)["ntiles"] == (s + 31) // 32, s
    # S = 16 / 17 under both values of xslot_small; the small kernels' token width at N = 64 / 65
    for on in (1, 0):
        with kk.switches(xslot_small=on):
            assert [q(49, s)["small"] for s in (1, 16, 17)] == [on, on, 0]
            assert [q(n, 10)["NJT"] for n in (64, 65)] == ([1, 2] if on else [2, 3])
            assert q(49, 16)["bwd"] == ("small" if on else "tile") and q(81, 16)["bwd"] == ("small" if on else "tile_wg")
    # the backward's walk: halves for one or two leftover tiles of the <1>, <2> kernels only
    for s, nfull, nhalf in ((16, 0, 1), (17, 0, 2), (32, 0, 2), (33, 0, 3), (48, 0, 3), (49, 0, 4), (64, 0, 4), (65, 3, 0),
                            (128, 4, 0), (129, 4, 1), (144, 4, 1), (145, 4, 2), (161, 4, 3), (177, 4, 4), (193, 7, 0),
                            (300, 8, 3), (512, 16, 0)):
        with kk.switches(xslot_small=0):
            i, w = q(64, s), q(65, s)
            assert (i["nfull"], i["nhalf"]) == (nfull, nhalf), s
            assert (w["nfull"], w["nhalf"]) == ((s + 31) // 32, 0), s
            with kk.switches(xslot_bwd_halves=0):
                assert (q(64, s)["nfull"], q(64, s)["nhalf"]) == ((s + 31) // 32, 0), s
    # the attn store form: S * N a multiple of four AND an aligned pointer
    assert q(20, 17, 3, 1, True)["attn_vec4"] == 1 and q(20, 17, 3, 1, False)["attn_vec4"] == 0
    assert q(33, 17, 3, 1, True)["attn_vec4"] == 0 and q(33, 34, 3, 1, True)["attn_vec4"] == 0 and q(33, 68)["attn_vec4"] == 1
    # the forward shares its leftover tiles between wave pairs -- three token tiles only when there are state rows to share through
    assert [q(49, s, 1)["share"] for s in (32, 64, 96, 128, 160)] == [1, 1, 0, 0, 1]
    assert q(81, 40, 1)["share"] == 0 and q(81, 40, 2)["share"] == 1


def test_workspace_covers_what_the_selected_instance_addresses(kk):
    """per image, from the kernels' comments -- tile kernels: ds' hand-off [Sp][64] floats, behind ALL images' hand-offs the parks:
    four waves x (4 NJT accumulator tiles x 4 quads x 64 lanes) float4;  scratch kernel: dsn [Sp][64] | per iteration A [Sp][NP],
    dD [Sp][NP], dU [Sp][64];  small kernels: parks of four waves x (NTW x 2 x 4 x 64) float4 for the wide form only."""
    from scouter_amd import _native
    ws = _native.lib().scouter_xslot_bwd_workspace_bytes
    for c in XC.CASES:
        for _, sw in XC.variants(c):
            with kk.switches(**sw):
                i = kk.xslot_instance(c.N, c.S, c.T, c.L)
                have = ws(c.B, c.N, XC.D, c.S, c.T)
            Sp, NP = 32 * i["ntiles"], 32 * i["NJT"]
            if i["bwd"] in ("tile", "tile_wg"):
                need = 4 * c.B * (Sp * 64 + 4 * (4 * i["NJT"] * 4 * 64) * 4)
            elif i["bwd"] == "scratch":
                need = 4 * c.B * Sp * (64 + c.T * (2 * NP + 64))
            else:
                need = 0 if i["NJT"] == 1 else 16 * c.B * 4 * (i["NJT"] * 2 * 4 * 64)
            assert have >= need, (XC.case_id(c), sw, have, need)
            assert 0 < i["bwd_lds_bytes"] <= 160 * 1024


def test_both_entry_points_launch_through_the_rule():
    """the launchers take NJT / TPW / the family -- and their limits -- from xs_instance (what they then launch is checked on the
    GPU, where tests/test_xslot_instances_gpu.py keys every comparison by the query's answer)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scouter_amd", "csrc")
    for name, entry in (("xslot_fwd.hip", "scouter_xslot_fwd_f32"), ("xslot_bwd.hip", "scouter_xslot_bwd_f32")):
        text = open(os.path.join(csrc, name)).read()
        assert "xs_instance(" in text[text.index('extern "C" int ' + entry):], name
