"""The case table of the head-instance tests (tests/test_xslot_instances_cpu.py counts the kernel instances it reaches,
tests/test_xslot_instances_gpu.py launches them) and the seeded inputs of a case with their fp64 truth.

A case is the SMALLEST shape that reaches its instance: N picks the token-tile count NJT (and GX = 11 for 65 <= N <= 88), S the slot
tiles per wave of the forward and the backward's walk -- ceil(S / 32) % 4 leftover tiles, walked whole or as 16-slot halves
(`xslot_bwd_halves`), with S = 32 k + 1 or 32 k + 17 leaving ONE live slot in the last (half) tile.  Test infrastructure only."""
import collections
import functools

import torch

from oracle import torch_oracle as O

import xslot_restatements as R

D = 64
Case = collections.namedtuple("Case", "B S N T L spc ls null_area")


def _c(B, S, N, T=2, L=1, spc=1, ls=1, null_area=False):
    return Case(B, S, N, T, L, spc, ls, null_area)


CASES = [
    # ---- one token tile (N <= 32): xslot_fwd_kernel<1, TPW>, xslot_bwd_kernel<1>
    _c(2, 16, 1, T=3),                      # S <= 16: the small kernels, or (xslot_small = 0) ONE half tile, nfull = 0
    _c(3, 17, 20, T=1),                     # one live slot in the second half tile; a single iteration: no GRU buffers at all
    _c(3, 33, 32, T=3, spc=3),              # three halves, the third with one live slot
    _c(1, 64, 20, L=2, ls=-1),              # four halves, no whole tile
    _c(2, 65, 32, null_area=True),          # ntiles % 4 = 3: whole tiles only, wave 3 owns none; last tile one live slot
    _c(1, 97, 20),                          # four tiles, the fourth with one live slot
    _c(1, 128, 20, T=3),                    # TPW 1 at its upper edge, ntiles % 4 = 0
    _c(2, 129, 32),                         # TPW 2 at its lower edge: 4 tiles + one half with one live slot
    _c(1, 145, 20, L=3),                    # 4 tiles + two halves, the second with one live slot
    _c(1, 161, 20, spc=7),                  # 4 tiles + three halves
    _c(1, 192, 32, T=3, spc=2),             # 4 tiles + four halves
    _c(1, 193, 20),                         # 7 tiles: ntiles % 4 = 3 behind whole rounds
    _c(1, 256, 32, ls=-1),                  # TPW 2 at its upper edge
    _c(1, 257, 20),                         # TPW 3 at its lower edge
    _c(1, 384, 32, spc=3),                  # TPW 3 at its upper edge
    _c(1, 385, 20, spc=5),                  # TPW 4 at its lower edge
    _c(1, 512, 32, T=3, spc=2),             # TPW 4, S at the limit
    # ---- two token tiles (33 <= N <= 64): xslot_fwd_kernel<2, TPW>, xslot_bwd_kernel<2>
    _c(2, 16, 33, T=3, L=2, null_area=True),
    _c(3, 17, 49, T=1, null_area=True),
    _c(2, 33, 64, T=3, spc=3, ls=-1),
    _c(1, 64, 49, L=3),
    _c(2, 65, 33),
    _c(1, 128, 64, T=3, spc=2),
    _c(1, 129, 49, null_area=True),
    _c(1, 145, 33),
    _c(1, 161, 64),
    _c(1, 192, 49, T=3),
    _c(1, 193, 33),
    _c(1, 256, 49),
    _c(1, 257, 64),
    _c(1, 384, 33, spc=2),
    _c(1, 385, 49),
    _c(2, 512, 64, T=8, L=2),               # S, T at the limits
    # ---- three token tiles (65 <= N <= 96): xslot_fwd_kernel<3, TPW, 11 | 12>, xslot_bwd_kernel<3, true> | scratch
    _c(2, 16, 81, T=3),                     # the small kernels' second token width
    _c(2, 17, 88, T=3),                     # one tile, waves 1..3 own none; N = 88: the last token of the GX = 11 form
    _c(2, 33, 65, T=3, null_area=True),     # two tiles, the second with one live slot; N = 65: the first token of the third tile
    _c(3, 40, 81, T=1, spc=2),              # a single iteration: the leftover tiles are NOT shared (no state rows to exchange through)
    _c(2, 65, 96, L=2),                     # three tiles (ntiles % 4 = 3, fewer than four)
    _c(1, 128, 89, T=3),                    # N = 89: the first shape of the full contraction; four tiles
    _c(1, 129, 96, ls=-1),                  # 5 tiles: ntiles % 4 = 1 behind a whole round
    _c(1, 256, 88),                         # 8 tiles
    _c(1, 257, 89),                         # 9 tiles: TPW 3 at its lower edge
    _c(2, 300, 81, T=3, L=3, spc=3),        # the reference's 260 x 260 input at 100 classes x 3: 10 tiles
    _c(1, 321, 96, L=8),                    # 11 tiles; L at the limit
    _c(1, 384, 81, spc=3),                  # 12 tiles: TPW 3 at its upper edge
    _c(1, 385, 88, spc=5),                  # 13 tiles
    _c(1, 512, 96, T=8, L=2, spc=2),        # S, N, T at the limits
]


def case_id(c):
    return "B%d-S%d-N%d-T%d-L%d-spc%d-ls%d%s" % (c.B, c.S, c.N, c.T, c.L, c.spc, c.ls, "-noarea" if c.null_area else "")


# ---- the conditions the inputs of a case must leave the reference in (asserted where the inputs are made)
DX_FP32_DEVIATION = 2e-4      # (a) fp32 autograd's own deviation of dX, relative to max |dX|
PREACT_MARGIN = 1e-4          # (b) no to_k pre-activation in front of a ReLU closer to zero: the mask is the same in fp32 and fp64
ROWSUM_MARGIN = 1e-2          # (c) no |r_i| below this fraction of the mean |r_i| of its image and iteration
# (d) the case says something: the sigmoid works in its active range and every row the backward emits carries a value
ACTIVE_SHARE = 0.5            #     share of the last attention map with A (1 - A) > ACTIVE_SLOPE, in every image
ACTIVE_SLOPE = 1e-2
ROW_FLOOR = 1e-3              #     max |dgi[t]|, |dgh[t]|, |ds0|, |dZ[l]|: a thousand times the bound's absolute term 1e-6
SLOT_SPREAD = 3e-4            #     U[t] and the last attention map differ between slots (N > 1): spread over slots / max |.|
                              #     (eight GRU iterations draw the slots of an image together: 5e-4 is what T = 8 leaves)
G_AREA = 0.01
TO_K_WEIGHT = {3: 0.12, 8: 0.15}     # scale of the to_k weights by depth; every other depth: 0.1


def _draw(c, seed):
    """The input recipe of tests/test_xslot_gpu.py (its limits test): slots |randn| / 2, GRU weights and every bias randn / 10, to_k
    weights randn / 10, tokens relu(randn), PE 0.3 randn, dlogits randn.  What differs, and why:
      1. the last to_k bias is shifted by +0.25 and that layer (weight and bias) is then scaled by one factor so that
         max_b |tau| / N = 1 in the first iteration.  The pre-sigmoid logits D / r_i * tau are homogeneous of degree one in K, so
         this puts them at O(1) whatever S -- as they come (tau ~ S) every sigmoid of a many-slot head saturates, the attention is
         a map of ones and all gradients through it vanish: condition (d).  The shift keeps K's column sums of one sign;
      2. the input bias of the GRU's candidate gate is shifted by +0.6, so that the slot states of the later iterations keep the
         sign of the initial slots: with 1. the row sums r_i = s_i . colsum(K) / 8 then stay away from zero, condition (c);
      3. to_k weights of 0.12 at L = 3 and 0.15 at L = 8, where that recipe has 0.2: at 0.2 the spread of K is wider than the
         shift of 1. and (c) fails; at L = 8 also (a);
      4. dlogits are 4 randn: the gate gradients of the first of eight iterations then stay a thousand times above the bound's
         absolute term (d)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)
    wk = TO_K_WEIGHT.get(c.L, 0.1)
    P = dict(slots0=r(c.S, D).abs() * 0.5, w_ih=r(3 * D, D) * 0.1, w_hh=r(3 * D, D) * 0.1, b_ih=r(3 * D) * 0.1,
             b_hh=r(3 * D) * 0.1, tok_w=[r(D, D) * wk for _ in range(c.L)], tok_b=[r(D) * 0.1 for _ in range(c.L)])
    X, PE = r(c.B, c.N, D).relu(), r(c.N, D) * 0.3
    dl = r(c.B, c.S // c.spc) * 4.0
    P["tok_b"][-1] += 0.25
    P["b_ih"][2 * D:] += 0.6
    tau = R.head(P, X, PE, c.spc, 1, c.ls, dl, 0.0)["r"][0].sum(1).abs().max()
    gain = (c.N / tau).float()
    P["tok_w"][-1] *= gain
    P["tok_b"][-1] *= gain
    return P, X, PE, dl, g


def _says_something(c, t64):
    """condition (d); None or what fails"""
    A = t64["attn"]
    if float(((A * (1 - A)) > ACTIVE_SLOPE).double().mean((1, 2)).min()) < ACTIVE_SHARE:
        return "d: saturated attention"
    if not (float(A.min()) > 0.0 and float(A.max()) < 1.0):
        return "d: attention at 0 or 1"
    for name in ("dgi", "dgh", "dZ"):
        for x in t64[name]:
            if float(x.abs().max()) < ROW_FLOOR:
                return "d: " + name + " at the bound's floor"
    if float(t64["ds0"].abs().max()) < ROW_FLOOR:
        return "d: ds0 at the bound's floor"
    if c.N > 1:
        for x in t64["U"] + [A]:
            if float(x.std(1).max()) < SLOT_SPREAD * float(x.abs().max()):
                return "d: the same row for every slot"
    return None


def _conditions(c, P, X, PE, dl, t64):
    """None if (a), (b), (c), (d) hold, else what fails"""
    fail = _says_something(c, t64)
    if fail:
        return fail
    for z in t64["Z"][:-1]:
        if float(z.abs().min()) < PREACT_MARGIN:
            return "b"
    for r in t64["r"]:
        if float((r.abs() / r.abs().mean(1, keepdim=True)).min()) < ROWSUM_MARGIN:
            return "c"
    gx = {}
    for dt in (torch.float64, torch.float32):
        Q = {"slot.initial_slots": P["slots0"][None], "slot.gru.weight_ih_l0": P["w_ih"], "slot.gru.weight_hh_l0": P["w_hh"],
             "slot.gru.bias_ih_l0": P["b_ih"], "slot.gru.bias_hh_l0": P["b_hh"]}
        for l in range(c.L):
            Q["slot.to_k.%d.weight" % (2 * l)], Q["slot.to_k.%d.bias" % (2 * l)] = P["tok_w"][l], P["tok_b"][l]
        Q = {k: v.to(dt) for k, v in Q.items()}
        x = X.to(dt).clone().requires_grad_(True)
        aux = {}
        lg, _ = O.xslot_forward(Q, x + PE.to(dt), x, c.S // c.spc, c.spc, c.ls, 1, iters=c.T, aux=aux)
        ((lg * dl.to(dt)).sum() + (0.0 if c.null_area else G_AREA) * aux["attn"].sum()).backward()
        gx[dt] = x.grad.double()
    if float((gx[torch.float32] - gx[torch.float64]).abs().max()) > DX_FP32_DEVIATION * float(gx[torch.float64].abs().max()):
        return "a"
    return None


@functools.lru_cache(maxsize=None)
def inputs_and_truth(c):
    """(P, X, PE, dlogits, g_area, truth64, truth32): seeded fp32 inputs of case c inside conditions (a) - (d) -- a case is re-seeded
    until they hold, and a token with a pre-activation at the ReLU's edge is redrawn on its own -- with the restatement at fp64
    (the truth) and at fp32 (the yardstick of the bounds).  Computed once per case; callers must not modify what they get."""
    ga = 0.0 if c.null_area else G_AREA
    why = []
    for attempt in range(12):
        P, X, PE, dl, g = _draw(c, 1000 * c.S + 10 * c.N + c.T + 100003 * attempt)
        for _ in range(50):                         # (b), token by token
            t64 = R.head(P, X, PE, c.spc, c.T, c.ls, dl, ga)
            bad = torch.zeros(c.B, c.N, dtype=torch.bool)
            for z in t64["Z"][:-1]:
                bad |= (z.abs() < PREACT_MARGIN).any(2)
            if not bool(bad.any()):
                break
            X[bad] = torch.randn(int(bad.sum()), D, generator=g).relu()
        fail = _conditions(c, P, X, PE, dl, t64)
        if fail is None:
            return P, X, PE, dl, ga, t64, R.head(P, X, PE, c.spc, c.T, c.ls, dl, ga, torch.float32)
        why.append(fail)
    raise AssertionError("case %s: no seed leaves the reference inside conditions (a)-(d): %s" % (case_id(c), why))


# ---- which instances a case reaches (asked of the library: scouter_amd.kernels.xslot_instance)
def fwd_keys(kk, c):
    """the forward instances of case c under the current switches: one per attn store form the shape allows"""
    keys = set()
    for aligned in (True, False):
        i = kk.xslot_instance(c.N, c.S, c.T, c.L, aligned)
        keys.add(("small", i["NJT"]) if i["small"] else ("tile", i["NJT"], i["GX"], i["TPW"], "vec4" if i["attn_vec4"] else "scalar"))
    return keys


def bwd_key(kk, c):
    """the backward instance of case c under the current switches.  Tile kernels: (family, NJT, ntiles % 4, fewer than four tiles --
    waves that own none --, live half tiles)"""
    i = kk.xslot_instance(c.N, c.S, c.T, c.L)
    if i["bwd"] == "small":
        return ("small", i["NJT"])
    return (i["bwd"], i["NJT"], i["ntiles"] % 4, i["ntiles"] < 4, i["nhalf"])


def variants(c):
    """the switch settings under which case c takes DIFFERENT instances: [(name, {switch: value})], the default first"""
    v = [("default", {})]
    if c.S <= 16:
        v.append(("tiles", {"xslot_small": 0}))
    if c.N <= 64 and ((c.S + 31) // 32) % 4 in (1, 2):
        v.append(("whole", dict(xslot_bwd_halves=0, xslot_small=0)))
    if c.N > 64:
        v.append(("scratch", dict(xslot_bwd_scratch=1, xslot_small=0)))
    return v
