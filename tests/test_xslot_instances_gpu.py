"""Every kernel instance of the fused xSlot head (csrc/xslot_fwd.hip, xslot_bwd.hip, xslot_small_*.h) against fp64, ROW BY ROW.

The cases are tests/xslot_cases.py (tests/test_xslot_instances_cpu.py proves that they reach every instance); the truth is the fp64
restatement tests/xslot_restatements.py.  The C ABI is called directly; every output buffer lies between sentinel guard rows and is
filled with NaN before the launch, so a row written outside [0, S) x [0, N) and a row NOT written both show.  Per case and per
switch setting that selects another instance for the same shape:
  forward   logits, attn, area_part, K, every H[l], every states[t] element-wise against fp64 -- with the attention map stored
            through both store forms (the pointer offset by one float forces the scalar one), bit-equal;
  backward  fed the kernel forward's own saved tensors: dX, ds0, every dZ[l], dgi[t], dgh[t], U[t] element-wise, then the weight and
            bias gradients sloter/utils/slot_attention.py forms from them (all of the GRU's and every to_k layer's);
  guards intact, every output finite, a second launch bit-equal, the instances of a shape agree with each other to rounding.
Bound per tensor (each t / l on its own), the project's yardstick for this head (tests/test_xslot_gpu.py) applied to every element:
  |HIP - fp64| <= 3e-3 max|fp64| + 3 max|fp32 restatement - fp64| + 1e-6;   logits, attn: max(1e-4, 3 x the logits' fp32 spread)."""
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import xslot_cases as XC                                                    # noqa: E402
import xslot_restatements as R                                              # noqa: E402

SENT, GUARD = 31337.0, 1024                  # sentinel value, guard floats on either side (>= 4 rows of the widest output, 3d)
AGREE_REL, AGREE_ABS = 2e-4, 1e-7            # two instances of one shape: tests/test_xslot_gpu.py, half tiles vs whole tiles
T0 = time.time()
WORST = {}                                   # kernel family -> (err / bound, tensor, case)
D = XC.D


@pytest.fixture(scope="module", autouse=True)
def report():
    """after the last test of this file that ran: the worst err / bound per kernel family among them, and the file's time"""
    yield
    for fam in sorted(WORST):
        print("\nworst err/bound  %-22s %.2e  (%s, %s)" % ((fam,) + WORST[fam]), end="")
    print("\ntests/test_xslot_instances_gpu.py: %.1f s in all" % (time.time() - T0))


class Buf:
    """an output of `shape` between guards; off: floats the payload is shifted by (1: not 16-byte aligned)"""

    def __init__(self, shape, off=0):
        n = 1
        for s in shape:
            n *= s
        self.raw = torch.full((GUARD + off + n + GUARD,), SENT, device="cuda")
        self.lo, self.n = GUARD + off, n
        self.t = self.raw[self.lo:self.lo + n].view(shape)
        self.t.fill_(float("nan"))
        assert (self.raw.data_ptr() & 15) == 0

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all())


def _p(b):
    return None if b is None else b.ptr()


def _lib():
    from scouter_amd import _native
    return _native, _native.lib()


def _upload(c):
    P, X, PE, dl, ga, t64, t32 = XC.inputs_and_truth(c)
    cu = lambda t: t.float().contiguous().cuda()
    dev = dict(X=cu(X), PE=cu(PE), dl=cu(dl), slots0=cu(P["slots0"]), w_ih=cu(P["w_ih"]), w_hh=cu(P["w_hh"]), b_ih=cu(P["b_ih"]),
               b_hh=cu(P["b_hh"]), tok_w=[cu(w) for w in P["tok_w"]], tok_b=[cu(b) for b in P["tok_b"]],
               ga=None if c.null_area else torch.full((1,), ga, device="cuda"))
    dev["tw_ptr"] = (ctypes.c_void_p * c.L)(*[w.data_ptr() for w in dev["tok_w"]])
    dev["tb_ptr"] = (ctypes.c_void_p * c.L)(*[b.data_ptr() for b in dev["tok_b"]])
    return dev


def launch_fwd(c, dev, attn_off=0):
    native, lib = _lib()
    C = c.S // c.spc
    o = dict(logits=Buf((c.B, C)), attn=Buf((c.B, c.S, c.N), attn_off), area_part=Buf((c.B,)), K=Buf((c.B, c.N, D)),
             H=Buf((c.L, c.B, c.N, D)), states=Buf((c.T - 1, c.B, c.S, D)) if c.T > 1 else None)
    native.check(lib.scouter_xslot_fwd_f32(
        dev["X"].data_ptr(), dev["PE"].data_ptr(), dev["tw_ptr"], dev["tb_ptr"], dev["slots0"].data_ptr(), dev["w_ih"].data_ptr(),
        dev["w_hh"].data_ptr(), dev["b_ih"].data_ptr(), dev["b_hh"].data_ptr(), c.B, c.N, D, c.S, c.spc, c.T, c.L, float(c.ls),
        _p(o["logits"]), _p(o["attn"]), _p(o["area_part"]), _p(o["K"]), _p(o["H"]), _p(o["states"]), None), "xslot_fwd")
    torch.cuda.synchronize()
    return o


def launch_bwd(c, dev, fwd):
    native, lib = _lib()
    nbytes = lib.scouter_xslot_bwd_workspace_bytes(c.B, c.N, D, c.S, c.T)
    gru = c.T > 1
    o = dict(dX=Buf((c.B, c.N, D)), ds0=Buf((c.B, c.S, D)), dZ=Buf((c.L, c.B, c.N, D)),
             dgi=Buf((c.T - 1, c.B, c.S, 3 * D)) if gru else None, dgh=Buf((c.T - 1, c.B, c.S, 3 * D)) if gru else None,
             U=Buf((c.T - 1, c.B, c.S, D)) if gru else None, ws=Buf(((nbytes + 3) // 4 + 4,)))
    native.check(lib.scouter_xslot_bwd_f32(
        dev["X"].data_ptr(), dev["PE"].data_ptr(), dev["tw_ptr"], dev["slots0"].data_ptr(), dev["w_ih"].data_ptr(),
        dev["w_hh"].data_ptr(), dev["b_ih"].data_ptr(), dev["b_hh"].data_ptr(), _p(fwd["K"]), _p(fwd["H"]), _p(fwd["states"]),
        dev["dl"].data_ptr(), None if dev["ga"] is None else dev["ga"].data_ptr(), c.B, c.N, D, c.S, c.spc, c.T, c.L, float(c.ls),
        _p(o["dX"]), _p(o["dgi"]), _p(o["dgh"]), _p(o["U"]), _p(o["ds0"]), _p(o["dZ"]), _p(o["ws"]), nbytes, None), "xslot_bwd")
    torch.cuda.synchronize()
    return o


def _same_bits(a, b, what, fails):
    for k in a:
        if a[k] is not None and k != "ws" and not torch.equal(a[k].t, b[k].t):
            fails.append("%s: %s differs between two launches / store forms" % (what, k))


def _guards(o, what, fails):
    for k, b in o.items():
        if b is not None and not b.intact():
            fails.append("%s: guard rows of %s overwritten" % (what, k))
        if b is not None and k != "ws" and not bool(torch.isfinite(b.t).all()):
            fails.append("%s: %s not finite (a row that was not written, or a NaN)" % (what, k))


class Judge:
    def __init__(self, c, vname, fails):
        self.c, self.vname, self.fails = c, vname, fails

    def __call__(self, family, name, got, ref, ref32, floor_tol=None):
        got, ref = got.double().cpu(), ref.double()
        bound = floor_tol if floor_tol is not None else \
            3e-3 * float(ref.abs().max()) + 3 * float((ref32.double() - ref).abs().max()) + 1e-6
        err = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
        ratio = err / bound
        print("%-34s %-8s %-20s %-9s err/bound %.2e" % (XC.case_id(self.c), self.vname, family, name, ratio))
        if ratio > WORST.get(family, (0.0,))[0]:
            WORST[family] = (ratio, name, XC.case_id(self.c) + "/" + self.vname)
        if not err <= bound:
            worst = int((got - ref).abs().flatten().nan_to_num(float("inf")).argmax())
            self.fails.append("%s %s: |HIP - fp64| = %.3g > %.3g at flat index %d of %s" % (family, name, err, bound, worst,
                                                                                      tuple(got.shape)))


def _rows(o, c):
    """kernel outputs as the lists the restatement returns"""
    r = dict(dX=o["dX"].t.cpu(), ds0=o["ds0"].t.cpu(), dZ=list(o["dZ"].t.cpu()))
    for k in ("dgi", "dgh", "U"):
        r[k] = [] if o[k] is None else list(o[k].t.cpu())
    return r


@pytest.mark.parametrize("c", XC.CASES, ids=XC.case_id)
def test_every_instance_of_a_shape_matches_fp64_row_by_row(c):
    from scouter_amd import kernels as kk
    P, X, PE, dl, ga, t64, t32 = XC.inputs_and_truth(c)
    dev = _upload(c)
    fails, kept = [], {}
    g64 = R.param_grads(t64, P["slots0"], t64["H"], t64["states"])
    g32 = R.param_grads(t32, P["slots0"], t32["H"], t32["states"])
    logit_tol = max(1e-4, 3 * float((t32["logits"].double() - t64["logits"]).abs().max()))
    for vname, sw in XC.variants(c):
        with kk.switches(**sw):
            inst = kk.xslot_instance(c.N, c.S, c.T, c.L)
            ffam = "fwd small<%d>" % inst["NJT"] if inst["small"] else "fwd tile<%d,TPW,%d>" % (inst["NJT"], inst["GX"])
            bfam = "bwd " + inst["bwd"] + ("<%d>" % inst["NJT"] if inst["bwd"] in ("tile", "small") else "")
            what = XC.case_id(c) + "/" + vname
            judge = Judge(c, vname, fails)
            # ---- forward: aligned attn (the 16-byte store form where S * N allows it), again (same bits), then attn off by one float
            f = launch_fwd(c, dev)
            _guards(f, what + " fwd", fails)
            _same_bits(f, launch_fwd(c, dev), what + " fwd", fails)
            if not inst["small"] and inst["attn_vec4"]:
                assert kk.xslot_instance(c.N, c.S, c.T, c.L, False)["attn_vec4"] == 0
                f1 = launch_fwd(c, dev, attn_off=1)
                assert f1["attn"].ptr() & 15
                _guards(f1, what + " fwd, attn not 16-byte aligned", fails)
                _same_bits(f, f1, what + " fwd, scalar attn stores", fails)
            judge(ffam, "logits", f["logits"].t, t64["logits"], None, logit_tol)
            judge(ffam, "attn", f["attn"].t, t64["attn"], None, logit_tol)
            if not (float(f["attn"].t.min()) > 0.0 and float(f["attn"].t.max()) < 1.0):       # (the truth is: condition (d))
                fails.append(what + ": attn not strictly inside (0, 1)")
            for name in ("area_part", "K"):
                judge(ffam, name, f[name].t, t64[name], t32[name])
            for l in range(c.L):
                judge(ffam, "H[%d]" % l, f["H"].t[l], t64["H"][l], t32["H"][l])
            for t in range(c.T - 1):
                judge(ffam, "states[%d]" % t, f["states"].t[t], t64["states"][t], t32["states"][t])
            # ---- backward from the kernel forward's own saved tensors
            b = launch_bwd(c, dev, f)
            _guards(b, what + " bwd", fails)
            _same_bits(b, launch_bwd(c, dev, f), what + " bwd", fails)
            _guards(f, what + " fwd buffers after the backward", fails)
            rows = _rows(b, c)
            judge(bfam, "dX", rows["dX"], t64["dX"], t32["dX"])
            judge(bfam, "ds0", rows["ds0"], t64["ds0"], t32["ds0"])
            for l in range(c.L):
                judge(bfam, "dZ[%d]" % l, rows["dZ"][l], t64["dZ"][l], t32["dZ"][l])
            for t in range(c.T - 1):
                for name in ("dgi", "dgh", "U"):
                    judge(bfam, "%s[%d]" % (name, t), rows[name][t], t64[name][t], t32[name][t])
            g = R.param_grads(rows, P["slots0"], list(f["H"].t.cpu()), [] if f["states"] is None else list(f["states"].t.cpu()))
            for name in g64:
                judge(bfam, "d " + name, g[name], g64[name], g32[name])
            kept[vname] = {k: v.t.double().cpu() for k, v in list(f.items()) + list(b.items()) if v is not None and k != "ws"}
    # ---- the instances of this shape agree with each other to rounding
    for vname in list(kept)[1:]:
        for k, a in kept[vname].items():
            ref = kept["default"][k]
            if not float((a - ref).abs().max()) <= AGREE_REL * float(ref.abs().max()) + AGREE_ABS:
                fails.append("%s: %s of `%s` and of the default instance differ by %.3g (max |ref| %.3g)"
                             % (XC.case_id(c), k, vname, float((a - ref).abs().max()), float(ref.abs().max())))
    assert not fails, "\n".join(fails)


