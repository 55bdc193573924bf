"""BatchNorm, split-attention and column-sum routes of csrc/bn_elem.hip on both sides of every switch, against fp64 (-m gpu).

Each entry point picks its kernels, grid and reduction geometry from M (rows = B*H*W) and C.  The library's profile label
names the route a call took, "<prefix><source,geometry,finalize,apply pass,loop>", and every test asserts the label its
shape must produce (the Python mirror of the rules below, _route_*).  The rules and the shapes on both sides:

  rule (csrc/bn_elem.hip)   condition                                             below / above
  ------------------------  ----------------------------------------------------  ------------------------------------------
  col_geom                  C/4 <= 256 && 256 % (C/4) == 0: whole-row slab         C = 1024 "row" / 2048 "slab"; 96 "slab"
                            (1024/C rows per pass), else 1024-channel slabs          (24 live lanes)
  col_blocks                nb = min(1024, ceil(M / (8 rpb))): "-cap" = the         C = 64: M = 131072 / 131073;
                            blocks loop over rows, ragged last pass                  C = 2048: M = 8192 / 12544
  fin_narrow                C <= 64 && nparts > 512 -> finalize<1> "fin1", else     C = 64: M = 65536 / 65537; C = 32 / 128 at
                            <4> "fin4" (nparts = nb or the producer's rows)          the stem's 70 x 112^2
  bn_bwd_small_kernel       fp32 io, no ext, M <= 24 rpb: "small"; 16-channel       C = 256: M = 96 / 97; C = 128: 192 / 193;
                            slabs "slab16" iff C % 16 == 0 && C >= 32                C = 20 (slab), 16 (row)
  ew_blocks                 <= 2048 workgroups: "loop" once n > grid * 256          C = 256: M = 8192 / 8193
  ew_blocks_hoist           256 % (C/4) == 0 "hoist"; (C/4) % 256 == 0              C = 256 / 96 "stride"; 2048 and 3072
                            "hoist-wide" (grid rounded to a multiple of C/1024);    (3072: the rounding changes the grid)
                            else "stride"
  bf16x8 passes             all-bf16 io, C % 8 == 0: "bf16x8h" iff 256 % (C/8)      C = 2048 / 96, 192
                            == 0, else "bf16x8"
  colsum                    M <= 12 rpb || M <= 256: "direct", else "partial,fin4"  C = 64 and 2048: M = 256 / 257
  sa_bn_bwd                 sums (from sa_dattn(want_stats)) / reduction pass;      C' = 512 (bf16x8h) / 96 (bf16x8), sums /
                            bf16x8 with one bf16 plane; hoisted or not               partial

PRODUCTION lists every distinct (entry point, shape, storage, flags) of one training step of BASELINE configs 2, 4 and 5.

References are float64 torch on the GPU, every element: batch mean, biased variance and the affine map written out and
differentiated by autograd, the running statistics with momentum and the unbiased variance.  The ReLU sign the backward uses
is the kernel's own (its mask bits / stored activation / bn_apply): the sums, not the sign decisions, are what is checked.
Bounds are a few fp32 unit roundoffs times the magnitude sum of each result's terms; bf16-stored results get half a bf16 ulp
on top.  bf16-stored inputs are drawn bf16-exact, so the fp32 statistics of the producer are those of the stored tensor.
An element whose fp64 value is further from zero than its bound must not come back as exactly 0 (a lost pass or slab)."""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24           # fp32 unit roundoff
HALF_BF16 = 2.0 ** -8      # half a bf16 ulp, relative (upper bound)
MAXB = 1024
D = torch.float64


def K():
    from scouter_amd import kernels
    return kernels


def _profiled(fn):
    """-> (fn(), names of the library kernels it launched)"""
    from scouter_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    L.scouter_prof_collect(buf, len(buf))
    L.scouter_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.scouter_prof_enable(0)
        L.scouter_prof_collect(buf, len(buf))
    return out, [row.split("\t")[0] for row in buf.value.decode().splitlines()]


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _no_lost_tail(got, ref, what):
    """an element the fp64 reference has non-zero must not come back as exactly zero"""
    lost = (got == 0) & (ref != 0)
    assert not bool(lost.any()), "%s: %d elements with a non-zero fp64 value read back as 0" % (what, int(lost.sum()))


def _close(name, got, ref, mag, k, bf16=False):
    """|got - ref| <= k * U32 * mag (+ half a bf16 ulp of ref for a bf16-stored result), every element"""
    got = got.double().reshape(ref.shape)
    tol = k * U32 * mag + 1e-30
    if bf16:
        tol = tol + HALF_BF16 * (ref.abs() + tol)
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), "%s: %d of %d elements off, worst %.3g x its bound" % (
        name, int(bad.sum()), err.numel(), float((err / tol).max()))
    # (a value within its bound of 0 may be a ReLU sign the fp32 rounding decided the other way)
    _no_lost_tail(got, torch.where(ref.abs() > tol, ref, torch.zeros_like(ref)), name)


def _check_planes(planes, f32, n):
    if n == 1:
        assert torch.equal(planes[0], f32.bfloat16())
    else:
        v = f32.double()
        assert bool(((planes.double().sum(0) - v).abs() <= U32 * v.abs()).all()), "three planes != the fp32 value"


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# the routing rules, mirrored (csrc/bn_elem.hip col_geom / col_blocks / fin_narrow / ew_blocks / ew_blocks_hoist)
# ---------------------------------------------------------------------------------------------------------------
def _geom(M, C):
    cs = C if (C // 4 <= 256 and 256 % (C // 4) == 0) else 1024
    rpb = 256 // (cs // 4)
    nb_raw = -(-M // (8 * rpb))
    return ("row" if cs == C else "slab") + ("-cap" if nb_raw > MAXB else ""), rpb, max(1, min(MAXB, nb_raw))


def _ew(n):
    return max(1, min(2048, -(-n // 256)))


def _apply(M, C, bf16x8):
    """(apply-pass field, loop field) of the channel-parameter pass over M x C"""
    n4 = M * C // 4
    if bf16x8:
        n = n4 // 2
        return ("bf16x8h" if 256 % (C // 8) == 0 else "bf16x8"), ("loop" if n > _ew(n) * 256 else None)
    cv = C // 4
    grid = _ew(n4)
    if 256 % cv == 0:
        kind = "hoist"
    elif cv % 256 == 0:
        kind, m = "hoist-wide", cv // 256
        grid = grid if grid <= 1 else -(-grid // m) * m
    else:
        kind = "stride"
    return kind, ("loop" if n4 > grid * 256 else None)


def _label(prefix, *fields):
    return "%s<%s>" % (prefix, ",".join(f for f in fields if f))


def _fin(C, nparts):
    return "fin1" if C <= 64 and nparts > 512 else "fin4"


def _route_bn_fwd(M, C, o):
    geom, _, nb = _geom(M, C)
    src = "partial" if not o["ext_rows"] else "ext"
    if not o.get("training", True):
        src = "eval"
    has_y = o.get("keep_f32", True) or o.get("planes", 0)
    bf16x8 = (o["x"] == "bf16" and o["y"] == "bf16" and o.get("keep_f32", True) and o.get("res") in (None, "bf16")
              and not o.get("planes", 0) and C % 8 == 0)
    apply, loop = _apply(M, C, bf16x8) if has_y else ("none", None)
    return _label("bn_fwd(stats+finalize+apply)", src, geom if src == "partial" else None,
                  _fin(C, o["ext_rows"] if src == "ext" else nb), apply, loop)


def _route_bn_bwd(M, C, o):
    geom, rpb, nb = _geom(M, C)
    ext = o["ext_rows"]
    if not ext and M <= 24 * rpb and o["dy"] == o["x"] == o["dx"] == "f32":
        return _label("bn_bwd(reduce+finalize+apply)", "small",
                      "slab16" if C % 16 == 0 and C >= 32 else geom.replace("-cap", ""))
    # (with ext the wrapper returns dy itself as the masked gradient: no gout pointer reaches the library)
    bf16x8 = (o["dy"] == o["x"] == o["dx"] == "bf16" and not o["ymask"] and not o["mask"] and not (o["gout"] and not ext)
              and C % 8 == 0)
    apply, loop = _apply(M, C, bf16x8)
    return _label("bn_bwd(finalize+apply)" if ext else "bn_bwd(reduce+finalize+apply)", "ext" if ext else "partial",
                  None if ext else geom, _fin(C, ext or nb), apply, loop)


def _route_colsum(M, C):
    geom, rpb, _ = _geom(M, C)
    if M <= 12 * rpb or M <= 256:
        return _label("colsum", "direct", geom.replace("-cap", ""))
    return _label("colsum", "partial", geom, "fin4")


def _route_sa_bn_bwd(B, HW, C2, o):
    M = B * HW
    geom, _, _ = _geom(M, C2)
    bf16x8 = o["x"] == "bf16" and not o["keep_f32"] and o["planes"] == 1 and (C2 // 2) % 8 == 0
    apply, loop = _apply(M, C2, bf16x8)
    if o["sums"]:
        return _label("sa_bn_bwd(finalize+apply)", "sums", apply, loop)
    return _label("sa_bn_bwd(reduce+finalize+apply)", "partial", geom, "fin4", apply, loop)


# ---------------------------------------------------------------------------------------------------------------
# data and fp64 references
# ---------------------------------------------------------------------------------------------------------------
def _act(shape, gen, bf16=False, mean=0.8):
    """an activation-like tensor: per-channel non-zero mean and spread; bf16=True: bf16-exact values (fp32 tensor)"""
    C = shape[-1]
    x = torch.randn(shape, device="cuda", generator=gen)
    x = x * (0.4 + torch.rand(C, device="cuda", generator=gen)) + mean * torch.randn(C, device="cuda", generator=gen)
    return x.bfloat16().float() if bf16 else x


def _store(t, dt):
    return t.bfloat16() if dt == "bf16" else t


def _ext_rows(cols, rows):
    """[rows, C, 2] fp64 statistics rows as a producer's epilogue writes them: row r holds the sums of a contiguous chunk"""
    M, C = cols[0].shape
    rid = torch.arange(M, device="cuda") * rows // M
    part = torch.zeros(rows, C, 2, dtype=D, device="cuda")
    for j, v in enumerate(cols):
        part[:, :, j].index_add_(0, rid, v)
    return part


def _params(C, gen):
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C, device="cuda", generator=gen) * 0.3
    rm = torch.randn(C, device="cuda", generator=gen) * 0.2
    rv = torch.rand(C, device="cuda", generator=gen) + 0.5
    return gamma, beta, rm, rv


def _bn64(x, gamma, beta, training, rm, rv, eps=1e-5):
    """fp64 train- / eval-mode BatchNorm of x [M, C] with autograd leaves (x, gamma, beta) -> (leaves, y, mean, var)"""
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    if training:
        mu = x64.mean(0)
        var = ((x64 - mu) ** 2).mean(0)
    else:
        mu, var = rm.double(), rv.double()
    y = (x64 - mu) * torch.rsqrt(var + eps) * g64 + b64
    return (x64, g64, b64), y, mu.detach(), var.detach()


def _check_saved(saved, gamma, beta, mu, var, eps=1e-5):
    rstd = torch.rsqrt(var + eps)
    _close("saved mean", saved[0], mu, mu.abs() + 1e-9 * var.sqrt(), 4)
    _close("saved rstd", saved[1], rstd, rstd, 4)
    _close("saved scale", saved[2], gamma.double() * rstd, gamma.double().abs() * rstd, 4)
    assert torch.equal(saved[3], beta)


def _check_running(rm_k, rv_k, rm0, rv0, mu, var, M, momentum=0.1):
    unb = var * M / (M - 1) if M > 1 else var
    ref_m = (1 - momentum) * rm0.double() + momentum * mu
    ref_v = (1 - momentum) * rv0.double() + momentum * unb
    _close("running mean", rm_k, ref_m, rm0.double().abs() + mu.abs(), 4)
    _close("running var", rv_k, ref_v, rv0.double().abs() + unb + mu * mu * 1e-6, 8)


def _mask_gate(mask, n):
    """the 0/1 gate of the ReLU sign bits (word (f >> 6) * 4 + k, bit f & 63 for element 4 f + k)"""
    w = mask.view(-1, 1, 4)
    bits = (w >> torch.arange(64, device="cuda").view(1, 64, 1)) & 1
    return bits.reshape(-1, 4)[: n // 4].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------
# runners: one call of an entry point, its route asserted, every output against fp64
# ---------------------------------------------------------------------------------------------------------------
def _prep_fwd(M, C, o, gen):
    """x (fp32 copy, bf16-exact where stored bf16), its stored form, params, ext statistics"""
    x = _act((M, C), gen, bf16=o["x"] == "bf16")
    st = None
    if o["ext_rows"]:
        xd = x.double()
        st = (_ext_rows((xd, xd * xd), o["ext_rows"]), o["ext_rows"])
    return x, _store(x, o["x"]), st


def run_bn_stats(M, C, o, seed):
    kk = K()
    gen = _gen(seed)
    x, xs, st = _prep_fwd(M, C, o, gen)
    gamma, beta, rm, rv = _params(C, gen)
    rm0, rv0 = rm.clone(), rv.clone()
    saved, names = _profiled(lambda: kk.bn_stats(xs, gamma, beta, rm, rv, o["training"], stats=st))
    want = _route_bn_fwd(M, C, dict(o, y="f32", keep_f32=False, planes=0))
    assert want in names, (want, names)
    _, _, mu, var = _bn64(x, gamma, beta, o["training"], rm0, rv0)
    _check_saved(saved, gamma, beta, mu, var)
    if o["training"]:
        _check_running(rm, rv, rm0, rv0, mu, var, M)


def run_bn_fwd(M, C, o, seed):
    kk = K()
    gen = _gen(seed)
    training = o.get("training", True)
    x, xs, st = _prep_fwd(M, C, o, gen)
    gamma, beta, rm, rv = _params(C, gen)
    rm0, rv0 = rm.clone(), rv.clone()
    res = res_bn = None
    if o["res"]:
        res = _act((M, C), gen, bf16=o["res"] == "bf16", mean=0.3)
        if o["res_bn"]:
            q = torch.stack([torch.randn(C, device="cuda", generator=gen) * 0.5, torch.rand(C, device="cuda", generator=gen) + 0.5])
            res_bn = torch.stack([q[0], q[1], q[1] * (torch.rand(C, device="cuda", generator=gen) + 0.5),
                                  torch.randn(C, device="cuda", generator=gen) * 0.2])
    out_dtype = torch.bfloat16 if o["y"] == "bf16" else torch.float32
    out, names = _profiled(lambda: kk.bn_fwd(xs, gamma, beta, rm, rv, training, o["relu"], _store(res, o["res"]) if res is not None else None,
                                             stats=st if training else None, want_mask=o["mask"], planes=o["planes"],
                                             residual_bn=res_bn, keep_f32=o["keep_f32"], out_dtype=out_dtype))
    want = _route_bn_fwd(M, C, o)
    assert want in names, (want, names)
    y, saved = out[0], out[1]
    _, y64, mu, var = _bn64(x, gamma, beta, training, rm0, rv0)
    y64 = y64.detach()
    _check_saved(saved, gamma, beta, mu, var)
    if training:
        _check_running(rm, rv, rm0, rv0, mu, var, M)
    else:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    mag = (x.double().abs() + mu.abs()) * gamma.double().abs() * torch.rsqrt(var + 1e-5) + beta.double().abs()
    if res is not None:
        r = res.double()
        if res_bn is not None:
            qb = res_bn.double()
            mag = mag + (r.abs() + qb[0].abs()) * qb[2].abs() + qb[3].abs()
            r = (r - qb[0]) * qb[2] + qb[3]
        else:
            mag = mag + r.abs()
        y64 = y64 + r
    if o["relu"]:
        y64 = y64.clamp_min(0)
    if isinstance(y, kk.PlaneTensor):
        planes, y = y.planes, y.f32
        if y is not None:       # the planes split the stored fp32 result: one plane = its bf16 rounding, three = its value
            _check_planes(planes, y, o["planes"])
        else:
            _close("bn_fwd plane", planes.double().sum(0).view(M, C), y64, mag, 8, bf16=o["planes"] == 1)
    if y is not None:
        _close("bn_fwd y", y.view(M, C), y64, mag, 8, bf16=o["y"] == "bf16")
    if o["mask"]:
        got = y if y is not None else planes[0]
        assert torch.equal(_mask_gate(out[2], M * C), (got.reshape(-1) > 0).long()), "ReLU sign bits"


def run_bn_bwd(M, C, o, seed):
    kk = K()
    gen = _gen(seed)
    training = o["training"]
    x = _act((M, C), gen, bf16=o["x"] == "bf16")
    gamma, beta, rm, rv = _params(C, gen)
    xd = x.double()
    st = (_ext_rows((xd, xd * xd), 64), 64) if o["x"] == "bf16" else None
    relu = o["ymask"] or o["mask"]
    fw = kk.bn_fwd(_store(x, o["x"]), gamma, beta, rm.clone(), rv.clone(), training, relu, stats=st if training else None,
                   want_mask=o["mask"])
    saved = fw[1]
    dy = torch.randn(M, C, device="cuda", generator=gen)
    if o["dy"] == "bf16":
        dy = dy.bfloat16().float()
    gate = torch.ones(M * C, dtype=torch.long, device="cuda")
    if o["mask"]:
        gate = _mask_gate(fw[2], M * C)
    elif o["ymask"]:
        gate = (fw[0].reshape(-1) > 0).long()
    g = dy * gate.view(M, C)                             # the masked gradient the kernel forms (exact: a product by 0 / 1)
    ext = None
    if o["ext_rows"]:
        xh = (xd - saved[0].double()) * saved[1].double()
        ext = (_ext_rows((g.double(), g.double() * xh), o["ext_rows"]), o["ext_rows"])
        dyk = _store(g, o["dy"])
    else:
        dyk = _store(dy, o["dy"])
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx_dtype = torch.bfloat16 if o["dx"] == "bf16" else torch.float32
    (dx, gout), names = _profiled(lambda: kk.bn_bwd(dyk, fw[0] if o["ymask"] else None, _store(x, o["x"]), saved, training, dg, db,
                                                    o["gout"], mask=fw[2] if o["mask"] else None, ext=ext, dx_dtype=dx_dtype))
    want = _route_bn_bwd(M, C, o)
    assert want in names, (want, names)
    if o["gout"]:
        assert torch.equal(gout, g)
    (x64, g64, b64), y64, mu, var = _bn64(x, gamma, beta, training, rm, rv)
    g64d = g.double()
    y64.backward(g64d)
    rstd = torch.rsqrt(var + 1e-5)
    mx = (xd.abs() + mu.abs()) * rstd                      # |xhat| plus what the fp32 mean / rstd put into it
    ga = g64d.abs()
    a1, a2 = ga.mean(0), (ga * mx).mean(0) if training else 0 * ga.mean(0)
    a1 = a1 if training else 0 * a1
    mag = gamma.double().abs() * rstd * (ga + a1 + mx * a2)
    _close("bn_bwd dx", dx.view(M, C), x64.grad, mag, 16, bf16=o["dx"] == "bf16")
    _close("bn_bwd dgamma", dg, g64.grad, (ga * mx).sum(0), 8)
    _close("bn_bwd dbeta", db, b64.grad, ga.sum(0), 4)


def run_colsum(M, C, o, seed):
    kk = K()
    gen = _gen(seed)
    a = _act((M, C), gen)
    b = _act((M, C), gen, mean=-0.5) if o["b"] else None
    out = torch.empty(C, device="cuda")
    _, names = _profiled(lambda: kk.colsum(a, out, b, o["alpha"]))
    want = _route_colsum(M, C)
    assert want in names, (want, names)
    t = a.double() * (b.double() if b is not None else 1.0)
    _close("colsum", out, o["alpha"] * t.sum(0), abs(o["alpha"]) * t.abs().sum(0), 4)


def _sa_data(B, HW, C2, o, gen):
    x = _act((B, HW, C2), gen, bf16=o["x"] == "bf16")
    gamma, beta, rm, rv = _params(C2, gen)
    saved = K().bn_stats(x, gamma, beta, rm, rv, True)          # (the fp32 copy: bf16-exact values, the same statistics)
    z = torch.randn(B, C2, device="cuda", generator=gen)
    a = torch.softmax(z.view(B, 2, C2 // 2), 1).reshape(B, C2).contiguous()
    return x, gamma, beta, rm, rv, saved, a


def _sa_h(x, gamma, beta, saved):
    """fp64 h = relu(bn0(x)) over [B*HW, C2] with autograd leaves; the ReLU sign taken from the kernel's affine map"""
    B, HW, C2 = x.shape
    (x64, g64, b64), y64, mu, var = _bn64(x.view(-1, C2), gamma, beta, True, None, None)
    gate = (K().bn_apply(x.view(-1, C2).contiguous(), saved, False) > 0).double()
    rstd = torch.rsqrt(var + 1e-5)
    hmag = ((x.view(-1, C2).double().abs() + mu.abs()) * gamma.double().abs() * rstd + beta.double().abs()) * gate
    return (x64, g64, b64), (y64 * gate).view(B, HW, C2), hmag.view(B, HW, C2), gate.view(B, HW, C2), mu, rstd


def run_sa(entry, B, HW, C2, o, seed):
    kk = K()
    gen = _gen(seed)
    Cp = C2 // 2
    x, gamma, beta, rm, rv, saved, a = _sa_data(B, HW, C2, o, gen)
    xs = _store(x, o["x"]).view(B, HW, 1, C2)
    (x64, g64, b64), h, hmag, gate, mu, rstd = _sa_h(x, gamma, beta, saved)
    assert o.get("bn", True)                                    # (the model's calls: x is bn0's raw input)
    if entry == "sa_gap":
        gap = kk.sa_gap(xs, saved if o["bn"] else None)
        ref = (h[..., :Cp] + h[..., Cp:]).mean(1).detach()
        _close("sa_gap", gap, ref, (hmag[..., :Cp] + hmag[..., Cp:]).mean(1), 8)
        return
    a64 = a.double().view(B, 1, C2)
    if entry == "sa_apply_fwd":
        out = kk.sa_apply_fwd(xs, a, saved if o["bn"] else None,
                              out_dtype=torch.bfloat16 if o["y"] == "bf16" else torch.float32)
        ha = h * a64
        ref = (ha[..., :Cp] + ha[..., Cp:]).detach()
        hm = hmag * a64
        _close("sa_apply_fwd", out.view(B, HW, Cp), ref, hm[..., :Cp] + hm[..., Cp:], 8, bf16=o["y"] == "bf16")
        return
    dout = torch.randn(B, HW, Cp, device="cuda", generator=gen)
    if entry == "sa_dattn":
        r = kk.sa_dattn(xs, dout.view(B, HW, 1, Cp), saved, want_stats=o["stats"])
        da = r[0] if o["stats"] else r
        d2 = dout.double().repeat(1, 1, 2)
        _close("sa_dattn", da, (h * d2).sum(1).detach(), (hmag * d2.abs()).sum(1), 8)
        return
    # sa_bn_bwd: L = sum dout * out + sum dgap * gap, differentiated through h = relu(bn0(x))
    dgap = torch.randn(B, Cp, device="cuda", generator=gen)
    sums = kk.sa_dattn(xs, dout.view(B, HW, 1, Cp), saved, want_stats=True)[1] if o["sums"] else None
    dg, db = torch.zeros(C2, device="cuda"), torch.zeros(C2, device="cuda")
    r, names = _profiled(lambda: kk.sa_bn_bwd(dout.view(B, HW, 1, Cp), a, dgap, xs, saved, o["training"], dg, db,
                                              planes=o["planes"], keep_f32=o["keep_f32"], sums=sums))
    want = _route_sa_bn_bwd(B, HW, C2, o)
    assert want in names, (want, names)
    ha = h * a64
    L = (dout.double() * (ha[..., :Cp] + ha[..., Cp:])).sum() + (dgap.double() * (h[..., :Cp] + h[..., Cp:]).mean(1)).sum()
    L.backward()
    gmag = (dout.double().abs().repeat(1, 1, 2) * a64.abs() + dgap.double().abs().repeat(1, 2).view(B, 1, C2) / HW) * gate
    gmag = gmag.view(-1, C2)
    mx = (x.view(-1, C2).double().abs() + mu.abs()) * rstd
    mag = gamma.double().abs() * rstd * (gmag + gmag.mean(0) + mx * (gmag * mx).mean(0))
    if isinstance(r, kk.PlaneTensor):
        if r.f32 is not None:
            _check_planes(r.planes, r.f32, o["planes"])
            r = r.f32
        else:
            _close("sa_bn_bwd plane", r.planes.double().sum(0).view(-1, C2), x64.grad, mag, 16, bf16=o["planes"] == 1)
            r = None
    if r is not None:
        _close("sa_bn_bwd dx", r.view(-1, C2), x64.grad, mag, 16)
    _close("sa_bn_bwd dgamma", dg, g64.grad, (gmag * mx).sum(0), 8)
    _close("sa_bn_bwd dbeta", db, b64.grad, gmag.sum(0), 4)


def _run(entry, shape, o, seed):
    if entry == "bn_stats":
        run_bn_stats(*shape, o, seed)
    elif entry == "bn_fwd":
        run_bn_fwd(*shape, o, seed)
    elif entry == "bn_bwd":
        run_bn_bwd(*shape, o, seed)
    elif entry == "colsum":
        run_colsum(*shape, o, seed)
    else:
        run_sa(entry, *shape, o, seed)
    _free()


# ---------------------------------------------------------------------------------------------------------------
# both sides of every rule
# ---------------------------------------------------------------------------------------------------------------
F = dict(x="f32", y="f32", training=True, relu=True, res=None, res_bn=False, ext_rows=0, mask=True, planes=0, keep_f32=True)
B_ = dict(dy="f32", x="f32", dx="f32", training=True, ymask=False, mask=True, gout=False, ext_rows=0)
BF = dict(F, x="bf16", y="bf16", ext_rows=96, mask=True)                          # all-bf16 forward (stats from the producer)
BB = dict(B_, dy="bf16", x="bf16", dx="bf16", mask=False)                         # all-bf16 backward (dy already masked)
SA = dict(x="f32", training=True, planes=0, keep_f32=True, sums=False)

ROUTES = [  # (rule, entry, shape, flags, route field the pair differs in)
    # col_geom: whole-row slab / two 1024-channel slabs / one slab with 24 live lanes
    ("col_geom", "bn_fwd", (4099, 1024), F), ("col_geom", "bn_fwd", (4099, 2048), F), ("col_geom", "bn_fwd", (4099, 96), F),
    ("col_geom", "bn_bwd", (4099, 1024), B_), ("col_geom", "bn_bwd", (4099, 2048), B_), ("col_geom", "bn_bwd", (4099, 96), B_),
    # col_blocks: at the cap the blocks loop over rows with a ragged last pass
    ("col_blocks", "bn_fwd", (131072, 64), dict(F, relu=False, mask=False)),
    ("col_blocks", "bn_fwd", (131073, 64), dict(F, relu=False, mask=False)),
    ("col_blocks", "bn_fwd", (131072 + 4 * 1024 * 16 * 8 + 77, 64), F),
    ("col_blocks", "bn_bwd", (131072, 64), B_), ("col_blocks", "bn_bwd", (131073, 64), B_),
    ("col_blocks", "bn_fwd", (8192, 2048), F), ("col_blocks", "bn_fwd", (12544, 2048), F),
    ("col_blocks", "bn_bwd", (8192, 2048), dict(B_, mask=False, ymask=True)), ("col_blocks", "bn_bwd", (12544, 2048), B_),
    # fin_narrow: nparts = nb (own reduction) or ext_rows (the producer's rows)
    ("fin_narrow", "bn_fwd", (65536, 64), F), ("fin_narrow", "bn_fwd", (65537, 64), F),
    ("fin_narrow", "bn_bwd", (65536, 64), B_), ("fin_narrow", "bn_bwd", (65537, 64), B_),
    ("fin_narrow", "bn_fwd", (70 * 112 * 112, 32), F), ("fin_narrow", "bn_fwd", (70 * 112 * 112, 128), F),
    ("fin_narrow", "bn_fwd", (20011, 64), dict(F, ext_rows=512)), ("fin_narrow", "bn_fwd", (20011, 64), dict(F, ext_rows=513)),
    ("fin_narrow", "bn_bwd", (20011, 64), dict(B_, mask=False, ext_rows=512)),
    ("fin_narrow", "bn_bwd", (20011, 64), dict(B_, mask=False, ext_rows=513)),
    # one-launch backward of the pooled vectors
    ("bn_bwd_small", "bn_bwd", (96, 256), B_), ("bn_bwd_small", "bn_bwd", (97, 256), B_),
    ("bn_bwd_small", "bn_bwd", (192, 128), dict(B_, gout=True)), ("bn_bwd_small", "bn_bwd", (193, 128), dict(B_, gout=True)),
    ("bn_bwd_small", "bn_bwd", (70, 2048), B_), ("bn_bwd_small", "bn_bwd", (24, 20), dict(B_, mask=False, ymask=True)),
    ("bn_bwd_small", "bn_bwd", (25, 20), dict(B_, mask=False, ymask=True)), ("bn_bwd_small", "bn_bwd", (1536, 16), B_),
    ("bn_bwd_small", "bn_bwd", (96, 256), dict(B_, dx="bf16")),
    # elementwise grid: one vector per thread / every thread strides
    ("ew_blocks", "bn_fwd", (8192, 256), F), ("ew_blocks", "bn_fwd", (8193, 256), F),
    ("ew_blocks", "bn_bwd", (8192, 256), B_), ("ew_blocks", "bn_bwd", (8193, 256), B_),
    # channel-hoisted passes: hoisted / rounded grid (3072: 2048 -> 2049 workgroups) / un-hoisted
    ("ew_blocks_hoist", "bn_fwd", (3001, 256), dict(F, res="f32")), ("ew_blocks_hoist", "bn_fwd", (3001, 192), dict(F, res="f32")),
    ("ew_blocks_hoist", "bn_fwd", (4099, 3072), dict(F, res="f32", res_bn=True)),
    ("ew_blocks_hoist", "bn_fwd", (3, 2048), dict(F, relu=False, mask=False, training=False)),
    ("ew_blocks_hoist", "bn_bwd", (4099, 3072), dict(B_, gout=True)), ("ew_blocks_hoist", "bn_bwd", (3001, 192), B_),
    ("ew_blocks_hoist", "bn_fwd", (3001, 256), dict(F, planes=3)), ("ew_blocks_hoist", "bn_fwd", (3001, 96), dict(F, planes=1, keep_f32=False)),
    # bf16x8 passes and the other storage combinations
    ("bf16x8", "bn_fwd", (4099, 2048), BF), ("bf16x8", "bn_fwd", (4099, 96), BF), ("bf16x8", "bn_fwd", (4099, 192), dict(BF, res="bf16")),
    ("bf16x8", "bn_fwd", (4099, 2048), dict(BF, res="bf16", res_bn=True)),
    ("bf16x8", "bn_fwd", (4099, 2048), dict(BF, res="f32")), ("bf16x8", "bn_fwd", (4099, 192), dict(F, y="bf16", res="bf16")),
    ("bf16x8", "bn_fwd", (4099, 96), dict(BF, y="f32")), ("bf16x8", "bn_fwd", (4099, 256), dict(F, x="bf16", ext_rows=40)),
    ("bf16x8", "bn_bwd", (4099, 2048), BB), ("bf16x8", "bn_bwd", (4099, 96), BB), ("bf16x8", "bn_bwd", (4099, 192), BB),
    ("bf16x8", "bn_bwd", (4099, 256), dict(BB, ext_rows=33)),
    ("bf16x8", "bn_bwd", (4099, 256), dict(B_, x="bf16")), ("bf16x8", "bn_bwd", (4099, 256), dict(B_, dx="bf16")),
    ("bf16x8", "bn_bwd", (4099, 96), dict(BB, dx="f32")), ("bf16x8", "bn_bwd", (4099, 192), dict(BB, x="f32")),
    ("bf16x8", "bn_bwd", (4099, 2048), dict(B_, x="bf16", dx="bf16", ymask=True, mask=False)),
    # column sums: one launch / partial + finalize
    ("colsum", "colsum", (256, 64), dict(b=False, alpha=1.0)), ("colsum", "colsum", (257, 64), dict(b=True, alpha=-0.5)),
    ("colsum", "colsum", (256, 2048), dict(b=True, alpha=0.25)), ("colsum", "colsum", (257, 2048), dict(b=False, alpha=1.0)),
    ("colsum", "colsum", (131073, 64), dict(b=False, alpha=1.0)), ("colsum", "colsum", (12, 96), dict(b=True, alpha=3.0)),
    # statistics only (no apply pass)
    ("bn_stats", "bn_stats", (65537, 64), dict(x="f32", training=True, ext_rows=0)),
    ("bn_stats", "bn_stats", (4099, 256), dict(x="bf16", training=True, ext_rows=700)),
    ("bn_stats", "bn_stats", (4099, 256), dict(x="f32", training=False, ext_rows=0)),
    # split attention + bn0 backward: statistics from sa_dattn or its own reduction; bf16x8 <true> / <false>; hoisted or not
    ("sa_bn_bwd", "sa_bn_bwd", (7, 197, 1024), dict(SA, x="bf16", planes=1, keep_f32=False, sums=True)),
    ("sa_bn_bwd", "sa_bn_bwd", (7, 197, 1024), dict(SA, x="bf16", planes=1, keep_f32=False)),
    ("sa_bn_bwd", "sa_bn_bwd", (7, 197, 192), dict(SA, x="bf16", planes=1, keep_f32=False)),
    ("sa_bn_bwd", "sa_bn_bwd", (7, 197, 192), dict(SA, planes=3)),
    ("sa_bn_bwd", "sa_bn_bwd", (5, 301, 2048), SA), ("sa_bn_bwd", "sa_bn_bwd", (5, 301, 256), dict(SA, sums=True)),
    ("sa_bn_bwd", "sa_bn_bwd", (70, 49, 1024), dict(SA, planes=3, keep_f32=False, sums=True)),
    ("sa_reduce", "sa_gap", (7, 197, 1024), dict(x="bf16", bn=True)), ("sa_reduce", "sa_gap", (7, 197, 128), dict(x="f32", bn=True)),
    ("sa_reduce", "sa_dattn", (7, 197, 1024), dict(x="bf16", bn=True, stats=True)),
    ("sa_reduce", "sa_apply_fwd", (7, 197, 1024), dict(x="bf16", bn=True, y="bf16")),
    ("sa_reduce", "sa_apply_fwd", (7, 197, 192), dict(x="bf16", bn=True, y="bf16")),
    ("sa_reduce", "sa_apply_fwd", (7, 197, 4096), dict(x="f32", bn=True, y="f32")),
]


def _rid(r):
    rule, entry, shape, o = r
    fl = "".join(k[0] + str(v)[0] for k, v in sorted(o.items()) if v not in (None, False, 0, "f32") or k == "x" and v == "bf16")
    return "%s-%s-%s-%s" % (rule, entry, "x".join(map(str, shape)), fl)


@pytest.mark.parametrize("row", ROUTES, ids=_rid)
def test_route(row):
    rule, entry, shape, o = row
    _run(entry, shape, o, zlib.crc32(repr(row).encode()) % 100003)


def test_every_rule_has_two_routes():
    """each rule's cases reach at least two different routes (the labels the tests assert)"""
    def route(entry, shape, o):
        if entry == "bn_fwd":
            return _route_bn_fwd(*shape, o)
        if entry == "bn_stats":
            return _route_bn_fwd(*shape, dict(o, y="f32", keep_f32=False))
        if entry == "bn_bwd":
            return _route_bn_bwd(*shape, o)
        if entry == "colsum":
            return _route_colsum(*shape)
        if entry == "sa_bn_bwd":
            return _route_sa_bn_bwd(*shape, o)
        return entry
    by_rule = {}
    for rule, entry, shape, o in ROUTES:
        by_rule.setdefault(rule, set()).add(route(entry, shape, o))
    for rule, routes in by_rule.items():
        if rule != "sa_reduce":
            assert len(routes) >= 2, (rule, routes)


# ---------------------------------------------------------------------------------------------------------------
# production shapes: every distinct call of one training step of BASELINE configs 2, 4 and 5 (bench.py's model, batch and
# precision), recorded by tools_dev/record_bn_calls.py (each scouter_amd.kernels entry point wrapped by a recorder, one
# eager step).  (config, entry, shape, flags); shape = (M, C) or (B, H*W, 2C') for the split-attention entry points.
# ---------------------------------------------------------------------------------------------------------------
PRODUCTION = [
    (2, 'bn_fwd', (878080, 32), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 6860, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_stats', (878080, 64), {'x': 'f32', 'training': True, 'ext_rows': 6860}),
    (2, 'bn_stats', (219520, 256), {'x': 'f32', 'training': True, 'ext_rows': 128}),
    (2, 'bn_fwd', (219520, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 512, 'mask': True, 'planes': 3, 'keep_f32': True}),
    (2, 'bn_stats', (219520, 128), {'x': 'f32', 'training': True, 'ext_rows': 858}),
    (2, 'sa_gap', (70, 3136, 128), {'x': 'f32', 'bn': True}),
    (2, 'bn_fwd', (70, 32), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 1, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'sa_apply_fwd', (70, 3136, 128), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (219520, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 128, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_fwd', (219520, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 256, 'mask': True, 'planes': 3, 'keep_f32': True}),
    (2, 'bn_fwd', (219520, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_stats', (54880, 512), {'x': 'f32', 'training': True, 'ext_rows': 215}),
    (2, 'bn_fwd', (219520, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'bn_stats', (219520, 256), {'x': 'f32', 'training': True, 'ext_rows': 858}),
    (2, 'sa_gap', (70, 3136, 256), {'x': 'f32', 'bn': True}),
    (2, 'bn_fwd', (70, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'sa_apply_fwd', (70, 3136, 256), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (54880, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 64, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_fwd', (54880, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 215, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'bn_stats', (54880, 256), {'x': 'f32', 'training': True, 'ext_rows': 215}),
    (2, 'sa_gap', (70, 784, 256), {'x': 'f32', 'bn': True}),
    (2, 'sa_apply_fwd', (70, 784, 256), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (54880, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 64, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_stats', (13720, 1024), {'x': 'f32', 'training': True, 'ext_rows': 54}),
    (2, 'bn_fwd', (54880, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 215, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'sa_gap', (70, 784, 512), {'x': 'f32', 'bn': True}),
    (2, 'bn_fwd', (70, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 1, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'sa_apply_fwd', (70, 784, 512), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (13720, 1024), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 54, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_fwd', (13720, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 108, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'bn_stats', (13720, 512), {'x': 'f32', 'training': True, 'ext_rows': 54}),
    (2, 'sa_gap', (70, 196, 512), {'x': 'f32', 'bn': True}),
    (2, 'sa_apply_fwd', (70, 196, 512), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (13720, 1024), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 54, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_stats', (3430, 2048), {'x': 'f32', 'training': True, 'ext_rows': 14}),
    (2, 'bn_fwd', (13720, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 54, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'sa_gap', (70, 196, 1024), {'x': 'f32', 'bn': True}),
    (2, 'bn_fwd', (70, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'sa_apply_fwd', (70, 196, 1024), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (3430, 2048), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 14, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'bn_fwd', (3430, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 54, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (2, 'bn_stats', (3430, 1024), {'x': 'f32', 'training': True, 'ext_rows': 27}),
    (2, 'sa_gap', (70, 49, 1024), {'x': 'f32', 'bn': True}),
    (2, 'sa_apply_fwd', (70, 49, 1024), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (2, 'bn_fwd', (3430, 2048), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 14, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (2, 'colsum', (70, 640), {'b': False, 'alpha': 1.0}),
    (2, 'colsum', (70, 1920), {'b': False, 'alpha': 1.0}),
    (2, 'colsum', (1400, 192), {'b': False, 'alpha': 1.0}),
    (2, 'colsum', (3430, 64), {'b': False, 'alpha': 1.0}),
    (2, 'bn_bwd', (3430, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 54}),
    (2, 'sa_dattn', (70, 49, 1024), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'colsum', (70, 1024), {'b': False, 'alpha': 1.0}),
    (2, 'bn_bwd', (70, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (2, 'colsum', (70, 256), {'b': False, 'alpha': 1.0}),
    (2, 'sa_bn_bwd', (70, 49, 1024), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (3430, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 54}),
    (2, 'bn_bwd', (3430, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 14}),
    (2, 'bn_bwd', (3430, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 14}),
    (2, 'sa_dattn', (70, 196, 1024), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'sa_bn_bwd', (70, 196, 1024), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (13720, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 54}),
    (2, 'bn_bwd', (13720, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 54}),
    (2, 'sa_dattn', (70, 196, 512), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'colsum', (70, 512), {'b': False, 'alpha': 1.0}),
    (2, 'bn_bwd', (70, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (2, 'colsum', (70, 128), {'b': False, 'alpha': 1.0}),
    (2, 'sa_bn_bwd', (70, 196, 512), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (13720, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 108}),
    (2, 'bn_bwd', (13720, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 16}),
    (2, 'bn_bwd', (13720, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 16}),
    (2, 'sa_dattn', (70, 784, 512), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'sa_bn_bwd', (70, 784, 512), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (54880, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 215}),
    (2, 'bn_bwd', (54880, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 32}),
    (2, 'sa_dattn', (70, 784, 256), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'bn_bwd', (70, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (2, 'colsum', (70, 64), {'b': False, 'alpha': 1.0}),
    (2, 'sa_bn_bwd', (70, 784, 256), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (54880, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 215}),
    (2, 'bn_bwd', (54880, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 64}),
    (2, 'bn_bwd', (54880, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 64}),
    (2, 'sa_dattn', (70, 3136, 256), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'sa_bn_bwd', (70, 3136, 256), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (2, 'bn_bwd', (219520, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 858}),
    (2, 'bn_bwd', (219520, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 128}),
    (2, 'sa_dattn', (70, 3136, 128), {'x': 'f32', 'bn': True, 'stats': True}),
    (2, 'bn_bwd', (70, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (2, 'colsum', (70, 32), {'b': False, 'alpha': 1.0}),
    (2, 'sa_bn_bwd', (70, 3136, 128), {'x': 'f32', 'training': True, 'planes': 0, 'keep_f32': True, 'sums': True}),
    (2, 'bn_bwd', (219520, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 128}),
    (2, 'bn_bwd', (219520, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 128}),
    (2, 'bn_bwd', (878080, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 256}),
    (4, 'bn_fwd', (1605632, 32), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 12544, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_stats', (1605632, 64), {'x': 'f32', 'training': True, 'ext_rows': 6272}),
    (4, 'bn_stats', (401408, 256), {'x': 'f32', 'training': True, 'ext_rows': 128}),
    (4, 'bn_fwd', (401408, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 512, 'mask': True, 'planes': 3, 'keep_f32': True}),
    (4, 'bn_stats', (401408, 128), {'x': 'f32', 'training': True, 'ext_rows': 1568}),
    (4, 'sa_gap', (128, 3136, 128), {'x': 'f32', 'bn': True}),
    (4, 'bn_fwd', (128, 32), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 1, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'sa_apply_fwd', (128, 3136, 128), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (401408, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 128, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_fwd', (401408, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 256, 'mask': True, 'planes': 3, 'keep_f32': True}),
    (4, 'bn_fwd', (401408, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_stats', (100352, 512), {'x': 'f32', 'training': True, 'ext_rows': 392}),
    (4, 'bn_fwd', (401408, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'bn_stats', (401408, 256), {'x': 'f32', 'training': True, 'ext_rows': 1568}),
    (4, 'sa_gap', (128, 3136, 256), {'x': 'f32', 'bn': True}),
    (4, 'bn_fwd', (128, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 1, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'sa_apply_fwd', (128, 3136, 256), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (100352, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 64, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_fwd', (100352, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 392, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'bn_stats', (100352, 256), {'x': 'f32', 'training': True, 'ext_rows': 392}),
    (4, 'sa_gap', (128, 784, 256), {'x': 'f32', 'bn': True}),
    (4, 'sa_apply_fwd', (128, 784, 256), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (100352, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 64, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_stats', (25088, 1024), {'x': 'f32', 'training': True, 'ext_rows': 98}),
    (4, 'bn_fwd', (100352, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 392, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'sa_gap', (128, 784, 512), {'x': 'f32', 'bn': True}),
    (4, 'bn_fwd', (128, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'sa_apply_fwd', (128, 784, 512), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (25088, 1024), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 196, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_fwd', (25088, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 98, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'bn_stats', (25088, 512), {'x': 'f32', 'training': True, 'ext_rows': 98}),
    (4, 'sa_gap', (128, 196, 512), {'x': 'f32', 'bn': True}),
    (4, 'sa_apply_fwd', (128, 196, 512), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (25088, 1024), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 196, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_stats', (6272, 2048), {'x': 'f32', 'training': True, 'ext_rows': 25}),
    (4, 'bn_fwd', (25088, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 98, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'sa_gap', (128, 196, 1024), {'x': 'f32', 'bn': True}),
    (4, 'bn_fwd', (128, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'sa_apply_fwd', (128, 196, 1024), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (6272, 2048), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': True, 'ext_rows': 25, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'bn_fwd', (6272, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 49, 'mask': True, 'planes': 3, 'keep_f32': False}),
    (4, 'bn_stats', (6272, 1024), {'x': 'f32', 'training': True, 'ext_rows': 100}),
    (4, 'sa_gap', (128, 49, 1024), {'x': 'f32', 'bn': True}),
    (4, 'sa_apply_fwd', (128, 49, 1024), {'x': 'f32', 'bn': True, 'y': 'f32'}),
    (4, 'bn_fwd', (6272, 2048), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'f32', 'res_bn': False, 'ext_rows': 25, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (4, 'colsum', (128, 12800), {'b': False, 'alpha': 1.0}),
    (4, 'colsum', (128, 38400), {'b': False, 'alpha': 1.0}),
    (4, 'colsum', (51200, 192), {'b': False, 'alpha': 1.0}),
    (4, 'colsum', (6272, 64), {'b': False, 'alpha': 1.0}),
    (4, 'bn_bwd', (6272, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 98}),
    (4, 'sa_dattn', (128, 49, 1024), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'colsum', (128, 1024), {'b': False, 'alpha': 1.0}),
    (4, 'bn_bwd', (128, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (4, 'colsum', (128, 256), {'b': False, 'alpha': 1.0}),
    (4, 'sa_bn_bwd', (128, 49, 1024), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (6272, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 49}),
    (4, 'bn_bwd', (6272, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 98}),
    (4, 'sa_dattn', (128, 196, 1024), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'sa_bn_bwd', (128, 196, 1024), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (25088, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 98}),
    (4, 'bn_bwd', (25088, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 392}),
    (4, 'sa_dattn', (128, 196, 512), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'colsum', (128, 512), {'b': False, 'alpha': 1.0}),
    (4, 'bn_bwd', (128, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (4, 'colsum', (128, 128), {'b': False, 'alpha': 1.0}),
    (4, 'sa_bn_bwd', (128, 196, 512), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (25088, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 98}),
    (4, 'bn_bwd', (25088, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 16}),
    (4, 'bn_bwd', (25088, 1024), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 16}),
    (4, 'sa_dattn', (128, 784, 512), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'sa_bn_bwd', (128, 784, 512), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (100352, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 392}),
    (4, 'bn_bwd', (100352, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 32}),
    (4, 'sa_dattn', (128, 784, 256), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'bn_bwd', (128, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (4, 'colsum', (128, 64), {'b': False, 'alpha': 1.0}),
    (4, 'sa_bn_bwd', (128, 784, 256), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (100352, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 392}),
    (4, 'bn_bwd', (100352, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 64}),
    (4, 'bn_bwd', (100352, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 64}),
    (4, 'sa_dattn', (128, 3136, 256), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'sa_bn_bwd', (128, 3136, 256), {'x': 'f32', 'training': True, 'planes': 3, 'keep_f32': False, 'sums': True}),
    (4, 'bn_bwd', (401408, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 1568}),
    (4, 'bn_bwd', (401408, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 128}),
    (4, 'sa_dattn', (128, 3136, 128), {'x': 'f32', 'bn': True, 'stats': True}),
    (4, 'bn_bwd', (128, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (4, 'colsum', (128, 32), {'b': False, 'alpha': 1.0}),
    (4, 'sa_bn_bwd', (128, 3136, 128), {'x': 'f32', 'training': True, 'planes': 0, 'keep_f32': True, 'sums': True}),
    (4, 'bn_bwd', (401408, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 128}),
    (4, 'bn_bwd', (401408, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 128}),
    (4, 'bn_bwd', (1605632, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 256}),
    (5, 'bn_fwd', (3211264, 32), {'x': 'f32', 'y': 'bf16', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 25088, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_stats', (3211264, 64), {'x': 'f32', 'training': True, 'ext_rows': 25088}),
    (5, 'bn_stats', (802816, 256), {'x': 'bf16', 'training': True, 'ext_rows': 6272}),
    (5, 'bn_fwd', (802816, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 12544, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (802816, 128), {'x': 'bf16', 'training': True, 'ext_rows': 3136}),
    (5, 'sa_gap', (256, 3136, 128), {'x': 'bf16', 'bn': True}),
    (5, 'bn_fwd', (256, 32), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'sa_apply_fwd', (256, 3136, 128), {'x': 'bf16', 'bn': True, 'y': 'bf16'}),
    (5, 'bn_fwd', (802816, 256), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': True, 'ext_rows': 384, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_fwd', (802816, 256), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': False, 'ext_rows': 384, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_stats', (200704, 512), {'x': 'bf16', 'training': True, 'ext_rows': 1568}),
    (5, 'bn_fwd', (802816, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 256, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (802816, 256), {'x': 'bf16', 'training': True, 'ext_rows': 3136}),
    (5, 'sa_gap', (256, 3136, 256), {'x': 'bf16', 'bn': True}),
    (5, 'bn_fwd', (256, 64), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'sa_apply_fwd', (256, 3136, 256), {'x': 'bf16', 'bn': True, 'y': 'f32'}),
    (5, 'bn_fwd', (200704, 512), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': True, 'ext_rows': 1568, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_fwd', (200704, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 256, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (200704, 256), {'x': 'bf16', 'training': True, 'ext_rows': 784}),
    (5, 'sa_gap', (256, 784, 256), {'x': 'bf16', 'bn': True}),
    (5, 'sa_apply_fwd', (256, 784, 256), {'x': 'bf16', 'bn': True, 'y': 'bf16'}),
    (5, 'bn_fwd', (200704, 512), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_stats', (50176, 1024), {'x': 'bf16', 'training': True, 'ext_rows': 392}),
    (5, 'bn_fwd', (200704, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 128, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (200704, 512), {'x': 'bf16', 'training': True, 'ext_rows': 784}),
    (5, 'sa_gap', (256, 784, 512), {'x': 'bf16', 'bn': True}),
    (5, 'bn_fwd', (256, 128), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 2, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'sa_apply_fwd', (256, 784, 512), {'x': 'bf16', 'bn': True, 'y': 'f32'}),
    (5, 'bn_fwd', (50176, 1024), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': True, 'ext_rows': 392, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_fwd', (50176, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 392, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (50176, 512), {'x': 'bf16', 'training': True, 'ext_rows': 196}),
    (5, 'sa_gap', (256, 196, 512), {'x': 'bf16', 'bn': True}),
    (5, 'sa_apply_fwd', (256, 196, 512), {'x': 'bf16', 'bn': True, 'y': 'bf16'}),
    (5, 'bn_fwd', (50176, 1024), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': False, 'ext_rows': 32, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_stats', (12544, 2048), {'x': 'bf16', 'training': True, 'ext_rows': 98}),
    (5, 'bn_fwd', (50176, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 392, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (50176, 1024), {'x': 'bf16', 'training': True, 'ext_rows': 196}),
    (5, 'sa_gap', (256, 196, 1024), {'x': 'bf16', 'bn': True}),
    (5, 'bn_fwd', (256, 256), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 4, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'sa_apply_fwd', (256, 196, 1024), {'x': 'bf16', 'bn': True, 'y': 'f32'}),
    (5, 'bn_fwd', (12544, 2048), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': True, 'ext_rows': 98, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_fwd', (12544, 512), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': None, 'res_bn': False, 'ext_rows': 98, 'mask': True, 'planes': 1, 'keep_f32': False}),
    (5, 'bn_stats', (12544, 1024), {'x': 'bf16', 'training': True, 'ext_rows': 98}),
    (5, 'sa_gap', (256, 49, 1024), {'x': 'bf16', 'bn': True}),
    (5, 'sa_apply_fwd', (256, 49, 1024), {'x': 'bf16', 'bn': True, 'y': 'bf16'}),
    (5, 'bn_fwd', (12544, 2048), {'x': 'bf16', 'y': 'bf16', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': False, 'ext_rows': 16, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'bn_stats', (12544, 1024), {'x': 'f32', 'training': True, 'ext_rows': 98}),
    (5, 'sa_gap', (256, 49, 1024), {'x': 'f32', 'bn': True}),
    (5, 'sa_apply_fwd', (256, 49, 1024), {'x': 'f32', 'bn': True, 'y': 'bf16'}),
    (5, 'bn_fwd', (12544, 2048), {'x': 'f32', 'y': 'f32', 'training': True, 'relu': True, 'res': 'bf16', 'res_bn': False, 'ext_rows': 16, 'mask': True, 'planes': 0, 'keep_f32': True}),
    (5, 'colsum', (256, 19200), {'b': False, 'alpha': 1.0}),
    (5, 'colsum', (256, 57600), {'b': False, 'alpha': 1.0}),
    (5, 'colsum', (153600, 192), {'b': False, 'alpha': 1.0}),
    (5, 'colsum', (12544, 64), {'b': False, 'alpha': 1.0}),
    (5, 'bn_bwd', (12544, 2048), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 196}),
    (5, 'sa_dattn', (256, 49, 1024), {'x': 'f32', 'bn': True, 'stats': True}),
    (5, 'colsum', (256, 1024), {'b': False, 'alpha': 1.0}),
    (5, 'bn_bwd', (256, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'colsum', (256, 256), {'b': False, 'alpha': 1.0}),
    (5, 'sa_bn_bwd', (256, 49, 1024), {'x': 'f32', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (12544, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (12544, 2048), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 196}),
    (5, 'sa_dattn', (256, 49, 1024), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'sa_bn_bwd', (256, 49, 1024), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (12544, 2048), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 16}),
    (5, 'bn_bwd', (12544, 2048), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 16}),
    (5, 'sa_dattn', (256, 196, 1024), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'sa_bn_bwd', (256, 196, 1024), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (50176, 512), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (50176, 1024), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 784}),
    (5, 'sa_dattn', (256, 196, 512), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'colsum', (256, 512), {'b': False, 'alpha': 1.0}),
    (5, 'bn_bwd', (256, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'colsum', (256, 128), {'b': False, 'alpha': 1.0}),
    (5, 'sa_bn_bwd', (256, 196, 512), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (50176, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (50176, 1024), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 32}),
    (5, 'bn_bwd', (50176, 1024), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 32}),
    (5, 'sa_dattn', (256, 784, 512), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'sa_bn_bwd', (256, 784, 512), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (200704, 256), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (200704, 512), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 3136}),
    (5, 'sa_dattn', (256, 784, 256), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'bn_bwd', (256, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'colsum', (256, 64), {'b': False, 'alpha': 1.0}),
    (5, 'sa_bn_bwd', (256, 784, 256), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (200704, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (200704, 512), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 128}),
    (5, 'bn_bwd', (200704, 512), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 64}),
    (5, 'bn_bwd', (200704, 512), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 64}),
    (5, 'sa_dattn', (256, 3136, 256), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'sa_bn_bwd', (256, 3136, 256), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (802816, 128), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'bn_bwd', (802816, 256), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 12544}),
    (5, 'sa_dattn', (256, 3136, 128), {'x': 'bf16', 'bn': True, 'stats': True}),
    (5, 'bn_bwd', (256, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': True, 'gout': False, 'ext_rows': 0}),
    (5, 'colsum', (256, 32), {'b': False, 'alpha': 1.0}),
    (5, 'sa_bn_bwd', (256, 3136, 128), {'x': 'bf16', 'training': True, 'planes': 1, 'keep_f32': False, 'sums': True}),
    (5, 'bn_bwd', (802816, 64), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 6272}),
    (5, 'bn_bwd', (802816, 256), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 256}),
    (5, 'bn_bwd', (802816, 256), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': True, 'ext_rows': 128}),
    (5, 'bn_bwd', (802816, 256), {'dy': 'bf16', 'x': 'bf16', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 128}),
    (5, 'bn_bwd', (3211264, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'bf16', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 25088}),
    (5, 'bn_bwd', (3211264, 32), {'dy': 'f32', 'x': 'f32', 'dx': 'f32', 'training': True, 'ymask': False, 'mask': False, 'gout': False, 'ext_rows': 25088}),
]


def _pid(r):
    c, entry, shape, o = r
    return "cfg%d-%s" % (c, _rid(("", entry, shape, o))[1:])


@pytest.mark.parametrize("row", PRODUCTION, ids=_pid)
def test_production_shape(row):
    c, entry, shape, o = row
    _run(entry, shape, o, zlib.crc32(repr(row).encode()) % 100003)
