"""Size-switched kernel routes on both sides of their thresholds (-m gpu).

Several dispatchers pick another kernel once a tensor passes a grid-row limit (65 535 workgroup rows, 2^20 threads along a
row) or a byte offset of 2^31 (the buffer descriptors of the resident-rows kernels hold 31-bit record counts, and a read
past the record count returns ZEROS without an error).  The rest of the suite never builds tensors that large, so here
every route below is launched just below and just above its threshold:
  * the library profiler (scouter_prof_enable / scouter_prof_collect) proves which kernel ran on each side -- a boundary
    test that never crosses its boundary proves nothing;
  * the values are checked against fp64 on both sides: every element where that is cheap (pools, im2col, BatchNorm), else
    a random sample of output elements with exact fp64 by indexing + einsum on the device, bounded relative to
    V = sqrt(sum of squared terms) (tests/test_table_entries_gpu.py).  A quarter of every sample is forced into the tail --
    the last image, its last 64 pixels, the last 32 channels -- where offsets pass 2^31 and a clipped descriptor would
    read zeros; no tail sample may be exactly zero unless its fp64 value is.

THRESHOLDS (the C guard and, for the convolution routes, the route query of include/scouter_hip.h through which the wrappers ask
it -- tests/test_route_queries_cpu.py flips each of those queries between the same two shapes without a device; kernel names as
the profiler reports them; the shape below / above):

  route                     guard                                          below kernel            above kernel
  ------------------------  ---------------------------------------------  ----------------------  ---------------------
  max / avg pool backward   B*H <= 65535, W*C/4 < 2^20, stride 1 / 2       maxpool_bwd<rows>       maxpool_bwd<grid>
                            (csrc/bn_elem.hip pool_bwd_rows_ok)            avgpool_bwd<rows>       avgpool_bwd<grid>
      B*H:    13107 x 5 x 5 x 8 (65 535 rows)      /  16384 x 4 x 4 x 8 (65 536 rows)
      W*C/4:  1 x 4 x 1023 x 4096 (2^20 - 1024)    /  1 x 4 x 1024 x 4096 (2^20)
      stride: 3 x 3 / stride 2 (rows kernel)        /  3 x 3 / stride 3 (grid kernel)
  stem bn1 + ReLU + maxpool B*H <= 65535 (csrc/bn_elem.hip                 bn_maxpool_fwd,         maxpool_bwd<grid> +
                            scouter_bn_maxpool_bwd_io; Python:             bn_maxpool_bwd(...)     bn_bwd(...): the
                            timm/models/resnet.py fwd, the fuse_stem_pool                          unfused chain
                            test)
      13107 x 5 x 5 x 64 (65 535 rows)  /  16384 x 4 x 4 x 64 (65 536 rows: the fused backward refuses it)
  im2col of the NCHW stem   rows = B*Ho <= 65535, Kpad <= 64 (Cin < 256    im2col<rows>            im2col<elem>
                            is implied by Kpad <= 64), Wo*Kpad/4 < 2^20
                            (csrc/misc_ops.hip scouter_im2col_nchw_f32)
      rows:  13107 x 3 x 10 x 10, 3x3 / 2 (65 535 rows)  /  16384 x 3 x 8 x 8 (65 536 rows)
      Kpad:  7 channels, 3x3 (Kpad 64)                   /  10 channels, 3x3 (Kpad 96); the 7x7 stem (Kpad 160)
  resident-rows register-   4*M*max(Cin, Cout) < 2^31 (csrc/conv_xhalo.hip  xhalo_fwd<bf16x3>       igemm_fwd<...>
  split kernel, tile 7:     sc_xhalo_ok; query: scouter_conv2d_{fwd,dgrad}  xhalo_dgrad<bf16x3>     igemm_dgrad<...>
  forward (x3 bit 7) and    _x3_tile_ok, asked by nn_hip.Conv2d.fwd / .bwd)                        (the fp32 MFMA kernels
  input gradient (bit 6)                                                                           that served them before)
      32 -> 32 forward + gradients, 64 x 64 maps:  4095 images (M*128 = 2^31 - 2^19)  /  4096 images (M*128 = 2^31)
      32 -> 64 input gradient, 64 x 64 maps:       2047 images (M*256 = 2^31 - 2^20)  /  2048 images (M*256 = 2^31)
      layer-level: the deep stem's 32 -> 64 module at 680 x 112 x 112 with default switches (above)

  persistent pointwise tile 4 4*M*max(K, N) < 2^31 (csrc/conv_igemm.hip        igemm_fwd<persistent>   igemm_fwd<...>
                            pwp_geom_ok; query: scouter_conv2d_{fwd,dgrad} igemm_dgrad<persistent> igemm_dgrad<...>
                            _tile_ok)
      1x1, 64 <-> 256 channels, 56 x 56:  668 images  /  669 images
  bf16 resident-rows input  M*Cout*2 < 2^31 - 2^20 for fp32-stored dy       bhalo_dgrad<bf16>       igemm_dgrad_bf16<...>
  gradient (BHALO)          (policy: kernels.dgrad_prerounds), (M + 512)*
                            Cout*2 < 2^31 for bf16-stored dy (conv_halo_
                            dgrad_bf16.h bhalo_dgrad_ok; query: scouter_
                            conv2d_dgrad_bf16_tile_ok, resident_rows = 1)
      32 -> 64, 64 x 64:  fp32 dy 4093 / 4094 images;  bf16 dy 4095 / 4096 images
  bf16 tap-fused weight     M*max(Cin, Cout)*2 < 2^31 - 2^20 (policy:         bwgrad_taps<bf16>       wgrad_bf16
  gradient (BWT)            kernels.wgrad_prerounds, over conv_igemm.hip
                            bwt_geom_ok = scouter_conv2d_wgrad_kernel_ok)
      32 -> 64, 64 x 64, fp32-stored operands:  4093 / 4094 images
  tap-fused plane weight    2*M*max(Cin, Cout) < 2^31, W <= 63 (conv_planes.  plan >= 64 (tap-fused)  plan < 64 (per tap)
  gradient                  hip pwgrad_fused_ok; query: scouter_conv2d_    (both report pwgrad<bf16>: read from the plan cache)
                            wgrad_planes_plan_ok)
      one plane, 128 -> 256 in two groups, 56 x 56:  1337 / 1338 images
  plane forward / input     nplanes*B*H*W*C*2 < 2^31 + H*W*C*2               pconv_fwd<bf16>         RuntimeError "tensor too
  gradient                  (csrc/conv_planes.hip pconv_size_ok; query:    pconv_dgrad<bf16>       large for 32-bit plane
                            scouter_conv2d_{fwd,dgrad}_planes_tile_ok): no                         offsets"
                            other kernel takes plane operands
      one plane, 64 channels, 32 x 32:  16384 images (the largest batch, PLANE_MAX_B)  /  16385

Peak device memory per test, as measured (torch.cuda.max_memory_allocated): at most 12.4 GB (the tile-7 rows and the layer-level
test); each test's docstring gives its own figure where it is above 1 GB.  Every case frees its tensors before the next."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NS = 2048                  # sampled output elements per tensor (a quarter of them in the tail)
NW = 12                    # sampled weight-gradient elements (each one is a sum over every pixel)
U32 = 2.0 ** -24           # fp32 unit roundoff


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


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _no_lost_tail(got, ref, what):
    """an element the fp64 reference has non-zero must not come back as exactly zero (a clipped buffer read)"""
    lost = (got == 0) & (ref != 0)
    assert not bool(lost.any()), "%s: %d elements with a non-zero fp64 value read back as 0" % (what, int(lost.sum()))


# ---------------------------------------------------------------------------------------------------------------
# pools: maxpool_bwd / avgpool_bwd, rows kernel vs grid-stride kernel
# ---------------------------------------------------------------------------------------------------------------
POOL_CASES = [  # (B, H, W, C, k, stride, pad, kernel suffix)
    (13107, 5, 5, 8, 3, 2, 1, "rows"),          # B*H = 65535
    (16384, 4, 4, 8, 3, 2, 1, "grid"),          # B*H = 65536
    (1, 4, 1023, 4096, 3, 2, 1, "rows"),        # W*C/4 = 2^20 - 1024
    (1, 4, 1024, 4096, 3, 2, 1, "grid"),        # W*C/4 = 2^20
    (7, 9, 11, 16, 3, 1, 1, "rows"),            # stride 1
    (7, 9, 11, 16, 3, 3, 0, "grid"),            # stride 3
]


def _scatter_taps(dy64, arg, x_shape, k, stride, pad):
    """fp64 max-pool backward along the kernel's OWN arg-max taps (ties in fp32 data decide nothing about the sums)"""
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy64.shape
    a = arg.long()
    oy = torch.arange(Ho, device="cuda").view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device="cuda").view(1, 1, Wo, 1)
    iy, ix = oy * stride - pad + a // k, ox * stride - pad + a % k
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), "an arg-max tap points into the padding"
    dx = torch.zeros(B, H * W, C, dtype=torch.float64, device="cuda")
    dx.scatter_add_(1, (iy * W + ix).reshape(B, Ho * Wo, C), dy64.reshape(B, Ho * Wo, C))
    return dx.view(B, H, W, C)


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "_s%d_%s" % (c[5], c[7]))
def test_maxpool_backward_both_sides_of_the_row_limits(case):
    B, H, W, C, k, s, p, route = case
    kk = K()
    gen = _gen(B + H + W + C + s)
    x = torch.randn(B, H, W, C, device="cuda", generator=gen)
    y, arg = kk.maxpool_fwd(x, k, s, p)
    # forward: a max of fp32 values is exact, and the tap must hold it
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2).double(), k, s, p).permute(0, 2, 3, 1)
    assert torch.equal(y.double(), ref)
    dy = torch.randn(y.shape, device="cuda", generator=gen)
    dx, names = _profiled(lambda: kk.maxpool_bwd(dy, arg, tuple(x.shape), k, s, p))
    assert "maxpool_bwd<%s>" % route in names, names
    ref = _scatter_taps(dy.double(), arg, tuple(x.shape), k, s, p)
    mag = _scatter_taps(dy.double().abs(), arg, tuple(x.shape), k, s, p)
    err = (dx.double() - ref).abs()
    assert bool((err <= 4 * U32 * mag).all()), float((err - 4 * U32 * mag).max())
    _no_lost_tail(dx, ref, "maxpool_bwd")
    del x, y, arg, dy, dx, ref, mag, err
    _free()


@pytest.mark.parametrize("ceil_mode,count_pad", [(False, True), (True, False)])
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "_s%d_%s" % (c[5], c[7]))
def test_avgpool_backward_both_sides_of_the_row_limits(case, ceil_mode, count_pad):
    B, H, W, C, k, s, p, route = case
    kk = K()
    gen = _gen(B + H + W + C + s + 7)
    xs = (B, H, W, C)
    Ho, Wo = kk.pool_out(H, k, s, p, ceil_mode), kk.pool_out(W, k, s, p, ceil_mode)
    dy = torch.randn(B, Ho, Wo, C, device="cuda", generator=gen)
    dx, names = _profiled(lambda: kk.avgpool_bwd(dy, xs, k, s, p, ceil_mode, count_pad))
    assert "avgpool_bwd<%s>" % route in names, names
    refs = []
    for d in (dy.double(), dy.double().abs()):
        x64 = torch.zeros(B, C, H, W, dtype=torch.float64, device="cuda", requires_grad=True)
        yy = torch.nn.functional.avg_pool2d(x64, k, s, p, ceil_mode, count_pad)
        assert tuple(yy.shape) == (B, C, Ho, Wo)
        (yy * d.permute(0, 3, 1, 2)).sum().backward()
        refs.append(x64.grad.permute(0, 2, 3, 1))
    ref, mag = refs
    err = (dx.double() - ref).abs()
    assert bool((err <= 6 * U32 * mag).all()), float((err - 6 * U32 * mag).max())
    _no_lost_tail(dx, ref, "avgpool_bwd")
    del dy, dx, ref, mag, err, refs
    _free()


# ---------------------------------------------------------------------------------------------------------------
# the stem's bn1 + ReLU + maxpool: fused pair below B*H = 65536, the unfused chain above
# ---------------------------------------------------------------------------------------------------------------
def _bn_pool_ref(x, gamma, beta, dp, arg, mask):
    """fp64 BatchNorm (training statistics) -> ReLU -> max-pool 3 / 2 / 1 forward values and backward (dx, dgamma, dbeta),
    the pool's arg-max and the ReLU sign taken from the kernel (fp32 decisions; the sums are what is checked)"""
    B, H, W, C = x.shape
    x64 = x.double()
    mu = x64.mean((0, 1, 2))
    var = x64.var((0, 1, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (x64 - mu) * rstd
    h = (xhat * gamma.double() + beta.double()).clamp_min(0)
    p_ref = torch.nn.functional.max_pool2d(h.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    g = _scatter_taps(dp.double(), arg, tuple(x.shape), 3, 2, 1) * mask
    n = B * H * W
    dbeta = g.sum((0, 1, 2))
    dgamma = (g * xhat).sum((0, 1, 2))
    dx = gamma.double() * rstd * (g - dbeta / n - xhat * dgamma / n)
    # (V: the absolute terms of dx = scale * (g - sum g / n - xhat * sum(g xhat) / n))
    mag = gamma.double().abs() * rstd * (g.abs() + (g.abs().sum((0, 1, 2)) + (xhat * g).abs().sum((0, 1, 2)) * xhat.abs()) / n)
    hmag = float((xhat * gamma.double()).abs().max() + beta.double().abs().max())
    return p_ref, hmag, dx, mag, dgamma, dbeta, (g * xhat).abs().sum((0, 1, 2)), g.abs().sum((0, 1, 2))


@pytest.mark.parametrize("B,H", [(13107, 5), (16384, 4)], ids=["rows65535", "rows65536"])
def test_stem_batchnorm_relu_maxpool_both_sides_of_the_fused_limit(B, H):
    kk = K()
    W, C = H, 64
    gen = _gen(B + H)
    x = torch.randn(B, H, W, C, device="cuda", generator=gen) * 1.3 - 0.2
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C, device="cuda", generator=gen) * 0.3
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    fused = kk.bn_maxpool_fused_ok(B, H)          # the stem's routing rule, as timm/models/resnet.py applies it
    assert fused == (B * H <= 65535)
    if fused:
        saved = kk.bn_stats(x, gamma, beta, rm, rv, True)
        p, arg = kk.bn_maxpool_fwd(x, saved, 3, 2, 1)
        dp = torch.randn(p.shape, device="cuda", generator=gen)
        dx, names = _profiled(lambda: kk.bn_maxpool_bwd(dp, arg, x, saved, True, dg, db, 3, 2, 1))
        assert "bn_maxpool_bwd(reduce+finalize+apply)" in names, names
    else:
        saved = kk.bn_stats(x, gamma, beta, rm.clone(), rv.clone(), True)
        p, arg = kk.bn_maxpool_fwd(x, saved, 3, 2, 1)
        with pytest.raises(RuntimeError, match="bn_maxpool_bwd"):          # the C guard the Python rule mirrors
            kk.bn_maxpool_bwd(torch.zeros_like(p), arg, x, saved, True, None, None, 3, 2, 1)
        del p, arg
        h, saved, rmask = kk.bn_fwd(x, gamma, beta, rm, rv, True, True, want_mask=True)
        p, arg = kk.maxpool_fwd(h, 3, 2, 1)
        dp = torch.randn(p.shape, device="cuda", generator=gen)

        def chain():
            dh = kk.maxpool_bwd(dp, arg, tuple(h.shape), 3, 2, 1)
            return kk.bn_bwd(dh, None, x, saved, True, dg, db, mask=rmask)[0]
        dx, names = _profiled(chain)
        assert "maxpool_bwd<grid>" in names and any(n.startswith("bn_bwd(") for n in names), names
        del h, rmask
    mask = (kk.bn_apply(x, saved, False) > 0).double()
    p_ref, hmag, dx_ref, mag, dg_ref, db_ref, dg_mag, db_mag = _bn_pool_ref(x, gamma, beta, dp, arg, mask)
    assert float((p.double() - p_ref).abs().max()) <= 8 * U32 * hmag
    _no_lost_tail(p, p_ref, "pooled")
    err = (dx.double() - dx_ref).abs()
    tol = 32 * U32 * mag + 1e-12
    assert bool((err <= tol).all()), float((err / tol).max())
    _no_lost_tail(dx, dx_ref, "dx")
    # dgamma / dbeta: sums over B*H*W elements (fp64 partial sums of fp32 products in the kernels)
    assert bool(((dg.double() - dg_ref).abs() <= 4 * U32 * dg_mag + 1e-9).all())
    assert bool(((db.double() - db_ref).abs() <= 4 * U32 * db_mag + 1e-9).all())
    del x, p, arg, dp, dx, mask, p_ref, dx_ref, mag, err, tol
    _free()


# ---------------------------------------------------------------------------------------------------------------
# im2col of the NCHW stem image: rows kernel vs element-wise kernel
# ---------------------------------------------------------------------------------------------------------------
IM2COL_CASES = [  # (B, Cin, H, W, k, stride, pad, kernel suffix)
    (13107, 3, 10, 10, 3, 2, 1, "rows"),        # rows = 65535, Kpad 32
    (16384, 3, 8, 8, 3, 2, 1, "elem"),          # rows = 65536
    (5, 7, 13, 11, 3, 1, 1, "rows"),            # Kpad 64
    (5, 10, 13, 11, 3, 1, 1, "elem"),           # Kpad 96
    (3, 3, 30, 26, 7, 2, 3, "elem"),            # the 7x7 stem, Kpad 160
]


@pytest.mark.parametrize("case", IM2COL_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "_k%d_%s" % (c[4], c[7]))
def test_im2col_both_sides_of_its_limits(case):
    B, Cin, H, W, k, s, p, route = case
    kk = K()
    kpad = (k * k * Cin + 31) // 32 * 32
    x = torch.randn(B, Cin, H, W, device="cuda", generator=_gen(B + Cin + H))
    col, names = _profiled(lambda: kk.im2col_nchw(x, k, s, p, kpad))
    assert "im2col<%s>" % route in names, names
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    u = torch.nn.functional.unfold(x.double(), k, padding=p, stride=s)              # [B, Cin * k * k, L], (ci, ky, kx)
    ref = u.view(B, Cin, k * k, Ho * Wo).permute(0, 3, 2, 1).reshape(B, Ho, Wo, k * k * Cin)
    assert torch.equal(col[..., :k * k * Cin].double(), ref)
    assert not bool(col[..., k * k * Cin:].any())
    del x, col, u, ref
    _free()


# ---------------------------------------------------------------------------------------------------------------
# the resident-rows register-split kernel (tile 7) and the fp32 MFMA kernels past its byte guards, through nn_hip.Conv2d
# ---------------------------------------------------------------------------------------------------------------
def _pick(n, B, H, W, C, gen):
    """n output positions (b, y, x, c) of a [B, H, W, C] tensor; the last quarter in the tail: the last image, its last 64
    pixels, the last 32 channels -- the very last element (the highest byte offset) always among them"""
    ri = lambda hi, m: torch.randint(0, hi, (m,), generator=gen, device="cuda")
    nt = n // 4
    b = torch.cat([ri(B, n - nt), torch.full((nt,), B - 1, device="cuda", dtype=torch.long)])
    pix = torch.cat([ri(H * W, n - nt), H * W - 1 - ri(min(64, H * W), nt)])
    c = torch.cat([ri(C, n - nt), C - 1 - ri(min(32, C), nt)])
    pix[-1], c[-1] = H * W - 1, C - 1
    return b, pix // W, pix % W, c, nt


def _w64(w, bf16):
    """the weight the kernel multiplies, in fp64: fp32, or its RNE bf16 rounding"""
    return (w.bfloat16() if bf16 else w).double()


def _sample_fwd(x, w, idx, bf16=False):
    """exact fp64 y[b, yo, xo, co] of a k x k / stride 1 / pad k // 2 / groups 1 convolution (x as stored: fp32 or bf16) and
    V = sqrt(sum of squared terms)"""
    B, H, W, _ = x.shape
    k = w.shape[0]
    b, yo, xo, co, _ = idx
    acc = torch.zeros(b.numel(), dtype=torch.float64, device="cuda")
    sq = torch.zeros_like(acc)
    for r in range(k):
        for s in range(k):
            yy, xx = yo - k // 2 + r, xo - k // 2 + s
            ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).double()
            xv = x[b, yy.clamp(0, H - 1), xx.clamp(0, W - 1)].double() * ok[:, None]    # [n, Cin]
            t = xv * _w64(w[r, s][:, co].t(), bf16)
            acc += t.sum(1)
            sq += (t * t).sum(1)
    return acc, sq.sqrt()


def _sample_dgrad(dy, w, idx, bf16=False):
    """exact fp64 dx[b, y, x, ci] (k x k / stride 1 / pad k // 2 / groups 1; dy as stored, or rounded to bf16 with bf16=True)"""
    B, H, W, _ = dy.shape
    k = w.shape[0]
    b, y, x_, ci, _ = idx
    acc = torch.zeros(b.numel(), dtype=torch.float64, device="cuda")
    sq = torch.zeros_like(acc)
    for r in range(k):
        for s in range(k):
            yo, xo = y + k // 2 - r, x_ + k // 2 - s
            ok = ((yo >= 0) & (yo < H) & (xo >= 0) & (xo < W)).double()
            dv = dy[b, yo.clamp(0, H - 1), xo.clamp(0, W - 1)]
            dv = (dv.bfloat16() if bf16 else dv).double() * ok[:, None]                  # [n, Cout]
            t = dv * _w64(w[r, s][ci], bf16)
            acc += t.sum(1)
            sq += (t * t).sum(1)
    return acc, sq.sqrt()


def _sample_wgrad(x, dy, gen, n=NW, groups=1, bf16=False):
    """exact fp64 dW[r, s, ci, co] (HWIO, 3x3 / pad 1; ci within the group) at n positions -- the last one always (2, 2) with
    the last channels: its sum runs through the last image's last pixels"""
    B, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    cg, ng = Cin // groups, Cout // groups
    op = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
    out = []
    for i in range(n):
        if i == n - 1:
            r, s, cil, co = 2, 2, cg - 1, Cout - 1
        else:
            r, s, cil, co = [int(torch.randint(0, m, (1,), generator=gen, device="cuda")) for m in (3, 3, cg, Cout)]
        ci = (co // ng) * cg + cil
        # dW[r, s, cil, co] = sum_{b, y, x} x[b, y + r - 1, x + s - 1, ci] * dy[b, y, x, co]
        y0, y1 = max(0, 1 - r), min(H, H + 1 - r)
        x0, x1 = max(0, 1 - s), min(W, W + 1 - s)
        t = op(x[:, y0 + r - 1:y1 + r - 1, x0 + s - 1:x1 + s - 1, ci]) * op(dy[:, y0:y1, x0:x1, co])
        out.append(((r, s, cil, co), float(t.sum()), float((t * t).sum().sqrt())))
        del t
    return out


def _check(name, got, ref, mag, k):
    err = (got.double() - ref).abs()
    tol = k * mag + 1e-12
    bad = int((err > tol).sum())
    assert bad == 0, "%s: %d of %d sampled elements off, worst %.3g x its tolerance (|err| %.3g)" % (
        name, bad, err.numel(), float((err / tol).max()), float(err.max()))


def _k_for(n_terms):
    """relative bound (to V) for an fp32-grade sum of n_terms products: 2e-5 for short sums (the table entries' bound),
    growing like the random walk of fp32 rounding for long ones (weight gradients over millions of pixels)"""
    return max(2e-5, 8 * U32 * np.sqrt(n_terms))


def _conv_layer(cin, cout, x3):
    from scouter_amd import nn_hip
    torch.manual_seed(cin * 1000 + cout)
    m = nn_hip.Conv2d(cin, cout, 3, 1, 1).cuda()
    m.x3 = x3
    m._dw = torch.zeros(3, 3, cin, cout, device="cuda")
    return m


def _check_fused_bwd(m, dy, ctx, plain, gen, names_want):
    """the same input gradient with the fused BatchNorm-backward epilogue (the model's call: the BatchNorm + ReLU in front of
    this layer): the masked gradient == the BatchNorm backward's own masking of the plain one, and the epilogue's fp64
    statistics rows == sums of that masked gradient (and of its product with xhat) over every pixel"""
    kk = K()
    C = plain.shape[-1]
    x1 = torch.randn(plain.shape, device="cuda", generator=gen) * 1.7 + 0.4
    gamma, beta = torch.rand(C, device="cuda", generator=gen) + 0.5, torch.randn(C, device="cuda", generator=gen)
    _, saved1, mask = kk.bn_fwd(x1, gamma, beta, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), True, True,
                                want_mask=True)
    post = kk.BnBwdFuse(mask, [(x1, saved1)])
    gf, names = _profiled(lambda: m.bwd(dy, ctx, post=post))
    kk.join_side_stream(dy.device)
    torch.cuda.synchronize()
    assert post.applied and any(n.startswith(w) for w in names_want for n in names), (names_want, names)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    _, gout = kk.bn_bwd(plain, None, x1, saved1, True, dg, db, True, mask=mask)
    sc = float(gout.abs().max())
    assert float((gf - gout).abs().max()) <= 4e-6 * sc
    _no_lost_tail(gf[-1], gout[-1], "masked gradient, last image")
    part, rows = post.ext(0)
    sums = part[:rows].sum(0)
    torch.testing.assert_close(sums[:, 0], _col_sums(gf), rtol=1e-9, atol=1e-7)
    gx = torch.cat([gf.view(-1, C), x1.view(-1, C)], 1)
    torch.testing.assert_close(sums[:, 1], _col_sums(gx, lambda v: v[:, :C] * ((v[:, C:].float() - saved1[0]) * saved1[1]).double()),
                               rtol=1e-9, atol=1e-7)
    del x1, mask, post, gf, gout, gx, part


def _run_layer(m, B, H, W, seed, fwd_names, dgrad_names, check_stats=True, fused_names=None):
    """forward (with the BatchNorm statistics rows) + backward of an nn_hip.Conv2d at B x H x W; asserts the kernels by
    name (an entry ending in "<" is a prefix) and every sampled value against fp64, tail included"""
    cin, cout = m.in_channels, m.out_channels
    gen = _gen(seed)
    x = torch.randn(B, H, W, cin, device="cuda", generator=gen)
    w = m.weight.detach().permute(2, 3, 1, 0).contiguous()                            # HWIO (fp32: the x3 kernels' operand)

    def has(names, want):
        return any(n.startswith(want) if want.endswith("<") else n == want for n in names)
    ((y, (part, rows)), ctx), names = _profiled(lambda: m.fwd(x, True, bn_stats=True))
    assert all(has(names, f) for f in fwd_names), (fwd_names, names)
    idx = _pick(NS, B, H, W, cout, gen)
    ref, mag = _sample_fwd(x, w, idx)
    got = y[idx[0], idx[1], idx[2], idx[3]]
    _check("forward", got, ref, mag, _k_for(9 * cin))
    nt = idx[4]
    _no_lost_tail(got[-nt:], ref[-nt:], "forward tail")
    if check_stats:
        _check_stats(y, part, rows)          # every pixel, the tail included
    del y, part, got
    dy = torch.randn(B, H, W, cout, device="cuda", generator=gen)
    dx, names = _profiled(lambda: m.bwd(dy, ctx))
    K().join_side_stream(dy.device)
    torch.cuda.synchronize()
    assert all(has(names, f) for f in dgrad_names), (dgrad_names, names)
    idx = _pick(NS, B, H, W, cin, gen)
    ref, mag = _sample_dgrad(dy, w, idx)
    got = dx[idx[0], idx[1], idx[2], idx[3]]
    _check("input gradient", got, ref, mag, _k_for(9 * cout))
    _no_lost_tail(got[-nt:], ref[-nt:], "input gradient tail")
    del got
    for (r, s, ci, co), v, vm in _sample_wgrad(x, dy, gen):
        g = float(m._dw[r, s, ci, co])
        assert abs(g - v) <= _k_for(B * H * W) * vm, ("weight gradient", (r, s, ci, co), g, v, vm)
    del x, w
    if fused_names:
        _check_fused_bwd(m, dy, ctx, dx, gen, fused_names)
    del dx, ctx, dy
    m._dw.zero_()
    _free()


XHALO_ROWS = [  # (Cin, Cout, x3 bits, B, H = W, forward kernels, input-gradient kernels)
    (32, 32, 255, 4095, 64, ("xhalo_fwd<bf16x3>",), ("xhalo_dgrad<bf16x3>",)),         # 4*M*32 = 2^31 - 2^19
    (32, 32, 255, 4096, 64, ("igemm_fwd<",), ("igemm_dgrad<",)),                       # 4*M*32 = 2^31
    (32, 64, 127, 2047, 64, ("xconv3_fwd<bf16x3>",), ("xhalo_dgrad<bf16x3>",)),        # 4*M*64 = 2^31 - 2^20
    (32, 64, 127, 2048, 64, ("xconv3_fwd<bf16x3>",), ("igemm_dgrad<",)),               # 4*M*64 = 2^31
]


@pytest.mark.parametrize("row", XHALO_ROWS, ids=lambda r: "%dto%d_B%d" % (r[0], r[1], r[3]))
def test_xhalo_both_sides_of_its_byte_guards(row):
    """Peak 12.1 GB measured (32 -> 64 rows: x, y, dy, dx of 1-2 GB each + the fused BatchNorm-backward operands)."""
    cin, cout, x3, B, HW, fwd_names, dgrad_names = row
    kk = K()
    M = B * HW * HW
    assert kk.x3_halo_fits(M, cin, cout) == dgrad_names[0].startswith("xhalo")
    m = _conv_layer(cin, cout, x3)
    # (the 32 -> 64 rows also run the input gradient with the fused BatchNorm-backward epilogue, as the model calls it)
    fused = None if cout == 32 else tuple(n.replace("<", "+bn_bwd<", 1) for n in dgrad_names)
    _run_layer(m, B, HW, HW, B + cin + cout, fwd_names, dgrad_names, fused_names=fused)


def test_deep_stem_32_to_64_layer_routed_to_xhalo_past_its_guard_with_default_switches():
    """The deep stem's 32 -> 64 3x3 convolution at 680 images of 112 x 112 with the default switches (SCOUTER_X3 as the model
    sets it): its input gradient is past tile 7's byte guard (4*M*64 >= 2^31 from 669 images on) and takes the fp32 MFMA
    kernel instead of raising from inside backward.  Peak 12.3 GB measured."""
    kk = K()
    B, H = 680, 112
    assert not kk.x3_halo_fits(B * H * H, 32, 64) and kk.x3_halo_fits(668 * H * H, 32, 64)
    m = _conv_layer(32, 64, kk.X3_DEFAULT)
    assert m.route().dgrad == ("xhalo",)
    _run_layer(m, B, H, H, 680, ("xconv3_fwd<bf16x3>",), ("igemm_dgrad<",), fused_names=("igemm_dgrad+bn_bwd<",))


def _col_sums(t, fn=lambda v: v, rows=1 << 21):
    """fp64 column sums of fn(t viewed as [-1, C]), in slices (no fp64 copy of a multi-GB tensor)"""
    v = t.view(-1, t.shape[-1])
    return sum(fn(v[i:i + rows].double()).sum(0) for i in range(0, v.shape[0], rows))


def _check_stats(y, part, rows):
    """statistics rows a forward wrote == fp64 sums (and sums of squares) of its stored fp32 outputs, every pixel"""
    s = part[:rows].sum(0)
    for j, (v, vmag) in enumerate(((_col_sums(y), _col_sums(y, torch.abs)), (_col_sums(y, lambda u: u * u),) * 2)):
        assert bool(((s[:, j] - v).abs() <= 1e-9 * (vmag + 1e-30)).all()), (j, float(((s[:, j] - v).abs() / (vmag + 1e-30)).max()))


def _check_sampled(name, out, ref_fn, gen, k):
    """sampled fp64 check of an NHWC result, a quarter of the samples in the tail, no tail sample lost to zero"""
    B, H, W, C = out.shape
    idx = _pick(NS, B, H, W, C, gen)
    ref, mag = ref_fn(idx)
    got = out[idx[0], idx[1], idx[2], idx[3]]
    _check(name, got, ref, mag, k)
    _no_lost_tail(got[-idx[4]:], ref[-idx[4]:], name + " tail")


# ---------------------------------------------------------------------------------------------------------------
# persistent pointwise kernel, tile 4 (csrc/conv_igemm.hip pwp_geom_ok, which kernels._pw_persist_legal asks): 4*M*max(K, N) < 2^31.
# The static table picks tile 4 for 56 x 56, 64 <-> 256 channels; past the guard the lookup falls back to the library's tile.
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [668, 669], ids=["M4x256_below", "M4x256_above"])
def test_pointwise_tile4_both_sides_of_its_byte_guard(B):
    """668 images: 4*M*256 < 2^31; 669: past it.  Peak 10.6 GB measured (y and dy of 2.15 GB and their fp64 sums)."""
    kk = K()
    H = W = 56
    M = B * H * W
    persistent = B == 668
    assert kk._pw_persist_legal(M, 64, 256, 1, 1, 1, 0, 1, True) == persistent
    assert kk._pw_persist_legal(M, 256, 64, 1, 1, 1, 0, 1, True) == persistent
    gen = _gen(B)
    x = torch.randn(B, H, W, 64, device="cuda", generator=gen)
    w = torch.randn(1, 1, 64, 256, device="cuda", generator=gen) / 8
    (y, (part, rows)), names = _profiled(lambda: kk.conv2d_fwd(x, w, bn_stats=True))
    assert ("igemm_fwd<persistent>" in names) == persistent and any(n.startswith("igemm_fwd<") for n in names), names
    _check_sampled("forward", y, lambda idx: _sample_fwd(x, w, idx), gen, _k_for(64))
    _check_stats(y, part, rows)
    del y, part
    dy = torch.randn(B, H, W, 256, device="cuda", generator=gen)
    dx, names = _profiled(lambda: kk.conv2d_dgrad(dy, w, (B, H, W, 64)))
    assert ("igemm_dgrad<persistent>" in names) == persistent and any(n.startswith("igemm_dgrad<") for n in names), names
    _check_sampled("input gradient", dx, lambda idx: _sample_dgrad(dy, w, idx), gen, _k_for(256))
    del x, w, dy, dx
    _free()


# ---------------------------------------------------------------------------------------------------------------
# bf16 mode, 3x3 layers with 32 input channels per group: resident-rows input gradient (BHALO) and tap-fused weight
# gradient (BWT).  fp32-stored operands: the Python rules (kernels.conv2d_dgrad / conv2d_wgrad, M*max(C)*2 < 2^31 - 2^20)
# decide; bf16-stored dy: the library's (csrc/conv_halo_dgrad_bf16.h bhalo_dgrad_ok, (M + 512)*Cout*2 < 2^31).
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4093, 4094], ids=["below", "above"])
def test_bf16_halo_input_gradient_and_tap_fused_weight_gradient_both_sides(B):
    """32 -> 64 channels, 64 x 64 maps: 4093 images (M*128 = 2^31 - 2^20 - 2^19), 4094 (= 2^31 - 2^20: past both rules).
    fp32 operands (x 2.1 GB, dy 4.3 GB) + their bf16 copies + dx: peak 9.1 GB measured."""
    kk = K()
    H = W = 64
    M = B * H * W
    below = M * 64 * 2 < (1 << 31) - (1 << 20)
    assert below == (B == 4093)
    gen = _gen(B)
    w = torch.randn(3, 3, 32, 64, device="cuda", generator=gen) / 24
    dy = torch.randn(B, H, W, 64, device="cuda", generator=gen)
    dx, names = _profiled(lambda: kk.conv2d_dgrad(dy, w, (B, H, W, 32), None, 1, 1, 1, precision="bf16"))
    want = "bhalo_dgrad<bf16>" if below else "igemm_dgrad_bf16<"
    assert any(n.startswith(want) for n in names) and (below or "bhalo_dgrad<bf16>" not in names), names
    _check_sampled("bf16 input gradient", dx, lambda idx: _sample_dgrad(dy, w, idx, bf16=True), gen, _k_for(576))
    del dx
    x = torch.randn(B, H, W, 32, device="cuda", generator=gen)
    dw = torch.zeros(3, 3, 32, 64, device="cuda")
    _, names = _profiled(lambda: kk.conv2d_wgrad(x, dy, dw, 1, 1, 1, precision="bf16"))
    assert ("bwgrad_taps<bf16>" in names) == below and (below or "wgrad_bf16" in names), names
    for (r, s, ci, co), v, vm in _sample_wgrad(x, dy, gen, bf16=True):
        assert abs(float(dw[r, s, ci, co]) - v) <= _k_for(M) * vm, ("bf16 weight gradient", (r, s, ci, co), float(dw[r, s, ci, co]), v)
    del x, dy, dw
    _free()


@pytest.mark.parametrize("B", [4095, 4096], ids=["below", "above"])
def test_bf16_halo_input_gradient_of_a_bf16_stored_dy_both_sides(B):
    """bf16-STORED dy: the library's rule, (M + 512)*64*2 < 2^31 -- 4095 images of 64 x 64 below, 4096 above.  Peak 4.1 GB measured."""
    kk = K()
    H = W = 64
    M = B * H * W
    below = (M + 512) * 64 * 2 < (1 << 31)
    assert below == (B == 4095)
    gen = _gen(B)
    w = torch.randn(3, 3, 32, 64, device="cuda", generator=gen) / 24
    dy = torch.randn(B, H, W, 64, device="cuda", generator=gen, dtype=torch.bfloat16)
    dx, names = _profiled(lambda: kk.conv2d_dgrad(dy, w, (B, H, W, 32), None, 1, 1, 1, precision="bf16"))
    assert ("bhalo_dgrad<bf16>" in names) == below and any(n.startswith("bhalo_dgrad<" if below else "igemm_dgrad_bf16<")
                                                           for n in names), names
    _check_sampled("bf16 input gradient", dx, lambda idx: _sample_dgrad(dy, w, idx, bf16=True), gen, _k_for(576))
    del dy, dx
    _free()


# ---------------------------------------------------------------------------------------------------------------
# tap-fused plane weight gradient (kernels.conv2d_wgrad_planes asks csrc/conv_planes.hip pwgrad_fused_ok, the fused plan's
# guard: 2*B*H*W*max(Cin, Cout) < 2^31).  Both plans report the profile row "pwgrad<bf16>" (bench.py's kernel classes list that name), so the
# switch is read from the plan the dispatcher cached: >= 64 = tap-fused (bit 6), < 64 = per-tap.
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1337, 1338], ids=["below", "above"])
def test_tap_fused_plane_weight_gradient_both_sides(B):
    """One bf16 plane (bf16 mode), layer1's radix convolution shape 128 -> 256 in two groups at 56 x 56 (the static table's
    tap-fused entry): 1337 images (2*M*256 < 2^31) below, 1338 above.  Peak 3.3 GB measured."""
    kk = K()
    H = W = 56
    M = B * H * W
    below = 2 * M * 256 < (1 << 31)
    assert below == (B == 1337)
    gen = _gen(B)
    xp = torch.randn(1, B, H, W, 128, device="cuda", generator=gen, dtype=torch.bfloat16)
    dyp = torch.randn(1, B, H, W, 256, device="cuda", generator=gen, dtype=torch.bfloat16)
    dw = torch.zeros(3, 3, 64, 256, device="cuda")
    _, names = _profiled(lambda: kk.conv2d_wgrad_planes(xp, dyp, dw, 1, 2))
    assert "pwgrad<bf16>" in names, names
    plan = kk._tile_cache[("pwgrad", 1, B, H, W, 128, 256, 3, 3, 1, 2)]
    assert (plan >= 64) == below, plan
    for (r, s, ci, co), v, vm in _sample_wgrad(xp[0], dyp[0], gen, groups=2):
        assert abs(float(dw[r, s, ci, co]) - v) <= _k_for(M) * vm, ("plane weight gradient", (r, s, ci, co), float(dw[r, s, ci, co]), v)
    del xp, dyp, dw
    _free()


# ---------------------------------------------------------------------------------------------------------------
# plane forward / input gradient (csrc/conv_planes.hip): nplanes*B*H*W*C*2 < 2^31 + H*W*C*2 for the input planes.  No other
# kernel takes plane operands, so this is the largest batch of a plane layer: the test runs it and asserts the clear error
# one image later.
# ---------------------------------------------------------------------------------------------------------------
PLANE_H, PLANE_C = 32, 64
PLANE_MAX_B = 16384            # one plane of 32 x 32 x 64: (2^31 + 131072) / 131072 - 1 images


def _plane_max_batch(nplanes, H, W, C):
    img = H * W * C * 2
    return ((1 << 31) + img - 1) // (nplanes * img)


@pytest.mark.parametrize("B", [PLANE_MAX_B, PLANE_MAX_B + 1], ids=["largest", "one_more"])
def test_plane_forward_at_its_largest_batch_and_the_error_past_it(B):
    """Peak 8.2 GB measured (the 2 GB plane and the 4.3 GB output)."""
    kk = K()
    H = W = PLANE_H
    assert _plane_max_batch(1, H, W, PLANE_C) == PLANE_MAX_B
    gen = _gen(B)
    xp = torch.randn(1, B, H, W, PLANE_C, device="cuda", generator=gen, dtype=torch.bfloat16)
    w = torch.randn(3, 3, PLANE_C, 64, device="cuda", generator=gen) / 24
    wf = kk.planes_split_weight(w, 1, 1, fwd=True, dgrad=False)[0]
    if B > PLANE_MAX_B:
        with pytest.raises(RuntimeError, match="tensor too large for 32-bit plane offsets"):
            kk.conv2d_fwd_planes(xp, wf, 3, 3, 1, 1, 1)
    else:
        (y, (part, rows)), names = _profiled(lambda: kk.conv2d_fwd_planes(xp, wf, 3, 3, 1, 1, 1, bn_stats=True))
        assert "pconv_fwd<bf16>" in names, names
        _check_sampled("plane forward", y, lambda idx: _sample_fwd(xp[0], w, idx, bf16=True), gen, _k_for(576))
        _check_stats(y, part, rows)
        del y, part
    del xp, wf
    _free()


@pytest.mark.parametrize("B", [PLANE_MAX_B, PLANE_MAX_B + 1], ids=["largest", "one_more"])
def test_plane_input_gradient_at_its_largest_batch_and_the_error_past_it(B):
    """Peak 6.1 GB measured (the 2 GB gradient plane and the 4.3 GB input gradient)."""
    kk = K()
    H = W = PLANE_H
    gen = _gen(B + 1)
    dyp = torch.randn(1, B, H, W, PLANE_C, device="cuda", generator=gen, dtype=torch.bfloat16)
    w = torch.randn(3, 3, 64, PLANE_C, device="cuda", generator=gen) / 24
    wd = kk.planes_split_weight(w, 1, 1, fwd=False, dgrad=True)[1]
    if B > PLANE_MAX_B:
        with pytest.raises(RuntimeError, match="tensor too large for 32-bit plane offsets"):
            kk.conv2d_dgrad_planes(dyp, wd, (B, H, W, 64), 3, 3, 1, 1, 1)
    else:
        dx, names = _profiled(lambda: kk.conv2d_dgrad_planes(dyp, wd, (B, H, W, 64), 3, 3, 1, 1, 1))
        assert "pconv_dgrad<bf16>" in names, names
        _check_sampled("plane input gradient", dx, lambda idx: _sample_dgrad(dyp[0], w, idx, bf16=True), gen, _k_for(576))
        del dx
    del dyp, wd
    _free()


# ---------------------------------------------------------------------------------------------------------------
# The route queries against the entry points themselves, at a size that costs nothing (B = 2, 8 x 8 maps): for every tile that
# is an ERROR when named where it does not apply, query 1 <=> the call runs that tile's kernel and matches fp64 (the bound of
# this file: _k_for relative to V), query 0 <=> the call returns the library's "unsupported" error -- before any launch.  For
# the hint tiles 0-3, query 0 <=> the profiler shows that another tile ran.  fp32 tile 4 is BOTH: a hint on a shape it does
# not cover (96 -> 128: another tile runs, on either pass), an error on a covered shape with an epilogue that is not its own
# (the forward with bias / addend / ReLU; the input gradient has no such epilogue, so naming its tile 4 never raises).  (tests/test_route_queries_cpu.py asks the same
# queries at the thresholds, without a device.)
# ---------------------------------------------------------------------------------------------------------------
QB, QH = 2, 8
EPI_BIAS, EPI_ADDEND, EPI_RELU, EPI_STATS, EPI_BWD = 1, 2, 4, 8, 16


def _full_ref(a, w, pad, dgrad, bf16):
    """fp64 convolution (dgrad: transposed) of NHWC `a` with HWIO `w` (stride 1, groups 1) and V = sqrt(sum of squared terms);
    bf16: both operands as the bf16-input kernels round them"""
    import torch.nn.functional as F
    op = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
    a64, w64 = op(a).permute(0, 3, 1, 2), op(w).permute(3, 2, 0, 1)          # NCHW, OIHW
    f = (lambda u, v: F.conv_transpose2d(u, v, padding=pad)) if dgrad else (lambda u, v: F.conv2d(u, v, padding=pad))
    return f(a64, w64).permute(0, 2, 3, 1), f(a64 * a64, w64 * w64).sqrt().permute(0, 2, 3, 1)


def _raw(fn_name, *args):
    from scouter_amd import _native
    _native.check(getattr(_native.lib(), fn_name)(*args), fn_name)


def _route_case(name, cin, cout):
    """-> (query name, query arguments after the shape, run() -> the result tensor, dgrad, bf16 operands, kernel name, K, pad)
    for the GEMM cin -> cout (an input gradient's layer has the channels exchanged)"""
    kk = K()
    from scouter_amd import kernels as k_
    p, st = k_._p, k_._stream
    gen = _gen(cin * 7 + cout + len(name))
    rnd = lambda *s, dtype=torch.float32: torch.randn(*s, device="cuda", generator=gen).to(dtype)
    if name in ("fwd tile 4", "fwd tile 5", "fwd tile 4 + relu", "fwd tile 4 + addend", "fwd tile 5 + bias"):
        tile = 4 if "4" in name else 5
        x, w = rnd(QB, QH, QH, cin), rnd(1, 1, cin, cout) / 8
        bias = rnd(cout) if "bias" in name else None
        add = rnd(QB, QH, QH, cout) if "addend" in name else None
        relu = int("relu" in name)
        y = torch.empty(QB, QH, QH, cout, device="cuda")
        run = lambda: (_raw("scouter_conv2d_fwd_f32", p(x), p(w), p(bias), p(add), p(y), None, QB, QH, QH, cin, cout, 1, 1, 1, 0, 1,
                            relu, tile, st()), y)[1]
        epi = (EPI_BIAS if bias is not None else 0) | (EPI_ADDEND if add is not None else 0) | (EPI_RELU if relu else 0)
        return ("fwd_tile_ok", (QB, QH, QH, cin, cout, 1, 1, 1, 0, 1, tile, epi), run, (x, w, 0, False, False),
                "igemm_fwd<persistent>" if tile == 4 else "xpw_fwd<bf16x3>")
    if name in ("dgrad tile 4", "dgrad tile 5", "dgrad tile 5 plain"):
        tile = 4 if "4" in name else 5
        Cin, Cout = cout, cin                                                   # (GEMM-K of the input gradient = Cout)
        dy, w = rnd(QB, QH, QH, Cout), rnd(1, 1, Cin, Cout) / 8
        dx = torch.empty(QB, QH, QH, Cin, device="cuda")
        fused = tile == 5 and "plain" not in name
        x1 = rnd(QB, QH, QH, Cin) if fused else None
        saved = torch.stack([torch.zeros(Cin), torch.ones(Cin), torch.ones(Cin), torch.zeros(Cin)]).cuda() if fused else None
        shape = (QB, QH, QH, Cin, Cout, 1, 1, 1, 0, 1)
        part = torch.zeros(max(kk.ask("dgrad_bn_partial_rows", *shape, tile), 1), Cin, 2, dtype=torch.float64, device="cuda") if fused else None
        run = lambda: (_raw("scouter_conv2d_dgrad_bnbwd_f32", p(dy), p(w), None, p(dx), *shape, tile, None, p(x1), p(saved), p(part),
                            None, None, None, st()), dx)[1]
        return ("dgrad_tile_ok", (*shape, tile, EPI_BWD if fused else 0), run, (dy, w, 0, True, False),
                {4: "igemm_dgrad<persistent>", 5: "xpw_dgrad+bn_bwd<bf16x3>"}[tile])
    if name in ("typed fwd tile 4", "typed fwd tile 4, x fp32"):
        io = 0 if "fp32" in name else 1
        x, w = rnd(QB, QH, QH, cin, dtype=torch.float32 if not io else torch.bfloat16), rnd(1, 1, cin, cout) / 8
        wt = kk.weight_bf16t(w)
        y = torch.empty(QB, QH, QH, cout, device="cuda")
        shape = (QB, QH, QH, cin, cout, 1, 1, 1, 0, 1)
        run = lambda: (_raw("scouter_conv2d_fwd_bf16_io", p(x), p(wt), None, None, p(y), None, *shape, 0, 4, io, st()), y)[1]
        return ("fwd_bf16_tile_ok", (*shape, 4, 0, io, 0), run, (x.float(), w, 0, False, True), "igemm_fwd_bf16<persistent>")
    if name in ("typed dgrad tile 4 plain", "typed dgrad tile 4 plain, dy fp32", "typed dgrad tile 4 fused", "typed dgrad tile 4 fused, x1 fp32"):
        Cin, Cout = cout, cin
        fused = "fused" in name
        io = (0 if "dy fp32" in name else 8) | (16 if fused else 0) | (1 if fused and "x1 fp32" not in name else 0)
        dy = rnd(QB, QH, QH, Cout, dtype=torch.bfloat16 if io & 8 else torch.float32)
        w = rnd(1, 1, Cin, Cout) / 8
        dx = torch.empty(QB, QH, QH, Cin, device="cuda", dtype=torch.bfloat16 if io & 16 else torch.float32)
        x1 = rnd(QB, QH, QH, Cin, dtype=torch.bfloat16 if io & 1 else torch.float32) if fused else None
        saved = torch.stack([torch.zeros(Cin), torch.ones(Cin), torch.ones(Cin), torch.zeros(Cin)]).cuda() if fused else None
        shape = (QB, QH, QH, Cin, Cout, 1, 1, 1, 0, 1)
        part = torch.zeros(max(kk.ask("dgrad_bn_partial_rows_bf16", *shape, 4, 0), 1), Cin, 2, dtype=torch.float64, device="cuda") if fused else None
        run = lambda: (_raw("scouter_conv2d_dgrad_bnbwd_bf16_io", p(dy), p(w), None, p(dx), *shape, 4, None, p(x1), p(saved), p(part),
                            None, None, None, io, st()), dx)[1]
        return ("dgrad_bf16_tile_ok", (*shape, 4, EPI_BWD if fused else 0, io, 0), run, (dy.float(), w, 0, True, True),
                "igemm_dgrad_bf16<persistent>")
    if name in ("x3 fwd tile 7", "x3 fwd tile 7 + addend"):
        x, w = rnd(QB, QH, QH, cin), rnd(3, 3, cin, cout) / 24
        wf = kk.planes_split_weight(w, 1, 3, fwd=True, dgrad=False)[0]
        add = rnd(QB, QH, QH, cout) if "addend" in name else None
        y = torch.empty(QB, QH, QH, cout, device="cuda")
        run = lambda: (_raw("scouter_conv2d_fwd_x3", p(x), p(wf), None, p(add), p(y), None, QB, QH, QH, cin, cout, 3, 3, 1, 1, 0, 7,
                            st()), y)[1]
        return ("fwd_x3_tile_ok", (QB, QH, QH, cin, cout, 3, 3, 1, 1, 1, 7, EPI_ADDEND if add is not None else 0), run,
                (x, w, 1, False, False), "xhalo_fwd<bf16x3>")
    if name == "x3 dgrad tile 7":
        Cin, Cout = cout, cin
        dy, w = rnd(QB, QH, QH, Cout), rnd(3, 3, Cin, Cout) / 24
        wd = kk.planes_split_weight(w, 1, 3, fwd=False, dgrad=True)[1]
        dx = torch.empty(QB, QH, QH, Cin, device="cuda")
        run = lambda: (_raw("scouter_conv2d_dgrad_x3_bnbwd", p(dy), p(wd), None, p(dx), QB, QH, QH, Cin, Cout, 3, 3, 1, 1, 7, None,
                            None, None, None, None, None, None, st()), dx)[1]
        return ("dgrad_x3_tile_ok", (QB, QH, QH, Cin, Cout, 3, 3, 1, 1, 1, 7, 0), run, (dy, w, 1, True, False),
                "xhalo_dgrad<bf16x3>")
    assert name in ("plane tile 6", "plane tile 6, bf16 output"), name
    out = torch.bfloat16 if "bf16" in name else torch.float32
    x, w = rnd(QB, QH, QH, cin), rnd(3, 3, cin, cout) / 24
    xp, wf = kk.planes_split(x, 3), kk.planes_split_weight(w, 1, 3, fwd=True, dgrad=False)[0]
    run = lambda: kk.conv2d_fwd_planes(xp, wf, 3, 3, 1, 1, 1, tile=6, out_dtype=out)
    return ("fwd_planes_tile_ok", (QB, QH, QH, cin, cout, 3, 3, 1, 1, 1, 3, 6, 0, 2 if out == torch.bfloat16 else 0), run,
            (x, w, 1, False, False), "pconv_fwd<bf16x3>")


ROUTE_CASES = [  # (case, GEMM K -> N, the query's answer; "hint": 0, and the library runs another tile instead of refusing)
    ("fwd tile 4", 64, 128, 1), ("fwd tile 4", 96, 128, "hint"), ("fwd tile 4 + relu", 64, 128, 0), ("fwd tile 4 + addend", 64, 128, 0),
    ("fwd tile 5", 64, 128, 1), ("fwd tile 5", 96, 128, 0), ("fwd tile 5 + bias", 64, 128, 0),
    ("dgrad tile 4", 64, 128, 1), ("dgrad tile 4", 96, 128, "hint"),
    ("dgrad tile 5", 64, 128, 1), ("dgrad tile 5", 96, 128, 0), ("dgrad tile 5 plain", 64, 128, 0),
    ("typed fwd tile 4", 64, 128, 1), ("typed fwd tile 4", 96, 128, 0), ("typed fwd tile 4, x fp32", 64, 128, 0),
    ("typed dgrad tile 4 plain", 64, 128, 1), ("typed dgrad tile 4 plain", 96, 128, 0), ("typed dgrad tile 4 plain, dy fp32", 64, 128, 0),
    ("typed dgrad tile 4 fused", 64, 128, 1), ("typed dgrad tile 4 fused", 96, 128, 0), ("typed dgrad tile 4 fused, x1 fp32", 64, 128, 0),
    ("x3 fwd tile 7", 64, 32, 1), ("x3 fwd tile 7", 64, 128, 0), ("x3 fwd tile 7 + addend", 64, 32, 0),
    ("x3 dgrad tile 7", 64, 32, 1), ("x3 dgrad tile 7", 64, 128, 0),
    ("plane tile 6", 64, 128, 1), ("plane tile 6, bf16 output", 64, 128, 0),
]


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: "%s_%dto%d" % (c[0].replace(" ", "_").replace(",", "").replace("+", "and"), c[1], c[2]))   # noqa: E501
def test_named_tile_runs_where_its_query_says_so_and_is_refused_where_not(case):
    """Tile 7 and the plane tile need 32 / 64 GEMM columns: their accepted shapes are 64 -> 32 and 64 -> 128, refused 64 -> 128 (tile
    7) and the bf16-stored output (plane tile 6).  A bf16-stored result (the typed fused input gradient) adds its storage
    rounding -- at most half a bf16 ulp, the unit roundoff 2^-8 of its 8-bit significand, of the value -- to the bound."""
    name, cin, cout, want = case
    kk = K()
    query, qargs, run, (a, w, pad, dgrad, bf16), kernel = _route_case(name, cin, cout)
    assert kk.ask(query, *qargs) == (1 if want == 1 else 0), (query, qargs)
    if want == 0:
        with pytest.raises(RuntimeError, match="rc=-3"):            # SC_ERR_UNSUPPORTED
            _, names = _profiled(run)
        return
    out, names = _profiled(run)
    if want == "hint":
        assert len(names) == 1 and names[0] != kernel and names[0].startswith(kernel.split("<")[0] + "<"), names
    else:
        assert kernel in names, names
    ref, mag = _full_ref(a, w, pad, dgrad, bf16)
    k = _k_for(a.shape[-1] * w.shape[0] * w.shape[1])
    if out.dtype == torch.bfloat16:
        mag = mag + ref.abs() * 2.0 ** -8 / k
    _check(name, out, ref, mag, k)


@pytest.mark.parametrize("cout", [96, 64, 128])
def test_hint_tiles_run_where_their_query_says_so_and_another_tile_where_not(cout):
    """Tiles 0-3 of the fp32 forward and input gradient are hints: a tile that does not divide the GEMM columns (the forward's
    output channels, the input gradient's input channels) is replaced, never refused -- and the query tells which.  (The typed
    kernels share the rule, sc_igemm_tile_ok; tests/test_route_queries_cpu.py asks their queries.)"""
    kk = K()
    gen = _gen(cout)
    x = torch.randn(QB, QH, QH, 64, device="cuda", generator=gen)
    w = torch.randn(1, 1, 64, cout, device="cuda", generator=gen) / 8
    ref, mag = _full_ref(x, w, 0, False, False)
    fwd_names = ["igemm_fwd<128x128>", "igemm_fwd<128x64>", "igemm_fwd<64x64>", "igemm_fwd<128x32>"]
    for t in range(4):
        y, names = _profiled(lambda: kk.conv2d_fwd(x, w, tile=t))
        assert (fwd_names[t] in names) == bool(kk.ask("fwd_tile_ok", QB, QH, QH, 64, cout, 1, 1, 1, 0, 1, t, 0)), (t, names)
        assert len(names) == 1 and names[0] in fwd_names, names
        _check("forward, tile hint %d" % t, y, ref, mag, _k_for(64))
    from scouter_amd import kernels as k_
    dy = torch.randn(QB, QH, QH, 64, device="cuda", generator=gen)
    wd = torch.randn(1, 1, cout, 64, device="cuda", generator=gen) / 8          # the layer cout -> 64: `cout` GEMM columns
    dx = torch.empty(QB, QH, QH, cout, device="cuda")
    ref, mag = _full_ref(dy, wd, 0, True, False)
    shape = (QB, QH, QH, cout, 64, 1, 1, 1, 0, 1)
    for t in range(4):
        _, names = _profiled(lambda: _raw("scouter_conv2d_dgrad_f32", k_._p(dy), k_._p(wd), None, k_._p(dx), *shape, t, k_._stream()))
        assert (fwd_names[t].replace("fwd", "dgrad") in names) == bool(kk.ask("dgrad_tile_ok", *shape, t, 0)), (t, names)
        assert len(names) == 1 and names[0].replace("dgrad", "fwd") in fwd_names, names
        _check("input gradient, tile hint %d" % t, dx, ref, mag, _k_for(64))


def test_plane_call_no_tile_admits_reaches_the_entry_point_for_its_error():
    """A plane convolution whose shape no tile's query accepts (96 output channels: not a 64-multiple per group) is still handed
    to the entry point, which says why -- as past the size guard at 16 385 images above."""
    kk = K()
    gen = _gen(96)
    x = torch.randn(QB, QH, QH, 64, device="cuda", generator=gen)
    w = torch.randn(3, 3, 64, 96, device="cuda", generator=gen) / 24
    xp = kk.planes_split(x, 3)
    wf = torch.zeros(3, 9, 96, 64, device="cuda", dtype=torch.bfloat16)
    assert not any(kk.ask("fwd_planes_tile_ok", QB, QH, QH, 64, 96, 3, 3, 1, 1, 1, 3, t, 0, 0) for t in range(7))
    with pytest.raises(RuntimeError, match="Cout/groups % 64 == 0"):
        kk.conv2d_fwd_planes(xp, wf, 3, 3, 1, 1, 1)
    dyp = kk.planes_split(torch.randn(QB, QH, QH, 64, device="cuda", generator=gen), 3)
    wd = torch.zeros(3, 9, 96, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="Cin/groups % 64 == 0"):
        kk.conv2d_dgrad_planes(dyp, wd, (QB, QH, QH, 96), 3, 3, 1, 1, 1)
