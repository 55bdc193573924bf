"""Layer IG, layer conductance, HiResCAM and LayerCAM at the backbone's output (-m gpu): the three kernels of csrc/layerattr.hip
against the float64 restatements of tests/layer_restatements.py with derived bounds, their refusals, the four methods of
tools/attribution.py on whole models -- against the CPU oracle under fp64 and fp32 autograd (the project's rule), against the
definition over the HIP path's own gradients (the kernels' bounds), and completeness -- and scouter_amd/tools/layer.py in both modes.

Bounds.  u = 2^-53.  A float64 sum of n terms in any order is within (n - 1) u sum|terms| (1 + O(n u)); forming a term costs one or
two roundings more.  So: conductance_accumulate within (r + 2) u (|acc0| + sum|terms|); a position's channel sum within
(C + 2) u sum|terms|, plus 2^-24 |ref| for the one rounding to fp32; an attribution within 2^-24 |ref| + 2 u |ref|; a class total
within (P C + 2) u sum|terms|."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import layer_restatements as R                                              # noqa: E402
from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import MODEL_CASES, LAMBDA, model_inputs             # noqa: E402

U = 2.0 ** -53
SENTINEL = -777.25
SHAPES = [(1, 1, 1, 0), (2, 3, 5, 0), (2, 2, 512, 0), (9, 9, 64, 0), (7, 7, 2048, 0), (2, 3, 8, 1)]     # (h, w, C, elements off 16 bytes)
SHAPE_IDS = ["x".join(str(v) for v in s[:3]) + ("_off" if s[3] else "") for s in SHAPES]


def dev(t, off=0, tail=0):
    """t on the device inside a longer buffer: `off` elements past the buffer's (16-byte aligned) start and with `tail` sentinel
    elements behind it -> (the view, the tail)"""
    flat = torch.full((off + t.numel() + tail,), SENTINEL, dtype=t.dtype, device="cuda")
    flat[off:off + t.numel()] = t.flatten().cuda()
    return flat[off:off + t.numel()].view(t.shape), flat[off + t.numel():]


def rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ 1: conductance_accumulate
def check_conductance(shape, r, seed=0):
    from scouter_amd import kernels as K
    h, w, C, off = shape
    feats, grads = rand((r, h, w, C), 100 + seed), rand((r, h, w, C), 200 + seed)
    acc0 = rand((h, w, C), 300 + seed, torch.float64)
    feats.view(-1)[0] = -0.0
    grads[-1] = float("nan")                                                # the last row's gradient is not read
    ref, mag = R.conductance_accumulate(feats, grads, acc0)
    fd, _ = dev(feats, off)
    gd, _ = dev(grads, off)
    acc, tail = dev(acc0, off, 8)
    assert (fd.data_ptr() % 16 != 0) == bool(off) and (acc.data_ptr() % 16 != 0) == bool(off)
    K.conductance_accumulate(fd, gd, acc)
    torch.cuda.synchronize()
    assert bool((tail == SENTINEL).all())
    got = acc.cpu()
    assert bool(torch.isfinite(got).all())
    err, bound = (got - ref).abs(), (r + 2) * U * mag
    print("conductance_accumulate", shape, "r", r, "max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    # two calls that share a row, and a repeat: the same bits
    again, _ = dev(acc0, off)
    K.conductance_accumulate(fd, gd, again)
    assert torch.equal(again, acc)
    if r >= 3:
        for m in {1, r // 2, r - 2}:
            split, _ = dev(acc0, off)
            K.conductance_accumulate(fd[:m + 1], gd[:m + 1], split)
            K.conductance_accumulate(fd[m:], gd[m:], split)
            assert torch.equal(split, acc), (shape, r, m)


@pytest.mark.parametrize("r", [2, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conductance_accumulate_against_fp64(shape, r):
    check_conductance(shape, r)


# ------------------------------------------------------------------------------------------------ 2: layer_attr_finish
def check_finish(shape, Kc, path, seed=0):
    from scouter_amd import kernels as K
    h, w, C, off = shape
    P = h * w
    acc = rand((Kc, h, w, C), 400 + seed, torch.float64)
    feat, base = rand((h, w, C), 500 + seed), rand((h, w, C), 600 + seed)
    acc[:, 0, 0] = 0.0                                                      # a position whose every term is 0
    if path and P > 1:
        base[-1, -1] = feat[-1, -1]                                         # ... and one where feat - base is
        feat.view(-1)[0] = -0.0
    want = R.layer_attr_finish(acc.view(Kc, P, C), feat.view(P, C) if path else None, base.view(P, C) if path else None)
    ad, _ = dev(acc, off)
    fd, bd = (dev(feat, off)[0], dev(base, off)[0])
    out, out_tail = dev(torch.zeros((Kc, h, w)), 0, 8)
    attr, attr_tail = dev(torch.zeros((Kc, h, w, C)), off, 8)
    total, total_tail = dev(torch.zeros(Kc, dtype=torch.float64), 0, 4)
    mode = K.LAYER_PATH if path else K.LAYER_SUM
    # (mode SUM ignores feat and base: given or not, the same bits)
    K.layer_attr_finish(mode, ad, out, feat=fd if path or seed else None, base=bd if path or seed else None, attr=attr, total=total)
    torch.cuda.synchronize()
    for t in (out_tail, attr_tail, total_tail):
        assert bool((t == SENTINEL).all())
    got, got_attr, got_total = out.cpu().double().view(Kc, P), attr.cpu().double().view(Kc, P, C), total.cpu()
    err, bound = (got - want["map"]).abs(), 2.0 ** -24 * want["map"].abs() + (C + 2) * U * want["map_mag"]
    aerr, abound = (got_attr - want["terms"]).abs(), (2.0 ** -24 + 2.0 ** -52) * want["terms"].abs()
    terr, tbound = (got_total - want["total"]).abs(), (P * C + 2) * U * want["total_mag"]
    print("layer_attr_finish", shape, "K", Kc, "path" if path else "sum", "map err / bound %.3f, attr %.3f, total %.3f (max total err %.3e)"
          % (float((err / bound.clamp_min(1e-300)).max()), float((aerr / abound.clamp_min(1e-300)).max()),
             float((terr / tbound).max()), float(terr.max())))
    assert bool((err <= bound).all()) and bool((aerr <= abound).all()) and bool((terr <= tbound).all())
    assert bool((got[:, 0] == 0.0).all())                                   # exactly 0 where every term is 0
    if path and P > 1:
        assert bool((got[:, -1] == 0.0).all())
    # a second call, and a call without attr and total: the same bits; base None is a base of zeros
    out2, attr2, total2 = torch.empty_like(out), torch.empty_like(attr), torch.empty_like(total)
    K.layer_attr_finish(mode, ad, out2, feat=fd, base=bd, attr=attr2 if not off else None, total=total2)
    assert torch.equal(out2, out) and torch.equal(total2, total) and (bool(off) or torch.equal(attr2, attr))
    out3 = torch.empty_like(out)
    K.layer_attr_finish(mode, ad, out3, feat=fd, base=bd)
    assert torch.equal(out3, out)
    if path:
        zeros, _ = dev(torch.zeros((h, w, C)), off)
        a, b, ta, tb = torch.empty_like(out), torch.empty_like(out), torch.empty_like(total), torch.empty_like(total)
        K.layer_attr_finish(mode, ad, a, feat=fd, base=None, total=ta)
        K.layer_attr_finish(mode, ad, b, feat=fd, base=zeros, total=tb)
        assert torch.equal(a, b) and torch.equal(ta, tb)


@pytest.mark.parametrize("path", [True, False], ids=["path", "sum"])
@pytest.mark.parametrize("Kc", [1, 3, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_layer_attr_finish_against_fp64(shape, Kc, path):
    check_finish(shape, Kc, path)


# ------------------------------------------------------------------------------------------------ 3: layer_gxa
def check_gxa(shape, rectify, relu, B=2, seed=0):
    from scouter_amd import kernels as K
    h, w, C, off = shape
    P = h * w
    feat, dfeat = rand((B, h, w, C), 700 + seed), rand((B, h, w, C), 800 + seed)
    feat[-1, -1, -1] = 0.0                                                  # a position whose every term is 0
    dfeat.view(-1)[0] = -0.0
    feat.view(-1)[min(1, feat.numel() - 1)] = -0.0
    ref, mag = R.layer_gxa(feat.view(B, P, C), dfeat.view(B, P, C), rectify, relu)
    fd, _ = dev(feat, off)
    dd, _ = dev(dfeat, off)
    full = torch.full((B, 3, h, w), SENTINEL, device="cuda")
    K.layer_gxa(fd, dd, full[:, 1], rectify=rectify, relu=relu)
    again, tail = dev(torch.zeros((B, P)), off, 8)
    K.layer_gxa(fd, dd, again, rectify=rectify, relu=relu)
    torch.cuda.synchronize()
    got = full[:, 1].reshape(B, P)
    assert torch.equal(got, again)                                          # two calls, two output strides: the same bits
    assert bool((full[:, 0] == SENTINEL).all()) and bool((full[:, 2] == SENTINEL).all()) and bool((tail == SENTINEL).all())
    got = got.cpu().double()
    err, bound = (got - ref).abs(), 2.0 ** -24 * ref.abs() + (C + 2) * U * mag
    print("layer_gxa", shape, "rectify", rectify, "relu", relu, "max err %.3e, max err / bound %.3f"
          % (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    assert float(got[-1, -1]) == 0.0
    if relu:
        assert bool((got >= 0).all())


@pytest.mark.parametrize("rectify,relu", [(False, False), (True, True), (True, False), (False, True)],
                         ids=["hirescam", "layercam", "rectify", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_layer_gxa_against_fp64(shape, rectify, relu):
    check_gxa(shape, rectify, relu)


# ------------------------------------------------------------------------------------------------ 4: refusals
REFUSALS = [(call, bad) for call, bads in [
    ("conductance_accumulate", ["null", "misaligned", "r1", "p0", "c0", "wrong_dtype", "wrong_shape"]),
    ("layer_attr_finish", ["null", "misaligned", "k0", "p0", "c0", "bad_mode", "wrong_dtype", "wrong_shape"]),
    ("layer_gxa", ["null", "misaligned", "b0", "p0", "c0", "small_stride", "wrong_dtype", "wrong_shape"])] for bad in bads]


@pytest.mark.parametrize("call,bad", REFUSALS, ids=["%s-%s" % r for r in REFUSALS])
def test_the_kernels_refuse_bad_arguments(call, bad):
    """error returns with nothing launched: an error that names the call from the library itself and from the wrapper, the
    sentinel-filled outputs untouched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    lib = _native.lib()
    r, h, w, C, Kc, B = 3, 2, 3, 8, 2, 2
    feats = torch.ones((r, h, w, C), device="cuda")
    grads = torch.ones((r, h, w, C), device="cuda")
    acc = torch.full((h, w, C), SENTINEL, dtype=torch.float64, device="cuda")
    sums = torch.ones((Kc, h, w, C), dtype=torch.float64, device="cuda")
    out = torch.full((Kc, h, w), SENTINEL, device="cuda")
    attr = torch.full((Kc, h, w, C), SENTINEL, device="cuda")
    total = torch.full((Kc,), SENTINEL, dtype=torch.float64, device="cuda")
    cam = torch.full((B, h, w), SENTINEL, device="cuda")
    odd = 2 if bad == "misaligned" else 0
    P_ = 0 if bad == "p0" else h * w
    C_ = 0 if bad == "c0" else C

    def ptr(t, null=False):
        return None if null and bad == "null" else t.data_ptr()

    def direct():
        if call == "conductance_accumulate":
            return lib.scouter_conductance_accumulate_f64(ptr(feats), ptr(grads, True) and ptr(grads) + odd, ptr(acc),
                                                          1 if bad == "r1" else r, P_, C_, None)
        if call == "layer_attr_finish":
            return lib.scouter_layer_attr_finish_f32(ptr(feats[0]), None, ptr(sums, True) and ptr(sums) + 2 * odd, ptr(out), ptr(attr),
                                                     ptr(total), 0 if bad == "k0" else Kc, P_, C_, 2 if bad == "bad_mode" else 0, None)
        return lib.scouter_layer_gxa_f32(ptr(feats[:B]), ptr(grads[:B], True) and ptr(grads[:B]) + odd, ptr(cam), 0 if bad == "b0" else B,
                                         P_, C_, h * w - 1 if bad == "small_stride" else h * w, 0, 0, None)

    def wrapped():
        wrong = bad == "wrong_dtype"
        if call == "conductance_accumulate":
            n = 1 if bad == "r1" else r
            f, g = (feats[:n, :, :0], grads[:n, :, :0]) if bad == "p0" else (feats[:n, ..., :0], grads[:n, ..., :0]) if bad == "c0" \
                else (feats[:n], grads[:n])
            a = acc[:, :0] if bad == "p0" else acc[..., :0] if bad == "c0" else acc
            if bad == "wrong_shape":
                g = grads[:n, :, :, :C - 1].contiguous()
            return K.conductance_accumulate(f.contiguous(), g.double() if wrong else g.contiguous(), a.contiguous())
        if call == "layer_attr_finish":
            k = 0 if bad == "k0" else Kc
            s = sums[:k, :, :0] if bad == "p0" else sums[:k, ..., :0] if bad == "c0" else sums[:k]
            o = out[:k, :, :0] if bad == "p0" else out[:k]
            f = feats[0, :, :0] if bad == "p0" else feats[0, ..., :0] if bad == "c0" else feats[0]
            if bad == "wrong_shape":
                o = out[:k, :, :w - 1].contiguous()
            return K.layer_attr_finish(2 if bad == "bad_mode" else K.LAYER_PATH, s.float() if wrong else s.contiguous(), o.contiguous(),
                                       feat=f.contiguous(), attr=None if bad in ("p0", "c0", "k0") else attr,
                                       total=None if bad == "k0" else total)
        b = 0 if bad == "b0" else B
        f, g = (feats[:b, :, :0], grads[:b, :, :0]) if bad == "p0" else (feats[:b, ..., :0], grads[:b, ..., :0]) if bad == "c0" \
            else (feats[:b], grads[:b])
        o = cam[:b, :, :0] if bad == "p0" else cam[:b]
        if bad == "wrong_shape":
            g = grads[:b, :, :, :C - 1].contiguous()
        if bad == "small_stride":
            o = cam.view(-1)[:(B - 1) * (h * w - 1) + h * w].as_strided((B, h * w), (h * w - 1, 1))
        return K.layer_gxa(f.contiguous(), g.double() if wrong else g.contiguous(), o if bad == "small_stride" else o.contiguous())

    if bad not in ("wrong_dtype", "wrong_shape"):                           # (dtypes and shapes: the wrapper's business alone)
        with pytest.raises(RuntimeError, match=call):
            _native.check(direct(), call)
    if bad not in ("null", "misaligned"):                                   # (a tensor has a pointer, and torch aligns it)
        with pytest.raises((RuntimeError, ValueError), match=call):
            wrapped()
    torch.cuda.synchronize()
    for t in (acc, out, attr, total, cam):
        assert bool((t == SENTINEL).all())
    check_conductance(SHAPES[1], 3, seed=1)
    check_finish(SHAPES[1], 3, True, seed=1)
    check_finish(SHAPES[1], 3, False, seed=1)
    check_gxa(SHAPES[1], True, True, seed=1)


# ------------------------------------------------------------------------------------------------ 5: whole models
N_STEPS = 8
CASES = ["resnet18_mnist_64", "resnest26d_96", "fc_resnet18_mnist_64"]


def model_args(arch, C, spc, L, ls, power, mnist, use_slot=True):
    return argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=use_slot, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=ls,
                              power=power, to_k_layer=L, lambda_value=LAMBDA)


def build(case):
    """-> (model on the device, parameters, images, oracle head configuration or None for the FC baseline, architecture); the
    models and inputs of tests/test_gradcam_gpu.py"""
    from scouter_amd.sloter.slot_model import SlotModel
    if case == "fc_resnet18_mnist_64":
        spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
        P = O.synth_state(spec, 400)
        m = SlotModel(model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=False))
        m.load_state_dict(P)
        images, _ = O.synth_batch(4, 1, 64, 10, 401)
        return m.cuda(), P, images, None, "resnet18"
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist))
    m.load_state_dict(P)
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=float(LAMBDA))
    return m.cuda(), P, images, cfg, arch


def check_rule(what, mine, ref64, ref32, kf=2.0, ks=1e-3):
    """the project's per-tensor rule: |HIP - fp64| <= max(2 |torch fp32 - fp64|, 1e-3 max|fp64|)"""
    mine = mine.detach().cpu().double()
    assert mine.shape == ref64.shape, (what, mine.shape, ref64.shape)
    assert bool(torch.isfinite(mine).all())
    scale = float(ref64.abs().max())
    e = float((mine - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    print("%s: |HIP - fp64| = %.3e, |torch fp32 - fp64| = %.3e, max|.| = %.3e" % (what, e, e32, scale))
    assert scale > 0
    assert e <= max(kf * e32, ks * scale) + 1e-12, (what, e, e32, scale)


def bn_buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def oracle_parts(P, cfg, arch, dtype):
    """-> (backbone: images [n, Cin, H, W] -> NHWC features, head: NHWC features -> log-probabilities), the oracle in `dtype`"""
    Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}

    def backbone(x):
        with torch.no_grad():
            return O.backbone_features(Pd, x.to(dtype), arch, training=False).permute(0, 2, 3, 1).contiguous()

    def head(feats):
        feat = feats.permute(0, 3, 1, 2)
        if cfg is not None:
            return O.head_forward(Pd, feat, None, cfg)
        return F.log_softmax(F.linear(feat.mean(dim=(2, 3)), Pd["backbone.fc.weight"], Pd["backbone.fc.bias"]), dim=1)

    return backbone, head


_ORACLE = {}         # case -> the oracle's results in (fp64, fp32): one run per model, shared and left unchanged


def oracle_results(case, P, images, cfg, arch, n_classes):
    """per dtype a dict: lig / lig_gap for every image, cond / cond_gap for image 0, hires / lcam for every image, and the
    differences of the outputs at the ends of the paths (the zero baseline, N_STEPS steps, the library's quadrature table)"""
    from scouter_amd.tools.attribution import ig_quadrature
    if case not in _ORACLE:
        alphas, weights = ig_quadrature(N_STEPS, "gausslegendre")
        cols, res = list(range(n_classes)), []
        for dtype in (torch.float64, torch.float32):
            backbone, head = oracle_parts(P, cfg, arch, dtype)
            B = images.shape[0]
            feats = backbone(torch.cat([torch.zeros_like(images[:1]), images]))
            a0, A = feats[0], feats[1:]
            lig = [R.layer_integrated_gradients(head, a0, A[b], alphas, weights, cols) for b in range(B)]
            steps = torch.arange(N_STEPS + 1, dtype=torch.float64).to(dtype) / N_STEPS
            cond = R.layer_conductance(head, backbone(steps[:, None, None, None] * images[0].to(dtype)[None]), cols)
            g, out = R.head_gradients(head, A, cols)                        # [K, B, h, w, C]
            hires = (g * A[None]).sum(dim=4).permute(1, 0, 2, 3)
            lcam = (g.clamp_min(0.0) * A[None]).sum(dim=4).clamp_min(0.0).permute(1, 0, 2, 3)
            with torch.no_grad():
                ends = out - head(a0[None])
            res.append(dict(lig=torch.stack([a.sum(dim=3) for a, _ in lig]), lig_gap=torch.stack([gap for _, gap in lig]),
                            cond=cond[0].sum(dim=3), cond_gap=cond[1], hires=hires, lcam=lcam, ends=ends))
        _ORACLE[case] = tuple(res)
    return _ORACLE[case]


def one_hot(shape, c):
    seed = torch.zeros(shape, device="cuda")
    seed[:, c] = 1.0
    return seed


def own_layer_ig(m, x, base_rows, alphas, weights, cols):
    """the definition over the HIP path's own passes, summed in float64 on the host: per image (terms [K, h, w, C], their
    magnitudes with the error of the float64 accumulation folded in)"""
    from scouter_amd import kernels as K
    nb = base_rows.shape[0]
    feats = m.feature_pass(torch.cat([base_rows, x])).features
    res = []
    for b in range(x.shape[0]):
        a0, a1 = feats[b if nb > 1 else 0], feats[nb + b]
        rows = K.path_images(a1, a0, alphas.cuda(), torch.empty((alphas.shape[0],) + tuple(a0.shape), device="cuda"), 0)
        fp = m.head_pass(rows)
        g = torch.stack([fp.grad(one_hot(fp.log_probs.shape, c)) for c in cols]).cpu().double()          # [K, n, h, w, C]
        wg = weights.double()[None, :, None, None, None] * g
        diff = (a1.cpu().double() - a0.cpu().double())[None]
        res.append((diff * wg.sum(dim=1), diff.abs() * wg.abs().sum(dim=1)))
    return res


def own_conductance(m, x, base, n_steps, cols):
    from scouter_amd import kernels as K
    alphas = torch.from_numpy((np.arange(n_steps + 1, dtype=np.float64) / n_steps).astype(np.float32)).cuda()
    res = []
    for b in range(x.shape[0]):
        rows = K.path_images(x[b], None if base is None else base[b], alphas, torch.empty((n_steps + 1,) + tuple(x[b].shape), device="cuda"), 0)
        fp = m.feature_pass(rows)
        f = fp.features.cpu().double()
        g = torch.stack([fp.grad(one_hot(fp.log_probs.shape, c)) for c in cols]).cpu().double()
        terms = g[:, :-1] * (f[1:] - f[:-1])[None]
        res.append((terms.sum(dim=1), terms.abs().sum(dim=1)))
    return res


def check_own(what, maps, attr, delta_sum, own, n_terms):
    """the method's maps [B, K, h, w], attributions [B, K, h, w, C] and float64-summed totals against the definition over the
    path's own gradients: the kernels' bounds, with the n_terms float64 additions of the accumulation folded in"""
    for b, (terms, mag) in enumerate(own):
        C = terms.shape[-1]
        ref, refmag = terms.sum(dim=3), mag.sum(dim=3)
        err = (maps[b].cpu().double() - ref).abs()
        bound = 2.0 ** -24 * ref.abs() + (C + n_terms + 4) * U * refmag
        aerr = (attr[b].cpu().double() - terms).abs()
        abound = (2.0 ** -24 + 2.0 ** -52) * terms.abs() + (n_terms + 4) * U * mag
        print("%s image %d: map err / bound %.3f, attr err / bound %.3f" % (what, b, float((err / bound.clamp_min(1e-300)).max()),
                                                                           float((aerr / abound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()) and bool((aerr <= abound).all()), what
        if delta_sum is not None:
            terr = (delta_sum[b] - terms.sum(dim=(1, 2, 3))).abs()
            assert bool((terr <= (terms[0].numel() + n_terms + 4) * U * mag.sum(dim=(1, 2, 3))).all()), what


@pytest.mark.parametrize("case", CASES)
def test_the_four_methods_on_whole_models(case):
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as AT
    m, P, images, cfg, arch = build(case)
    images = images[:2].contiguous()
    x = images.cuda()
    B = 2
    m.train()
    before = bn_buffers(m)
    lig, lig_attr, lig_delta = AT.layer_integrated_gradients(m, x, n_steps=N_STEPS, return_attr=True, return_delta=True)
    cond, cond_attr, cond_delta = AT.layer_conductance(m, x, n_steps=N_STEPS, return_attr=True, return_delta=True)
    hires, lcam = AT.hirescam(m, x), AT.layercam(m, x)
    torch.cuda.synchronize()
    assert m.training                                                       # the caller's mode is back
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    named = dict(m.named_parameters())                                      # only head parameters got a gradient
    head = [k for k in named if (k.startswith("backbone.fc.") if cfg is None else not k.startswith("backbone.")) and "to_q" not in k]
    assert head and all(named[k].grad is not None for k in head)
    assert all(p.grad is None for k, p in named.items() if k not in head)
    n = lig_delta.shape[1]
    h, w, C = lig_attr.shape[2:]
    for t in (lig, cond, hires, lcam):
        assert tuple(t.shape) == (B, n, h, w) and t.dtype == torch.float32 and t.is_cuda
    assert tuple(cond_attr.shape) == (B, n, h, w, C) and tuple(cond_delta.shape) == (B, n) and lig_delta.dtype == torch.float32
    assert bool((lcam >= 0).all())

    # ---- the oracle under fp64 and fp32 autograd: the project's rule, and completeness
    o64, o32 = oracle_results(case, P, images, cfg, arch, n)
    for c in range(n):
        check_rule("%s layerig(class %d)" % (case, c), lig[:, c], o64["lig"][:, c], o32["lig"][:, c])
        check_rule("%s conductance(class %d)" % (case, c), cond[0, c], o64["cond"][c], o32["cond"][c])
        check_rule("%s hirescam(class %d)" % (case, c), hires[:, c], o64["hires"][:, c], o32["hires"][:, c])
    check_rule("%s layercam" % case, lcam, o64["lcam"], o32["lcam"])
    for name, delta, gap in (("layerig", lig_delta.cpu().double(), o64["lig_gap"]), ("conductance", cond_delta[:1].cpu().double(), o64["cond_gap"][None])):
        ends = o64["ends"][:delta.shape[0]]
        allowed = 2.0 * gap.abs() + 1e-3 * ends.abs()
        print("%s %s completeness: max |gap| HIP %.3e, fp64 oracle %.3e, max |out(x) - out(x')| %.3e, worst gap / allowed %.3f"
              % (case, name, float(delta.abs().max()), float(gap.abs().max()), float(ends.abs().max()), float((delta.abs() / allowed).max())))
        assert bool((delta.abs() <= allowed).all()), (case, name)

    # ---- the definition over the HIP path's own gradients: the kernels' bounds
    cols = list(range(n))
    alphas, weights = AT.ig_quadrature(N_STEPS, "gausslegendre")
    own_lig = own_layer_ig(m, x, torch.zeros_like(x[:1]), alphas, weights, cols)
    check_own(case + " layerig", lig, lig_attr, None, own_lig, N_STEPS)
    own_cond = own_conductance(m, x, None, N_STEPS, cols)
    check_own(case + " conductance", cond, cond_attr, None, own_cond, N_STEPS)
    fp = m.feature_pass(x)
    feat = fp.features
    for c in (0, n - 1):
        g = fp.grad(one_hot(fp.log_probs.shape, c))
        ref, mag = R.layer_gxa(feat.cpu().view(B, h * w, C), g.cpu().view(B, h * w, C), False, False)
        err, bound = (hires[:, c].cpu().double().view(B, h * w) - ref).abs(), 2.0 ** -24 * ref.abs() + (C + 2) * U * mag
        assert bool((err <= bound).all()), (case, "hirescam", c)
        ref, mag = R.layer_gxa(feat.cpu().view(B, h * w, C), g.cpu().view(B, h * w, C), True, True)
        err, bound = (lcam[:, c].cpu().double().view(B, h * w) - ref).abs(), 2.0 ** -24 * ref.abs() + (C + 2) * U * mag
        assert bool((err <= bound).all()), (case, "layercam", c)
    assert torch.equal(AT.layer_gradxact(m, x, classes=[1], rectify=True, relu=True)[:, 0], lcam[:, 1])

    # ---- a baseline image per image and one for the batch, against the same definition
    base = (0.5 * images.flip(0)).contiguous()
    got = AT.layer_integrated_gradients(m, x, classes=[1, 4], baseline=base, n_steps=N_STEPS, return_attr=True)
    check_own(case + " layerig, baseline [B, C, H, W]", got[0], got[1], None, own_layer_ig(m, x, base.cuda(), alphas, weights, [1, 4]), N_STEPS)
    got = AT.layer_conductance(m, x, classes=[1, 4], baseline=base[0], n_steps=5, return_attr=True)
    check_own(case + " conductance, baseline [C, H, W]", got[0], got[1], None,
              own_conductance(m, x, base[:1].expand(B, -1, -1, -1).cuda(), 5, [1, 4]), 5)

    # ---- classes: a list gives the same columns bit for bit, a LongTensor the diagonal, a class outside the outputs is refused
    cls = (torch.arange(B) * 3 + 1) % n
    idx = torch.arange(B)
    for name, fn, full, kw in (("layerig", AT.layer_integrated_gradients, lig, dict(n_steps=N_STEPS)),
                               ("conductance", AT.layer_conductance, cond, dict(n_steps=N_STEPS)),
                               ("hirescam", AT.hirescam, hires, {}), ("layercam", AT.layercam, lcam, {})):
        two = fn(m, x, classes=[0, 3], **kw)
        assert tuple(two.shape) == (B, 2, h, w) and torch.equal(two[:, 0], full[:, 0]) and torch.equal(two[:, 1], full[:, 3]), name
        own = fn(m, x, classes=cls, **kw)
        assert tuple(own.shape) == (B, 1, h, w)
        key = {"layerig": "lig", "hirescam": "hires", "layercam": "lcam"}.get(name)
        if key:
            check_rule("%s %s(per-image classes)" % (case, name), own[:, 0], o64[key][idx, cls], o32[key][idx, cls])
        else:
            check_rule("%s %s(per-image classes)" % (case, name), own[0, 0], o64["cond"][cls[0]], o32["cond"][cls[0]])
        for bad in ([n], [-1], torch.tensor([0] * (B - 1) + [n])):
            with pytest.raises(IndexError):
                fn(m, x, classes=bad, **kw)
        assert tuple(fn(m, x, classes=[], **kw).shape) == (B, 0, h, w)

    # ---- chunks that split the steps differently: within the kernels' bound of the same definition
    for batch in (3, 5, 8):
        got = AT.layer_integrated_gradients(m, x, n_steps=N_STEPS, batch=batch, return_attr=True)
        check_own("%s layerig, batch %d" % (case, batch), got[0], got[1], None, own_lig, N_STEPS)
    for batch in (2, 4, 9):
        got = AT.layer_conductance(m, x, n_steps=N_STEPS, batch=batch, return_attr=True)
        check_own("%s conductance, batch %d" % (case, batch), got[0], got[1], None, own_cond, N_STEPS)

    # ---- the maps: K.cam_maps of the float maps, byte for byte
    H, W = images.shape[2:]
    assert torch.equal(AT.layerig_maps(m, x, min_level=0.2, n_steps=N_STEPS), K.cam_maps(lig, H, W, 0.2))
    assert torch.equal(AT.conductance_maps(m, x, classes=[0, 3], size=(20, 30), n_steps=N_STEPS), K.cam_maps(cond[:, [0, 3]].contiguous(), 20, 30, 0.0))
    assert torch.equal(AT.hirescam_maps(m, x, min_level=0.2), K.cam_maps(hires, H, W, 0.2))
    assert torch.equal(AT.layercam_maps(m, x, size=(20, 30)), K.cam_maps(lcam, 20, 30, 0.0))

    # ---- BatchNorm-folded: the oracle's rule and the definition over the folded path's own gradients
    m.eval()
    m.set_inference_fold(True)
    try:
        flig, flig_attr, flig_delta = AT.layer_integrated_gradients(m, x, n_steps=N_STEPS, return_attr=True, return_delta=True)
        fcond, fcond_attr = AT.layer_conductance(m, x, n_steps=N_STEPS, return_attr=True)
        fhires, flcam = AT.hirescam(m, x), AT.layercam(m, x)
        for c in range(n):
            check_rule("%s folded layerig(class %d)" % (case, c), flig[:, c], o64["lig"][:, c], o32["lig"][:, c])
            check_rule("%s folded conductance(class %d)" % (case, c), fcond[0, c], o64["cond"][c], o32["cond"][c])
            check_rule("%s folded hirescam(class %d)" % (case, c), fhires[:, c], o64["hires"][:, c], o32["hires"][:, c])
        check_rule("%s folded layercam" % case, flcam, o64["lcam"], o32["lcam"])
        assert bool((flig_delta.cpu().double().abs() <= 2.0 * o64["lig_gap"].abs() + 1e-3 * o64["ends"].abs()).all())
        check_own(case + " folded layerig", flig, flig_attr, None, own_layer_ig(m, x, torch.zeros_like(x[:1]), alphas, weights, cols), N_STEPS)
        check_own(case + " folded conductance", fcond, fcond_attr, None, own_conductance(m, x, None, N_STEPS, cols), N_STEPS)
    finally:
        m.set_inference_fold(False)
    assert not m.training
    after = bn_buffers(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 6: the tool
TOOL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--layerig", "true", "--conductance", "true",
        "--hirescam", "true", "--layercam", "true", "--layerig_steps", "8", "--layerig_batch", "5", "--conductance_steps", "6",
        "--conductance_batch", "4", "--grad_min_level", "0.2", "--eval_fold", "true"]
NAMES = ["layerig", "conductance", "hirescam", "layercam"]


@pytest.mark.parametrize("use_slot", [True, False], ids=["slot", "fc"])
def test_the_tool_on_one_image(use_slot, tmp_path, monkeypatch, capsys):
    """--table_images 0 (the default) writes the four PNG sets of every class, the bytes of the library's *_maps, no other
    family's files, and one causal line per row"""
    from PIL import Image
    from scouter_amd import test as T
    from scouter_amd.tools import attribution as AT
    from scouter_amd.tools import layer as L
    vis_dir = str(tmp_path / "vis")
    argv = ["layer.py"] + TOOL + ["--use_slot", "true" if use_slot else "false", "--causal", "true", "--causal_step", "2048",
                                  "--vis_dir", vis_dir, "--output_dir", str(tmp_path / "none")]
    monkeypatch.setattr(sys, "argv", argv)
    torch.manual_seed(11)
    L.main()
    out = capsys.readouterr().out
    names = (["slot"] if use_slot else []) + NAMES
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("causal ")]
    assert [ln[1] for ln in lines] == names, lines
    for ln in lines:
        values = [float(v) for v in ln[4:] if v[0].isdigit() or v[0] == "-"]
        assert len(values) == 2 and all(math.isfinite(v) for v in values), ln
    assert sorted(os.listdir(vis_dir)) == sorted("%s_%d.png" % (n, c) for n in names for c in range(10))
    args = L.get_layer_parser().parse_args(argv[1:])
    assert L.option_kwargs(args, "layerig") == dict(n_steps=8, batch=5) and L.option_kwargs(args, "conductance") == dict(n_steps=6, batch=4)
    torch.manual_seed(11)
    model, _ = T.build_model(args)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 64, 64), dtype=np.float32))[None].cuda()
    want = {"layerig": AT.layerig_maps(model, x, min_level=0.2, n_steps=8, batch=5),
            "conductance": AT.conductance_maps(model, x, min_level=0.2, n_steps=6, batch=4),
            "hirescam": AT.hirescam_maps(model, x, min_level=0.2), "layercam": AT.layercam_maps(model, x, min_level=0.2)}
    for name, maps in want.items():
        maps = maps[0].cpu().numpy()
        assert maps.shape == (10, 64, 64) and maps.dtype == np.uint8 and any(m.any() for m in maps)
        for c in range(10):
            png = np.asarray(Image.open(os.path.join(vis_dir, "%s_%d.png" % (name, c))))
            assert png.shape == (64, 64) and png.dtype == np.uint8 and np.array_equal(png, maps[c]), (name, c)


def test_the_tool_on_a_table(tmp_path, monkeypatch, capsys):
    """--table_images 2 on synthetic data: one `table <family>:` line for each of the four rows after the table's own"""
    from scouter_amd.tools import layer as L
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["layer.py"] + TOOL + [
        "--use_slot", "true", "--synthetic_data", "true", "--num_workers", "0", "--table_images", "2", "--batch_size", "2",
        "--localization", "true", "--output_dir", str(tmp_path / "none")])
    result = L.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == ["slot:"] + [n + ":" for n in NAMES] + ["accuracy"]
    for ln in lines[1:5]:
        words = ln.split()
        assert words[2:4] == ["images", "2"] and words[4] == "area" and 0.0 <= float(words[5]) <= 1.0
    for name in NAMES:
        cols = result.rows[name]
        assert all(v.dtype == np.float64 and v.shape == (2,) for v in cols.values())
        assert ((cols["area"] >= 0) & (cols["area"] <= 1)).all()
