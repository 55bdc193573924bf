"""BatchNorm-folded inference (SlotModel.set_inference_fold) on the device (-m gpu): the one-launch fold and the one-launch
split-attention gate against fp64, the folded eval forward of the whole model against the fixtures' fp64 eval run and an
in-test fp64 oracle on the model's own parameters (fp32 and --precision bf16), staleness of the folded tensors, no change
of the training step or of the unfolded eval forward, launch accounting, the FC baseline and engine.evaluate."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                                    # noqa: E402
from oracle.gen_golden import MODEL_CASES, LAMBDA, ENGINE_BATCH, ENGINE_SIZE, model_inputs   # noqa: E402
from test_fold_cpu import fold_pair_fp64, model_args                                    # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EVAL_CASES = ["resnet18_mnist_64", "resnest26d_96", "resnest50d_64_spc3", "resnest26d_224"]


def build(case, precision="fp32", state=None):
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist, precision=precision))
    m.load_state_dict(P if state is None else state)
    return m.cuda(), P, images, labels


def case_cfg(case):
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    return dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=float(LAMBDA))


def oracle_eval(sd, images, cfg, dtype):
    """eval forward of the oracle on a state dict (the model's own, after its training forward) -> (log_probs, attn)"""
    P = {k: (v.detach().cpu().to(dtype) if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in sd.items()}
    aux = {}
    with torch.no_grad():
        out = O.slot_model_forward(P, images.to(dtype), None, cfg, training=False, aux=aux)
    return out.double(), aux["attn"].double()


def eval_fwd(m, images, fold):
    m.set_inference_fold(fold)
    m.eval()
    with torch.no_grad():
        out = m(images)
    torch.cuda.synchronize()
    return out.detach().cpu().double(), m.slot.last_attn.detach().cpu().double() if m.use_slot else None


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96", "resnest50d_64_spc3"])
def test_fold_kernel_against_fp64_rounded_once(case):
    """Every folded weight and bias of the backbone against the fp64 restatement rounded to fp32: equal up to 1 ulp (the
    kernel forms the same fp64 products; only the contraction of beta - mean * s + bias * s may differ).  Includes
    gamma = 0 (a zero-initialised last BatchNorm) and negative gammas."""
    from scouter_amd.nn_hip import StemConv2d
    spec, P, images, labels = model_inputs(case)
    P = {k: v.clone() for k, v in P.items()}
    last_bn = "backbone.layer1.0.bn2.weight" if "resnet18" in case else "backbone.layer1.0.bn3.weight"
    P[last_bn].zero_()
    P["backbone.layer2.0.bn1.weight"][::3] *= -1.0
    P["backbone.bn1.weight"][1] = -0.75
    m, _, images, _ = build(case, state=P)
    eval_fwd(m, images.cuda(), True)
    mods = dict(m.named_modules())
    exact = total = 0
    for conv, bn in m.fold_pairs():
        c, f = mods[conv], mods[conv]._fold
        w64, b64 = fold_pair_fp64(P[conv + ".weight"], P.get(conv + ".bias"), P[bn + ".weight"], P[bn + ".bias"],
                                  P[bn + ".running_mean"], P[bn + ".running_var"])
        want_w, want_b = w64.float(), b64.float()
        got_w = f.w.detach().cpu()
        if isinstance(c, StemConv2d):
            k = c.kernel_size
            flat = got_w.reshape(c.kpad, c.out_channels)
            assert float(flat[c.kdim:].abs().max()) == 0.0 if c.kpad > c.kdim else True
            got_w = flat[:c.kdim].reshape(k, k, c.in_channels, c.out_channels)
        got_w = got_w.permute(3, 2, 0, 1)
        for got, want, what in ((got_w, want_w, conv + ".weight"), (f.b.detach().cpu(), want_b, conv + ".bias")):
            assert got.shape == want.shape, what
            inf = torch.full_like(want, float("inf"))
            ok = (got == want) | (got == torch.nextafter(want, inf)) | (got == torch.nextafter(want, -inf))
            assert bool(ok.all()), (what, float((got.double() - want.double()).abs().max()))
            exact += int((got == want).sum())
            total += want.numel()
    if last_bn[:-len(".weight")] in [b for _, b in m.fold_pairs()]:
        conv0 = [c for c, b in m.fold_pairs() if b == last_bn[:-len(".weight")]][0]
        assert float(mods[conv0]._fold.w.abs().max()) == 0.0
    print(case, "folded elements bit-equal to the fp64 restatement rounded once: %d of %d%s"
          % (exact, total, " (all)" if exact == total else ""))


# ---------------------------------------------------------------------------------------------------------------- 2
def _gate_inputs(Cp, A, B, seed):
    g = torch.Generator().manual_seed(seed)
    gap = torch.randn(B, Cp, generator=g).abs() * 0.6                       # (a mean of ReLU outputs)
    w1 = torch.randn(Cp, A, generator=g) * (2.0 / Cp) ** 0.5
    b1 = torch.randn(A, generator=g) * 0.1
    w2 = torch.randn(A, 2 * Cp, generator=g) * (2.0 / A) ** 0.5
    b2 = torch.randn(2 * Cp, generator=g) * 0.1
    return gap, w1, b1, w2, b2


def _gate_ref(gap, w1, b1, w2, b2, dtype):
    gap, w1, b1, w2, b2 = (t.to(dtype) for t in (gap, w1, b1, w2, b2))
    z = torch.relu(gap @ w1 + b1) @ w2 + b2
    B, Cp = gap.shape
    return torch.softmax(z.view(B, 2, Cp), dim=1).reshape(B, 2 * Cp).double()


@pytest.mark.parametrize("Cp,A", [(64, 32), (128, 64), (256, 128), (512, 256)])
def test_gate_kernel_against_fp64(Cp, A):
    """scouter_sa_gate_fwd_f32 for every (C', attention width) of resnest26d / 50d at B = 1, 3, 70.  Yardstick: the error of
    the fp32 PyTorch restatement against fp64 on the same inputs, times the project's per-tensor factor 2, with a floor of
    4 fp32 ulps of 1 (the outputs are softmax weights in [0, 1]).  A row does not depend on the batch it is computed in."""
    from scouter_amd import kernels as K
    assert K.sa_gate_eligible(Cp, A)
    floor = 4 * 2.0 ** -23
    big = None
    for B in (1, 3, 70):
        ins = _gate_inputs(Cp, A, B, 500 + Cp + B)
        ref64, ref32 = _gate_ref(*ins, torch.float64), _gate_ref(*ins, torch.float32)
        dev = [t.cuda().contiguous() for t in ins]
        a = K.sa_gate_fwd(dev[0], dev[1].view(1, 1, Cp, A), dev[2], dev[3].view(1, 1, A, 2 * Cp), dev[4])
        torch.cuda.synchronize()
        err = float((a.cpu().double() - ref64).abs().max())
        err32 = float((ref32 - ref64).abs().max())
        print("gate Cp %d A %d B %d: |HIP - fp64| = %.3g, |torch fp32 - fp64| = %.3g" % (Cp, A, B, err, err32))
        assert err <= max(2 * err32, floor), (B, err, err32)
        assert float((a.view(B, 2, Cp).sum(1) - 1).abs().max()) <= 4e-7
        if B == 70:
            big = (dev, a)
    dev, a70 = big
    a1 = K.sa_gate_fwd(dev[0][5:6].contiguous(), dev[1].view(1, 1, Cp, A), dev[2], dev[3].view(1, 1, A, 2 * Cp), dev[4])
    assert torch.equal(a1[0], a70[5])


def test_gate_kernel_refuses_shapes_it_does_not_cover():
    from scouter_amd import kernels as K, _native
    assert not K.sa_gate_eligible(96, 48) and not K.sa_gate_eligible(1024, 256) and not K.sa_gate_eligible(32, 32)
    t = torch.zeros(4096, device="cuda")
    rc = _native.lib().scouter_sa_gate_fwd_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                               1, 96, 48, 0)
    assert rc == -3, rc                                                     # SC_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", EVAL_CASES)
def test_folded_eval_forward_fp32(case):
    """The procedure of tests/test_model_gpu.py (one training forward, then eval) with the switch on: the folded
    log-probabilities meet north_star's gate max(1e-4, 3 x |f32_eval - f64_eval|) against the fixture's fp64 eval run, and
    the same gate against the in-test fp64 oracle on the model's OWN post-step state_dict (which takes the running-statistic
    differences out); attention maps by the attention rule of test_model_gpu.py.
    resnest26d_224 adds a batch-70 run, where no fp64 oracle is run: with the bound = the sum of the two paths' fp64-oracle
    errors at batch 6, the condition is no NaN and the same argmax wherever the unfolded top-2 margin exceeds that bound.
    (The largest elementwise difference over the 700 log-probabilities is printed, not bounded: measured 1.7e-3 against a
    bound of 9.6e-4 taken over 60 -- the head amplifies any rounding difference and a maximum grows with the sample.)"""
    g = np.load(os.path.join(GOLD, "model_%s.npz" % case))
    m, P, images, labels = build(case)
    m.train()
    m(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    unf, unf_attn = eval_fwd(m, images.cuda(), False)
    fold, fold_attn = eval_fwd(m, images.cuda(), True)
    floor = float(np.abs(g["f32_eval_log_probs"] - g["f64_eval_log_probs"]).max())
    tol = max(1e-4, 3 * floor)
    err_fix = float(np.abs(fold.numpy() - g["f64_eval_log_probs"]).max())
    err_fix_unf = float(np.abs(unf.numpy() - g["f64_eval_log_probs"]).max())
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    sd = m.state_dict()
    cfg = case_cfg(case)
    ref, ref_attn = oracle_eval(sd, images, cfg, torch.float64)
    ref32, ref32_attn = oracle_eval(sd, images, cfg, torch.float32)
    floor_own = float((ref32 - ref).abs().max())
    err, err_unf = float((fold - ref).abs().max()), float((unf - ref).abs().max())
    floor_a = float((ref32_attn - ref_attn).abs().max())
    err_a, err_a_unf = float((fold_attn - ref_attn).abs().max()), float((unf_attn - ref_attn).abs().max())
    print("%s folded eval: |log_probs - fixture fp64| %.3g (unfolded %.3g, fixture fp32 %.3g) | own-state oracle: folded %.3g, "
          "unfolded %.3g, torch fp32 %.3g, ratio folded / unfolded %.2f | attention: folded %.3g, unfolded %.3g, torch fp32 %.3g"
          % (case, err_fix, err_fix_unf, floor, err, err_unf, floor_own, err / max(err_unf, 1e-30), err_a, err_a_unf, floor_a))
    assert err_fix <= tol, (err_fix, tol, floor)
    tol_own = max(1e-4, 3 * floor_own)
    assert err <= tol_own, (err, tol_own, floor_own)
    assert err_a <= max(1e-4, tol_own, 3 * floor_a), (err_a, floor_a, tol_own)
    assert err_a <= max(2.0 * floor_a, 2e-5), (err_a, floor_a)              # (the tight form of tests/test_model_gpu.py)
    if case != "resnest26d_224":
        return
    bound = err + err_unf
    big, _ = O.synth_batch(70, 3, 224, cfg["num_classes"], 777)
    u70, _ = eval_fwd(m, big.cuda(), False)
    f70, _ = eval_fwd(m, big.cuda(), True)
    assert bool(torch.isfinite(f70).all()) and bool(torch.isfinite(u70).all())
    d70 = float((f70 - u70).abs().max())
    print("batch 70 x 224^2: max |folded - unfolded| = %.3g, bound (sum of the two batch-6 oracle errors) %.3g" % (d70, bound))
    top2 = u70.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > bound
    print("images whose top-2 margin exceeds the bound: %d of 70" % int(sure.sum()))
    assert int(sure.sum()) > 0 and bool((f70.argmax(1)[sure] == u70.argmax(1)[sure]).all())


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("case", ["resnest26d_96", "resnest26d_224"])
def test_folded_eval_forward_bf16(case):
    """--precision bf16: the folded path's error against fp64 (the oracle on the model's own state) is at most twice that
    of the unfolded bf16 eval path with fp32 activation storage on the same inputs -- both round the same operands to bf16
    once, the folded path after the BatchNorm scale went into the weights."""
    m, P, images, labels = build(case, precision="bf16")
    m.set_activation_storage("fp32")
    m.train()
    m(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    unf, _ = eval_fwd(m, images.cuda(), False)
    fold, _ = eval_fwd(m, images.cuda(), True)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    ref, _ = oracle_eval(m.state_dict(), images, case_cfg(case), torch.float64)
    err, err_unf = float((fold - ref).abs().max()), float((unf - ref).abs().max())
    print("%s bf16: |folded - fp64| %.3g, |unfolded - fp64| %.3g, ratio %.2f" % (case, err, err_unf, err / max(err_unf, 1e-30)))
    assert bool(torch.isfinite(fold).all())
    assert err <= 2 * err_unf, (err, err_unf)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96"])
def test_folded_tensors_follow_the_parameters(case):
    from scouter_amd.optim import FusedAdamW
    g = np.load(os.path.join(GOLD, "model_%s.npz" % case))
    tol = max(1e-4, 3 * float(np.abs(g["f32_eval_log_probs"] - g["f64_eval_log_probs"]).max()))
    m, P, images, labels = build(case)
    x, y = images.cuda(), labels.cuda()
    first, _ = eval_fwd(m, x, True)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    m.train()
    out, losses = m(x, y)
    losses[0].backward()
    opt.step()
    second, _ = eval_fwd(m, x, True)
    unf, _ = eval_fwd(m, x, False)
    assert float((second - unf).abs().max()) <= tol, (float((second - unf).abs().max()), tol)
    assert float((second - first).abs().max()) > 10 * tol
    m.set_inference_fold(True)
    m.eval()
    with torch.no_grad():
        m(x)                                                    # (folded tensors are current; only load_state_dict follows)
    m.load_state_dict(P)
    with torch.no_grad():
        third = m(x).detach().cpu().double()
    unf0, _ = eval_fwd(m, x, False)
    assert float((third - unf0).abs().max()) <= tol
    assert float((third - second).abs().max()) > 10 * tol
    assert torch.equal(third, first)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_switch_changes_no_training_step_no_unfolded_eval_and_no_state():
    case = "resnest26d_96"
    m, P, images, labels = build(case)
    x, y = images.cuda(), labels.cuda()
    ev0, _ = eval_fwd(m, x, False)
    keys0 = list(m.state_dict().keys())

    def step(fold):
        m.load_state_dict(P)
        m.set_inference_fold(fold)
        m.train()
        out, losses = m(x, y)
        losses[0].backward()
        torch.cuda.synchronize()
        return out.detach().clone(), losses[0].detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()
                                                                    if p.grad is not None}
    out_a, loss_a, grads_a = step(False)
    out_b, loss_b, grads_b = step(True)
    assert torch.equal(out_a, out_b) and torch.equal(loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys() and len(grads_a) > 100
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
    # the unfolded eval forward has the bits it had before the folded path ever ran, and switching leaves the state alone
    m.load_state_dict(P)
    f1, _ = eval_fwd(m, x, True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ev1, _ = eval_fwd(m, x, False)
    assert torch.equal(ev0, ev1)
    after = m.state_dict()
    assert list(after.keys()) == keys0 == list(before.keys())
    for k in before:
        assert torch.equal(before[k], after[k]) and torch.equal(after[k].cpu(), P[k]), k
    assert not any("fold" in k for k in keys0)


# ---------------------------------------------------------------------------------------------------------------- 7
def _profiled(fn):
    from scouter_amd import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(1 << 18)
    torch.cuda.synchronize()
    L.scouter_prof_collect(buf, len(buf))
    L.scouter_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.scouter_prof_enable(0)
        L.scouter_prof_collect(buf, len(buf))
    rows = [r.split("\t") for r in buf.value.decode().splitlines()]
    return {r[0]: int(r[1]) for r in rows}


def test_folded_forward_launches_no_batchnorm_kernel_and_fewer_kernels():
    m, P, images, labels = build("resnest26d_96")
    x = images.cuda()
    eval_fwd(m, x, False)
    unf = _profiled(lambda: eval_fwd(m, x, False))
    eval_fwd(m, x, True)                                        # (the fold itself runs here, once)

    def again():
        with torch.no_grad():
            m(x)
    fold = _profiled(again)
    # (every label of bn_elem.hip's BatchNorm passes -- bn_fwd(...), bn_maxpool_fwd, sa_bn_* -- and every convolution label with
    #  a fused BatchNorm epilogue has "bn" in it; the fold's own launch is the one exception and does not run here)
    bn = lambda d: {k: v for k, v in d.items() if "bn" in k and k != "bn_fold_multi"}
    print("profiled launches of one resnest26d eval forward: unfolded %d (BatchNorm kernels %d), folded %d (BatchNorm kernels %d)"
          % (sum(unf.values()), sum(bn(unf).values()), sum(fold.values()), sum(bn(fold).values())))
    assert sum(bn(unf).values()) > 0 and not bn(fold), bn(fold)
    assert "bn_fold_multi" not in fold and fold.get("sa_gate_fwd", 0) == 8
    assert sum(fold.values()) < sum(unf.values())


# ---------------------------------------------------------------------------------------------------------------- 8
def test_fc_baseline_and_engine_evaluate_with_the_switch_on():
    from scouter_amd import engine
    from scouter_amd.sloter.slot_model import SlotModel
    from scouter_amd.tools.calculate_tool import MetricLog
    # FC baseline: global pool + fc behind the same folded backbone
    spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
    P = O.synth_state(spec, 200)
    m = SlotModel(model_args("resnet18", 10, 1, 1, 1, 1, True, use_slot=False))
    m.load_state_dict(P)
    m = m.cuda()
    images, labels = O.synth_batch(4, 1, 64, 10, 201)
    unf, _ = eval_fwd(m, images.cuda(), False)
    fold, _ = eval_fwd(m, images.cuda(), True)
    Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    with torch.no_grad():
        ref = O.fc_model_forward(Pd, images.double(), None, "resnet18", training=False)
        ref32 = O.fc_model_forward({k: v.clone() for k, v in P.items()}, images, None, "resnet18", training=False).double()
    tol = max(1e-4, 3 * float((ref32 - ref).abs().max()))
    assert float((fold - ref).abs().max()) <= tol and float((unf - ref).abs().max()) <= tol
    # engine.evaluate on the MNIST engine fixture's inputs: the record with the switch on equals the unfolded record within
    # the rounding of its three decimals
    spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True)
    m = SlotModel(model_args("resnet18", 10, 1, 1, 1, 1, True))
    m.load_state_dict(O.synth_state(spec, 300))
    m = m.cuda()
    loader = []
    for i in range(2):
        img, lab = O.synth_batch(ENGINE_BATCH, 1, ENGINE_SIZE, 10, 310 + i)
        loader.append({"image": img.double(), "label": lab})
    recs = []
    for on in (False, True):
        m.set_inference_fold(on)
        log = MetricLog()
        engine.evaluate(m, loader, torch.device("cuda"), log.record, 0)
        recs.append(np.array([log.record["val"][k][0] for k in ("loss", "acc", "log_loss", "att_loss")]))
    print("engine.evaluate record unfolded", recs[0], "folded", recs[1])
    np.testing.assert_allclose(recs[1], recs[0], atol=1.01e-3, rtol=0)
    assert recs[1][1] == recs[0][1]
