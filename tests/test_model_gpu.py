"""Whole-network parity (-m gpu): SlotModel on the HIP path vs the golden vectors generated from the reference
(tests/golden/model_*.npz) and vs the CPU oracle on the same seeded parameters / inputs -- forward, every parameter
gradient, BatchNorm running statistics, eval-mode forward."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402
from oracle.gen_golden import MODEL_CASES, LAMBDA, HEAD_PREFIXES, model_inputs, grad_digest   # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def build(case):
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    args = argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=True, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0,
                              loss_status=ls, power=power, to_k_layer=L, lambda_value=LAMBDA)
    spec, P, images, labels = model_inputs(case)
    m = SlotModel(args)
    assert list(m.state_dict().keys()) == list(spec.keys())
    m.load_state_dict(P)
    return m.cuda(), P, images, labels


def capture_relu_signs(m):
    """Arms every BatchNorm2d(+ReLU) of the HIP model to record its output; returns the dict (name -> NHWC tensor)."""
    from scouter_amd.nn_hip import BatchNorm2d, Conv2d
    store = {}
    for name, mod in m.named_modules():
        if isinstance(mod, BatchNorm2d) or (isinstance(mod, Conv2d) and name == "conv1x1"):
            mod._capture = (store, name)
    m.backbone._capture = (store, "maxpool")              # window indices of the stem's max-pool
    return store


def oracle_run(case, dtype, relu_masks=None, sign_log=None, pool_arg=None):
    """relu_masks {layer name: bool NCHW}: evaluate every listed ReLU as x * mask (the HIP path's sign pattern);
    sign_log: dict filled with the oracle's own sign pattern (pre-activation > 0); pool_arg: the HIP path's max-pool
    window indices [B, C, Ho, Wo]."""
    if pool_arg is not None:
        O.MAXPOOL_HOOK = lambda x: O.maxpool_with_indices(x, pool_arg)
    if relu_masks is not None or sign_log is not None:
        def hook(name, x):
            if sign_log is not None:
                sign_log[name] = (x > 0)
            if relu_masks is not None and name in relu_masks:
                return x * relu_masks[name].to(x.dtype)
            return torch.relu(x)
        O.RELU_HOOK = hook
    try:
        if isinstance(case, tuple):                       # (P, images, labels, cfg): a synthetic model, not a fixture
            return _oracle_run_inputs(*case, dtype)
        return _oracle_run(case, dtype)
    finally:
        O.RELU_HOOK = None
        O.MAXPOOL_HOOK = None


def _oracle_run(case, dtype):
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=float(LAMBDA))
    return _oracle_run_inputs(P, images, labels, cfg, dtype)


def _oracle_run_inputs(P, images, labels, cfg, dtype):
    P = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    keys = O.trainable_keys(P)
    leaves = {k: P[k].clone().requires_grad_(True) for k in keys}
    Q = dict(P)
    Q.update(leaves)
    aux = {}
    out, losses = O.slot_model_forward(Q, images.to(dtype), labels, cfg, training=True, aux=aux)
    losses[0].backward()
    return out, losses, aux, leaves, Q


def pinned_gradient_check(what, case, signs, named, kf=2.0, ks=1e-3, kf_squeeze=None, kf_head=None):
    """Every parameter gradient of the HIP model against the oracle's fp64 autograd evaluated under the SIGN PATTERN the
    HIP forward produced (`signs` from capture_relu_signs: every BatchNorm+ReLU output, conv1x1, the stem max-pool's
    window indices), next to the oracle's fp32 autograd under the same pattern:
        |HIP - fp64| <= max(kf x |torch fp32 - fp64|, ks x max|grad|)        for EVERY tensor.
    `case`: a MODEL_CASES name or (P, images, labels, cfg)."""
    pool_arg = signs.pop("maxpool").permute(0, 3, 1, 2).cpu()
    masks = {k: (v > 0).permute(0, 3, 1, 2).cpu() for k, v in signs.items()}
    own = {}
    _, _, _, lv64, _ = oracle_run(case, torch.float64, relu_masks=masks, sign_log=own, pool_arg=pool_arg)
    _, _, _, lv32, _ = oracle_run(case, torch.float32, relu_masks=masks, pool_arg=pool_arg)
    flips = {k: int((own[k] != masks[k]).sum()) for k in masks if int((own[k] != masks[k]).sum())}
    # S = 300 slots (resnest50d case): the head's row-sum division is ill-conditioned and its noise
    # enters every backbone gradient through d(features); PyTorch fp32 and the HIP path then differ from fp64 by the
    # same order but not tensor by tensor -- factor 8 / 8e-3 there, 2 / 1e-3 for the well-conditioned heads
    bad, worst = [], (0.0, None)
    for k, ref in lv64.items():
        if k.endswith("conv2.fc1.bias"):
            continue
        mine = named[k].grad.detach().cpu().double()
        scale = float(ref.grad.abs().max())
        e = float((mine - ref.grad).abs().max())
        e32 = float((lv32[k].grad.double() - ref.grad).abs().max())
        squeeze = ".conv2.bn1." in k or ".conv2.fc1." in k or ".conv2.fc2." in k
        f = kf_squeeze if squeeze and kf_squeeze else (kf_head if kf_head and k.startswith(HEAD_PREFIXES) else kf)
        if e > max(f * e32, ks * scale) + 1e-9:
            bad.append((k, e, e32, scale))
        if scale > 0 and e / scale > worst[0]:
            worst = (e / scale, k)
    print(what, "ReLU sign flips HIP vs oracle fp64 (layer: elements):", flips or "none",
          "| tensors over the tight bound:", bad or "none", "| worst |HIP - fp64| / max|grad| = %.2e (%s) over %d tensors"
          % (worst[0], worst[1], len(lv64)))
    assert not bad, bad


@pytest.mark.parametrize("case", ["resnet18_mnist_64", "resnest26d_96", "resnest50d_64_spc3"])
def test_model_fwd_bwd_parity(case):
    g = np.load(os.path.join(GOLD, "model_%s.npz" % case))
    m, P, images, labels = build(case)
    m.train()
    signs = capture_relu_signs(m)
    out, (loss, nll, area) = m(images.cuda(), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    floor = float(np.abs(g["f32_log_probs"] - g["f64_log_probs"]).max())
    tol = max(1e-4, 3 * floor)
    err = np.abs(out.detach().cpu().numpy() - g["f64_log_probs"]).max()
    assert err <= tol, (err, tol, floor)
    # The tight statement: against the fp64 run of the reference, the HIP path loses no more than 1.5x
    # what the reference's OWN fp32 arithmetic (PyTorch fp32, fixture f32_*) loses on the same inputs -- or is below
    # 1e-5, a tenth of north_star's 1e-4.  Measured r2: 6.6e-6 vs 2.1e-6 (resnet18), 1.5e-4 vs 1.2e-4 (resnest26d 96^2),
    # 3.9e-4 vs 7.4e-4 (resnest50d S=300).
    assert err <= max(1.5 * floor, 1e-5), (err, floor)
    # attention maps against the reference's own fp32 deviation ON THE MAPS (the normaliser of slot_attention.py:56 makes it
    # larger than on the log-probabilities: resnest50d S = 36: 2.3e-3 / 2.5e-3 / 1.6e-3 at 8 / 16 / 32 threads vs 7.4e-4):
    # north_star's gate max(1e-4, 3 x floor) with the floor of the quantity itself, and the tight 2 x form next to it
    floor_a = float(np.abs(g["f32_attn"] - g["f64_attn"]).max())
    err_a = float(np.abs(m.slot.last_attn.cpu().numpy() - g["f64_attn"]).max())
    assert err_a <= max(1e-4, tol, 3 * floor_a), (err_a, floor_a, tol)
    assert err_a <= max(2.0 * floor_a, 2e-5), (err_a, floor_a)
    np.testing.assert_allclose([float(loss), float(nll), float(area)],
                               [float(g["f64_loss"]), float(g["f64_nll"]), float(g["f64_area"])], atol=tol, rtol=1e-4)
    # gradients vs the oracle's fp64 autograd (full tensors)
    _, _, _, leaves, Q = oracle_run(case, torch.float64)
    _, _, _, leaves32, _ = oracle_run(case, torch.float32)      # the reference arithmetic's own fp32 backward noise
    named = dict(m.named_parameters())
    assert named["slot.to_q.0.weight"].grad is None and named["slot.to_q.0.bias"].grad is None
    worst, rels, rels32 = 0.0, [], []
    for k, ref in leaves.items():
        mine = named[k].grad.detach().cpu().double()
        r = ref.grad
        scale = float(r.abs().max())
        if k.endswith("conv2.fc1.bias"):                     # bias in front of a train-mode BN: exact gradient 0
            assert float(mine.abs().max()) < 1e-3
            continue
        e = float((mine - r).abs().max())
        e32 = float((leaves32[k].grad.double() - r).abs().max())
        worst = max(worst, e / max(scale, 1e-6))
        rels.append(e / max(scale, 1e-6))
        rels32.append(e32 / max(scale, 1e-6))
        # Per-tensor cap.  At these toy resolutions (BatchNorm over 36-144 samples) ONE ReLU of a ~0 pre-activation
        # flipping under fp32 rounding moves every upstream gradient by ~1/samples; plain fp32 PyTorch shows the same
        # isolated outliers against its own fp64 run (measured: up to 9e-2 with other seeds), so the cap is loose and
        # the tight statement is the median below (and the resnet18 / full-size 224x224 cases).
        assert e <= max(1e-1 * scale, 4 * e32) + 50 * floor + 2e-5, (k, e, e32, scale)
    assert float(np.median(rels)) <= max(1.5e-2, 3 * float(np.median(rels32))), (np.median(rels), np.median(rels32))
    if case == "resnet18_mnist_64":
        assert worst <= 2e-3, worst
    # ---- tight per-tensor gradient check under ONE sign pattern.  The loose cap above exists because a single ReLU
    # flipping on a ~0 pre-activation changes every upstream gradient; that is a property of the inputs, not of the
    # kernels.  So: take the sign pattern the HIP forward actually produced (captured per BatchNorm+ReLU layer), run the
    # oracle's fp64 AND fp32 autograd under exactly that pattern (ReLU := x * mask), and demand of every tensor
    #     |HIP - fp64| <= max(2 x |torch fp32 - fp64|, 1e-3 x max|grad|)
    # -- a 5 % error in one layer's weight gradient cannot hide behind a flip any more.  (The stem's max-pool is pinned
    # to the HIP path's window choice the same way.)
    kf, ks = (8.0, 8e-3) if case == "resnest50d_64_spc3" else (2.0, 1e-3)
    pinned_gradient_check(case, case, signs, named, kf, ks)
    # BN running statistics after one training forward
    sd = m.state_dict()
    for k in Q:
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd[k].cpu().numpy(), Q[k].numpy(), rtol=2e-4, atol=5e-5, err_msg=k)
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 1
    # eval-mode forward on the updated buffers
    m.eval()
    with torch.no_grad():
        ev = m(images.cuda())
    np.testing.assert_allclose(ev.cpu().numpy(), g["f64_eval_log_probs"], atol=max(tol, 2e-4), rtol=1e-3)
    print(case, "max |log_probs - fp64 ref| = %.3g (ref fp32 noise %.3g), worst rel grad err %.3g" % (err, floor, worst))


def test_full_size_resnest26d_224_against_reference_fp64_digests():
    """BASELINE input size (224x224), batch 6: log_probs / attention vs the reference's fp64 run, every gradient vs
    the reference's fp64 gradient digest (sum, abs-sum, first 16 entries)."""
    case = "resnest26d_224"
    g = np.load(os.path.join(GOLD, "model_%s.npz" % case))
    m, P, images, labels = build(case)
    m.train()
    signs = capture_relu_signs(m)
    out, (loss, nll, area) = m(images.cuda(), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    floor = float(np.abs(g["f32_log_probs"] - g["f64_log_probs"]).max())
    tol = max(1e-4, 3 * floor)
    err = float(np.abs(out.detach().cpu().numpy() - g["f64_log_probs"]).max())
    assert err <= tol                                    # north_star's gate on this draw: unchanged
    # The tight statement is a DISTRIBUTION (round 6): `floor` is ONE draw of PyTorch's own fp32 noise (8
    # threads: 4.0e-5; the same reference at 16 / 32 threads: 1.06e-4 / 6.9e-5), and the HIP path's error is one draw of the
    # same kind of noise for every choice of (bit-compatible or not) kernel instance.  This seed is seed 0 of
    # model_resnest26d_224_seeds.npz: test_rounding_noise_over_five_seeds holds the geometric mean of |HIP - fp64| / |PyTorch
    # fp32 - fp64| over five seeds to <= 1.5 and every seed to <= 3; here the per-seed cap of that statement, against the
    # geometric mean of the reference's three thread counts on THIS seed.  (Round 5 held this one draw to 1.5 x the 8-thread
    # draw: 5.1e-5 vs 4.0e-5 for the default path then, 7.4e-5 / 8.5e-5 for the options that are defaults now.)
    gs = np.load(os.path.join(GOLD, "model_%s_seeds.npz" % case))
    assert int(gs["seeds"][0]) == 200 and np.array_equal(gs["f64_log_probs"][0], g["f64_log_probs"])
    floors = np.abs(gs["f32_log_probs"][0].astype(np.float64) - gs["f64_log_probs"][0][None]).max((1, 2))
    assert err <= max(3.0 * float(np.exp(np.log(floors).mean())), 1e-5), (err, floors)
    # attention maps: against the reference's own fp32 deviation on the maps (4.4e-4 here -- larger than on the
    # log-probabilities, the normaliser of slot_attention.py:56 is the ill-conditioned step)
    floor_a = float(np.abs(g["f32_attn"] - g["f64_attn"]).max())
    np.testing.assert_allclose(m.slot.last_attn.cpu().numpy(), g["f64_attn"], atol=max(1e-4, 1.5 * floor_a), rtol=0)
    named = dict(m.named_parameters())
    for k, d in zip(g["f32_grad_keys"], g["f64_grad_digest"]):
        k = str(k)
        if k.endswith("conv2.fc1.bias"):
            continue
        mine = grad_digest(named[k].grad.detach().cpu())
        assert abs(mine[0] - d[0]) <= 2e-2 * d[1] + 2e-4, k
        assert abs(mine[1] - d[1]) <= 2e-2 * d[1] + 2e-4, k
        scale = max(d[1] / max(named[k].numel(), 1), 1e-8)
        np.testing.assert_allclose(mine[2:], d[2:], atol=50 * scale * 2e-2 + 2e-5, rtol=5e-2, err_msg=k)
    # the digests above are loose by necessity (a ReLU flipping on a ~0 pre-activation moves every
    # upstream gradient in EITHER implementation); the sharp statement is the per-tensor bound under the HIP path's own
    # sign pattern, here at the full 224 x 224 size too
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    # backbone tensors: kf = 2 as everywhere.  Head tensors (slot.*, conv1x1.*) see the forward's feature noise coherently
    # -- on one seed all thirteen sit at the same multiple of PyTorch-fp32's own deviation (seed 200: 1.3-1.6 x for the round-5
    # default, 2.2-2.6 x with the stem on the register-split kernel, 0.4 x with every option on; other seeds 0.1-1.3 x) -- so
    # their tight bound is the distribution over five seeds (test_gradient_noise_over_five_seeds: geometric mean <= 1.5, no
    # seed > 3) and this single seed gets that statement's per-seed cap.
    pinned_gradient_check(case, case, signs, named, kf_head=3.0)


def _seed_model(seed):
    from scouter_amd.sloter.slot_model import SlotModel
    from oracle.gen_golden import SEED_CASE
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[SEED_CASE]
    args = argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="ImageNet", use_slot=True, use_pre=False,
                              grad=False, channel=O.ARCHS[arch]["channel"], slots_per_class=spc, hidden_dim=64,
                              freeze_layers=0, vis=False, vis_id=0, loss_status=ls, power=power, to_k_layer=L,
                              lambda_value=LAMBDA)
    spec, P, images, labels = model_inputs(SEED_CASE, int(seed))
    m = SlotModel(args)
    m.load_state_dict(P)
    return m.cuda().train(), images, labels


# the forward-option sets the distribution tests cover: the defaults (round 6: every option on), round 5's defaults, each option
# alone on top of those, and the exact-fp32 / plane-free path
NOISE_SWITCHES = [{}, {"x3": 15, "halo": 2}, {"x3": 31, "halo": 2}, {"x3": 47, "halo": 2}, {"x3": 15, "halo": 3},
                  {"x3": 0, "halo": 2}]


@pytest.mark.parametrize("switches", NOISE_SWITCHES)
def test_gradient_noise_over_five_seeds(switches, monkeypatch):
    """The gradient yardstick as a DISTRIBUTION (round 6).  tests/golden/model_resnest26d_224_seeds.npz holds,
    for the five seeds of the forward test below, the REFERENCE's fp64 gradients of the head tensors (`slot.*`, `conv1x1.*`) and,
    per tensor, max |fp32 - fp64| of the reference's plain-fp32 backward at 8 / 16 / 32 CPU threads (oracle/gen_golden.py).
    Head gradients are produced before the backward crosses any backbone ReLU / max-pool, so no sign flip of a ~0 backbone
    pre-activation can move them: what moves them is the rounding noise of the forward's features, coherently -- on one seed
    every head tensor sits at about the same multiple of PyTorch-fp32's own deviation, which is why ONE seed held to 2 x
    (round 5) rejected forward options whose noise is no larger: seed 200 draws 1.3-1.6 x for round 5's default, 2.6 x with the
    stem's 3x3 on the register-split kernel, 0.4 x with every option on.  Per seed and tensor
        r = |HIP - fp64| / max(geometric mean over the thread counts of |PyTorch fp32 - fp64|, 5e-4 max|grad|)
    (the second term = ks / kf of pinned_gradient_check).  TIGHT, on the tensors behind which no ReLU of the head sits either
    (last to_k layer, GRU, initial slots): worst tensor per seed, geometric mean over the seeds <= 1.5, no seed > 3.  The tensors
    in front of the head's own ReLUs (conv1x1, the earlier to_k layers) additionally move by ~1 / (B N) of their largest entry
    when one ~0 pre-activation of conv1x1 / the to_k MLP lands on the other side (seed 4200 does, for several option sets:
    4.8e-3): they get the per-seed cap with that allowance, and their tight bound is the pinned check of
    test_full_size_resnest26d_224_against_reference_fp64_digests.  Every seed also keeps north_star's gate on the forward."""
    from scouter_amd import kernels as K
    from oracle.gen_golden import SEED_CASE
    g = np.load(os.path.join(GOLD, "model_%s_seeds.npz" % SEED_CASE))
    if "halo" in switches:
        monkeypatch.setattr(K, "HALO_TILE", switches["halo"])
    keys = [str(k) for k in g["grad_keys"]]
    head = [str(k) for k in g["head_keys"]]
    offs = np.concatenate([[0], np.cumsum(g["head_sizes"])])
    last_to_k = max(int(k.split(".")[2]) for k in head if k.startswith("slot.to_k."))
    flip_free = [k for k in head if k.startswith(("slot.gru.", "slot.initial_slots", "slot.to_k.%d." % last_to_k))]
    assert len(flip_free) == 7 and len(head) == 13
    worst, table = [], []
    for i, seed in enumerate(g["seeds"]):
        m, images, labels = _seed_model(seed)
        if "x3" in switches:
            m.set_x3(switches["x3"])
        out, losses = m(images.cuda(), labels.cuda())
        losses[0].backward()
        torch.cuda.synchronize()
        err = float(np.abs(out.detach().cpu().numpy().astype(np.float64) - g["f64_log_probs"][i]).max())
        floors = np.abs(g["f32_log_probs"][i].astype(np.float64) - g["f64_log_probs"][i][None]).max((1, 2))
        assert err <= max(1e-4, 3 * float(floors.max())), (int(seed), err, floors)      # north_star's gate, per seed
        named = dict(m.named_parameters())
        r = {}
        for j, k in enumerate(head):
            ref = g["f64_head_grads"][i][offs[j]:offs[j + 1]].astype(np.float64)
            mine = named[k].grad.detach().cpu().double().flatten().numpy()
            e = float(np.abs(mine - ref).max())
            e32 = g["f32_grad_maxdev"][i][:, keys.index(k)]
            scale = float(g["f64_grad_absmax"][i][keys.index(k)])
            r[k] = e / max(float(np.exp(np.log(e32).mean())), 5e-4 * scale)
            if k not in flip_free:
                # per-seed cap + one head-ReLU flip among the B x N = 294 rows (measured 4.8e-3 of the largest entry)
                assert e <= max(3.0 * float(np.exp(np.log(e32).mean())), 1.5e-3 * scale) + 1e-2 * scale, (int(seed), k, e, e32, scale)
        worst.append(max(r[k] for k in flip_free))
        table.append(["%.2f" % r[k] for k in head])
        del m
    gm = float(np.exp(np.log(worst).mean()))
    print("gradient noise over five seeds", switches or "(default)", "worst flip-free head tensor per seed",
          ["%.2f" % w for w in worst], "geometric mean %.2f" % gm, "| all head tensors per seed:", table)
    assert gm <= 1.5 and max(worst) <= 3.0, (worst, gm)


@pytest.mark.parametrize("switches", NOISE_SWITCHES)
def test_rounding_noise_over_five_seeds(switches, monkeypatch):
    """The yardstick as a DISTRIBUTION (round 5).  tests/golden/model_resnest26d_224_seeds.npz holds, for five parameter / input
    seeds of the BASELINE-size network (224 x 224, batch 6, train-mode BatchNorm), the reference's fp64 log-probabilities and its
    plain-fp32 ones at 8 / 16 / 32 CPU threads: PyTorch's own fp32 lands 4.0e-5 / 1.06e-4 / 6.9e-5 from fp64 on seed 200 just by
    the thread count (another summation order), and 3e-6 ... 2.9e-4 across the seeds -- one draw is no yardstick.  Here: per
    seed r = |HIP - fp64| / geometric mean over the thread counts of |PyTorch fp32 - fp64|; the geometric mean of r over the five
    seeds stays <= 1.5 and no seed exceeds 3 -- for the default path (round 6: SCOUTER_X3 bit 4, the stem's 3x3 on the
    register-split kernel, bit 5, the short-K pointwise forward on the persistent bf16x3 kernel, and SCOUTER_HALO=3, the
    resident-rows plane forward, are ON), for round 5's defaults, for each of those options alone and for the exact-fp32 path
    (NOISE_SWITCHES).  One draw (seed 200 at 8 threads) had put each option over round 5's single-draw 1.5 x."""
    from scouter_amd import kernels as K
    from oracle.gen_golden import SEED_CASE
    g = np.load(os.path.join(GOLD, "model_%s_seeds.npz" % SEED_CASE))
    if "halo" in switches:
        monkeypatch.setattr(K, "HALO_TILE", switches["halo"])
    ratios = []
    for i, seed in enumerate(g["seeds"]):
        m, images, labels = _seed_model(seed)
        if "x3" in switches:
            m.set_x3(switches["x3"])
        with torch.no_grad():
            out, _ = m(images.cuda(), labels.cuda())
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - g["f64_log_probs"][i]).max())
        floors = np.abs(g["f32_log_probs"][i].astype(np.float64) - g["f64_log_probs"][i][None]).max((1, 2))
        floor = float(np.exp(np.log(floors).mean()))
        assert err <= max(1e-4, 3 * float(floors.max())), (int(seed), err, floors)      # north_star's gate, per seed
        ratios.append(err / floor)
        del m
    gm = float(np.exp(np.log(ratios).mean()))
    print("rounding noise over five seeds", switches or "(default)", "ratios |HIP - fp64| / |PyTorch fp32 - fp64| =",
          ["%.2f" % r for r in ratios], "geometric mean %.2f" % gm)
    assert gm <= 1.5 and max(ratios) <= 3.0, (ratios, gm)


def test_frozen_backbone_and_no_cpu_fallback(pretrained_dir):
    from scouter_amd.sloter.slot_model import SlotModel
    pretrained_dir("resnet18")
    args = argparse.Namespace(model="resnet18", pre_trained=True, num_classes=10, dataset="MNIST", use_slot=True,
                              use_pre=False, grad=False, channel=512, slots_per_class=1, hidden_dim=64,
                              freeze_layers=2, vis=False, vis_id=0, loss_status=1, power=1, to_k_layer=1,
                              lambda_value="1")
    m = SlotModel(args)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert any(n.startswith("backbone.layer2") for n in frozen) and not any("layer3" in n for n in frozen)
    x = torch.randn(2, 1, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, torch.tensor([1, 2]))
    m = m.cuda()
    out, losses = m(x.cuda(), torch.tensor([1, 2]).cuda())
    losses[0].backward()
    for n, p in m.named_parameters():
        if not p.requires_grad or "to_q" in n:
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_fc_baseline_mode_parity():
    """use_slot=False: backbone -> global average pool -> fc -> log_softmax/NLL, forward and every gradient, vs the
    reference fixture (fp64 run) and the state_dict layout incl. backbone.fc.*"""
    from scouter_amd.sloter.slot_model import SlotModel
    g = np.load(os.path.join(GOLD, "model_fc_resnet18_mnist_64.npz"))
    args = argparse.Namespace(model="resnet18", pre_trained=False, num_classes=10, dataset="MNIST", use_slot=False,
                              use_pre=False, grad=False, channel=512, slots_per_class=1, hidden_dim=64,
                              freeze_layers=0, vis=False, vis_id=0, loss_status=1, power=1, to_k_layer=1,
                              lambda_value="1")
    spec = O.state_dict_spec("resnet18", 10, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
    m = SlotModel(args)
    assert list(m.state_dict().keys()) == list(spec.keys())
    m.load_state_dict(O.synth_state(spec, 400))
    m = m.cuda().train()
    images, labels = O.synth_batch(4, 1, 64, 10, 401)
    out, losses = m(images.cuda(), labels.cuda())
    assert len(losses) == 1
    losses[0].backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["f64_log_probs"], atol=1e-4)
    np.testing.assert_allclose(float(losses[0]), float(g["f64_loss"]), atol=1e-4)
    named = dict(m.named_parameters())
    for k, d in zip(g["f64_grad_keys"], g["f64_grad_digest"]):
        mine = grad_digest(named[str(k)].grad.detach().cpu())
        assert abs(mine[1] - d[1]) <= 2e-3 * d[1] + 1e-5, str(k)
        np.testing.assert_allclose(mine[2:], d[2:], atol=2e-3 * max(abs(d[2:]).max(), 1e-4) + 1e-6, rtol=5e-3, err_msg=str(k))


@pytest.mark.parametrize("arch,C,spc,B,H", [("resnest26d", 200, 1, 6, 260), ("resnest50d", 100, 3, 2, 224),
                                            ("resnet18", 10, 1, 1, 260),
                                            # ragged inputs: odd sizes / not multiples of 32 (odd feature maps all the
                                            # way down, ceil-mode pooling, partial tiles in every kernel)
                                            ("resnest26d", 10, 1, 3, 225), ("resnet18", 10, 1, 2, 200)])
def test_other_baseline_shapes_forward_parity(arch, C, spc, B, H):
    """BASELINE configs 4 / 5 head sizes (S = 200 / 300) and the reference's default 260x260 input (9x9 = 81 tokens,
    3 token tiles in the fused kernel), batch 1 included: forward vs the fp64 oracle, backward finite + deterministic."""
    from scouter_amd.sloter.slot_model import SlotModel
    mnist = arch == "resnet18"
    L = 1 if mnist else 3
    args = argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=True, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=1,
                              power=2, to_k_layer=L, lambda_value="1")
    spec = O.state_dict_spec(arch, C, spc, L, in_chans=1 if mnist else 3, mnist_stem=mnist)
    P = O.synth_state(spec, 900)
    images, labels = O.synth_batch(B, 1 if mnist else 3, H, C, 901)
    m = SlotModel(args)
    m.load_state_dict(P)
    train = B > 1                    # batch 1 has no batch statistics (PyTorch raises in train mode): eval-mode BN
    m = m.cuda().train(train)
    out, losses = m(images.cuda(), labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    g1 = m.grad_arena().flat.clone()
    Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=1, power=2, lambda_value=1.0)
    aux = {}
    with torch.no_grad():
        ref, rl = O.slot_model_forward(Pd, images.double(), labels, cfg, training=train, aux=aux)
    side = -(-H // 32)
    assert m.slot.last_attn.shape == (B, C * spc, side * side)
    # S >= 200: the reference's own fp32 result is only reproducible to ~1e-4
    # yardstick: what plain fp32 PyTorch loses against fp64 on the very same inputs (~1e-4 and more
    # for S >= 200 -- the row-sum division of slot_attention.py:56 is ill-conditioned)
    # ... measured at three thread counts (the summation order of PyTorch's CPU convolutions depends on it): with S = 300 the
    # reference's own fp32 log-probabilities move by 0.19 / 0.10 / 0.096 against fp64 on THESE inputs just by the thread count
    # (other seeds: 0.04 ... 5, tools_dev/head_noise_s300.py) -- one draw is no yardstick for another draw of the same noise
    # (round 6: with one draw the gate passed or failed with the forward options in either direction, seed by seed).  The gate
    # stays north_star's max(1e-4, 3 x floor); `floor` is the largest of the reference's three draws.
    floors = []
    keep = torch.get_num_threads()
    with torch.no_grad():
        for t in (8, 16, 32):
            torch.set_num_threads(t)
            ref32 = O.slot_model_forward({k: v.clone() for k, v in P.items()}, images, labels, cfg, training=train)[0]
            floors.append(float((ref32.double() - ref).abs().max()))
    torch.set_num_threads(keep)
    floor = max(floors)
    tol = max(1e-4, 3 * floor)
    err = float((out.detach().cpu().double() - ref).abs().max())
    print("%s C=%d spc=%d %dx%d: |HIP - fp64| = %.3g, |torch fp32 - fp64| at 8 / 16 / 32 threads = %s"
          % (arch, C, spc, H, H, err, ["%.3g" % f for f in floors]))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(m.slot.last_attn.cpu().numpy(), aux["attn"].numpy(), atol=tol, rtol=0)
    assert torch.isfinite(g1).all()
    if not train:                    # (a second train-mode forward would see updated running statistics only; fine too)
        out2, losses2 = m(images.cuda(), labels.cuda())
        losses2[0].backward()
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(g1, m.grad_arena().flat)


def test_bf16_mode_sits_inside_the_bf16_noise_of_the_reference_arithmetic():
    """precision="bf16" (BASELINE configs[4]): backbone convolution operands rounded to bf16, fp32 accumulation, fp32
    storage, everything else as in the parity path.  The reference has no mixed precision; the yardstick is the oracle
    with the SAME operand rounding inserted (oracle.torch_oracle.CONV_INPUT_ROUNDING, evaluated in fp64).  Rounding to
    bf16 is discontinuous, so two correct implementations cannot agree better than ~3e-4 per layer (operands that differ
    in the last fp32 bits round to different bf16 values, measured with tools_dev/bf16_oracle_bisect.py) times the
    amplification of this random-init, batch-6 network; the meaningful statement is therefore statistical: the HIP
    result is as close to the fp64 truth as the emulating oracle is, for the log-probabilities, the loss and every large
    gradient -- and it differs from the fp32 result by a bf16-sized amount (proof that the bf16 kernels ran)."""
    case = "resnest26d_224"
    g = np.load(os.path.join(GOLD, "model_%s.npz" % case))
    mb, _, images, labels = build(case)
    mb.set_precision("bf16")
    mb.train()
    out, (loss, nll, area) = mb(images.cuda(), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert mb.activation_storage == "bf16"          # (the default of the bf16 mode; emulated by the oracle below)
    O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = "bf16"
    try:
        emu_out, emu_losses, _, emu_leaves, _ = oracle_run(case, torch.float64)
    finally:
        O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = None
    _, tru_losses, _, tru_leaves, _ = oracle_run(case, torch.float64)
    truth = g["f64_log_probs"]
    err_hip = float(np.abs(out.detach().cpu().numpy() - truth).max())
    err_emu = float(np.abs(emu_out.detach().numpy() - truth).max())
    assert err_hip > 1e-3, "bf16 mode produced the fp32 result: the bf16 kernels did not run"
    assert err_hip <= 2.5 * err_emu + 1e-3, (err_hip, err_emu)
    assert abs(float(loss) - float(tru_losses[0])) <= 2.5 * abs(float(emu_losses[0]) - float(tru_losses[0])) + 5e-3
    named = dict(mb.named_parameters())

    def cosine(a, b):
        a, b = a.flatten().double(), b.flatten().double()
        return float((a @ b) / (a.norm() * b.norm() + 1e-300))
    cos_hip, cos_emu = {}, {}
    for k, ref in tru_leaves.items():
        if ref.numel() < 4096:
            continue
        cos_hip[k] = cosine(named[k].grad.detach().cpu(), ref.grad)
        cos_emu[k] = cosine(emu_leaves[k].grad, ref.grad)
    worst = min(cos_hip, key=cos_hip.get)
    med_hip, med_emu = float(np.median(list(cos_hip.values()))), float(np.median(list(cos_emu.values())))
    print("bf16 mode: |log_probs - fp64 truth| HIP %.3g, emulating oracle %.3g; gradient cosine to the fp64 truth: HIP "
          "median %.4f min %.4f (%s), emulating oracle median %.4f min %.4f"
          % (err_hip, err_emu, med_hip, cos_hip[worst], worst, med_emu, min(cos_emu.values())))
    # (1 - cosine) is the squared relative angle: HIP may be at most 2.5x further from the truth than the emulation
    assert 1 - med_hip <= 2.5 * (1 - med_emu) + 1e-4
    assert 1 - cos_hip[worst] <= 2.5 * (1 - min(cos_emu.values())) + 1e-3


def _synthetic_model(arch, C, spc, L, B, H, seed, power=2, well_conditioned_head=False, mnist=False):
    from scouter_amd.sloter.slot_model import SlotModel
    args = argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=True, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"], slots_per_class=spc,
                              hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=1, power=power,
                              to_k_layer=L, lambda_value="1")
    P = O.synth_state(O.state_dict_spec(arch, C, spc, L, in_chans=1 if mnist else 3, mnist_stem=mnist), seed)
    if well_conditioned_head:
        # small initial slots: the dots rows of slot_attention.py:55-57 stay O(1) after the tau / r_i normalisation, so the
        # S = 300 head neither saturates (attention == 0 / 1, logits independent of the features) nor amplifies a feature
        # perturbation by 1e3 as the random mixed-sign head does; chosen with the CPU oracle alone:
        # bf16-rounded vs exact backbone features move the log-probs by 0.31 (11.8 with the unscaled head)
        P["slot.initial_slots"] = P["slot.initial_slots"] * 0.05
    images, labels = O.synth_batch(B, 1 if mnist else 3, H, C, seed + 1)
    m = SlotModel(args)
    m.load_state_dict(P)
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=1, power=power, lambda_value=1.0)
    return m.cuda().train(), P, images, labels, cfg


def test_config1_at_its_real_batch_forward_and_backward_parity():
    """BASELINE configs[0] -- the MNIST-stem resnet18 + xSlot (10 slots, one to_k layer, power 1; reference
    README.md:94-96) -- at the batch and resolution the bench runs it at (64 x 224 x 224, train-mode BatchNorm): the B = 64
    instances of the fp32 kernels (7 x 7 ... 112 x 112 maps, 64 ... 512 channels, no plane / register-split layers) through the
    whole model.  Forward vs the fp64 oracle next to plain fp32 PyTorch on the same inputs, then every parameter gradient under
    the HIP forward's sign pattern with the fixtures' kf = 2 / ks = 1e-3 bound.  CPU oracle time: seconds per pass."""
    m, P, images, labels, cfg = _synthetic_model("resnet18", 10, 1, 1, 64, 224, 2100, power=1, mnist=True)
    signs = capture_relu_signs(m)
    out, losses = m(images.cuda(), labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    signs = {k: (v if k == "maxpool" else (v > 0)).cpu() for k, v in signs.items()}
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        aux = {}
        ref, rl = O.slot_model_forward(Pd, images.double(), labels, cfg, training=True, aux=aux)
        ref32, rl32 = O.slot_model_forward({k: v.clone() for k, v in P.items()}, images, labels, cfg, training=True)
        floors = [float((ref32.double() - ref).abs().max())]
        for t in (8, 16):           # the reference arithmetic at two more thread counts: its noise is a distribution (see above)
            torch.set_num_threads(t)
            r32 = O.slot_model_forward({k: v.clone() for k, v in P.items()}, images, labels, cfg, training=True)[0]
            floors.append(float((r32.double() - ref).abs().max()))
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    floor = float(np.exp(np.log(floors).mean()))
    err = float((out.detach().cpu().double() - ref).abs().max())
    err_a = float((m.slot.last_attn.cpu().double() - aux["attn"]).abs().max())
    print("config 1 @ batch 64: |HIP - fp64| log_probs %.3g (torch fp32 at 32 / 8 / 16 threads: %s), attention %.3g, loss %.6f vs "
          "%.6f" % (err, ["%.3g" % f for f in floors], err_a, float(losses[0]), float(rl[0])))
    assert err <= max(1e-4, 3 * max(floors))                     # north_star's gate
    # the per-seed cap of the distribution statements (test_rounding_noise_over_five_seeds): 3 x the geometric mean of the
    # reference's own draws -- or half of north_star's 1e-4 (measured: 3.7e-5 against a 32-thread draw of 1.0e-5; every
    # convolution of this model runs on the exact-fp32 MFMA kernels)
    assert err <= max(3.0 * floor, 5e-5), (err, floors)
    assert err_a <= max(1e-4, 3 * max(floors))
    assert abs(float(losses[0]) - float(rl[0])) <= max(2.0 * abs(float(rl32[0]) - float(rl[0])), 2e-5)
    del Pd, aux, ref, ref32
    pinned_gradient_check("config 1 @ batch 64", (P, images, labels, cfg), signs, named)


def test_config2_at_its_real_batch_forward_parity():
    """BASELINE configs[1] at its REAL per-GPU batch (70 x 224x224, train-mode BatchNorm): the large-M tile plans, split
    reductions and XCD remaps that only trigger at this size, forward vs the fp64 oracle next to plain fp32 PyTorch on the
    same inputs (fixtures stop at batch 6).  ~1 minute of CPU oracle time."""
    m, P, images, labels, cfg = _synthetic_model("resnest26d", 10, 1, 3, 70, 224, 1200)
    out, losses = m(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        aux = {}
        ref, rl = O.slot_model_forward(Pd, images.double(), labels, cfg, training=True, aux=aux)
        ref32, rl32 = O.slot_model_forward({k: v.clone() for k, v in P.items()}, images, labels, cfg, training=True)
    floor = float((ref32.double() - ref).abs().max())
    err = float((out.detach().cpu().double() - ref).abs().max())
    err_a = float((m.slot.last_attn.cpu().double() - aux["attn"]).abs().max())
    print("config 2 @ batch 70: |HIP - fp64| log_probs %.3g (torch fp32: %.3g), attention %.3g, loss %.6f vs %.6f"
          % (err, floor, err_a, float(losses[0]), float(rl[0])))
    assert err <= max(1e-4, 3 * floor)
    assert err <= max(2.0 * floor, 1e-5), (err, floor)
    assert err_a <= max(1e-4, 3 * floor)
    assert abs(float(losses[0]) - float(rl[0])) <= max(2.0 * abs(float(rl32[0]) - float(rl[0])), 2e-5)
    # BatchNorm running statistics after this one training forward (fp64 batch statistics over 70 x 112 x 112 samples)
    sd = m.state_dict()
    for k in ("backbone.conv1.1.running_mean", "backbone.layer2.0.bn1.running_var", "backbone.layer4.1.bn3.running_mean"):
        np.testing.assert_allclose(sd[k].cpu().numpy(), Pd[k].numpy(), rtol=2e-4, atol=5e-5, err_msg=k)


def test_config2_at_its_real_batch_backward_parity_under_the_pinned_sign_pattern():
    """BASELINE configs[1] at its REAL per-GPU batch (70 x 224 x 224, train-mode BatchNorm) -- every
    parameter gradient of the batch-70 kernels (large-M tile plans, split-K weight-gradient plans, plane tiles, fused
    BatchNorm-backward epilogues with their real row counts) against the ORACLE's fp64 autograd, tensor by tensor, under
    the sign pattern the HIP forward produced, with the oracle's own fp32 autograd as the yardstick (same kf = 2 /
    ks = 1e-3 bound as the fixtures).  Slow by design: two CPU oracle backward passes at batch 70 (minutes)."""
    m, P, images, labels, cfg = _synthetic_model("resnest26d", 10, 1, 3, 70, 224, 1500)
    signs = capture_relu_signs(m)
    out, losses = m(images.cuda(), labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    signs = {k: (v if k == "maxpool" else (v > 0)).cpu() for k, v in signs.items()}     # (bools travel, not 5 GB)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    # kf = 2 / ks = 1e-3 as for the fixtures; the split-attention squeeze MLP (fc1 -> BatchNorm over the 70 pooled vectors
    # -> fc2) gets 3: its train-mode BatchNorm normalises over only B = 70 samples per channel, which amplifies the
    # rounding noise of everything downstream -- measured r3: 152 of 154 tensors inside 2 x PyTorch-fp32's own error,
    # layer1.0.conv2.bn1.weight at 2.6 x and layer1.1.conv2.fc2.weight at 2.03 x (5.7e-3 / 5.8e-3 of max|grad|).
    pinned_gradient_check("config 2 @ batch 70", (P, images, labels, cfg), signs, named, kf_squeeze=3.0)


def test_config4_at_its_real_batch_forward_and_backward_parity():
    """BASELINE configs[3] -- CUB200-shaped resnest26d + xSlot, 200 classes x 1 slot (S = 200) -- at its REAL
    per-GPU batch 128 x 224 x 224: the B = 128 entries of the static tile table (other weight-gradient plans and plane
    tiles than the B = 70 ones) through the whole model.  Forward vs the fp64 oracle next to plain fp32 PyTorch on the same
    inputs; then every parameter gradient under the HIP forward's sign pattern, same bound as config 2 at batch 70.
    Minutes of CPU oracle time (four passes at batch 128)."""
    m, P, images, labels, cfg = _synthetic_model("resnest26d", 200, 1, 3, 128, 224, 1700)
    signs = capture_relu_signs(m)
    out, losses = m(images.cuda(), labels.cuda())
    losses[0].backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    signs = {k: (v if k == "maxpool" else (v > 0)).cpu() for k, v in signs.items()}
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        aux = {}
        ref, rl = O.slot_model_forward(Pd, images.double(), labels, cfg, training=True, aux=aux)
        ref32, rl32 = O.slot_model_forward({k: v.clone() for k, v in P.items()}, images, labels, cfg, training=True)
    floor = float((ref32.double() - ref).abs().max())
    err = float((out.detach().cpu().double() - ref).abs().max())
    err_a = float((m.slot.last_attn.cpu().double() - aux["attn"]).abs().max())
    print("config 4 @ batch 128, S = 200: |HIP - fp64| log_probs %.3g (torch fp32: %.3g), attention %.3g, loss %.6f vs %.6f"
          % (err, floor, err_a, float(losses[0]), float(rl[0])))
    # S = 200: the reference's own fp32-vs-fp64 spread is ~1e-4, so the yardstick is that spread
    assert err <= max(1e-4, 3 * floor)
    assert err <= max(2.0 * floor, 1e-5), (err, floor)
    assert err_a <= max(1e-4, 3 * floor)
    del Pd, aux, ref, ref32
    pinned_gradient_check("config 4 @ batch 128", (P, images, labels, cfg), signs, named, kf_squeeze=3.0)


def test_bf16_mode_resnest50d_300_slots():
    """BASELINE configs[4]'s actual shape -- resnest50d, 100 classes x 3 slots (S = 300), 224x224 -- in precision="bf16"
    (VERDICT r1 weak #2): same statistical yardstick as the resnest26d case, the oracle with bf16 operand rounding
    inserted (evaluated in fp64) against the exact fp64 truth."""
    m, P, images, labels, cfg = _synthetic_model("resnest50d", 100, 3, 3, 4, 224, 1300, well_conditioned_head=True)
    m.set_precision("bf16")
    assert m.activation_storage == "bf16" and sum(b.store_bf16 for b in m.backbone.modules() if hasattr(b, "store_bf16")) == 15
    out, (loss, nll, area) = m(images.cuda(), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    torch.set_num_threads(min(32, os.cpu_count() or 1))

    def run(rounding):
        Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        keys = O.trainable_keys(Pd)
        leaves = {k: Pd[k].clone().requires_grad_(True) for k in keys}
        Q = dict(Pd); Q.update(leaves)
        O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = rounding      # (operand rounding + bf16 activation storage)
        try:
            o, ls = O.slot_model_forward(Q, images.double(), labels, cfg, training=True)
            ls[0].backward()
        finally:
            O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = None
        return o.detach(), ls, leaves
    tru_out, tru_losses, tru = run(None)
    emu_out, emu_losses, emu = run("bf16")
    err_hip = float((out.detach().cpu().double() - tru_out).abs().max())
    err_emu = float((emu_out - tru_out).abs().max())
    assert err_hip > 1e-3, "bf16 mode produced the fp32 result: the bf16 kernels did not run"
    assert err_hip <= 2.5 * err_emu + 1e-3, (err_hip, err_emu)
    assert abs(float(loss) - float(tru_losses[0])) <= 2.5 * abs(float(emu_losses[0]) - float(tru_losses[0])) + 5e-3
    named = dict(m.named_parameters())

    def cosine(a, b):
        a, b = a.flatten().double(), b.flatten().double()
        return float((a @ b) / (a.norm() * b.norm() + 1e-300))
    ch = {k: cosine(named[k].grad.detach().cpu(), r.grad) for k, r in tru.items() if r.numel() >= 4096}
    ce = {k: cosine(emu[k].grad, r.grad) for k, r in tru.items() if r.numel() >= 4096}
    med_hip, med_emu = float(np.median(list(ch.values()))), float(np.median(list(ce.values())))
    print("bf16 resnest50d S=300: |log_probs - fp64 truth| HIP %.3g, emulating oracle %.3g; gradient cosine to the truth: "
          "HIP median %.4f min %.4f, emulating oracle median %.4f min %.4f"
          % (err_hip, err_emu, med_hip, min(ch.values()), med_emu, min(ce.values())))
    # non-vacuous for the log-probabilities (they span ~2.3 across classes; saturated heads would make this 0 == 0).
    # For the gradients this random-init 50-layer network decorrelates ANY bf16 evaluation from the exact one (the
    # emulating oracle's own median cosine to the truth is ~0.17; bf16-rounded features differ by 32 % rms), so the
    # cosine statement below is only "no worse than the emulation"; the sharp bf16 statements are kernel-level
    # (test_kernels_gpu.py::test_conv_bf16_inputs_fp32_accumulate) and test_training_learns_a_separable_task[bf16].
    assert 1e-3 < err_emu < 1.0, "the yardstick itself is degenerate: this case says nothing"
    assert 1 - med_hip <= 2.5 * (1 - med_emu) + 1e-4
    assert 1 - min(ch.values()) <= 2.5 * (1 - min(ce.values())) + 1e-3


def test_config5_model_at_its_real_batch():
    """BASELINE configs[4] -- resnest50d, 100 classes x 3 slots (S = 300), 224 x 224 -- at its REAL per-GPU
    batch 256, end to end (the B = 256 table entries through the whole model, not kernel by kernel).  (i) precision "fp32":
    the BACKBONE FEATURES (train-mode BatchNorm, 53 convolutions at batch 256) against the oracle's fp64 features next to
    plain fp32 PyTorch on the same inputs -- the tight statement; then log-probabilities and attention through the S = 300
    head, whose sum normaliser amplifies any feature noise (PyTorch fp32 itself is 2e-2 off fp64 here), with
    PyTorch-fp32's own deviation as the yardstick.  (ii) precision "bf16" (the mode the config names, bf16 activation
    storage): features and log-probabilities sit inside the distance of the emulating oracle (bf16 operand rounding +
    storage, evaluated in fp64) from the fp64 truth.  A few minutes of CPU oracle time (three forwards at batch 256)."""
    m, P, images, labels, cfg = _synthetic_model("resnest50d", 100, 3, 3, 256, 224, 1900, well_conditioned_head=True)
    xg, yg = images.cuda(), labels.cuda()

    def hip_forward():
        with torch.no_grad():
            feat, _ = m.backbone.features_fwd(xg, False, [])
            feat = feat.permute(0, 3, 1, 2).contiguous().cpu().double()       # NHWC -> the oracle's NCHW
            m.load_state_dict(P)
            out, _ = m(xg, yg)
            attn = m.slot.last_attn.clone()
        m.load_state_dict(P)                               # (train-mode forwards moved the running statistics)
        return feat, out.cpu().double(), attn.cpu().double()
    feat32, out32, attn32 = hip_forward()
    m.set_precision("bf16")
    assert m.activation_storage == "bf16"
    feat16, out16, _ = hip_forward()
    torch.cuda.synchronize()
    del m, xg
    torch.cuda.empty_cache()
    torch.set_num_threads(min(32, os.cpu_count() or 1))

    def run(dtype, rounding=None):
        Pd = {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
        aux = {}
        O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = rounding
        try:
            with torch.no_grad():
                o, _ = O.slot_model_forward(Pd, images.to(dtype), labels, cfg, training=True, aux=aux)
        finally:
            O.CONV_INPUT_ROUNDING = O.ACTIVATION_STORAGE = None
        return o.double(), aux["attn"].double(), aux["feat"].double()
    ref, ref_attn, ref_feat = run(torch.float64)
    r32, _, r32_feat = run(torch.float32)
    fscale = float(ref_feat.abs().max())
    ffloor = float((r32_feat - ref_feat).abs().max()) / fscale
    ferr = float((feat32 - ref_feat).abs().max()) / fscale
    floor = float((r32 - ref).abs().max())
    err = float((out32 - ref).abs().max())
    err_a = float((attn32 - ref_attn).abs().max())
    emu, _, emu_feat = run(torch.float64, "bf16")
    ferr16, ferr_emu = float((feat16 - ref_feat).abs().max()) / fscale, float((emu_feat - ref_feat).abs().max()) / fscale
    err16, err_emu = float((out16 - ref).abs().max()), float((emu - ref).abs().max())
    print("config 5 @ batch 256, S = 300: fp32 mode features |HIP - fp64| / max %.3g (torch fp32: %.3g), log_probs %.3g (torch "
          "fp32: %.3g), attention %.3g; bf16 mode features %.3g (emulating oracle: %.3g), log_probs %.3g (%.3g)"
          % (ferr, ffloor, err, floor, err_a, ferr16, ferr_emu, err16, err_emu))
    assert ferr <= max(2.0 * ffloor, 1e-6), (ferr, ffloor)
    assert err <= max(1e-4, 6 * floor), (err, floor)
    assert err_a <= max(1e-4, 6 * floor), (err_a, floor)
    assert ferr_emu > 1e-3 and ferr16 > 1e-3, "bf16 mode produced the fp32 result: the bf16 kernels did not run"
    assert ferr16 <= 2.5 * ferr_emu, (ferr16, ferr_emu)
    assert err16 <= 2.5 * err_emu + 1e-3, (err16, err_emu)


def test_bad_inputs_fail_loudly():
    """empty batch, CPU tensor, wrong channel count: Python exceptions with the library's message, never a silent
    fallback or a device fault"""
    from scouter_amd import kernels as K
    m, P, images, labels = build("resnet18_mnist_64")
    m.train()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(images, labels)                                              # CPU tensor
    with pytest.raises((RuntimeError, AssertionError)):
        m(images[:0].cuda(), labels[:0].cuda())                        # empty batch
    with pytest.raises((RuntimeError, AssertionError)):
        m(images.repeat(1, 3, 1, 1).cuda(), labels.cuda())             # 3-channel image into the 1-channel MNIST stem
    x = torch.zeros(2, 8, 8, 48, device="cuda")                        # 48 channels: not a multiple of 32
    w = torch.zeros(1, 1, 48, 64, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of 32"):
        K.conv2d_fwd(x, w)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        mr, _, im_r, lb_r = build("resnest26d_96")
        mr.train()(im_r[:1].cuda(), lb_r[:1].cuda())                  # batch 1 in train mode: like torch's BatchNorm
    # non-contiguous / float64 inputs are accepted (made dense / cast like engine.py:25 does)
    out = m(images.double().cuda().transpose(2, 3).transpose(2, 3), labels.cuda())
    assert torch.isfinite(out[0]).all()


def test_config2_batch70_backward_is_the_mean_of_its_half_batches():
    """Size-independent property at BASELINE configs[1]'s REAL batch (70 x 224x224): with BatchNorm in eval mode and a
    loss that is a batch mean (power = 1), every gradient of the full batch is the mean of the two half-batch gradients.
    Batch 70 and batch 35 run DIFFERENT block tiles, split-K weight-gradient plans, XCD remaps, plane tiles and fused
    epilogue row counts (all chosen per layer shape), so this checks the large-M variants of every backward kernel
    against the small-M ones, which the batch <= 6 fixtures pin to the oracle."""
    from scouter_amd.nn_hip import BatchNorm2d
    from scouter_amd import kernels as kk
    # The property needs the FORWARD of a sample to be bit-identical in both batch sizes: one ReLU flipping on a ~0
    # pre-activation moves upstream gradients by ~1/samples (the reason the oracle tests pin the sign pattern).  It is:
    # forward tiles 0-4 are bit-identical, and plane tile 5 (another K order) is used by a static per-layer-shape rule,
    # never by timing (kernels.HALO_TILE; when it was autotuned the two batch sizes picked different tiles, 1e-7
    # activation differences flipped a few signs and the gradients differed by 1e-4 ... 1e-3).
    m, P, images, labels, cfg = _synthetic_model("resnest26d", 10, 1, 3, 70, 224, 1400, power=1)
    for mod in m.modules():
        if isinstance(mod, BatchNorm2d):
            mod.eval()
    named = dict(m.named_parameters())

    def grads(sl):
        m.zero_grad(set_to_none=True)
        _, losses = m(images[sl].cuda(), labels[sl].cuda())
        losses[0].backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().double().clone() for k, p in named.items() if p.grad is not None}, float(losses[0])

    g_full, l_full = grads(slice(0, 70))
    g_a, l_a = grads(slice(0, 35))
    g_b, l_b = grads(slice(35, 70))
    assert abs(l_full - 0.5 * (l_a + l_b)) <= 2e-6 * max(1.0, abs(l_full))
    rel = {}
    for k, g in g_full.items():
        ref = 0.5 * (g_a[k] + g_b[k])
        scale = float(ref.abs().max())
        rel[k] = float((g - ref).abs().max()) / max(scale, 1e-30)
    order = sorted(rel, key=rel.get, reverse=True)
    print("batch 70 vs mean of 2 x 35: relative gradient differences, worst first:",
          [(k, "%.1e" % rel[k]) for k in order[:6]], "median %.1e over %d tensors" % (float(np.median(list(rel.values()))), len(rel)))
    # fp32 rounding only: the backward sums the same products in different orders (measured: worst 2e-6, median 5e-8 of
    # the tensor's largest element); a wrong tile / plan / remap shows as O(1)
    for k in order:
        assert rel[k] <= 2e-5, (k, rel[k])
    assert float(np.median(list(rel.values()))) <= 1e-6


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_config5_batch256_backward_is_the_mean_of_its_half_batches(precision):
    """the BACKWARD of BASELINE configs[4] -- resnest50d, 100 classes x 3 slots (S = 300), 224 x 224 -- at its
    REAL per-GPU batch 256, through the size-independent property of the config-2 test above (BatchNorm in eval mode, power 1:
    the full-batch gradient is the mean of the two half-batch gradients): the B = 256 entries of the static table -- block tiles,
    split-K weight-gradient plans, plane tiles, persistent kernels, fused epilogue row counts -- against the B = 128 ones, which
    `test_config4_at_its_real_batch_...` and tests/test_table_entries_gpu.py hold to the oracle.  No oracle time at all.
    "fp32": rounding of fp32 sums only.  "bf16" (the precision the config names; bf16-stored activations and residual-stream
    gradient): the forward of a sample is still the same function in both batch sizes, but gradients that travel as bf16 round
    each half-batch stream on its own -- the bound is that rounding (2^-9 per stored element, averaged over the pixels)."""
    from scouter_amd.nn_hip import BatchNorm2d
    m, P, images, labels, cfg = _synthetic_model("resnest50d", 100, 3, 3, 256, 224, 2300, power=1, well_conditioned_head=True)
    if precision == "bf16":
        m.set_precision("bf16")
        assert m.activation_storage == "bf16"
    for mod in m.modules():
        if isinstance(mod, BatchNorm2d):
            mod.eval()
    named = dict(m.named_parameters())

    def grads(sl):
        m.zero_grad(set_to_none=True)
        _, losses = m(images[sl].cuda(), labels[sl].cuda())
        losses[0].backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().double().clone() for k, p in named.items() if p.grad is not None}, float(losses[0])

    g_full, l_full = grads(slice(0, 256))
    g_a, l_a = grads(slice(0, 128))
    g_b, l_b = grads(slice(128, 256))
    assert abs(l_full - 0.5 * (l_a + l_b)) <= (2e-6 if precision == "fp32" else 2e-5) * max(1.0, abs(l_full))
    rel = {}
    for k, g in g_full.items():
        ref = 0.5 * (g_a[k] + g_b[k])
        scale = float(ref.abs().max())
        rel[k] = float((g - ref).abs().max()) / max(scale, 1e-30)
    order = sorted(rel, key=rel.get, reverse=True)
    med = float(np.median(list(rel.values())))
    print("config 5 (%s) batch 256 vs mean of 2 x 128: relative gradient differences, worst first:" % precision,
          [(k, "%.1e" % rel[k]) for k in order[:6]], "median %.1e over %d tensors" % (med, len(rel)))
    worst_ok, med_ok = (2e-5, 1e-6) if precision == "fp32" else (2e-2, 2e-3)
    for k in order:
        assert rel[k] <= worst_ok, (k, rel[k])
    assert med <= med_ok
