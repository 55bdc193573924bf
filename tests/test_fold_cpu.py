"""The algebra of the BatchNorm-folded inference path (SlotModel.set_inference_fold), on the CPU in fp64: folding every
(convolution, BatchNorm) pair the model names (SlotModel.fold_pairs) into the convolution and replacing the BatchNorm by
the identity must leave the eval forward of the oracle unchanged -- for the three backbones, which between them have the
fc1 bias term, the downsample branch, the deep stem and the MNIST stem."""
import argparse

import pytest
import torch

from oracle import torch_oracle as O

EPS = 1e-5          # nn.BatchNorm2d default (oracle.torch_oracle._bn)

CASES = {       # arch, classes, slots per class, to_k layers, loss_status, power, batch, size, in_chans, mnist
    "resnet18_mnist": ("resnet18", 10, 1, 1, 1, 1, 3, 64, 1, True),
    "resnest26d": ("resnest26d", 10, 1, 3, 1, 2, 2, 96, 3, False),
    "resnest50d": ("resnest50d", 12, 3, 3, -1, 2, 2, 64, 3, False),
}


def model_args(arch, C, spc, L, ls, power, mnist, use_slot=True, precision="fp32"):
    return argparse.Namespace(model=arch, pre_trained=False, num_classes=C, dataset="MNIST" if mnist else "ImageNet",
                              use_slot=use_slot, use_pre=False, grad=False, channel=O.ARCHS[arch]["channel"],
                              slots_per_class=spc, hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=ls,
                              power=power, to_k_layer=L, lambda_value="1", precision=precision)


def fold_pair_fp64(w_oihw, conv_bias, gamma, beta, mean, var, eps=EPS):
    """The fold as the issue states it, every product in fp64: s = gamma / sqrt(var + eps), w' = w * s per output channel,
    b' = beta - mean * s (+ conv_bias * s).  Tensors of any float type in, fp64 out."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    w = w_oihw.double() * s.view(-1, 1, 1, 1)
    b = beta.double() - mean.double() * s
    if conv_bias is not None:
        b = b + conv_bias.double() * s
    return w, b


def fold_state(P, pairs):
    """fp64 state dict with every pair folded and its BatchNorm made the identity (gamma 1, mean 0, var 1 - eps).  The
    oracle's bias-less convolutions have nowhere to put b', so there it rides on the identity BatchNorm's beta (beta = 0
    where the convolution has a bias of its own: fc1)."""
    Q = {k: (v.double().clone() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    for conv, bn in pairs:
        cb = Q.get(conv + ".bias")
        w, b = fold_pair_fp64(Q[conv + ".weight"], cb, Q[bn + ".weight"], Q[bn + ".bias"], Q[bn + ".running_mean"],
                              Q[bn + ".running_var"])
        Q[conv + ".weight"] = w
        Q[bn + ".weight"] = torch.ones_like(b)
        Q[bn + ".running_mean"] = torch.zeros_like(b)
        Q[bn + ".running_var"] = torch.full_like(b, 1.0 - EPS)
        if cb is not None:
            Q[conv + ".bias"], Q[bn + ".bias"] = b, torch.zeros_like(b)
        else:
            Q[bn + ".bias"] = b
    return Q


@pytest.mark.parametrize("case", sorted(CASES))
def test_folded_state_gives_the_unfolded_eval_forward_in_fp64(case):
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = CASES[case]
    spec = O.state_dict_spec(arch, C, spc, L, in_chans=in_chans, mnist_stem=mnist)
    P = O.synth_state(spec, 410)
    images, labels = O.synth_batch(B, in_chans, H, C, 411)
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist))
    assert list(m.state_dict().keys()) == list(spec.keys())
    assert not m.inference_fold                                  # off by default
    pairs = m.fold_pairs()
    # every BatchNorm of the model is folded exactly once, into a convolution of the state dict
    bns = [k[:-len(".running_mean")] for k in spec if k.endswith(".running_mean")]
    assert sorted(b for _, b in pairs) == sorted(bns) and len(set(c for c, _ in pairs)) == len(pairs)
    assert all(c + ".weight" in spec and len(spec[c + ".weight"]) == 4 for c, _ in pairs)
    with_bias = [c for c, _ in pairs if c + ".bias" in spec]
    assert all(c.endswith(".conv2.fc1") for c in with_bias) and bool(with_bias) == (arch != "resnet18")
    cfg = dict(model=arch, num_classes=C, slots_per_class=spc, loss_status=ls, power=power, lambda_value=1.0)
    Pd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in P.items()}
    with torch.no_grad():
        ref, ref_losses = O.slot_model_forward(Pd, images.double(), labels, cfg, training=False)
        out, losses = O.slot_model_forward(fold_state(P, pairs), images.double(), labels, cfg, training=False)
    err = float((out - ref).abs().max())
    print(case, "max |folded - unfolded| (fp64 log-probabilities) = %.3g over %d pairs" % (err, len(pairs)))
    assert err <= 1e-10, err
    assert abs(float(losses[0]) - float(ref_losses[0])) <= 1e-10


def test_switch_keeps_the_state_dict_and_is_off_in_train_mode():
    from scouter_amd.sloter.slot_model import SlotModel
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = CASES["resnet18_mnist"]
    m = SlotModel(model_args(arch, C, spc, L, ls, power, mnist))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.set_inference_fold(True)
    after = m.state_dict()
    assert list(after.keys()) == list(before.keys()) and all(torch.equal(after[k], before[k]) for k in before)
    assert m.inference_fold and m._fold_stale
    m._fold_stale = False
    for event in (m.eval, m.train, m.refold, lambda: m.load_state_dict(before), lambda: m.set_precision("fp32"),
                  lambda: m.set_planes(3), lambda: m.set_x3(0), m.float):
        event()
        assert m._fold_stale, event
        m._fold_stale = False
