"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/*.npz by running the *reference itself* (imported
read-only from /root/reference through oracle/ref_import.py) on seeded synthetic parameters and inputs.

Run in the build container only:   python -m oracle.gen_golden
Only OUTPUTS are stored; every input / parameter is re-drawn from numpy.random.default_rng(seed) through
oracle.torch_oracle.{state_dict_spec, synth_state, synth_batch}, so the fixtures stay small.

Fixture families
  head_<name>.npz    reference SlotAttention (+conv1x1/PE/loss glue of SlotModel.forward) on random features
  model_<name>.npz   reference SlotModel fwd+bwd (whole network), fp32 and an fp64 "truth" run
  engine_mnist.npz   reference engine.train_one_epoch + evaluate, 2 steps of config 1 (batch 16, 128x128): record +
                     parameter digests
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_import as R          # noqa: E402
from oracle import torch_oracle as O        # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# name -> (C, spc, N-side, L, loss_status, power, B, Cin)  -- the five BASELINE configs' head shapes + edge cases
HEAD_CASES = {
    "c1_mnist": (10, 1, 9, 1, 1, 1, 4, 512),
    "c2_in10_pos": (10, 1, 7, 3, 1, 2, 4, 2048),
    "c3_in10_neg": (10, 1, 7, 3, -1, 2, 4, 2048),
    "c4_cub200": (200, 1, 7, 3, 1, 2, 3, 2048),
    "c5_in100_spc3": (100, 3, 7, 3, 1, 2, 3, 2048),
    "tiny_spc2": (3, 2, 3, 2, 1, 1, 2, 64),
    "one_token": (5, 1, 1, 1, 1, 2, 2, 64),
    "grid9_spc3": (7, 3, 9, 3, -1, 2, 2, 256),
}

# name -> (arch, C, spc, L, ls, power, B, H, in_chans, mnist)
MODEL_CASES = {
    "resnet18_mnist_64": ("resnet18", 10, 1, 1, 1, 1, 4, 64, 1, True),
    "resnest26d_96": ("resnest26d", 10, 1, 3, 1, 2, 4, 96, 3, False),
    "resnest26d_224": ("resnest26d", 10, 1, 3, 1, 2, 6, 224, 3, False),
    "resnest50d_64_spc3": ("resnest50d", 12, 3, 3, -1, 2, 3, 64, 3, False),
}
LAMBDA = "1"
ENGINE_BATCH, ENGINE_SIZE = 16, 128      # engine fixture: 2 AdamW steps of config 1 at reduced batch / resolution
GEN_THREADS = 8                          # intra-op threads the head / model / engine fixtures were recorded with


def head_inputs(case, seed=100):
    C, spc, side, L, ls, power, B, Cin = HEAD_CASES[case]
    rng = np.random.default_rng(seed)
    feat = np.maximum(rng.standard_normal((B, Cin, side, side)), 0.0).astype(np.float32)  # post-ReLU backbone output
    labels = rng.integers(0, C, B).astype(np.int64)
    spec = {k: v for k, v in O.state_dict_spec("resnet18", C, spc, L).items()
            if not k.startswith("backbone.")}
    spec["conv1x1.weight"] = (64, Cin, 1, 1)
    P = O.synth_state(spec, seed + 1)
    return torch.from_numpy(feat), torch.from_numpy(labels), P


def run_reference_head(case, dtype):
    """Reference SlotAttention + the glue lines of SlotModel.forward (slot_model.py:108-121), verbatim calls."""
    C, spc, side, L, ls, power, B, Cin = HEAD_CASES[case]
    feat, labels, P = head_inputs(case)
    R.install_shims()
    from sloter.utils.position_encode import build_position_encoding   # noqa: reference
    slot = R.build_reference_slot_attention(C, spc, 64, loss_status=ls, power=power, to_k_layer=L)
    slot.load_state_dict({k[5:]: v for k, v in P.items() if k.startswith("slot.")})
    conv = torch.nn.Conv2d(Cin, 64, 1)
    conv.load_state_dict({"weight": P["conv1x1.weight"], "bias": P["conv1x1.bias"]})
    pos = build_position_encoding("sine", hidden_dim=64)
    slot, conv = slot.to(dtype), conv.to(dtype)
    feat = feat.to(dtype).requires_grad_(True)
    store = []
    with R.capture_python_sigmoid(store):
        x = torch.relu(conv(feat))
        pe = pos(x)
        x_pe = x + pe
        b, n, r, c = x.shape
        x = x.reshape((b, n, -1)).permute((0, 2, 1))
        x_pe = x_pe.reshape((b, n, -1)).permute((0, 2, 1))
        logits, attn_loss = slot(x_pe, x)
    output = torch.nn.functional.log_softmax(logits, dim=1)
    nll = torch.nn.functional.nll_loss(output, labels)
    loss = nll + float(LAMBDA) * attn_loss
    loss.backward()
    # dfeat / d_conv_w are large (B*Cin*N, d*Cin): keep a digest + a leading sub-block (channels 0..15 / 0..31)
    res = dict(logits=logits, log_probs=output, loss=loss, nll=nll, area=attn_loss, attn=store[-1],
               pe=pe[0], dfeat_head=feat.grad[:, :16], dfeat_digest=torch.from_numpy(grad_digest(feat.grad)),
               d_conv_w_head=conv.weight.grad[:, :32],
               d_conv_w_digest=torch.from_numpy(grad_digest(conv.weight.grad)), d_conv_b=conv.bias.grad)
    for k, p in slot.named_parameters():
        res["d_slot." + k] = p.grad if p.grad is not None else torch.zeros(0)
    res["vis"] = torch.from_numpy(reference_vis_pngs(slot, x_pe.detach(), x.detach(), C))
    return {k: v.detach().numpy() for k, v in res.items()}


def reference_vis_pngs(slot, x_pe, x, C):
    """The reference's OWN --vis output (sloter/utils/slot_attention.py:68-85): a second forward of the same module with
    vis=True / vis_id=0 in a scratch working directory holding `sloter/vis/`; the `slot_{id}.png` files it writes are read
    back -> uint8 [C, side, side].  (Round 2 applied the oracle's vis_maps to the captured attention instead, which pinned
    the oracle to itself.)"""
    import contextlib
    import io
    import tempfile
    from PIL import Image
    side = int(x.shape[1] ** 0.5)
    cwd = os.getcwd()
    slot.vis, slot.vis_id = True, 0
    try:
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "sloter", "vis"))
            os.chdir(tmp)
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                slot(x_pe, x)
            maps = np.stack([np.array(Image.open(os.path.join(tmp, "sloter", "vis", "slot_%d.png" % i))) for i in range(C)])
    finally:
        os.chdir(cwd)
        slot.vis = False
    assert maps.dtype == np.uint8 and maps.shape == (C, side, side), (maps.dtype, maps.shape)
    return maps


def model_inputs(case, seed=200):
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec = O.state_dict_spec(arch, C, spc, L, in_chans=in_chans, mnist_stem=mnist)
    P = O.synth_state(spec, seed)
    images, labels = O.synth_batch(B, in_chans, H, C, seed + 1)
    return spec, P, images, labels


def grad_digest(g):
    """A gradient tensor reduced to (sum, abs-sum, first 16 entries) -- enough to pin it, small enough to commit."""
    f = g.detach().double().flatten()
    head = np.zeros(16)
    head[:min(16, f.numel())] = f[:16].numpy()
    return np.concatenate([[f.sum().item(), f.abs().sum().item()], head])


def run_reference_model(case, dtype):
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[case]
    spec, P, images, labels = model_inputs(case)
    args = R.make_args(model=arch, num_classes=C, slots_per_class=spc, channel=O.ARCHS[arch]["channel"],
                       to_k_layer=L, power=power, loss_status=ls, lambda_value=LAMBDA,
                       dataset="MNIST" if mnist else "ImageNet")
    m = R.build_reference_slot_model(args, feature_size=-(-H // 32))
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys()), "state_dict_spec order/keys differ from the reference"
    for k in sd:
        assert tuple(sd[k].shape) == tuple(spec[k]), (k, sd[k].shape, spec[k])
    m.load_state_dict(P)
    m = m.to(dtype)
    m.train()
    store = []
    with R.capture_python_sigmoid(store):
        out, losses = m(images.to(dtype), labels)
    losses[0].backward()
    res = dict(log_probs=out, loss=losses[0], nll=losses[1], area=losses[2], attn=store[-1])
    grads = {k: p.grad for k, p in m.named_parameters()}
    res["grad_keys"] = np.array([k for k in grads if grads[k] is not None])
    res["grad_digest"] = np.stack([grad_digest(grads[k]) for k in grads if grads[k] is not None])
    sd2 = m.state_dict()
    bn_keys = [k for k in sd2 if k.endswith("running_mean") or k.endswith("running_var")]
    res["bn_digest"] = np.stack([grad_digest(sd2[k]) for k in bn_keys])
    res["unused"] = np.array([k for k in grads if grads[k] is None])
    out_np = {}
    for k, v in res.items():
        out_np[k] = v.detach().numpy() if isinstance(v, torch.Tensor) else v
    # eval-mode forward (running statistics) on the post-step buffers
    m.eval()
    with torch.no_grad():
        out_np["eval_log_probs"] = m(images.to(dtype)).numpy()
    return out_np


SEED_CASE, SEED_LIST = "resnest26d_224", (200, 1200, 2200, 3200, 4200)       # 200 = the seed of model_resnest26d_224.npz
SEED_THREADS = (8, 16, 32)


HEAD_PREFIXES = ("slot.", "conv1x1.")         # tensors whose gradient no backbone ReLU / max-pool choice can move (see below)


def run_reference_forward_seeds():
    """Train-mode FORWARD AND BACKWARD of the reference SlotModel at the BASELINE input size for five parameter / input seeds:
    fp64 once, and plain fp32 PyTorch at 8 / 16 / 32 CPU threads -- the summation order of its convolutions depends on the
    thread count, and so does the distance of its log-probabilities from fp64 (seed 200: 4.0e-5 / 1.06e-4 / 6.9e-5): the
    yardstick the HIP path's rounding noise is held to is a DISTRIBUTION, not one draw
    (tests/test_model_gpu.py::test_rounding_noise_over_five_seeds, ::test_gradient_noise_over_five_seeds).

    Gradients (round 6): for every parameter tensor the (sum, abs-sum, first 16 entries) digest of the fp64 gradient and of
    the fp32 gradient at each thread count, and max |fp32 - fp64| per tensor and thread count.  For the HEAD tensors
    (`slot.*`, `conv1x1.*`) the full fp64 gradient is kept (stored as float32: its 6e-8 relative rounding is far below the
    fp32 noise being measured): in the backward they are produced BEFORE any backbone ReLU / max-pool is crossed, so no sign
    flip of a ~0 pre-activation can move them -- what moves them is the rounding noise of the forward features, which is what
    the distribution test measures.  Backbone gradients depend on those flips in either implementation; the tests pin them
    with the live oracle under the HIP path's own sign pattern instead."""
    arch, C, spc, L, ls, power, B, H, in_chans, mnist = MODEL_CASES[SEED_CASE]
    out = {"seeds": np.array(SEED_LIST), "threads": np.array(SEED_THREADS)}

    def run(seed, dtype):
        spec, P, images, labels = model_inputs(SEED_CASE, seed)
        args = R.make_args(model=arch, num_classes=C, slots_per_class=spc, channel=O.ARCHS[arch]["channel"], to_k_layer=L,
                           power=power, loss_status=ls, lambda_value=LAMBDA, dataset="ImageNet")
        m = R.build_reference_slot_model(args, feature_size=-(-H // 32))
        m.load_state_dict(P)
        m = m.to(dtype).train()
        store = []
        with R.capture_python_sigmoid(store):
            o, losses = m(images.to(dtype), labels)
        losses[0].backward()
        grads = {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}
        return o.detach().numpy(), store[-1].detach().numpy(), grads
    keep = torch.get_num_threads()
    torch.set_num_threads(16)
    r64 = [run(seed, torch.float64) for seed in SEED_LIST]
    out["f64_log_probs"] = np.stack([r[0] for r in r64])
    out["f64_attn"] = np.stack([r[1] for r in r64])
    keys = list(r64[0][2])
    head = [k for k in keys if k.startswith(HEAD_PREFIXES)]
    out["grad_keys"] = np.array(keys)
    out["head_keys"] = np.array(head)
    out["head_sizes"] = np.array([r64[0][2][k].numel() for k in head])
    out["f64_grad_digest"] = np.stack([np.stack([grad_digest(r[2][k]) for k in keys]) for r in r64])       # [seed][tensor][18]
    out["f64_grad_absmax"] = np.array([[float(r[2][k].abs().max()) for k in keys] for r in r64])            # [seed][tensor]
    out["f64_head_grads"] = np.stack([np.concatenate([r[2][k].flatten().numpy() for k in head]).astype(np.float32)
                                      for r in r64])                                                       # [seed][sum of sizes]
    rows, digs, devs = [], [], []
    for t in SEED_THREADS:
        torch.set_num_threads(t)
        r32 = [run(seed, torch.float32) for seed in SEED_LIST]
        rows.append(np.stack([r[0] for r in r32]))
        digs.append(np.stack([np.stack([grad_digest(r[2][k]) for k in keys]) for r in r32]))
        devs.append(np.array([[float((r[2][k].double() - q[2][k]).abs().max()) for k in keys] for r, q in zip(r32, r64)]))
    torch.set_num_threads(keep)
    out["f32_log_probs"] = np.stack(rows, axis=1)                # [seed][thread count][B][C]
    out["f32_grad_digest"] = np.stack(digs, axis=1)              # [seed][thread count][tensor][18]
    out["f32_grad_maxdev"] = np.stack(devs, axis=1)              # [seed][thread count][tensor]: max |fp32 - fp64|
    return out


def run_reference_fc(dtype):
    """FC baseline (use_slot=False, slot_model.py:75-77,123-125): resnet18 MNIST stem, batch 4, 64x64."""
    arch, C, B, H = "resnet18", 10, 4, 64
    args = R.make_args(model=arch, num_classes=C, channel=512, dataset="MNIST", use_slot=False)
    m = R.build_reference_slot_model(args)
    spec = O.state_dict_spec(arch, C, 1, 1, in_chans=1, mnist_stem=True, use_slot=False)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    m.load_state_dict(O.synth_state(spec, 400))
    m = m.to(dtype).train()
    images, labels = O.synth_batch(B, 1, H, C, 401)
    out, losses = m(images.to(dtype), labels)
    losses[0].backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    return dict(log_probs=out.detach().numpy(), loss=losses[0].detach().numpy(),
                grad_keys=np.array(list(grads)), grad_digest=np.stack([grad_digest(g) for g in grads.values()]))


def run_reference_engine():
    """engine.train_one_epoch + evaluate of the reference on a 2-batch synthetic loader (config 1, tiny)."""
    R.install_shims()
    import engine as ref_engine                             # noqa: reference
    from tools.calculate_tool import MetricLog              # noqa: reference
    arch, C, spc, L = "resnet18", 10, 1, 1
    args = R.make_args(model=arch, num_classes=C, slots_per_class=spc, channel=512, to_k_layer=L, power=1,
                       loss_status=1, lambda_value=LAMBDA, dataset="MNIST")
    m = R.build_reference_slot_model(args, feature_size=ENGINE_SIZE // 32)
    spec = O.state_dict_spec(arch, C, spc, L, in_chans=1, mnist_stem=True)
    m.load_state_dict(O.synth_state(spec, 300))
    loader = []
    for i in range(2):
        img, lab = O.synth_batch(ENGINE_BATCH, 1, ENGINE_SIZE, C, 310 + i)
        loader.append({"image": img.double(), "label": lab})
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4)
    log = MetricLog()
    ref_engine.train_one_epoch(m, loader, opt, torch.device("cpu"), log.record, 0)
    ref_engine.evaluate(m, loader, torch.device("cpu"), log.record, 0)
    sd = m.state_dict()
    keys = [k for k in sd if sd[k].dtype.is_floating_point]
    return dict(
        record_train=np.array([log.record["train"][k][0] for k in ("loss", "acc", "log_loss", "att_loss")]),
        record_val=np.array([log.record["val"][k][0] for k in ("loss", "acc", "log_loss", "att_loss")]),
        param_keys=np.array(keys), param_digest=np.stack([grad_digest(sd[k]) for k in keys]))


def main(heads_only=False):
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(GEN_THREADS)
    for case in HEAD_CASES:
        f32 = run_reference_head(case, torch.float32)
        f64 = run_reference_head(case, torch.float64)
        blob = {"f32_" + k: v for k, v in f32.items()}
        blob.update({"f64_" + k: v for k, v in f64.items() if k in ("logits", "log_probs", "loss", "nll", "area",
                                                                     "attn")})
        np.savez_compressed(os.path.join(OUT, f"head_{case}.npz"), **blob)
        print("head", case, "logit fp32-vs-fp64 gap", np.abs(f32["logits"] - f64["logits"]).max())
    if heads_only:
        return
    for case in MODEL_CASES:
        f32 = run_reference_model(case, torch.float32)
        f64 = run_reference_model(case, torch.float64)
        blob = {"f32_" + k: v for k, v in f32.items()}
        blob.update({"f64_" + k: v for k, v in f64.items() if k in ("log_probs", "loss", "nll", "area", "attn",
                                                                     "grad_digest", "eval_log_probs")})
        np.savez_compressed(os.path.join(OUT, f"model_{case}.npz"), **blob)
        print("model", case, "log_probs fp32-vs-fp64 gap", np.abs(f32["log_probs"] - f64["log_probs"]).max())
    seeds = run_reference_forward_seeds()
    np.savez_compressed(os.path.join(OUT, "model_%s_seeds.npz" % SEED_CASE), **seeds)
    print("seeds x threads: fp32-vs-fp64 gap", np.abs(seeds["f32_log_probs"] - seeds["f64_log_probs"][:, None]).max((2, 3)))
    fc32, fc64 = run_reference_fc(torch.float32), run_reference_fc(torch.float64)
    blob = {"f32_" + k: v for k, v in fc32.items()}
    blob.update({"f64_" + k: v for k, v in fc64.items()})
    np.savez_compressed(os.path.join(OUT, "model_fc_resnet18_mnist_64.npz"), **blob)
    np.savez_compressed(os.path.join(OUT, "engine_mnist.npz"), **run_reference_engine())
    print("done ->", OUT)


if __name__ == "__main__":
    if "--seeds-only" in sys.argv:           # (only the five-seed forward fixture; the others are left as committed)
        torch.manual_seed(0)
        torch.set_num_threads(16)
        blob = run_reference_forward_seeds()
        np.savez_compressed(os.path.join(OUT, "model_%s_seeds.npz" % SEED_CASE), **blob)
        print("seeds x threads: fp32-vs-fp64 gap\n", np.abs(blob["f32_log_probs"] - blob["f64_log_probs"][:, None]).max((2, 3)))
    else:
        main(heads_only="--heads-only" in sys.argv)
