"""Cost of an input-gradient (saliency) batch next to a training step, and the stem input-gradient kernel alone.

    python tools_dev/input_grad_bench.py [resnest26d resnet18] [--batch 70] [--seconds 1.0] [--repeats 3] [--iters N]

Per model (224^2, fp32, 10 classes): ms of one saliency batch -- eval mode, nothing trainable, one class: forward + backward to
the image (tools/attribution.input_gradients) -- of one training step's forward + backward at the same shape, and of the stem
input-gradient kernel (kernels.stem_dgrad) on a gradient of the stem's output shape, with its byte floor
(dy bytes + dx bytes) / --hbm-tbs.  Device events around windows of at least --seconds each.  --iters N: instead, N saliency
batches and nothing else (the body of a `rocprofv3 --kernel-trace --stats` run)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import torch_oracle as O                     # noqa: E402
from scouter_amd import kernels as K                     # noqa: E402
from scouter_amd.sloter.slot_model import SlotModel      # noqa: E402
from scouter_amd.tools.attribution import input_gradients   # noqa: E402

STEMS = {"resnest26d": (3, 32, 3, 2, 1), "resnet18": (3, 64, 7, 2, 3)}      # Cin, Cout, k, stride, pad


def make(model, batch):
    args = argparse.Namespace(model=model, pre_trained=False, num_classes=10, dataset="ImageNet", use_slot=True, use_pre=False,
                              grad=False, channel=O.ARCHS[model]["channel"], slots_per_class=1, hidden_dim=64, freeze_layers=0,
                              vis=False, vis_id=0, loss_status=1, power=2, to_k_layer=3, lambda_value="1", precision="fp32")
    m = SlotModel(args)
    m.load_state_dict(O.synth_state(O.state_dict_spec(model, 10, 1, 3), 300))
    images, labels = O.synth_batch(batch, 3, 224, 10, 301)
    return m.cuda(), images.cuda(), labels.cuda()


def window(fn, seconds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 2
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1000.0 * seconds:
            return ms / n
        n = max(n * 2, int(n * 1100.0 * seconds / max(ms, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floor, TB/s")
    a = ap.parse_args()
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, labels = make(model, a.batch)

        def train_step():
            out, losses = m(x, labels)
            losses[0].backward(m.loss_seed(losses[0]))

        def saliency():
            return input_gradients(m, x, classes=[3])

        if a.iters:
            m.requires_grad_(False)
            for _ in range(a.iters):
                saliency()
            torch.cuda.synchronize()
            continue
        m.train()
        for _ in range(3):
            train_step()
        t_train = [window(train_step, a.seconds) for _ in range(a.repeats)]
        m.requires_grad_(False)
        for _ in range(3):
            saliency()
        t_sal = [window(saliency, a.seconds) for _ in range(a.repeats)]
        cin, cout, k, s, p = STEMS[model]
        ho = K.conv_out(224, k, s, p)
        dy = torch.randn(a.batch, ho, ho, cout, device="cuda")
        w = torch.randn(k, k, cin, cout, device="cuda")
        fn = lambda: K.stem_dgrad(dy, w, (a.batch, cin, 224, 224), k, s, p)
        fn()
        t_k = [window(fn, a.seconds / 4) * 1000.0 for _ in range(a.repeats)]
        nbytes = 4.0 * (dy.numel() + a.batch * cin * 224 * 224)
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        fmt = lambda v: " ".join("%.3f" % t for t in v)
        print("%s batch %d 224^2: training step (fwd + bwd) ms %s | saliency batch (eval fwd + bwd to the image) ms %s"
              % (model, a.batch, fmt(t_train), fmt(t_sal)))
        print("%s stem_dgrad %d -> %d %dx%d/%d: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
              % (model, cin, cout, k, k, s, " ".join("%.1f" % t for t in t_k), nbytes / 1e6, floor, a.hbm_tbs, min(t_k) / floor))


if __name__ == "__main__":
    main()
