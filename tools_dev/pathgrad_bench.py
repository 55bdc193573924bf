"""Cost of Integrated Gradients and SmoothGrad next to the bare forward + backward batches they are made of, and the five
kernels of csrc/pathgrad.hip alone.

    python tools_dev/pathgrad_bench.py [models ...] [--steps 50] [--batch 50] [--repeats 3] [--out FILE]

Per model (default resnest26d and resnet18; 224^2, fp32, 10 classes, one image, one class, parameters frozen): ms of one
tools/attribution.integrated_gradients call (--steps Gauss-Legendre steps in chunks of --batch: kernels.path_images, the
eval-mode forward and the backward to the image, kernels.grad_accumulate, kernels.attr_finish), ms of one smoothgrad call with as
many samples, and ms of the bare eval forward + backward at the same batch sizes (a leaf that requires grad, one
torch.autograd.grad with a one-hot column), the three alternating, device events around whole calls.  bare / call is what the
batch writers, the float64 sums, the finish and the host gaps between chunks cost.  Then the five kernels alone at the shapes
of such a call, each with its byte floor / --hbm-tbs; grad_accumulate also in its one-element form (a misaligned pointer)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                               # noqa: E402
from scouter_amd.tools.attribution import ig_quadrature, integrated_gradients, smoothgrad    # noqa: E402
from tools_dev.input_grad_bench import make, window                               # noqa: E402
from tools_dev.rise_bench import events_ms                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    N, batch = a.steps, min(a.batch, a.steps)
    sizes = [batch] * (N // batch) + ([N % batch] if N % batch else [])
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, _ = make(model, batch)
        m.requires_grad_(False)
        m.eval()
        image = x[:1]
        seed = torch.zeros((batch, 10), device="cuda")
        seed[:, 0] = 1.0
        leaf = x.detach().clone().requires_grad_(True)

        def bare():
            for n in sizes:
                xb = leaf[:n].detach().requires_grad_(True)
                torch.autograd.grad(m(xb), xb, seed[:n])

        f_ig = lambda: integrated_gradients(m, image, classes=[0], n_steps=N, batch=batch)
        f_sg = lambda: smoothgrad(m, image, classes=[0], n_samples=N, batch=batch)
        for _ in range(2):                                      # every shape on this path warmed up
            f_ig(); f_sg(); bare()
        t_ig, t_sg, t_bare = [], [], []
        for _ in range(a.repeats):
            t_ig.append(events_ms(f_ig))
            t_sg.append(events_ms(f_sg))
            t_bare.append(events_ms(bare))
        fmt = lambda ts: " ".join("%.2f" % t for t in ts)
        say("%s 224^2, one image, one class, %d steps / samples in chunks of %d, parameters frozen: integrated_gradients ms %s | "
            "smoothgrad ms %s | bare eval forward + backward at batch %s, ms %s | bare / integrated_gradients %.3f, bare / "
            "smoothgrad %.3f" % (model, N, batch, fmt(t_ig), fmt(t_sg), " + ".join(str(n) for n in sizes), fmt(t_bare),
                                 min(t_bare) / min(t_ig), min(t_bare) / min(t_sg)))
        del m, leaf

    # ---- the five kernels alone
    shape = (3, 224, 224)
    E = 3 * 224 * 224
    gen = torch.Generator().manual_seed(1)
    img, base = torch.randn(shape, generator=gen).cuda(), torch.randn(shape, generator=gen).cuda()
    alphas = ig_quadrature(N)[0].cuda()
    weights = ig_quadrature(N)[1].cuda()
    buf = torch.empty((batch,) + shape, device="cuda")
    grads = torch.randn((batch,) + shape, device="cuda")
    acc, acc_sq = torch.zeros(shape, dtype=torch.float64, device="cuda"), torch.zeros(shape, dtype=torch.float64, device="cuda")
    out, total = torch.empty(shape, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    attr = torch.randn((10,) + shape, device="cuda")
    cm = torch.empty((10, 224, 224), device="cuda")
    off = torch.empty(batch * E + 1, device="cuda")[1:].view((batch,) + shape)
    off.copy_(grads)
    acc_off = torch.zeros(E + 1, dtype=torch.float64, device="cuda")[1:].view(shape)
    kernels = (
        ("path_images [%d, 3, 224, 224]" % batch, lambda: K.path_images(img, base, alphas, buf, 0), 4.0 * (batch * E + 2 * E)),
        ("noise_images [%d, 3, 224, 224]" % batch, lambda: K.noise_images(img, buf, 1.0, 0, 0), 4.0 * (batch * E + E)),
        ("grad_accumulate %d gradients, weighted" % batch, lambda: K.grad_accumulate(grads, weights, acc, None, 0),
         4.0 * batch * E + 16.0 * E),
        ("grad_accumulate %d gradients, with squares" % batch, lambda: K.grad_accumulate(grads, None, acc, acc_sq, 0),
         4.0 * batch * E + 32.0 * E),
        ("grad_accumulate %d gradients, weighted, one-element form" % batch,
         lambda: K.grad_accumulate(off, weights, acc_off, None, 0), 4.0 * batch * E + 16.0 * E),
        ("attr_finish mode 0 with the total", lambda: K.attr_finish(K.ATTR_IG, acc, image=img, base=base, out=out, total=total),
         20.0 * E),
        ("attr_finish mode 3", lambda: K.attr_finish(K.ATTR_VAR, acc, acc_sq, inv_n=1.0 / N, out=out), 20.0 * E),
        ("channel_mean [10, 3, 224, 224]", lambda: K.channel_mean(attr, out=cm), 4.0 * 10 * 4 * 224 * 224))
    for name, fn, nbytes in kernels:
        fn()
        ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, best / floor = %.2f"
            % (name, " ".join("%.1f" % t for t in ts), nbytes / 1e6, floor, a.hbm_tbs, min(ts) / floor))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
