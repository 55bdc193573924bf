"""Cost of RISE next to the bare forward it is made of, and its three kernels alone.

    python tools_dev/rise_bench.py [--model resnest26d] [--masks 4000] [--batch 250] [--repeats 3] [--out FILE] [--iters N]

224^2, fp32, 10 classes, one image, with the inference fold off and on: masked images per second through
tools/attribution.rise (every chunk: kernels.rise_mask_images, the model, kernels.rise_accumulate) and images per second of a
bare `model(x)` under no_grad at the same batch, device events around whole calls, the two alternating; their ratio is what the
mask writer, the accumulation and the host gaps between chunks cost.  Then the three kernels at the chunk's shapes with their
byte floors / --hbm-tbs.  --iters N: instead, N chunks (mask writer, forward, accumulation) and nothing else -- the body of a
`rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                 # noqa: E402
from scouter_amd.tools.attribution import rise, rise_masks          # noqa: E402
from tools_dev.input_grad_bench import make, window                 # noqa: E402


def events_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--masks", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, x, _ = make(a.model, a.batch)
    m.requires_grad_(False)
    m.eval()
    image = x[:1]
    masks = rise_masks(a.masks, (224, 224), s=7, p=0.5, seed=0, device="cuda")
    cols = torch.arange(10, dtype=torch.int32, device="cuda")
    g, sh = masks.grids[:a.batch], masks.shifts[:a.batch]
    buf = torch.empty((g.shape[0], 3, 224, 224), device="cuda")
    acc = torch.zeros((10, 224, 224), device="cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def chunk():
        with torch.no_grad():
            logp = m(K.rise_mask_images(image[0], g, sh, buf, 7, check_shifts=False))
        K.rise_accumulate(logp, cols, g, sh, acc, 7, 1.0 / (a.masks * 0.5), check_shifts=False)

    if a.iters:
        m.set_inference_fold(True)
        for _ in range(a.iters):
            chunk()
        torch.cuda.synchronize()
        return

    def bare():
        with torch.no_grad():
            for _ in range(-(-a.masks // a.batch)):
                m(x)

    for fold in (False, True):
        m.set_inference_fold(fold)
        for _ in range(2):                                   # every shape on this path warmed up
            rise(m, image, batch=a.batch, masks=masks)
            bare()
        t_rise, t_bare = [], []
        for _ in range(a.repeats):
            t_rise.append(events_ms(lambda: rise(m, image, batch=a.batch, masks=masks)))
            t_bare.append(events_ms(bare))
        n_bare = -(-a.masks // a.batch) * a.batch
        r, b = a.masks / min(t_rise) * 1e3, n_bare / min(t_bare) * 1e3
        say("%s 224^2, 10 classes, %d masks in chunks of %d, %s: rise ms %s -> %.0f masked images/s | bare model(x) at batch %d, "
            "%d forwards ms %s -> %.0f images/s | ratio %.3f"
            % (a.model, a.masks, a.batch, "folded" if fold else "unfolded", " ".join("%.2f" % t for t in t_rise), r, a.batch,
               -(-a.masks // a.batch), " ".join("%.2f" % t for t in t_bare), b, r / b))

    n = g.shape[0]
    logp = torch.log_softmax(torch.randn(n, 10, device="cuda"), dim=1)
    big = torch.randn(10, 224, 224, device="cuda")
    for name, fn, nbytes in (
            ("rise_mask_images [%d, 3, 224, 224]" % n, lambda: K.rise_mask_images(image[0], g, sh, buf, 7, check_shifts=False),
             4.0 * (buf.numel() + image[0].numel())),
            ("rise_accumulate %d masks onto [10, 224, 224]" % n,
             lambda: K.rise_accumulate(logp, cols, g, sh, acc, 7, 1e-4, check_shifts=False), 8.0 * acc.numel()),
            ("heat_maps [10, 224, 224]", lambda: K.heat_maps(big), 9.0 * big.numel())):
        fn()
        t = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
            % (name, " ".join("%.1f" % v for v in t), nbytes / 1e6, floor, a.hbm_tbs, min(t) / floor))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
