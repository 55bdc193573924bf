"""Cost of the insertion / deletion scores next to the bare forward they are made of, and their kernels alone.

    python tools_dev/causal_bench.py [--model resnest26d] [--maps 10] [--step 224] [--batch 250] [--repeats 3] [--out FILE] [--iters N]

224^2, fp32, 10 classes, one image with --maps saliency maps, with the inference fold off and on: edited images per second through
tools/attribution.causal_metrics (per image: kernels.saliency_ranks and separable_filter; every chunk: kernels.causal_step_images,
the model, kernels.causal_curve; kernels.causal_auc at the end) and images per second of a bare `model(x)` under no_grad at the
same batch for the same number of images (the last forward short, as in the call), device events around whole calls, the two
alternating; their ratio is what everything around the forwards costs.  Then causal_step_images next to rise_mask_images at the
chunk's shape with their byte floors / --hbm-tbs, and the per-image kernels (ranks, blur, resize of 7 x 7 maps) with their share
of the whole call.  --iters N: instead, N chunks (step images, forward, curve) and nothing else -- the body of a
`rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                             # noqa: E402
from scouter_amd.tools.attribution import causal_metrics, gaussian_taps, rise_masks      # noqa: E402
from tools_dev.input_grad_bench import make, window                             # noqa: E402
from tools_dev.rise_bench import events_ms                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--maps", type=int, default=10)
    ap.add_argument("--step", type=int, default=224)
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
    H = W = 224
    maps = torch.rand((1, a.maps, H, W), generator=torch.Generator().manual_seed(5)).cuda()
    n_points = -(-(H * W) // a.step) + 1
    total = 2 * a.maps * n_points
    sizes = [min(a.batch, total - f) for f in range(0, total, a.batch)]
    cols = torch.arange(a.maps, dtype=torch.int32, device="cuda")
    taps = gaussian_taps(11, 5.0).cuda()
    n = min(a.batch, total)
    buf = torch.empty((n, 3, H, W), device="cuda")
    blurred = K.separable_filter(image[0], taps)
    ranks = K.saliency_ranks(maps[0].view(a.maps, H * W))
    curves = torch.empty((a.maps, 2, n_points), device="cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def chunk():
        with torch.no_grad():
            logp = m(K.causal_step_images(image[0], blurred, ranks, buf, n_points - n // 2, n_points, a.step))
        K.causal_curve(logp, cols, curves, n_points - n // 2, n_points)

    if a.iters:
        m.set_inference_fold(True)
        for _ in range(a.iters):
            chunk()
        torch.cuda.synchronize()
        return

    def call():
        return causal_metrics(m, image, maps, step=a.step, batch=a.batch)

    def bare():
        with torch.no_grad():
            for s in sizes:
                m(x[:s])

    best_call = {}
    for fold in (False, True):
        m.set_inference_fold(fold)
        for _ in range(2):                                   # every shape on this path warmed up
            call()
            bare()
        t_call, t_bare = [], []
        for _ in range(a.repeats):
            t_call.append(events_ms(call))
            t_bare.append(events_ms(bare))
        best_call[fold] = min(t_call)
        r, b = total / min(t_call) * 1e3, total / min(t_bare) * 1e3
        say("%s 224^2, 10 classes, %d maps, step %d (%d points x 2 x %d = %d edited images) in chunks of %d, %s: causal_metrics ms %s "
            "-> %.0f edited images/s | bare model(x) at batch %d, %d forwards (the last of %d) ms %s -> %.0f images/s | ratio %.3f"
            % (a.model, a.maps, a.step, n_points, a.maps, total, a.batch, "folded" if fold else "unfolded",
               " ".join("%.2f" % t for t in t_call), r, a.batch, len(sizes), sizes[-1], " ".join("%.2f" % t for t in t_bare), b,
               r / b))

    masks = rise_masks(n, (H, W), s=7, p=0.5, seed=0, device="cuda")
    for name, fn, nbytes in (
            ("causal_step_images [%d, 3, 224, 224]" % n,
             lambda: K.causal_step_images(image[0], blurred, ranks, buf, n_points - n // 2, n_points, a.step),
             4.0 * (buf.numel() + image[0].numel())),
            ("rise_mask_images [%d, 3, 224, 224]" % n,
             lambda: K.rise_mask_images(image[0], masks.grids, masks.shifts, buf, 7, check_shifts=False),
             4.0 * (buf.numel() + image[0].numel()))):
        fn()
        t = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
            % (name, " ".join("%.1f" % v for v in t), nbytes / 1e6, floor, a.hbm_tbs, min(t) / floor))
    coarse = torch.rand((a.maps, 7, 7), generator=torch.Generator().manual_seed(6)).cuda()
    flat = maps[0].view(a.maps, H * W)
    for name, fn in (("saliency_ranks [%d, 224 x 224]" % a.maps, lambda: K.saliency_ranks(flat, out=ranks)),
                     ("separable_filter [3, 224, 224], 11 taps", lambda: K.separable_filter(image[0], taps, out=blurred)),
                     ("resize_bilinear [%d, 7, 7] -> 224 x 224" % a.maps, lambda: K.resize_bilinear(coarse, H, W))):
        fn()
        t = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        say("%s: us %s | once per image: %.4f %% of the unfolded call, %.4f %% of the folded one"
            % (name, " ".join("%.1f" % v for v in t), min(t) / best_call[False] * 0.1, min(t) / best_call[True] * 0.1))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
