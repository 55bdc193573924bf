"""Cost of the Grad-CAM++ kernels and of per-class Grad-CAM++ maps next to Grad-CAM on the same model.

    python tools_dev/campp_bench.py [--model resnest26d] [--seconds 0.5] [--repeats 3] [--samples 4]

The three kernels of csrc/gradcampp.hip at 7 x 7 x 2048 and 9 x 9 x 2048 with B = 1 and 10, beside kernels.gradcam on the same
operands: us per call (device events around windows of back-to-back calls of at least --seconds) and the bytes each call
loads and stores (feat and the gradient operand are loaded twice by the class-map kernels; whether the second load comes from
L2 is not measured here).  Then tools/attribution.gradcampp and gradcam for all 10 classes of ONE image (224^2, fp32, nothing
trainable, unfolded): one backbone forward, ten head backwards, ten kernel calls each; and smooth_gradcampp with its defaults
(--samples noisy copies in one chunk)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                                    # noqa: E402
from scouter_amd.tools.attribution import gradcam, gradcampp, smooth_gradcampp          # noqa: E402
from tools_dev.input_grad_bench import make, window                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4)
    a = ap.parse_args()
    fmt = lambda v, f="%.1f": " ".join(f % t for t in v)
    C, n = 2048, a.samples
    for h in (7, 9):
        for B in (1, 10):
            gen = torch.Generator().manual_seed(B * h)
            feat = (0.5 * torch.randn((B, h, h, C), generator=gen).abs()).cuda()
            grads = (1.0 + 0.5 * torch.randn((n, B, h, h, C), generator=gen)).cuda()
            cam = torch.empty((B, 10, h, h), device="cuda")
            acc2 = torch.zeros((B, h, h, C), dtype=torch.float64, device="cuda")
            acc3 = torch.zeros_like(acc2)
            el = float(feat.numel())
            calls = (("gradcam", lambda: K.gradcam(feat, grads[0], cam[:, 3]), 8.0 * el),
                     ("gradcampp", lambda: K.gradcampp(feat, grads[0], cam[:, 3]), 16.0 * el),
                     ("grad_powers_accumulate n = %d" % n, lambda: K.grad_powers_accumulate(grads, acc2, acc3),
                      (4.0 * n + 32.0) * el),
                     ("gradcampp_smooth", lambda: K.gradcampp_smooth(feat, acc2, acc3, grads[n - 1], cam[:, 3], n), 28.0 * el))
            for name, fn, nbytes in calls:
                fn()
                t = [window(fn, a.seconds / 4) * 1e3 for _ in range(a.repeats)]
                print("%s [%d, %d, %d, %d]: us %s | %.2f MB loaded and stored per call" % (name, B, h, h, C, fmt(t), nbytes / 1e6))
    m, x, _ = make(a.model, 1)
    m.requires_grad_(False)
    m.eval()
    tools = (("gradcam", lambda: gradcam(m, x)), ("gradcampp", lambda: gradcampp(m, x)),
             ("smooth_gradcampp n_samples %d batch %d" % (n, n), lambda: smooth_gradcampp(m, x, n_samples=n, batch=n)))
    for name, fn in tools:
        for _ in range(3):
            fn()
    for _ in range(a.repeats):                                         # alternating
        for name, fn in tools:
            print("%s one image 224^2, 10 classes, %s: ms %.3f (device events)" % (a.model, name, window(fn, a.seconds)))


if __name__ == "__main__":
    main()
