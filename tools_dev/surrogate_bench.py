"""Cost of LIME and KernelSHAP next to RISE at the same number of forwards, and the share their six kernels take.

    python tools_dev/surrogate_bench.py [--model resnest26d] [--samples 1000] [--batch 250] [--segments 8] [--repeats 3] [--out FILE]

224^2, fp32, 10 classes, one image, the inference fold on: milliseconds per image of tools/attribution.lime and kernelshap
(superpixels, then every chunk: kernels.segment_images, the model, kernels.surrogate_accumulate; then the fit and the painting)
and of tools/attribution.rise with as many masks at the same batch, device events around whole calls, the three alternating.
Then the six kernels of csrc/surrogate.hip at the shapes of that run, each times the launches an image needs, against the
method's whole time: the share that is not forwards."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                                       # noqa: E402
from scouter_amd.tools import attribution as A                                             # noqa: E402
from tools_dev.input_grad_bench import make, window                                        # noqa: E402
from tools_dev.rise_bench import events_ms                                                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--slic-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, x, _ = make(a.model, a.batch)
    m.requires_grad_(False)
    m.eval()
    m.set_inference_fold(True)
    image = x[:1].contiguous()
    N, g, d, n_classes = a.samples, a.segments, a.segments * a.segments, 10
    masks = A.rise_masks(N, (224, 224), s=7, p=0.5, seed=0, device="cuda")
    kw = dict(n_samples=N, segments=g, batch=a.batch, slic_iters=a.slic_iters)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    methods = (("lime", lambda: A.lime(m, image, **kw)), ("kernelshap", lambda: A.kernelshap(m, image, **kw)),
               ("rise", lambda: A.rise(m, image, batch=a.batch, masks=masks)))
    for _ in range(2):                                           # every shape on these paths warmed up
        for _, fn in methods:
            fn()
    times = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            times[name].append(events_ms(fn))
    for name, _ in methods:
        say("%s, %s 224^2, 10 classes, folded, %d rows in chunks of %d%s: ms per image %s -> best %.2f"
            % (name, a.model, N, a.batch, "" if name == "rise" else ", %d x %d superpixels, %d SLIC iterations" % (g, g, a.slic_iters),
               " ".join("%.2f" % t for t in times[name]), min(times[name])))
    say("lime / rise = %.3f, kernelshap / rise = %.3f (best of %d each)"
        % (min(times["lime"]) / min(times["rise"]), min(times["kernelshap"]) / min(times["rise"]), a.repeats))

    # ---- the six kernels at the shapes of one image, times the launches an image needs
    n = min(a.batch, N)
    chunks = -(-N // a.batch)
    seg = A.superpixels(image, g, iters=a.slic_iters)
    centres = torch.zeros((1, d, 5), device="cuda")
    means = torch.empty((1, d, 3), device="cuda")
    labels = seg.labels.clone()
    z = A.lime_samples(N, d, 0).cuda()[:n].contiguous()
    buf = torch.empty((n, 3, 224, 224), device="cuda")
    logp = torch.log_softmax(torch.randn(n, n_classes, device="cuda"), dim=1)
    cols = torch.arange(n_classes, dtype=torch.int32, device="cuda")
    S = torch.zeros((1, d + 1, d + 1), dtype=torch.float64, device="cuda")
    T = torch.zeros((1, d + 1, n_classes), dtype=torch.float64, device="cuda")
    yref = torch.zeros((1, 2, n_classes), dtype=torch.float64, device="cuda")
    zs = A.kernelshap_samples(N, d, 0).cuda()
    for n0 in range(0, N, n):                                    # moments a solve can factor
        K.surrogate_accumulate(logp[:zs[n0:n0 + n].shape[0]], cols, zs[n0:n0 + n], S[0], T[0], yref[0], n0, K.SURROGATE_SHAP)
    coef, _ = K.surrogate_solve(S, T, yref, K.SURROGATE_SHAP, 0.0)
    lam = (1.0 / (224 * 224 / float(d)) ** 0.5) ** 2
    scratch_S, scratch_T = torch.zeros_like(S[0]), torch.zeros_like(T[0])
    total_us = 0.0
    for name, fn, launches in (
            ("slic_update [1, 3, 224, 224], %d segments" % d, lambda: K.slic_update(image, labels, centres, means, g, g), a.slic_iters + 1),
            ("slic_assign [1, 3, 224, 224], %d segments" % d, lambda: K.slic_assign(image, centres, labels, g, g, lam), a.slic_iters),
            ("segment_images [%d, 3, 224, 224], mean colours" % n, lambda: K.segment_images(image[0], seg.labels[0], z, buf, seg.means[0]),
             chunks),
            ("surrogate_accumulate %d rows, d %d, K %d" % (n, d, n_classes),
             lambda: K.surrogate_accumulate(logp, cols, z, scratch_S, scratch_T, None, 0, K.SURROGATE_LIME), chunks),
            ("surrogate_solve d %d, K %d (KernelSHAP)" % (d, n_classes), lambda: K.surrogate_solve(S, T, yref, K.SURROGATE_SHAP, 0.0), 1),
            ("segment_paint [1, %d, 224, 224]" % n_classes, lambda: K.segment_paint(coef, seg.labels), 1)):
        fn()
        t = [window(fn, 0.1) * 1e3 for _ in range(a.repeats)]
        total_us += min(t) * launches
        say("%s: us %s | x %d launches per image = %.1f us" % (name, " ".join("%.1f" % v for v in t), launches, min(t) * launches))
    say("the six kernels: %.3f ms per image = %.2f %% of lime's %.2f ms, %.2f %% of kernelshap's %.2f ms"
        % (total_us / 1e3, 0.1 * total_us / min(times["lime"]), min(times["lime"]), 0.1 * total_us / min(times["kernelshap"]),
           min(times["kernelshap"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
