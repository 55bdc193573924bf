"""Cost of occlusion maps and Ablation-CAM next to the model passes they are made of, and the share their kernels take.

    python tools_dev/ablation_bench.py [--model resnest26d] [--window 16] [--stride 8] [--batch 250] [--head-batch 256] [--repeats 3]
                                       [--out FILE]

224^2, fp32, 10 classes, one image, the inference fold on.  tools/attribution.occlusion (every chunk: kernels.occlude_images, the
model, kernels.output_deltas; then kernels.occlusion_finish) against the same forwards alone -- the same row counts, no_grad, the
buffer left as it is; tools/attribution.ablationcam (one feature pass; every chunk: kernels.ablate_channels, SlotModel.head_pass,
kernels.output_deltas; then kernels.ablation_contract) against the feature pass and the same head passes alone.  Device events
around whole calls, the pairs alternating.  The share of a call spent outside the model is 1 - passes / call.  Then the kernels
alone at the shapes of that run, each times the launches an image needs."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                                       # noqa: E402
from scouter_amd.tools import attribution as A                                             # noqa: E402
from tools_dev.input_grad_bench import make, window                                        # noqa: E402
from tools_dev.rise_bench import events_ms                                                 # noqa: E402


def chunk_rows(total, batch):
    """the row counts (the clean row included) of the chunks a stream of `total` changed rows is cut into"""
    return [1 + min(batch - 1, total - first) for first in range(0, total, batch - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--head-batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, x, _ = make(a.model, max(a.batch, 2))
    m.requires_grad_(False)
    m.eval()
    m.set_inference_fold(True)
    image = x[:1].contiguous()
    n_classes = 10
    ny, nx = A.occlusion_windows((224, 224), a.window, a.stride)
    N = ny * nx
    feat = m.feature_pass(image).features.detach().contiguous()
    _, h, w, C = feat.shape
    occ_rows, abl_rows = chunk_rows(N, a.batch), chunk_rows(C, a.head_batch)
    buf = x[:max(occ_rows)].contiguous()
    fbuf = feat.repeat(max(abl_rows), 1, 1, 1).contiguous()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def forwards():
        with torch.no_grad():
            for rows in occ_rows:
                m(buf[:rows])

    def head_passes():
        m.feature_pass(image)
        for rows in abl_rows:
            m.head_pass(fbuf[:rows])

    methods = (("occlusion", lambda: A.occlusion(m, image, window=a.window, stride=a.stride, batch=a.batch)),
               ("forwards", forwards),
               ("ablationcam", lambda: A.ablationcam(m, image, batch=a.head_batch)),
               ("head passes", head_passes))
    for _ in range(2):                                           # every shape on these paths warmed up
        for _, fn in methods:
            fn()
    times = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            times[name].append(events_ms(fn))
    best = {name: min(t) for name, t in times.items()}
    what = {"occlusion": "occlusion, window %d, stride %d: %d windows in chunks of %d rows" % (a.window, a.stride, N, a.batch),
            "forwards": "the same %d forwards alone (rows %s)" % (len(occ_rows), " ".join(str(r) for r in occ_rows)),
            "ablationcam": "ablationcam, %d channels at %d x %d in chunks of %d rows" % (C, h, w, a.head_batch),
            "head passes": "one feature pass and the same %d head passes alone (rows %s)"
                           % (len(abl_rows), " ".join(str(r) for r in abl_rows))}
    for name, _ in methods:
        say("%s, %s 224^2, 10 classes, folded: ms per image %s -> best %.2f"
            % (what[name], a.model, " ".join("%.2f" % t for t in times[name]), best[name]))
    say("occlusion: %.2f %% of the call is spent outside the model (best of %d each)"
        % (100.0 * (1.0 - best["forwards"] / best["occlusion"]), a.repeats))
    say("ablationcam: %.2f %% of the call is spent outside the model (best of %d each)"
        % (100.0 * (1.0 - best["head passes"] / best["ablationcam"]), a.repeats))

    # ---- the kernels at the shapes of one image, times the launches an image needs
    cols = torch.arange(n_classes, dtype=torch.int32, device="cuda")
    rows, frows = max(occ_rows), max(abl_rows)
    logp = torch.log_softmax(torch.randn(max(rows, frows), n_classes, device="cuda"), dim=1)
    deltas = torch.zeros((n_classes, N), dtype=torch.float64, device="cuda")
    fdeltas = torch.zeros((n_classes, C), dtype=torch.float64, device="cuda")
    smap = torch.empty((n_classes, 224, 224), device="cuda")
    cam = torch.empty((n_classes, h, w), device="cuda")
    obuf = torch.empty((rows, 3, 224, 224), device="cuda")
    for method, kernels in (("occlusion", (
            ("occlude_images [%d, 3, 224, 224]" % rows, lambda: K.occlude_images(image[0], obuf, 0, a.window, a.stride), len(occ_rows)),
            ("output_deltas %d rows, K %d" % (rows, n_classes), lambda: K.output_deltas(logp[:rows], cols, deltas, 0, "prob"),
             len(occ_rows)),
            ("occlusion_finish [%d, 224, 224], %d windows" % (n_classes, N),
             lambda: K.occlusion_finish(deltas, smap, a.window, a.stride), 1))),
                            ("ablationcam", (
            ("ablate_channels [%d, %d, %d, %d]" % (frows, h, w, C), lambda: K.ablate_channels(feat[0], fbuf[:frows], 0), len(abl_rows)),
            ("output_deltas %d rows, K %d" % (frows, n_classes), lambda: K.output_deltas(logp[:frows], cols, fdeltas, 0, "prob"),
             len(abl_rows)),
            ("ablation_contract K %d, %d positions, %d channels" % (n_classes, h * w, C),
             lambda: K.ablation_contract(fdeltas, logp[0], cols, feat[0], cam), 1)))):
        total_us = 0.0
        for name, fn, launches in kernels:
            fn()
            t = [window(fn, 0.1) * 1e3 for _ in range(a.repeats)]
            total_us += min(t) * launches
            say("%s: us %s | x %d launches per image = %.1f us" % (name, " ".join("%.1f" % v for v in t), launches, min(t) * launches))
        say("the kernels of %s: %.3f ms per image = %.2f %% of its %.2f ms"
            % (method, total_us / 1e3, 0.1 * total_us / best[method], best[method]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
