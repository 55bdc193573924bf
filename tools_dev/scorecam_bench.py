"""Cost of Score-CAM next to the bare forwards it is made of, and its three kernels alone.

    python tools_dev/scorecam_bench.py [--model resnest26d] [--batch 250] [--repeats 3] [--out FILE] [--iters N]

224^2, fp32, 10 classes, one image, with the inference fold off and on: ms of one tools/attribution.scorecam call (one feature
pass, kernels.scorecam_ranges, then per chunk kernels.scorecam_mask_images, the model, kernels.scorecam_accumulate) and ms of
bare `model(x)` forwards under no_grad at the same batch sizes (C // batch at `batch` and one at C % batch), device events around
whole calls, the two alternating; their ratio is what the feature pass, the range kernel, the mask writer, the accumulation
and the host gaps between chunks cost.  Then kernels.scorecam_mask_images next to kernels.rise_mask_images at the same output
shape, alternating, and kernels.scorecam_ranges / scorecam_accumulate once each, with their byte floors / --hbm-tbs.
--iters N: instead, N chunks (mask writer, forward, accumulation) and nothing else -- the body of a
`rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                 # noqa: E402
from scouter_amd.tools.attribution import rise_masks, scorecam      # noqa: E402
from tools_dev.input_grad_bench import make, window                 # noqa: E402
from tools_dev.rise_bench import events_ms                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
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
    feat = m.feature_pass(image).features[0].contiguous()
    h, w, C = feat.shape
    full, tail = C // a.batch, C % a.batch
    cols = torch.arange(10, dtype=torch.int32, device="cuda")
    ranges = K.scorecam_ranges(feat, 224, 224)
    n = min(a.batch, C)
    buf = torch.empty((n, 3, 224, 224), device="cuda")
    acc = torch.zeros((10, h, w), device="cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def chunk():
        with torch.no_grad():
            logp = m(K.scorecam_mask_images(image[0], feat, ranges, buf, 0))
        K.scorecam_accumulate(logp, cols, feat, ranges, acc, 0)

    if a.iters:
        m.set_inference_fold(True)
        for _ in range(a.iters):
            chunk()
        torch.cuda.synchronize()
        return

    def bare():
        with torch.no_grad():
            for _ in range(full):
                m(x)
            if tail:
                m(x[:tail])

    say("%s features [%d, %d, %d]: %d live of %d channels" % (a.model, h, w, C, int((ranges[:, 1] - ranges[:, 0] > 0).sum()), C))
    for fold in (False, True):
        m.set_inference_fold(fold)
        for _ in range(2):                                   # every shape on this path warmed up
            scorecam(m, image, batch=a.batch)
            bare()
        t_cam, t_bare = [], []
        for _ in range(a.repeats):
            t_cam.append(events_ms(lambda: scorecam(m, image, batch=a.batch)))
            t_bare.append(events_ms(bare))
        say("%s 224^2, 10 classes, %d channels in chunks of %d, %s: scorecam ms %s -> %.0f masked images/s | bare model(x), %d "
            "forwards at batch %d%s, ms %s -> %.0f images/s | ratio %.3f"
            % (a.model, C, a.batch, "folded" if fold else "unfolded", " ".join("%.2f" % t for t in t_cam),
               C / min(t_cam) * 1e3, full, a.batch, " and one at %d" % tail if tail else "", " ".join("%.2f" % t for t in t_bare),
               C / min(t_bare) * 1e3, min(t_bare) / min(t_cam)))
        t_fp = [events_ms(lambda: m.feature_pass(image)) for _ in range(a.repeats)]
        say("%s %s: the feature pass of the one image alone: ms %s" % (a.model, "folded" if fold else "unfolded",
                                                                       " ".join("%.2f" % t for t in t_fp)))

    # ---- the mask writer next to RISE's at the same output shape, alternating
    masks = rise_masks(n, (224, 224), s=7, p=0.5, seed=0, device="cuda")
    f_cam = lambda: K.scorecam_mask_images(image[0], feat, ranges, buf, 0)
    f_rise = lambda: K.rise_mask_images(image[0], masks.grids, masks.shifts, buf, 7, check_shifts=False)
    f_cam(); f_rise()
    t_cam, t_rise = [], []
    for _ in range(a.repeats):
        t_cam.append(window(f_cam, 0.25) * 1e3)
        t_rise.append(window(f_rise, 0.25) * 1e3)
    nbytes = 4.0 * (buf.numel() + image[0].numel())
    floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
    say("scorecam_mask_images [%d, 3, 224, 224]: us %s | rise_mask_images at the same shape: us %s | best / best = %.2f | %.1f MB, "
        "floor %.1f us at %.1f TB/s, best / floor = %.2f"
        % (n, " ".join("%.1f" % v for v in t_cam), " ".join("%.1f" % v for v in t_rise), min(t_cam) / min(t_rise), nbytes / 1e6,
           floor, a.hbm_tbs, min(t_cam) / floor))

    # ---- the two small kernels
    logp = torch.log_softmax(torch.randn(n, 10, device="cuda"), dim=1)
    for name, fn, nbytes in (
            ("scorecam_ranges [%d, %d, %d] -> 224^2" % (h, w, C), lambda: K.scorecam_ranges(feat, 224, 224, out=ranges),
             4.0 * (feat.numel() + ranges.numel())),
            ("scorecam_accumulate %d channels onto [10, %d, %d]" % (n, h, w),
             lambda: K.scorecam_accumulate(logp, cols, feat, ranges, acc, 0),
             4.0 * (2 * acc.numel() + logp.numel() + n * h * w))):
        fn()
        t = window(fn, 0.25) * 1e3
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %.1f | %.3f MB, floor %.2f us at %.1f TB/s" % (name, t, nbytes / 1e6, floor, a.hbm_tbs))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
