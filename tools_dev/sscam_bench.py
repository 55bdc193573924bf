"""Cost of SS-CAM next to the bare forwards it is made of, next to Score-CAM in the same run, and the family's four kernels alone.

    python tools_dev/sscam_bench.py [--model resnest26d] [--batch 250] [--samples 35] [--sigma 2.0] [--repeats 3] [--out FILE]
                                    [--iters N]

224^2, fp32, 10 classes, one image, with the inference fold off and on: ms of one tools/attribution.sscam call at the defaults
(one feature pass, kernels.scorecam_ranges, then per chunk kernels.sscam_mask_images, the model, kernels.sscam_weights, and
kernels.sscam_contract at the end) and ms of bare `model(x)` forwards under no_grad at the same batch sizes (N C // batch at
`batch` and one at N C % batch), device events around whole calls, the two alternating; then the same pair for
tools/attribution.scorecam, the same loop with one sample and no noise.  The two ratios side by side are what the noise costs
per chunk.  Then kernels.sscam_mask_images without and with noise at the same output shape, alternating, with the byte floor at
--hbm-tbs and the share of one forward of the same chunk, and kernels.scorecam_ranges / kernels.sscam_weights /
kernels.sscam_contract once each.
--iters N: instead, N chunks (mask writer with noise, forward, weights) and nothing else -- the body of a
`rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                 # noqa: E402
from scouter_amd.tools.attribution import scorecam, sscam           # noqa: E402
from tools_dev.input_grad_bench import make, window                 # noqa: E402
from tools_dev.rise_bench import events_ms                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--samples", type=int, default=35)
    ap.add_argument("--sigma", type=float, default=2.0)
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
    N = a.samples
    cols = torch.arange(10, dtype=torch.int32, device="cuda")
    ranges = K.scorecam_ranges(feat, 224, 224)
    n = min(a.batch, C)
    buf = torch.empty((n, 3, 224, 224), device="cuda")
    wsum = torch.zeros((C, 10), dtype=torch.float64, device="cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def chunk():
        with torch.no_grad():
            logp = m(K.sscam_mask_images(image[0], feat, ranges, buf, 0, N, a.sigma, 0))
        K.sscam_weights(logp, cols, wsum, 0)

    if a.iters:
        m.set_inference_fold(True)
        for _ in range(a.iters):
            chunk()
        torch.cuda.synchronize()
        return

    def bare(rows):
        full, tail = rows // n, rows % n

        def run():
            with torch.no_grad():
                for _ in range(full):
                    m(x[:n])
                if tail:
                    m(x[:tail])
        return run, full, tail

    say("%s features [%d, %d, %d]: %d live of %d channels" % (a.model, h, w, C, int((ranges[:, 1] - ranges[:, 0] > 0).sum()), C))
    for fold in (False, True):
        m.set_inference_fold(fold)
        state = "folded" if fold else "unfolded"
        ratios = {}
        for name, rows, call in (("sscam", N * C, lambda: sscam(m, image, n_samples=N, sigma=a.sigma, batch=a.batch)),
                                 ("scorecam", C, lambda: scorecam(m, image, batch=a.batch))):
            run, full, tail = bare(rows)
            call()                                           # every shape on this path warmed up
            run()
            t_cam, t_bare = [], []
            for _ in range(a.repeats):
                t_cam.append(events_ms(call))
                t_bare.append(events_ms(run))
            ratios[name] = min(t_bare) / min(t_cam)
            say("%s 224^2, 10 classes, %d rows in chunks of %d, %s: %s ms %s -> %.0f masked images/s | bare model(x), %d forwards "
                "at batch %d%s, ms %s -> %.0f images/s | ratio %.3f"
                % (a.model, rows, n, state, name, " ".join("%.2f" % t for t in t_cam), rows / min(t_cam) * 1e3, full, n,
                   " and one at %d" % tail if tail else "", " ".join("%.2f" % t for t in t_bare), rows / min(t_bare) * 1e3,
                   ratios[name]))
        say("%s %s: sscam ratio %.3f against scorecam ratio %.3f from the same run: %+.3f"
            % (a.model, state, ratios["sscam"], ratios["scorecam"], ratios["sscam"] - ratios["scorecam"]))

    # ---- the mask writer without and with noise at the same output shape, alternating
    m.set_inference_fold(False)
    f_new = lambda: K.sscam_mask_images(image[0], feat, ranges, buf, 0, N, 0.0, 0)
    f_noise = lambda: K.sscam_mask_images(image[0], feat, ranges, buf, 0, N, a.sigma, 0)

    def forward():
        with torch.no_grad():
            m(buf)
    f_new(); f_noise(); forward()
    t_new, t_noise, t_fwd = [], [], []
    for _ in range(a.repeats):
        t_new.append(window(f_new, 0.25) * 1e3)
        t_noise.append(window(f_noise, 0.25) * 1e3)
        t_fwd.append(window(forward, 0.25) * 1e3)
    nbytes = 4.0 * (buf.numel() + image[0].numel())
    floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
    us = lambda ts: " ".join("%.1f" % v for v in ts)
    say("sscam_mask_images [%d, 3, 224, 224] sigma 0: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
        % (n, us(t_new), nbytes / 1e6, floor, a.hbm_tbs, min(t_new) / floor))
    say("sscam_mask_images [%d, 3, 224, 224] sigma %g: us %s | best / floor = %.2f | one unfolded forward of the chunk: us %s | "
        "share of the forward %.4f"
        % (n, a.sigma, us(t_noise), min(t_noise) / floor, us(t_fwd), min(t_noise) / min(t_fwd)))

    # ---- the three small kernels
    logp = torch.log_softmax(torch.randn(n, 10, device="cuda"), dim=1)
    out = torch.empty((10, h, w), device="cuda")
    for name, fn, nbytes in (
            ("scorecam_ranges [%d, %d, %d] -> 224^2" % (h, w, C), lambda: K.scorecam_ranges(feat, 224, 224, out=ranges),
             4.0 * (feat.numel() + ranges.numel())),
            ("sscam_weights [%d rows, 10 classes]" % n, lambda: K.sscam_weights(logp, cols, wsum, 0),
             4.0 * logp.numel() + 16.0 * n * 10),
            ("sscam_contract [10, %d, %d] x %d" % (h, w, C), lambda: K.sscam_contract(wsum, feat, ranges, out, 1.0 / N),
             4.0 * (out.numel() + feat.numel() + ranges.numel()) + 8.0 * wsum.numel())):
        fn()
        ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %s | %.3f MB, floor %.2f us at %.1f TB/s" % (name, us(ts), nbytes / 1e6, floor, a.hbm_tbs))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
