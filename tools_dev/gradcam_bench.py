"""Cost of per-class Grad-CAM heat maps for a batch, next to the gradient attribution maps, and the two kernels alone.

    python tools_dev/gradcam_bench.py [--model resnest26d] [--batch 70] [--seconds 1.0] [--repeats 3]

224^2, fp32, 10 classes, nothing trainable: ms of tools/attribution.gradcam_maps for every class of the batch (one backbone
forward, ten head backwards, ten kernels.gradcam, one kernels.cam_maps), unfolded and BatchNorm-folded, and of
attribution_maps(input_gradients(...)) on the same inputs (ten whole-model forwards and backwards, the maps on the host: a host
clock around calls that end with the maps on the host for both).  Then kernels.gradcam on [batch, 7, 7, 2048] and
kernels.cam_maps on [batch * 10, 7, 7] -> 224^2 with their byte floors (feat + dfeat read once and the map written; the
sources read and the bytes written) / --hbm-tbs, device events around windows of at least --seconds / 4."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                                    # noqa: E402
from scouter_amd.tools.attribution import attribution_maps, gradcam_maps, input_gradients   # noqa: E402
from tools_dev.input_grad_bench import make, window                                     # noqa: E402


def host_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    a = ap.parse_args()
    m, x, _ = make(a.model, a.batch)
    m.requires_grad_(False)
    m.eval()
    fmt = lambda v: " ".join("%.3f" % t for t in v)
    for fold in (False, True):
        m.set_inference_fold(fold)
        fn = lambda: gradcam_maps(m, x)
        for _ in range(3):
            fn()
        dev = [window(fn, a.seconds) for _ in range(a.repeats)]
        host = host_ms(lambda: gradcam_maps(m, x).cpu(), a.repeats)
        print("%s batch %d 224^2, 10 classes, %s: gradcam_maps ms %s (device events) | with the maps on the host ms %s"
              % (a.model, a.batch, "folded" if fold else "unfolded", fmt(dev), fmt(host)))
    m.set_inference_fold(False)
    grads = lambda: attribution_maps(input_gradients(m, x))
    grads()
    print("%s batch %d 224^2, 10 classes: attribution_maps(input_gradients) ms %s (host clock, maps on the host)"
          % (a.model, a.batch, fmt(host_ms(grads, a.repeats))))
    sal = lambda: input_gradients(m, x)
    print("%s batch %d 224^2, 10 classes: input_gradients alone ms %s (device events)"
          % (a.model, a.batch, fmt([window(sal, a.seconds) for _ in range(a.repeats)])))

    B, h, C, S = a.batch, 7, 2048, 224
    feat, dfeat = torch.randn(B, h, h, C, device="cuda"), torch.randn(B, h, h, C, device="cuda")
    cam = torch.empty(B, 10, h, h, device="cuda")
    fn = lambda: K.gradcam(feat, dfeat, cam[:, 3])
    fn()
    t = [window(fn, a.seconds / 4) * 1e3 for _ in range(a.repeats)]
    nbytes = 4.0 * (2 * feat.numel() + B * h * h)
    floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
    print("gradcam [%d, %d, %d, %d]: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
          % (B, h, h, C, " ".join("%.1f" % v for v in t), nbytes / 1e6, floor, a.hbm_tbs, min(t) / floor))
    cam.normal_()
    fn = lambda: K.cam_maps(cam, S, S, 0.0)
    fn()
    t = [window(fn, a.seconds / 4) * 1e3 for _ in range(a.repeats)]
    nbytes = 4.0 * cam.numel() + float(B * 10 * S * S)
    floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
    print("cam_maps [%d, %d, %d] -> %d^2: us %s | %.1f MB, floor %.1f us at %.1f TB/s, best / floor = %.2f"
          % (B * 10, h, h, S, " ".join("%.1f" % v for v in t), nbytes / 1e6, floor, a.hbm_tbs, min(t) / floor))


if __name__ == "__main__":
    main()
