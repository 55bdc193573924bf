"""Cost of the infidelity and max-sensitivity scores next to the forwards and explanations they are made of, and the two
streaming kernels of csrc/fidelity.hip alone.

    python tools_dev/fidelity_bench.py [models ...] [--samples 50] [--sens-samples 10] [--repeats 3] [--out FILE]

Per model (default resnest26d and resnet18; 224^2, fp32, 10 classes, one image, one class, parameters frozen): ms of one
tools/attribution.infidelity call of a full [3, 224, 224] attribution (--samples noisy copies and the clean image in ONE forward,
batch = samples + 1: kernels.noise_images, the eval-mode forward, kernels.output_deltas, kernels.perturb_dots,
kernels.infidelity_finish) next to ms of the bare eval forwards at the same batch sizes, and ms of one sensitivity_max call of
`gradcam` (--sens-samples perturbed copies, batch = samples + 1: kernels.uniform_images, gradcam, kernels.map_distances,
kernels.sensitivity_finish) next to ms of the bare gradcam calls at the same batch sizes; the pairs alternate, device events
around whole calls.  bare / call is what everything around the forwards costs.  Then perturb_dots (K = 1 and K = 10 attributions,
full and map form) and uniform_images alone at [--samples, 3, 224, 224] with the bytes they move and their floor at --hbm-tbs;
perturb_dots reads K attributions once per tile of samples and writes next to nothing -- it is bound by Philox and Box-Muller,
not by bytes -- so its time is also given relative to noise_images at the same shape, which draws the same normals."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                               # noqa: E402
from scouter_amd.tools.attribution import gradcam, infidelity, sensitivity_max    # noqa: E402
from tools_dev.input_grad_bench import make, window                               # noqa: E402
from tools_dev.rise_bench import events_ms                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--sens-samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fmt = lambda ts: " ".join("%.2f" % t for t in ts)                              # noqa: E731
    N, Ns = a.samples, a.sens_samples
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, _ = make(model, N + 1)
        m.requires_grad_(False)
        m.eval()
        image = x[:1]
        attr = torch.randn((1, 1, 3, 224, 224), generator=torch.Generator().manual_seed(3)).cuda()

        def bare_forward():
            with torch.no_grad():
                m(x[:N + 1])

        def bare_cam():
            gradcam(m, x[:Ns + 1], classes=[0])

        f_inf = lambda: infidelity(m, image, attr, classes=[0], n_samples=N, batch=N + 1)                      # noqa: E731
        f_sens = lambda: sensitivity_max(lambda im: gradcam(m, im, classes=[0]), image, n_samples=Ns, batch=Ns + 1)   # noqa: E731
        for _ in range(2):                                      # every shape on this path warmed up
            f_inf(); bare_forward(); f_sens(); bare_cam()
        t_inf, t_fwd, t_sens, t_cam = [], [], [], []
        for _ in range(a.repeats):
            t_inf.append(events_ms(f_inf))
            t_fwd.append(events_ms(bare_forward))
            t_sens.append(events_ms(f_sens))
            t_cam.append(events_ms(bare_cam))
        say("%s 224^2, one image, one class, parameters frozen: infidelity (%d samples, batch %d) ms %s | bare eval forward at batch "
            "%d, ms %s | bare / infidelity %.3f || sensitivity_max of gradcam (%d samples, batch %d) ms %s | bare gradcam at batch %d, "
            "ms %s | bare / sensitivity_max %.3f" % (model, N, N + 1, fmt(t_inf), N + 1, fmt(t_fwd), min(t_fwd) / min(t_inf), Ns,
                                                     Ns + 1, fmt(t_sens), Ns + 1, fmt(t_cam), min(t_cam) / min(t_sens)))
        del m

    # ---- the two streaming kernels alone
    shape = (3, 224, 224)
    E = 3 * 224 * 224
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(shape, generator=gen).cuda()
    buf = torch.empty((N,) + shape, device="cuda")
    full = torch.randn((10,) + shape, generator=gen).cuda()
    maps = torch.randn((10,) + shape[1:], generator=gen).cuda()
    dots = torch.zeros((10, N), dtype=torch.float64, device="cuda")
    tiles = -(-N // K.PERTURB_DOTS_SAMPLE_TILE)                # the attributions are read once per tile of samples
    noise = lambda: K.noise_images(img, buf, 1.0, 0, 0)                            # noqa: E731
    noise()
    t_noise = min(window(noise, 0.25) * 1e3 for _ in range(a.repeats))
    kernels = (
        ("noise_images [%d, 3, 224, 224]" % N, noise, 4.0 * (N * E + E)),
        ("uniform_images [%d, 3, 224, 224]" % N, lambda: K.uniform_images(img, buf, 1.0, 0, 0), 4.0 * (N * E + E)),
        ("perturb_dots %d samples, K = 1, full" % N, lambda: K.perturb_dots(full[:1], dots[:1], 1.0, 0, 0, N), 4.0 * E * tiles),
        ("perturb_dots %d samples, K = 10, full" % N, lambda: K.perturb_dots(full, dots, 1.0, 0, 0, N), 4.0 * 10 * E * tiles),
        ("perturb_dots %d samples, K = 1, map" % N, lambda: K.perturb_dots(maps[:1], dots[:1], 1.0, 0, 0, N, channels=3),
         4.0 * E * tiles),
        ("perturb_dots %d samples, K = 10, map" % N, lambda: K.perturb_dots(maps, dots, 1.0, 0, 0, N, channels=3),
         4.0 * 10 * E * tiles))
    for name, fn, nbytes in kernels:
        fn()
        ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        say("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, best / floor = %.2f | best / noise_images = %.2f"
            % (name, " ".join("%.1f" % t for t in ts), nbytes / 1e6, floor, a.hbm_tbs, min(ts) / floor, min(ts) / t_noise))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
