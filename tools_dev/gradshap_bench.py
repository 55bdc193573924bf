"""Cost of GradientSHAP at the image and at the backbone's output next to Integrated Gradients and layer IG at the same number of
path rows, the share of each spent outside the model passes, and the three kernels of csrc/gradshap.hip next to the pair they stand
in for (kernels.path_images, kernels.grad_accumulate), timed in the same run.

    python tools_dev/gradshap_bench.py [--model resnest26d] [--samples 50] [--batch 50] [--layer-samples 200] [--head-batch 256]
                                       [--baselines 10] [--repeats 3] [--hbm-tbs 6.3] [--out FILE]

224^2, fp32, 10 classes, one image, the inference fold on, no parameter trainable.  tools/attribution.gradient_shap (per class and
chunk: kernels.gradshap_images, a forward and a backward, kernels.gradshap_accumulate; kernels.attr_finish per class) with sigma 0
and 0.1, and integrated_gradients at n_steps = samples, against the same forwards and backwards alone; layer_gradient_shap (one
feature pass of the bank and the image; per chunk kernels.gradshap_images and ONE head pass, per class a `.grad` and
kernels.gradshap_accumulate; kernels.layer_attr_finish) and layer_integrated_gradients at the same number of path rows against
their feature pass, head passes and head backwards alone.  Device events around whole calls, the image calls alternating among
themselves and the layer calls among themselves.  The share of a call spent outside the model passes is 1 - passes / call.

Then the kernels alone, back to back in a timing window: the bytes a kernel must move once (rows written or gradients read, the
image, the bank rows that are drawn, the float64 sums both ways) over its time, against --hbm-tbs (bench.py HBM_ACHIEVABLE_TBS).
Back-to-back launches over a few tens of megabytes find part of their data in the last-level cache, so a rate above that figure is
no error; the ratio to the old kernel at the same shape, measured the same way, is what the comparison rests on."""
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
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--layer-samples", type=int, default=200)
    ap.add_argument("--head-batch", type=int, default=256)
    ap.add_argument("--baselines", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the kernels' rates are set against, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    R, n_classes, seed = a.baselines, 10, 0
    img_rows = [min(a.batch, a.samples - first) for first in range(0, a.samples, a.batch)]
    head_rows = [min(a.head_batch, a.layer_samples - first) for first in range(0, a.layer_samples, a.head_batch)]
    m, x, _ = make(a.model, max(img_rows + [R + 1]))
    m.requires_grad_(False)
    m.eval()
    m.set_inference_fold(True)
    image = x[:1].contiguous()
    feat = m.feature_pass(image).features.detach().contiguous()
    _, h, w, C = feat.shape
    fbuf = feat.repeat(max(head_rows), 1, 1, 1).contiguous()
    onehot = torch.zeros((max(img_rows + head_rows), n_classes), device="cuda")
    onehot[:, 0] = 1.0
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def image_passes():
        with torch.enable_grad():
            for _ in range(n_classes):
                for rows in img_rows:
                    A._chunk_gradient(m, x[:rows], onehot)

    def head_passes(first_rows):
        def run():
            m.feature_pass(x[:first_rows])
            for rows in head_rows:
                fp = m.head_pass(fbuf[:rows])
                for _ in range(n_classes):
                    fp.grad(onehot[:rows])
        return run

    gs = dict(baselines=R, n_samples=a.samples, batch=a.batch, seed=seed)
    lgs = dict(baselines=R, n_samples=a.layer_samples, batch=a.head_batch, seed=seed)
    methods = (("gradshap", lambda: A.gradient_shap(m, image, sigma=0.0, **gs)),
               ("gradshap sigma 0.1", lambda: A.gradient_shap(m, image, sigma=0.1, **gs)),
               ("ig", lambda: A.integrated_gradients(m, image, n_steps=a.samples, batch=a.batch)),
               ("image passes", image_passes),
               ("layergradshap", lambda: A.layer_gradient_shap(m, image, **lgs)),
               ("layergradshap passes", head_passes(R + 1)),
               ("layerig", lambda: A.layer_integrated_gradients(m, image, n_steps=a.layer_samples, batch=a.head_batch)),
               ("layerig passes", head_passes(2)))
    # the image methods and the layer methods alternate among themselves: the layer calls are bound by the host's launch rate
    # (4 ms of launches), and one that follows 90 ms of image passes measured a millisecond slower than the same call among its like
    times = {name: [] for name, _ in methods}
    for group in (methods[:4], methods[4:]):
        for _ in range(2):                                       # every shape on these paths warmed up
            for _, fn in group:
                fn()
        for _ in range(a.repeats):
            for name, fn in group:
                times[name].append(events_ms(fn))
    best = {name: min(t) for name, t in times.items()}
    rows_of = lambda rows: " ".join(str(r) for r in rows)        # noqa: E731
    what = {"gradshap": "gradshap, %d samples in chunks of %d, a Gaussian bank of %d, sigma 0" % (a.samples, a.batch, R),
            "gradshap sigma 0.1": "gradshap, the same with sigma 0.1",
            "ig": "ig, %d steps in chunks of %d" % (a.samples, a.batch),
            "image passes": "the same %d forwards and backwards per class (rows %s) alone" % (len(img_rows), rows_of(img_rows)),
            "layergradshap": "layergradshap, %d samples in chunks of %d rows, a bank of %d" % (a.layer_samples, a.head_batch, R),
            "layergradshap passes": "one feature pass of %d rows, the same %d head passes (rows %s) and %d head backwards each, alone"
                                    % (R + 1, len(head_rows), rows_of(head_rows), n_classes),
            "layerig": "layerig, %d steps in chunks of %d rows" % (a.layer_samples, a.head_batch),
            "layerig passes": "one feature pass of 2 rows, the same %d head passes (rows %s) and %d head backwards each, alone"
                              % (len(head_rows), rows_of(head_rows), n_classes)}
    for name, _ in methods:
        say("%s, %s 224^2 (%d x %d x %d), 10 classes, folded: ms per image %s -> best %.3f"
            % (what[name], a.model, h, w, C, " ".join("%.3f" % t for t in times[name]), best[name]))
    share = {}
    for name, passes in (("gradshap", "image passes"), ("gradshap sigma 0.1", "image passes"), ("ig", "image passes"),
                         ("layergradshap", "layergradshap passes"), ("layerig", "layerig passes")):
        share[name] = 100.0 * (1.0 - best[passes] / best[name])
        say("%s: %.2f %% of the call is spent outside the model passes (best of %d each)" % (name, share[name], a.repeats))

    # ---- the kernels alone, the old pair at the same E and n in the same run
    def timed(name, fn, nbytes):
        fn()
        t = [window(fn, 0.1) * 1e3 for _ in range(a.repeats)]
        tbs = nbytes / (min(t) * 1e-6) / 1e12
        say("%s: us %s | %.2f MB once -> %.2f TB/s = %.0f %% of %.1f TB/s" % (name, " ".join("%.1f" % v for v in t), nbytes / 1e6, tbs,
                                                                             100.0 * tbs / a.hbm_tbs, a.hbm_tbs))
        return t

    spread = 0.0
    # (the layer shape at the method's sample count and at a full chunk of --head-batch rows)
    for label, shape, n in (("image", (3, 224, 224), a.samples), ("layer", (h, w, C), a.layer_samples),
                            ("layer, a full chunk", (h, w, C), a.head_batch)):
        E = shape[0] * shape[1] * shape[2]
        img = torch.randn(shape, device="cuda")
        bank = torch.randn((R,) + shape, device="cuda")
        rows = torch.empty((n,) + shape, device="cuda")
        grads = torch.randn((n,) + shape, device="cuda")
        acc = torch.zeros(shape, dtype=torch.float64, device="cuda")
        alphas = torch.rand(n, device="cuda")
        weights = torch.rand(n, device="cuda")
        drawn = min(R, n)
        say("-- %s shape: E = %d, n = %d, R = %d" % (label, E, n, R))
        timed("gradshap_draws [%d]" % n, lambda: K.gradshap_draws(n, R, seed), 8.0 * n)
        old_rows = timed("path_images [%d, %s]" % (n, ", ".join(map(str, shape))), lambda: K.path_images(img, bank[0], alphas, rows, 0),
                         4.0 * E * (n + 2))
        old_acc = timed("grad_accumulate [%d, %s]" % (n, ", ".join(map(str, shape))), lambda: K.grad_accumulate(grads, weights, acc, None, 0),
                        4.0 * E * n + 16.0 * E)
        for sigma in ((0.0, 0.1) if label == "image" else (0.0,)):
            new_rows = timed("gradshap_images [%d, %s], sigma %g" % (n, ", ".join(map(str, shape)), sigma),
                             lambda: K.gradshap_images(img, bank, rows, sigma, seed, 0), 4.0 * E * (n + 1 + drawn))
            new_acc = timed("gradshap_accumulate [%d, %s], sigma %g" % (n, ", ".join(map(str, shape)), sigma),
                            lambda: K.gradshap_accumulate(grads, img, bank, acc, sigma, seed, 0, 1.0 / n), 4.0 * E * (n + 1 + drawn) + 16.0 * E)
            for new, old, pair in ((new_rows, old_rows, "gradshap_images / path_images"), (new_acc, old_acc, "gradshap_accumulate / grad_accumulate")):
                say("%s, sigma %g: %.2f (best of %d each)" % (pair, sigma, min(new) / min(old), a.repeats))
            for t in (new_rows, new_acc):
                spread = max(spread, (max(t) - min(t)) / min(t))
        for t in (old_rows, old_acc):
            spread = max(spread, (max(t) - min(t)) / min(t))
    say("spread of a kernel's time over its %d windows, the largest of all the kernels timed above (draws apart): %.1f %%"
        % (a.repeats, 100.0 * spread))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
