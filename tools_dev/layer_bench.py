"""Cost of layer IG, layer conductance, HiResCAM and LayerCAM next to the model passes they are made of, and the share their kernels
take.

    python tools_dev/layer_bench.py [--model resnest26d] [--steps 50] [--head-batch 256] [--batch 50] [--repeats 3] [--out FILE]

224^2, fp32, 10 classes, one image, the inference fold on, no parameter trainable.  tools/attribution.layer_integrated_gradients
(one feature pass of two rows; every chunk: kernels.path_images, ONE SlotModel.head_pass, per class a `.grad` and
kernels.grad_accumulate; then kernels.layer_attr_finish) against the same passes alone -- the feature pass, the head passes at the
same row counts and the same number of head backwards; layer_conductance (every chunk: kernels.path_images, one feature pass,
per class a `.grad` and kernels.conductance_accumulate; then layer_attr_finish) against its feature passes and head backwards
alone; hirescam and layercam (one feature pass, per class a `.grad` and kernels.layer_gxa) against theirs.  Device events around
whole calls, the calls alternating.  The share of a call spent outside the model passes is 1 - passes / call.  Then the kernels
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--head-batch", type=int, default=256)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lig_rows = [min(a.head_batch, a.steps - first) for first in range(0, a.steps, a.head_batch)]
    cond_rows = [1 + min(a.batch - 1, a.steps - first) for first in range(0, a.steps, a.batch - 1)]
    m, x, _ = make(a.model, max(cond_rows + [2]))
    m.requires_grad_(False)
    m.eval()
    m.set_inference_fold(True)
    image = x[:1].contiguous()
    n_classes = 10
    feat = m.feature_pass(image).features.detach().contiguous()
    _, h, w, C = feat.shape
    fbuf = feat.repeat(max(lig_rows), 1, 1, 1).contiguous()
    seed = torch.zeros((max(lig_rows + cond_rows), n_classes), device="cuda")
    seed[:, 0] = 1.0
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def backwards(fp, rows):
        for _ in range(n_classes):
            fp.grad(seed[:rows])

    def lig_passes():
        m.feature_pass(x[:2])
        for rows in lig_rows:
            backwards(m.head_pass(fbuf[:rows]), rows)

    def cond_passes():
        for rows in cond_rows:
            backwards(m.feature_pass(x[:rows]), rows)

    def cam_passes():
        backwards(m.feature_pass(image), 1)

    methods = (("layerig", lambda: A.layer_integrated_gradients(m, image, n_steps=a.steps, batch=a.head_batch)),
               ("layerig passes", lig_passes),
               ("conductance", lambda: A.layer_conductance(m, image, n_steps=a.steps, batch=a.batch)),
               ("conductance passes", cond_passes),
               ("hirescam", lambda: A.hirescam(m, image)),
               ("layercam", lambda: A.layercam(m, image)),
               ("cam passes", cam_passes))
    for _ in range(2):                                           # every shape on these paths warmed up
        for _, fn in methods:
            fn()
    times = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            times[name].append(events_ms(fn))
    best = {name: min(t) for name, t in times.items()}
    rows_of = lambda rows: " ".join(str(r) for r in rows)        # noqa: E731
    what = {"layerig": "layerig, %d steps in chunks of %d rows" % (a.steps, a.head_batch),
            "layerig passes": "one feature pass of 2 rows, the same %d head passes (rows %s) and %d head backwards each, alone"
                              % (len(lig_rows), rows_of(lig_rows), n_classes),
            "conductance": "conductance, %d steps in chunks of %d rows" % (a.steps, a.batch),
            "conductance passes": "the same %d feature passes (rows %s) and %d head backwards each, alone"
                                  % (len(cond_rows), rows_of(cond_rows), n_classes),
            "hirescam": "hirescam", "layercam": "layercam",
            "cam passes": "one feature pass and %d head backwards alone" % n_classes}
    for name, _ in methods:
        say("%s, %s 224^2 (%d x %d x %d), 10 classes, folded: ms per image %s -> best %.3f"
            % (what[name], a.model, h, w, C, " ".join("%.3f" % t for t in times[name]), best[name]))
    share = {}
    for name, passes in (("layerig", "layerig passes"), ("conductance", "conductance passes"), ("hirescam", "cam passes"),
                         ("layercam", "cam passes")):
        share[name] = 100.0 * (1.0 - best[passes] / best[name])
        say("%s: %.2f %% of the call is spent outside the model passes (best of %d each)" % (name, share[name], a.repeats))

    # ---- the kernels at the shapes of one image, times the launches an image needs
    rows, crows = max(lig_rows), max(cond_rows)
    alphas, weights = (t.cuda() for t in A.ig_quadrature(a.steps))
    grads = torch.randn((max(rows, crows), h, w, C), device="cuda")
    feats = torch.randn((crows, h, w, C), device="cuda")
    acc = torch.zeros((n_classes, h, w, C), dtype=torch.float64, device="cuda")
    cam = torch.empty((n_classes, h, w), device="cuda")
    one = torch.empty((1, n_classes, h, w), device="cuda")
    for method, kernels in (("layerig", (
            ("path_images [%d, %d, %d, %d]" % (rows, h, w, C), lambda: K.path_images(feat[0], None, alphas, fbuf[:rows], 0), len(lig_rows)),
            ("grad_accumulate [%d, %d, %d, %d]" % (rows, h, w, C), lambda: K.grad_accumulate(grads[:rows], weights, acc[0], None, 0),
             len(lig_rows) * n_classes),
            ("layer_attr_finish path, K %d, %d positions, %d channels" % (n_classes, h * w, C),
             lambda: K.layer_attr_finish(K.LAYER_PATH, acc, cam, feat=feat[0]), 1))),
                            ("conductance", (
            ("path_images [%d, 3, 224, 224]" % crows, lambda: K.path_images(image[0], None, alphas, x[:crows], 0), len(cond_rows)),
            ("conductance_accumulate [%d, %d, %d, %d]" % (crows, h, w, C), lambda: K.conductance_accumulate(feats, grads[:crows], acc[0]),
             len(cond_rows) * n_classes),
            ("layer_attr_finish sum, K %d, %d positions, %d channels" % (n_classes, h * w, C),
             lambda: K.layer_attr_finish(K.LAYER_SUM, acc, cam), 1))),
                            ("hirescam", (
            ("layer_gxa [1, %d, %d, %d]" % (h, w, C), lambda: K.layer_gxa(feat, grads[:1], one[:, 0]), n_classes),)),
                            ("layercam", (
            ("layer_gxa [1, %d, %d, %d], rectify and relu" % (h, w, C), lambda: K.layer_gxa(feat, grads[:1], one[:, 0], True, True),
             n_classes),))):
        total_us = 0.0
        for name, fn, launches in kernels:
            fn()
            t = [window(fn, 0.1) * 1e3 for _ in range(a.repeats)]
            total_us += min(t) * launches
            say("%s: us %s | x %d launches per image = %.1f us" % (name, " ".join("%.1f" % v for v in t), launches, min(t) * launches))
        say("the kernels of %s: %.3f ms per image = %.2f %% of its %.3f ms (%.2f %% of the call is outside the model passes)"
            % (method, total_us / 1e3, 0.1 * total_us / best[method], best[method], share[method]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
