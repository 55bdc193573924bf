"""Cost of the three kernels the explanation table adds, next to the eval forward they are called beside, and the wall time of
the table tool.

    python tools_dev/explanation_table_bench.py [--model resnest26d] [--batch 70] [--seconds 0.25] [--repeats 3] [--table 64]

Device events around windows of at least --seconds after a warm-up: kernels.cam_fc on [batch, 7, 7, 2048] with 10 and 200 classes
and on [64, 2, 2, 512] with 10, and with per-image columns (K = 1, the table tool's call), kernels.map_localization on [batch, 1, 224, 224] with one box an image, kernels.group_maps on
[batch, 10, 49], each with its byte floor (every operand read or written once) / --hbm-tbs, and SlotModel.feature_pass of the
same batch at 224^2.  Then a host clock around one run of `python -m scouter_amd.tools.explanation_table` for --table images
(0: skipped) at 224^2 with the options of tests/test_explanation_table_gpu.py: slot, grad, cam and rise (6 masks) with
--localization, --causal (--causal_step 2048) and --infidelity (3 samples), batches of 4."""
import argparse
import contextlib
import io
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                                    # noqa: E402
from tools_dev.input_grad_bench import make, window                                     # noqa: E402


def report(what, fn, nbytes, a):
    for _ in range(3):
        fn()
    t = [window(fn, a.seconds) * 1e3 for _ in range(a.repeats)]
    floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
    print("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, best / floor = %.1f"
          % (what, " ".join("%.1f" % v for v in t), nbytes / 1e6, floor, a.hbm_tbs, min(t) / floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--seconds", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--table", type=int, default=64, help="images of the table tool's run (0: skip it)")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    a = ap.parse_args()
    B = a.batch
    for shape, n in (((B, 7, 7, 2048), 10), ((B, 7, 7, 2048), 200), ((64, 2, 2, 512), 10)):
        feat, w = torch.randn(shape, device="cuda"), torch.randn((n, shape[3]), device="cuda")
        cols = torch.arange(n, dtype=torch.int32, device="cuda")
        out = torch.empty((shape[0], n, shape[1], shape[2]), device="cuda")
        report("cam_fc %s, %d classes" % (list(shape), n), lambda: K.cam_fc(feat, w, cols, out),
               4.0 * (feat.numel() + w.numel() + out.numel()), a)
    # the call of the table tool: every image its own class, K = 1 (one of a workgroup's eight waves contracts)
    feat, w = torch.randn((B, 7, 7, 2048), device="cuda"), torch.randn((10, 2048), device="cuda")
    own = (torch.arange(B, device="cuda") % 10).to(torch.int32)
    out = torch.empty((B, 1, 7, 7), device="cuda")
    report("cam_fc %s, 10 classes, per image (K = 1)" % [B, 7, 7, 2048], lambda: K.cam_fc(feat, w, own, out, per_image=True),
           4.0 * (feat.numel() + w.numel() + out.numel()), a)
    maps = torch.randint(0, 256, (B, 1, 224, 224), dtype=torch.uint8, device="cuda")
    boxes = torch.tensor([[[40, 50, 180, 200]]] * B, dtype=torch.int32, device="cuda")
    n_boxes = torch.ones(B, dtype=torch.int32, device="cuda")
    report("map_localization [%d, 1, 224, 224], one box" % B, lambda: K.map_localization(maps, boxes, n_boxes), float(maps.numel()), a)
    attn = torch.rand((B, 10, 49), device="cuda")
    report("group_maps [%d, 10, 49]" % B, lambda: K.group_maps(attn), 5.0 * attn.numel(), a)

    m, x, _ = make(a.model, B)
    m.requires_grad_(False)
    m.eval()
    for fold in (False, True):
        m.set_inference_fold(fold)
        fn = lambda: m.feature_pass(x)
        for _ in range(3):
            fn()
        print("%s batch %d 224^2, %s: feature_pass ms %s (device events)"
              % (a.model, B, "folded" if fold else "unfolded", " ".join("%.3f" % window(fn, a.seconds) for _ in range(a.repeats))))
    del m, x

    if a.table > 0:
        from scouter_amd.tools import explanation_table as X
        argv = ["explanation_table.py", "--model", a.model, "--dataset", "ImageNet", "--channel", "2048", "--num_classes", "10",
                "--slots_per_class", "1", "--to_k_layer", "3", "--power", "2", "--use_slot", "true", "--pre_trained", "false",
                "--img_size", "224", "--synthetic_data", "true", "--num_workers", "0", "--output_dir", "",
                "--table_images", str(a.table), "--batch_size", "4", "--localization", "true", "--causal", "true", "--causal_step",
                "2048", "--infidelity", "true", "--infidelity_samples", "3", "--cam", "true", "--rise", "true", "--rise_masks", "6",
                "--rise_batch", "4", "--grad", "true"]
        old, sys.argv = sys.argv, argv
        text = io.StringIO()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                X.main()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            sys.argv = old
        print("table tool, %s 224^2, %d images in batches of 4, slot grad cam rise x localization causal infidelity: %.1f s wall "
              "(model construction and the first launches included)" % (a.model, a.table, wall))
        for line in text.getvalue().splitlines():
            if line.startswith("table "):
                print("    " + line)


if __name__ == "__main__":
    main()
