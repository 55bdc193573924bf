"""Guided backpropagation, deconvnet and Guided Grad-CAM next to the plain folded gradient (tools/attribution.py), and the rule
kernels of csrc/bn_elem.hip / csrc/fold_bwd.hip and the product kernel of csrc/guided.hip at their largest shapes.

    python tools_dev/guided_bench.py [--model resnest26d] [--size 224] [--classes 10] [--batch 50] [--repeats 3] [--seconds 0.5]
                                     [--out profiles/guided_bench.txt]

Parameters frozen, fp32, device events; every figure is the best of --repeats windows of at least --seconds each, the calls taking
turns window by window in one process; every window is printed, so the spread is on the line.  Per batch size (1 and --batch):
  input_gradients(route="folded"), guided_backprop, deconvnet, guided_gradcam, and input_gradients(route="folded") followed by
  gradcam(relu=True) -- what Guided Grad-CAM would cost without the shared pass and head backward;
then the kernels back to back, rule 0 beside rules 1 and 2, with the bytes they must move and the rate against --hbm-tbs:
  relu_bwd at the stem's 112^2 x 64, sa_apply_relu_bwd at layer1's radix tensor (56^2 x 2 x 64), maxpool_relu_bwd at the stem,
  sa_gate_bwd at layer4's gate, guided_cam at the image's size in both modes."""
import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                     # noqa: E402
from scouter_amd.tools import attribution as AT          # noqa: E402
from tools_dev.foldgrad_bench import alternate, make     # noqa: E402

_OUT = [sys.stdout]


def emit(text):
    for f in _OUT:
        print(text, file=f, flush=True)


def line(what, times, unit="ms", scale=1.0, nbytes=None, tbs=None):
    """one line per call: every window, the best, the spread (max - min) / best; with nbytes {name: bytes} the rate of the best"""
    emit(what)
    best = {}
    for n, ts in times.items():
        v = [t * scale for t in ts]
        best[n] = min(v)
        rate = ""
        if nbytes is not None:
            r = nbytes[n] / (min(ts) * 1e-3) / 1e12
            rate = "  %.1f MB  %.2f TB/s = %.0f %% of %.1f" % (nbytes[n] / 1e6, r, 100.0 * r / tbs, tbs)
        emit("    %-34s %s  best %.3f %s  spread %.1f %%%s" % (n, " ".join("%.3f" % t for t in v), best[n], unit,
                                                             100.0 * (max(v) - min(v)) / min(v), rate))
    return best


def method_lines(a, m, x):
    cols = list(range(a.classes))
    fns = {
        "input_gradients(folded)": lambda: AT.input_gradients(m, x, classes=cols, route="folded"),
        "guided_backprop": lambda: AT.guided_backprop(m, x, classes=cols),
        "deconvnet": lambda: AT.deconvnet(m, x, classes=cols),
        "guided_gradcam": lambda: AT.guided_gradcam(m, x, classes=cols),
        "input_gradients(folded) + gradcam": lambda: (AT.input_gradients(m, x, classes=cols, route="folded"),
                                                      AT.gradcam(m, x, classes=cols, relu=True)),
    }
    best = line("%s %d^2, %d classes, batch %d, ms per call" % (a.model, a.size, a.classes, x.shape[0]),
                alternate(fns, a.repeats, a.seconds))
    base = best["input_gradients(folded)"]
    emit("    guided / gradient = %.3f   deconvnet / gradient = %.3f   guided_gradcam / (gradient + gradcam) = %.3f"
         % (best["guided_backprop"] / base, best["deconvnet"] / base, best["guided_gradcam"] / best["input_gradients(folded) + gradcam"]))


def kernel_lines(a):
    B, tbs = a.batch, a.hbm_tbs
    names = {0: "rule 0 gradient", 1: "rule 1 guided", 2: "rule 2 deconvnet"}
    hs = a.size // 2
    # relu_bwd at the stem's output
    y = torch.relu(torch.randn(B, hs, hs, 64, device="cuda"))
    dy = torch.randn_like(y)
    n = float(y.numel())
    t = alternate({names[r]: (lambda r=r: K.relu_bwd(dy, y, r)) for r in (0, 1, 2)}, a.repeats, a.seconds / 4)
    line("relu_bwd %dx%d x 64, %d rows, us per call" % (hs, hs, B), t, "us", 1000.0,
         {names[0]: 12.0 * n, names[1]: 12.0 * n, names[2]: 8.0 * n}, tbs)
    # maxpool_relu_bwd at the stem
    p, arg = K.maxpool_fwd(y, 3, 2, 1, want_argmax=True)
    dp = torch.randn_like(p)
    t = alternate({names[r]: (lambda r=r: K.maxpool_relu_bwd(dp, arg, y, rule=r)) for r in (0, 1, 2)}, a.repeats, a.seconds / 4)
    full, less = 8.0 * n + 5.0 * p.numel(), 4.0 * n + 5.0 * p.numel()
    line("maxpool_relu_bwd %dx%d x 64, %d rows, us per call" % (hs, hs, B), t, "us", 1000.0,
         {names[0]: full, names[1]: full, names[2]: less}, tbs)
    # sa_apply_relu_bwd at layer1's radix tensor
    hw, Cp = a.size // 4, 64
    dout, x0 = torch.randn(B, hw, hw, Cp, device="cuda"), torch.relu(torch.randn(B, hw, hw, 2 * Cp, device="cuda"))
    att = torch.softmax(torch.randn(B, 2, Cp, device="cuda"), dim=1).reshape(B, 2 * Cp).contiguous()
    dgap = torch.randn(B, Cp, device="cuda")
    t = alternate({names[r]: (lambda r=r: K.sa_apply_relu_bwd(dout, att, dgap, x0, r)) for r in (0, 1, 2)}, a.repeats, a.seconds / 4)
    e = float(dout.numel())
    line("sa_apply_relu_bwd %dx%d x %d, %d rows, us per call" % (hw, hw, Cp, B), t, "us", 1000.0,
         {names[0]: 20.0 * e, names[1]: 20.0 * e, names[2]: 12.0 * e}, tbs)
    # sa_gate_bwd at layer4's gate (launch-bound: no rate)
    Cp, A = 512, 256
    gap, w1, b1 = torch.randn(B, Cp, device="cuda"), torch.randn(1, 1, Cp, A, device="cuda"), torch.randn(A, device="cuda")
    w2 = torch.randn(1, 1, A, 2 * Cp, device="cuda")
    att = torch.softmax(torch.randn(B, 2, Cp, device="cuda"), dim=1).reshape(B, 2 * Cp).contiguous()
    da = torch.randn(B, 2 * Cp, device="cuda")
    t = alternate({names[r]: (lambda r=r: K.sa_gate_bwd(gap, w1, b1, w2, att, da, rule=r)) for r in (0, 1, 2)}, a.repeats, a.seconds / 4)
    line("sa_gate_bwd Cp %d A %d, %d rows, us per call" % (Cp, A, B), t, "us", 1000.0)
    # guided_cam at the image's size
    grad, cam = torch.randn(B, 3, a.size, a.size, device="cuda"), torch.rand(B, a.classes, a.size // 32, a.size // 32, device="cuda")
    out = torch.empty_like(grad)
    t = alternate({mode: (lambda mode=mode: K.guided_cam(grad, cam[:, 1], out=out, mode=mode)) for mode in ("nearest", "bilinear")},
                  a.repeats, a.seconds / 4)
    nb = 8.0 * grad.numel()
    line("guided_cam 3 x %d^2 from %d^2, %d rows, us per call" % (a.size, a.size // 32, B), t, "us", 1000.0,
         {"nearest": nb, "bilinear": nb}, tbs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the kernels' rates are set against, TB/s")
    ap.add_argument("--out", default=None, help="also write the lines to this file (profiles/guided_bench.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guided_bench: no HIP device -- nothing is measured without one")
    with contextlib.ExitStack() as stack:
        if a.out:
            _OUT.append(stack.enter_context(open(a.out, "w")))
        emit("guided_bench: %s, fp32, %s; best of %d windows of >= %.2f s, the calls taking turns"
             % (a.model, torch.cuda.get_device_name(0), a.repeats, a.seconds))
        m = make(a.model, a.classes)
        g = torch.Generator().manual_seed(301)
        for B in (1, a.batch):
            method_lines(a, m, torch.randn((B, 3, a.size, a.size), generator=g).cuda())
        if not a.skip_kernels:
            kernel_lines(a)


if __name__ == "__main__":
    main()
