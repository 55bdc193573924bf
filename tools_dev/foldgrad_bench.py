"""Image-space gradients by the two routes of tools/attribution.py: the autograd route (the unfolded eval forward and the training
backward walked on to the image, once per class) against the folded route (SlotModel.image_pass: one BatchNorm-folded forward per
batch of rows, a gradient-only backward per class), and the three kernels of csrc/fold_bwd.hip at their real shapes.

    python tools_dev/foldgrad_bench.py [--model resnest26d] [--size 224] [--classes 10] [--repeats 3] [--seconds 0.5]
    python tools_dev/foldgrad_bench.py --iters 10 --batch 70         # the body of a `rocprofv3 --kernel-trace --stats` run

Parameters frozen, fp32, device events; every figure is the best of --repeats windows of at least --seconds each, the two routes
ALTERNATING window by window in one process.  Per model:
  input_gradients, every class, at batch 1 and at batch 50;
  integrated_gradients at 50 steps in one chunk, one image, every class;
  one image_pass + one .grad per class against as many autograd forward and backward pairs, 50 rows;
  sa_gate_bwd, sa_apply_relu_bwd and maxpool_relu_bwd at the shapes of the four stages (50 rows) with the bytes they must move
  over --hbm-tbs, next to the passes they replace (radix_softmax_bwd .. fc1's input gradient; sa_apply_bwd + relu_bwd;
  maxpool_bwd + relu_bwd)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import torch_oracle as O                     # noqa: E402
from scouter_amd import kernels as K                     # noqa: E402
from scouter_amd.sloter.slot_model import SlotModel      # noqa: E402
from scouter_amd.tools import attribution as AT          # noqa: E402


def make(model, n_classes):
    args = argparse.Namespace(model=model, pre_trained=False, num_classes=n_classes, dataset="ImageNet", use_slot=True, use_pre=False,
                              grad=False, channel=O.ARCHS[model]["channel"], slots_per_class=1, hidden_dim=64, freeze_layers=0,
                              vis=False, vis_id=0, loss_status=1, power=2, to_k_layer=3, lambda_value="1", precision="fp32")
    m = SlotModel(args)
    m.load_state_dict(O.synth_state(O.state_dict_spec(model, n_classes, 1, 3), 300))
    m.requires_grad_(False)
    return m.cuda().eval()


def window(fn, seconds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1000.0 * seconds:
            return ms / n
        n = max(n * 2, int(n * 1100.0 * seconds / max(ms, 1e-3)) + 1)


def alternate(fns, repeats, seconds):
    """{name: [ms per call of every window]}: the functions take turns, window by window"""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            times[name].append(window(fn, seconds))
    return times


def line(what, times, unit="ms", scale=1.0):
    names = list(times)
    best = {n: min(times[n]) * scale for n in names}
    cells = " | ".join("%s %s (best %.3f)" % (n, " ".join("%.3f" % (t * scale) for t in times[n]), best[n]) for n in names)
    ratio = "" if len(names) != 2 else " | %s / %s = %.2f" % (names[0], names[1], best[names[0]] / best[names[1]])
    print("%s, %s: %s%s" % (what, unit, cells, ratio), flush=True)
    return best


def kernel_lines(a):
    """the three kernels at the shapes of resnest's four stages, `--batch` rows of a --size image"""
    B = a.batch
    floor = lambda nbytes: nbytes / (a.hbm_tbs * 1e12) * 1e6
    for stage, (Cp, A) in enumerate(((64, 32), (128, 64), (256, 128), (512, 256)), 1):
        hw = a.size // 2 ** (stage + 1)                                      # the stage's stride-1 blocks: 56, 28, 14, 7 at 224
        HW = hw * hw
        gap, w1, b1 = torch.randn(B, Cp, device="cuda"), torch.randn(1, 1, Cp, A, device="cuda"), torch.randn(A, device="cuda")
        w2 = torch.randn(1, 1, A, 2 * Cp, device="cuda")
        att = torch.softmax(torch.randn(B, 2, Cp, device="cuda"), dim=1).reshape(B, 2 * Cp).contiguous()
        da = torch.randn(B, 2 * Cp, device="cuda")
        g1 = torch.relu(torch.randn(B, 1, 1, A, device="cuda"))

        def unfused_gate():
            dz2 = K.radix_softmax_bwd(att, da)
            dg1 = K.conv2d_dgrad(dz2.view(B, 1, 1, -1), w2, (B, 1, 1, A))
            return K.conv2d_dgrad(K.relu_bwd(dg1, g1), w1, (B, 1, 1, Cp))

        t = alternate({"sa_gate_bwd": lambda: K.sa_gate_bwd(gap, w1, b1, w2, att, da), "unfused chain": unfused_gate}, a.repeats,
                      a.seconds / 4)
        nbytes = 4.0 * (B * (Cp + 4 * Cp + Cp) + 2 * Cp * A + A)
        line("stage %d gate backward Cp %d A %d, %d rows (%.2f MB, floor %.2f us at %.1f TB/s)"
             % (stage, Cp, A, B, nbytes / 1e6, floor(nbytes), a.hbm_tbs), t, "us", 1000.0)
        dout, x0 = torch.randn(B, hw, hw, Cp, device="cuda"), torch.relu(torch.randn(B, hw, hw, 2 * Cp, device="cuda"))
        dgap = torch.randn(B, Cp, device="cuda")
        t = alternate({"sa_apply_relu_bwd": lambda: K.sa_apply_relu_bwd(dout, att, dgap, x0),
                       "sa_apply_bwd + relu_bwd": lambda: K.relu_bwd(K.sa_apply_bwd(dout, att, dgap), x0)}, a.repeats, a.seconds / 4)
        nbytes = 4.0 * B * HW * Cp * 5                                       # dout once, x0 and dx twice the width
        line("stage %d apply backward %dx%d x %d, %d rows (%.1f MB, floor %.1f us)" % (stage, hw, hw, Cp, B, nbytes / 1e6, floor(nbytes)),
             t, "us", 1000.0)
    hs = a.size // 2
    h = torch.relu(torch.randn(B, hs, hs, 64, device="cuda"))
    p, arg = K.maxpool_fwd(h, 3, 2, 1, want_argmax=True)
    dy = torch.randn_like(p)
    t = alternate({"maxpool_relu_bwd": lambda: K.maxpool_relu_bwd(dy, arg, h),
                   "maxpool_bwd + relu_bwd": lambda: K.relu_bwd(K.maxpool_bwd(dy, arg, tuple(h.shape)), h)}, a.repeats, a.seconds / 4)
    nbytes = 8.0 * h.numel() + 5.0 * p.numel()
    line("stem pool backward %dx%d x 64, %d rows (%.1f MB, floor %.1f us)" % (hs, hs, B, nbytes / 1e6, floor(nbytes)), t, "us", 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnest26d")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=0, help="N folded saliency batches (one class) and nothing else")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("foldgrad_bench: no HIP device -- nothing is measured without one")
    m = make(a.model, a.classes)
    g = torch.Generator().manual_seed(301)
    x1 = torch.randn((1, 3, a.size, a.size), generator=g).cuda()
    xb = torch.randn((a.batch, 3, a.size, a.size), generator=g).cuda()
    if a.iters:
        for _ in range(a.iters):
            AT.input_gradients(m, xb, classes=[3], route="folded")
        torch.cuda.synchronize()
        return
    cols = list(range(a.classes))
    routes = lambda f: {"autograd": lambda: f("autograd"), "folded": lambda: f("folded")}
    what = "%s %d^2, %d classes" % (a.model, a.size, a.classes)
    line("%s: input_gradients, batch 1" % what, alternate(routes(lambda r: AT.input_gradients(m, x1, route=r)), a.repeats, a.seconds))
    line("%s: input_gradients, batch %d" % (what, a.batch),
         alternate(routes(lambda r: AT.input_gradients(m, xb, route=r)), a.repeats, a.seconds))
    line("%s: integrated_gradients, 50 steps in one chunk, one image" % what,
         alternate(routes(lambda r: AT.integrated_gradients_by_route(m, x1, n_steps=50, batch=50, route=r)), a.repeats, a.seconds))
    seeds = []
    for c in cols:
        s = torch.zeros((a.batch, a.classes), device="cuda")
        s[:, c] = 1.0
        seeds.append(s)

    def pairs():
        with torch.enable_grad():
            for s in seeds:
                AT._chunk_gradient(m, xb, s)

    def one_pass():
        ip = m.image_pass(xb)
        for s in seeds:
            ip.grad(s)

    line("%s: %d autograd forward + backward pairs against one image_pass + %d .grad, %d rows" % (what, a.classes, a.classes, a.batch),
         alternate({"autograd": pairs, "folded": one_pass}, a.repeats, a.seconds))
    ip = m.image_pass(xb)
    t = alternate({"image_pass": lambda: m.image_pass(xb), "one .grad": lambda: ip.grad(seeds[0]),
                   "folded eval forward": lambda: m._forward_folded(xb, None)}, a.repeats, a.seconds)
    line("%s: the parts, %d rows" % (what, a.batch), t)
    if not a.skip_kernels:
        kernel_lines(a)


if __name__ == "__main__":
    main()
