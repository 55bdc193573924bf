"""Eval forward with the BatchNorms folded (SlotModel.set_inference_fold) against the layer-by-layer eval forward, in one
process, alternating, device events, every shape warmed up first, windows of at least --seconds each.

    python tools_dev/eval_fold_bench.py [c2 c5 b1] [--seconds 1.0] [--repeats 3] [--radix] [--out FILE.json]

c2: BASELINE config 2 (resnest26d, batch 70, 224^2, fp32); c5: config 5 (resnest50d, 100 classes x 3 slots, bf16, batch 256);
b1: one 224^2 image through resnest26d (scouter_amd/test.py's case: launch overhead).  Prints images/s and ms per forward
of each window and the spread over the repeats; --radix times the two candidates for the 3x3 radix convolutions of the
folded fp32 path at config 2's shapes (the register-split forward fed the fp32 tensor, against K.planes_split + the plane
kernel), per layer and as the whole forward."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import torch_oracle as O                     # noqa: E402
from scouter_amd import kernels as K, nn_hip             # noqa: E402
from scouter_amd.sloter.slot_model import SlotModel      # noqa: E402

CONFIGS = {
    "c2": dict(model="resnest26d", num_classes=10, slots_per_class=1, batch=70, precision="fp32"),
    "c5": dict(model="resnest50d", num_classes=100, slots_per_class=3, batch=256, precision="bf16"),
    "b1": dict(model="resnest26d", num_classes=10, slots_per_class=1, batch=1, precision="fp32"),
}


def make(cfg):
    args = argparse.Namespace(model=cfg["model"], pre_trained=False, num_classes=cfg["num_classes"], dataset="ImageNet",
                              use_slot=True, use_pre=False, grad=False, channel=2048, slots_per_class=cfg["slots_per_class"],
                              hidden_dim=64, freeze_layers=0, vis=False, vis_id=0, loss_status=1, power=2, to_k_layer=3,
                              lambda_value="1", precision=cfg["precision"])
    m = SlotModel(args)
    m.load_state_dict(O.synth_state(O.state_dict_spec(cfg["model"], cfg["num_classes"], cfg["slots_per_class"], 3), 300))
    images, _ = O.synth_batch(cfg["batch"], 3, 224, cfg["num_classes"], 301)
    return m.cuda().eval(), images.cuda()


def window(fn, seconds):
    """-> ms per call over a window of at least `seconds` (device events around the whole window)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, ms = 4, 0.0
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


def run(m, x):
    with torch.no_grad():
        return m(x)


def bench_config(name, seconds, repeats):
    m, x = make(CONFIGS[name])
    res = {"unfolded_ms": [], "folded_ms": []}
    for fold in (False, True):                           # warm-up of every shape on both paths (tile lookup, fold, planes)
        m.set_inference_fold(fold)
        for _ in range(3):
            run(m, x)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for fold, key in ((False, "unfolded_ms"), (True, "folded_ms")):
            m.inference_fold = fold                      # (the attribute: the folded tensors stay current between windows)
            res[key].append(window(lambda: run(m, x), seconds))
    B = x.shape[0]
    for key in ("unfolded_ms", "folded_ms"):
        v = res[key]
        res[key.replace("_ms", "_img_s")] = [1000.0 * B / t for t in v]
        print("%s %-9s ms/forward %s  images/s %s  spread %.2f %%" % (
            name, key[:-3], " ".join("%.3f" % t for t in v), " ".join("%.0f" % (1000.0 * B / t) for t in v),
            100.0 * (max(v) - min(v)) / min(v)))
    res["speedup"] = min(res["unfolded_ms"]) / min(res["folded_ms"])
    print("%s folded / unfolded: %.3f x (best windows)" % (name, res["speedup"]))
    return res


def bench_radix(seconds, repeats):
    """The radix convolutions of the folded fp32 path at config 2's shapes: conv + bias + ReLU on the fp32 tensor."""
    out = {"layers": [], "forward": {}}
    g = torch.Generator().manual_seed(5)
    for C, HW in ((64, 56), (128, 28), (256, 14), (512, 7)):     # C' of layer1..4 (stride-2 blocks run theirs one map larger)
        for hw in sorted({HW, min(2 * HW, 56)}):
            B, cin, cout = 70, C, 2 * C
            x = torch.randn(B, hw, hw, cin, generator=g).cuda()
            w = (torch.randn(3, 3, cin // 2, cout, generator=g) * 0.05).cuda()
            b = torch.randn(cout, generator=g).cuda()
            wf, _ = K.planes_split_weight(w, 2, 3, fwd=True, dgrad=False)
            cands = {"x3": lambda: K.conv2d_fwd_x3(x, wf, None, True, kh=3, pad=1, groups=2, bias=b),
                     "planes_split+planes": lambda: K.conv2d_fwd_planes(K.planes_split(x, 3), wf, 3, 3, 1, 1, 2, b, None, True)}
            if (cout // 2) % 64:
                del cands["planes_split+planes"]         # (the plane kernel wants 64-multiples of output channels per group)
            row = {"cin": cin, "cout": cout, "hw": hw}
            for k, fn in cands.items():
                fn()
                torch.cuda.synchronize()
                row[k + "_us"] = min(window(fn, seconds / 4) for _ in range(repeats)) * 1000.0
            print("radix 3x3 %4d -> %4d (2 groups) at 70 x %2d x %2d: %s" % (
                cin, cout, hw, hw, "  ".join("%s %.1f us" % (k, v) for k, v in row.items() if k.endswith("_us"))))
            out["layers"].append(row)
    m, x = make(CONFIGS["c2"])
    m.set_inference_fold(True)
    for radix in ("x3", "planes"):
        nn_hip.FOLD_RADIX = radix
        m.refold()
        for _ in range(3):
            run(m, x)
        out["forward"][radix] = [window(lambda: run(m, x), seconds) for _ in range(repeats)]
        print("c2 folded forward, radix convolutions on %-6s: ms %s" % (radix, " ".join("%.3f" % t for t in out["forward"][radix])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=[])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--radix", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {}
    if a.radix:
        res["radix"] = bench_radix(a.seconds, a.repeats)
    for name in a.configs or ([] if a.radix else ["c2", "c5", "b1"]):
        res[name] = bench_config(name, a.seconds, a.repeats)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
