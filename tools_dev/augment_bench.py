"""The train transform of one batch of 70 mixed-size frames to 224 x 224, with and without `--aug true`: device events around
the call on an otherwise idle stream after warm-up (the frames already packed in pinned memory, as the DataLoader delivers
them), then the per-kernel split from the library's own event timing.
usage: python tools_dev/augment_bench.py [step_ms of `python bench.py` for the comparison] [output file]"""
import ctypes
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from scouter_amd import _native                                                   # noqa: E402
from scouter_amd.dataset.transform_func import GpuTransform, PackedImages         # noqa: E402

B, S, REPS = 70, 224, 30
step_ms = float(sys.argv[1]) if len(sys.argv) > 1 else None
rng = np.random.default_rng(0)
sizes = [(int(rng.integers(300, 520)), int(rng.integers(330, 640))) for _ in range(B)]       # typical ImageNet frames
packed = PackedImages.pack([torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]).pin_memory()
dev = torch.device("cuda")
L = _native.lib()
buf = ctypes.create_string_buffer(1 << 14)
lines = ["train transform, %d frames (%d-%d x %d-%d) -> %d^2, %s" % (B, 300, 519, 330, 639, S, torch.cuda.get_device_name(0))]


def measure(tf):
    for _ in range(5):
        tf(packed, dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tf(packed, dev)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    L.scouter_prof_collect(buf, len(buf)); L.scouter_prof_enable(1)
    for _ in range(REPS):
        tf(packed, dev)
    torch.cuda.synchronize()
    L.scouter_prof_enable(0); L.scouter_prof_collect(buf, len(buf))
    split = []
    for row in buf.value.decode().splitlines():
        name, n, ms = row.split("\t")[:3]
        split.append("    %-18s %2d launches per call, %7.1f us per call" % (name, round(float(n) / REPS), float(ms) / REPS * 1e3))
    return float(np.median(times)), float(np.min(times)), split


for label, tf in (("aug off", GpuTransform("ImageNet", S)), ("aug on ", GpuTransform("ImageNet", S, aug=True, aug_seed=1))):
    med, low, split = measure(tf)
    lines.append("%s: %.3f ms per call (median of %d; fastest %.3f), H2D copy of %.1f MB included"
                 % (label, med, REPS, low, packed.flat.numel() / 1e6))
    lines += split
    if label.startswith("aug on") and step_ms is not None:
        lines.append("training step it hides behind (bench.py of the parent commit, same machine): %.2f ms -> the augmenting "
                     "transform is %s (%.0f %% of the step)" % (step_ms, "shorter" if med < step_ms else "NOT shorter",
                                                              100 * med / step_ms))
text = "\n".join(lines)
print(text)
if len(sys.argv) > 2:
    open(sys.argv[2], "w").write(text + "\n")
