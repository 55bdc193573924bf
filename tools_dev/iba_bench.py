"""Cost of one iteration of tools/attribution.information_bottleneck next to the head pass it drives, the two mask-side kernels of
csrc/iba.hip alone, and the same two steps written with eager torch ops -- what a port of the reference's IBA would run.

    python tools_dev/iba_bench.py [models ...] [--classes 10] [--samples 10] [--repeats 3] [--out FILE]

Per model (default resnest26d and resnet18; 224^2, fp32, 10 outputs, one image, --classes x --samples head rows in one pass): ms
per iteration of information_bottleneck -- the difference of a call of 41 and a call of 9 forwards over 32, so that the feature
pass and the allocations drop out -- next to ms of the bare head_pass + .grad at the same rows; the pairs alternate, device events
around whole calls.  Then iba_sample and iba_step alone at the model's feature shape -- device events around windows of
back-to-back launches -- with the bytes each has to move and its floor at --hbm-tbs, the two in sequence, and the eager
restatement of the same two steps on the device: sigmoid, ReflectionPad2d, a depthwise conv2d, normal_() noise, the blend, the KL
term and its mean, autograd through all of them and torch.optim.Adam -- one noise tensor and one blend of [K S, C, h, w] each way,
as the reference's _do_restrict_information builds them (one mask per class here, batched)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                               # noqa: E402
from scouter_amd.tools.attribution import IbaEstimate, information_bottleneck      # noqa: E402
from tools_dev.input_grad_bench import make, window                               # noqa: E402
from tools_dev.rise_bench import events_ms                                        # noqa: E402

SIGMA, BETA, MIN_STD = 1.0, 10.0, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fmt = lambda ts: " ".join("%.2f" % t for t in ts)                              # noqa: E731
    Kc, S = a.classes, a.samples
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, _ = make(model, 8)
        m.requires_grad_(False)
        m.eval()
        feats = m.feature_pass(x).features
        _, h, w, C = feats.shape
        est = IbaEstimate(feats.mean(0), feats.std(0).contiguous(), torch.ones((h, w, C), device="cuda"), 8)
        image, feat = x[:1], feats[0].contiguous()
        rows = torch.randn((Kc * S, h, w, C), device="cuda")
        seed = torch.zeros((Kc * S, 10), device="cuda")
        seed[torch.arange(Kc * S), (torch.arange(Kc * S) // S) % 10] = -1.0 / S

        def bare():
            m.head_pass(rows).grad(seed)

        run = lambda steps: information_bottleneck(m, image, est, classes=list(range(Kc)), steps=steps, samples=S)   # noqa: E731
        for _ in range(2):                                      # every shape on this path warmed up
            run(9); bare()
        t_long, t_short, t_bare = [], [], []
        for _ in range(a.repeats):
            t_long.append(events_ms(lambda: run(41)))
            t_short.append(events_ms(lambda: run(9)))
            t_bare.append(window(bare, 0.25))
        per_it = (min(t_long) - min(t_short)) / 32.0
        say("%s 224^2, one image, features %d x %d x %d, %d classes x %d samples in one pass: information_bottleneck 41 forwards ms %s | "
            "9 forwards ms %s | per iteration %.3f ms | bare head_pass + grad at %d rows, ms %s | bare / iteration %.3f"
            % (model, h, w, C, Kc, S, fmt(t_long), fmt(t_short), per_it, Kc * S, fmt(t_bare), min(t_bare) / per_it))

        # ---- the two kernels alone
        E = float(h * w * C)
        alpha = torch.full((Kc, h, w, C), 5.0, device="cuda")
        am, av = torch.zeros_like(alpha), torch.zeros_like(alpha)
        z, dz = torch.empty_like(rows), torch.randn((Kc * S, h, w, C), device="cuda") * 1e-3
        mean, std, act = est.mean.contiguous(), est.std, est.active

        def sample():
            K.iba_sample(feat, mean, std, act, alpha, z, None, SIGMA, 0, 1, False)

        def step():                                             # (in place: the masks drift, the work does not change)
            K.iba_step(feat, mean, std, act, alpha, dz, am, av, SIGMA, 0, 1, BETA, 1.0, False)

        kernels = (("iba_sample [%d, %d, %d, %d]" % (Kc * S, h, w, C), sample, 4.0 * E * (Kc * S + Kc + 4)),
                   ("iba_step [%d, %d, %d, %d]" % (Kc * S, h, w, C), step, 4.0 * E * (Kc * S + 6 * Kc + 4)))
        total = 0.0
        for name, fn, nbytes in kernels:
            fn()
            ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
            floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
            total += min(ts)
            say("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, best / floor = %.2f, %.1f %% of that rate"
                % (name, " ".join("%.1f" % t for t in ts), nbytes / 1e6, floor, a.hbm_tbs, min(ts) / floor, 100.0 * floor / min(ts)))

        def hip_side():
            sample(); step()

        # ---- the same two steps with eager torch ops, NCHW as the reference holds them
        r = K.iba_radius(SIGMA)
        d = torch.arange(-r, r + 1, device="cuda", dtype=torch.float32)
        g2 = torch.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * SIGMA * SIGMA))
        weight = (g2 / g2.sum()).expand(C, 1, -1, -1).contiguous()
        pad = torch.nn.ReflectionPad2d(r)
        xc, mc, ac = (v.permute(2, 0, 1).contiguous() for v in (feat, mean, act))
        sc = torch.clamp(std.permute(2, 0, 1), min=MIN_STD).contiguous()
        leaf = torch.full((Kc, C, h, w), 5.0, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([leaf], lr=1.0)
        dzc = dz.permute(0, 3, 1, 2).contiguous().view(Kc, S, C, h, w)

        def eager_side():
            lamb = torch.nn.functional.conv2d(pad(torch.sigmoid(leaf)), weight, groups=C)
            rn = (xc - mc) / sc
            var = (1.0 - lamb) ** 2
            cap = -0.5 * (1.0 + torch.log(var) - (rn * lamb) ** 2 - var) * ac
            eps = torch.empty((Kc, S, C, h, w), device="cuda").normal_()
            zz = (lamb[:, None] * xc + (1.0 - lamb[:, None]) * (sc * eps + mc)) * ac
            opt.zero_grad(set_to_none=True)
            ((zz * dzc).sum() + BETA * cap.mean((1, 2, 3)).sum()).backward()   # (dzc stands for the head's backward)
            opt.step()

        hip_side(); eager_side()
        t_hip = [window(hip_side, 0.25) * 1e3 for _ in range(a.repeats)]
        t_eager = [window(eager_side, 0.25) * 1e3 for _ in range(a.repeats)]
        say("%s: the two mask-side steps in sequence: HIP us %s (sum of the single best times %.1f) | eager torch us %s | eager / HIP = "
            "%.1f" % (model, " ".join("%.1f" % t for t in t_hip), total, " ".join("%.1f" % t for t in t_eager),
                      min(t_eager) / min(t_hip)))
        say("%s: the mask side is %.1f %% of an iteration (%.1f us of %.1f), the head pass and its backward %.1f %%"
            % (model, 100.0 * min(t_hip) / (1e3 * per_it), min(t_hip), 1e3 * per_it, 100.0 * min(t_bare) / per_it))
        del m
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
