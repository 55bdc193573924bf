"""Cost of one iteration of tools/attribution.igos next to the model passes it contains, the mask-side kernels of csrc/igos.hip
alone, and the same mask-side steps written with eager torch ops on the device -- what a port of the reference's Integrated_Mask
would run once its host round trips were taken out.

    python tools_dev/igos_bench.py [models ...] [--classes 10] [--repeats 3] [--out FILE]

Per model (default resnest26d and resnet18; 224^2, fp32, one image, --classes classes, the defaults of `igos`: an 8 x 8 mask, 20
path points, 12 trial steps, batch 50, parameters frozen): ms per iteration of igos -- the difference of a call of 3 and a call of
1 iteration over 2, so that the blur and the allocations drop out -- next to ms of the bare model passes of an iteration at the
same batches: R S eval forward + input backward and R T1 eval forwards; the pairs alternate, device events around whole calls.
Then each kernel alone at the shapes of that iteration (a chunk of 50 rows) -- device events around windows of back-to-back
launches -- with the bytes it has to move, its floor at --hbm-tbs and its share of that rate; the mask side of one iteration in
sequence (4 path chunks, 4 contractions, the mask gradient, 3 trial chunks, the step); and the eager restatement of the same work:
F.interpolate(align_corners=True), torch.randn for the noise, autograd through the upsampler for the adjoint and the L1 / TV terms,
the candidates of the whole ladder and their selection by torch ops."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                               # noqa: E402
from scouter_amd.tools.attribution import igos, igos_ladder                         # noqa: E402
from tools_dev.input_grad_bench import make, window                               # noqa: E402
from tools_dev.rise_bench import events_ms                                        # noqa: E402

H = W = 224
HM, S, BATCH, SIGMA, L1, TV, BETA, ALPHA = 8, 20, 50, 0.2, 1.0, 20.0, 2.0, 1e-4


def chunks(total):
    return [(first, min(BATCH, total - first)) for first in range(0, total, BATCH)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fmt = lambda ts: " ".join("%.2f" % t for t in ts)                              # noqa: E731
    us = lambda ts: " ".join("%.1f" % t for t in ts)                               # noqa: E731
    R = a.classes
    ladder = igos_ladder()
    T1 = len(ladder)
    iteration_ms = {}
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, _ = make(model, BATCH)
        m.requires_grad_(False)
        m.eval()
        image = x[:1]
        seed = torch.zeros((BATCH, 10), device="cuda")
        seed[torch.arange(BATCH), torch.arange(BATCH) % 10] = 0.1

        def bare():
            for _, n in chunks(R * S):
                leaf = x[:n].detach().requires_grad_(True)
                torch.autograd.grad(m(leaf), leaf, seed[:n])
            with torch.no_grad():
                for _, n in chunks(R * T1):
                    m(x[:n])

        run = lambda iters: igos(m, image, classes=list(range(R)), n_iters=iters, batch=BATCH)   # noqa: E731
        for _ in range(2):                                      # every shape on this path warmed up
            run(1); bare()
        t_long, t_short, t_bare = [], [], []
        for _ in range(a.repeats):
            t_long.append(events_ms(lambda: run(3)))
            t_short.append(events_ms(lambda: run(1)))
            t_bare.append(events_ms(bare))
        per_it = (min(t_long) - min(t_short)) / 2.0
        iteration_ms[model] = (per_it, min(t_bare))
        say("%s 224^2, one image, %d classes, %d x %d mask, %d path points, %d trial steps, batch %d, parameters frozen: igos 3 iterations "
            "ms %s | 1 iteration ms %s | per iteration %.3f ms | the bare passes of an iteration (%d forward + backward, %d forwards) ms %s "
            "| bare / iteration %.3f" % (model, R, HM, HM, S, T1 - 1, BATCH, fmt(t_long), fmt(t_short), per_it, R * S, R * T1, fmt(t_bare),
                                        min(t_bare) / per_it))
        del m

    # ---- the kernels alone, at the shapes of one iteration
    gen = torch.Generator().manual_seed(1)
    img, base = torch.randn((3, H, W), generator=gen).cuda(), torch.randn((3, H, W), generator=gen).cuda()
    p0 = torch.rand((R, HM, HM), generator=gen).cuda()
    pm = p0.clone()
    buf = torch.empty((BATCH, 3, H, W), device="cuda")
    dx = torch.randn((BATCH, 3, H, W), generator=gen).cuda()
    acc = torch.zeros((R, H, W), dtype=torch.float64, device="cuda")
    l1 = torch.full((R,), L1, device="cuda")
    dmask, stats = torch.empty((R, HM, HM), device="cuda"), torch.empty((R, 2), dtype=torch.float64, device="cuda")
    steps = torch.tensor(ladder, dtype=torch.float64).float().cuda()
    logp = torch.log_softmax(torch.randn((R * T1, 10), generator=gen), dim=1).cuda()
    cols = (torch.arange(R) % 10).to(torch.int32).cuda()
    curves = torch.zeros((R, 15, 4), dtype=torch.float64, device="cuda")
    up = torch.empty((R, H, W), device="cuda")
    E, px, cells = float(3 * H * W), float(H * W), float(R * HM * HM)
    rows_acc = (BATCH - 1) // S + 1

    def step():                                                 # (in place on a copy: the masks drift, the work does not change)
        K.igos_step(pm, dmask, steps, logp, cols, stats, l1, curves, 1, 15, ALPHA, TV, BETA, False)

    K.igos_mask_grad(p0, acc, l1, dmask, stats, TV, BETA)
    kernels = (
        ("igos_path_images [%d, 3, 224, 224]" % BATCH, lambda: K.igos_path_images(img, base, p0, buf, 0, S, SIGMA, 0, 0), 4.0 * (BATCH * E + 2 * E + cells)),
        ("igos_accumulate [%d, 3, 224, 224]" % BATCH, lambda: K.igos_accumulate(img, base, dx, acc, 0, S), 4.0 * (BATCH * E + 2 * E) + 16.0 * rows_acc * px),
        ("igos_mask_grad [%d, %d, %d] <- [%d, 224, 224]" % (R, HM, HM, R), lambda: K.igos_mask_grad(p0, acc, l1, dmask, stats, TV, BETA), 8.0 * R * px + 8.0 * cells),
        ("igos_trial_images [%d, 3, 224, 224]" % BATCH, lambda: K.igos_trial_images(img, base, p0, dmask, steps, buf, 0), 4.0 * (BATCH * E + 2 * E + 2 * cells)),
        ("igos_step [%d, %d, %d], %d candidates" % (R, HM, HM, T1), step, 4.0 * (3 * cells + R * T1)),
        ("igos_upsample [%d, 224, 224]" % R, lambda: K.igos_upsample(p0, up), 4.0 * (R * px + cells)))
    for name, fn, nbytes in kernels:
        fn()
        ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        if nbytes < 1e5:                                        # a launch, not a stream: a byte floor would be noise
            say("%s: us %s | %.0f bytes" % (name, us(ts), nbytes))
            continue
        say("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, %.1f %% of that rate" % (name, us(ts), nbytes / 1e6, floor, a.hbm_tbs,
                                                                                     100.0 * floor / min(ts)))

    def hip_side():
        acc.zero_()
        for first, n in chunks(R * S):
            K.igos_path_images(img, base, p0, buf[:n], first, S, SIGMA, 0, 0)
            K.igos_accumulate(img, base, dx[:n], acc, first, S)
        K.igos_mask_grad(p0, acc, l1, dmask, stats, TV, BETA)
        for first, n in chunks(R * T1):
            K.igos_trial_images(img, base, p0, dmask, steps, buf[:n], first)
        step()

    # ---- the same steps with eager torch ops on the device
    leaf = p0.clone().requires_grad_(True)
    d = img - base
    a_path = (torch.arange(1, S + 1, device="cuda", dtype=torch.float32) / S)
    w_path = (a_path / S).view(1, S, 1, 1)
    prob = torch.exp(logp.view(R, T1, 10)[torch.arange(R), :, cols.long()])
    rows = torch.arange(R, device="cuda")

    def tv_l1(p):
        return L1 * (1.0 - p).abs().mean((-2, -1)) + TV * ((p[..., :-1, :] - p[..., 1:, :]).abs().pow(BETA).mean((-2, -1)) +
                                                          (p[..., :, :-1] - p[..., :, 1:]).abs().pow(BETA).mean((-2, -1)))

    def eager_side():
        u = torch.nn.functional.interpolate(leaf[:, None], size=(H, W), mode="bilinear", align_corners=True)[:, 0]
        noise = SIGMA * torch.randn((S, 3, H, W), device="cuda")
        contraction = torch.zeros((R, H, W), device="cuda")
        for first, n in chunks(R * S):
            g = torch.arange(first, first + n, device="cuda")
            r, j = g // S, g % S
            buf[:n] = base + (a_path[j].view(n, 1, 1) * u.detach()[r])[:, None] * d + noise[j]
            contraction.index_add_(0, r, (a_path[j] / S).view(n, 1, 1) * (dx[:n] * d).sum(1))
        grad = torch.autograd.grad((u * contraction).sum() + tv_l1(leaf).sum(), leaf)[0]
        cand = torch.clamp(leaf.detach()[:, None] - steps.view(1, T1, 1, 1) * grad[:, None], 0.0, 1.0)
        uc = torch.nn.functional.interpolate(cand, size=(H, W), mode="bilinear", align_corners=True).flatten(0, 1)
        for first, n in chunks(R * T1):
            buf[:n] = base + uc[first:first + n, None] * d
        tot = tv_l1(cand) + prob
        ok = ~(tot > tot[:, :1] - ALPHA * steps * (grad * grad).sum((1, 2))[:, None])
        ok[:, 0], ok[:, -1] = False, True
        chosen = torch.argmax(ok.to(torch.int32), dim=1)
        with torch.no_grad():
            leaf.copy_(cand[rows, chosen])
        return w_path

    hip_side(); eager_side()
    t_hip = [window(hip_side, 0.25) * 1e3 for _ in range(a.repeats)]
    t_eager = [window(eager_side, 0.25) * 1e3 for _ in range(a.repeats)]
    say("the mask side of one iteration in sequence, %d classes (4 path chunks, 4 contractions, mask gradient, 3 trial chunks, step): "
        "HIP us %s | eager torch us %s | eager / HIP = %.1f" % (R, us(t_hip), us(t_eager), min(t_eager) / min(t_hip)))
    for model, (per_it, bare_ms) in iteration_ms.items():
        say("%s: an iteration is %.2f ms: model passes %.2f ms (%.1f %%), mask-side kernels %.3f ms (%.1f %%)"
            % (model, per_it, bare_ms, 100.0 * bare_ms / per_it, 1e-3 * min(t_hip), 100.0 * min(t_hip) / (1e3 * per_it)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
