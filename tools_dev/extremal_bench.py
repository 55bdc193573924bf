"""Cost of one iteration of tools/attribution.extremal_perturbation next to the model step it drives, the mask-side kernels of
csrc/extremal.hip alone, and the same mask-side steps written with eager torch ops -- what a port of TorchRay would run.

    python tools_dev/extremal_bench.py [models ...] [--masks 10] [--repeats 3] [--out FILE]

Per model (default resnest26d and resnet18; 224^2, fp32, 10 classes, one image, --masks classes x one area in one batch,
parameters frozen): ms per iteration of extremal_perturbation -- the difference of a call of 40 and a call of 8 iterations over
32, so that the pyramid and the allocations drop out -- next to ms of the bare eval forward + input backward at batch --masks;
the pairs alternate, device events around whole calls.  Then each mask-side step alone at [--masks, 224, 224] (extremal_mask,
extremal_blend, extremal_seed, saliency_ranks, extremal_mask_grad, extremal_step) -- device events around windows of
back-to-back launches on buffers of 6 - 17 MB that stay in cache, so launch rates, not profiler kernel times -- with the bytes
it has to move (blend and mask_grad: two pyramid levels per pixel and channel) and its floor at --hbm-tbs, their sum, and the
eager restatement of the same six steps on the device: the gather formulation of the upsampler (a [n, H, W, 81] window tensor,
as TorchRay's unfold builds), torch.gather on the pyramid, torch.sort for the area term, autograd for both backwards and
torch.optim.SGD(momentum, dampening) for the update."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scouter_amd import kernels as K                                               # noqa: E402
from scouter_amd.tools.attribution import extremal_perturbation, perturbation_pyramid   # noqa: E402
from tools_dev.input_grad_bench import make, window                               # noqa: E402
from tools_dev.rise_bench import events_ms                                        # noqa: E402

H = W = 224
STEP, SIGMA, LEVELS, BETA = 7, 21.0, 8, 20.0


def eager_tables():
    """kern, cell, inside [H, W, D, D] of the upsampler on the device (fp32 / int64 / bool)"""
    hm, wm, r = K.extremal_grid(H, W, STEP, SIGMA)
    a = torch.arange(-r, r + 1, device="cuda")
    ci = (torch.arange(H, device="cuda") // STEP)[:, None] + a
    cj = (torch.arange(W, device="cuda") // STEP)[:, None] + a
    dy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] - ((ci.float() + 0.5) * STEP - 0.5)
    dx = torch.arange(W, device="cuda", dtype=torch.float32)[:, None] - ((cj.float() + 0.5) * STEP - 0.5)
    z = torch.sqrt(dy[:, None, :, None] ** 2 + dx[None, :, None, :] ** 2) / SIGMA
    kern = torch.exp(-2.0 * torch.clamp(z - 0.5, min=0.0) ** 2)
    inside = ((ci >= 0) & (ci < hm))[:, None, :, None] & ((cj >= 0) & (cj < wm))[None, :, None, :]
    cell = ci.clamp(0, hm - 1)[:, None, :, None] * wm + cj.clamp(0, wm - 1)[None, :, None, :]
    return kern * inside, cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=[])
    ap.add_argument("--masks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate of the byte floors, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fmt = lambda ts: " ".join("%.2f" % t for t in ts)                              # noqa: E731
    n = a.masks
    iteration_ms = {}
    for model in a.models or ["resnest26d", "resnet18"]:
        m, x, _ = make(model, n)
        m.requires_grad_(False)
        m.eval()
        image = x[:1]
        seed = torch.zeros((n, 10), device="cuda")
        seed[torch.arange(n), torch.arange(n) % 10] = -0.1

        def bare():
            leaf = x.detach().requires_grad_(True)
            torch.autograd.grad(m(leaf), leaf, seed)

        run = lambda iters: extremal_perturbation(m, image, classes=list(range(n)), areas=(0.1,), n_iters=iters, batch=n)   # noqa: E731
        for _ in range(2):                                      # every shape on this path warmed up
            run(8); bare()
        t_long, t_short, t_bare = [], [], []
        for _ in range(a.repeats):
            t_long.append(events_ms(lambda: run(40)))
            t_short.append(events_ms(lambda: run(8)))
            t_bare.append(window(bare, 0.25))
        per_it = (min(t_long) - min(t_short)) / 32.0
        iteration_ms[model] = per_it
        say("%s 224^2, one image, %d classes x one area in one batch, parameters frozen: extremal_perturbation 40 iterations ms %s | "
            "8 iterations ms %s | per iteration %.3f ms | bare eval forward + backward at batch %d, ms %s | bare / iteration %.3f"
            % (model, n, fmt(t_long), fmt(t_short), per_it, n, fmt(t_bare), min(t_bare) / per_it))
        del m

    # ---- the mask-side steps alone
    gen = torch.Generator().manual_seed(1)
    hm, wm, _ = K.extremal_grid(H, W, STEP, SIGMA)
    img = torch.randn((3, H, W), generator=gen).cuda()
    pyr = perturbation_pyramid(img, LEVELS, 20.0)
    p0 = torch.rand((n, hm, wm), generator=gen).cuda()
    pm, mom = p0.clone(), torch.zeros_like(p0)
    mask, dmask = torch.empty((n, H, W), device="cuda"), torch.empty((n, H, W), device="cuda")
    stats = torch.empty((n, H, W, 2), device="cuda")
    buf = torch.empty((n, 3, H, W), device="cuda")
    dx = torch.randn((n, 3, H, W), generator=gen).cuda()
    ranks = torch.empty((n, H * W), dtype=torch.int32, device="cuda")
    logp = torch.log_softmax(torch.randn((n, 10), generator=gen), dim=1).cuda()
    cols = (torch.arange(n) % 10).to(torch.int32).cuda()
    targets = torch.full((n,), int(0.1 * H * W + 0.5), dtype=torch.int32).cuda()
    seed, rewards = torch.empty((n, 10), device="cuda"), torch.empty((4, n), device="cuda")
    px, E = float(n * H * W), float(n * 3 * H * W)

    def step():                                                 # (in place on a copy: the masks drift, the work does not change)
        K.extremal_step(pm, mom, mask, dmask, stats, STEP, SIGMA, 0.01, 0.9, False)

    K.extremal_mask(pm, mask, STEP, SIGMA, stats)
    kernels = (
        ("extremal_mask [%d, 224, 224] with statistics" % n, lambda: K.extremal_mask(p0, mask, STEP, SIGMA, stats), 4.0 * (3 * px + n * hm * wm)),
        ("extremal_blend [%d, 3, 224, 224]" % n, lambda: K.extremal_blend(pyr, mask, buf, "preserve", False), 4.0 * (px + E + 2 * E)),
        ("extremal_seed [%d, 10]" % n, lambda: K.extremal_seed(logp, cols, seed, rewards, 0, "preserve"), 4.0 * (2 * n * 10 + 2 * n)),
        ("saliency_ranks [%d, 224, 224]" % n, lambda: K.saliency_ranks(mask.view(n, H * W), out=ranks), 8.0 * px),
        ("extremal_mask_grad [%d, 224, 224]" % n, lambda: K.extremal_mask_grad(pyr, mask, dx, ranks, targets, dmask, 300.0, "preserve", False),
         4.0 * (3 * px + E + 2 * E)),
        ("extremal_step [%d, %d, %d]" % (n, hm, wm), step, 4.0 * (4 * px + 4 * n * hm * wm)))
    total = 0.0
    for name, fn, nbytes in kernels:
        fn()
        ts = [window(fn, 0.25) * 1e3 for _ in range(a.repeats)]
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        total += min(ts)
        if nbytes < 1e5:                                        # a launch, not a stream: a byte floor would be noise
            say("%s: us %s | %.0f bytes" % (name, " ".join("%.1f" % t for t in ts), nbytes))
            continue
        say("%s: us %s | %.2f MB, floor %.2f us at %.1f TB/s, best / floor = %.2f"
            % (name, " ".join("%.1f" % t for t in ts), nbytes / 1e6, floor, a.hbm_tbs, min(ts) / floor))

    def hip_side():
        for _, fn, _ in kernels:
            fn()

    # ---- the same six steps with eager torch ops
    kern, cell = eager_tables()
    leaf = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([leaf], lr=0.01, momentum=0.9, dampening=0.9)
    A = int(targets[0])
    template = torch.cat([torch.zeros(H * W - A), torch.ones(A)]).cuda()
    rows = torch.arange(n, device="cuda")

    def eager_side():
        v = kern * leaf.flatten(1)[:, cell]
        w = torch.softmax(BETA * v.flatten(3), dim=3).view_as(v)
        mk = (v * w).sum((3, 4))
        t = mk * (LEVELS - 1)
        k = torch.clamp(torch.floor(t), 0, LEVELS - 2).detach()
        wt = (t - k)[:, None]
        idx = k.long()[:, None, None].expand(n, 1, 3, H, W)
        lv = pyr.unsqueeze(0).expand(n, LEVELS, 3, H, W)
        xt = (1.0 - wt) * torch.gather(lv, 1, idx).squeeze(1) + wt * torch.gather(lv, 1, idx + 1).squeeze(1)
        prob = torch.exp(logp[rows, cols.long()])
        sd = torch.zeros_like(logp)
        sd[rows, cols.long()] = -prob
        area = ((torch.sort(mk.flatten(1), dim=1).values - template) ** 2).mean(1)
        opt.zero_grad(set_to_none=True)
        ((xt * dx).sum() + 300.0 * area.sum()).backward()
        opt.step()
        with torch.no_grad():
            leaf.clamp_(0.0, 1.0)
        return sd

    hip_side(); eager_side()
    t_hip = [window(hip_side, 0.25) * 1e3 for _ in range(a.repeats)]
    t_eager = [window(eager_side, 0.25) * 1e3 for _ in range(a.repeats)]
    say("the six mask-side steps in sequence, %d masks: HIP us %s (sum of the single best times %.1f) | eager torch us %s | eager / HIP "
        "= %.1f" % (n, " ".join("%.1f" % t for t in t_hip), total, " ".join("%.1f" % t for t in t_eager), min(t_eager) / min(t_hip)))
    for model, per_it in iteration_ms.items():
        say("%s: the mask-side kernels are %.1f %% of an iteration (%.1f us of %.1f)"
            % (model, 100.0 * min(t_hip) / (1e3 * per_it), min(t_hip), 1e3 * per_it))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
