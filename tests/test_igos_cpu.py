"""I-GOS (tools/attribution.py igos, csrc/igos.hip) on the CPU: the float64 restatement of every definition in the docstring of
`igos` and in include/scouter_hip.h -- tests/test_igos_gpu.py holds the kernels and the tool to it -- with the noise taken as an
argument, and what needs no device: the analytic mask gradient against autograd, the step ladder, what `igos` and the kernel
wrappers refuse, the new flags of test.py.  No reference program is involved (the reference's I-GOS needs cv2 and skimage, and
its noise is host cv2.randn): the restatement is written from the definitions."""
import numpy as np
import pytest
import torch

from scouter_amd import kernels as K                                        # noqa: E402
from scouter_amd.tools.attribution import igos, igos_ladder                 # noqa: E402
from test_extremal_cpu import LinearBox, fp32, patch_case                   # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement
def source(n_in, n_out):
    """(i0, i1, t) of every destination index of an axis of n_in cells upsampled to n_out pixels, align_corners = True.  The
    coordinate is fp32 BY DEFINITION: scale = (float)(n_in - 1) / (float)(n_out - 1), s = (float)d * scale, i0 = min((int)s, n_in - 1),
    i1 = min(i0 + 1, n_in - 1), t = s - i0 (exact)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1)
    s = (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    t = (s - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(t)


def upsample_matrix(n_in, n_out, dtype=torch.float64):
    """M [n_out, n_in]: row d holds 1 - t at i0 and t at i1 (their sum where the two coincide)"""
    i0, i1, t = source(n_in, n_out)
    M = torch.zeros((n_out, n_in), dtype=torch.float64)
    rows = torch.arange(n_out)
    M.index_put_((rows, i0), 1.0 - t.double(), accumulate=True)
    M.index_put_((rows, i1), t.double(), accumulate=True)
    return M.to(dtype)


def upsample(p, H, W):
    """U(p): [..., hm, wm] -> [..., H, W]"""
    return upsample_matrix(p.shape[-2], H, p.dtype) @ p @ upsample_matrix(p.shape[-1], W, p.dtype).t()


def upsample_adjoint(a, hm, wm):
    """U^T(a): [..., H, W] -> [..., hm, wm]"""
    return upsample_matrix(hm, a.shape[-2], a.dtype).t() @ a @ upsample_matrix(wm, a.shape[-1], a.dtype)


def loss1(p, l1, tv, beta):
    """the regulariser of masks p [..., hm, wm] with l1 broadcast over the leading axes -> [...]"""
    rows = (p[..., :-1, :] - p[..., 1:, :]).abs().pow(beta).mean((-2, -1))
    cols = (p[..., :, :-1] - p[..., :, 1:]).abs().pow(beta).mean((-2, -1))
    return l1 * (1.0 - p).abs().mean((-2, -1)) + tv * (rows + cols)


def tv_slope(delta, beta):
    """d |delta|^beta / d delta, 0 at 0"""
    mag = torch.where(delta != 0, delta.abs(), torch.ones_like(delta)).pow(beta - 1.0) * beta
    return torch.where(delta != 0, mag * torch.sign(delta), torch.zeros_like(delta))


def loss1_gradient(p, l1, tv, beta):
    """d loss1 / d p by hand; l1 [R] for p [R, hm, wm]"""
    R, hm, wm = p.shape
    g = -torch.sign(1.0 - p) * l1.view(R, 1, 1) / (hm * wm)
    dr = tv_slope(p[:, :-1, :] - p[:, 1:, :], beta) * (tv / ((hm - 1) * wm))
    dc = tv_slope(p[:, :, :-1] - p[:, :, 1:], beta) * (tv / (hm * (wm - 1)))
    g[:, :-1, :] += dr
    g[:, 1:, :] -= dr
    g[:, :, :-1] += dc
    g[:, :, 1:] -= dc
    return g


def path_weights(S, dtype=torch.float64):
    """(a_j, w_j), j < S: the position (j + 1) / S and the weight a_j / S"""
    a = torch.arange(1, S + 1, dtype=torch.float64) / S
    return a.to(dtype), (a / S).to(dtype)


def path_images(image, base, p, S, sigma, z):
    """x[r, j] = base + a_j U(p_r) (image - base) + sigma z[j]: [R, S, C, H, W] for image / base [C, H, W], p [R, hm, wm], z [S, C, H, W]"""
    a, _ = path_weights(S, p.dtype)
    u = upsample(p, image.shape[-2], image.shape[-1])
    return base + a.view(1, S, 1, 1, 1) * u[:, None, None] * (image - base) + sigma * z[None]


def contraction(image, base, dx, S):
    """acc[r] = sum_j w_j sum_c dx[r, j, c] (image - base)[c] for dx [R, S, C, H, W]"""
    _, w = path_weights(S, dx.dtype)
    return (w.view(1, S, 1, 1) * (dx * (image - base)).sum(2)).sum(1)


def direction(box, image, base, p, cols, S, sigma, z, l1, tv, beta):
    """the analytic mask gradient of one iteration, as the tool forms it -> (g [R, hm, wm], acc [R, H, W])"""
    R = p.shape[0]
    leaf = path_images(image, base, p, S, sigma, z).detach().requires_grad_(True)
    prob = torch.exp(box(leaf.flatten(0, 1)).view(R, S, -1)[torch.arange(R), :, cols])
    dx = torch.autograd.grad(prob.sum(), leaf)[0]
    acc = contraction(image, base, dx, S)
    return upsample_adjoint(acc, p.shape[-2], p.shape[-1]) + loss1_gradient(p, l1, tv, beta), acc


def objective(box, image, base, p, cols, S, sigma, z, l1, tv, beta):
    """loss1(p_r) + (1 / S) sum_j prob(x[r, j]), summed over the rows"""
    R = p.shape[0]
    x = path_images(image, base, p, S, sigma, z)
    prob = torch.exp(box(x.flatten(0, 1)).view(R, S, -1)[torch.arange(R), :, cols])
    return (loss1(p, l1, tv, beta) + prob.sum(1) / S).sum()


def candidates(p, g, steps):
    """cand[r, k] = clamp(p_r - steps[k] g_r, 0, 1): [R, T1, hm, wm]"""
    return torch.clamp(p[:, None] - steps.view(1, -1, 1, 1) * g[:, None], 0.0, 1.0)


def select(tot, steps, sumsq, alpha):
    """per row the first k >= 1 with not (tot_k > tot_0 - alpha steps[k] sumsq), the last when none passes -> (chosen [R] as a
    list, the least |tot_k - thr_k| over the comparisons made)"""
    chosen, margin = [], float("inf")
    for r in range(tot.shape[0]):
        pick = tot.shape[1] - 1
        for k in range(1, tot.shape[1]):
            thr = float(tot[r, 0]) - alpha * float(steps[k]) * float(sumsq[r])
            margin = min(margin, abs(float(tot[r, k]) - thr))
            if not float(tot[r, k]) > thr:
                pick = k
                break
        chosen.append(pick)
    return chosen, margin


def adapt(l1, prob_now, prob_first, it, n_iters):
    """the mid-run adjustment of l1 [R], in place"""
    if n_iters <= 3:
        return
    moved = (prob_now - prob_first).abs()
    if it == n_iters // 2:
        l1[moved <= 1e-3] /= 10.0
    elif it == int(n_iters / 1.25):
        l1[moved <= 1e-2] /= 5.0


def run(box, image, base, p0, cols, n_iters, S, l1_coeff, tv, beta, sigma, noise, ladder, alpha=1e-4, adapt_l1=True):
    """the whole loop in the dtype of p0: noise [n_iters, S, C, H, W] -> (pmasks [n_iters + 1, R, hm, wm] before every iteration and
    at the end, curves [R, n_iters, 4], the least margin of the comparisons made, the chosen rungs [n_iters][R]).  The ladder, the
    coefficients and sigma enter as their fp32 roundings."""
    dt, R = p0.dtype, p0.shape[0]
    steps = torch.tensor([fp32(v) for v in ladder], dtype=dt)
    tv, beta, sigma = fp32(tv), fp32(beta), fp32(sigma)
    l1 = torch.full((R,), fp32(l1_coeff), dtype=dt)
    cols = torch.as_tensor(cols)
    p, trail, curves, margin, rungs = p0.clone(), [p0.clone()], torch.zeros((R, n_iters, 4), dtype=dt), float("inf"), []
    for it in range(n_iters):
        g, _ = direction(box, image, base, p, cols, S, sigma, noise[it].to(dt), l1, tv, beta)
        g = g.detach()
        cand = candidates(p, g, steps)
        with torch.no_grad():
            x = base + upsample(cand, image.shape[-2], image.shape[-1])[:, :, None] * (image - base)
            prob = torch.exp(box(x.flatten(0, 1)).view(R, len(ladder), -1)[torch.arange(R), :, cols])
        tot = loss1(cand, l1.view(R, 1), tv, beta) + prob
        chosen, m = select(tot, steps, (g * g).sum((1, 2)), alpha)
        margin = min(margin, m)
        curves[:, it, 0], curves[:, it, 1] = tot[:, 0] - prob[:, 0], prob[:, 0]
        curves[:, it, 2], curves[:, it, 3] = steps[chosen], torch.tensor(chosen, dtype=dt)
        p = cand[torch.arange(R), chosen].clone()
        if adapt_l1:
            adapt(l1, curves[:, it, 1], curves[:, 0, 1], it, n_iters)
        rungs.append(chosen)
        trail.append(p.clone())
    return torch.stack(trail), curves, margin, rungs


def trajectory_case():
    """the six-iteration trajectory of tests/test_igos_gpu.py: the 16 x 16 patch box of test_extremal_cpu.patch_case (two outputs,
    the evidence for class 1 in rows 4..7, columns 8..11), a zero baseline, a 4 x 4 mask that starts at 1, five path points,
    l1 0.05, tv 0.5 (at l1 0.1 / tv 1.0 the margins of the line search fall to 1e-9: not used)."""
    c = patch_case()
    return dict(H=16, W=16, hm=4, wm=4, image=c["image"], base=torch.zeros_like(c["image"]), W_box=c["W_box"], b_box=c["b_box"],
                inside=c["inside"], cols=[1], n_iters=6, S=5, l1=0.05, tv=0.5, beta=2.0, sigma=0.2, ladder=igos_ladder())


def run_trajectory(case, noise, dtype):
    box = LinearBox(case["W_box"].to(dtype), case["b_box"].to(dtype))
    p0 = torch.ones((len(case["cols"]), case["hm"], case["wm"]), dtype=dtype)
    return run(box, case["image"].to(dtype), case["base"].to(dtype), p0, case["cols"], case["n_iters"], case["S"], case["l1"],
               case["tv"], case["beta"], case["sigma"], noise, case["ladder"])


# ------------------------------------------------------------------------------------------------ the restatement against itself
SHAPES = [(16, 16, 4, 4), (13, 10, 3, 5), (9, 7, 2, 2)]


def random_case(H, W, hm, wm, seed, R=2, C=2, S=3, n_out=3):
    gen = torch.Generator().manual_seed(seed)
    image = torch.randn((C, H, W), generator=gen, dtype=torch.float64)
    base = torch.randn((C, H, W), generator=gen, dtype=torch.float64)
    box = LinearBox(torch.randn((n_out, C * H * W), generator=gen, dtype=torch.float64) * 0.2,
                    torch.randn((n_out,), generator=gen, dtype=torch.float64))
    p = torch.rand((R, hm, wm), generator=gen, dtype=torch.float64)
    p[0, 0, 0], p[R - 1, hm - 1, wm - 1] = 1.0, 0.0                        # cells on both clamps
    z = torch.randn((S, C, H, W), generator=gen, dtype=torch.float64)
    return image, base, box, p, z


@pytest.mark.parametrize("beta", [1.0, 2.0])
@pytest.mark.parametrize("H,W,hm,wm", SHAPES)
def test_the_analytic_mask_gradient_is_autograds(H, W, hm, wm, beta):
    """contraction, adjoint and the L1 / TV terms against torch autograd of the restated objective: 1e-12 relative"""
    image, base, box, p, z = random_case(H, W, hm, wm, 10 * H + hm)
    cols, l1 = torch.tensor([2, 0]), torch.tensor([0.7, 1.3], dtype=torch.float64)
    g, _ = direction(box, image, base, p, cols, 3, 0.2, z, l1, 2.5, beta)
    leaf = p.clone().requires_grad_(True)
    want = torch.autograd.grad(objective(box, image, base, leaf, cols, 3, 0.2, z, l1, 2.5, beta), leaf)[0]
    err = float((g - want).abs().max()) / float(want.abs().max())
    print("analytic mask gradient %dx%d <- %dx%d beta %g: relative error %.3e" % (H, W, hm, wm, beta, err))
    assert float(want.abs().max()) > 1e-3 and err <= 1e-12


@pytest.mark.parametrize("H,W,hm,wm", SHAPES + [(12, 8, 12, 8)])
def test_the_upsampler_is_torchs_and_its_adjoint_is_one(H, W, hm, wm):
    gen = torch.Generator().manual_seed(H + wm)
    p = torch.rand((2, hm, wm), generator=gen, dtype=torch.float64)
    a = torch.randn((2, H, W), generator=gen, dtype=torch.float64)
    want = torch.nn.functional.interpolate(p[None], size=(H, W), mode="bilinear", align_corners=True)[0]
    assert float((upsample(p, H, W) - want).abs().max()) <= 1e-6          # (the coordinate is fp32 by definition)
    lhs, rhs = float((upsample(p, H, W) * a).sum()), float((p * upsample_adjoint(a, hm, wm)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    ones = upsample(torch.ones((hm, wm), dtype=torch.float64), H, W)
    assert float((ones - 1.0).abs().max()) <= 1e-15
    if (hm, wm) == (H, W):
        assert torch.equal(upsample(p, H, W), p)


def test_the_selection_rule():
    steps = torch.tensor([0.0, 8.0, 4.0, 2.0], dtype=torch.float64)
    sumsq = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    nan = float("nan")
    tot = torch.tensor([[1.0, 0.5, 9.0, 9.0], [1.0, 2.0, 0.9, 9.0], [1.0, 2.0, 2.0, 2.0], [1.0, nan, 0.0, 0.0]], dtype=torch.float64)
    chosen, margin = select(tot, steps, sumsq, 1e-2)
    assert chosen == [1, 2, 3, 1]
    l1 = torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64)
    adapt(l1, torch.tensor([0.5, 0.5005, 0.6]), torch.tensor([0.5, 0.5, 0.5]), 7, 15)
    assert l1.tolist() == [0.1, 0.1, 1.0]
    adapt(l1, torch.tensor([0.5, 0.505, 0.52]), torch.tensor([0.5, 0.5, 0.5]), 12, 15)
    assert l1.tolist() == [0.1 / 5.0, 0.1 / 5.0, 1.0]
    adapt(l1, torch.tensor([0.5, 0.5, 0.5]), torch.tensor([0.5, 0.5, 0.5]), 1, 3)
    assert l1.tolist() == [0.1 / 5.0, 0.1 / 5.0, 1.0]


# ------------------------------------------------------------------------------------------------ the ladder, the refusals, the flags
def test_the_ladder():
    ladder = igos_ladder()
    assert len(ladder) == 13 and ladder[0] == 0.0 and ladder[1] == 200.0
    assert all(ladder[k + 1] == ladder[k] * 0.2 for k in range(1, 12))
    assert ladder[-2] >= 1e-5 > ladder[-1] > 0.0
    assert igos_ladder(1.0, 0.5, 0.3) == [0.0, 1.0, 0.5, 0.25]
    assert igos_ladder(1e-6, 0.5, 1e-5) == [0.0, 1e-6]                      # the first step is tried whatever its size
    for bad in ((0.0, 0.2, 1e-5), (-1.0, 0.2, 1e-5), (float("inf"), 0.2, 1e-5), (200.0, 0.0, 1e-5), (200.0, 1.0, 1e-5),
                (200.0, 1.5, 1e-5), (200.0, 0.2, 0.0), (200.0, float("nan"), 1e-5), (200.0, 0.99, 1e-5)):
        with pytest.raises(ValueError):
            igos_ladder(*bad)


def test_igos_refuses_bad_arguments():
    gen = torch.Generator().manual_seed(5)
    box = LinearBox(torch.randn((3, 2 * 13 * 10), generator=gen), torch.zeros(3))
    images = torch.randn((2, 2, 13, 10), generator=gen)
    bad = [dict(size=1), dict(size=(2,)), dict(size=(2, 3, 4)), dict(size=14), dict(size=(4, 11)), dict(size="x"), dict(n_iters=0),
           dict(n_steps=0), dict(l1_coeff=-1.0), dict(tv_coeff=float("inf")), dict(tv_beta=0.5), dict(tv_beta=100.0), dict(sigma=-0.1),
           dict(sigma=float("nan")), dict(alpha=-1.0), dict(batch=0), dict(step0=0.0), dict(shrink=1.0), dict(min_step=0.0),
           dict(blur_klen=33), dict(blur_klen=4), dict(blur_sigma=0.0), dict(baseline=torch.zeros((3, 13, 10))),
           dict(baseline=torch.zeros((1, 2, 13, 10))), dict(baseline=0.0), dict(init=torch.ones((3, 3))),
           dict(init=torch.ones((2, 2, 4, 4)), classes=[0]), dict(init=torch.ones((1, 1, 4, 4)), classes=[0]),
           dict(classes=torch.tensor([0, 1, 2]))]
    for kw in bad:
        with pytest.raises(ValueError):
            igos(box, images, **dict(dict(size=4), **kw))
            pytest.fail("%r was accepted" % (kw,))
    with pytest.raises(ValueError):
        igos(box, images[0], size=4)
    with pytest.raises(ValueError):
        igos(box, torch.zeros((1, 2, 1, 10)), size=2)
    with pytest.raises(ValueError):
        igos(box, torch.zeros((1, 1, 224, 224)), size=200)                  # 40000 cells: past the 16384 of the per-row kernels
    with pytest.raises(IndexError):
        igos(box, images, size=4, classes=[3])
    with pytest.raises(RuntimeError):                                       # every check passed: the host has no path
        igos(box, images, size=4, classes=[0])


def test_the_kernel_wrappers_refuse_the_host():
    z = torch.zeros
    image, p = z((2, 13, 10)), z((2, 3, 5))
    calls = [lambda: K.igos_upsample(p, z((2, 13, 10))),
             lambda: K.igos_path_images(image, image, p, z((4, 2, 13, 10)), 0, 2, 0.2, 0, 0),
             lambda: K.igos_accumulate(image, image, z((4, 2, 13, 10)), z((2, 13, 10), dtype=torch.float64), 0, 2),
             lambda: K.igos_mask_grad(p, z((2, 13, 10), dtype=torch.float64), z(2), z((2, 3, 5)), z((2, 2), dtype=torch.float64), 1.0, 2.0),
             lambda: K.igos_trial_images(image, image, p, p.clone(), z(3), z((6, 2, 13, 10)), 0),
             lambda: K.igos_step(p, p.clone(), z(3), z((6, 4)), z(2, dtype=torch.int32), z((2, 2), dtype=torch.float64), z(2),
                                 z((2, 5, 4), dtype=torch.float64), 0, 5, 1e-4, 1.0, 2.0, True)]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
            pytest.fail("call %d was accepted" % i)


def test_the_new_test_flags_parse():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.igos is False and a.igos_size == 8 and a.igos_iters == 15 and a.igos_steps == 20
    assert a.igos_l1 == 1.0 and a.igos_tv == 20.0 and a.igos_batch == 50
    # the older flags keep their defaults
    assert a.extremal is False and a.extremal_iters == 800 and a.iba is False and a.iba_steps == 10 and a.causal is False
    a = T.get_test_parser().parse_args(["--igos", "true", "--igos_size", "14", "--igos_iters", "3", "--igos_steps", "4", "--igos_l1",
                                        "0.5", "--igos_tv", "2.0", "--igos_batch", "7"])
    assert a.igos is True and (a.igos_size, a.igos_iters, a.igos_steps, a.igos_l1, a.igos_tv, a.igos_batch) == (14, 3, 4, 0.5, 2.0, 7)
    assert T._igos_kwargs(a) == dict(size=14, n_iters=3, n_steps=4, l1_coeff=0.5, tv_coeff=2.0, batch=7)
    assert callable(T.run_igos)
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--igos", "true"])


def test_the_trajectory_case_on_stand_in_noise():
    """the case of the GPU trajectory with torch.randn in place of the Philox stream: the line search keeps its margins, the fp32
    run follows the fp64 one, and the mask ends lower inside the patch than outside"""
    case = trajectory_case()
    noise = torch.randn((case["n_iters"], case["S"], 1, 16, 16), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    noise = noise.float().double()
    t64, c64, margin, rungs = run_trajectory(case, noise, torch.float64)
    t32, _, _, _ = run_trajectory(case, noise, torch.float32)
    T = len(case["ladder"]) - 1
    print("stand-in trajectory: margin %.3e, rungs %s, fp32 drift %.3e" % (margin, rungs, float((t32.double() - t64).abs().max())))
    assert margin >= 1e-4 and all(k < T for it in rungs for k in it)
    assert float((t32.double() - t64).abs().max()) <= 1e-5
    mask = upsample(t64[-1], 16, 16)[0]
    assert float(mask[case["inside"]].mean()) < float(mask[~case["inside"]].mean()) - 0.1
