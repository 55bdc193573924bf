"""Extremal perturbation without a device: the definition of tools/attribution.py extremal_perturbation restated in torch, in the
gather formulation (every pixel reads the cells of its window), for any dtype -- float64 is the reference
tests/test_extremal_gpu.py holds the HIP kernels against, float32 on the CPU its parity yardstick -- and that restatement checked
against itself: the hand derivatives against fp64 autograd of the restated forward and against central differences, the mask's
range, the ends of the blend, the area term against TorchRay's sorted form, the pyramid's pass plan, the lambda schedule, the
momentum rule against torch.optim.SGD, and every refusal of the Python surface that needs no device."""
import math

import numpy as np
import pytest
import torch

from scouter_amd import kernels as K                                        # noqa: E402
from scouter_amd.tools.attribution import extremal_schedule                 # noqa: E402

BETA = 20.0                                                                 # restated, and held to the library's own below
assert K.EXTREMAL_BETA == BETA


# ------------------------------------------------------------------------------------------------ the restatement
def geometry(H, W, s, sigma):
    """(hm, wm, r): the coarse grid and the window's radius in cells, restated; the library's grid must be the same"""
    g = -(-H // s), -(-W // s), 1 + math.ceil(sigma / s)
    assert K.extremal_grid(H, W, s, sigma) == g
    return g


def window(H, W, s, sigma, dtype=torch.float64):
    """the gather tables of the upsampler: kern [H, W, D, D] = k(|u - centre| / sigma), cell [H, W, D, D] = the flat index of the
    cell (clamped into the grid) and inside [H, W, D, D] = whether the cell lies in the grid"""
    hm, wm, r = geometry(H, W, s, sigma)
    a = torch.arange(-r, r + 1)
    ci, cj = (torch.arange(H) // s)[:, None] + a, (torch.arange(W) // s)[:, None] + a                 # [H, D], [W, D]
    dy = torch.arange(H, dtype=dtype)[:, None] - ((ci.to(dtype) + 0.5) * s - 0.5)
    dx = torch.arange(W, dtype=dtype)[:, None] - ((cj.to(dtype) + 0.5) * s - 0.5)
    z = torch.sqrt(dy[:, None, :, None] ** 2 + dx[None, :, None, :] ** 2) / sigma
    kern = torch.exp(-2.0 * torch.clamp(z - 0.5, min=0.0) ** 2)
    inside = ((ci >= 0) & (ci < hm))[:, None, :, None] & ((cj >= 0) & (cj < wm))[None, :, None, :]
    cell = ci.clamp(0, hm - 1)[:, None, :, None] * wm + cj.clamp(0, wm - 1)[None, :, None, :]
    return kern, cell, inside


def smooth_mask(p, win):
    """p [n, hm, wm] -> (m [n, H, W], v, w [n, H, W, D, D]): v = k p (0 outside the grid), w = softmax(BETA v), m = sum v w"""
    kern, cell, inside = win
    v = kern * p.flatten(1)[:, cell] * inside
    w = torch.softmax(BETA * v.flatten(3), dim=3).view_as(v)
    return (v * w).sum((3, 4)), v, w


def cell_gradient(dm, p, win):
    """g [n, hm, wm] = sum_u dm[u] d m(u) / d p_c with the hand derivative k w (1 + BETA (v - m(u)))"""
    kern, cell, inside = win
    m, v, w = smooth_mask(p, win)
    coef = dm[..., None, None] * kern * w * (1.0 + BETA * (v - m[..., None, None])) * inside
    g = torch.zeros_like(p).flatten(1)
    return g.index_add_(1, cell.flatten(), coef.flatten(1)).view_as(p)


def knots(m, L, variant):
    """(k int64, w): the piece of the pyramid m selects and the position inside it; the right-hand piece at an interior knot"""
    t = (1.0 - m if variant == "delete" else m) * (L - 1)
    k = torch.clamp(torch.floor(t), 0, L - 2)
    return k.long(), t - k


def blend(P, m, variant):
    """P [L, C, H, W], m [n, H, W] -> (x~ [n, C, H, W], d x~ / d m): (1 - w) P[k] + w P[k + 1] and +-(L - 1) (P[k + 1] - P[k])"""
    L, n = P.shape[0], m.shape[0]
    k, w = knots(m, L, variant)
    Pn = P.unsqueeze(0).expand((n,) + tuple(P.shape))
    idx = k[:, None, None].expand(n, 1, *P.shape[1:])
    p0, p1 = torch.gather(Pn, 1, idx).squeeze(1), torch.gather(Pn, 1, idx + 1).squeeze(1)
    w = w[:, None]
    return (1.0 - w) * p0 + w * p1, (-(L - 1.0) if variant == "delete" else (L - 1.0)) * (p1 - p0)


def area_template(m, A):
    """tau [n, H, W]: 1 for the A pixels ranked first, most salient first and ties by ascending index"""
    order = torch.argsort(-m.flatten(1), dim=1, stable=True)
    return torch.zeros_like(m).flatten(1).scatter_(1, order[:, :A], 1.0).view_as(m)


def fp32(v):
    """a Python float rounded to fp32: the scalars reach the kernels as fp32"""
    return float(np.float32(v))


def schedule(n_iters, area_weight=300.0, area_growth=1.0035):
    """lambda_it, restated; the tool's own schedule must be these very floats"""
    lams = [area_weight * area_growth ** it for it in range(n_iters)]
    assert lams == extremal_schedule(n_iters, area_weight, area_growth)
    return lams


def mask_gradient(P, m, dx, A, lam, variant, flip):
    """d (loss + lam mean (m - tau)^2) / d m for dx = d loss / d (the image handed to the model)"""
    _, slope = blend(P, m, variant)
    g = dx.flip(-1) if flip else dx
    return (slope * g).sum(1) + (2.0 * lam / m[0].numel()) * (m - area_template(m, A))


def momentum_step(p, buf, g, lr, mu, first):
    """SGD with momentum mu and dampening mu, then the clamp -> (p, buf)"""
    buf = g if first else mu * buf + (1.0 - mu) * g
    return torch.clamp(p - lr * buf, 0.0, 1.0), buf


def run(box, P, p0, cols, A, n_iters, win, variant="preserve", lr=0.01, mu=0.9, jitter=True, area_weight=300.0,
        area_growth=1.0035):
    """the whole loop in the dtype of p0: -> (pmasks [n_iters + 1, n, hm, wm] before every iteration and at the end, rewards
    [n_iters, n], rank gaps and knot distances [n_iters] of the masks the iterations saw).  `box` maps [n, C, H, W] to
    log-probabilities; lr, mu and every lambda enter as their fp32 roundings."""
    dt, n, L = p0.dtype, p0.shape[0], P.shape[0]
    lr, mu, lams = fp32(lr), fp32(mu), [fp32(v) for v in schedule(n_iters, area_weight, area_growth)]
    p, buf, trail, rewards, gaps, dists = p0.clone(), None, [p0.clone()], [], [], []
    for it in range(n_iters):
        m, _, _ = smooth_mask(p, win)
        flip = jitter and it % 2 == 1
        xt, _ = blend(P, m, variant)
        leaf = (xt.flip(-1) if flip else xt).detach().requires_grad_(True)
        prob = torch.exp(box(leaf)[torch.arange(n), cols])
        dx = torch.autograd.grad((prob if variant == "delete" else -prob).sum(), leaf)[0]
        dm = mask_gradient(P, m, dx, A, lams[it], variant, flip)
        p, buf = momentum_step(p, buf, cell_gradient(dm, p, win), lr, mu, it == 0)
        srt = torch.sort(m.flatten(1), dim=1, descending=True).values
        t = (1.0 - m if variant == "delete" else m) * (L - 1)
        near = (t - torch.round(t)).abs()[(torch.round(t) >= 1) & (torch.round(t) <= L - 2)]
        gaps.append(float((srt[:, A - 1] - srt[:, A]).min()))
        dists.append(float(near.min()) if near.numel() else 1.0)
        rewards.append(prob.detach().to(dt))
        trail.append(p.clone())
    return torch.stack(trail), torch.stack(rewards), gaps, dists


class LinearBox(torch.nn.Module):
    """log_softmax(W x + b): the small differentiable black box of the trajectories"""

    def __init__(self, Wt, b):
        super().__init__()
        self.W, self.b = torch.nn.Parameter(Wt.clone()), torch.nn.Parameter(b.clone())

    def forward(self, x):
        return torch.log_softmax(x.flatten(1) @ self.W.t() + self.b, dim=1)


def pyramid_restated(image, levels, max_blur):
    """the pyramid of perturbation_pyramid in the dtype of `image` [C, H, W]: its pass plan, its fp32 taps, zeros outside"""
    from scouter_amd.tools.attribution import gaussian_taps, pyramid_pass_plan
    out = [image]
    for passes, sd, klen in reversed(pyramid_pass_plan(levels, max_blur)):
        taps, x = gaussian_taps(klen, sd).to(image.dtype), out[0]
        for _ in range(passes):
            x = torch.nn.functional.conv2d(x[:, None], taps.view(1, 1, 1, -1), padding=(0, klen // 2))
            x = torch.nn.functional.conv2d(x, taps.view(1, 1, -1, 1), padding=(klen // 2, 0))[:, 0]
        out.insert(0, x)
    return torch.stack(out)


def trajectory_case(variant, seed=1):
    """the short trajectories of tests/test_extremal_gpu.py: (13, 10, 4, 6), L = 3, areas (0.3,), two masks, a linear box of three
    outputs, a random uniform init -- everything fp32-representable and held in fp64.  The seed is pinned: of the seeds 0 .. 15
    it is the one whose fp64 run keeps, over all six iterations and for both variants, the gap between the A-th and (A + 1)-th
    largest mask value above 1e-4 (1.17e-4 preserve, 1.21e-4 delete) and every t more than 1e-4 from an interior knot (4.6e-4,
    6.4e-4); the fp32 restatement drifts 4.3e-7 / 3.6e-7 from it, and 12 of the 24 cells end clamped."""
    H, W, s, sigma, C, L = 13, 10, 4, 6.0, 2, 3
    gen = torch.Generator().manual_seed(seed)
    image = torch.randn((C, H, W), generator=gen).float().double()
    Wt = (torch.randn((3, C * H * W), generator=gen) * 0.15).float().double()
    b = torch.randn((3,), generator=gen).float().double()
    hm, wm, _ = geometry(H, W, s, sigma)
    p0 = torch.rand((2, hm, wm), generator=gen).float().double()
    return dict(H=H, W=W, s=s, sigma=sigma, C=C, L=L, max_blur=3.0, image=image, W_box=Wt, b_box=b, p0=p0, cols=[2, 0], area=0.3,
                A=int(math.floor(0.3 * H * W + 0.5)), n_iters=6, variant=variant)


def run_trajectory(case, dtype):
    win = window(case["H"], case["W"], case["s"], case["sigma"], dtype)
    P = pyramid_restated(case["image"].to(dtype), case["L"], case["max_blur"])
    box = LinearBox(case["W_box"].to(dtype), case["b_box"].to(dtype))
    return run(box, P, case["p0"].to(dtype), torch.tensor(case["cols"]), case["A"], case["n_iters"], win, case["variant"])


def patch_case():
    """a box whose evidence for class 1 sits in one patch: two outputs, logit 1 = 6 (mean of the patch) - 3, on an image that is 1
    inside the patch and 0 outside -- (16, 16, 4, 4), L = 3, the patch rows 4..7 and columns 8..11; twelve iterations at lr 0.05
    with the area weight 3 (at 300 the area term alone decides the first ranking of the constant initial mask, by index).  The fp64
    restatement ends with the mask's mean inside the patch 0.41 above its mean outside."""
    H, W = 16, 16
    image = torch.zeros((1, H, W), dtype=torch.float64)
    image[0, 4:8, 8:12] = 1.0
    Wt = torch.zeros((2, H * W), dtype=torch.float64)
    Wt.view(2, H, W)[1, 4:8, 8:12] = 6.0 / 16
    inside = torch.zeros((H, W), dtype=torch.bool)
    inside[4:8, 8:12] = True
    return dict(H=H, W=W, s=4, sigma=4.0, L=3, max_blur=4.0, image=image, W_box=Wt, b_box=torch.tensor([0.0, -3.0], dtype=torch.float64),
                inside=inside, area=0.1, n_iters=12, lr=0.05, area_weight=3.0)


def patch_margin(masks, inside):
    """the mask's mean inside the patch minus its mean outside"""
    return float(masks[..., inside].mean() - masks[..., ~inside].mean())


def run_patch(case, dtype=torch.float64):
    win = window(case["H"], case["W"], case["s"], case["sigma"], dtype)
    P = pyramid_restated(case["image"].to(dtype), case["L"], case["max_blur"])
    box = LinearBox(case["W_box"].to(dtype), case["b_box"].to(dtype))
    hm, wm, _ = geometry(case["H"], case["W"], case["s"], case["sigma"])
    A = int(math.floor(case["area"] * case["H"] * case["W"] + 0.5))
    trail, rewards, _, _ = run(box, P, torch.full((1, hm, wm), 0.5, dtype=dtype), torch.tensor([1]), A, case["n_iters"], win,
                               "preserve", lr=case["lr"], area_weight=case["area_weight"])
    return smooth_mask(trail[-1], win)[0], rewards


# ------------------------------------------------------------------------------------------------ the restatement against itself
SHAPES = [(13, 10, 4, 6.0), (16, 16, 4, 4.0), (9, 7, 7, 21.0)]


def random_p(H, W, s, sigma, n, seed):
    hm, wm, _ = geometry(H, W, s, sigma)
    return torch.rand((n, hm, wm), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("H,W,s,sigma", SHAPES)
def test_the_mask_stays_in_the_unit_interval(H, W, s, sigma):
    win = window(H, W, s, sigma)
    p = random_p(H, W, s, sigma, 3, 1)
    p[1], p[2] = 0.0, 1.0
    m, v, w = smooth_mask(p, win)
    assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0
    assert float(m[1].abs().max()) == 0.0 and float(m[2].max()) > 0.9                       # all zeros; a smooth maximum near 1
    assert torch.allclose(w.sum((3, 4)), torch.ones_like(m), atol=1e-12)


@pytest.mark.parametrize("H,W,s,sigma", SHAPES)
def test_the_hand_derivative_of_the_mask(H, W, s, sigma):
    """against fp64 autograd of the restated forward, and against central differences"""
    win = window(H, W, s, sigma)
    p = random_p(H, W, s, sigma, 2, 2)
    dm = torch.randn((2, H, W), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    hand = cell_gradient(dm, p, win)
    leaf = p.clone().requires_grad_(True)
    auto = torch.autograd.grad((smooth_mask(leaf, win)[0] * dm).sum(), leaf)[0]
    assert float((hand - auto).abs().max()) <= 1e-12 * float(auto.abs().max())
    h = 1e-6
    for c in range(p[0].numel()):
        e = torch.zeros_like(p).flatten(1)
        e[:, c] = h
        e = e.view_as(p)
        cd = ((smooth_mask(p + e, win)[0] - smooth_mask(p - e, win)[0]) * dm).sum((1, 2)) / (2 * h)
        assert float((cd - hand.flatten(1)[:, c]).abs().max()) <= 1e-6 * max(1.0, float(hand.abs().max()))


@pytest.mark.parametrize("variant", ["preserve", "delete"])
@pytest.mark.parametrize("L", [3, 5, 8])
def test_the_blend_and_its_derivative(L, variant):
    gen = torch.Generator().manual_seed(10 + L)
    P = torch.randn((L, 2, 5, 6), generator=gen, dtype=torch.float64)
    one = torch.ones((1, 5, 6), dtype=torch.float64)
    keep = one if variant == "preserve" else 1.0 - one                                      # m' = 1
    assert torch.equal(blend(P, keep, variant)[0][0], P[L - 1])                             # the image exactly
    assert torch.equal(blend(P, 1.0 - keep, variant)[0][0], P[0])                           # level 0 exactly
    m = torch.rand((3, 5, 6), generator=gen, dtype=torch.float64)
    t = (1.0 - m if variant == "delete" else m) * (L - 1)
    assert float((t - torch.round(t)).abs().min()) > 1e-4                                   # away from the knots
    leaf = m.clone().requires_grad_(True)
    probe = torch.randn((3, 2, 5, 6), generator=gen, dtype=torch.float64)
    auto = torch.autograd.grad((blend(P, leaf, variant)[0] * probe).sum(), leaf)[0]
    hand = (blend(P, m, variant)[1] * probe).sum(1)
    assert float((hand - auto).abs().max()) <= 1e-12 * float(auto.abs().max())
    h = 1e-6
    cd = ((blend(P, m + h, variant)[0] - blend(P, m - h, variant)[0]) * probe).sum(1) / (2 * h)
    assert float((cd - hand).abs().max()) <= 1e-7 * float(hand.abs().max())
    # on an interior knot j the value is level j and the slope is the piece [j, j + 1]'s; at m' = 1 the last piece's (L = 3 and
    # L = 5 have exactly representable knots, j / 7 is not one)
    for j in range(1, L if L in (3, 5) else 0):
        mp = torch.full((1, 5, 6), j / (L - 1.0), dtype=torch.float64)
        at = mp if variant == "preserve" else 1.0 - mp
        x, slope = blend(P, at, variant)
        assert float((x[0] - P[j]).abs().max()) <= 1e-14 * float(P.abs().max())
        lo = min(j, L - 2)
        assert torch.allclose(slope[0], (-(L - 1.0) if variant == "delete" else (L - 1.0)) * (P[lo + 1] - P[lo]), atol=1e-14)


def test_the_area_term_is_torchrays_sorted_form():
    """mean (m - tau)^2 with tau = 1 on the A first-ranked pixels equals |sort(m) - template|^2 / (H W), ties or not; the ties of a
    constant mask go to the lowest indices"""
    gen = torch.Generator().manual_seed(20)
    m = torch.rand((3, 6, 7), generator=gen, dtype=torch.float64)
    m[1] = torch.round(m[1] * 4) / 4                                                        # many ties
    m[2] = 0.5
    for A in (1, 13, 41):
        tau = area_template(m, A)
        assert bool((tau.sum((1, 2)) == A).all())
        template = torch.cat([torch.zeros(42 - A, dtype=torch.float64), torch.ones(A, dtype=torch.float64)])
        want = ((torch.sort(m.flatten(1), dim=1).values - template) ** 2).sum(1)
        assert torch.allclose(((m - tau) ** 2).sum((1, 2)), want, rtol=1e-13, atol=0)
        assert torch.equal(tau[2].flatten(), (torch.arange(42) < A).double())
        leaf = m.clone().requires_grad_(True)                                               # its gradient is 2 (m - tau)
        sorted_form = ((torch.sort(leaf.flatten(1), dim=1).values - template) ** 2).sum()
        auto = torch.autograd.grad(sorted_form, leaf)[0]
        assert torch.allclose(auto[0], 2.0 * (m[0] - tau[0]), atol=1e-14)                   # (no ties in m[0])


@pytest.mark.parametrize("variant", ["preserve", "delete"])
def test_the_whole_gradient_against_autograd(variant):
    """d (loss + lambda area) / d pmask by the hand chain (mask_gradient, cell_gradient) equals fp64 autograd through the restated
    upsampler, blend, mirror, box and TorchRay's sorted area term"""
    case = trajectory_case(variant)
    win = window(case["H"], case["W"], case["s"], case["sigma"])
    P = pyramid_restated(case["image"], case["L"], case["max_blur"])
    box = LinearBox(case["W_box"], case["b_box"])
    cols, A, lam, HW = torch.tensor(case["cols"]), case["A"], 300.0, case["H"] * case["W"]
    template = torch.cat([torch.zeros(HW - A, dtype=torch.float64), torch.ones(A, dtype=torch.float64)])
    for flip in (False, True):
        leaf = case["p0"].clone().requires_grad_(True)
        m = smooth_mask(leaf, win)[0]
        x = blend(P, m, variant)[0]
        prob = torch.exp(box(x.flip(-1) if flip else x)[torch.arange(2), cols])
        area = ((torch.sort(m.flatten(1), dim=1).values - template) ** 2).sum(1) / HW
        auto = torch.autograd.grad(((prob if variant == "delete" else -prob) + lam * area).sum(), leaf)[0]
        m = m.detach()
        xin = blend(P, m, variant)[0]
        xin = (xin.flip(-1) if flip else xin).requires_grad_(True)
        pr = torch.exp(box(xin)[torch.arange(2), cols])
        dx = torch.autograd.grad((pr if variant == "delete" else -pr).sum(), xin)[0]
        hand = cell_gradient(mask_gradient(P, m, dx, A, lam, variant, flip), case["p0"], win)
        assert float((hand - auto).abs().max()) <= 1e-11 * float(auto.abs().max())


def test_the_momentum_rule_is_sgd_with_dampening():
    gen = torch.Generator().manual_seed(30)
    p = torch.rand((2, 4, 3), generator=gen, dtype=torch.float64)
    grads = [torch.randn((2, 4, 3), generator=gen, dtype=torch.float64) * 30 for _ in range(4)]
    leaf = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([leaf], lr=0.01, momentum=0.9, dampening=0.9)
    mine, buf = p.clone(), None
    for it, g in enumerate(grads):
        leaf.grad = g.clone()
        opt.step()
        with torch.no_grad():
            leaf.clamp_(0.0, 1.0)
        mine, buf = momentum_step(mine, buf, g, 0.01, 0.9, it == 0)
        assert torch.allclose(mine, leaf.detach(), rtol=0, atol=1e-15)
    assert bool((mine == 0).any()) and bool((mine == 1).any())                              # both ends of the clamp were met


# ------------------------------------------------------------------------------------------------ the Python surface
def test_the_pyramids_pass_plan():
    from scouter_amd.tools.attribution import pyramid_pass_plan
    for levels, max_blur in ((8, 20.0), (3, 4.0), (2, 5.0), (5, 33.0), (3, 3.0)):
        plan = pyramid_pass_plan(levels, max_blur)
        assert len(plan) == levels - 1
        var = 0.0
        for l in range(levels - 2, -1, -1):                                                 # downwards from the image
            passes, sd, klen = plan[l]
            assert passes >= 1 and 0.0 < sd <= 5.0 and klen == 2 * math.ceil(3 * sd) + 1 and klen <= 31 and klen % 2 == 1
            var += passes * sd * sd
            sigma_l = max_blur * (1.0 - l / (levels - 1.0))
            assert abs(var - sigma_l ** 2) <= 1e-12 * sigma_l ** 2
    assert sum(p[0] for p in pyramid_pass_plan(8, 20.0)) == 19
    for bad in ((1, 20.0), (0, 20.0), (8, 0.0), (8, -1.0), (8, float("inf"))):
        with pytest.raises(ValueError):
            pyramid_pass_plan(*bad)


def test_the_lambda_schedule():
    lams = extremal_schedule(800)
    assert len(lams) == 800 and lams[0] == 300.0 and lams == schedule(800)
    assert all(b > a for a, b in zip(lams, lams[1:]))
    assert abs(lams[799] - 300.0 * math.exp(799 * math.log(1.0035))) <= 1e-9 * lams[799]
    assert extremal_schedule(3, 2.0, 0.5) == [2.0, 1.0, 0.5]


def test_the_grid_is_the_restatements():
    for H, W, s, sigma in SHAPES + [(224, 224, 7, 21.0), (224, 224, 7, 21.5), (5, 5, 1, 0.5)]:
        assert K.extremal_grid(H, W, s, sigma) == geometry(H, W, s, sigma)
    assert K.EXTREMAL_BETA == BETA


def test_extremal_perturbation_refuses_bad_arguments():
    """every refusal comes before any kernel: a CPU module and CPU images reach none"""
    from scouter_amd.tools.attribution import extremal_maps, extremal_perturbation, perturbation_pyramid
    box = LinearBox(torch.zeros((3, 2 * 13 * 10)), torch.zeros(3))
    x = torch.zeros((1, 2, 13, 10))
    bad = [dict(variant="dual"), dict(variant=0), dict(n_iters=0), dict(n_iters=-3), dict(levels=1), dict(levels=0),
           dict(areas=()), dict(areas=(0.0,)), dict(areas=(1.0,)), dict(areas=(0.3, 0.999)), dict(areas=(0.003,)),
           dict(areas=(float("nan"),)), dict(areas=0.3), dict(step=0), dict(sigma=0.0), dict(sigma=-1.0), dict(batch=0),
           dict(lr=-0.1), dict(momentum=1.5), dict(max_blur=0.0),
           dict(init=torch.zeros((3, 3))), dict(init=torch.zeros((4, 3, 1))), dict(init=torch.zeros((1, 3, 2, 4, 3))),
           dict(init=torch.zeros((2, 3, 1, 4, 3))), dict(init=[[0.5] * 3] * 4)]
    for kw in bad:
        kwargs = dict(step=4, sigma=6.0, levels=3, max_blur=3.0, n_iters=2)
        kwargs.update(kw)
        with pytest.raises(ValueError):
            extremal_perturbation(box, x, **kwargs)
        with pytest.raises(ValueError):
            extremal_maps(box, x, **kwargs)
    with pytest.raises(IndexError):
        extremal_perturbation(box, x, classes=[3], step=4, sigma=6.0, levels=3)
    with pytest.raises(ValueError):
        extremal_perturbation(box, x, classes=torch.tensor([0, 1]), step=4, sigma=6.0, levels=3)
    with pytest.raises(ValueError):
        extremal_perturbation(box, x[0], step=4, sigma=6.0, levels=3)
    with pytest.raises(ValueError):
        perturbation_pyramid(x)
    assert box.training                                                                     # no refusal left the box in eval mode


def test_the_kernel_wrappers_refuse_the_host():
    """no CPU fall-back: host tensors raise before the library is asked for anything"""
    p, m = torch.zeros((1, 4, 3)), torch.zeros((1, 13, 10))
    with pytest.raises(RuntimeError):
        K.extremal_mask(p, m, 4, 6.0)
    with pytest.raises(RuntimeError):
        K.extremal_blend(torch.zeros((3, 2, 13, 10)), m, torch.zeros((1, 2, 13, 10)))
    with pytest.raises(ValueError):
        K.extremal_blend(torch.zeros((3, 2, 13, 10)), m, torch.zeros((1, 2, 13, 10)), variant="dual")
    with pytest.raises(RuntimeError):
        K.extremal_step(p, p.clone(), m, m.clone(), torch.zeros((1, 13, 10, 2)), 4, 6.0, 0.01, 0.9, True)


def test_the_trajectory_cases_meet_their_conditions():
    """the two conditions tests/test_extremal_gpu.py asserts on the fp64 run, here without a device, and the fp32 drift"""
    for variant in ("preserve", "delete"):
        case = trajectory_case(variant)
        t64, r64, gaps, dists = run_trajectory(case, torch.float64)
        t32, r32, _, _ = run_trajectory(case, torch.float32)
        drift = float((t32.double() - t64).abs().max())
        clamped = int(((t64[-1] == 0) | (t64[-1] == 1)).sum())
        print("%s: rank gap %.3e, knot distance %.3e, fp32-vs-fp64 drift %.3e, clamped cells %d of %d"
              % (variant, min(gaps), min(dists), drift, clamped, t64[-1].numel()))
        assert min(gaps) >= 1e-4 and min(dists) >= 1e-4
        assert float((t64[-1] - t64[0]).abs().max()) > 0.01                                 # the masks moved


def test_the_patch_box_shows_its_margin():
    case = patch_case()
    masks, rewards = run_patch(case)
    margin = patch_margin(masks, case["inside"])
    print("patch margin %.4f, reward %.4f -> %.4f" % (margin, float(rewards[0, 0]), float(rewards[-1, 0])))
    assert margin >= 0.1
