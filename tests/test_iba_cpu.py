"""Information-bottleneck attribution without a device: the definition of tools/attribution.py information_bottleneck restated in
torch for any dtype -- float64 is the reference tests/test_iba_gpu.py holds the HIP kernels against, float32 on the CPU its parity
yardstick -- and that restatement checked against itself and against the reference program: the window, the reflecting index map
and its adjoint (as the exact transpose, and in the mirrored-sources form the kernel gathers by), kappa + lambda = 1, the analytic
gradient against fp64 autograd of the restated forward, Adam against torch.optim.Adam, Welford against the two-pass moments, the
reference's own IBA class on a tiny CPU network by the parity rule, and every refusal of the Python surface that needs no device.

Features are NHWC; the restatement flattens the positions: x, m, s, a [N, C], alpha [K, N, C], eps and z [K, S, N, C], N = h w."""
import inspect
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from scouter_amd import kernels as K                                        # noqa: E402
from scouter_amd.tools import attribution as A                              # noqa: E402

from oracle.ref_import import REFERENCE_ROOT as REFERENCE                 # noqa: E402
LN2 = math.log(2.0)
# the reference's fp32 error against the fp64 restatement over the fp32 restatement's: measured 8.35 in test_the_reference_program_
# agrees (7.9e-6 against 9.5e-7 bits on capacities up to 9.8 bits: the reference forms kappa as fp32 1 - lambda, whose rounding at
# lambda = sigmoid(5) is a relative 1e-5 of kappa, the restatement does not); twice that, as DESIGN.md records
K_REFERENCE = 16.7


# ------------------------------------------------------------------------------------------------ the restatement
def radius(sigma):
    r = 0 if not sigma else int(round(2.0 * float(np.float32(sigma))))
    assert K.iba_radius(sigma) == r
    return r


def window(sigma, dtype=torch.float64):
    """[D, D], D = 2 r + 1: exp(-d^2 / (2 sigma^2)) normalised to sum 1; the one value 1 without smoothing"""
    r = radius(sigma)
    if r == 0:
        return torch.ones((1, 1), dtype=dtype)
    d = torch.arange(-r, r + 1, dtype=torch.float64)
    g = torch.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(np.float32(sigma)) ** 2))
    return (g / g.sum()).to(dtype)


def reflect(i, n):
    """index i of an axis of n cells under reflection padding that does not repeat the edge"""
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def sources(c, n, r):
    """the adjoint of reflect: the padded indices in [-r, n - 1 + r] that land on cell c (the kernel's ib_sources)"""
    u = [c]
    if 0 < c <= r:
        u.append(-c)
    if c < n - 1 and n - 1 - c <= r:
        u.append(2 * (n - 1) - c)
    return u


def smoothing_matrix(h, w, sigma, dtype=torch.float64):
    """G [N, N]: (G v)[p] = sum_{a, b} win[a, b] v[reflect(y + a - r), reflect(x + b - r)]"""
    win, r = window(sigma, dtype), radius(sigma)
    assert r < h and r < w
    G = torch.zeros((h * w, h * w), dtype=dtype)
    for y in range(h):
        for x in range(w):
            for a in range(2 * r + 1):
                for b in range(2 * r + 1):
                    G[y * w + x, reflect(y + a - r, h) * w + reflect(x + b - r, w)] += win[a, b]
    return G


def adjoint_matrix(h, w, sigma, dtype=torch.float64):
    """G^T [N, N] built the way iba_step gathers it: cell p' collects win[a, b] g[u - (a - r)] over its padded sources u"""
    win, r = window(sigma, dtype), radius(sigma)
    T = torch.zeros((h * w, h * w), dtype=dtype)
    for y in range(h):
        for x in range(w):
            for uy in sources(y, h, r):
                for ux in sources(x, w, r):
                    for a in range(2 * r + 1):
                        for b in range(2 * r + 1):
                            oy, ox = uy - (a - r), ux - (b - r)
                            if 0 <= oy < h and 0 <= ox < w:
                                T[y * w + x, oy * w + ox] += win[a, b]
    return T


def masks(alpha, G):
    """alpha [K, N, C] -> (lambda, kappa) = (G sigmoid(alpha), G sigmoid(-alpha))"""
    return torch.einsum("pq,kqc->kpc", G, torch.sigmoid(alpha)), torch.einsum("pq,kqc->kpc", G, torch.sigmoid(-alpha))


def sample(x, m, s, a, lam, kap, eps, relu=False, min_std=0.01):
    """z [K, S, N, C] = a (lambda x + kappa (max(s, min_std) eps + m)), clamped at 0 with relu"""
    sd = torch.clamp(s, min=min_std)
    z = a * (lam[:, None] * x + kap[:, None] * (sd * eps + m))
    return torch.clamp(z, min=0.0) if relu else z


def capacity(x, m, s, a, lam, kap, min_std=0.01):
    """cap [K, N, C] in nats; exactly 0 where a = 0"""
    r = (x - m) / torch.clamp(s, min=min_std)
    cap = -0.5 * (1.0 + 2.0 * torch.log(kap) - r * r * lam * lam - kap * kap)
    return torch.where(a > 0, cap, torch.zeros_like(cap))


def mask_gradient(x, m, s, a, alpha, G, eps, dz, beta, relu=False, min_std=0.01):
    """G_alpha [K, N, C] for dz [K, S, N, C] = d loss / d z, the analytic form of the docstring"""
    lam, kap = masks(alpha, G)
    sd = torch.clamp(s, min=min_std)
    e = sd * eps + m
    t = dz * (x - e)
    if relu:
        t = t * (lam[:, None] * x + kap[:, None] * e > 0)
    r = (x - m) / sd
    gl = a * (t.sum(1) + beta / x.numel() * (1.0 / kap + r * r * lam - kap))
    sp = torch.sigmoid(alpha)
    return sp * torch.sigmoid(-alpha) * torch.einsum("qp,kqc->kpc", G, gl), gl


def adam_step(alpha, g, mm, vv, t, lr=1.0):
    """torch.optim.Adam at iteration t (from 0): betas (0.9, 0.999), eps 1e-8, no weight decay -> (alpha, m, v)"""
    mm = 0.9 * mm + 0.1 * g
    vv = 0.999 * vv + 0.001 * g * g
    step = lr / (1.0 - 0.9 ** (t + 1))
    return alpha - step * mm / (vv.sqrt() / math.sqrt(1.0 - 0.999 ** (t + 1)) + 1e-8), mm, vv


def welford(rows):
    """rows [n, ...] in order -> (mean, M2, nonzero), the streaming form"""
    mean, m2 = torch.zeros_like(rows[0]), torch.zeros_like(rows[0])
    nz = torch.zeros(rows[0].shape, dtype=torch.int64)
    for i, v in enumerate(rows):
        d = v - mean
        mean = mean + d / (i + 1)
        m2 = m2 + d * (v - mean)
        nz += v != 0
    return mean, m2, nz


def bits(cap):
    return cap.sum(-1) / LN2


class LinearHead:
    """log_softmax(flatten(z) W + b) on features [n, h, w, C]: the model of the trajectories, with the two passes
    information_bottleneck calls -- feature_pass (the `images` ARE the features, NCHW) and head_pass"""

    class Pass:
        def __init__(self, head, feat):
            self.features, self._head = feat, head
            self.log_probs = torch.log_softmax(head.mm(feat.flatten(1), head.W) + head.b, dim=1)

        def grad(self, seed):
            dlogits = seed - torch.exp(self.log_probs) * seed.sum(1, keepdim=True)
            return self._head.mm(dlogits, self._head.W.t()).view_as(self.features).contiguous()

    def __init__(self, W, b, rowwise=False):
        self.W, self.b, self.rowwise = W, b, rowwise

    def mm(self, a, b):
        """a b; rowwise: one product per row, so that a row's bits do not depend on the rows it came with"""
        return torch.cat([a[i:i + 1] @ b for i in range(a.shape[0])]) if self.rowwise else a @ b

    def feature_pass(self, images):
        return self.head_pass(images.permute(0, 2, 3, 1).contiguous())

    def head_pass(self, feat):
        return LinearHead.Pass(self, feat)

    def logp(self, z):
        return torch.log_softmax(z.flatten(1) @ self.W + self.b, dim=1)


def run_trajectory(x, m, s, a, h, w, cols, head_logp, noise, steps, S, beta=10.0, sigma=1.0, lr=1.0, relu=False, min_std=0.01,
                   dtype=torch.float64):
    """the loop of information_bottleneck for one image in `dtype`: x, m, s, a [N, C]; head_logp(z [rows, h, w, C]) -> log-probabilities
    (differentiated by autograd); noise(t) -> eps [K, S, N, C].  Returns (cap of the last forward [K, N, C], the alphas before
    every forward, the smallest |z| and the smallest active |G_alpha| met)"""
    x, m, s, a = (v.to(dtype) for v in (x, m, s, a))
    N, C = x.shape
    Kc = len(cols)
    G = smoothing_matrix(h, w, sigma, dtype)
    alpha = torch.full((Kc, N, C), 5.0, dtype=dtype)
    mm, vv = torch.zeros_like(alpha), torch.zeros_like(alpha)
    alphas, zmin, gmin = [], float("inf"), float("inf")
    for t in range(steps):
        alphas.append(alpha.clone())
        lam, kap = masks(alpha, G)
        if t == steps - 1:
            break
        eps = noise(t).to(dtype)
        z = sample(x, m, s, a, lam, kap, eps, relu, min_std).detach().requires_grad_(True)
        logp = head_logp(z.view(Kc * S, h, w, C))
        seed = torch.zeros_like(logp)
        seed[torch.arange(Kc * S), torch.tensor([c for c in cols for _ in range(S)])] = -1.0 / S
        dz = torch.autograd.grad(logp, z, seed)[0]
        g, _ = mask_gradient(x, m, s, a, alpha, G, eps, dz, beta, relu, min_std)
        zmin = min(zmin, float(z.detach()[:, :, a > 0].abs().min()))
        gmin = min(gmin, float(g[:, a > 0].abs().min()))
        alpha, mm, vv = adam_step(alpha, g, mm, vv, t, lr)
    return capacity(x, m, s, a, lam, kap, min_std), alphas, zmin, gmin


def feature_case(h, w, C, seed, inactive=(), relu=False):
    """fp32 x, m, s, a [N, C] of one image: the channels in `inactive` are always 0 (mean 0, std 0, activity 0)"""
    g = torch.Generator().manual_seed(seed)
    N = h * w
    m = torch.randn((N, C), generator=g)
    s = 0.5 + torch.rand((N, C), generator=g)
    x = m + s * torch.randn((N, C), generator=g)
    if relu:
        x, m = x.abs() + 0.05, m.abs()
    a = torch.ones((N, C))
    for c in inactive:
        x[:, c], m[:, c], s[:, c], a[:, c] = 0.0, 0.0, 0.0, 0.0
    return x, m, s, a


def trajectory_case():
    """a 4 x 5 x 6 feature tensor with one channel that never fires, a linear head of 4 outputs, two classes, three samples"""
    h, w, C, n_out = 4, 5, 6, 4
    x, m, s, a = feature_case(h, w, C, 60, inactive=(4,))
    g = torch.Generator().manual_seed(61)
    W = torch.randn((h * w * C, n_out), generator=g, dtype=torch.float64) * 0.3
    b = torch.randn((n_out,), generator=g, dtype=torch.float64)
    return dict(h=h, w=w, C=C, x=x, m=m, s=s, a=a, W=W, b=b, cols=[2, 0], S=3, steps=5, seed=77)


def patch_case():
    """class 1 of a linear head reads one cell alone, (1, 3) of a 5 x 5 x 8 grid: its evidence is planted there"""
    h, w, C = 5, 5, 8
    x, m, s, a = feature_case(h, w, C, 70)
    cell = 1 * w + 3
    W = torch.zeros((h * w, C, 3), dtype=torch.float64)
    W[cell, :, 1] = 2.0 * (x[cell] - m[cell]).double()
    return dict(h=h, w=w, C=C, x=x, m=m, s=s, a=a, W=W.view(h * w * C, 3), b=torch.zeros(3, dtype=torch.float64), cols=[1], S=4,
                steps=10, seed=78, cell=cell)


def patch_margin(m, case):
    """the map's value at the planted cell over its largest value outside that cell's 3 x 3 neighbourhood (the window spreads a
    mask over its neighbours); 0 when the map does not peak at the cell"""
    m = m.detach().double().cpu().flatten()
    if int(m.argmax()) != case["cell"]:
        return 0.0
    y, x = divmod(case["cell"], case["w"])
    far = [m[i * case["w"] + j] for i in range(case["h"]) for j in range(case["w"]) if abs(i - y) > 1 or abs(j - x) > 1]
    return float(m[case["cell"]] / max(far))


def cpu_noise(case, Kc):
    g = torch.Generator().manual_seed(case["seed"])
    draws = [torch.randn((Kc, case["S"], case["h"] * case["w"], case["C"]), generator=g, dtype=torch.float64)
             for _ in range(case["steps"])]
    return lambda t: draws[t]


def run_case(case, noise, steps=None, dtype=torch.float64, **kw):
    head = LinearHead(case["W"].to(dtype), case["b"].to(dtype))
    return run_trajectory(case["x"], case["m"], case["s"], case["a"], case["h"], case["w"], case["cols"], head.logp, noise,
                          steps or case["steps"], case["S"], dtype=dtype, **kw)


def test_the_restated_trajectory_moves_and_finds_the_patch():
    case = trajectory_case()
    cap, alphas, _, gmin = run_case(case, cpu_noise(case, 2))
    assert gmin >= 1e-4 and float((alphas[-1] - 5.0).abs().max()) > 2.0
    assert bool((alphas[-1][:, :, 4] == 5.0).all()) and bool((cap[:, :, 4] == 0).all()) and bool((cap >= 0).all())
    case = patch_case()
    cap, alphas, _, _ = run_case(case, cpu_noise(case, 1))
    assert patch_margin(bits(cap)[0], case) >= 1.5


# ------------------------------------------------------------------------------------------------ the window and its adjoint
@pytest.mark.parametrize("sigma,side", [(1.0, 5), (0.5, 3), (1.25, 5), (0.75, 5), (2.0, 9), (None, 1)])
def test_the_window(sigma, side):
    win = window(sigma)
    assert tuple(win.shape) == (side, side) and abs(float(win.sum()) - 1.0) < 1e-15
    assert torch.equal(win, win.t()) and torch.equal(win, win.flip(0))
    if sigma:
        r = side // 2
        assert abs(float(win[r, r] / win[r, r + 1]) - math.exp(1.0 / (2.0 * sigma * sigma))) < 1e-12


@pytest.mark.parametrize("h,w,sigma", [(3, 3, 1.0), (4, 5, 1.0), (7, 7, 1.0), (3, 4, 0.5), (9, 9, 2.0), (2, 2, None), (5, 3, 1.0)])
def test_the_adjoint_is_the_exact_transpose(h, w, sigma):
    """3 x 3 at radius 2 pads by dim - 1: every cell but the centre row is mirrored on both sides"""
    G, T = smoothing_matrix(h, w, sigma), adjoint_matrix(h, w, sigma)
    assert float((T - G.t()).abs().max()) < 1e-15
    assert float((G.sum(1) - 1.0).abs().max()) < 1e-14                      # every output's taps sum to 1
    # against ReflectionPad2d + a depthwise convolution, which is what the reference runs
    r = radius(sigma)
    v = torch.randn((1, 2, h, w), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = torch.nn.functional.conv2d(torch.nn.ReflectionPad2d(r)(v), window(sigma)[None, None].expand(2, 1, -1, -1), groups=2)
    got = torch.einsum("pq,cq->cp", G, v[0].flatten(1)).view(2, h, w)
    assert float((got - want[0]).abs().max()) < 1e-14


def test_sources_cover_every_padded_index_once():
    for n, r in ((3, 2), (4, 2), (7, 2), (5, 4), (2, 1), (9, 0)):
        seen = sorted(u for c in range(n) for u in sources(c, n, r))
        assert seen == list(range(-r, n + r)) and all(reflect(u, n) == c for c in range(n) for u in sources(c, n, r))


def test_kappa_and_lambda_sum_to_one():
    G = smoothing_matrix(4, 5, 1.0)
    alpha = torch.linspace(-30.0, 30.0, 20 * 3, dtype=torch.float64).view(1, 20, 3)
    lam, kap = masks(alpha, G)
    assert float((lam + kap - 1.0).abs().max()) < 1e-15
    # the point of forming kappa from sigmoid(-alpha): in fp32 at alpha = 17 the difference 1 - lambda is a multiple of 2^-24 next
    # to a true 4.1e-8 -- nothing of it is left -- and kappa is right to a few ulps
    a32 = torch.full((1, 20, 3), 17.0)
    lam32, kap32 = masks(a32, G.float())
    true = masks(a32.double(), G)[1]
    assert float(((1.0 - lam32).double() / true - 1.0).abs().min()) > 0.4
    assert float((kap32.double() / true - 1.0).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ gradient, Adam, Welford, bits
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("h,w,sigma", [(3, 3, 1.0), (4, 5, 1.0), (3, 2, None)])
def test_the_analytic_gradient_is_the_gradient(h, w, sigma, relu):
    C, Kc, S, beta = 3, 2, 3, 10.0
    x, m, s, a = (v.double() for v in feature_case(h, w, C, 5, inactive=(1,)))
    g = torch.Generator().manual_seed(6)
    alpha = (5.0 + torch.randn((Kc, h * w, C), generator=g, dtype=torch.float64)).requires_grad_(True)
    eps = torch.randn((Kc, S, h * w, C), generator=g, dtype=torch.float64)
    dz = torch.randn((Kc, S, h * w, C), generator=g, dtype=torch.float64)
    G = smoothing_matrix(h, w, sigma)
    lam, kap = masks(alpha, G)
    z = sample(x, m, s, a, lam, kap, eps, relu)
    loss = (dz * z).sum() + beta * capacity(x, m, s, a, lam, kap).mean((1, 2)).sum()
    want = torch.autograd.grad(loss, alpha)[0]
    got, gl = mask_gradient(x, m, s, a, alpha.detach(), G, eps, dz, beta, relu)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((got[:, :, 1] == 0).all()) and bool((gl[:, :, 1] == 0).all()) and bool((z[:, :, :, 1] == 0).all())


def test_adam_is_torch_adam():
    g = torch.Generator().manual_seed(8)
    p = torch.nn.Parameter(torch.full((4, 3), 5.0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1.0)
    alpha, mm, vv = p.detach().clone(), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    for t in range(5):
        grad = torch.randn((4, 3), generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        alpha, mm, vv = adam_step(alpha, grad, mm, vv, t)
        assert float((alpha - p.detach()).abs().max()) < 1e-13
    # a zero gradient from a zero state does not move alpha: 0 / (0 + eps)
    still, _, _ = adam_step(torch.full((2,), 5.0), torch.zeros(2), torch.zeros(2), torch.zeros(2), 0)
    assert bool((still == 5.0).all())


def test_welford_is_the_mean_and_variance():
    rows = torch.randn((37, 5, 4), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    rows[:, 0, 0] = 0.0
    rows[::2, 1, 1] = 0.0
    mean, m2, nz = welford(rows)
    assert float((mean - rows.mean(0)).abs().max()) < 1e-14
    assert float((torch.sqrt(m2 / 36) - rows.std(0)).abs().max()) < 1e-14
    assert int(nz[0, 0]) == 0 and int(nz[1, 1]) == 18 and int(nz[2, 2]) == 37


def test_bits():
    cap = torch.rand((2, 6, 5), dtype=torch.float64)
    assert float((bits(cap) * LN2 - cap.sum(2)).abs().max()) < 1e-14


# ------------------------------------------------------------------------------------------------ the reference program
def _load_reference_iba(monkeypatch):
    """the reference's torchcam/IBA/pytorch.py, with the two libraries it imports but this machine lacks stubbed"""
    import importlib.util
    base = os.path.join(REFERENCE, "torchcam", "IBA")
    skt = types.ModuleType("skimage.transform")
    skt.resize = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("skimage is a stub"))
    tvt = types.ModuleType("torchvision.transforms")
    tvt.Normalize = tvt.Compose = object
    pkgs = {"skimage": types.ModuleType("skimage"), "skimage.transform": skt, "torchvision": types.ModuleType("torchvision"),
            "torchvision.transforms": tvt, "torchcam": types.ModuleType("torchcam"), "torchcam.IBA": types.ModuleType("torchcam.IBA")}
    for name in ("skimage", "torchvision", "torchcam", "torchcam.IBA"):
        pkgs[name].__path__ = []
    for name, mod in pkgs.items():
        monkeypatch.setitem(sys.modules, name, mod)
    for name in ("utils", "pytorch"):
        spec = importlib.util.spec_from_file_location("torchcam.IBA." + name, os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        monkeypatch.setitem(sys.modules, "torchcam.IBA." + name, mod)
        spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_the_reference_program_agrees(monkeypatch):
    """The reference's IBA class on a tiny network, its estimator fed directly, three optimisation steps, mode="capacity", against
    the restatement under the same normal_() draws, by the parity rule: the reference (fp32) must be within K_REFERENCE times the
    fp32 restatement's error of the fp64 restatement, or within 1e-5."""
    ref = _load_reference_iba(monkeypatch)
    C, h, w, S, steps, target, n_out = 4, 4, 5, 3, 3, 2, 5
    torch.manual_seed(40)
    layer = torch.nn.Conv2d(2, C, 3, padding=1)
    fc = torch.nn.Linear(C * h * w, n_out)
    net = torch.nn.Sequential(layer, torch.nn.Flatten(), fc).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    iba = ref.IBA(layer, sigma=1.0, beta=10, optimization_steps=steps, batch_size=S)
    fit = torch.randn((50, 2, h, w))
    with torch.no_grad():
        iba.estimator(layer(fit))
    iba._build()
    image = torch.randn((1, 2, h, w))
    with torch.no_grad():
        feat = layer(image)[0]                                              # [C, h, w], before the hook's bottleneck
    import warnings
    torch.manual_seed(41)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cap_ref = iba.analyze(image, lambda b: -torch.log_softmax(net(b), dim=1)[:, target].mean(), mode="capacity")
    iba.detach()
    cap_ref = torch.from_numpy(np.asarray(cap_ref)).double().permute(1, 2, 0).reshape(h * w, C)       # bits, [N, C]

    torch.manual_seed(41)
    draws = [torch.empty((S, C, h, w)).normal_() for _ in range(steps)]
    nhwc = lambda v: v.permute(1, 2, 0).reshape(h * w, C)                   # noqa: E731
    x, m = nhwc(feat), nhwc(iba.estimator.mean())
    s, a = nhwc(iba.estimator.std()), nhwc(iba.estimator.active_neurons(0.01).float())
    assert bool((a == 1).all())

    def run(dtype):
        Wd, bd = fc.weight.to(dtype), fc.bias.to(dtype)
        head = lambda z: torch.log_softmax(z.permute(0, 3, 1, 2).flatten(1) @ Wd.t() + bd, dim=1)     # noqa: E731
        noise = lambda t: draws[t].permute(0, 2, 3, 1).reshape(1, S, h * w, C)                        # noqa: E731
        cap, alphas, _, _ = run_trajectory(x, m, s, a, h, w, [target], head, noise, steps, S, dtype=dtype)
        return cap[0].double() / LN2, alphas

    cap64, alphas = run(torch.float64)
    cap32, _ = run(torch.float32)
    assert float((alphas[-1] - 5.0).abs().max()) > 0.5                      # the masks moved
    err_ref, err_32 = float((cap_ref - cap64).abs().max()), float((cap32 - cap64).abs().max())
    print("reference fp32 error %.3e, restatement fp32 error %.3e, ratio %.2f; capacities up to %.2f bits"
          % (err_ref, err_32, err_ref / err_32, float(cap64.max())))
    assert err_ref <= max(K_REFERENCE * err_32, 1e-5)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_signatures():
    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(K.iba_sample)[:11] == ["x", "mean", "std", "active", "alpha", "z_out", "cap_out", "sigma", "seed", "t", "relu"]
    assert names(K.iba_step)[:14] == ["x", "mean", "std", "active", "alpha", "dz", "adam_m", "adam_v", "sigma", "seed", "t", "beta", "lr",
                                      "relu"]
    assert names(K.iba_estimate)[:2] == ["features", "state"] and names(K.iba_estimate_finish) == ["state", "threshold"]
    assert names(K.iba_bits)[0] == "cap"
    sig = inspect.signature(A.information_bottleneck)
    assert names(A.information_bottleneck) == ["model", "images", "estimate", "classes", "beta", "steps", "samples", "sigma", "lr",
                                               "min_std", "relu", "batch", "seed"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["classes"], d["beta"], d["steps"], d["samples"], d["sigma"], d["lr"], d["min_std"], d["relu"], d["batch"], d["seed"]) == \
        (None, 10.0, 10, 10, 1.0, 1.0, 0.01, False, None, 0)
    sig = inspect.signature(A.iba_estimate)
    assert names(A.iba_estimate) == ["model", "batches", "n_samples", "threshold"]
    assert (sig.parameters["n_samples"].default, sig.parameters["threshold"].default) == (5000, 0.01)
    assert A.IbaEstimate._fields == ("mean", "std", "active", "n")
    assert names(A.iba_saliency)[:4] == names(A.iba_maps)[:4] == ["model", "images", "estimate", "classes"]
    from scouter_amd.sloter.slot_model import SlotModel
    assert names(SlotModel.head_pass) == ["self", "features"]
    assert "iba          lambda im: information_bottleneck(model, im, estimate, classes=cs)" in A.sensitivity_max.__doc__
    assert [K.iba_radius(v) for v in (None, 0, 0.5, 0.75, 1.0, 1.25, 1.75, 2.0)] == [0, 0, 1, 2, 2, 2, 4, 4]


def test_refusals_before_any_launch():
    est = A.IbaEstimate(torch.zeros(3, 3, 8), torch.ones(3, 3, 8), torch.ones(3, 3, 8), 10)
    images = torch.zeros(1, 3, 96, 96)

    class NoModel:
        def __getattr__(self, name):
            raise AssertionError("the model was touched")

    for kw in (dict(steps=0), dict(samples=0), dict(batch=0), dict(sigma=1.5), dict(sigma=float("nan")), dict(sigma=-1.0)):
        with pytest.raises(ValueError):
            A.information_bottleneck(NoModel(), images, est, **kw)
    with pytest.raises(ValueError):                                        # 2 x 2 features: sigma = 1 needs more than its radius 2
        A.information_bottleneck(NoModel(), images, A.IbaEstimate(torch.zeros(2, 2, 8), torch.ones(2, 2, 8), torch.ones(2, 2, 8), 10))
    with pytest.raises(ValueError):                                        # an estimate whose parts disagree
        A.information_bottleneck(NoModel(), images, A.IbaEstimate(torch.zeros(3, 3, 8), torch.ones(3, 3, 4), torch.ones(3, 3, 8), 10))
    with pytest.raises(ValueError):
        A.information_bottleneck(NoModel(), images, (est.mean, est.std, est.active))
    with pytest.raises(ValueError):
        A.information_bottleneck(NoModel(), images[0], est)
    with pytest.raises(RuntimeError):                                      # CPU tensors
        A.information_bottleneck(NoModel(), images, est)
    with pytest.raises(ValueError):
        A.iba_estimate(NoModel(), [])
    # the wrappers refuse CPU tensors before the library is asked
    x, al = torch.zeros(3, 3, 8), torch.zeros(2, 3, 3, 8)
    z = torch.zeros(4, 3, 3, 8)
    with pytest.raises(RuntimeError):
        K.iba_sample(x, x, x, x, al, z, None, 1.0, 0, 0, False)
    with pytest.raises(RuntimeError):
        K.iba_step(x, x, x, x, al, z, al.clone(), al.clone(), 1.0, 0, 0, 10.0, 1.0, False)
    with pytest.raises(RuntimeError):
        K.iba_estimate(z)
    with pytest.raises(RuntimeError):
        K.iba_bits(al)
    with pytest.raises(RuntimeError):
        K.iba_estimate_finish(None)
    from scouter_amd.sloter.slot_model import SlotModel
    with pytest.raises(RuntimeError):
        SlotModel.head_pass(NoModel(), z)
