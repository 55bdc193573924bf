"""Restatements of csrc/gradshap.hip's draws (NumPy, on the Philox restatement of tests/test_pathgrad_cpu.py) and of the two
GradientSHAP methods of tools/attribution.py (plain torch, in the dtype of their inputs: float64 for the references, float32 for the
yardstick of the project's rule), shared by tests/test_gradshap_cpu.py and tests/test_gradshap_gpu.py.  Everything runs on the host."""
import numpy as np
import torch

from test_pathgrad_cpu import MASK, philox4x32_10


# ------------------------------------------------------------------------------------------------ the draws
def draw_words(seed, first, n):
    """(r0, r1) uint64 [n] below 2^32: the first two Philox words of the counter (0, s, 2, 0) for s = first .. first + n - 1 under
    the key (seed mod 2^32, seed / 2^32)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = np.arange(first, first + n, dtype=np.uint64)
    r = philox4x32_10((0, s, 2, 0), (seed & MASK, seed >> 32))
    return r[0], r[1]


def draws(seed, first, n, R):
    """(picks int32 [n] = (r0 R) >> 32, alphas float32 [n] = (2 (r1 >> 9) + 1) 2^-24, exact) of the samples first .. first + n - 1"""
    r0, r1 = draw_words(seed, first, n)
    picks = ((r0 * np.uint64(R)) >> np.uint64(32)).astype(np.int32)         # (r0 < 2^32 and R < 2^31: no overflow in uint64)
    alphas = ((2.0 * (r1 >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)
    return picks, alphas


def shares(picks, R):
    """n_r / n, float64 [R]: the share of the samples that drew baseline r"""
    return torch.from_numpy(np.bincount(np.asarray(picks), minlength=R).astype(np.float64) / len(picks))


# ------------------------------------------------------------------------------------------------ the kernels
def accumulate(grads, diffs, acc0, inv_n):
    """grads, diffs [n, ...] (the rows' own differences), acc0 [...] -> (acc0 + sum_j grads[j] diffs[j] inv_n,
    |acc0| + sum_j |grads[j] diffs[j] inv_n|), float64"""
    t = grads.double() * diffs.double() * float(inv_n)
    return acc0.double() + t.sum(dim=0), acc0.double().abs() + t.abs().sum(dim=0)


# ------------------------------------------------------------------------------------------------ the methods
def gradient_shap(f, ends, bank, picks, alphas, cols, x=None):
    """f: rows [n, ...] -> outputs [n, classes], differentiable.  ends [n, ...]: the noisy copies x~_s (or x itself, repeated),
    bank [R, ...], picks / alphas [n] -> (attr [K, ...] = (1 / n) sum_s g_s d_s with d_s = ends[s] - bank[picks[s]] and g_s the
    gradient of out[:, c] at bank[picks[s]] + alphas[s] d_s; the gap [K] = sum attr - (f(x)[c] - sum_r (n_r / n) f(bank[r])[c]),
    x None: ends[0]), in the dtype of ends"""
    dt = ends.dtype
    n = ends.shape[0]
    picks = torch.as_tensor(np.asarray(picks), dtype=torch.int64)
    a = torch.as_tensor(np.asarray(alphas)).to(dt).view((n,) + (1,) * (ends.dim() - 1))
    b = bank.to(dt)[picks]
    d = ends - b
    rows = (b + a * d).detach().clone().requires_grad_(True)
    out = f(rows)
    g = torch.stack([torch.autograd.grad(out[:, c].sum(), rows, retain_graph=True)[0] for c in cols])
    attr = (g * d[None]).sum(dim=1) / n
    with torch.no_grad():
        at_x = f((ends[0] if x is None else x.to(dt))[None])[0]
        at_bank = f(bank.to(dt))
    expected = shares(picks.numpy(), bank.shape[0]).to(dt) @ at_bank
    gap = attr.reshape(len(cols), -1).sum(dim=1) - (at_x - expected)[list(cols)]
    return attr, gap
