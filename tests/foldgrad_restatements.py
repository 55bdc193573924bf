"""float64 restatements of the three kernels of csrc/fold_bwd.hip (torch, on the host), with the magnitudes the derived bounds of
tests/test_foldgrad_gpu.py are made of.  Test infrastructure only: nothing here is imported by the package."""
import math

import torch

EPS = 2.0 ** -24


def gate_group(length):
    """lanes that share a row of `length` elements in the kernel's row dots: length / 4 pieces rounded up to a power of two, at most
    a wave (csrc/fold_bwd.hip gate_group)"""
    g = 1
    while g < 64 and 4 * g < length:
        g <<= 1
    return g


def row_chain(length):
    """additions on the longest path to one output of a row dot of `length` terms: the fmas of a lane's chain, the two levels that
    combine its four chains, the butterfly over the lanes"""
    g = gate_group(length)
    return -(-length // (4 * g)) + 2 + int(math.log2(g))


def hidden_chain(Cp, A, threads=256):
    """... of the forward's fc1 column (csrc/sa_gate.h): a slice's eight chains, their three levels, the slices, the bias"""
    parts = threads // A
    return Cp // parts // 8 + 3 + (parts - 1) + 1


def sa_gate_bwd(gap, w1, b1, w2, a, da):
    """gap [B, Cp], w1 [Cp, A], b1 [A], w2 [A, 2Cp], a / da [B, 2Cp] (fp32 values) -> dict of float64 tensors:
    pre [B, A] the hidden pre-activation and pre_mag its sum of magnitudes, h = relu(pre), dz, dz_err (the bound on the kernel's
    fp32 dz: three roundings in the dot -- two products and their sum --, one in the difference, one in the product),
    dh and dh_mag / dh_in (sum |dz w2| and the propagated sum dz_err |w2|), dgap and dgap_mag (sum |dh w1|)"""
    gap, w1, b1, w2, a, da = (t.double() for t in (gap, w1, b1, w2, a, da))
    Cp = gap.shape[1]
    pre = gap @ w1 + b1
    pre_mag = gap.abs() @ w1.abs() + b1.abs()
    h = pre.clamp_min(0.0)
    a0, a1, d0, d1 = a[:, :Cp], a[:, Cp:], da[:, :Cp], da[:, Cp:]
    dot, S = a0 * d0 + a1 * d1, (a0 * d0).abs() + (a1 * d1).abs()
    dz = torch.cat([a0 * (d0 - dot), a1 * (d1 - dot)], dim=1)
    dz_err = EPS * (3.0 * torch.cat([a0.abs() * S, a1.abs() * S], dim=1) + 3.0 * dz.abs())
    mask = (pre > 0).double()
    dh = (dz @ w2.t()) * mask
    dh_mag = (dz.abs() @ w2.abs().t()) * mask
    dh_in = (dz_err @ w2.abs().t()) * mask
    return dict(pre=pre, pre_mag=pre_mag, h=h, dz=dz, dz_err=dz_err, dh=dh, dh_mag=dh_mag, dh_in=dh_in, dgap=dh @ w1.t(),
                dgap_mag=dh.abs() @ w1.abs().t())


def sa_apply_relu_bwd(dout, a, dgap, x0):
    """dout [B, HW, Cp], a [B, 2Cp], dgap [B, Cp], x0 [B, HW, 2Cp] -> (dx [B, HW, 2Cp] float64, |dout a| + |dgap| / HW, x0 > 0)"""
    dout, a, dgap = dout.double(), a.double(), dgap.double()
    HW = dout.shape[1]
    d2 = torch.cat([dout, dout], dim=2)
    g2 = torch.cat([dgap, dgap], dim=1)[:, None] / HW
    keep = x0 > 0
    return (d2 * a[:, None] + g2) * keep, (d2 * a[:, None]).abs() + g2.abs(), keep
