"""Plain-torch restatements of csrc/layerattr.hip's three kernels and of the two layer path methods of tools/attribution.py
(layer_integrated_gradients, layer_conductance), shared by tests/test_layer_cpu.py and tests/test_layer_gpu.py.  Everything runs on
the host in the dtype of its inputs: float64 for the references, float32 for the yardstick of the project's rule.  Each kernel
restatement also returns the magnitude sum |terms| its error bound is relative to."""
import torch


# ------------------------------------------------------------------------------------------------ the kernels
def conductance_accumulate(feats, grads, acc0):
    """feats, grads [r, ...], acc0 [...] -> (acc0 + sum_{j < r - 1} grads[j] (feats[j + 1] - feats[j]), |acc0| + sum |terms|)"""
    f, g, a = feats.double(), grads.double(), acc0.double()
    terms = g[:-1] * (f[1:] - f[:-1])
    return a + terms.sum(dim=0), a.abs() + terms.abs().sum(dim=0)


def layer_attr_finish(acc, feat=None, base=None):
    """acc [K, P, C]; feat given: mode PATH, terms = (feat - base) acc (base None: zeros), else mode SUM, terms = acc
    -> dict(terms [K, P, C], map [K, P], map_mag [K, P], total [K], total_mag [K])"""
    terms = acc.double()
    if feat is not None:
        diff = feat.double() - (base.double() if base is not None else 0.0)
        terms = diff[None] * terms
    return dict(terms=terms, map=terms.sum(dim=2), map_mag=terms.abs().sum(dim=2), total=terms.sum(dim=(1, 2)),
                total_mag=terms.abs().sum(dim=(1, 2)))


def layer_gxa(feat, dfeat, rectify, relu):
    """feat, dfeat [B, P, C] -> (sum_c r(dfeat) feat [B, P] clamped at 0 with relu, sum_c |terms|)"""
    g = dfeat.double()
    terms = (g.clamp_min(0.0) if rectify else g) * feat.double()
    ref = terms.sum(dim=2)
    return (ref.clamp_min(0.0) if relu else ref), terms.abs().sum(dim=2)


# ------------------------------------------------------------------------------------------------ the path methods
def head_gradients(head, feats, cols):
    """head: features [n, h, w, C] -> outputs [n, classes], differentiable -> (d sum_n out[:, c] / d feats for c in cols, stacked
    [K, n, h, w, C], the outputs detached)"""
    x = feats.detach().clone().requires_grad_(True)
    out = head(x)
    grads = [torch.autograd.grad(out[:, c].sum(), x, retain_graph=True)[0] for c in cols]
    return torch.stack(grads), out.detach()


def layer_integrated_gradients(head, a0, a1, alphas, weights, cols):
    """a0, a1 [h, w, C] (the baseline's and the image's features), alphas / weights [n] -> (attr [K, h, w, C] =
    (a1 - a0) sum_i w_i g(a0 + alpha_i (a1 - a0)), the gap [K] = sum attr - (out(a1) - out(a0))[cols]), in the dtype of a0"""
    dt = a0.dtype
    diff = a1 - a0
    rows = a0[None] + alphas.to(dt)[:, None, None, None] * diff[None]
    g, _ = head_gradients(head, rows, cols)
    attr = diff[None] * (weights.to(dt)[None, :, None, None, None] * g).sum(dim=1)
    with torch.no_grad():
        ends = head(torch.stack([a0, a1]))
    return attr, attr.sum(dim=(1, 2, 3)) - (ends[1] - ends[0])[list(cols)]


def layer_conductance(head, feats, cols):
    """feats [n + 1, h, w, C], the layer along the path -> (attr [K, h, w, C] = sum_{i < n} g(feats[i]) (feats[i + 1] - feats[i]),
    the gap [K] = sum attr - (out(feats[n]) - out(feats[0]))[cols]), in the dtype of feats"""
    g, out = head_gradients(head, feats, cols)
    attr = (g[:, :-1] * (feats[1:] - feats[:-1])[None]).sum(dim=1)
    return attr, attr.sum(dim=(1, 2, 3)) - (out[-1] - out[0])[list(cols)]


def linear_head(W):
    """out[n, k] = <W[k], mean_p A[n, p]>: the head the closed forms of tests/test_layer_cpu.py hold for"""
    return lambda feats: torch.einsum("kc,nc->nk", W, feats.mean(dim=(1, 2)))
