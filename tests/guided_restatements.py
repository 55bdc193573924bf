"""Host restatements (torch) of what guided backpropagation, the deconvnet rule and Guided Grad-CAM add: the rule a ReLU's backward
applies (csrc/relu_rule.h), the gate's backward of tests/foldgrad_restatements.py extended by the rule, the integer nearest index
of csrc/guided.hip, and the autograd Function that pins the CPU oracle's ReLUs to a rule.  Test infrastructure only: nothing here
is imported by the package."""
import torch

import foldgrad_restatements as F0

EPS = F0.EPS
RULES = {"gradient": 0, "guided": 1, "deconvnet": 2}


def rule_keep(g, act, rule):
    """where the gradient g arriving at a ReLU whose output was act leaves it: plain comparisons, so a NaN or a zero of either
    sign in g is not `> 0`.  rule: a name or its number"""
    rule = RULES.get(rule, rule)
    if rule == 0:
        return (act > 0).expand(g.shape)
    if rule == 1:
        return (act > 0) & (g > 0)
    if rule == 2:
        return g > 0
    raise ValueError("unknown rule %r" % (rule,))


def rule_select(g, act, rule):
    """the gradient leaving the ReLU: g where rule_keep, an exact +0 elsewhere; g's own bits (a -0 or a NaN passes under rule 0)"""
    return torch.where(rule_keep(g, act, rule), g, torch.zeros_like(g))


def quadrants(g, act):
    """how many elements fall into each (act > 0, g > 0) quadrant: [(T, T), (T, F), (F, T), (F, F)]"""
    a, p = act > 0, g > 0
    return [int((a & p).sum()), int((a & ~p).sum()), int((~a & p).sum()), int((~a & ~p).sum())]


def zeros_of_both_signs(t):
    z = t == 0
    return bool((z & torch.signbit(t)).any()) and bool((z & ~torch.signbit(t)).any())


def sa_gate_bwd(gap, w1, b1, w2, a, da, rule="gradient"):
    """foldgrad_restatements.sa_gate_bwd under a rule at the hidden ReLU: g = dz . w2^T, dh = rule_select(g, h).  relu(.) is
    1-Lipschitz, so a sign of g decided differently within g's own error moves dh by no more than that error: dh_mag / dh_in are
    taken WITHOUT the g > 0 factor, and under "deconvnet" without [h > 0] too."""
    r = F0.sa_gate_bwd(gap, w1, b1, w2, a, da)
    w1d, w2d = w1.double(), w2.double()
    g = r["dz"] @ w2d.t()
    pos = r["pre"] > 0
    dh = rule_select(g, pos.double(), rule)
    seen = pos.double() if RULES.get(rule, rule) != 2 else torch.ones_like(g)
    r.update(g=g, dh=dh, dh_mag=(r["dz"].abs() @ w2d.abs().t()) * seen, dh_in=(r["dz_err"] @ w2d.abs().t()) * seen,
             dgap=dh @ w1d.t(), dgap_mag=dh.abs() @ w1d.abs().t())
    return r


def nearest_index(n_out, n_in):
    """source index of every destination index of an axis: (d n_in) // n_out in integer arithmetic (csrc/guided.hip)"""
    return (torch.arange(n_out, dtype=torch.int64) * n_in) // n_out


def upsample_nearest(cam, H, W):
    """cam [..., h, w] -> [..., H, W] by the integer indices"""
    h, w = cam.shape[-2:]
    iy, ix = nearest_index(H, h).to(cam.device), nearest_index(W, w).to(cam.device)
    return cam[..., iy, :][..., ix]


class Rule(torch.autograd.Function):
    """y = x * mask with the rule's table as its backward: what pins a ReLU of the CPU oracle to the pass's own sign pattern AND
    to a rule.  mask: bool, the shape of x."""

    @staticmethod
    def forward(ctx, x, mask, rule):
        ctx.save_for_backward(mask)
        ctx.rule = rule
        return x * mask.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return rule_select(g, mask.to(g.dtype), ctx.rule), None, None
