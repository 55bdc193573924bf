"""GradientSHAP without a device: the NumPy restatement of the draws of csrc/gradshap.hip (known answers, and what a uniform pick and
a uniform fraction must look like), the tool that adds the two rows (scouter_amd/tools/gradshap.py) -- its table, its parser, the
keywords its options become -- the header's three entry points, the refusals that come before any launch, and the float64
restatement the GPU tests hold the methods to (tests/gradshap_restatements.py), checked where the method has a closed form:
out = <w, x> and out = |x|^2 / 2."""
import argparse
import ctypes
import inspect

import numpy as np
import pytest
import torch

import gradshap_restatements as R
from scouter_amd import _native
from scouter_amd import kernels as K
from scouter_amd import test as T
from scouter_amd.tools import ablation as A
from scouter_amd.tools import attribution as AT
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import gradshap as G
from scouter_amd.tools import layer as L
from scouter_amd.tools import surrogate as S

TOOL_DEFAULTS = {"gradshap": False, "layergradshap": False, "gradshap_samples": 50, "gradshap_baselines": 10,
                 "gradshap_bank_sigma": 1.0, "gradshap_sigma": 0.0, "gradshap_batch": 50, "gradshap_seed": 0,
                 "layergradshap_samples": 200, "layergradshap_baselines": 10, "layergradshap_bank_sigma": 1.0,
                 "layergradshap_batch": 256, "layergradshap_seed": 0}


# ------------------------------------------------------------------------------------------------ the draws
def test_the_draw_restatement_reproduces_known_answers():
    """seed 0, R = 3, samples 0 .. 7: the counter (0, s, 2, 0), the key (0, 0)"""
    r0, r1 = R.draw_words(0, 0, 8)
    assert ["%08x" % int(v) for v in r1] == ["b6826759", "2f5f3cd9", "d6a52dd9", "d078ad44", "b68b5374", "c7ded33c", "a6c13eb7",
                                             "e9a31887"]
    picks, alphas = R.draws(0, 0, 8, 3)
    assert picks.dtype == np.int32 and alphas.dtype == np.float32
    assert picks.tolist() == [0, 0, 0, 2, 2, 0, 2, 2]
    assert picks.tolist() == [(int(v) * 3) >> 32 for v in r0]
    assert alphas.tolist() == [(2 * (int(v) >> 9) + 1) * 2.0 ** -24 for v in r1]          # exact in fp32
    # a chunk that starts later is the same samples, and the draws of one R say nothing about another's
    later, la = R.draws(0, 5, 3, 3)
    assert later.tolist() == picks[5:].tolist() and la.tolist() == alphas[5:].tolist()
    assert R.draws(0, 0, 8, 1)[0].tolist() == [0] * 8 and R.draws(0, 0, 8, 1)[1].tolist() == alphas.tolist()


@pytest.mark.parametrize("seed", [0, 1, 2 ** 40 + 7, 2 ** 64 - 1])
def test_the_draws_look_uniform(seed):
    """4096 samples: every alpha strictly inside (0, 1) with a mean within 4 standard errors of 1 / 2, every baseline's count within
    4 binomial standard deviations of n / R"""
    n = 4096
    for Rn in (1, 2, 3, 7, 10):
        picks, alphas = R.draws(seed, 0, n, Rn)
        assert picks.min() >= 0 and picks.max() < Rn
        assert float(alphas.min()) > 0.0 and float(alphas.max()) < 1.0
        counts = np.bincount(picks, minlength=Rn)
        assert counts.sum() == n
        sd = np.sqrt(n * (1.0 / Rn) * (1.0 - 1.0 / Rn))
        dev = float(np.abs(counts - n / Rn).max()) / sd if Rn > 1 else 0.0
        z = abs(float(alphas.astype(np.float64).mean()) - 0.5) / (0.288675 / 64)
        print("seed %d R %d: worst count %.2f sd, mean alpha %.2f se" % (seed, Rn, dev, z))
        assert dev <= 4.0 and z <= 4.0
    assert not np.array_equal(R.draws(seed, 0, 64, 10)[0], R.draws(seed ^ 1, 0, 64, 10)[0])


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_extends_the_layer_table_by_two_rows():
    assert G.FAMILIES[:len(L.FAMILIES)] == L.FAMILIES and G.FAMILIES == L.FAMILIES + G.SHAPS
    assert [f.name for f in G.SHAPS] == ["gradshap", "layergradshap"]
    for rows in (T._ROWS, X._ROWS, S._ROWS, A._ROWS, L._ROWS):              # the pinned tables do not know the rows
        assert not any(f.name in rows for f in G.SHAPS)
    for fams in (T.FAMILIES, X.FAMILIES, S.FAMILIES, A.FAMILIES, L.FAMILIES):
        assert not any(f.name in ("gradshap", "layergradshap") for f in fams)
    want = {"gradshap": ("gradient_shap", "gradient_maps", T._channel_mean, ["samples", "baselines", "bank_sigma", "sigma", "batch", "seed"]),
            "layergradshap": ("layer_gradient_shap", "layergradshap_maps", None, ["samples", "baselines", "bank_sigma", "batch", "seed"])}
    for name, (explain, maps, reduce, suffixes) in want.items():
        row = T._row(name, G._ROWS)
        assert (row.explain, row.maps, row.reduce, row.flag, row.estimate) == (explain, maps, reduce, True, False)
        assert [o.suffix for o in row.options] == suffixes
        params = inspect.signature(getattr(AT, row.explain)).parameters     # the library functions take the keywords
        assert all(o.keyword in params for o in row.options) and "classes" in params
        assert all(params[o.keyword].default == o.default for o in row.options)
    assert {"size", "min_level", "classes"} <= set(inspect.signature(AT.layergradshap_maps).parameters)
    gs, lgs = inspect.signature(AT.gradient_shap).parameters, inspect.signature(AT.layer_gradient_shap).parameters
    assert [gs[k].default for k in ("classes", "baselines", "bank_sigma", "n_samples", "sigma", "batch", "seed", "return_delta")] == \
        [None, 10, 1.0, 50, 0.0, 50, 0, False]
    assert [lgs[k].default for k in ("classes", "baselines", "bank_sigma", "n_samples", "batch", "seed", "return_attr", "return_delta")] == \
        [None, 10, 1.0, 200, 256, 0, False, False]
    assert "sigma" not in lgs
    X.check_request(["slot", "layerig", "gradshap", "layergradshap"], True, False, G._ROWS)


def test_the_tool_parser_adds_the_two_rows_and_nothing_else():
    base = vars(L.get_layer_parser().parse_args([]))
    tool = vars(G.get_gradshap_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base} == base and tool["table_images"] == 0
    for k, v in TOOL_DEFAULTS.items():
        assert type(tool[k]) is type(v), k
    # an unchanged command line of the layer tool parses to the same values
    line = ["--layerig", "true", "--conductance", "true", "--layerig_steps", "20", "--conductance_batch", "9", "--occlusion", "true",
            "--occlusion_window", "32", "--lime", "true", "--rise_masks", "6", "--cam", "true", "--table_images", "8",
            "--localization", "true", "--model", "resnet18", "--img_size", "64"]
    old, new = vars(L.get_layer_parser().parse_args(line)), vars(G.get_gradshap_parser().parse_args(line))
    assert {k: new[k] for k in old} == old and {k: v for k, v in new.items() if k not in old} == TOOL_DEFAULTS
    a = G.get_gradshap_parser().parse_args(line + ["--gradshap", "true", "--layergradshap", "true", "--gradshap_samples", "20",
                                                  "--gradshap_sigma", "0.25", "--layergradshap_seed", "9"])
    assert (a.gradshap, a.layergradshap, a.gradshap_samples, a.gradshap_sigma, a.layergradshap_seed) == (True, True, 20, 0.25, 9)
    assert X.chosen_families(a, G.FAMILIES) == ["slot", "cam", "lime", "occlusion", "layerig", "conductance", "gradshap",
                                                "layergradshap"]
    assert X.chosen_families(a, L.FAMILIES) == ["slot", "cam", "lime", "occlusion", "layerig", "conductance"]


def test_the_options_become_the_library_keywords():
    assert G.option_kwargs(argparse.Namespace(), "gradshap") == dict(n_samples=50, baselines=10, bank_sigma=1.0, sigma=0.0, batch=50,
                                                                    seed=0)
    assert G.option_kwargs(argparse.Namespace(), "layergradshap") == dict(n_samples=200, baselines=10, bank_sigma=1.0, batch=256, seed=0)
    a = G.get_gradshap_parser().parse_args(["--gradshap_samples", "8", "--gradshap_baselines", "3", "--gradshap_bank_sigma", "0.5",
                                            "--gradshap_sigma", "0.1", "--gradshap_batch", "4", "--gradshap_seed", "7",
                                            "--layergradshap_samples", "12", "--layergradshap_baselines", "2",
                                            "--layergradshap_bank_sigma", "0", "--layergradshap_batch", "5", "--layergradshap_seed", "3",
                                            "--layerig_steps", "6"])
    assert G.option_kwargs(a, "gradshap") == dict(n_samples=8, baselines=3, bank_sigma=0.5, sigma=0.1, batch=4, seed=7)
    assert G.option_kwargs(a, "layergradshap") == dict(n_samples=12, baselines=2, bank_sigma=0.0, batch=5, seed=3)
    assert G.option_kwargs(a, "layerig") == dict(n_steps=6, batch=256) and G.option_kwargs(a, "rise") == dict(n_masks=4000, batch=250)
    assert T.option_kwargs(a, "gradshap", G._ROWS) == G.option_kwargs(a, "gradshap")
    with pytest.raises(ValueError, match="gradshap"):
        L.option_kwargs(a, "gradshap")                                      # the layer tool's table has no such row


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    import sys
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["gradshap.py", "--gradshap", "true", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        G.main()


# ------------------------------------------------------------------------------------------------ the header and the wrappers
def test_the_header_declares_the_three_kernels():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    i, l, p, f, d = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    want = {"scouter_gradshap_draws": [p, p, i, i, i, i, i, p],
            "scouter_gradshap_images_f32": [p, p, p, f, i, i, i, i, i, l, p],
            "scouter_gradshap_accumulate_f64": [p, p, p, p, f, d, i, i, i, i, i, l, p]}
    for name, argtypes in want.items():
        assert name in declared and declared[name] == (ctypes.c_int, argtypes), name
    lib = _native.lib()                                                     # binds every declaration: the library exports them
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes


def test_the_methods_and_wrappers_refuse_before_any_launch():
    x = torch.zeros((1, 3, 16, 16))                                         # on the host: a launch would raise RuntimeError
    for fn in (AT.gradient_shap, AT.layer_gradient_shap, AT.layergradshap_maps):
        with pytest.raises(ValueError, match="images"):
            fn(None, x[0])
        for batch in (0, -3):
            with pytest.raises(ValueError, match="batch"):
                fn(None, x, batch=batch)
        with pytest.raises(ValueError, match="n_samples"):
            fn(None, x, n_samples=0)
        for bad in (-1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="bank_sigma"):
                fn(None, x, bank_sigma=bad)
        for bad in (0, -2, torch.zeros((2, 3, 16, 15)), torch.zeros((3, 16, 16)), torch.zeros((0, 3, 16, 16)), None, 2.5, "ten", True):
            with pytest.raises(ValueError, match="baselines"):
                fn(None, x, baselines=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="^sigma"):
            AT.gradient_shap(None, x, sigma=bad)
    with pytest.raises(TypeError):
        AT.layer_gradient_shap(None, x, sigma=0.1)                          # the layer method has no noise option
    image, bank = torch.zeros((3, 4, 4)), torch.zeros((2, 3, 4, 4))
    rows, acc = torch.zeros((5, 3, 4, 4)), torch.zeros((3, 4, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="gradshap_draws"):              # the wrappers: a host tensor is refused by name
        K.gradshap_draws(5, 2, 0, picks=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="gradshap_draws"):
        K.gradshap_draws(5, 2, 0, alphas=torch.zeros(5))
    with pytest.raises(RuntimeError, match="gradshap_images"):
        K.gradshap_images(image, bank, rows, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="gradshap_accumulate"):
        K.gradshap_accumulate(rows, image, bank, acc, 0.0, 0, 0)


# ------------------------------------------------------------------------------------------------ the restatement of the method
def _case(seed, shape=(3, 5, 7), Rn=3, n=16):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    bank = torch.randn((Rn,) + shape, generator=gen, dtype=torch.float64)
    picks, alphas = R.draws(seed, 0, n, Rn)
    return x, bank, picks, alphas


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
def test_gradient_shap_restated_on_a_linear_model(noisy):
    """out = <w, x>: the gradient is w everywhere, so attr = w (mean_s x~_s - sum_r (n_r / n) b_r) and, without noise, the gap is 0"""
    x, bank, picks, alphas = _case(1)
    n = len(picks)
    gen = torch.Generator().manual_seed(2)
    W = torch.randn((4,) + tuple(x.shape), generator=gen, dtype=torch.float64)
    ends = x[None].repeat(n, 1, 1, 1) + (0.3 * torch.randn((n,) + tuple(x.shape), generator=gen, dtype=torch.float64) if noisy else 0.0)
    cols = [0, 3, 1]
    attr, gap = R.gradient_shap(lambda rows: torch.einsum("kchw,nchw->nk", W, rows), ends, bank, picks, alphas, cols, x=x)
    share = R.shares(picks, bank.shape[0])
    assert float(share.sum()) == 1.0
    centre = ends.mean(dim=0) - torch.einsum("r,rchw->chw", share, bank)
    want = W[cols] * centre[None]
    mag = W[cols].abs() * (ends.abs().mean(dim=0) + torch.einsum("r,rchw->chw", share, bank.abs()))[None]
    assert tuple(attr.shape) == (3,) + tuple(x.shape)
    assert bool(((attr - want).abs() <= (n + 4) * 2.0 ** -52 * mag).all())
    terms = mag.sum(dim=(1, 2, 3)) + (W[cols] * x[None]).abs().sum(dim=(1, 2, 3)) + \
        torch.einsum("r,krchw->k", share, (W[cols][:, None] * bank[None]).abs())
    bound = (x.numel() + n + 4) * 2.0 ** -52 * terms
    noise = torch.einsum("kchw,chw->k", W[cols], ends.mean(dim=0) - x)      # with sigma > 0 the gap also holds the noise
    print("gradient SHAP, linear model, %s: max |gap - noise| %.3e, bound %.3e" % ("noisy" if noisy else "clean",
                                                                                  float((gap - noise).abs().max()), float(bound.min())))
    assert bool(((gap - noise).abs() <= bound).all())
    if not noisy:
        assert bool((gap.abs() <= bound).all())


def test_gradient_shap_restated_on_a_quadratic_model():
    """out = |x|^2 / 2: the gradient at a row is the row, so attr = (1 / n) sum_s (b + alpha_s (x - b)) (x - b) over the exact draws"""
    x, bank, picks, alphas = _case(3, shape=(2, 3, 4), Rn=7, n=24)
    n = len(picks)
    ends = x[None].repeat(n, 1, 1, 1)
    attr, gap = R.gradient_shap(lambda rows: 0.5 * (rows * rows).sum(dim=(1, 2, 3))[:, None], ends, bank, picks, alphas, [0])
    want, mag = torch.zeros_like(x), torch.zeros_like(x)
    for s in range(n):
        b = bank[int(picks[s])]
        t = (b + float(alphas[s]) * (x - b)) * (x - b) / n
        want, mag = want + t, mag + t.abs()
    assert bool(((attr[0] - want).abs() <= (n + 4) * 2.0 ** -52 * mag).all())
    # the gap is the Monte-Carlo error of one point per line: (1 / n) sum_s (alpha_s - 1 / 2) |x - b_s|^2, not rounding
    d2 = torch.stack([((x - bank[int(p)]) ** 2).sum() for p in picks])
    mc = float(((torch.from_numpy(alphas.astype(np.float64)) - 0.5) * d2).sum() / n)
    assert abs(float(gap[0]) - mc) <= (x.numel() + n + 4) * 2.0 ** -52 * float(mag.sum() + 0.5 * (x * x).sum() + 0.5 * (bank * bank).sum())
    assert abs(mc) > 1e-6


def test_the_accumulate_restatement_by_hand():
    g = torch.tensor([[2.0, -1.0], [0.5, 3.0]])
    d = torch.tensor([[1.0, 4.0], [-2.0, 0.5]])
    ref, mag = R.accumulate(g, d, torch.tensor([10.0, -1.0], dtype=torch.float64), 0.5)
    assert ref.tolist() == [10.0 + 1.0 - 0.5, -1.0 - 2.0 + 0.75] and mag.tolist() == [11.5, 3.75]
