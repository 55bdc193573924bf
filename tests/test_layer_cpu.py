"""Layer IG, layer conductance, HiResCAM and LayerCAM without a device: the tool that adds the four rows (scouter_amd/tools/layer.py)
-- its table, its parser, the keywords its options become -- the header's three entry points, the refusals that come before any
launch, and the float64 restatements the GPU tests hold the kernels and the methods to (tests/layer_restatements.py), checked on
a head that is linear in the features, out = <W, mean_p A>, where both path methods have a closed form."""
import argparse
import ctypes
import inspect

import numpy as np
import pytest
import torch

import layer_restatements as R
from scouter_amd import _native
from scouter_amd import kernels as K
from scouter_amd import test as T
from scouter_amd.tools import ablation as A
from scouter_amd.tools import attribution as AT
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import layer as L

TOOL_DEFAULTS = {"layerig": False, "conductance": False, "hirescam": False, "layercam": False, "layerig_steps": 50,
                 "layerig_batch": 256, "conductance_steps": 50, "conductance_batch": 50}


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_extends_the_ablation_table_by_four_rows():
    assert L.FAMILIES[:len(A.FAMILIES)] == A.FAMILIES and L.FAMILIES == A.FAMILIES + L.LAYERS
    assert [f.name for f in L.LAYERS] == ["layerig", "conductance", "hirescam", "layercam"]
    for rows in (T._ROWS, X._ROWS, A._ROWS):                                # the pinned tables do not know the rows
        assert not any(f.name in rows for f in L.LAYERS)
    want = {"layerig": ("layer_integrated_gradients", "layerig_maps", ["steps", "batch"]),
            "conductance": ("layer_conductance", "conductance_maps", ["steps", "batch"]),
            "hirescam": ("hirescam", "hirescam_maps", []), "layercam": ("layercam", "layercam_maps", [])}
    for name, (explain, maps, suffixes) in want.items():
        row = T._row(name, L._ROWS)
        assert (row.explain, row.maps, row.reduce, row.flag, row.estimate) == (explain, maps, None, True, False)
        assert [o.suffix for o in row.options] == suffixes
        params = inspect.signature(getattr(AT, row.explain)).parameters     # the library functions take the keywords
        assert all(o.keyword in params for o in row.options) and "classes" in params
        assert {"size", "min_level", "classes"} <= set(inspect.signature(getattr(AT, row.maps)).parameters)
    lig, cond = inspect.signature(AT.layer_integrated_gradients).parameters, inspect.signature(AT.layer_conductance).parameters
    assert [lig[k].default for k in ("baseline", "n_steps", "method", "batch", "return_attr", "return_delta")] == \
        [None, 50, "gausslegendre", 256, False, False]
    assert [cond[k].default for k in ("baseline", "n_steps", "batch", "return_attr", "return_delta")] == [None, 50, 50, False, False]
    gxa = inspect.signature(AT.layer_gradxact).parameters
    assert (gxa["rectify"].default, gxa["relu"].default) == (False, False)
    X.check_request(["slot", "occlusion", "layerig", "conductance", "hirescam", "layercam"], True, False, L._ROWS)


def test_the_tool_parser_adds_the_four_rows_and_nothing_else():
    base = vars(A.get_ablation_parser().parse_args([]))
    tool = vars(L.get_layer_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base} == base and tool["table_images"] == 0
    for k, v in TOOL_DEFAULTS.items():
        assert type(tool[k]) is type(v), k
    # an unchanged command line of the ablation tool parses to the same values
    line = ["--occlusion", "true", "--ablationcam", "true", "--occlusion_window", "32", "--occlusion_fill", "-0.5",
            "--ablationcam_batch", "64", "--lime", "true", "--rise_masks", "6", "--cam", "true", "--table_images", "8",
            "--localization", "true", "--model", "resnet18", "--img_size", "64"]
    old, new = vars(A.get_ablation_parser().parse_args(line)), vars(L.get_layer_parser().parse_args(line))
    assert {k: new[k] for k in old} == old and {k: v for k, v in new.items() if k not in old} == TOOL_DEFAULTS
    a = L.get_layer_parser().parse_args(line + ["--layerig", "true", "--conductance", "true", "--hirescam", "true", "--layercam",
                                               "true", "--layerig_steps", "20", "--conductance_batch", "9"])
    assert (a.layerig, a.conductance, a.hirescam, a.layercam, a.layerig_steps, a.conductance_batch) == (True, True, True, True, 20, 9)
    assert X.chosen_families(a, L.FAMILIES) == ["slot", "cam", "lime", "occlusion", "ablationcam", "layerig", "conductance",
                                                "hirescam", "layercam"]
    assert X.chosen_families(a, A.FAMILIES) == ["slot", "cam", "lime", "occlusion", "ablationcam"]


def test_the_options_become_the_library_keywords():
    assert L.option_kwargs(argparse.Namespace(), "layerig") == dict(n_steps=50, batch=256)
    assert L.option_kwargs(argparse.Namespace(), "conductance") == dict(n_steps=50, batch=50)
    assert L.option_kwargs(argparse.Namespace(), "hirescam") == {} and L.option_kwargs(argparse.Namespace(), "layercam") == {}
    a = L.get_layer_parser().parse_args(["--layerig_steps", "8", "--layerig_batch", "3", "--conductance_steps", "12",
                                         "--conductance_batch", "5", "--occlusion_window", "24"])
    assert L.option_kwargs(a, "layerig") == dict(n_steps=8, batch=3)
    assert L.option_kwargs(a, "conductance") == dict(n_steps=12, batch=5)
    assert L.option_kwargs(a, "occlusion")["window"] == 24 and L.option_kwargs(a, "rise") == dict(n_masks=4000, batch=250)
    assert T.option_kwargs(a, "layerig", L._ROWS) == L.option_kwargs(a, "layerig")
    with pytest.raises(ValueError, match="layerig"):
        A.option_kwargs(a, "layerig")                                       # the ablation tool's table has no such row


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    import sys
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["layer.py", "--layerig", "true", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        L.main()


# ------------------------------------------------------------------------------------------------ the header and the wrappers
def test_the_header_declares_the_three_kernels():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {"scouter_conductance_accumulate_f64": [p, p, p, i, i, i, p],
            "scouter_layer_attr_finish_f32": [p] * 6 + [i] * 4 + [p],
            "scouter_layer_gxa_f32": [p, p, p, i, i, i, l, i, i, p]}
    for name, argtypes in want.items():
        assert name in declared and declared[name] == (ctypes.c_int, argtypes), name
    lib = _native.lib()                                                     # binds every declaration: the library exports them
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes
    assert (K.LAYER_PATH, K.LAYER_SUM) == (0, 1)


def test_the_methods_and_wrappers_refuse_before_any_launch():
    x = torch.zeros((1, 3, 16, 16))                                         # on the host: a launch would raise RuntimeError
    for fn in (AT.layer_integrated_gradients, AT.layer_conductance, AT.layer_gradxact, AT.hirescam, AT.layercam):
        with pytest.raises(ValueError, match="images"):
            fn(None, x[0])
    for batch in (1, 0, -3):
        with pytest.raises(ValueError, match="batch"):
            AT.layer_conductance(None, x, batch=batch)
    with pytest.raises(ValueError, match="batch"):
        AT.layer_integrated_gradients(None, x, batch=0)
    with pytest.raises(ValueError, match="n_steps"):
        AT.layer_conductance(None, x, n_steps=0)
    with pytest.raises(ValueError, match="n_steps"):
        AT.layer_integrated_gradients(None, x, n_steps=0)
    with pytest.raises(ValueError, match="method"):
        AT.layer_integrated_gradients(None, x, method="simpson")
    for fn in (AT.layer_integrated_gradients, AT.layer_conductance):
        with pytest.raises(ValueError, match="baseline"):
            fn(None, x, baseline=torch.zeros((3, 16, 15)))
    f, a = torch.zeros((3, 2, 2, 8)), torch.zeros((2, 2, 8), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="conductance_accumulate"):      # the wrappers: a host tensor is refused by name
        K.conductance_accumulate(f, f.clone(), a)
    with pytest.raises(RuntimeError, match="layer_attr_finish"):
        K.layer_attr_finish(K.LAYER_SUM, a[None], torch.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match="layer_attr_finish"):
        K.layer_attr_finish(2, a[None], torch.zeros((1, 2, 2)))
    with pytest.raises(RuntimeError, match="layer_gxa"):
        K.layer_gxa(f, f.clone(), torch.zeros((3, 2, 2)))


# ------------------------------------------------------------------------------------------------ the restatements
def _linear_case(seed, h=3, w=2, C=7, classes=4):
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn((classes, C), generator=gen, dtype=torch.float64)
    a0 = torch.randn((h, w, C), generator=gen, dtype=torch.float64)
    a1 = torch.randn((h, w, C), generator=gen, dtype=torch.float64)
    return W, a0, a1


@pytest.mark.parametrize("table", ["gausslegendre", "riemann_trapezoid", "random"])
def test_layer_ig_restated_on_a_linear_head(table):
    """attr = (A - A') W / (h w) and a completeness gap of 0 up to float64 rounding for ANY table whose weights sum to 1"""
    W, a0, a1 = _linear_case(1)
    h, w, C = a0.shape
    n = 8
    if table == "random":
        gen = torch.Generator().manual_seed(2)
        alphas = torch.rand(n, generator=gen, dtype=torch.float64)
        weights = torch.rand(n, generator=gen, dtype=torch.float64)
        weights = weights / weights.sum()
    else:
        alphas, weights = (t.double() for t in AT.ig_quadrature(n, table))
        weights = weights / weights.sum()                                   # (the fp32 table sums to 1 within 2^-24 only)
    cols = [0, 3, 1]
    attr, gap = R.layer_integrated_gradients(R.linear_head(W), a0, a1, alphas, weights, cols)
    want = (a1 - a0)[None] * W[cols][:, None, None, :] / (h * w)
    mag = want.abs()
    assert tuple(attr.shape) == (3, h, w, C)
    assert bool(((attr - want).abs() <= n * 2.0 ** -52 * mag + 1e-300).all())
    # the outputs themselves are sums of |W A| / (h w) terms: the gap is rounding of those and of the attributions
    terms = mag.sum(dim=(1, 2, 3)) + (W[cols][:, None, None, :] * a0[None]).abs().sum(dim=(1, 2, 3)) / (h * w) + \
        (W[cols][:, None, None, :] * a1[None]).abs().sum(dim=(1, 2, 3)) / (h * w)
    print("layer IG, linear head, %s: max |gap| %.3e, bound %.3e" % (table, float(gap.abs().max()), float((n * 2.0 ** -52 * terms).min())))
    assert bool((gap.abs() <= n * 2.0 ** -52 * terms).all())


def test_conductance_restated_telescopes_on_a_linear_head():
    """g is W / (h w) everywhere, so sum attr = out(f_n) - out(f_0) whatever the points in between"""
    W, a0, a1 = _linear_case(3)
    h, w, C = a0.shape
    n = 8
    gen = torch.Generator().manual_seed(4)
    feats = torch.cat([a0[None], torch.randn((n - 1, h, w, C), generator=gen, dtype=torch.float64), a1[None]])
    cols = [2, 0]
    attr, gap = R.layer_conductance(R.linear_head(W), feats, cols)
    want = (a1 - a0)[None] * W[cols][:, None, None, :] / (h * w)
    steps = ((feats[1:] - feats[:-1]).abs().sum(dim=0)[None] * W[cols][:, None, None, :].abs()) / (h * w)
    assert bool(((attr - want).abs() <= n * 2.0 ** -52 * (steps + (W[cols][:, None, None, :] * feats.abs().sum(dim=0)[None]).abs() / (h * w))).all())
    terms = steps.sum(dim=(1, 2, 3)) + (W[cols][:, None, None, :] * (feats[0].abs() + feats[-1].abs())[None]).abs().sum(dim=(1, 2, 3)) / (h * w)
    print("conductance, linear head: max |gap| %.3e, bound %.3e" % (float(gap.abs().max()), float((n * 2.0 ** -52 * terms).min())))
    assert bool((gap.abs() <= n * 2.0 ** -52 * terms).all())
    # the same sum over positions as layer IG from feats[0] to feats[n]
    alphas, weights = torch.tensor([0.5], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64)
    lig, _ = R.layer_integrated_gradients(R.linear_head(W), a0, a1, alphas, weights, cols)
    assert bool(((lig.sum(dim=(1, 2, 3)) - attr.sum(dim=(1, 2, 3))).abs() <= n * 2.0 ** -52 * terms).all())


def test_the_kernel_restatements_by_hand():
    f = torch.tensor([[1.0, 2.0], [3.0, 5.0], [4.0, 4.0]])
    g = torch.tensor([[2.0, -1.0], [0.5, 3.0], [100.0, 100.0]])            # (the last row's gradient takes no part)
    ref, mag = R.conductance_accumulate(f, g, torch.tensor([10.0, -1.0], dtype=torch.float64))
    assert ref.tolist() == [10.0 + 2.0 * 2.0 + 0.5 * 1.0, -1.0 - 3.0 - 3.0] and mag.tolist() == [14.5, 7.0]
    acc = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]], dtype=torch.float64)
    s = R.layer_attr_finish(acc)
    assert s["map"].tolist() == [[3.0, 7.0]] and s["total"].tolist() == [10.0]
    p = R.layer_attr_finish(acc, torch.tensor([[1.0, 1.0], [2.0, 0.0]]), torch.tensor([[0.0, 2.0], [0.0, 0.0]]))
    assert p["terms"].tolist() == [[[1.0, -2.0], [6.0, 0.0]]] and p["map"].tolist() == [[-1.0, 6.0]] and p["map_mag"].tolist() == [[3.0, 6.0]]
    assert R.layer_attr_finish(acc, torch.ones((2, 2)))["total"].tolist() == [10.0]
    feat, dfeat = torch.tensor([[[1.0, 2.0, 3.0]]]), torch.tensor([[[-4.0, 1.0, -1.0]]])
    assert R.layer_gxa(feat, dfeat, False, False)[0].tolist() == [[-5.0]] and R.layer_gxa(feat, dfeat, False, True)[0].tolist() == [[0.0]]
    assert R.layer_gxa(feat, dfeat, True, True)[0].tolist() == [[2.0]] and R.layer_gxa(feat, dfeat, True, False)[1].tolist() == [[2.0]]
    assert np.isclose(float(R.layer_gxa(feat, dfeat, False, False)[1]), 9.0)
