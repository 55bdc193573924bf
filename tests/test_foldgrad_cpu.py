"""The gradient-only backward of the folded eval path without a device: the header's three entry points, the refusals that come
before any launch (a bad route, of="loss" on the folded route, a host tensor), the tool that adds the four route options
(scouter_amd/tools/foldgrad.py) -- its table, its parser, the keywords its options become -- and the float64 restatement of the
gate's backward (tests/foldgrad_restatements.py) against torch's own autograd."""
import argparse
import ctypes
import inspect

import pytest
import torch

import foldgrad_restatements as R
from scouter_amd import _native
from scouter_amd import test as T
from scouter_amd.tools import ablation as A
from scouter_amd.tools import attribution as AT
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import foldgrad as FG
from scouter_amd.tools import gradshap as G
from scouter_amd.tools import layer as L
from scouter_amd.tools import surrogate as S

ROUTED = ["grad", "ig", "smoothgrad", "gradshap"]
TOOL_DEFAULTS = {"grad_route": "autograd", "ig_route": "autograd", "smoothgrad_route": "autograd", "gradshap_route": "autograd"}
METHODS = {"grad": AT.input_gradients, "ig": AT.integrated_gradients_by_route, "smoothgrad": AT.smoothgrad_by_route,
           "gradshap": AT.gradient_shap}
BY_ROUTE = {"ig": "integrated_gradients_by_route", "smoothgrad": "smoothgrad_by_route"}


# ------------------------------------------------------------------------------------------------ the header
def test_the_header_declares_the_three_kernels():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    i, p = ctypes.c_int, ctypes.c_void_p
    want = {"scouter_sa_gate_bwd_f32": [p, p, p, p, p, p, p, p, i, i, i, p],
            "scouter_sa_apply_relu_bwd_f32": [p, p, p, p, p, i, i, i, p],
            "scouter_maxpool_relu_bwd_f32": [p, p, p, p, i, i, i, i, i, i, i, p]}
    for name, argtypes in want.items():
        assert name in declared and declared[name] == (ctypes.c_int, argtypes), name
    lib = _native.lib()                                                     # binds every declaration: the library exports them
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes


def test_the_model_has_the_pass():
    from scouter_amd import kernels as K
    from scouter_amd.sloter.slot_model import ImagePass, SlotModel
    assert list(inspect.signature(SlotModel.image_pass).parameters) == ["self", "x"]
    for name in ("grad", "relu_outputs"):
        assert callable(getattr(ImagePass, name))
    assert list(inspect.signature(ImagePass.grad).parameters) == ["self", "seed"]           # no rule argument
    for name in ("sa_gate_bwd", "sa_apply_relu_bwd", "maxpool_relu_bwd"):
        assert callable(getattr(K, name))
    assert "no backward" not in SlotModel.set_inference_fold.__doc__ and "image_pass" in SlotModel.set_inference_fold.__doc__


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_the_methods_refuse_before_any_launch():
    x = torch.zeros((1, 3, 16, 16))                                         # on the host: a launch would raise from the library
    for name, fn in METHODS.items():
        params = inspect.signature(fn).parameters
        assert params["route"].default == "autograd" and list(params)[-1] == "route", name
        for bad in ("fold", "Folded", "", None, 1):
            with pytest.raises(ValueError, match="route"):
                fn(None, x, route=bad)
        with pytest.raises(RuntimeError, match="folded"):                   # a host tensor: no model is touched (it is None)
            fn(None, x, route="folded")
        with pytest.raises(ValueError, match="images"):
            fn(None, x[0], route="folded")
    with pytest.raises(ValueError, match="loss"):
        AT.input_gradients(None, x, of="loss", target=torch.zeros(1, dtype=torch.long), route="folded")
    with pytest.raises(ValueError, match="of must be"):
        AT.input_gradients(None, x, of="prob", route="folded")
    for fn in (AT.integrated_gradients_by_route, AT.smoothgrad_by_route, AT.gradient_shap):   # the methods' own refusals come first
        with pytest.raises(ValueError, match="batch"):
            fn(None, x, batch=0, route="folded")


def test_the_folded_loop_order_is_image_chunk_class():
    """_path_method(route="folded") on a stand-in model: ONE fill and ONE image_pass per chunk, one .grad per class and chunk, the
    chunks of a class in ascending order, `finish` per class at the end"""
    log = []

    class Pass:
        def __init__(self, rows):
            self.rows = rows

        def grad(self, seed):
            log.append(("grad", int(seed[0].argmax()), self.rows))
            return None

    class Model(torch.nn.Module):
        def image_pass(self, chunk):
            log.append(("pass", chunk.shape[0]))
            return Pass(chunk.shape[0])

    def fill(b, buf, first):
        log.append(("fill", b, first, buf.shape[0]))
        return buf

    images = torch.zeros((2, 1, 4, 4))
    out = AT._path_method(Model(), images, 5, False, [4, 1], 3, 7, fill, None, True,
                          lambda b, acc, acc_sq, o, total: log.append(("finish", b, tuple(acc.shape), acc_sq is not None)),
                          accumulate=lambda b, grads, acc, first: log.append(("acc", b, first, tuple(acc.shape))), route="folded")
    assert tuple(out.shape) == (2, 2, 1, 4, 4)
    per_image = []
    for b in range(2):
        for first, n in ((0, 3), (3, 3), (6, 1)):
            per_image += [("fill", b, first, n), ("pass", n)]
            for c in (4, 1):
                per_image += [("grad", c, n), ("acc", b, first, (1, 4, 4))]
        per_image += [("finish", b, (1, 4, 4), True)] * 2
    assert log == per_image


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_replaces_four_rows_by_copies_with_one_more_option():
    assert [f.name for f in FG.FAMILIES] == [f.name for f in G.FAMILIES] and list(FG.ROUTED) == ROUTED
    for mine, theirs in zip(FG.FAMILIES, G.FAMILIES):
        if mine.name in ROUTED:
            assert mine.explain == BY_ROUTE.get(mine.name, theirs.explain)
            assert mine._replace(options=theirs.options, explain=theirs.explain) == theirs
            assert mine.options[:-1] == tuple(theirs.options) and mine.options[-1] is FG._ROUTE
        else:
            assert mine is theirs
    o = FG._ROUTE
    assert (o.suffix, o.keyword, o.type, o.default, o.choices, o.convert) == ("route", "route", str, "autograd", ("autograd", "folded"), None)
    # the pinned tables do not know the option
    for rows in (T._ROWS, X._ROWS, S._ROWS, A._ROWS, L._ROWS, G._ROWS):
        for name in ROUTED:
            if name in rows:
                assert all(op.suffix != "route" for op in rows[name].options), name
    assert [f.name for f in T.FAMILIES][:2] == ["slot", "grad"] and T._row("grad").options == ()
    assert [op.suffix for op in T._row("ig").options] == ["steps", "batch"]
    assert [op.suffix for op in T._row("smoothgrad").options] == ["samples", "sigma", "batch"]
    assert [op.suffix for op in T._row("gradshap", G._ROWS).options] == ["samples", "baselines", "bank_sigma", "sigma", "batch", "seed"]
    for name in ROUTED:                                                     # the library functions take the keywords
        row = T._row(name, FG._ROWS)
        params = inspect.signature(getattr(AT, row.explain)).parameters
        assert all(op.keyword in params and params[op.keyword].default == op.default for op in row.options), name
        assert (row.maps, row.flag, row.reduce) == (T._row(name, G._ROWS).maps, T._row(name, G._ROWS).flag, T._row(name, G._ROWS).reduce)
    # the two methods whose parameter lists are pinned keep them, and their *_by_route forms add exactly the one option
    for old, new in ((AT.integrated_gradients, AT.integrated_gradients_by_route), (AT.smoothgrad, AT.smoothgrad_by_route)):
        po, pn = inspect.signature(old).parameters, inspect.signature(new).parameters
        assert "route" not in po and list(pn) == list(po) + ["route"]
        assert all(pn[k].default == po[k].default for k in po)
    X.check_request(["slot", "ig", "gradshap", "layergradshap"], True, False, FG._ROWS)


def test_the_tool_parser_adds_the_four_options_and_nothing_else():
    base = vars(G.get_gradshap_parser().parse_args([]))
    tool = vars(FG.get_foldgrad_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base} == base and tool["table_images"] == 0
    # an unchanged command line of the GradientSHAP tool parses to the same values
    line = ["--gradshap", "true", "--layergradshap", "true", "--gradshap_samples", "20", "--gradshap_sigma", "0.25", "--ig", "true",
            "--ig_steps", "9", "--smoothgrad", "true", "--smoothgrad_sigma", "0.5", "--grad", "true", "--layerig", "true", "--cam", "true",
            "--table_images", "8", "--localization", "true", "--model", "resnet18", "--img_size", "64", "--infidelity", "true"]
    old, new = vars(G.get_gradshap_parser().parse_args(line)), vars(FG.get_foldgrad_parser().parse_args(line))
    assert {k: new[k] for k in old} == old and {k: v for k, v in new.items() if k not in old} == TOOL_DEFAULTS
    a = FG.get_foldgrad_parser().parse_args(line + ["--ig_route", "folded", "--gradshap_route", "folded"])
    assert (a.grad_route, a.ig_route, a.smoothgrad_route, a.gradshap_route) == ("autograd", "folded", "autograd", "folded")
    assert X.chosen_families(a, FG.FAMILIES) == X.chosen_families(a, G.FAMILIES)
    with pytest.raises(SystemExit):
        FG.get_foldgrad_parser().parse_args(["--ig_route", "fold"])


def test_the_options_become_the_library_keywords():
    ns = argparse.Namespace()
    assert FG.option_kwargs(ns, "grad") == dict(route="autograd")
    assert FG.option_kwargs(ns, "ig") == dict(n_steps=50, batch=50, route="autograd")
    assert FG.option_kwargs(ns, "smoothgrad") == dict(n_samples=50, sigma=1.0, batch=50, route="autograd")
    assert FG.option_kwargs(ns, "gradshap") == dict(n_samples=50, baselines=10, bank_sigma=1.0, sigma=0.0, batch=50, seed=0,
                                                    route="autograd")
    assert FG.option_kwargs(ns, "layergradshap") == G.option_kwargs(ns, "layergradshap")
    a = FG.get_foldgrad_parser().parse_args(["--grad_route", "folded", "--smoothgrad_route", "folded", "--smoothgrad_samples", "8"])
    assert FG.option_kwargs(a, "grad") == dict(route="folded")
    assert FG.option_kwargs(a, "smoothgrad") == dict(n_samples=8, sigma=1.0, batch=50, route="folded")
    assert G.option_kwargs(a, "smoothgrad") == dict(n_samples=8, sigma=1.0, batch=50)      # the pinned table: no such keyword


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    import sys
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["foldgrad.py", "--ig", "true", "--ig_route", "folded", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        FG.main()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("Cp,A", [(8, 32), (16, 64)])
def test_the_gate_restatement_is_the_gradient_of_the_forward(Cp, A):
    """float64 autograd through relu(gap w1 + b1) w2 -> radix softmax, seeded with da: the restated dgap, dh and dz"""
    g = torch.Generator().manual_seed(Cp)
    B = 3
    gap = torch.randn((B, Cp), generator=g, dtype=torch.float64).requires_grad_(True)
    w1, b1 = torch.randn((Cp, A), generator=g, dtype=torch.float64), torch.randn((A,), generator=g, dtype=torch.float64)
    w2, da = torch.randn((A, 2 * Cp), generator=g, dtype=torch.float64), torch.randn((B, 2 * Cp), generator=g, dtype=torch.float64)
    h = torch.relu(gap @ w1 + b1)
    a = torch.softmax((h @ w2).view(B, 2, Cp), dim=1).reshape(B, 2 * Cp)
    want, = torch.autograd.grad(a, gap, da)
    ref = R.sa_gate_bwd(gap.detach(), w1, b1, w2, a.detach(), da)
    assert torch.allclose(ref["dgap"], want, rtol=1e-10, atol=1e-12) and torch.equal(ref["h"], h.detach())
    assert bool((ref["dgap_mag"] >= ref["dgap"].abs() - 1e-12).all()) and bool((ref["dh_mag"] >= ref["dh"].abs() - 1e-12).all())
    assert (R.gate_group(16), R.gate_group(128), R.gate_group(256), R.gate_group(1024)) == (4, 32, 64, 64)
    assert (R.row_chain(32), R.row_chain(256), R.row_chain(1024)) == (1 + 2 + 3, 1 + 2 + 6, 4 + 2 + 6)
    assert (R.hidden_chain(64, 32), R.hidden_chain(512, 256)) == (1 + 3 + 7 + 1, 64 + 3 + 0 + 1)
