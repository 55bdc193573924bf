"""Guided backpropagation, the deconvnet rule and Guided Grad-CAM without a device: the tool that adds the three rows
(scouter_amd/tools/guided.py) -- its table, its parser, the keywords its option becomes --, the header's five new entry points,
every refusal that comes before any launch, the host restatements the GPU tests hold the kernels to (tests/guided_restatements.py)
on known answers, the integer nearest index against F.interpolate, and the autograd Function that pins the CPU oracle to a rule on
a two-layer net against gradients computed by hand."""
import argparse
import ctypes
import inspect
import sys

import pytest
import torch
import torch.nn.functional as F

import guided_restatements as R
from scouter_amd import _native
from scouter_amd import kernels as K
from scouter_amd import test as T
from scouter_amd.tools import attribution as AT
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import foldgrad as FG
from scouter_amd.tools import guided as GD

TOOL_DEFAULTS = {"guidedbp": False, "deconvnet": False, "guidedcam": False, "guidedcam_interpolate": "nearest"}


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_extends_the_foldgrad_table_by_three_rows():
    assert GD.FAMILIES[:len(FG.FAMILIES)] == FG.FAMILIES and GD.FAMILIES == FG.FAMILIES + GD.GUIDED
    assert [f.name for f in GD.GUIDED] == ["guidedbp", "deconvnet", "guidedcam"]
    assert not any(f.name in FG._ROWS for f in GD.GUIDED) and not any(f.name in T._ROWS for f in GD.GUIDED)
    want = {"guidedbp": ("guided_backprop", []), "deconvnet": ("deconvnet", []), "guidedcam": ("guided_gradcam", ["interpolate"])}
    for name, (explain, suffixes) in want.items():
        row = T._row(name, GD._ROWS)
        assert (row.explain, row.maps, row.reduce, row.flag, row.estimate) == (explain, "gradient_maps", T._channel_mean, True, False)
        assert [o.suffix for o in row.options] == suffixes
        params = inspect.signature(getattr(AT, row.explain)).parameters     # the library functions take the keywords
        assert all(o.keyword in params and params[o.keyword].default == o.default for o in row.options) and "classes" in params
    o = T._row("guidedcam", GD._ROWS).options[0]
    assert (o.keyword, o.type, o.default, o.choices) == ("interpolate", str, "nearest", ("nearest", "bilinear"))
    assert list(inspect.signature(AT.guided_backprop).parameters) == ["model", "images", "classes", "rule"]
    assert inspect.signature(AT.guided_backprop).parameters["rule"].default == "guided"
    assert list(inspect.signature(AT.deconvnet).parameters) == ["model", "images", "classes"]
    assert list(inspect.signature(AT.guided_gradcam).parameters) == ["model", "images", "classes", "interpolate"]
    X.check_request(["slot", "ig", "guidedbp", "deconvnet", "guidedcam"], True, False, GD._ROWS)
    for name in ("guided_backprop", "deconvnet", "guided_gradcam", "Guided Grad-CAM"):
        assert name in AT.__doc__


def test_the_tool_parser_adds_the_three_rows_and_nothing_else():
    base = vars(FG.get_foldgrad_parser().parse_args([]))
    tool = vars(GD.get_guided_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base} == base and tool["table_images"] == 0
    for k, v in TOOL_DEFAULTS.items():
        assert type(tool[k]) is type(v), k
    line = ["--ig", "true", "--ig_route", "folded", "--gradshap", "true", "--cam", "true", "--table_images", "8", "--model", "resnet18",
            "--img_size", "64", "--infidelity", "true"]
    old, new = vars(FG.get_foldgrad_parser().parse_args(line)), vars(GD.get_guided_parser().parse_args(line))
    assert {k: new[k] for k in old} == old and {k: v for k, v in new.items() if k not in old} == TOOL_DEFAULTS
    a = GD.get_guided_parser().parse_args(line + ["--guidedbp", "true", "--guidedcam", "true", "--guidedcam_interpolate", "bilinear"])
    assert (a.guidedbp, a.deconvnet, a.guidedcam, a.guidedcam_interpolate) == (True, False, True, "bilinear")
    assert X.chosen_families(a, GD.FAMILIES) == X.chosen_families(a, FG.FAMILIES) + ["guidedbp", "guidedcam"]
    with pytest.raises(SystemExit):
        GD.get_guided_parser().parse_args(["--guidedcam_interpolate", "cubic"])
    header = "Guided backpropagation, the deconvnet rule and Guided Grad-CAM as rows of the two explanation tools"
    assert GD.__doc__.startswith(header) and "python -m scouter_amd.tools.guided" in GD.__doc__


def test_the_option_becomes_the_library_keyword():
    ns = argparse.Namespace()
    assert GD.option_kwargs(ns, "guidedbp") == {} and GD.option_kwargs(ns, "deconvnet") == {}
    assert GD.option_kwargs(ns, "guidedcam") == dict(interpolate="nearest")
    a = GD.get_guided_parser().parse_args(["--guidedcam_interpolate", "bilinear", "--ig_steps", "6", "--ig_route", "folded"])
    assert GD.option_kwargs(a, "guidedcam") == dict(interpolate="bilinear")
    assert GD.option_kwargs(a, "ig") == FG.option_kwargs(a, "ig") == dict(n_steps=6, batch=50, route="folded")
    with pytest.raises(ValueError, match="guidedcam"):
        FG.option_kwargs(a, "guidedcam")                                    # the foldgrad tool's table has no such row


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["guided.py", "--guidedbp", "true", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        GD.main()


# ------------------------------------------------------------------------------------------------ the header and the wrappers
def test_the_header_declares_the_five_entry_points():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {"scouter_relu_bwd_rule_f32": [p, p, p, l, i, p],
            "scouter_sa_gate_bwd_rule_f32": [p, p, p, p, p, p, p, p, i, i, i, i, p],
            "scouter_sa_apply_relu_bwd_rule_f32": [p, p, p, p, p, i, i, i, i, p],
            "scouter_maxpool_relu_bwd_rule_f32": [p, p, p, p, i, i, i, i, i, i, i, i, p],
            "scouter_guided_cam_f32": [p, p, p, i, i, i, i, i, i, l, i, p]}
    for name, argtypes in want.items():
        assert name in declared and declared[name] == (ctypes.c_int, argtypes), name
    # the four entry points without a rule keep their signatures
    assert declared["scouter_relu_bwd_f32"] == (ctypes.c_int, [p, p, p, l, p])
    assert declared["scouter_sa_apply_relu_bwd_f32"] == (ctypes.c_int, [p, p, p, p, p, i, i, i, p])
    lib = _native.lib()                                                     # binds every declaration: the library exports them
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes
    assert (K.RULE_GRADIENT, K.RULE_GUIDED, K.RULE_DECONVNET) == (0, 1, 2)
    for fn in (K.relu_bwd, K.sa_gate_bwd, K.sa_apply_relu_bwd, K.maxpool_relu_bwd):    # `rule` is the last keyword and defaults to 0
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "rule" and params["rule"].default == K.RULE_GRADIENT, fn.__name__
    assert list(inspect.signature(K.guided_cam).parameters) == ["grad", "cam", "out", "mode"]
    assert inspect.signature(K.guided_cam).parameters["mode"].default == "nearest"


def test_the_pass_takes_a_rule():
    from scouter_amd.sloter.slot_model import ImagePass
    from scouter_amd.timm.models.layers.split_attn import SplitAttnConv2d
    from scouter_amd.timm.models.resnest import ResNestBottleneck
    from scouter_amd.timm.models.resnet import BasicBlock, Downsample, ResNet
    assert list(inspect.signature(ImagePass.grad).parameters) == ["self", "seed"]       # pinned by tests/test_foldgrad_cpu.py: the rule is grad_from's
    assert list(inspect.signature(ImagePass.grad_from).parameters) == ["self", "dfeat", "rule"]
    assert list(inspect.signature(ImagePass.feature_grad).parameters) == ["self", "seed"]
    assert inspect.signature(ImagePass.grad_from).parameters["rule"].default == "gradient"
    assert ImagePass.RULES == {"gradient": K.RULE_GRADIENT, "guided": K.RULE_GUIDED, "deconvnet": K.RULE_DECONVNET}
    for fn in (ResNet.image_bwd, BasicBlock.bwd_image, ResNestBottleneck.bwd_image, SplitAttnConv2d.bwd_image):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "rule" and params["rule"].default == K.RULE_GRADIENT, fn.__qualname__
    assert "rule" not in inspect.signature(Downsample.bwd_image).parameters  # no ReLU there


def test_every_host_side_refusal():
    x = torch.zeros((1, 3, 16, 16))                                         # on the host: a launch would raise from the library
    for bad in ("Guided", "gbp", "", None, 1):
        with pytest.raises(ValueError, match="rule"):
            AT.guided_backprop(None, x, rule=bad)
    for bad in ("linear", "Nearest", "", None, 0):
        with pytest.raises(ValueError, match="interpolate"):
            AT.guided_gradcam(None, x, interpolate=bad)
    for fn in (AT.guided_backprop, AT.deconvnet, AT.guided_gradcam):
        with pytest.raises(RuntimeError, match="HIP device"):               # a host tensor: no model is touched (it is None)
            fn(None, x)
        with pytest.raises(ValueError, match="images"):
            fn(None, x[0])
    # the kernels' wrappers: the rule is checked before any tensor is looked at, a host tensor is refused by name
    t = torch.zeros(8)
    for bad in (3, -1, "guided", None, 1.0, True):
        for call in (lambda r: K.relu_bwd(t, t, r), lambda r: K.sa_gate_bwd(t, t, t, t, t, t, rule=r),
                     lambda r: K.sa_apply_relu_bwd(t, t, t, t, r), lambda r: K.maxpool_relu_bwd(t, t, t, rule=r)):
            with pytest.raises(ValueError, match="rule"):
                call(bad)
    with pytest.raises(RuntimeError, match="dy"):
        K.relu_bwd(t, t, K.RULE_GUIDED)
    with pytest.raises(ValueError, match="mode"):
        K.guided_cam(torch.zeros((1, 1, 4, 4)), torch.zeros((1, 2, 2)), mode="cubic")
    with pytest.raises(RuntimeError, match="guided_cam: grad"):
        K.guided_cam(torch.zeros((1, 1, 4, 4)), torch.zeros((1, 2, 2)))


# ------------------------------------------------------------------------------------------------ the restatements
def test_the_rule_restatement_on_the_four_quadrants():
    nan = float("nan")
    #                    (T, T) (T, F) (F, T) (F, F)  +0 / -0 in g         NaN in g    -0 / subnormal in act
    act = torch.tensor([1.0, 2.0, 0.0, 0.0, 3.0, 4.0, 0.0, 0.0, 5.0, -0.0, -0.0, 2.0 ** -149, -1.0])
    g = torch.tensor([1.5, -2.5, 3.5, -4.5, 0.0, -0.0, 0.0, -0.0, nan, nan, 6.5, -7.5, 8.5])
    assert R.quadrants(g[:4], act[:4]) == [1, 1, 1, 1] and R.zeros_of_both_signs(g) and R.zeros_of_both_signs(act)
    want = {"gradient": [1.5, -2.5, 0.0, 0.0, 0.0, -0.0, 0.0, 0.0, nan, 0.0, 0.0, -7.5, 0.0],
            "guided": [1.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
            "deconvnet": [1.5, 0.0, 3.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 6.5, 0.0, 8.5]}
    for rule, vals in want.items():
        for form in (rule, R.RULES[rule]):
            got = R.rule_select(g, act, form)
            assert torch.equal(got.view(torch.int32), torch.tensor(vals).view(torch.int32)), (rule, got.tolist())
    # under the two new rules nothing negative, no NaN and no -0 leaves a ReLU
    for rule in ("guided", "deconvnet"):
        out = R.rule_select(g, act, rule)
        assert bool((out >= 0).all()) and not bool(torch.signbit(out).any())
    with pytest.raises(ValueError):
        R.rule_select(g, act, 3)


def test_the_gate_restatement_under_a_rule():
    gen = torch.Generator().manual_seed(5)
    B, Cp, A = 3, 8, 32
    gap, w1, b1 = (torch.randn(s, generator=gen) for s in ((B, Cp), (Cp, A), (A,)))
    w2, da = torch.randn((A, 2 * Cp), generator=gen), torch.randn((B, 2 * Cp), generator=gen)
    a = torch.softmax(torch.randn((B, 2, Cp), generator=gen), dim=1).reshape(B, 2 * Cp)
    import foldgrad_restatements as R0
    base, plain = R0.sa_gate_bwd(gap, w1, b1, w2, a, da), R.sa_gate_bwd(gap, w1, b1, w2, a, da, "gradient")
    for k in base:
        assert torch.equal(base[k], plain[k]), k                            # rule 0 is the restatement it extends
    g, pos = plain["g"], plain["pre"] > 0
    guided, deconv = R.sa_gate_bwd(gap, w1, b1, w2, a, da, "guided"), R.sa_gate_bwd(gap, w1, b1, w2, a, da, "deconvnet")
    assert torch.equal(guided["dh"], g.clamp_min(0.0) * pos) and torch.equal(deconv["dh"], g.clamp_min(0.0))
    assert torch.equal(guided["dh_mag"], base["dh_mag"]) and torch.equal(guided["dh_in"], base["dh_in"])          # no g > 0 factor
    assert bool((deconv["dh_mag"] >= base["dh_mag"]).all()) and bool((deconv["dh_mag"][~pos] > 0).all())         # nor [h > 0]
    assert torch.equal(deconv["dgap"], deconv["dh"] @ w1.double().t())
    assert R.quadrants(g, plain["pre"]) and min(R.quadrants(g, plain["pre"])) > 0


@pytest.mark.parametrize("h,H", [(7, 224), (3, 96), (2, 64), (1, 5)])
def test_the_integer_nearest_index_is_interpolates(h, H):
    src = torch.arange(h, dtype=torch.float32)
    want = F.interpolate(src.view(1, 1, h, 1), size=(H, 1), mode="nearest").view(H).long()
    assert torch.equal(R.nearest_index(H, h), want)
    cam = torch.arange(h * h, dtype=torch.float32).view(1, h, h)
    assert torch.equal(R.upsample_nearest(cam, H, H), F.interpolate(cam[None], size=(H, H), mode="nearest")[0])


def test_the_rule_function_on_a_two_layer_net():
    """y = w2 . relu(W1 x): W1 = [[1, 0], [0, 1], [1, 1]], x = (1, -2), w2 = (1, -1, 2).  Pre-activations (1, -2, -1): the mask is
    (1, 0, 0); the gradient arriving at the ReLU is w2 = (1, -1, 2)."""
    W1 = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
    w2 = torch.tensor([1.0, -1.0, 2.0], dtype=torch.float64)
    #  leaving the ReLU:  gradient (1, 0, 0)   guided (1, 0, 0) [and (0, 0, 0) for -w2]   deconvnet (1, 0, 2)
    want = {"gradient": [1.0, 0.0], "guided": [1.0, 0.0], "deconvnet": [3.0, 2.0]}
    flipped = {"gradient": [-1.0, 0.0], "guided": [0.0, 0.0], "deconvnet": [0.0, 1.0]}
    for rule in want:
        for sign, table in ((1.0, want), (-1.0, flipped)):
            x = torch.tensor([1.0, -2.0], dtype=torch.float64, requires_grad=True)
            pre = W1 @ x
            y = (sign * w2 * R.Rule.apply(pre, pre.detach() > 0, rule)).sum()
            assert float(y.detach()) == sign * 1.0                                  # the forward is relu's
            y.backward()
            assert x.grad.tolist() == table[rule], (rule, sign, x.grad.tolist())
