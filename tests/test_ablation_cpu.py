"""Occlusion maps and Ablation-CAM without a device: the window geometry against a brute-force count, the refusals that come before
any launch, the header's four entry points, and the tool that adds the two rows (scouter_amd/tools/ablation.py) -- its parser, the
keywords its options become, and the three pinned tables it must leave alone."""
import argparse
import ctypes
import inspect

import pytest
import torch

from scouter_amd import _native
from scouter_amd import kernels as K
from scouter_amd import test as T
from scouter_amd.tools import ablation as A
from scouter_amd.tools import attribution as AT
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import surrogate as S

NAMES = ["slot", "grad", "cam", "rise", "scorecam", "ig", "smoothgrad", "campp", "smoothcampp", "extremal", "iba", "igos", "sscam",
         "iscam"]


# ------------------------------------------------------------------------------------------------ the windows
def test_occlusion_windows_against_a_brute_force_count():
    """every (size, window, stride) with size < 24: the number of windows is the smallest whose union is the axis, and the
    windows that cover a pixel are exactly the closed range the header states, never empty"""
    for size in range(1, 24):
        for window in range(1, size + 1):
            for stride in range(1, window + 1):
                n, other = AT.occlusion_windows((size, 23), (window, 5), (stride, 3))
                assert other == 7                                           # 1 + ceil(18 / 3): the axes do not mix
                count = 1
                while (count - 1) * stride + window < size:
                    count += 1
                assert n == count, (size, window, stride)
                covered = [[i for i in range(n) if i * stride <= y < min(i * stride + window, size)] for y in range(size)]
                for y, cover in enumerate(covered):
                    lo, hi = max(0, -(-(y - window + 1) // stride)), min(n - 1, y // stride)
                    assert cover and cover == list(range(lo, hi + 1)), (size, window, stride, y)
    assert AT.occlusion_windows((224, 224), 16, 8) == (27, 27) and AT.occlusion_windows((64, 64), 16, 8) == (7, 7)
    assert AT.occlusion_windows((33, 47), (16, 16), (8, 8)) == (4, 5) and AT.occlusion_windows((16, 16), 16, 16) == (1, 1)
    assert AT.occlusion_windows(torch.Size([5, 7]), (2, 3), (1, 2)) == (4, 3)
    assert K.occlusion_windows((64, 64), 16, 8) == (7, 7)


@pytest.mark.parametrize("size,window,stride", [((8, 8), 4, 5), ((8, 8), 9, 2), ((8, 8), 4, 0), ((8, 8), 0, 0), ((8, 8), (4, 9), 2),
                                                ((8, 8), 4, (2, 5)), ((8, 8), 4, -1), ((0, 8), 1, 1), ((8, 8), (4, 4, 4), 2),
                                                ((8, 8), "wide", 2), ((8, 8), 4, None)])
def test_occlusion_windows_refuses_bad_geometry(size, window, stride):
    with pytest.raises(ValueError, match="occlusion_windows"):
        AT.occlusion_windows(size, window, stride)
    with pytest.raises(ValueError, match="occlude_images"):
        K.occlusion_windows(size, window, stride, "occlude_images")


def test_the_methods_refuse_before_any_launch():
    x = torch.zeros((1, 3, 16, 16))                                         # on the host: a launch would raise RuntimeError
    for window, stride in ((8, 9), (17, 4), (8, 0), ((8, 17), 4)):
        with pytest.raises(ValueError, match="stride"):
            AT.occlusion(None, x, window=window, stride=stride)
    with pytest.raises(ValueError, match="of"):
        AT.occlusion(None, x, of="logit")
    with pytest.raises(ValueError, match="fill"):
        AT.occlusion(None, x, fill=float("nan"))
    for batch in (1, 0, -3):
        with pytest.raises(ValueError, match="batch"):
            AT.occlusion(None, x, batch=batch)
    with pytest.raises(ValueError, match="images"):
        AT.occlusion(None, x[0])
    with pytest.raises(ValueError, match="images"):
        AT.ablationcam(None, x[0])
    with pytest.raises(RuntimeError, match="occlude_images"):              # the wrappers: a host tensor is refused by name
        K.occlude_images(x[0], torch.zeros((2, 3, 16, 16)), 0, 8, 4)
    with pytest.raises(RuntimeError, match="ablate_channels"):
        K.ablate_channels(torch.zeros((2, 2, 8)), torch.zeros((2, 2, 2, 8)), 0)


# ------------------------------------------------------------------------------------------------ the header
def test_the_header_declares_the_four_kernels():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    want = {"scouter_occlude_images_f32": [p, p] + [i] * 9 + [f, p],
            "scouter_occlusion_finish_f32": [p, p] + [i] * 7 + [p],
            "scouter_ablate_channels_f32": [p, p] + [i] * 4 + [p],
            "scouter_ablation_contract_f32": [p] * 5 + [i] * 5 + [p]}
    for name, argtypes in want.items():
        assert name in declared and declared[name] == (ctypes.c_int, argtypes), name
    lib = _native.lib()                                                     # binds every declaration: the library exports them
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes


# ------------------------------------------------------------------------------------------------ the tool
TOOL_DEFAULTS = {"occlusion": False, "ablationcam": False, "occlusion_window": 16, "occlusion_stride": 8, "occlusion_fill": 0.0,
                 "occlusion_batch": 250, "ablationcam_batch": 256}


def test_the_three_pinned_tables_are_unchanged():
    assert len(T.FAMILIES) == 14 and [f.name for f in T.FAMILIES] == NAMES
    assert [f.name for f in X.FAMILIES] == NAMES + ["fccam"]
    assert [f.name for f in S.FAMILIES] == NAMES + ["fccam", "lime", "shap"] and S.FAMILIES == X.FAMILIES + S.SURROGATES
    for rows in (T._ROWS, X._ROWS, S._ROWS):
        assert "occlusion" not in rows and "ablationcam" not in rows
    for parser in (T.get_test_parser(), X.get_table_parser(), S.get_surrogate_parser()):
        known = vars(parser.parse_args([]))
        assert not any(k.startswith(("occlusion", "ablationcam")) for k in known)
    with pytest.raises(ValueError, match="occlusion"):
        T._row("occlusion")
    with pytest.raises(ValueError, match="ablationcam"):
        T._row("ablationcam", S._ROWS)


def test_the_tool_extends_the_table_by_two_rows():
    assert A.FAMILIES == S.FAMILIES + A.ABLATIONS and [f.name for f in A.ABLATIONS] == ["occlusion", "ablationcam"]
    occ, abl = T._row("occlusion", A._ROWS), T._row("ablationcam", A._ROWS)
    assert (occ.explain, occ.maps, occ.reduce, occ.flag, occ.estimate) == ("occlusion", "occlusion_maps", None, True, False)
    assert (abl.explain, abl.maps, abl.reduce, abl.flag, abl.estimate) == ("ablationcam", "ablationcam_maps", None, True, False)
    assert [o.suffix for o in occ.options] == ["window", "stride", "fill", "batch"]
    assert [o.suffix for o in abl.options] == ["batch"]
    for row in (occ, abl):                                                  # the library functions exist and take the keywords
        params = inspect.signature(getattr(AT, row.explain)).parameters
        assert all(o.keyword in params for o in row.options), row.name
        assert "classes" in params and callable(getattr(AT, row.maps))
    assert inspect.signature(AT.occlusion).parameters["of"].default == "prob"
    assert [inspect.signature(AT.occlusion).parameters[k].default for k in ("window", "stride", "fill", "batch")] == [16, 8, 0.0, 250]
    assert [inspect.signature(AT.ablationcam).parameters[k].default for k in ("batch", "relu")] == [256, True]
    X.check_request(["slot", "lime", "occlusion", "ablationcam"], True, False, A._ROWS)
    with pytest.raises(ValueError, match="sensitivity"):
        X.check_request(["occlusion"], True, True, A._ROWS)


def test_the_tool_parser_adds_the_two_rows_and_nothing_else():
    base = vars(S.get_surrogate_parser().parse_args([]))
    tool = vars(A.get_ablation_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base} == base and tool["table_images"] == 0
    for k, v in TOOL_DEFAULTS.items():
        assert type(tool[k]) is type(v), k
    a = A.get_ablation_parser().parse_args(["--occlusion", "true", "--ablationcam", "true", "--occlusion_window", "32",
                                            "--occlusion_fill", "-0.5", "--ablationcam_batch", "64", "--lime", "true", "--rise_masks",
                                            "6", "--cam", "true", "--table_images", "8", "--localization", "true"])
    assert (a.occlusion, a.ablationcam, a.occlusion_window, a.occlusion_fill, a.ablationcam_batch) == (True, True, 32, -0.5, 64)
    assert (a.lime, a.rise_masks, a.cam, a.table_images, a.localization) == (True, 6, True, 8, True)
    assert X.chosen_families(a, A.FAMILIES) == ["slot", "cam", "lime", "occlusion", "ablationcam"]
    assert X.chosen_families(a, S.FAMILIES) == ["slot", "cam", "lime"]      # the surrogate tool's own families: as before


def test_the_options_become_the_library_keywords():
    assert A.option_kwargs(argparse.Namespace(), "occlusion") == dict(window=16, stride=8, fill=0.0, batch=250)
    assert A.option_kwargs(argparse.Namespace(), "ablationcam") == dict(batch=256)
    a = A.get_ablation_parser().parse_args(["--occlusion_window", "24", "--occlusion_stride", "12", "--occlusion_fill", "1",
                                            "--occlusion_batch", "20", "--ablationcam_batch", "128", "--lime_samples", "64"])
    assert A.option_kwargs(a, "occlusion") == dict(window=24, stride=12, fill=1.0, batch=20)
    assert A.option_kwargs(a, "ablationcam") == dict(batch=128)
    assert A.option_kwargs(a, "rise") == dict(n_masks=4000, batch=250)      # the inherited rows read as before
    assert A.option_kwargs(a, "lime")["n_samples"] == 64
    assert T.option_kwargs(a, "occlusion", A._ROWS) == A.option_kwargs(a, "occlusion")
    with pytest.raises(ValueError, match="occlusion"):
        T.option_kwargs(a, "occlusion")                                     # the single-image tool's own table has no such row
    with pytest.raises(ValueError, match="ablationcam"):
        S.option_kwargs(a, "ablationcam")


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    import sys
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["ablation.py", "--occlusion", "true", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        A.main()
    monkeypatch.setattr(sys, "argv", ["ablation.py", "--ablationcam", "true", "--table_images", "4", "--sensitivity", "true"])
    with pytest.raises(ValueError, match="sensitivity"):
        A.main()
