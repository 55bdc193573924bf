"""LIME and KernelSHAP without a device: the host-drawn sample matrices, the refusals that come before any launch, the header's
six entry points, and the tool that adds the two rows (scouter_amd/tools/surrogate.py) -- its parser, the keywords its options
become, and the two pinned tables it must leave alone."""
import argparse
import ctypes

import pytest
import torch

from scouter_amd import _native
from scouter_amd import test as T
from scouter_amd.tools import attribution as A
from scouter_amd.tools import explanation_table as X
from scouter_amd.tools import surrogate as S

NAMES = ["slot", "grad", "cam", "rise", "scorecam", "ig", "smoothgrad", "campp", "smoothcampp", "extremal", "iba", "igos", "sscam",
         "iscam"]


# ------------------------------------------------------------------------------------------------ the samples
@pytest.mark.parametrize("d", [1, 2, 12, 64, 128])
def test_lime_samples(d):
    z = A.lime_samples(40, d, seed=3)
    assert z.dtype == torch.uint8 and tuple(z.shape) == (40, d) and not z.is_cuda and int(z.max()) == 1
    assert bool(z[0].all())                                                 # row 0: the image itself
    assert z.numpy().tobytes() == A.lime_samples(40, d, seed=3).numpy().tobytes()
    if d >= 12:
        assert z.numpy().tobytes() != A.lime_samples(40, d, seed=4).numpy().tobytes()
        assert 0.3 < float(z[1:].float().mean()) < 0.7
    want = (torch.rand(40, d, generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8)
    assert torch.equal(z[1:], want[1:])


@pytest.mark.parametrize("d", [2, 3, 12, 64, 128])
def test_kernelshap_samples(d):
    N = d + 2 + 30
    z = A.kernelshap_samples(N, d, seed=5)
    assert z.dtype == torch.uint8 and tuple(z.shape) == (N, d) and not z.is_cuda
    assert bool(z[0].all()) and not bool(z[1].any())                        # row 0 all ones, row 1 all zeros
    sizes = z[2:].sum(dim=1)
    assert int(sizes.min()) >= 1 and int(sizes.max()) <= d - 1              # every drawn row: a size in [1, d - 1]
    assert int(z.max()) == 1
    assert z.numpy().tobytes() == A.kernelshap_samples(N, d, seed=5).numpy().tobytes()
    if d >= 12:
        assert z.numpy().tobytes() != A.kernelshap_samples(N, d, seed=6).numpy().tobytes()
    assert tuple(A.kernelshap_samples(d + 2, d).shape) == (d + 2, d)        # the smallest N


def test_kernelshap_sizes_follow_the_shapley_kernel():
    """the size law, probability proportional to (d - 1) / (m (d - m)), at d = 10: the frequencies of the sizes over 20000 rows
    lie within 5 standard deviations of a binomial (the seed is fixed, so the test cannot flicker)"""
    d, N = 10, 20002
    sizes = A.kernelshap_samples(N, d, seed=1)[2:].sum(dim=1)
    m = torch.arange(1, d, dtype=torch.float64)
    p = (d - 1) / (m * (d - m))
    p = p / p.sum()
    freq = torch.bincount(sizes, minlength=d)[1:].double() / (N - 2)
    assert bool(((freq - p).abs() <= 5 * (p * (1 - p) / (N - 2)).sqrt()).all())


def test_kernelshap_samples_for_one_segment():
    z = A.kernelshap_samples(2, 1)
    assert z.tolist() == [[1], [0]] and A.kernelshap_samples(50, 1).tolist() == [[1], [0]]      # only rows 0 and 1 are used


@pytest.mark.parametrize("N,d", [(0, 4), (-3, 4), (10, 0), (10, 129), (10, -1)])
def test_the_sample_generators_refuse_bad_sizes(N, d):
    with pytest.raises(ValueError):
        A.lime_samples(N, d)
    with pytest.raises(ValueError):
        A.kernelshap_samples(N, d)


@pytest.mark.parametrize("N,d", [(13, 12), (5, 4), (2, 2), (1, 1)])
def test_kernelshap_needs_d_plus_two_samples(N, d):
    with pytest.raises(ValueError, match="d \\+ 2"):
        A.kernelshap_samples(N, d)
    A.lime_samples(N, d)                                                    # LIME has no such rule


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_superpixels_refuses_before_any_launch():
    x = torch.zeros((2, 3, 16, 16))                                         # on the host: a launch would raise RuntimeError
    for segments in [(12, 12), (1, 129), (0, 4), (4, 0), (17, 2), (2, 17)]:
        with pytest.raises(ValueError):
            A.superpixels(x, segments)
    with pytest.raises(ValueError, match="128"):
        A.superpixels(x, (12, 12))                                          # d = 144 > 128
    with pytest.raises(ValueError):
        A.superpixels(x, (4, 4), iters=-1)
    with pytest.raises(ValueError):
        A.superpixels(x[0], (4, 4))
    labels = torch.zeros((2, 16, 16), dtype=torch.int32)
    with pytest.raises(ValueError, match="d="):
        A.superpixels(x, labels)
    with pytest.raises(ValueError, match="128"):
        A.superpixels(x, labels, d=129)
    with pytest.raises(ValueError, match="int32"):
        A.superpixels(x, labels.long(), d=4)
    with pytest.raises(ValueError, match="int32"):
        A.superpixels(x, labels[:1], d=4)
    for bad in (4, -1):                                                     # a label out of [0, d)
        wrong = labels.clone()
        wrong[1, 3, 5] = bad
        with pytest.raises(ValueError, match="outside"):
            A.superpixels(x, wrong, d=4)


def test_the_fits_refuse_before_any_launch():
    x = torch.zeros((1, 3, 16, 16))
    with pytest.raises(ValueError, match="128"):
        A.lime_fit(None, x, segments=(12, 12))
    with pytest.raises(ValueError, match="128"):
        A.kernelshap_fit(None, x, segments=(12, 12))
    seg = A.Superpixels(torch.zeros((1, 16, 16), dtype=torch.int32), 12, torch.zeros((1, 12, 3)))
    with pytest.raises(ValueError, match="d \\+ 2"):
        A.kernelshap_fit(None, x, n_samples=13, segments=seg)               # N < d + 2
    with pytest.raises(ValueError, match="kernel_width"):
        A.lime_fit(None, x, segments=seg, kernel_width=0.0)
    with pytest.raises(ValueError, match="samples"):
        A.lime_fit(None, x, segments=seg, samples=torch.ones((5, 11), dtype=torch.uint8))
    with pytest.raises(ValueError, match="row 0"):
        A.kernelshap_fit(None, x, segments=seg, samples=torch.ones((20, 12), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the header
def test_the_header_declares_the_six_kernels():
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    for name in ("scouter_slic_update_f32", "scouter_slic_assign_f32", "scouter_segment_images_f32",
                 "scouter_surrogate_accumulate_f64", "scouter_surrogate_solve_f64", "scouter_segment_paint_f32"):
        assert name in declared and declared[name][0] is ctypes.c_int, name
        assert declared[name][1][-1] is ctypes.c_void_p                     # the stream comes last
    assert declared["scouter_surrogate_solve_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    acc = declared["scouter_surrogate_accumulate_f64"][1]
    assert acc[6] is ctypes.c_long and acc[-2] is ctypes.c_double and len(acc) == 14
    assert declared["scouter_slic_assign_f32"][1][-2] is ctypes.c_float


# ------------------------------------------------------------------------------------------------ the tool
SHARED = {"samples": 1000, "batch": 250, "segments": 8, "slic_iters": 10, "compactness": 1.0}
TOOL_DEFAULTS = dict({"lime": False, "shap": False, "lime_ridge": 1.0, "shap_ridge": 0.0, "lime_kernel_width": 0.25, "shap_hide": 0.0},
                     **{"%s_%s" % (row, k): v for row in ("lime", "shap") for k, v in SHARED.items()})


def test_the_two_pinned_tables_are_unchanged():
    assert len(T.FAMILIES) == 14 and [f.name for f in T.FAMILIES] == NAMES
    assert [f.name for f in X.FAMILIES] == NAMES + ["fccam"]
    assert "lime" not in T._ROWS and "shap" not in T._ROWS and "lime" not in X._ROWS and "shap" not in X._ROWS
    for parser in (T.get_test_parser(), X.get_table_parser()):
        known = vars(parser.parse_args([]))
        assert not any(k.startswith(("lime", "shap")) for k in known)
    with pytest.raises(ValueError, match="lime"):
        T._row("lime")
    with pytest.raises(ValueError, match="shap"):
        X.check_request(["shap"], True)


def test_the_tool_extends_the_table_by_two_rows():
    assert S.FAMILIES == X.FAMILIES + S.SURROGATES and [f.name for f in S.SURROGATES] == ["lime", "shap"]
    lime, shap = T._row("lime", S._ROWS), T._row("shap", S._ROWS)
    assert (lime.explain, lime.maps, lime.reduce, lime.flag, lime.estimate) == ("lime", "lime_maps", None, True, False)
    assert (shap.explain, shap.maps, shap.reduce, shap.flag, shap.estimate) == ("kernelshap", "kernelshap_maps", None, True, False)
    assert [o.suffix for o in lime.options] == ["samples", "batch", "segments", "slic_iters", "compactness", "ridge", "kernel_width"]
    assert [o.suffix for o in shap.options] == ["samples", "batch", "segments", "slic_iters", "compactness", "ridge", "hide"]
    import inspect
    for row in (lime, shap):                                                # the library functions exist and take the keywords
        params = inspect.signature(getattr(A, row.explain + "_fit")).parameters
        assert all(o.keyword in params for o in row.options), row.name
        assert callable(getattr(A, row.explain)) and callable(getattr(A, row.maps))
    X.check_request(["slot", "lime", "shap"], True, False, S._ROWS)
    with pytest.raises(ValueError, match="sensitivity"):
        X.check_request(["lime"], True, True, S._ROWS)


def test_the_tool_parser_adds_the_two_rows_and_nothing_else():
    base = vars(X.get_table_parser().parse_args([]))
    tool = vars(S.get_surrogate_parser().parse_args([]))
    assert {k: v for k, v in tool.items() if k not in base} == TOOL_DEFAULTS
    assert {k: tool[k] for k in base if k != "table_images"} == {k: v for k, v in base.items() if k != "table_images"}
    assert tool["table_images"] == 0 and base["table_images"] == 64         # the single-image mode is this tool's default
    for k, v in TOOL_DEFAULTS.items():
        assert type(tool[k]) is type(v), k
    a = S.get_surrogate_parser().parse_args(["--lime", "true", "--shap", "true", "--lime_samples", "64", "--shap_segments", "4",
                                             "--shap_hide", "-0.5", "--lime_kernel_width", "0.5", "--rise_masks", "6", "--cam", "true",
                                             "--table_images", "8", "--localization", "true"])
    assert (a.lime, a.shap, a.lime_samples, a.shap_segments, a.shap_hide, a.lime_kernel_width) == (True, True, 64, 4, -0.5, 0.5)
    assert (a.rise_masks, a.cam, a.table_images, a.localization) == (6, True, 8, True)
    assert X.chosen_families(a, S.FAMILIES) == ["slot", "cam", "lime", "shap"]
    assert X.chosen_families(a) == ["slot", "cam"]                          # the table tool's own families: as before


def test_the_options_become_the_library_keywords():
    assert S.option_kwargs(argparse.Namespace(), "lime") == dict(n_samples=1000, batch=250, segments=8, slic_iters=10,
                                                                 compactness=1.0, ridge=1.0, kernel_width=0.25)
    assert S.option_kwargs(argparse.Namespace(), "shap") == dict(n_samples=1000, batch=250, segments=8, slic_iters=10,
                                                                 compactness=1.0, ridge=0.0, hide=0.0)
    a = S.get_surrogate_parser().parse_args(["--lime_samples", "64", "--lime_batch", "16", "--lime_segments", "3", "--lime_ridge", "0",
                                             "--shap_slic_iters", "0", "--shap_compactness", "2.5", "--shap_hide", "1"])
    assert S.option_kwargs(a, "lime") == dict(n_samples=64, batch=16, segments=3, slic_iters=10, compactness=1.0, ridge=0.0,
                                              kernel_width=0.25)
    assert S.option_kwargs(a, "shap") == dict(n_samples=1000, batch=250, segments=8, slic_iters=0, compactness=2.5, ridge=0.0,
                                              hide=1.0)
    assert S.option_kwargs(a, "rise") == dict(n_masks=4000, batch=250)      # the inherited rows read as before
    with pytest.raises(ValueError, match="lime"):
        T.option_kwargs(a, "lime")                                          # the single-image tool's own table has no such row


def test_the_tool_refuses_before_it_builds_a_model(monkeypatch):
    import sys
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["surrogate.py", "--lime", "true", "--table_images", "4", "--sensitivity", "true"])
    with pytest.raises(ValueError, match="sensitivity"):
        S.main()
    monkeypatch.setattr(sys, "argv", ["surrogate.py", "--lime", "true", "--table_images", "-1"])
    with pytest.raises(ValueError, match="table_images"):
        S.main()
