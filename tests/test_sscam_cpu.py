"""SS-CAM and IS-CAM without a GPU: the three sscam_* entry points of csrc/scorecam.hip are declared in include/scouter_hip.h with
their argument lists and exported by the built library, the wrappers and host functions have the specified signatures and defaults,
scouter_amd.test's parser knows --sscam / --iscam and their options while train.py's does not, CPU tensors are refused with an
error naming the call, and iscam_ramp is the fp32 rounding of the reference's own accumulation."""
import ctypes
import inspect

import numpy as np
import pytest

P, I, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double

DECLARED = {
    # image, feat, ranges, out, first_row, n, n_samples, ramp, sigma, seed_lo, seed_hi, Cin, H, W, h, w, C, stream
    "scouter_sscam_mask_images_f32": [P, P, P, P, I, I, I, I, F, I, I, I, I, I, I, I, I, P],
    # logp, cols, wsum, first_row, n, n_classes, K, C, stream
    "scouter_sscam_weights_f64": [P, P, P, I, I, I, I, I, P],
    # wsum, feat, ranges, out, norm, K, h, w, C, stream
    "scouter_sscam_contract_f32": [P, P, P, P, D, I, I, I, I, P],
}


def test_sscam_symbols_are_declared_and_exported():
    import __graft_entry__ as G
    G.build()
    from scouter_amd import _native
    declared = {name: (restype, argtypes) for name, restype, argtypes in _native.declared_symbols()}
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, argtypes in DECLARED.items():
        assert name in declared, name
        assert declared[name] == (ctypes.c_int, argtypes), (name, declared[name])
        assert hasattr(lib, name), name
        assert getattr(_native.lib(), name).argtypes == argtypes


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_sscam_wrappers_and_host_functions_exist():
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as A
    assert list(inspect.signature(K.sscam_mask_images).parameters) == ["image", "feat", "ranges", "out", "first_row", "n_samples",
                                                                       "sigma", "seed", "ramp"]
    assert _defaults(K.sscam_mask_images) == {"sigma": 0.0, "seed": 0, "ramp": False}
    assert list(inspect.signature(K.sscam_weights).parameters) == ["logp", "cols", "wsum", "first_row"]
    assert list(inspect.signature(K.sscam_contract).parameters) == ["wsum", "feat", "ranges", "out", "norm"]
    assert _defaults(K.sscam_contract) == {"norm": 1.0}
    assert list(inspect.signature(A.sscam).parameters) == ["model", "images", "classes", "n_samples", "sigma", "batch", "seed"]
    assert _defaults(A.sscam) == {"classes": None, "n_samples": 35, "sigma": 2.0, "batch": 250, "seed": 0}
    assert list(inspect.signature(A.iscam).parameters) == ["model", "images", "classes", "n_samples", "batch"]
    assert _defaults(A.iscam) == {"classes": None, "n_samples": 10, "batch": 250}
    assert list(inspect.signature(A.sscam_maps).parameters) == ["model", "images", "classes", "size", "min_level", "n_samples",
                                                                "sigma", "batch", "seed"]
    assert _defaults(A.sscam_maps) == {"classes": None, "size": None, "min_level": 0.0, "n_samples": 35, "sigma": 2.0,
                                       "batch": 250, "seed": 0}
    assert list(inspect.signature(A.iscam_maps).parameters) == ["model", "images", "classes", "size", "min_level", "n_samples",
                                                                "batch"]
    assert _defaults(A.iscam_maps) == {"classes": None, "size": None, "min_level": 0.0, "n_samples": 10, "batch": 250}
    assert list(inspect.signature(A.iscam_ramp).parameters) == ["n_samples"]
    # the documented departures from torchcam are in the docstrings
    for word in ("Philox", "one noise field", "per class", "0 / 0", "no final ReLU"):
        assert word in A.sscam.__doc__, word


def test_test_tool_parser_knows_sscam_and_iscam():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.sscam is False and a.sscam_samples == 35 and a.sscam_sigma == 2.0 and a.sscam_batch == 250
    assert a.iscam is False and a.iscam_samples == 10 and a.iscam_batch == 250
    a = T.get_test_parser().parse_args(["--sscam", "true", "--sscam_samples", "3", "--sscam_sigma", "0.5", "--sscam_batch", "100",
                                        "--iscam", "true", "--iscam_samples", "4", "--iscam_batch", "96"])
    assert a.sscam is True and a.sscam_samples == 3 and a.sscam_sigma == 0.5 and a.sscam_batch == 100
    assert a.iscam is True and a.iscam_samples == 4 and a.iscam_batch == 96
    # the other flags keep theirs
    assert a.scorecam is False and a.scorecam_batch == 250 and a.rise is False and a.rise_batch == 250 and a.cam is False
    assert a.causal is False and a.igos is False and a.smoothgrad_samples == 50 and a.smoothgrad_sigma == 1.0
    assert callable(T.run_sscam) and callable(T.run_iscam)


@pytest.mark.parametrize("flag", ["--sscam", "--sscam_samples", "--sscam_sigma", "--sscam_batch", "--iscam", "--iscam_samples",
                                  "--iscam_batch"])
def test_train_parser_does_not_know_sscam_or_iscam(flag):
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args([flag, "true" if flag in ("--sscam", "--iscam") else "3"])


def test_cpu_tensors_are_refused():
    import torch
    from scouter_amd import kernels as K
    feat = torch.zeros((2, 2, 4))
    with pytest.raises(RuntimeError, match="sscam_mask_images"):
        K.sscam_mask_images(torch.zeros((1, 8, 8)), feat, torch.zeros((4, 2)), torch.zeros((4, 1, 8, 8)), 0, 2, sigma=1.0)
    with pytest.raises(RuntimeError, match="sscam_weights"):
        K.sscam_weights(torch.zeros((4, 3)), torch.zeros(3, dtype=torch.int32), torch.zeros((4, 3), dtype=torch.float64), 0)
    with pytest.raises(RuntimeError, match="sscam_contract"):
        K.sscam_contract(torch.zeros((4, 3), dtype=torch.float64), feat, torch.zeros((4, 2)), torch.zeros((3, 2, 2)))


@pytest.mark.parametrize("n", [1, 2, 10])
def test_iscam_ramp_is_the_reference_accumulation(n):
    """the reference accumulates fmap += (i + 1) / n * input * mask: step i carries sum_{t <= i} (t + 1) / n"""
    from scouter_amd.tools.attribution import iscam_ramp
    got = iscam_ramp(n)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n,)
    want, s = [], np.float64(0.0)
    for t in range(n):
        s = s + np.float64(t + 1) / np.float64(n)
        want.append(np.float32(s))
    assert np.array_equal(got, np.array(want, dtype=np.float32)), (got, want)
    if n == 1:
        assert got.tolist() == [1.0]
    with pytest.raises(ValueError):
        iscam_ramp(0)
