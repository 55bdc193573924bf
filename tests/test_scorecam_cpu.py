"""Score-CAM without a GPU: scouter_scorecam_ranges_f32 of csrc/scorecam.hip is declared in include/scouter_hip.h with its
argument list and exported by the built library (the sscam_* entry points Score-CAM runs on: test_sscam_cpu.py), the two entry points
Score-CAM once had for itself are gone from both, scouter_amd.test's parser knows --scorecam / --scorecam_batch, and scorecam /
scorecam_maps can be imported from tools/attribution.py."""
import ctypes
import inspect

P, I = ctypes.c_void_p, ctypes.c_int

DECLARED = {
    # feat, ranges, h, w, C, H, W, stream
    "scouter_scorecam_ranges_f32": [P, P, I, I, I, I, I, P],
}
# the mask writer and the accumulation Score-CAM had for itself: sscam_mask_images, sscam_weights and sscam_contract do their work
REMOVED = ["scouter_scorecam_%s_f32" % part for part in ("mask_images", "accumulate")]


def test_scorecam_symbols_are_declared_and_exported():
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
    for name in REMOVED:                          # (an object file left behind by an earlier build would still export them)
        assert name not in declared, name
        assert not hasattr(lib, name), name


def test_scorecam_wrappers_and_host_functions_exist():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import scorecam, scorecam_maps
    assert list(inspect.signature(K.scorecam_ranges).parameters) == ["feat", "H", "W", "out"]
    sig = inspect.signature(scorecam)
    assert list(sig.parameters) == ["model", "images", "classes", "batch"]
    assert sig.parameters["classes"].default is None and sig.parameters["batch"].default == 250
    sig = inspect.signature(scorecam_maps)
    assert list(sig.parameters) == ["model", "images", "classes", "size", "min_level", "batch"]
    assert sig.parameters["min_level"].default == 0.0 and sig.parameters["batch"].default == 250


def test_test_tool_parser_knows_scorecam():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.scorecam is False and a.scorecam_batch == 250
    a = T.get_test_parser().parse_args(["--scorecam", "true", "--scorecam_batch", "96"])
    assert a.scorecam is True and a.scorecam_batch == 96
    assert a.rise is False and a.rise_batch == 250 and a.cam is False and a.causal is False     # the other flags keep theirs
    assert callable(T.run_scorecam)


def test_train_parser_does_not_know_scorecam():
    import pytest
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--scorecam", "true"])


def test_cpu_tensors_are_refused():
    import pytest
    import torch
    from scouter_amd import kernels as K
    feat = torch.zeros((2, 2, 4))
    with pytest.raises(RuntimeError, match="scorecam_ranges"):
        K.scorecam_ranges(feat, 8, 8)
