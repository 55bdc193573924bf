"""Score-CAM without a GPU: the three entry points of csrc/scorecam.hip are declared in include/scouter_hip.h with their argument
lists and exported by the built library, scouter_amd.test's parser knows --scorecam / --scorecam_batch, and scorecam /
scorecam_maps can be imported from tools/attribution.py."""
import ctypes
import inspect

P, I = ctypes.c_void_p, ctypes.c_int

DECLARED = {
    # feat, ranges, h, w, C, H, W, stream
    "scouter_scorecam_ranges_f32": [P, P, I, I, I, I, I, P],
    # image, feat, ranges, out, first, n, Cin, H, W, h, w, C, stream
    "scouter_scorecam_mask_images_f32": [P, P, P, P, I, I, I, I, I, I, I, I, P],
    # logp, cols, feat, ranges, acc, first, n, n_classes, K, h, w, C, stream
    "scouter_scorecam_accumulate_f32": [P, P, P, P, P, I, I, I, I, I, I, I, P],
}


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


def test_scorecam_wrappers_and_host_functions_exist():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import scorecam, scorecam_maps
    assert list(inspect.signature(K.scorecam_ranges).parameters) == ["feat", "H", "W", "out"]
    assert list(inspect.signature(K.scorecam_mask_images).parameters) == ["image", "feat", "ranges", "out", "first"]
    assert list(inspect.signature(K.scorecam_accumulate).parameters) == ["logp", "cols", "feat", "ranges", "acc", "first"]
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
    with pytest.raises(RuntimeError, match="scorecam_mask_images"):
        K.scorecam_mask_images(torch.zeros((1, 8, 8)), feat, torch.zeros((4, 2)), torch.zeros((4, 1, 8, 8)), 0)
    with pytest.raises(RuntimeError, match="scorecam_accumulate"):
        K.scorecam_accumulate(torch.zeros((4, 3)), torch.zeros(3, dtype=torch.int32), feat, torch.zeros((4, 2)),
                              torch.zeros((3, 2, 2)), 0)
