"""Grad-CAM++ / Smooth Grad-CAM++ without a GPU: the three entry points of csrc/gradcampp.hip are declared in
include/scouter_hip.h with their argument lists and exported by the built library, the wrappers and tools have their signatures
and defaults, scouter_amd.test's parser knows the five new flags (train.py's does not), and gradcampp / smooth_gradcampp refuse
bad arguments before any device call."""
import ctypes
import inspect
import types

import pytest

P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long

DECLARED = {
    # feat, dfeat, out, B, N, C, out_stride, relu, stream
    "scouter_gradcampp_f32": [P, P, P, I, I, I, L, I, P],
    # grads, acc2, acc3, n, E, stream
    "scouter_grad_powers_accumulate": [P, P, P, I, L, P],
    # feat, acc2, acc3, glast, out, n_samples, B, N, C, out_stride, relu, stream
    "scouter_gradcampp_smooth_f32": [P, P, P, P, P, I, I, I, I, L, I, P],
}


def test_gradcampp_symbols_are_declared_and_exported():
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


def test_gradcampp_wrappers_and_tools_have_their_signatures():
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as A

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(K.gradcampp) == [("feat", E), ("dfeat", E), ("out", E), ("relu", True)]
    assert params(K.grad_powers_accumulate) == [("grads", E), ("acc2", E), ("acc3", E)]
    assert params(K.gradcampp_smooth) == [("feat", E), ("acc2", E), ("acc3", E), ("glast", E), ("out", E), ("n_samples", E),
                                          ("relu", True)]
    assert params(K.gradcam) == [("feat", E), ("dfeat", E), ("out", E), ("relu", False)]          # (as it was)
    assert params(A.gradcampp) == [("model", E), ("images", E), ("classes", None), ("relu", True)]
    assert params(A.smooth_gradcampp) == [("model", E), ("images", E), ("classes", None), ("n_samples", 4), ("sigma", 0.3),
                                          ("batch", 4), ("seed", 0), ("relu", True)]
    assert params(A.gradcam) == [("model", E), ("images", E), ("classes", None), ("relu", False)]
    assert callable(A.gradcampp_maps) and callable(A.smooth_gradcampp_maps)
    for word in ("gradcampp", "smooth_gradcampp", "gradcampp_maps", "smooth_gradcampp_maps", "grad_powers_accumulate"):
        assert word in A.__doc__, word
    for f in (A.gradcampp, A.smooth_gradcampp):                       # the stated departures are written down
        assert "log-probability" in f.__doc__.lower() and "0 / 0" in A.gradcampp.__doc__
    assert "LAST sample" in A.smooth_gradcampp.__doc__


def test_cpu_tensors_are_refused():
    import torch
    from scouter_amd import kernels as K
    f = torch.zeros((1, 2, 2, 4))
    d = torch.zeros((1, 2, 2, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="gradcampp"):
        K.gradcampp(f, f.clone(), torch.zeros((1, 4)))
    with pytest.raises(RuntimeError, match="grad_powers_accumulate"):
        K.grad_powers_accumulate(f, d[0], d[0].clone())
    with pytest.raises(RuntimeError, match="gradcampp_smooth"):
        K.gradcampp_smooth(f, d, d.clone(), f.clone(), torch.zeros((1, 4)), 1)


class _NoDevice:
    """a model of 10 outputs whose every device entry point fails the test"""
    slot = types.SimpleNamespace(num_classes=10)
    training = False

    def feature_pass(self, x):
        raise AssertionError("the device was reached")

    __call__ = eval = train = feature_pass


def test_tools_refuse_bad_arguments_before_any_device_call():
    import torch
    from scouter_amd.tools.attribution import gradcampp, smooth_gradcampp
    m = _NoDevice()
    x = torch.zeros((2, 1, 8, 8))
    with pytest.raises(ValueError, match="images"):
        gradcampp(m, x[0])
    with pytest.raises(ValueError, match="images"):
        smooth_gradcampp(m, x[0])
    with pytest.raises(ValueError, match="n_samples"):
        smooth_gradcampp(m, x, n_samples=0)
    with pytest.raises(ValueError, match="batch"):
        smooth_gradcampp(m, x, batch=0)
    with pytest.raises(ValueError, match="sigma"):
        smooth_gradcampp(m, x, sigma=-0.1)
    with pytest.raises(ValueError, match="sigma"):
        smooth_gradcampp(m, x, sigma=float("nan"))
    for tool in (gradcampp, smooth_gradcampp):
        for bad in ([10], [-1], torch.tensor([0, 10])):
            with pytest.raises(IndexError):
                tool(m, x, classes=bad)
        for bad in (torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
            with pytest.raises(ValueError):
                tool(m, x, classes=bad)


def test_test_tool_parser_knows_the_campp_flags():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.campp is False and a.smoothcampp is False
    assert a.smoothcampp_samples == 4 and a.smoothcampp_sigma == 0.3 and a.smoothcampp_batch == 4
    # the older flags keep their defaults
    assert a.cam is False and a.causal is False and a.causal_step == 0 and a.smoothgrad is False and a.smoothgrad_samples == 50
    a = T.get_test_parser().parse_args(["--campp", "true", "--smoothcampp", "true", "--smoothcampp_samples", "7",
                                        "--smoothcampp_sigma", "0.5", "--smoothcampp_batch", "3"])
    assert a.campp is True and a.smoothcampp is True
    assert a.smoothcampp_samples == 7 and a.smoothcampp_sigma == 0.5 and a.smoothcampp_batch == 3
    assert callable(T.run_campp) and callable(T.run_smoothcampp)


@pytest.mark.parametrize("flag", ["--campp", "--smoothcampp"])
def test_train_parser_does_not_know_the_new_flags(flag):
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args([flag, "true"])
