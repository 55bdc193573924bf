"""Infidelity / max-sensitivity without a GPU: the entry points of csrc/fidelity.hip are declared in include/scouter_hip.h with
their argument lists and exported by the built library, the wrappers and tools have their signatures and defaults, CPU tensors
are refused, scouter_amd.test's parser knows the new flags (train.py's does not), and a NumPy restatement of the uniform
perturbation stream -- the one tests/test_fidelity_gpu.py checks kernels.uniform_images against -- has the properties the
definition promises.

The uniform stream: d = 2 u - 1 with u = (2 (r >> 9) + 1) 2^-24, r a Philox4x32-10 word of the counter (e / 4, sample, 1, 0), so
d = ((2 (r >> 9) + 1) - 2^23) 2^-23: an odd multiple of 2^-23, never 0, |d| <= 1 - 2^-23.  For n independent draws of a uniform
variable on (-1, 1) the mean has standard error sqrt(1 / (3 n)) and the sample variance sqrt((E d^4 - (E d^2)^2) / n) =
sqrt((1 / 5 - 1 / 9) / n) = sqrt(4 / (45 n)); the bounds are 4 standard errors, as for the normal stream in
tests/test_pathgrad_cpu.py."""
import ctypes
import inspect

import numpy as np
import pytest

from test_pathgrad_cpu import MASK, philox4x32_10

P, I, L, F, D, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

DECLARED = {
    # attrs, dots, sigma, seed_lo, seed_hi, first, n, N, K, E, A, then the workspace of the partial sums (ws, ws_bytes), stream
    "scouter_perturb_dots_f64": [P, P, F, I, I, I, I, I, I, L, L, P, Z, P],
    # image, out, radius, seed_lo, seed_hi, first, n, E, stream
    "scouter_uniform_images_f32": [P, P, F, I, I, I, I, L, P],
    # out, cols, deltas, first, n, N, K, n_classes, of, stream
    "scouter_output_deltas_f64": [P, P, P, I, I, I, I, I, I, P],
    # maps, terms, first, n, N, K, M, stream
    "scouter_map_distances_f64": [P, P, I, I, I, I, L, P],
    # dots, deltas, raw, beta, normalized, R, N, stream
    "scouter_infidelity_finish_f64": [P, P, P, P, P, L, I, P],
    # terms, score, R, N, stream
    "scouter_sensitivity_finish_f64": [P, P, L, I, P],
}


# ------------------------------------------------------------------------------------------------ the uniform stream, restated
def uniform_words(seed, sample, E, stream=1):
    """the Philox words [ceil(E / 4), 4] (uint64 below 2^32) of the counter (q, sample, stream, 0) under the 64-bit seed"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((E + 3) // 4, dtype=np.uint64)
    return np.stack(philox4x32_10((q, int(sample), int(stream), 0), (seed & MASK, seed >> 32)), axis=1)


def uniform_fp64(seed, sample, E):
    """d [E] in float64, exactly: the definition of kernels.uniform_images' d(seed, sample, e) -- word e mod 4 of the counter
    (e / 4, sample, 1, 0), d = ((2 (r >> 9) + 1) - 2^23) 2^-23"""
    r = uniform_words(seed, sample, E)
    d = ((2.0 * (r >> np.uint64(9)).astype(np.float64) + 1.0) - 2.0 ** 23) * 2.0 ** -23
    return d.reshape(-1)[:E]


@pytest.mark.parametrize("seed", [0, 1, 0x9E3779B97F4A7C15])
def test_restated_uniform_stream_has_its_properties(seed):
    E, n = 3 * 64 * 64, 8
    d = np.stack([uniform_fp64(seed, s, E) for s in range(n)])
    assert d.shape == (n, E)
    assert float(np.abs(d).max()) < 1.0 and float(np.abs(d).min()) > 0.0                 # inside (-1, 1), never 0
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d)                    # every value is an fp32 number
    u32 = ((2.0 * (uniform_words(seed, 0, E) >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal((np.float32(2.0) * u32 - np.float32(1.0)).astype(np.float64).reshape(-1)[:E], d[0])   # 2 u - 1 in fp32
    figures = (abs(d.mean()) * np.sqrt(3.0 * d.size), abs(d.var() - 1.0 / 3.0) * np.sqrt(45.0 * d.size / 4.0))
    print("seed %x: |mean|, |var - 1/3| in standard errors: %.2f %.2f (bound 4)" % ((seed,) + figures))
    assert all(f <= 4.0 for f in figures)
    # the noise stream's words for the same (seed, sample, q) are other words: the third counter word sets the streams apart
    for s in range(n):
        own, noise = uniform_words(seed, s, E, stream=1), uniform_words(seed, s, E, stream=0)
        same = float((own == noise).mean())
        assert same < 1e-3, (s, same)
    # a sample is not its neighbour, a seed that differs in the high word alone is another stream, a partial group uses its
    # leading words
    assert not np.array_equal(d[0], d[1])
    assert not np.array_equal(uniform_fp64(seed ^ (1 << 32), 0, E), d[0])
    assert np.array_equal(uniform_fp64(seed, 3, 35), d[3][:35])


# ------------------------------------------------------------------------------------------------ the library and the wrappers
def test_fidelity_symbols_are_declared_and_exported():
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
    assert declared["scouter_perturb_dots_workspace_bytes"] == (Z, [I, I, L])
    nbytes = _native.lib().scouter_perturb_dots_workspace_bytes
    assert nbytes(1, 1, 1) == 8 and nbytes(0, 1, 1) == 0 and nbytes(1, 0, 1) == 0 and nbytes(1, 1, 0) == 0
    assert nbytes(3, 5, 4 * 256) == 8 * 15 and nbytes(3, 5, 4 * 256 + 1) == 2 * 8 * 15    # one workgroup per 256 groups of four
    assert nbytes(1, 1, 3 * 224 * 224) == 8 * 147 and nbytes(1, 1, 3 * 300 * 300) == nbytes(1, 1, 1 << 30) == 8 * 256   # ... up to 256
    header = open(_native.HEADER_PATH).read()
    for word in ("SCOUTER_DELTA_LOG_PROB 0", "SCOUTER_DELTA_PROB 1", "Yeh et al."):
        assert word in header, word


def test_fidelity_wrappers_and_tools_have_their_signatures():
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as A

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(K.perturb_dots) == [("attrs", E), ("dots", E), ("sigma", E), ("seed", E), ("first", E), ("n", E),
                                      ("channels", None)]
    assert params(K.uniform_images) == [("image", E), ("out", E), ("radius", E), ("seed", E), ("first", E)]
    assert params(K.uniform_images) == [(n.replace("sigma", "radius"), d) for n, d in params(K.noise_images)]     # the twin
    assert params(K.output_deltas) == [("out", E), ("cols", E), ("deltas", E), ("first", E), ("of", "log_prob")]
    assert params(K.map_distances) == [("maps", E), ("terms", E), ("first", E)]
    assert params(K.infidelity_finish) == [("dots", E), ("deltas", E), ("out", None)]
    assert params(K.sensitivity_finish) == [("terms", E), ("out", None)]
    assert (K.DELTA_LOG_PROB, K.DELTA_PROB) == (0, 1)
    assert K.PERTURB_DOTS_CLASS_TILE >= 1 and K.PERTURB_DOTS_SAMPLE_TILE >= 1
    assert params(A.infidelity) == [("model", E), ("images", E), ("attributions", E), ("classes", None), ("n_samples", 50),
                                    ("sigma", 0.003), ("batch", 50), ("seed", 0), ("of", "log_prob")]
    assert params(A.sensitivity_max) == [("explain", E), ("images", E), ("n_samples", 10), ("radius", 0.02), ("batch", 11),
                                         ("seed", 0)]
    assert A.InfidelityScores._fields == ("raw", "normalized", "beta", "dots", "deltas")
    assert A.SensitivityScores._fields == ("score", "terms")
    for word in ("infidelity", "sensitivity_max", "perturb_dots", "uniform_images", "output_deltas", "map_distances",
                 "infidelity_finish", "sensitivity_finish", "Yeh et"):
        assert word in A.__doc__, word
    for f in (A.infidelity, A.sensitivity_max):
        assert "could not be checked" in f.__doc__                                        # the defaults are remembered, not verified
    for family in ("input_gradients", "gradcam(", "gradcampp(", "smooth_gradcampp(", "rise(", "scorecam(", "integrated_gradients(",
                   "smoothgrad(", "slot_saliency("):
        assert "lambda im: " in A.sensitivity_max.__doc__ and family in A.sensitivity_max.__doc__, family


def test_cpu_tensors_are_refused():
    import torch
    from scouter_amd import kernels as K
    f64 = dict(dtype=torch.float64)
    with pytest.raises(RuntimeError, match="perturb_dots"):
        K.perturb_dots(torch.zeros((2, 1, 4, 4)), torch.zeros((2, 3), **f64), 1.0, 0, 0, 3)
    with pytest.raises(RuntimeError, match="uniform_images"):
        K.uniform_images(torch.zeros((1, 4, 4)), torch.zeros((3, 1, 4, 4)), 1.0, 0, 0)
    with pytest.raises(RuntimeError, match="output_deltas"):
        K.output_deltas(torch.zeros((4, 5)), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 3), **f64), 0)
    with pytest.raises(RuntimeError, match="map_distances"):
        K.map_distances(torch.zeros((4, 2, 3, 3)), torch.zeros((2, 3), **f64), 0)
    with pytest.raises(RuntimeError, match="infidelity_finish"):
        K.infidelity_finish(torch.zeros((2, 3), **f64), torch.zeros((2, 3), **f64))
    with pytest.raises(RuntimeError, match="sensitivity_finish"):
        K.sensitivity_finish(torch.zeros((2, 3), **f64))
    with pytest.raises(ValueError, match="of must be"):
        K.output_deltas(torch.zeros((4, 5)), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 3), **f64), 0, of="logit")


def test_tools_refuse_bad_arguments_before_any_launch():
    """batch < 2, a bad `of`, n_samples < 1, a negative sigma / radius, a wrong attribution rank: ValueError from the tools on
    CPU tensors, before anything touches the device"""
    import torch
    from scouter_amd.tools.attribution import infidelity, sensitivity_max
    x, a = torch.zeros((1, 1, 4, 4)), torch.zeros((1, 1, 4, 4))
    model = torch.nn.Flatten()
    for kwargs in (dict(batch=1), dict(batch=0), dict(of="logit"), dict(n_samples=0), dict(sigma=-1.0), dict(sigma=float("inf"))):
        with pytest.raises(ValueError):
            infidelity(model, x, a, classes=[0], **kwargs)
    for bad in (a[0], torch.zeros((2, 1, 4, 4)), torch.zeros((1, 1, 1, 4, 4), dtype=torch.float64), torch.zeros((1, 1, 2, 4, 4)),
                torch.zeros((1, 1, 4, 4), dtype=torch.int32), [a]):
        with pytest.raises(ValueError):
            infidelity(model, x, bad, classes=[0])
    with pytest.raises(ValueError):
        infidelity(model, x[0], a, classes=[0])
    for kwargs in (dict(batch=1), dict(n_samples=0), dict(radius=-0.1), dict(radius=float("nan"))):
        with pytest.raises(ValueError):
            sensitivity_max(lambda im: im[:, None], x, **kwargs)
    with pytest.raises(ValueError):
        sensitivity_max(None, x)
    with pytest.raises(ValueError):
        sensitivity_max(lambda im: im[:, None], x[0])


# ------------------------------------------------------------------------------------------------ the command-line tool
def test_test_tool_parser_knows_infidelity_and_sensitivity():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.infidelity is False and a.infidelity_samples == 50 and a.infidelity_sigma == 0.003 and a.infidelity_batch == 50
    assert a.sensitivity is False and a.sensitivity_samples == 10 and a.sensitivity_radius == 0.02 and a.sensitivity_batch == 11
    # the older flags keep their defaults
    assert a.causal is False and a.causal_step == 0 and a.cam is False and a.ig is False and a.smoothgrad_sigma == 1.0
    a = T.get_test_parser().parse_args(["--infidelity", "true", "--infidelity_samples", "6", "--infidelity_sigma", "0.01",
                                        "--infidelity_batch", "4", "--sensitivity", "true", "--sensitivity_samples", "3",
                                        "--sensitivity_radius", "0.05", "--sensitivity_batch", "2"])
    assert a.infidelity is True and a.infidelity_samples == 6 and a.infidelity_sigma == 0.01 and a.infidelity_batch == 4
    assert a.sensitivity is True and a.sensitivity_samples == 3 and a.sensitivity_radius == 0.05 and a.sensitivity_batch == 2
    assert callable(T.run_infidelity) and callable(T.run_sensitivity) and callable(T.run_causal)
    for word in ("--infidelity true", "--sensitivity true", "infidelity <family> class <c>: raw <r> normalized <n> beta <b>",
                 "sensitivity <family> class <c>: max <s>"):
        assert word in T.__doc__, word


@pytest.mark.parametrize("flag", ["--infidelity", "--sensitivity", "--infidelity_samples", "--sensitivity_radius"])
def test_train_parser_does_not_know_the_new_flags(flag):
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args([flag, "1"])
