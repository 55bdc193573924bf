"""Integrated Gradients / SmoothGrad without a GPU: the entry points of csrc/pathgrad.hip are declared in include/scouter_hip.h
with their argument lists and exported by the built library, the wrappers and tools have their signatures and defaults,
scouter_amd.test's parser knows the new flags (train.py's does not), the host quadrature tables of ig_quadrature are right, and a
NumPy restatement of Philox4x32-10 -- the one tests/test_pathgrad_gpu.py checks kernels.noise_images against -- reproduces three
known answers.

EPS = 2^-24.  The fp32-rounded weights w_i > 0 each carry a relative error of at most EPS, so their float64 sum is within
EPS * sum w = EPS of 1; the two-node Gauss-Legendre rule with rounded nodes a_i (relative error EPS each) and rounded weights
gives sum w_i a_i^p within (p + 1) EPS * (1 / (p + 1)) = EPS of 1 / (p + 1).  The bounds below are 4 EPS."""
import ctypes
import inspect

import numpy as np
import pytest

P, I, L, F, D, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
EPS = 2.0 ** -24

DECLARED = {
    # image, base, alphas, out, first, n, N, E, stream
    "scouter_path_images_f32": [P, P, P, P, I, I, I, L, P],
    # image, out, sigma, seed_lo, seed_hi, first, n, E, stream
    "scouter_noise_images_f32": [P, P, F, I, I, I, I, L, P],
    # grads, weights, acc, acc_sq, first, n, N, E, stream
    "scouter_grad_accumulate_f64": [P, P, P, P, I, I, I, L, P],
    # mode, acc, acc_sq, image, base, inv_n, out, total, E, then the workspace of the total (ws, ws_bytes), stream
    "scouter_attr_finish_f32": [I, P, P, P, P, D, P, P, L, P, Z, P],
    # x, out, M, C, HW, absolute, stream
    "scouter_channel_mean_f32": [P, P, L, I, L, I, P],
}


# ------------------------------------------------------------------------------------------------ Philox4x32-10, restated
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> the four output words as uint64 arrays below 2^32"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def normal_fp64(seed, sample, E):
    """(z [E], rad [E]) in float64: the definition of kernels.noise_images' z(seed, sample, e) -- the counter
    (e / 4, sample, 0, 0), the key (seed mod 2^32, seed / 2^32), u = (2 (r >> 9) + 1) 2^-24, Box-Muller with the angle
    6.283185307179586f * u (the fp32 constant, exactly) -- and the radius sqrt(-2 ln u) each element was scaled by"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((E + 3) // 4, dtype=np.uint64)
    r = philox4x32_10((q, int(sample), 0, 0), (seed & MASK, seed >> 32))
    u = [(2.0 * (w >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24 for w in r]
    two_pi = float(np.float32(6.283185307179586))
    z, rad = np.empty((len(q), 4)), np.empty((len(q), 4))
    for a in (0, 2):
        rr, ang = np.sqrt(-2.0 * np.log(u[a])), two_pi * u[a + 1]
        z[:, a], z[:, a + 1] = rr * np.cos(ang), rr * np.sin(ang)
        rad[:, a] = rad[:, a + 1] = rr
    return z.reshape(-1)[:E], rad.reshape(-1)[:E]


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK,) * 4, (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_restatement_reproduces_known_answers(counter, key, want):
    got = tuple(int(v) for v in philox4x32_10(counter, key))
    print("philox", ["%08x" % v for v in got])
    assert got == want
    # an array of counters gives the scalar answers element by element
    many = philox4x32_10((np.array([counter[0], 0, 5]), counter[1], counter[2], counter[3]), key)
    assert tuple(int(v[0]) for v in many) == want


def test_restated_normals_look_normal():
    """the float64 restatement alone: mean, variance and the correlation of the two halves of 8 samples of 3 * 64 * 64 elements
    lie within 4 standard errors (the GPU test holds the kernel to the same three)"""
    for seed in (0, 1):
        z = np.stack([normal_fp64(seed, s, 3 * 64 * 64)[0] for s in range(8)])
        n = z.size
        mean, var = z.mean(), z.var()
        a, b = z[:4].ravel(), z[4:].ravel()
        corr = float(np.corrcoef(a, b)[0, 1])
        figures = (abs(mean) * np.sqrt(n), abs(var - 1.0) * np.sqrt(n / 2.0), abs(corr) * np.sqrt(a.size))
        print("seed %d: |mean|, |var - 1|, |corr| in standard errors: %.2f %.2f %.2f" % ((seed,) + figures))
        assert all(f <= 4.0 for f in figures)
        u_min = np.exp(-0.5 * normal_fp64(seed, 0, 64)[1].max() ** 2)
        assert 0.0 < u_min < 1.0


# ------------------------------------------------------------------------------------------------ the library and the wrappers
def test_pathgrad_symbols_are_declared_and_exported():
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
    assert declared["scouter_attr_finish_workspace_bytes"] == (Z, [])
    assert _native.lib().scouter_attr_finish_workspace_bytes() >= 8


def test_pathgrad_wrappers_and_tools_have_their_signatures():
    from scouter_amd import kernels as K
    from scouter_amd.tools import attribution as A

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(K.path_images) == [("image", E), ("base", E), ("alphas", E), ("out", E), ("first", E)]
    assert params(K.noise_images) == [("image", E), ("out", E), ("sigma", E), ("seed", E), ("first", E)]
    assert params(K.grad_accumulate) == [("grads", E), ("weights", E), ("acc", E), ("acc_sq", None), ("first", 0)]
    assert params(K.attr_finish) == [("mode", E), ("acc", None), ("acc_sq", None), ("image", None), ("base", None), ("inv_n", 1.0),
                                     ("out", None), ("total", None)]
    assert params(K.channel_mean) == [("x", E), ("absolute", False), ("out", None)]
    assert (K.ATTR_IG, K.ATTR_MEAN, K.ATTR_MEAN_SQ, K.ATTR_VAR) == (0, 1, 2, 3)
    assert params(A.integrated_gradients) == [("model", E), ("images", E), ("classes", None), ("baseline", None), ("n_steps", 50),
                                              ("method", "gausslegendre"), ("batch", 50), ("return_delta", False)]
    assert params(A.smoothgrad) == [("model", E), ("images", E), ("classes", None), ("n_samples", 50), ("sigma", 1.0),
                                    ("kind", "smoothgrad"), ("batch", 50), ("seed", 0)]
    assert params(A.gradient_maps) == [("attr", E), ("min_level", 0.0), ("absolute", False)]
    assert params(A.ig_quadrature) == [("n_steps", 50), ("method", "gausslegendre")]
    assert params(A.attribution_maps) == [("grads", E), ("min_level", 0.0)]                  # the host version stays as it is
    for word in ("integrated_gradients", "smoothgrad", "gradient_maps", "path_images", "noise_images", "grad_accumulate"):
        assert word in A.__doc__, word


def test_cpu_tensors_are_refused():
    import torch
    from scouter_amd import kernels as K
    img = torch.zeros((1, 4, 4))
    with pytest.raises(RuntimeError, match="path_images"):
        K.path_images(img, None, torch.zeros(3), torch.zeros((3, 1, 4, 4)), 0)
    with pytest.raises(RuntimeError, match="noise_images"):
        K.noise_images(img, torch.zeros((3, 1, 4, 4)), 1.0, 0, 0)
    with pytest.raises(RuntimeError, match="grad_accumulate"):
        K.grad_accumulate(torch.zeros((3, 1, 4, 4)), None, torch.zeros((1, 4, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="attr_finish"):
        K.attr_finish(K.ATTR_MEAN, torch.zeros((1, 4, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="channel_mean"):
        K.channel_mean(img)


# ------------------------------------------------------------------------------------------------ the command-line tool
def test_test_tool_parser_knows_ig_and_smoothgrad():
    from scouter_amd import test as T
    a = T.get_test_parser().parse_args([])
    assert a.ig is False and a.ig_steps == 50 and a.ig_batch == 50
    assert a.smoothgrad is False and a.smoothgrad_samples == 50 and a.smoothgrad_sigma == 1.0 and a.smoothgrad_batch == 50
    # the older flags keep their defaults
    assert a.scorecam is False and a.scorecam_batch == 250 and a.rise is False and a.rise_batch == 250 and a.rise_masks == 4000
    assert a.cam is False and a.causal is False and a.causal_step == 0
    a = T.get_test_parser().parse_args(["--ig", "true", "--ig_steps", "12", "--ig_batch", "5", "--smoothgrad", "true",
                                        "--smoothgrad_samples", "7", "--smoothgrad_sigma", "0.5", "--smoothgrad_batch", "3"])
    assert a.ig is True and a.ig_steps == 12 and a.ig_batch == 5
    assert a.smoothgrad is True and a.smoothgrad_samples == 7 and a.smoothgrad_sigma == 0.5 and a.smoothgrad_batch == 3
    assert callable(T.run_ig) and callable(T.run_smoothgrad)


@pytest.mark.parametrize("flag", ["--ig", "--smoothgrad"])
def test_train_parser_does_not_know_the_new_flags(flag):
    from scouter_amd.train import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args([flag, "true"])


# ------------------------------------------------------------------------------------------------ the quadrature tables
@pytest.mark.parametrize("method", ["gausslegendre", "riemann_trapezoid"])
@pytest.mark.parametrize("n_steps", [1, 2, 7, 50])
def test_quadrature_weights_sum_to_one(method, n_steps):
    """(the trapezoid rule needs two nodes: its n_steps = 1 is the ValueError the tools raise)"""
    import torch
    from scouter_amd.tools.attribution import ig_quadrature
    if method == "riemann_trapezoid" and n_steps == 1:
        with pytest.raises(ValueError):
            ig_quadrature(n_steps, method)
        return
    alphas, weights = ig_quadrature(n_steps, method)
    assert alphas.dtype == torch.float32 and weights.dtype == torch.float32 and not alphas.is_cuda
    assert tuple(alphas.shape) == (n_steps,) and tuple(weights.shape) == (n_steps,)
    a, w = alphas.double().numpy(), weights.double().numpy()
    err = abs(float(w.sum()) - 1.0)
    print("%s n_steps %d: |sum w - 1| = %.3e, bound %.3e" % (method, n_steps, err, 4 * EPS))
    assert err <= 4 * EPS
    assert bool((w > 0).all()) and bool((np.diff(a) > 0).all()) and a[0] >= 0.0 and a[-1] <= 1.0
    assert np.array_equal(a, 1.0 - a[::-1]) or float(np.abs(a - (1.0 - a[::-1])).max()) <= 2 * EPS     # symmetric nodes
    if method == "riemann_trapezoid":
        assert a[0] == 0.0 and a[-1] == 1.0 and w[0] == w[-1] and (n_steps == 2 or abs(w[1] - 2 * w[0]) <= 2 * EPS * w[1])


def test_two_node_gauss_legendre_is_exact_to_degree_three():
    from scouter_amd.tools.attribution import ig_quadrature
    alphas, weights = ig_quadrature(2)
    a, w = alphas.double().numpy(), weights.double().numpy()
    for p, want in ((2, 1.0 / 3.0), (3, 0.25)):
        err = abs(float((w * a ** p).sum()) - want)
        print("integral of alpha^%d: error %.3e, bound %.3e" % (p, err, 4 * EPS))
        assert err <= 4 * EPS


def test_quadrature_refuses_bad_arguments():
    from scouter_amd.tools.attribution import ig_quadrature
    for bad in ((0, "gausslegendre"), (-3, "gausslegendre"), (1, "riemann_trapezoid"), (5, "simpson")):
        with pytest.raises(ValueError):
            ig_quadrature(*bad)
