"""`--aug true` without a GPU: the random draws, the reduction of a drawn sequence to blur / warp / blur, the host
definition `augment_host` (dataset/augment.py) at its exact cases, and the interface around it (make_transform's
declaration, the parser, main's refusal of synthetic data)."""
import types

import numpy as np
import pytest
import torch

from scouter_amd.dataset import augment as A

KEYS = ("fliplr", "flipud", "affine", "blur", "rotate", "scale_x", "scale_y", "translate_x", "translate_y", "sigma", "order")


def _draws(n=1, **kw):
    """hand-made draws: nothing present unless named; order = the order of OPS unless given"""
    d = {"fliplr": np.zeros(n, bool), "flipud": np.zeros(n, bool), "affine": np.zeros(n, bool), "blur": np.zeros(n, bool),
         "rotate": np.zeros(n, np.int64), "scale_x": np.ones(n), "scale_y": np.ones(n), "translate_x": np.zeros(n),
         "translate_y": np.zeros(n), "sigma": np.zeros(n), "order": np.tile(np.arange(4), (n, 1))}
    for k, v in kw.items():
        d[k] = np.asarray(v)
        assert len(d[k]) == n, k
    return d


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def test_draws_are_a_pure_function_of_seed_call_and_rank():
    a = A.draw_params(64, 7, 3, 1)
    assert set(a) == set(KEYS)
    assert _same(a, A.draw_params(64, 7, 3, 1))
    assert _same(a, A.draw_params(64, 7, 3, rank=1))
    for other in (A.draw_params(64, 8, 3, 1), A.draw_params(64, 7, 4, 1), A.draw_params(64, 7, 3, 0)):
        assert not _same(a, other)
    assert _same(A.draw_params(64, 7, 3), A.draw_params(64, 7, 3, 0))


def test_ranges_coins_and_orders_over_10000_draws():
    d = A.draw_params(10000, 1, 0)
    for coin in A.OPS:
        assert d[coin].dtype == bool and 0.45 <= d[coin].mean() <= 0.55, coin
    aff, blur = d["affine"], d["blur"]
    assert d["rotate"].dtype.kind == "i" and set(np.unique(d["rotate"][aff])) == set(range(-10, 10))
    for k, lo, hi in (("scale_x", 0.8, 1.0), ("scale_y", 0.8, 1.0), ("translate_x", 0.0, 0.1), ("translate_y", -0.1, 0.1)):
        v = d[k][aff]
        assert v.min() >= lo and v.max() <= hi and v.max() - v.min() > 0.9 * (hi - lo), k
    assert d["sigma"][blur].min() >= 0.0 and d["sigma"][blur].max() <= 3.0 and d["sigma"][blur].max() > 2.9
    # where the coin is off the value is the neutral one
    assert not d["rotate"][~aff].any() and (d["scale_x"][~aff] == 1).all() and (d["scale_y"][~aff] == 1).all()
    assert not d["translate_x"][~aff].any() and not d["translate_y"][~aff].any() and not d["sigma"][~blur].any()
    assert (np.sort(d["order"], axis=1) == np.arange(4)).all()
    # every order of three present operations occurs (for every triple), about equally often
    for triple in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        rest = [j for j in range(4) if j not in triple][0]
        rows = d[A.OPS[triple[0]]] & d[A.OPS[triple[1]]] & d[A.OPS[triple[2]]] & ~d[A.OPS[rest]]
        seen = {}
        for o in d["order"][rows][:, list(triple)]:
            key = tuple(np.argsort(o))
            seen[key] = seen.get(key, 0) + 1
        assert len(seen) == 6 and min(seen.values()) > rows.sum() / 6 * 0.6, (triple, seen)


def test_blur_first_follows_the_drawn_order_and_blur_alone_blurs_last():
    # order[j] = rank of OPS[j]: blur (3) before affine (2) / after it / without it
    p = A.build_params(_draws(3, affine=[1, 1, 0], blur=[1, 1, 1], rotate=[5, 5, 0], sigma=[2.2, 2.2, 2.2],
                              order=[[2, 3, 1, 0], [2, 3, 0, 1], [2, 3, 1, 0]]), 17)
    assert p["klen_first"].tolist() == [7, 0, 0] and p["klen_last"].tolist() == [0, 7, 7]
    assert p["identity"].tolist() == [0, 0, 1]
    assert np.array_equal(p["taps"][0], p["taps"][1]) and not p["taps"][0][7:].any()
    packed = A.pack_params(p)
    assert packed.shape == (3, A.ROW_WORDS) and packed.dtype == np.int32
    v = A.unpack_views(torch.from_numpy(packed))
    for k in ("klen_first", "klen_last", "identity", "minv", "taps"):
        assert np.array_equal(v[k].numpy(), p[k]), k


@pytest.mark.parametrize("S", [5, 17, 32])
def test_mirrors_are_integer_matrices_and_exact_flips(S):
    rng = np.random.default_rng(S)
    img = rng.integers(0, 256, (4, 3, S, S), dtype=np.uint8)
    p = A.build_params(_draws(4, fliplr=[0, 1, 0, 1], flipud=[0, 0, 1, 1], order=[[0, 1, 2, 3]] * 3 + [[1, 0, 2, 3]]), S)
    assert np.array_equal(p["minv"], np.rint(p["minv"])) and p["identity"].tolist() == [1, 0, 0, 0]
    out = A.augment_host(img, p)
    assert np.array_equal(out[0], img[0])
    assert np.array_equal(out[1], np.flip(img[1], axis=2))
    assert np.array_equal(out[2], np.flip(img[2], axis=1))
    assert np.array_equal(out[3], np.flip(img[3], axis=(1, 2)))


def test_affine_and_mirror_do_not_commute():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 1, 17, 17), dtype=np.uint8)
    img[1] = img[0]
    kw = dict(fliplr=[1, 1], affine=[1, 1], rotate=[7, 7], scale_x=[0.85, 0.85], scale_y=[0.95, 0.95],
              translate_x=[0.08, 0.08], translate_y=[-0.05, -0.05])
    p = A.build_params(_draws(2, order=[[1, 2, 0, 3], [0, 2, 1, 3]], **kw), 17)       # affine first / fliplr first
    assert not np.allclose(p["minv"][0], p["minv"][1])
    out = A.augment_host(img, p)
    assert not np.array_equal(out[0], out[1])
    # the composition is the product in the drawn order: later operations multiply on the left
    F = A.op_matrix("fliplr", 17)
    Aff = A.op_matrix("affine", 17, 7, 0.85, 0.95, 0.08, -0.05)
    assert np.allclose(p["minv"][0], np.linalg.inv(F @ Aff)[:2].reshape(6), atol=1e-5)
    assert np.allclose(p["minv"][1], np.linalg.inv(Aff @ F)[:2].reshape(6), atol=1e-5)


def test_affine_matrix_is_the_stated_product():
    S, c = 33, 16.0
    M = A.op_matrix("affine", S, rotate=-10, scale_x=0.8, scale_y=0.9, translate_x=0.1, translate_y=-0.1)
    th = np.deg2rad(-10.0)
    for x, y in ((0.0, 0.0), (c, c), (32.0, 5.0)):
        sx, sy = 0.8 * (x - c), 0.9 * (y - c)
        want = (np.cos(th) * sx - np.sin(th) * sy + 0.1 * S + c, np.sin(th) * sx + np.cos(th) * sy - 0.1 * S + c)
        assert np.allclose((M @ [x, y, 1.0])[:2], want, atol=1e-12)


def test_klen_rule_and_taps():
    assert [A.blur_klen(s) for s in (0.5, 1.6, 2.2, 2.8, 2.999)] == [5, 5, 7, 9, 9]
    assert A.blur_klen(0.0) == 0 and A.blur_klen(9.99e-4) == 0 and A.blur_klen(1e-3) == 5
    assert A.blur_klen(4.0) == 11 and A.blur_klen(6.0) == 15            # the 2.9 and 2.6 branches of imgaug's rule
    for s in (1e-3, 0.5, 1.6, 2.2, 2.8, 2.999):
        t = A.blur_taps(s)
        assert t.dtype == np.float32 and len(t) == A.blur_klen(s) and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6
        assert np.array_equal(t, t[::-1]) and t.argmax() == len(t) // 2
    with pytest.raises(ValueError, match="taps"):
        A.build_params(_draws(1, blur=[1], sigma=[4.0]), 17)
    with pytest.raises(ValueError, match="at least 5"):
        A.build_params(_draws(1), 4)


@pytest.mark.parametrize("S", [5, 17])
def test_constant_image_stays_constant_under_blur(S):
    img = np.full((3, 1, S, S), 0, np.uint8)
    img[0], img[1], img[2] = 255, 1, 130
    p = A.build_params(_draws(3, blur=[1, 1, 1], sigma=[0.5, 2.2, 2.999]), S)
    assert p["klen_last"].tolist() == [5, 7, 9]
    assert np.array_equal(A.augment_host(img, p), img)


def test_blur_border_is_reflect_101():
    S = 7
    img = np.zeros((1, 1, S, S), np.uint8)
    img[0, 0, 0, 1] = 200                          # one pixel next to the left border, in the top row
    t = A.blur_taps(1.0).astype(np.float64)        # 5 taps, radius 2
    raw = A.blur_host_unrounded(img[0], A.blur_taps(1.0))
    # column 0 of row 0 sees pixel 1 twice along x (as itself and as the reflection of index -1) and row 0 once along y
    assert np.isclose(raw[0, 0, 0], 200 * (t[3] + t[1]) * t[2])
    assert np.isclose(raw[0, 1, 0], 200 * (t[3] + t[1]) * t[1])       # row 1's window -1 .. 3 reads rows 1, 0, 1, 2, 3
    assert np.isclose(raw[0, 0, 3], 200 * t[0] * t[2])


def test_integer_translation_shifts_with_zeros():
    S = 17
    rng = np.random.default_rng(4)
    img = rng.integers(1, 256, (1, 3, S, S), dtype=np.uint8)
    p = A.build_params(_draws(1), S)
    p["identity"][0] = 0
    p["minv"][0] = [1, 0, -3, 0, 1, 2]             # destination (x, y) reads source (x - 3, y + 2)
    out = A.augment_host(img, p)
    want = np.zeros_like(img)
    want[0, :, :S - 2, 3:] = img[0, :, 2:, :S - 3]
    assert np.array_equal(out, want)
    out, raw = A.augment_host(img, A.build_params(_draws(1), S), return_unrounded=True)
    assert np.array_equal(out, img) and np.array_equal(raw, img.astype(np.float64))


def test_cpu_device_runs_the_host_definition():
    from scouter_amd.dataset.transform_func import GpuTransform
    S = 9
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (5, 3, S, S), dtype=np.uint8)
    tf = GpuTransform("ImageNet", S, aug=True, aug_seed=11, rank=2)
    got = tf.augment(torch.from_numpy(img), "cpu")
    want = A.augment_host(img, A.build_params(A.draw_params(5, 11, 0, 2), S))
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3, S, S) and tf.calls == 1
    for c in range(3):
        assert torch.equal(got[:, c], tf.table[c][torch.from_numpy(want[:, c]).long()])
    again = tf.augment(torch.from_numpy(img), "cpu")               # call 1: other draws
    assert tf.calls == 2 and not torch.equal(again, got)


def test_host_half_refuses_aug_unless_the_device_half_is_declared():
    from scouter_amd.dataset.transform_func import Decode, GpuTransform, make_gpu_transform, make_transform
    args = types.SimpleNamespace(dataset="ImageNet", img_size=16, aug=True)
    with pytest.raises(NotImplementedError, match="make_gpu_transform"):
        make_transform(args, "train")
    assert isinstance(make_transform(args, "val"), Decode)
    args.aug_on_device = True
    assert isinstance(make_transform(args, "train"), Decode)
    args.aug_seed, args.distributed, args.rank = 5, True, 3
    tf = make_gpu_transform(args, "train")
    assert tf.aug and tf.aug_seed == 5 and tf.rank == 3
    assert not make_gpu_transform(args).aug and not make_gpu_transform(args, "val").aug
    assert not GpuTransform("ImageNet", 16).aug
    with pytest.raises(ValueError):
        make_gpu_transform(args, "test")


def test_parser_knows_aug_seed_and_main_refuses_synthetic_data():
    from scouter_amd import train
    args = train.get_args_parser().parse_args([])
    assert args.aug_seed == 0 and args.aug is False
    args = train.get_args_parser().parse_args(["--aug", "true", "--aug_seed", "12", "--synthetic_data", "true"])
    assert args.aug_seed == 12 and args.aug is True
    with pytest.raises(ValueError, match="decoded"):
        train.main(args)
