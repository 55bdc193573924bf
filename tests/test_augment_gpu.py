"""`--aug true` on the GPU (csrc/augment.hip through kernels.aug_blur / aug_warp / aug_finish / resize_u8 and
GpuTransform(aug=True)) against the host definition `augment_host` of dataset/augment.py.

The yardstick is float64, the kernels compute in float32, both round ONCE per stage to a byte.  So a byte may differ from
the definition's, by 1, only where the definition's unrounded value lies within 1e-3 of a half-integer (float32 error of a
9 x 9 convex combination of bytes is below 255 * 20 * 2^-24 = 3e-4), and such bytes are at most 0.5 % of all: a condition on
the random data, not a tolerance -- exact ties are rare and near-ties within 1e-3 are 0.2 % of the bytes.  Everything else
(mirrors, identity, klen 0, per-image selection, reproducibility, aug=False) is bit for bit."""
import numpy as np
import pytest
import torch

from oracle import pil_resize as P
from scouter_amd.dataset import augment as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [5, 17, 33]
B = 6
SIGMAS = {5: [0.3, 0.5, 0.9, 1.2, 1.5, 1.8], 7: [1.9, 2.0, 2.1, 2.2, 2.3, 2.4], 9: [2.5, 2.6, 2.7, 2.8, 2.9, 2.999]}


def _draws(n, **kw):
    d = {"fliplr": np.zeros(n, bool), "flipud": np.zeros(n, bool), "affine": np.zeros(n, bool), "blur": np.zeros(n, bool),
         "rotate": np.zeros(n, np.int64), "scale_x": np.ones(n), "scale_y": np.ones(n), "translate_x": np.zeros(n),
         "translate_y": np.zeros(n), "sigma": np.zeros(n), "order": np.tile(np.arange(4), (n, 1))}
    for k, v in kw.items():
        d[k] = np.asarray(v)
        assert len(d[k]) == n, k
    return d


def _affine_draws(n, rng, **kw):
    return _draws(n, affine=np.ones(n, bool), rotate=rng.integers(-10, 10, n), scale_x=rng.uniform(0.8, 1.0, n),
                  scale_y=rng.uniform(0.8, 1.0, n), translate_x=rng.uniform(0.0, 0.1, n),
                  translate_y=rng.uniform(-0.1, 0.1, n), **kw)


def _bytes(S, C, seed, n=B):
    return np.random.default_rng(seed).integers(0, 256, (n, C, S, S), dtype=np.uint8)


def _dev(p):
    """stage parameters -> device views of ONE packed table, as GpuTransform hands them to the kernels"""
    return A.unpack_views(torch.from_numpy(A.pack_params(p)).to(DEV))


def _chain(img, p):
    from scouter_amd import kernels as K
    return K.augment_bytes(torch.from_numpy(img).to(DEV), _dev(p)).cpu().numpy()


def _against_definition(what, got, img, p):
    want, raw = A.augment_host(img, p, return_unrounded=True)
    differ = got != want
    off = np.abs(got.astype(np.int64) - want.astype(np.int64))
    tie = np.abs(raw - np.floor(raw) - 0.5) < 1e-3
    print("%s: %d of %d bytes differ (largest step %d), %d of them away from a tie; %d bytes are within 1e-3 of a tie"
          % (what, differ.sum(), differ.size, off.max(), (differ & ~tie).sum(), tie.sum()))
    assert off.max() <= 1, what
    assert not (differ & ~tie).any(), what
    assert differ.mean() <= 0.005, what


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", SIZES)
def test_warp_against_definition(S, C):
    from scouter_amd import kernels as K
    rng = np.random.default_rng(100 + S + C)
    img = _bytes(S, C, 1000 + S + C)
    p = A.build_params(_affine_draws(B, rng, fliplr=[0, 1, 0, 1, 0, 1], flipud=[0, 0, 1, 1, 0, 0],
                                     order=[rng.permutation(4) for _ in range(B)]), S)
    assert not p["identity"].any() and not p["klen_first"].any() and not p["klen_last"].any()
    v = _dev(p)
    got = K.aug_warp(torch.from_numpy(img).to(DEV), v["minv"], v["identity"]).cpu().numpy()
    _against_definition("warp S %d C %d" % (S, C), got, img, p)
    # dense tables of their own give the same bytes as views into the packed one
    again = K.aug_warp(torch.from_numpy(img).to(DEV), torch.from_numpy(p["minv"]).to(DEV),
                       torch.from_numpy(p["identity"]).to(DEV)).cpu().numpy()
    assert np.array_equal(again, got)


@pytest.mark.parametrize("klen", [5, 7, 9])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", SIZES)
def test_blur_against_definition(S, C, klen):
    from scouter_amd import kernels as K
    img = _bytes(S, C, 2000 + 10 * S + C + klen)
    p = A.build_params(_draws(B, blur=np.ones(B, bool), sigma=SIGMAS[klen]), S)
    assert p["klen_last"].tolist() == [klen] * B and p["identity"].all()
    v = _dev(p)
    got = K.aug_blur(torch.from_numpy(img).to(DEV), v["klen_last"], v["taps"]).cpu().numpy()
    _against_definition("blur S %d C %d klen %d" % (S, C, klen), got, img, p)
    # a constant image stays constant (reflect-101 keeps the weights summing to 1 at the border)
    flat = np.broadcast_to(np.array([0, 1, 127, 128, 254, 255], np.uint8)[:, None, None, None], img.shape).copy()
    assert np.array_equal(K.aug_blur(torch.from_numpy(flat).to(DEV), v["klen_last"], v["taps"]).cpu().numpy(), flat)


@pytest.mark.parametrize("blur_first", [True, False])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", SIZES)
def test_full_chain_against_definition(S, C, blur_first):
    rng = np.random.default_rng(300 + S + C + int(blur_first))
    img = _bytes(S, C, 3000 + 10 * S + C + int(blur_first))
    order = [3, 2, 1, 0] if blur_first else [0, 1, 2, 3]          # rank of (fliplr, flipud, affine, blur)
    p = A.build_params(_affine_draws(B, rng, fliplr=[1, 0, 1, 0, 1, 0], flipud=[0, 0, 1, 1, 0, 1], blur=np.ones(B, bool),
                                     sigma=[0.5, 1.6, 2.2, 2.4, 2.8, 2.999], order=[order] * B), S)
    assert p["klen_first" if blur_first else "klen_last"].tolist() == [5, 5, 7, 7, 9, 9]
    assert not p["klen_last" if blur_first else "klen_first"].any() and not p["identity"].any()
    _against_definition("chain S %d C %d blur %s" % (S, C, "first" if blur_first else "last"), _chain(img, p), img, p)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", SIZES)
def test_mirrors_identity_and_klen_0_are_exact(S, C):
    from scouter_amd import kernels as K
    img = _bytes(S, C, 4000 + S + C)
    p = A.build_params(_draws(B, fliplr=[0, 1, 0, 1, 1, 0], flipud=[0, 0, 1, 1, 1, 0],
                              order=[[0, 1, 2, 3]] * 4 + [[1, 0, 2, 3]] * 2), S)
    assert p["identity"].tolist() == [1, 0, 0, 0, 0, 1] and np.array_equal(p["minv"], np.rint(p["minv"]))
    got = _chain(img, p)
    for b, axes in enumerate([None, (2,), (1,), (1, 2), (1, 2), None]):
        assert np.array_equal(got[b], img[b] if axes is None else np.flip(img[b], axis=axes)), b
    # the identity MATRIX without the flag copies as well
    v = _dev(p)
    eye = torch.tensor([[1, 0, 0, 0, 1, 0]] * B, dtype=torch.float32, device=DEV)
    off = torch.zeros(B, dtype=torch.int32, device=DEV)
    assert np.array_equal(K.aug_warp(torch.from_numpy(img).to(DEV), eye, off).cpu().numpy(), img)
    assert np.array_equal(K.aug_blur(torch.from_numpy(img).to(DEV), off, v["taps"]).cpu().numpy(), img)
    # an integer translation shifts, with zeros shifted in
    if S > 5:
        shift = torch.tensor([[1, 0, -3, 0, 1, 2]] * B, dtype=torch.float32, device=DEV)
        want = np.zeros_like(img)
        want[:, :, :S - 2, 3:] = img[:, :, 2:, :S - 3]
        assert np.array_equal(K.aug_warp(torch.from_numpy(img).to(DEV), shift, off).cpu().numpy(), want)


def test_every_image_takes_its_own_stages():
    """all 16 combinations of the four coins, affine + blur in both orders: the batch equals the images one at a time"""
    S, C = 17, 3
    rng = np.random.default_rng(5)
    combos = [(f, u, a, b, first) for f in (0, 1) for u in (0, 1) for a in (0, 1) for b in (0, 1)
              for first in ((0, 1) if a and b else (0,))]
    n = len(combos)
    assert n == 20
    d = _affine_draws(n, rng, fliplr=[c[0] for c in combos], flipud=[c[1] for c in combos],
                      blur=[c[3] for c in combos], sigma=rng.uniform(0.2, 3.0, n),
                      order=[[0, 1, 3, 2] if c[4] else [0, 1, 2, 3] for c in combos])
    d["affine"] = np.asarray([c[2] for c in combos])
    p = A.build_params(d, S)
    assert sorted(set(zip((p["klen_first"] > 0).tolist(), (p["klen_last"] > 0).tolist(), p["identity"].tolist()))) == \
        [(False, False, 0), (False, False, 1), (False, True, 0), (False, True, 1), (True, False, 0)]
    img = _bytes(S, C, 5000, n)
    got = _chain(img, p)
    for b in range(n):
        one = {k: v[b:b + 1] for k, v in p.items()}
        assert np.array_equal(_chain(img[b:b + 1], one)[0], got[b]), combos[b]
    _against_definition("mixed batch", got, img, p)


def test_finish_is_the_table_lookup():
    from scouter_amd import kernels as K
    from scouter_amd.dataset.transform_func import NORMALIZE_VALUE, normalize_table
    for S, C, name in ((5, 1, "MNIST"), (17, 3, "ImageNet"), (33, 3, "ImageNet"), (32, 3, "ImageNet")):   # 32: four bytes at once
        lut = normalize_table(*NORMALIZE_VALUE[name])
        img = _bytes(S, C, 6000 + S)
        got = K.aug_finish(torch.from_numpy(img).to(DEV), lut.to(DEV)).cpu()
        want = lut[torch.arange(C)[None, :, None, None], torch.from_numpy(img).long()]
        assert got.dtype == torch.float32 and torch.equal(got, want), (S, C)


def _frames(rng, C=3):
    return [rng.integers(0, 256, (int(h), int(w), C), dtype=np.uint8)
            for h, w in [(37, 91), (17, 17), (120, 75), (64, 30), (5, 4), (300, 23), (96, 96)]]


def test_whole_transform_against_resize_oracle_and_definition():
    from scouter_amd import kernels as K
    from scouter_amd.dataset.transform_func import GpuTransform
    S = 17
    imgs = _frames(np.random.default_rng(12))
    frames = [torch.from_numpy(a) for a in imgs]
    resized = np.stack([P.resize_bilinear_u8(a, S, S).transpose(2, 0, 1) for a in imgs])
    assert np.array_equal(K.resize_u8([f.to(DEV) for f in frames], S).cpu().numpy(), resized)        # Pillow-exact bytes
    tf = GpuTransform("ImageNet", S, aug=True, aug_seed=3)
    got = tf(frames, DEV).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(imgs), 3, S, S) and tf.calls == 1
    p = A.build_params(A.draw_params(len(imgs), 3, 0, 0), S)
    want, raw = A.augment_host(resized, p, return_unrounded=True)
    c = torch.arange(3)[None, :, None, None]
    lut = tf.table
    differ = (got != lut[c, torch.from_numpy(want).long()]).numpy()
    tie = np.abs(raw - np.floor(raw) - 0.5) < 1e-3
    print("whole transform: %d of %d values differ, %d of them away from a tie" % (differ.sum(), differ.size, (differ & ~tie).sum()))
    assert not (differ & ~tie).any() and differ.mean() <= 0.005
    near = torch.from_numpy(want).long()
    one_off = (got == lut[c, (near + 1).clamp(max=255)]) | (got == lut[c, (near - 1).clamp(min=0)])
    assert one_off.numpy()[differ].all()                                                    # within 1 byte of the definition
    # aug=False is today's transform, bit for bit
    plain = GpuTransform("ImageNet", S, aug=False)(frames, DEV).cpu().numpy()
    assert np.array_equal(plain, GpuTransform("ImageNet", S)(frames, DEV).cpu().numpy())
    for b, a in enumerate(imgs):
        assert np.array_equal(plain[b], P.transform(a, S, "ImageNet")), b


def test_same_seed_same_batches_other_seed_or_rank_other_batches():
    from scouter_amd.dataset.transform_func import GpuTransform
    frames = [torch.from_numpy(a) for a in _frames(np.random.default_rng(13))]
    runs = {}
    for name, kw in (("a", dict(aug_seed=3)), ("b", dict(aug_seed=3)), ("seed", dict(aug_seed=4)),
                     ("rank", dict(aug_seed=3, rank=1))):
        tf = GpuTransform("ImageNet", 17, aug=True, **kw)
        runs[name] = [tf(frames, DEV).cpu() for _ in range(3)]
    for n in range(3):
        assert torch.equal(runs["a"][n], runs["b"][n]), n
        assert not torch.equal(runs["a"][n], runs["seed"][n]) and not torch.equal(runs["a"][n], runs["rank"][n]), n
    assert not torch.equal(runs["a"][0], runs["a"][1])                  # the transform counts its calls


def test_train_main_with_aug_on_image_folders(tmp_path, monkeypatch):
    """`python -m scouter_amd.train --aug true --synthetic_data false ...` end to end: the train loader augments, the
    validation loader does not"""
    Image = pytest.importorskip("PIL.Image")
    from scouter_amd import train
    rng = np.random.default_rng(9)
    for phase, n in (("train", 4), ("val", 2)):
        for wnid in ("n001", "n002"):
            d = tmp_path / "data" / phase / wnid
            d.mkdir(parents=True)
            for k in range(n):
                h, w = int(rng.integers(40, 90)), int(rng.integers(40, 90))
                Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / ("%d.jpg" % k), quality=90)
    args = train.get_args_parser().parse_args([
        "--dataset", "ImageNet", "--model", "resnet18", "--channel", "512", "--img_size", "32", "--num_classes", "2",
        "--slots_per_class", "1", "--pre_trained", "false", "--batch_size", "4", "--epochs", "1", "--num_workers", "0",
        "--synthetic_data", "false", "--aug", "true", "--aug_seed", "5", "--dataset_dir", str(tmp_path / "data") + "/",
        "--output_dir", ""])
    seen = []
    build = train._build_loaders

    def spy(a):
        out = build(a)
        seen.append(out)
        return out
    monkeypatch.setattr(train, "_build_loaders", spy)
    accs = train.param_translation(args)
    assert len(accs) == 2 and all(np.isfinite(a) and 0.0 <= a <= 1.0 for a in accs)
    (train_loader, val_loader, _), = seen
    assert train_loader.gpu_transform.aug and train_loader.gpu_transform.aug_seed == 5
    assert train_loader.gpu_transform.calls == 2                      # 8 training images in batches of 4
    assert not val_loader.gpu_transform.aug and val_loader.gpu_transform is not train_loader.gpu_transform
    assert args.aug_on_device is True
