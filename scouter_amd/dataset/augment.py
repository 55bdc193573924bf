"""`--aug true`: the reference's training augmentation (tools/image_aug.py, an imgaug Sequential with random_order=True)
as a definition that a device can run.  It sits where the reference has it (dataset/transform_func.py:112-118): after
Resize((S, S)), before ToTensor and Normalize, on the S x S x C BYTE image -- here planar bytes [B, C, S, S].

Per image (`draw_params`; ranges of image_aug.py:14-24, 46-57): four independent fair coins fliplr, flipud, affine, blur;
with affine an integer rotation in [-10, 9] degrees, scale_x, scale_y ~ U(0.8, 1.0), translate_x ~ U(0, 0.1) and
translate_y ~ U(-0.1, 0.1) as fractions of S; with blur sigma ~ U(0, 3.0); and a uniformly random order of the
operations that are present.

Reduction to at most three stages (`build_params`).  A mirror commutes exactly with a symmetric blur under a reflecting
border, and bilinear sampling with a constant-0 border commutes exactly with a mirror of the source; so the mirrors and
the affine compose, in their drawn order, into ONE 3x3 matrix M (source -> destination; each later operation multiplies
on the left) and only the relative order of affine and blur survives: blur_first, warp, blur_last.  An image with blur
and no affine blurs last.  In float64:
    fliplr [[-1, 0, S-1], [0, 1, 0]]        flipud [[1, 0, 0], [0, -1, S-1]]
    affine T(c, c) . T(tx S, ty S) . R(theta) . diag(sx, sy) . T(-c, -c),  c = (S - 1) / 2,
           R = [[cos, -sin], [sin, cos]] acting on (x, y) with y pointing down
The top two rows of the inverse of M travel as float32 [B, 6].

Warp.  Output pixel (x, y) reads u = m0 x + m1 y + m2, v = m3 x + m4 y + m5, evaluated in float32 as two rounded
products, their rounded sum, then the rounded sum with the constant (no fused multiply-add).  The four taps around
(floor u, floor v) are weighted with the fractional parts, a tap outside the image counts as 0, top and bottom rows are
interpolated along x and then along y; the result is rounded half to even, clamped to [0, 255] and stored as a byte.
With mirrors only every entry of the matrix is an integer and the result is an exact permutation of the bytes; the
identity copies.

Blur.  sigma < 1e-3: none.  Otherwise k = 3.3 sigma below sigma 3 (2.9 sigma below 5, 2.6 sigma above: imgaug's rule,
kept whole), klen = int(max(k, 5)), plus 1 if even -- 5, 7 or 9 for the drawn range.  Taps exp(-i^2 / (2 sigma^2)),
normalised to sum 1 in float64, then float32.  Border reflect-101 (index -i reads i, S-1+i reads S-1-i; needs S >= 5).
Row pass, then column pass, no rounding in between, products summed in ascending tap order, ONE round-half-to-even to a
byte at the end.

Finish.  out[b, c, y, x] = table[c][byte] with the [C, 256] normalisation table (transform_func.normalize_table).

Departures from imgaug / OpenCV, all deliberate: (1) our own random stream (Philox keyed by seed, batch number and rank,
not Python's and numpy's global generators); (2) a float bilinear warp instead of OpenCV's 1/32-pixel fixed-point warp;
(3) a float blur instead of its 8-bit fixed-point blur; (4) the translation is not rounded to whole pixels.

`augment_host` is this definition in numpy float64 (coordinates from the same float32 matrix in the float32 steps named
above, blur from the same float32 taps): the yardstick of the tests, and what GpuTransform runs when the target device is
not a GPU.  The device kernels are csrc/augment.hip (kernels.aug_blur / aug_warp / aug_finish)."""
import numpy as np

OPS = ("fliplr", "flipud", "affine", "blur")
MAX_KLEN = 9
ROW_WORDS = 20      # one image's row of the packed device table, in 4-byte words (pack_params)


def draw_params(n, seed, call, rank=0):
    """The random draws of `n` images of batch number `call`: a pure function of (seed, call, rank).  dict of arrays [n]:
    the four coins (bool), rotate (int64 degrees), scale_x, scale_y, translate_x, translate_y, sigma (float64; the neutral
    value where the coin is off) and `order` [n, 4]: the rank of OPS[j] in the image's sequence (a uniform permutation;
    the operations that are present run in the order of their ranks)."""
    gen = np.random.Generator(np.random.Philox(key=int(seed), counter=[int(call), int(rank), 0, 0]))
    coins = gen.integers(0, 2, size=(n, 4)).astype(bool)
    rotate = gen.integers(-10, 10, size=n)
    scale = gen.uniform(0.8, 1.0, size=(n, 2))
    tx, ty = gen.uniform(0.0, 0.1, size=n), gen.uniform(-0.1, 0.1, size=n)
    sigma = gen.uniform(0.0, 3.0, size=n)
    order = np.argsort(gen.random(size=(n, 4)), axis=1).argsort(axis=1)
    aff, blur = coins[:, 2], coins[:, 3]
    return {"fliplr": coins[:, 0].copy(), "flipud": coins[:, 1].copy(), "affine": aff.copy(), "blur": blur.copy(),
            "rotate": np.where(aff, rotate, 0), "scale_x": np.where(aff, scale[:, 0], 1.0),
            "scale_y": np.where(aff, scale[:, 1], 1.0), "translate_x": np.where(aff, tx, 0.0),
            "translate_y": np.where(aff, ty, 0.0), "sigma": np.where(blur, sigma, 0.0), "order": order}


def blur_klen(sigma):
    """imgaug's kernel length for GaussianBlur(sigma); 0 = no blur"""
    if sigma < 1e-3:
        return 0
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    klen = int(max(k, 5))
    return klen + 1 if klen % 2 == 0 else klen


def blur_taps(sigma):
    """float32 [klen]: the sampled Gaussian, normalised in float64"""
    klen = blur_klen(sigma)
    i = np.arange(klen, dtype=np.float64) - klen // 2
    t = np.exp(-i * i / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).astype(np.float32)


def _translations(tx, ty):
    m = np.tile(np.eye(3), (len(tx), 1, 1))
    m[:, 0, 2], m[:, 1, 2] = tx, ty
    return m


def affine_matrices(S, rotate, scale_x, scale_y, translate_x, translate_y):
    """float64 [n, 3, 3]: T(c, c) . T(tx S, ty S) . R(theta) . diag(sx, sy) . T(-c, -c) for n images at once"""
    rotate, scale_x, scale_y, translate_x, translate_y = (np.atleast_1d(np.asarray(v, np.float64)) for v in
                                                          (rotate, scale_x, scale_y, translate_x, translate_y))
    n, c, th = len(rotate), (S - 1) / 2.0, np.radians(rotate)
    rot, dia = np.tile(np.eye(3), (n, 1, 1)), np.tile(np.eye(3), (n, 1, 1))
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    dia[:, 0, 0], dia[:, 1, 1] = scale_x, scale_y
    centre = np.full(n, c)
    return _translations(centre, centre) @ _translations(translate_x * S, translate_y * S) @ rot @ dia \
        @ _translations(-centre, -centre)


def op_matrix(op, S, rotate=0, scale_x=1.0, scale_y=1.0, translate_x=0.0, translate_y=0.0):
    """float64 3x3 (source -> destination) of one geometric operation on an S x S image"""
    if op == "fliplr":
        return np.array([[-1.0, 0.0, S - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    if op == "flipud":
        return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, S - 1.0], [0.0, 0.0, 1.0]])
    if op != "affine":
        raise ValueError("no matrix for %r" % (op,))
    return affine_matrices(S, rotate, scale_x, scale_y, translate_x, translate_y)[0]


def build_params(draws, S):
    """draws of `draw_params` (or hand-made ones with the same keys) -> the stage parameters of the n images:
    minv float32 [n, 6] (top two rows of the inverse of M), identity int32 [n] (1: M is the identity, the warp copies),
    klen_first / klen_last int32 [n] (0: that blur copies), taps float32 [n, 9] (the first klen entries).  All images at
    once: this runs on the training thread for every batch."""
    S = int(S)
    if S < 5:
        raise ValueError("augmentation needs an image side of at least 5 (reflect-101 border of a 9-tap blur), got %d" % S)
    coin = {op: np.asarray(draws[op]).astype(bool) for op in OPS}
    order = np.asarray(draws["order"])
    n = len(coin["affine"])
    # the three geometric operations, the identity where the coin is off, multiplied from the left in the order of their ranks
    eye = np.eye(3)
    geo = np.stack([np.where(coin["fliplr"][:, None, None], op_matrix("fliplr", S), eye),
                    np.where(coin["flipud"][:, None, None], op_matrix("flipud", S), eye),
                    np.where(coin["affine"][:, None, None],
                             affine_matrices(S, draws["rotate"], draws["scale_x"], draws["scale_y"], draws["translate_x"],
                                             draws["translate_y"]), eye)], axis=1)
    turn = np.argsort(order[:, :3], axis=1, kind="stable")
    M = np.tile(eye, (n, 1, 1))
    for k in range(3):
        M = geo[np.arange(n), turn[:, k]] @ M
    out = {"minv": np.linalg.inv(M)[:, :2].reshape(n, 6).astype(np.float32),
           "identity": (~(coin["fliplr"] | coin["flipud"] | coin["affine"])).astype(np.int32),
           "klen_first": np.zeros(n, np.int32), "klen_last": np.zeros(n, np.int32),
           "taps": np.zeros((n, MAX_KLEN), np.float32)}
    sigma = np.where(coin["blur"], np.asarray(draws["sigma"], np.float64), 0.0)
    klen = np.array([blur_klen(v) for v in sigma], np.int32)
    if klen.max(initial=0) > MAX_KLEN:
        raise ValueError("blur of sigma %g needs %d taps, more than %d" % (sigma.max(), klen.max(), MAX_KLEN))
    for k in np.unique(klen[klen > 0]):                      # (the same expression as blur_taps, a kernel length at a time)
        rows = klen == k
        i = np.arange(k, dtype=np.float64) - k // 2
        t = np.exp(-i * i / (2.0 * sigma[rows, None] ** 2))
        out["taps"][rows, :k] = (t / t.sum(axis=1, keepdims=True)).astype(np.float32)
    first = coin["affine"] & (order[:, 3] < order[:, 2])
    out["klen_first"], out["klen_last"] = np.where(first, klen, 0).astype(np.int32), np.where(first, 0, klen).astype(np.int32)
    return out


def pack_params(p):
    """stage parameters -> ONE int32 array [n, ROW_WORDS] for one host-to-device copy: words 0-2 klen_first, klen_last,
    identity; 4-9 the bits of minv; 10-18 the bits of taps (views: `unpack_views`)."""
    n = len(p["identity"])
    row = np.zeros((n, ROW_WORDS), np.int32)
    row[:, 0], row[:, 1], row[:, 2] = p["klen_first"], p["klen_last"], p["identity"]
    row[:, 4:10] = np.ascontiguousarray(p["minv"], np.float32).view(np.int32)
    row[:, 10:19] = np.ascontiguousarray(p["taps"], np.float32).view(np.int32)
    return row


def unpack_views(table):
    """int32 torch tensor [n, ROW_WORDS] (any device) -> dict of strided views with the keys of `build_params`"""
    import torch
    f = table.view(torch.float32)
    return {"klen_first": table[:, 0], "klen_last": table[:, 1], "identity": table[:, 2], "minv": f[:, 4:10],
            "taps": f[:, 10:19]}


# ---- the definition, stage by stage, in float64 (values BEFORE the final rounding)
def warp_host_unrounded(img, minv):
    """img uint8 [C, S, S], minv float32 [6] -> float64 [C, S, S]"""
    C, S, _ = img.shape
    m = np.asarray(minv, np.float32)
    x, y = np.arange(S, dtype=np.float32)[None, :], np.arange(S, dtype=np.float32)[:, None]
    u = ((m[0] * x).astype(np.float32) + (m[1] * y).astype(np.float32)).astype(np.float32) + m[2]
    v = ((m[3] * x).astype(np.float32) + (m[4] * y).astype(np.float32)).astype(np.float32) + m[5]
    assert u.dtype == np.float32 and v.dtype == np.float32
    fu, fv = np.floor(u), np.floor(v)
    ax, ay = (u - fu).astype(np.float64), (v - fv).astype(np.float64)
    x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
    src = img.astype(np.float64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
        return np.where(ok[None], src[:, np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)], 0.0)
    top = tap(y0, x0) * (1.0 - ax) + tap(y0, x0 + 1) * ax
    bottom = tap(y0 + 1, x0) * (1.0 - ax) + tap(y0 + 1, x0 + 1) * ax
    return top * (1.0 - ay) + bottom * ay


def blur_host_unrounded(img, taps):
    """img uint8 [C, S, S], float32 taps [klen] (odd) -> float64 [C, S, S]"""
    C, S, _ = img.shape
    klen = len(taps)
    r, t = klen // 2, np.asarray(taps, np.float32).astype(np.float64)
    if klen % 2 != 1 or r > S - 1:
        raise ValueError("blur: odd tap count with radius below the image side expected (klen %d, side %d)" % (klen, S))
    p = np.pad(img.astype(np.float64), ((0, 0), (0, 0), (r, r)), mode="reflect")
    rows = np.zeros((C, S, S))
    for i in range(klen):
        rows += t[i] * p[:, :, i:i + S]
    p = np.pad(rows, ((0, 0), (r, r), (0, 0)), mode="reflect")
    out = np.zeros((C, S, S))
    for i in range(klen):
        out += t[i] * p[:, i:i + S, :]
    return out


def to_byte(values):
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)


def augment_host(bytes_bcss, params, return_unrounded=False):
    """uint8 [B, C, S, S] and the stage parameters of `build_params` -> augmented uint8 [B, C, S, S].  With
    `return_unrounded` also the float64 values of every image's LAST stage before they were rounded (the bytes themselves
    for an image no stage touches)."""
    src = np.asarray(bytes_bcss)
    if src.dtype != np.uint8 or src.ndim != 4 or src.shape[2] != src.shape[3]:
        raise ValueError("augment_host: uint8 [B, C, S, S] expected, got %s %s" % (src.dtype, src.shape))
    if src.shape[2] < 5:
        raise ValueError("augment_host: an image side of at least 5 expected, got %d" % src.shape[2])
    out, raw = np.empty_like(src), np.empty(src.shape, np.float64)
    for b in range(src.shape[0]):
        img = src[b]
        val = img.astype(np.float64)
        if params["klen_first"][b]:
            val = blur_host_unrounded(img, params["taps"][b][:int(params["klen_first"][b])])
            img = to_byte(val)
        if not params["identity"][b]:
            val = warp_host_unrounded(img, params["minv"][b])
            img = to_byte(val)
        if params["klen_last"][b]:
            val = blur_host_unrounded(img, params["taps"][b][:int(params["klen_last"][b])])
            img = to_byte(val)
        out[b], raw[b] = img, val
    return (out, raw) if return_unrounded else out
