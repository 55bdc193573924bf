"""Edge tests of the small kernels that close every training step (-m gpu): the FC head, the loss head, the elementwise passes,
the forward pools, the layout transposes, the radix softmax, fused AdamW and the int64 counter bump -- each against a plain fp64
restatement written here with torch-CPU / numpy (nothing of scouter_amd is used to form an expected value; the AdamW maths is
oracle.torch_oracle.adamw_step), at the sizes where a loop takes its second pass, a workgroup is partly idle, an optional argument
is absent or a pointer is not 16-byte aligned.  Inputs are fp32 values from seeded generators; the restatement reads the same fp32
values in fp64.

EPS = 2^-24 (half an fp32 ulp, relative); fp32 products, sums, quotients and square roots are correctly rounded; a contracted
multiply-add rounds once where the two operations round twice, so every count below holds either way.  Every derived bound is
twice a worst case: the roundings are counted and multiplied by the magnitude that is actually summed.

linear_small_fwd   a lane adds ceil(K / 64) products into its sum (one rounding each, fma or not more than two: the product's is
                   charged to the same term), the butterfly adds six levels, the bias one more: every term of sum |x w| passes
                   through at most ceil(K / 64) + 6 + 1 roundings of partial sums no larger than sum |x w| + |b|:
                   |y - ref| <= (ceil(K / 64) + 7) EPS (sum_k |x w| + |b|); twice that.
linear_small_bwd   dw[c][k] is one thread's sum of B products in the order of b: B EPS sum_b |dy x|; db likewise B EPS sum_b |dy|;
                   dx[b][k] is a sum of C products: C EPS sum_c |dy w|.  Twice each.  Two calls give the same bits (fixed order).
slot_loss          log_softmax: the maximum is exact, the sum of C exponentials rounds C times, m + logf(s) and row - lse once
                   each, the argument of expf once: C + 4 roundings plus the ulp errors of expf and logf, which the device libm
                   does not state.  So logp, the scalars of `stats` (sums over the batch of such terms, powf for the area term)
                   and the backward (expf(logp), powf) follow the project's parity rule: the HIP error is at most 1.5 times the
                   error of the same restatement evaluated in torch fp32 on the CPU, with a floor of 1e-6 of the result's scale
                   (the largest |entry| of the fp64 result).  top-1 is a count divided by B in fp32: exact.  stats[4], the area,
                   is an fp64 sum rounded once: 2 EPS.
relu_bwd           a selection: exact.  `v > 0` is false for +0, -0 and NaN and true for the smallest subnormal.
axpby              a alpha and b beta round once each (EPS |alpha a|, EPS |beta b|), their sum once more (EPS (|alpha a| +
                   |beta b|)); a contracted multiply-add saves one of them: 2 EPS (|alpha a| + |beta b|), the worst case itself
                   (not doubled).  (alpha, beta are the fp32 values the entry point receives.)
maxpool_fwd        a selection: values exact.  maxpool_bwd adds at most four dy (k = 3, s = 2) in fp32: 3 EPS sum |dy|, twice; with
                   integer-valued dy the sums are exact and the comparison with fp64 autograd is bit for bit.
bn_maxpool_fwd     against max_pool2d(relu(batch_norm(x))) in fp64 under the bound of test_batchnorm_relu_maxpool_fused:
                   2e-6 max |ref| + 1e-7.
avgpool_fwd        at most nine terms: eight additions and the division, 9 roundings of partial sums <= sum |x|:
                   9 EPS avg_pool(|x|), twice.  A bf16-stored input is read exactly, so the same bound holds against the fp64 pool
                   of the bf16-rounded values.
sa_apply_bwd       1 / HW rounds once and its product with dgap once (2 EPS |gp|); dout a + gp rounds at most twice
                   (EPS |dout a| + EPS (|dout a| + |gp|)): EPS (2 |dout a| + 3 |gp|), twice.
transpose          a copy: exact.
radix_softmax_fwd  d = z0 - z1; the rounding of d moves exp(-|d|) by |d| exp(-|d|) EPS <= 0.37 EPS, expf by 2 EPS e / (1 + e)^2 <=
                   0.5 EPS, the sum, the reciprocal and the product by EPS a each: under 4 EPS absolute (not doubled).  The
                   pair sums to 1 within 2 EPS.
radix_softmax_bwd  S = |a0 da0| + |a1 da1|.  Five roundings: two products and their sum (dot within 2 EPS S), the difference
                   da0 - dot (EPS (|da0| + S)) and the product with a0 (EPS a0 (|da0| + S)): a0 EPS (2 |da0| + 4 S).  The kernel
                   reads `a` as fp32, a relative EPS on a0 and a1: a0 EPS (|da0| + 2 S) more.  |dz - ref| <= a0 EPS (3 |da0| + 6 S)
                   + TINY (|da0| + S), TINY = 2^-126 for attention weights below the normal range (exp(-200) is 0 in fp32); twice.
adamw              the tolerance of test_fused_adamw_matches_adamw_maths (rtol 2e-6, atol 2e-7) after three steps; an aligned and a
                   misaligned copy of one parameter end with the same bits; elements next to a view keep their bits.
iadd_i64           integer: exact.

Measured on the MI355X (errors as fractions of the bound, and the parity figures): DESIGN.md, "Edge tests of the small kernels"."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as O                                        # noqa: E402

EPS = 2.0 ** -24
TINY = 2.0 ** -126
SENTINEL = -777.25
GRID_CAP_VECTORS = 2048 * 256           # ew_blocks caps the grid at 2048 workgroups of 256 threads, one 16-byte vector each


def K():
    from scouter_amd import kernels
    return kernels


def N():
    from scouter_amd import _native
    return _native


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def host64(t):
    return t.detach().cpu().double()


def figure(name, err, bound):
    """prints a measured error next to its bound before anything is asserted (DESIGN.md quotes these)"""
    print("EDGE %-44s err %.3e  bound %.3e  ratio %.3f" % (name, err, bound, err / bound if bound > 0 else 0.0))


def within(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound: fp64 tensor or number); NaN or inf in `got` fails"""
    got = host64(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
    i = int(ratio.argmax()) if ratio.numel() else 0
    figure(name, float(err.flatten()[i]), float(bound.flatten()[i]))
    assert bool((err <= bound).all()), "%s: |err| %.3e over the bound %.3e at flat index %d" % (
        name, float(err.flatten()[i]), float(bound.flatten()[i]), i)


def parity(name, got, ref64, ref32):
    """the project's parity rule: max |HIP - fp64| <= max(1.5 max |torch fp32 - fp64|, 1e-6 max |fp64|)"""
    got, ref32 = host64(got), host64(ref32)
    assert got.shape == ref64.shape == ref32.shape, (name, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    err = float((got - ref64).abs().max())
    err32 = float((ref32 - ref64).abs().max())
    scale = float(ref64.abs().max())
    bound = max(1.5 * err32, 1e-6 * scale)
    print("EDGE %-44s hip %.3e  torch-fp32 %.3e  scale %.3e  bound %.3e" % (name, err, err32, scale, bound))
    assert err <= bound, "%s: HIP error %.3e, torch fp32 error %.3e, scale %.3e" % (name, err, err32, scale)


# ---------------------------------------------------------------------------------------------------------------
# 1 / 2. FC head
# ---------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1), (3, 63, 5), (3, 64, 5), (3, 65, 5), (7, 130, 3), (70, 2048, 10), (2, 512, 200),
               (2, 3, 1)]             # (the last one: B C = 2 mod 4, which none of the others gives)
_head = {}


def head_case(shape):
    """inputs and fp64 results of one (B, K, C), formed once and left unchanged"""
    if shape not in _head:
        B, Kd, C = shape
        g = gen(1000 + B * 7 + Kd * 3 + C)
        x, w, b, dy = randn(g, B, Kd), randn(g, C, Kd) * 0.5, randn(g, C), randn(g, B, C)
        X, W, Bi, DY = x.double(), w.double(), b.double(), dy.double()
        r = dict(x=x, w=w, b=b, dy=dy)
        r["y0"] = X @ W.t()
        r["ymag"] = X.abs() @ W.abs().t()
        r["dx"], r["dxmag"] = DY @ W, DY.abs() @ W.abs()
        r["dw"], r["dwmag"] = DY.t() @ X, DY.abs().t() @ X.abs()
        r["db"], r["dbmag"] = DY.sum(0), DY.abs().sum(0)
        _head[shape] = r
    return _head[shape]


def test_head_shape_list_covers_the_partly_idle_workgroups():
    """the forward gives one wave to an output, four outputs to a workgroup: B C = 1, 2, 3 mod 4 leave waves idle behind the
    early return; K below, at and above one 64-lane pass"""
    assert {(B * C) % 4 for B, _, C in HEAD_SHAPES} >= {1, 2, 3}
    assert {Kd for _, Kd, _ in HEAD_SHAPES} >= {1, 63, 64, 65}


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "B%d_K%d_C%d" % s)
def test_head_forward(shape, with_bias):
    B, Kd, C = shape
    r = head_case(shape)
    kk = K()
    x, w, b = dev(r["x"]), dev(r["w"]), dev(r["b"]) if with_bias else None
    y = kk.linear_small_fwd(x, w, b)
    ref = r["y0"] + (r["b"].double() if with_bias else 0.0)
    mag = r["ymag"] + (r["b"].double().abs() if with_bias else 0.0)
    within("head fwd %s bias=%d" % (shape, with_bias), y, ref, 2 * (math.ceil(Kd / 64) + 7) * EPS * mag)
    assert torch.equal(y, kk.linear_small_fwd(x, w, b)), "two identical calls differ"


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "B%d_K%d_C%d" % s)
def test_head_backward(shape):
    """every combination of outputs the entry point allows: all three; dw and db without dx; dw alone; db alone (the bias of a
    frozen weight) -- an output that is given is written whichever others are left out, into buffers pre-filled with a sentinel"""
    B, Kd, C = shape
    r = head_case(shape)
    kk = K()
    x, w, dy = dev(r["x"]), dev(r["w"]), dev(r["dy"])
    bdx, bdw, bdb = 2 * C * EPS * r["dxmag"], 2 * B * EPS * r["dwmag"], 2 * B * EPS * r["dbmag"]
    new_dw = lambda: torch.full((C, Kd), SENTINEL, dtype=torch.float32, device="cuda")
    new_db = lambda: torch.full((C,), SENTINEL, dtype=torch.float32, device="cuda")
    tag = "head bwd %s " % (shape,)
    # all three, twice: same bits
    dw, db = new_dw(), new_db()
    dx = kk.linear_small_bwd(dy, x, w, dw, db)
    within(tag + "dx", dx, r["dx"], bdx)
    within(tag + "dw", dw, r["dw"], bdw)
    within(tag + "db", db, r["db"], bdb)
    dw2, db2 = new_dw(), new_db()
    dx2 = kk.linear_small_bwd(dy, x, w, dw2, db2)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), "two identical calls differ"
    # no dx
    dw3, db3 = new_dw(), new_db()
    assert kk.linear_small_bwd(dy, x, w, dw3, db3, need_dx=False) is None
    assert torch.equal(dw3, dw) and torch.equal(db3, db)
    # dw alone
    dw4 = new_dw()
    dx4 = kk.linear_small_bwd(dy, x, w, dw4, None)
    within(tag + "dw (db absent)", dw4, r["dw"], bdw)
    assert torch.equal(dw4, dw) and torch.equal(dx4, dx)
    # db alone
    db5 = new_db()
    dx5 = kk.linear_small_bwd(dy, x, w, None, db5)
    within(tag + "db (dw absent)", db5, r["db"], bdb)
    assert torch.equal(db5, db) and torch.equal(dx5, dx)
    db6 = new_db()
    kk.linear_small_bwd(dy, x, w, None, db6, need_dx=False)
    assert torch.equal(db6, db)


# ---------------------------------------------------------------------------------------------------------------
# 3. loss head
# ---------------------------------------------------------------------------------------------------------------
LAM = 0.7
LOSS_SHAPES = [(1, 10), (255, 10), (256, 10), (257, 10), (600, 10), (5, 1), (33, 200)]


def loss_inputs(B, C, area, scale=3.0, seed=0):
    g = gen(2000 + 13 * B + C + seed)
    logits = randn(g, B, C) * scale
    labels = torch.randint(0, C, (B,), generator=g)
    n_part = {"B": B, "1": 1, "none": 0}[area]
    area_part = (torch.rand(n_part, generator=g, dtype=torch.float32) * 100 + 100) if n_part else None
    G = randn(g, B, C)
    ups = torch.tensor([1.3, -0.6, 0.45], dtype=torch.float32)               # g_loss, g_nll, g_term
    return logits, labels, area_part, G, ups


def loss_restated(dtype, logits, labels, area_part, area_count, power, ups, G):
    """log_softmax -> nll_loss -> + lam * (sum(area_part) / area_count) ** power, and the gradients of
    a loss + b nll + c term + (G * logp).sum(), all in `dtype` on the CPU"""
    lg = logits.to(dtype).clone().requires_grad_(True)
    ap = None if area_part is None else area_part.to(dtype).clone().requires_grad_(True)
    logp = F.log_softmax(lg, 1)
    nll = F.nll_loss(logp, labels) if labels is not None else logp.sum() * 0
    if ap is not None:
        area = ap.sum() / area_count
        term = area ** power
    else:
        area = term = logp.sum() * 0
    loss = nll + LAM * term
    a, b, c = (0.0 if u is None else float(u) for u in ups)
    obj = a * loss + b * nll + c * term + ((G.to(dtype) * logp).sum() if G is not None else 0.0)
    if obj.requires_grad and (ups != (None, None, None) or G is not None):
        obj.backward()
    dl = lg.grad if lg.grad is not None else torch.zeros_like(lg)
    ga = None if ap is None else (ap.grad[:1] if ap.grad is not None else torch.zeros(1, dtype=dtype))
    return dict(logp=logp.detach(), loss=loss.detach().reshape(1), nll=nll.detach().reshape(1),
                term=term.detach().reshape(1), area=area.detach().reshape(1), dlogits=dl, g_area=ga)


def loss_fwd_raw(logits, labels, area_part, area_count, power):
    """the forward through the C ABI with every output word pre-filled: an unwritten word keeps the sentinel"""
    B, C = logits.shape
    lg, lb, ap = dev(logits), dev(labels), dev(area_part)
    logp = torch.full((B, C), SENTINEL, dtype=torch.float32, device="cuda")
    stats = torch.full((8,), SENTINEL, dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    N().check(N().lib().scouter_slot_loss_fwd_f32(p(lg), p(lb), p(ap), 0 if ap is None else ap.numel(), B, C,
                                                  float(area_count), LAM, float(power), p(logp), p(stats), K()._stream()),
              "slot_loss_fwd")
    return logp, stats


def loss_bwd_raw(logp32, labels, area32, ups, G, area_count, power):
    """the backward on the fp32 roundings of the restated logp and area (the forward kernel is not involved)"""
    kk = K()
    stats = torch.zeros(8, dtype=torch.float32)
    stats[4] = area32
    one = lambda u: None if u is None else torch.tensor([float(u)], dtype=torch.float32).cuda()
    return kk.slot_loss_bwd(dev(logp32), dev(labels), stats.cuda(), one(ups[0]), one(ups[1]), one(ups[2]), dev(G),
                            area_count, LAM, power)


def check_loss(tag, logits, labels, area_part, power, ups, G, area_count, check_fwd=True):
    r64 = loss_restated(torch.float64, logits, labels, area_part, area_count, power, ups, G)
    r32 = loss_restated(torch.float32, logits, labels, area_part, area_count, power, ups, G)
    B, C = logits.shape
    if check_fwd:
        logp, stats = loss_fwd_raw(logits, labels, area_part, area_count, power)
        parity(tag + " logp", logp, r64["logp"], r32["logp"])
        st = stats.cpu()
        for i, key in enumerate(("loss", "nll", "term")):
            parity(tag + " " + key, st[i:i + 1], r64[key], r32[key])
        if labels is not None:
            correct = int((logits.argmax(1) == labels).sum())
            assert float(st[3]) == float(np.float32(correct) / np.float32(B)), (tag, float(st[3]), correct, B)
        else:
            assert float(st[1]) == 0.0 and float(st[3]) == 0.0, tag
        within(tag + " area", st[4:5], r64["area"], 2 * EPS * r64["area"].abs())
        assert st[5:].tolist() == [0.0, 0.0, 0.0], (tag, st.tolist())
    dl, ga = loss_bwd_raw(r64["logp"].float(), labels, float(r64["area"].float()), ups, G, area_count, power)
    if all(u is None for u in ups) and G is None:
        assert not bool(dl.any()) and float(ga) == 0.0, tag
        return
    parity(tag + " dlogits", dl, r64["dlogits"], r32["dlogits"])
    if area_part is not None:
        parity(tag + " g_area_sum", ga, r64["g_area"], r32["g_area"])


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "B%d_C%d" % s)
def test_loss_shapes_powers_and_area_parts(shape):
    """B below, at and past one 256-thread pass (and far past it), C = 1 and C = 200, the three powers (power 1 has its own branch
    in the backward), the area partial sums per image, as one value and absent; all four upstream gradients present"""
    B, C = shape
    for power in (1, 2, 3):
        for area in ("B", "1", "none"):
            logits, labels, area_part, G, ups = loss_inputs(B, C, area, seed=power)
            check_loss("loss B%d C%d p%d area=%s" % (B, C, power, area), logits, labels, area_part, power, tuple(ups.tolist()),
                       G, float(B * 10 * 49))


@pytest.mark.parametrize("mask", range(16))
def test_loss_backward_every_subset_of_upstream_gradients(mask):
    """g_loss, g_nll, g_term and g_logp each present or NULL (NULL = 0) at B = 257"""
    B, C, power = 257, 10, 2
    logits, labels, area_part, G, ups = loss_inputs(B, C, "B")
    ups = tuple(float(u) if mask >> i & 1 else None for i, u in enumerate(ups))
    check_loss("loss subset %d%d%d%d" % tuple(mask >> i & 1 for i in range(4)), logits, labels, area_part, power, ups,
               G if mask >> 3 & 1 else None, float(B * 10 * 49), check_fwd=False)


def test_loss_without_labels():
    """labels = NULL on both kernels: nll = 0 and top-1 = 0 with logp still exact; dlogits = the softmax backward of g_logp alone"""
    B, C, power = 257, 10, 2
    logits, _, area_part, G, ups = loss_inputs(B, C, "B")
    check_loss("loss no labels", logits, None, area_part, power, tuple(ups.tolist()), G, float(B * 10 * 49))
    # the label terms really are absent: the same backward with g_loss = g_nll = 0 in the restatement of the labelled loss
    r = loss_restated(torch.float64, logits, None, area_part, float(B * 10 * 49), power, tuple(ups.tolist()), G)
    sm = F.softmax(logits.double(), 1)
    assert torch.allclose(r["dlogits"], G.double() - sm * G.double().sum(1, keepdim=True), rtol=0, atol=1e-12)


def test_loss_large_logits_need_the_max_subtraction():
    """logits of magnitude 80, a row holding +88 next to -88 and a row holding +100 next to -100: e^88 is within a factor two of
    the largest fp32 and e^100 is past it (expf overflows from 88.73 on), so logp is finite and right only with the row maximum
    subtracted first"""
    B, C, power = 33, 10, 2
    logits, labels, area_part, G, ups = loss_inputs(B, C, "B", scale=1.0)
    logits = (logits / logits.abs().max() * 80.0).contiguous()
    logits[7, 2], logits[7, 3] = 88.0, -88.0
    logits[11, 5], logits[11, 0] = 100.0, -100.0
    assert float(logits[:11].abs().max()) == 88.0 and float(logits.abs().max()) == 100.0
    assert math.isinf(float(torch.exp(logits.max()))) and not math.isinf(float(torch.exp(logits[:11].max())))      # (in fp32)
    check_loss("loss +-80", logits, labels, area_part, power, tuple(ups.tolist()), G, float(B * 10 * 49))
    logp, _ = loss_fwd_raw(logits, labels, area_part, float(B * 10 * 49), power)
    assert bool(torch.isfinite(logp).all()) and float(logp[7].min()) < -175.0 and float(logp[11].min()) < -199.0


def test_loss_argmax_tie_goes_to_the_first_maximum():
    """a row whose two largest logits are exactly equal counts as correct iff the label is the first of them"""
    g = gen(2100)
    B, C = 6, 10
    logits = randn(g, B, C)
    for b in (0, 1, 4):
        logits[b, 2] = logits[b, 7] = logits[b].max() + 1.0
    labels = torch.tensor([2, 7, int(logits[2].argmax()), (int(logits[3].argmax()) + 1) % C, 2, (int(logits[5].argmax()) + 1) % C])
    for b in (0, 1, 4):                     # the tie is there in fp32, and it is the maximum
        top = torch.sort(logits[b], descending=True).values
        assert float(top[0]) == float(top[1]) > float(top[2]) and int(logits[b].argmax()) == 2
    _, stats = loss_fwd_raw(logits, labels, None, 1.0, 1)
    assert float(stats[3]) == float(np.float32(3) / np.float32(B)), float(stats[3])      # rows 0, 2 and 4
    labels[0], labels[4] = 7, 7
    _, stats = loss_fwd_raw(logits, labels, None, 1.0, 1)
    assert float(stats[3]) == float(np.float32(1) / np.float32(B)), float(stats[3])      # row 2 alone


def test_loss_bad_labels_in_both_passes_of_a_thread():
    """B = 600: thread 3 holds row 3 in its first pass, thread 44 row 300 in its second.  Labels outside [0, C) are counted,
    poison loss / nll and exactly their own rows of dlogits; every other row is what it would be without them"""
    B, C, power = 600, 10, 2
    logits, labels, area_part, G, ups = loss_inputs(B, C, "B")
    ups = tuple(ups.tolist())
    good = labels.clone()
    labels[3], labels[300] = C, -1
    logp, stats = loss_fwd_raw(logits, labels, area_part, float(B * 10 * 49), power)
    r64 = loss_restated(torch.float64, logits, good, area_part, float(B * 10 * 49), power, ups, G)
    r32 = loss_restated(torch.float32, logits, good, area_part, float(B * 10 * 49), power, ups, G)
    st = stats.cpu()
    assert float(st[5]) == 2.0 and math.isnan(float(st[0])) and math.isnan(float(st[1])), st.tolist()
    assert st[6:].tolist() == [0.0, 0.0]
    parity("loss bad labels logp", logp, r64["logp"], r32["logp"])
    parity("loss bad labels term", st[2:3], r64["term"], r32["term"])
    dl, _ = loss_bwd_raw(r64["logp"].float(), labels, float(r64["area"].float()), ups, G, float(B * 10 * 49), power)
    nan_rows = torch.isnan(dl).all(1).cpu()
    assert nan_rows.nonzero().flatten().tolist() == [3, 300]
    keep = ~nan_rows
    assert bool(torch.isfinite(dl.cpu()[keep]).all())
    parity("loss bad labels dlogits (other rows)", dl.cpu()[keep], r64["dlogits"][keep], r32["dlogits"][keep])


# ---------------------------------------------------------------------------------------------------------------
# 4. elementwise passes
# ---------------------------------------------------------------------------------------------------------------
EW_SIZES = [4, 1024, 4 * (GRID_CAP_VECTORS + 257)]
SUBNORMAL = float(np.float32(2.0 ** -149))


@pytest.mark.parametrize("n", EW_SIZES)
def test_relu_bwd_mask_and_second_pass(n):
    """n = 4 (one vector), 1024 (one workgroup), and 257 vectors past the grid cap: those threads take a second vector and the
    last pass is ragged.  y holds +0, -0, the smallest subnormal and NaN at known places (in the second pass too)"""
    g = gen(3000 + n % 97)
    dy, y = randn(g, n), randn(g, n)
    specials = [0.0, -0.0, SUBNORMAL, math.nan]
    places = [0] if n == 4 else [0, n // 2, n - 4]
    for p0 in places:
        y[p0:p0 + 4] = torch.tensor(specials)
        dy[p0:p0 + 4] = torch.tensor([1.5, -2.5, 3.5, -4.5])
    assert float(y[places[-1] + 2]) == SUBNORMAL > 0.0 and math.copysign(1.0, float(y[places[-1] + 1])) == -1.0
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    if n > 4:
        frac = float((y > 0).float().mean())
        assert 0.4 < frac < 0.6, frac                                                 # (the mask is neither all ones nor all zeros)
    dx = K().relu_bwd(dev(dy), dev(y)).cpu()
    assert bool(torch.isfinite(dx).all())
    np.testing.assert_array_equal(dx.numpy(), ref.numpy())
    for p0 in places:
        assert dx[p0:p0 + 4].tolist() == [0.0, 0.0, 3.5, 0.0]


@pytest.mark.parametrize("n", EW_SIZES)
def test_axpby_forms(n):
    """alpha a + beta b; alpha a alone (b = NULL); in place (out = a); alpha = 0"""
    g = gen(3100 + n % 97)
    a, b = randn(g, n), randn(g, n)
    kk = K()
    al, be = float(np.float32(1.7)), float(np.float32(-0.3))
    A, Bt = a.double(), b.double()
    ad, bd = dev(a), dev(b)
    within("axpby n=%d" % n, kk.axpby(ad, bd, al, be), al * A + be * Bt, 2 * EPS * ((al * A).abs() + (be * Bt).abs()))
    within("axpby n=%d b=None" % n, kk.axpby(ad, None, al, be), al * A, 2 * EPS * (al * A).abs())
    within("axpby n=%d alpha=0" % n, kk.axpby(ad, bd, 0.0, be), be * Bt, 2 * EPS * (be * Bt).abs())
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b), "an input was written"
    io = dev(a).clone()
    out = kk.axpby(io, bd, al, be, out=io)
    assert out.data_ptr() == io.data_ptr()
    within("axpby n=%d out=a" % n, io, al * A + be * Bt, 2 * EPS * ((al * A).abs() + (be * Bt).abs()))
    io = dev(a).clone()
    kk.axpby(io, None, al, 1.0, out=io)
    within("axpby n=%d out=a b=None" % n, io, al * A, 2 * EPS * (al * A).abs())


def test_elementwise_refuse_a_length_that_is_no_multiple_of_four():
    """n = 6: refused with the entry point's message before any launch, the output keeps its contents"""
    kk, nat = K(), N()
    a = torch.arange(6, dtype=torch.float32, device="cuda") + 1.0
    b = -a
    out = torch.full((8,), SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"axpby: null pointer or n % 4 != 0"):
        kk.axpby(a, b, 2.0, 3.0, out=out[:6])
    with pytest.raises(RuntimeError, match=r"relu_bwd: null pointer or n % 4 != 0"):
        nat.check(nat.lib().scouter_relu_bwd_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), 6, kk._stream()), "relu_bwd")
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [SENTINEL] * 8


# ---------------------------------------------------------------------------------------------------------------
# 5. forward pools (and sa_apply_bwd) past the grid cap
# ---------------------------------------------------------------------------------------------------------------
POOL_SHAPE = (2, 257, 257, 64)
_pool = {}


def pool_input():
    """x as NHWC fp32 (host) and its NCHW fp64 view, formed once"""
    if not _pool:
        x = randn(gen(4000), *POOL_SHAPE)
        _pool["x"] = x
        _pool["x64"] = x.permute(0, 3, 1, 2).double()
        B, H, W, C = POOL_SHAPE
        assert B * 129 * 129 * C // 4 == 532512 > GRID_CAP_VECTORS
    return _pool["x"], _pool["x64"]


def nchw64(t):
    return host64(t).permute(0, 3, 1, 2)


def test_maxpool_forward_past_the_grid_cap():
    x, x64 = pool_input()
    kk = K()
    xr = x64.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    y, arg = kk.maxpool_fwd(dev(x))
    assert tuple(y.shape) == (2, 129, 129, 64)
    np.testing.assert_array_equal(nchw64(y).numpy(), ref.detach().numpy())
    # the arg-max taps, through the backward: fp64 autograd sends dy to the same input elements
    dy = randn(gen(4001), *y.shape)
    dy64 = dy.permute(0, 3, 1, 2).double()
    ref.backward(dy64)
    xa = x64.clone().requires_grad_(True)
    F.max_pool2d(xa, 3, 2, 1).backward(dy64.abs())
    dx = kk.maxpool_bwd(dev(dy), arg, POOL_SHAPE)
    within("maxpool_bwd past the cap", nchw64(dx), xr.grad, 2 * 3 * EPS * xa.grad)


def test_bn_maxpool_forward_past_the_grid_cap():
    """max_pool2d(relu(batch_norm(x))) with the batch statistics, the stem's fused forward"""
    x, x64 = pool_input()
    kk = K()
    C = POOL_SHAPE[3]
    g = gen(4002)
    gamma, beta = torch.rand(C, generator=g) + 0.5, randn(g, C) * 0.3
    rm, rv = randn(g, C) * 0.1, torch.rand(C, generator=g) + 0.5
    ref = F.max_pool2d(torch.relu(F.batch_norm(x64, rm.double(), rv.double(), gamma.double(), beta.double(), True, 0.1, 1e-5)),
                       3, 2, 1)
    xd = dev(x)
    saved = kk.bn_stats(xd, dev(gamma), dev(beta), dev(rm), dev(rv), True)
    y, arg = kk.bn_maxpool_fwd(xd, saved, 3, 2, 1)
    frac = float((ref == 0).double().mean())
    assert 0.0 < frac < 0.5, frac                               # some windows are all-negative (ReLU ties at zero), most are not
    within("bn_maxpool_fwd past the cap", nchw64(y), ref, 2e-6 * float(ref.abs().max()) + 1e-7)
    assert int(arg.max()) <= 8


@pytest.mark.parametrize("ceil_mode,count_include_pad", [(False, True), (True, False)], ids=["floor_cip", "ceil_nocip"])
@pytest.mark.parametrize("store", ["fp32", "bf16"])
def test_avgpool_forward_past_the_grid_cap(store, ceil_mode, count_include_pad):
    x, x64 = pool_input()
    kk = K()
    if store == "bf16":
        xs = x.to(torch.bfloat16)
        x64 = xs.permute(0, 3, 1, 2).double()
        assert not torch.equal(xs.float(), x)
    else:
        xs = x
    ref = F.avg_pool2d(x64, 3, 2, 1, ceil_mode=ceil_mode, count_include_pad=count_include_pad)
    mag = F.avg_pool2d(x64.abs(), 3, 2, 1, ceil_mode=ceil_mode, count_include_pad=count_include_pad)
    y = kk.avgpool_fwd(dev(xs), 3, 2, 1, ceil_mode, count_include_pad)
    assert tuple(y.shape) == (2, 129, 129, 64) == tuple(ref.permute(0, 2, 3, 1).shape)
    within("avgpool_fwd %s ceil=%d cip=%d" % (store, ceil_mode, count_include_pad), nchw64(y), ref, 2 * 9 * EPS * mag)


def test_sa_apply_bwd_past_the_grid_cap():
    """dx[b, hw, r Cp + c] = dout[b, hw, c] a[b, r Cp + c] + dgap[b, c] / HW at (B, HW, Cp) = (2, 4100, 256): 524 800 vectors"""
    B, H, W, Cp = 2, 50, 82, 256
    assert H * W == 4100 and B * H * W * Cp // 4 == 524800 > GRID_CAP_VECTORS
    g = gen(4003)
    dout, dgap = randn(g, B, H, W, Cp), randn(g, B, Cp) * 50.0
    a = torch.softmax(randn(g, B, 2, Cp), 1).reshape(B, 2 * Cp).contiguous()
    dx = K().sa_apply_bwd(dev(dout), dev(a), dev(dgap))
    D, A, Gp = dout.double(), a.double(), dgap.double() / (H * W)
    da = torch.cat([D * A[:, None, None, :Cp], D * A[:, None, None, Cp:]], -1)
    gp = torch.cat([Gp, Gp], 1)[:, None, None, :]
    assert float(gp.abs().mean()) > 1e-3 * float(da.abs().mean())             # (the dgap term is not lost in the bound)
    within("sa_apply_bwd past the cap", dx, da + gp, 2 * EPS * (2 * da.abs() + 3 * gp.abs()))


# ---------------------------------------------------------------------------------------------------------------
# 6. max-pool semantics: ties and NaN
# ---------------------------------------------------------------------------------------------------------------
def tie_input():
    g = gen(5000)
    x = torch.randint(-1, 2, (2, 9, 9, 8), generator=g).float()
    dy = torch.randint(-8, 9, (2, 5, 5, 8), generator=g).float()                   # (integers: the backward's sums are exact)
    return x, dy


def check_maxpool_like_torch_cpu(tag, x, dy):
    kk = K()
    xr = x.permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    ref.backward(dy.permute(0, 3, 1, 2).double().contiguous())
    y, arg = kk.maxpool_fwd(dev(x))
    np.testing.assert_array_equal(nchw64(y).numpy(), ref.detach().numpy(), err_msg=tag + ": values")
    dx = kk.maxpool_bwd(dev(dy), arg, tuple(x.shape))
    assert bool(torch.isfinite(dx).all())
    np.testing.assert_array_equal(nchw64(dx).numpy(), xr.grad.numpy(), err_msg=tag + ": gradient (arg-max taps)")
    return ref.detach()


def test_maxpool_first_maximum_wins_on_ties():
    x, dy = tie_input()
    patches = F.unfold(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=-math.inf), 3, stride=2).view(2, 8, 9, 25)
    tied = ((patches == patches.max(2, keepdim=True).values).sum(2) >= 2).float().mean()
    assert float(tied) >= 0.5, float(tied)
    assert bool((dy != 0).float().mean() > 0.8)
    check_maxpool_like_torch_cpu("ties", x, dy)


def test_maxpool_nan_propagates_and_takes_the_gradient():
    """NaN at an interior pixel, at a corner, at the last tap of a window, and two in one window: every window that holds one
    returns NaN and its gradient goes to the last NaN in scan order (torch CPU: `val > max || isnan(val)`)"""
    x, dy = tie_input()
    x[0, 4, 4, 0] = math.nan            # interior, the centre tap of window (2, 2)
    x[0, 0, 0, 1] = math.nan            # corner: window (0, 0) alone
    x[1, 8, 8, 2] = math.nan            # the other corner: the last valid tap of window (4, 4)
    x[1, 3, 3, 3] = math.nan            # tap (2, 2), the last, of window (1, 1) -- and the first of window (2, 2)
    x[0, 3, 3, 4] = x[0, 3, 4, 4] = math.nan                                     # two in window (2, 2): (3, 4) is the later one
    ref = check_maxpool_like_torch_cpu("nan", x, dy)
    nan = torch.isnan(ref)
    assert nan[0, 0].nonzero().tolist() == [[2, 2]]
    assert nan[0, 1].nonzero().tolist() == [[0, 0]] and nan[1, 2].nonzero().tolist() == [[4, 4]]
    assert nan[1, 3].nonzero().tolist() == [[1, 1], [1, 2], [2, 1], [2, 2]]
    assert nan[0, 4].nonzero().tolist() == [[1, 1], [1, 2], [2, 1], [2, 2]]      # (windows (1, 2) and (2, 2) hold both)
    assert int(nan.sum()) == 1 + 1 + 1 + 4 + 4


# ---------------------------------------------------------------------------------------------------------------
# 7. layout transposes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 1, 1), (2, 1, 5, 10), (3, 31, 3, 11), (2, 33, 31, 1), (1, 64, 25, 41),
                                   (2, 200, 7, 7)], ids=lambda s: "B%d_C%d_%dx%d" % s)
def test_transposes_ragged_against_the_tile(shape):
    """rows and columns below 32, equal to 1, ragged against the 32 x 32 tile on both sides, batch 1; every element distinct"""
    B, C, H, W = shape
    kk = K()
    x = (torch.arange(B * C * H * W, dtype=torch.float32) * 0.5 - 7.0).view(B, C, H, W)
    nhwc = kk.nchw_to_nhwc(dev(x))
    assert tuple(nhwc.shape) == (B, H, W, C)
    assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous())
    back = kk.nhwc_to_nchw(nhwc)
    assert torch.equal(back.cpu(), x)
    y = (torch.arange(B * C * H * W, dtype=torch.float32) * -0.25 + 3.0).view(B, H, W, C)
    assert torch.equal(kk.nhwc_to_nchw(dev(y)).cpu(), y.permute(0, 3, 1, 2).contiguous())


# ---------------------------------------------------------------------------------------------------------------
# 8. radix softmax
# ---------------------------------------------------------------------------------------------------------------
RADIX_SHAPES = [(1, 4), (3, 100), (5, 512)]


def test_radix_shape_list_has_partly_idle_workgroups():
    """one thread per radix pair, 256 to a workgroup: a last workgroup that is partly idle, and more than one workgroup"""
    assert sum((B * Cp) % 256 != 0 for B, Cp in RADIX_SHAPES) >= 2 and max(B * Cp for B, Cp in RADIX_SHAPES) > 256


@pytest.mark.parametrize("B,Cp", RADIX_SHAPES)
def test_radix_softmax_large_differences(B, Cp):
    g = gen(6000 + Cp)
    z = randn(g, B, 2, Cp)
    z[:, :, 0::4] *= 120.0                                 # every fourth column: z0 - z1 of either sign in the hundreds
    z[0, 0, 0], z[0, 1, 0] = 130.0, -90.0                  # +220
    z[0, 0, 1 % Cp + 1], z[0, 1, 1 % Cp + 1] = -101.0, 100.0     # -201
    d = z[:, 0] - z[:, 1]
    assert float(d.max()) >= 200.0 and float(d.min()) <= -200.0 and float(d.abs().min()) < 5.0      # (saturated and not)
    kk = K()
    zf = z.reshape(B, 2 * Cp).contiguous()
    a = kk.radix_softmax_fwd(dev(zf))
    zr = zf.double().clone().requires_grad_(True)
    ref = torch.softmax(zr.view(B, 2, Cp), 1).view(B, 2 * Cp)
    within("radix_softmax_fwd B%d Cp%d" % (B, Cp), a, ref.detach(), 4 * EPS)
    ah = host64(a)
    assert float(ah.min()) >= 0.0 and float(ah.max()) <= 1.0
    pair = float((ah[:, :Cp] + ah[:, Cp:] - 1.0).abs().max())
    figure("radix_softmax_fwd B%d Cp%d pair sum" % (B, Cp), pair, 2 * EPS)
    assert pair <= 2 * EPS
    assert float(ah.min()) == 0.0 and float(ah.max()) == 1.0                     # (the saturated columns are there)
    # backward on the fp32 rounding of the restated attention
    da = randn(g, B, 2 * Cp) * 2.0
    ref.backward(da.double())
    a32 = ref.detach().float()
    dz = kk.radix_softmax_bwd(dev(a32), dev(da))
    A, D = ref.detach(), da.double()
    S = (A[:, :Cp] * D[:, :Cp]).abs() + (A[:, Cp:] * D[:, Cp:]).abs()
    S2 = torch.cat([S, S], 1)
    within("radix_softmax_bwd B%d Cp%d" % (B, Cp), dz, zr.grad,
           2 * (EPS * A * (3 * D.abs() + 6 * S2) + TINY * (D.abs() + S2)))


# ---------------------------------------------------------------------------------------------------------------
# 9. fused AdamW
# ---------------------------------------------------------------------------------------------------------------
def test_adamw_chunk_edges_and_misaligned_parameters():
    """Lengths around the 16 384-element chunk that are no multiples of four, and two parameters that are views one and two
    elements into a larger allocation: their chunks fail `(p & 15) == 0` and take the scalar route.  The second view's gradient
    (and moments) sit at an odd arena offset as well."""
    from scouter_amd.optim import FusedAdamW
    g = gen(7000)
    lengths = [1, 3, 16383, 16384, 16385, 16387, 32768 + 5]
    assert FusedAdamW.CHUNK == 16384
    VIEW1, VIEW2 = 16387, 37                     # view 1 repeats the aligned parameter of the same length (index 5)
    init = [randn(g, n) for n in lengths]
    init_v2 = randn(g, VIEW2)
    back1 = torch.full((VIEW1 + 9,), SENTINEL, dtype=torch.float32, device="cuda")
    back2 = torch.full((VIEW2 + 9,), SENTINEL, dtype=torch.float32, device="cuda")
    ps = [torch.nn.Parameter(t.cuda()) for t in init]
    p_v1 = torch.nn.Parameter(back1[1:1 + VIEW1])
    p_v2 = torch.nn.Parameter(back2[2:2 + VIEW2])
    with torch.no_grad():
        p_v1.copy_(init[5].cuda())
        p_v2.copy_(init_v2.cuda())
    assert p_v1.data_ptr() == back1.data_ptr() + 4 and p_v1.data_ptr() % 16 == 4
    assert p_v2.data_ptr() == back2.data_ptr() + 8 and p_v2.data_ptr() % 16 == 8
    assert all(p.data_ptr() % 16 == 0 for p in ps)
    params = ps + [p_v1, p_v2]
    sizes = lengths + [VIEW1, VIEW2]
    flat = torch.zeros(sum((n + 3) // 4 * 4 for n in sizes) + 4, device="cuda")
    off = 0
    for i, (p, n) in enumerate(zip(params, sizes)):
        o = off + 1 if i == len(params) - 1 else off
        p.grad = flat[o:o + n]
        off += (n + 3) // 4 * 4
    assert (p_v2.grad.data_ptr() - flat.data_ptr()) // 4 % 4 == 1 and (p_v1.grad.data_ptr() - flat.data_ptr()) % 16 == 0
    inits = init + [init[5], init_v2]
    ref_p = [t.double().clone() for t in inits]
    ref_m = [torch.zeros_like(r) for r in ref_p]
    ref_v = [torch.zeros_like(r) for r in ref_p]
    opt = FusedAdamW(params, lr=1e-2, weight_decay=0.05)
    for step in range(1, 4):
        grads = [randn(g, n) for n in sizes]
        grads[7] = grads[5]                      # the misaligned copy gets the aligned parameter's gradients
        for p, gi in zip(params, grads):
            p.grad.copy_(gi.cuda())
        opt.step()
        for r, gi, m, v in zip(ref_p, grads, ref_m, ref_v):
            O.adamw_step(r, gi.double(), m, v, step, lr=1e-2, weight_decay=0.05)
    for i, (p, r) in enumerate(zip(params, ref_p)):
        got = p.detach().cpu().double()
        figure("adamw param %d (n = %d)" % (i, sizes[i]), float((got - r).abs().max()), 2e-7 + 2e-6 * float(r.abs().max()))
        np.testing.assert_allclose(got.numpy(), r.numpy(), rtol=2e-6, atol=2e-7)
    assert torch.equal(p_v1.detach(), ps[5].detach()), "the scalar route and the 16-byte route give different bits"
    for back, lo, n in ((back1, 1, VIEW1), (back2, 2, VIEW2)):
        outside = torch.cat([back[:lo], back[lo + n:]]).cpu()
        assert outside.numel() == 9 and outside.tolist() == [SENTINEL] * 9, outside.tolist()


# ---------------------------------------------------------------------------------------------------------------
# 10. the int64 counter bump
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2 ** 40 + 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_iadd_i64(n, v):
    """values past 2^31 and past 2^53 (no detour through int32 or a double); the element after the n-th keeps its value"""
    g = gen(8000 + n)
    start = torch.randint(-2 ** 40, 2 ** 40, (n + 1,), generator=g, dtype=torch.int64)
    start[0] = 2 ** 31 - 1
    start[n - 1] = 2 ** 53 + 1
    if n > 2:
        start[1] = 2 ** 31 - 1
    buf = start.cuda()
    out = K().iadd_i64(buf[:n], v)
    assert out.data_ptr() == buf.data_ptr()
    expect = start.clone()
    expect[:n] += v
    assert torch.equal(buf.cpu(), expect)
    assert int(buf[n]) == int(start[n])
