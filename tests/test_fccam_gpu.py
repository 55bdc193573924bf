"""CAM of the FC baseline (-m gpu): the kernel of csrc/fccam.hip against fp64 under the worst-case fp32 bound of any summation
order, the bit identities its fixed order promises, its refusals, and tools/attribution.py fccam / fccam_maps on a whole model:
against the fp64 contraction of the fc weight with the HIP path's own features, and against the model's own output (the maps of
an image, averaged and biased, are its logits)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gradcam_gpu import bn_buffers, build                             # noqa: E402

# the ragged and the largest columns of test_gradcam_gpu.py GRADCAM_SHAPES: C off a multiple of 4 (the scalar route), below,
# at and above one 2048-channel piece, N off a multiple of the 8-position tile
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 70), (3, 2, 3, 65), (2, 7, 7, 512), (2, 7, 7, 2048), (1, 9, 9, 2048), (2, 3, 3, 130),
          (1, 4, 4, 4100), (1, 5, 5, 8192)]
N_CLASSES = [1, 10, 200]
SENTINEL = -777.25
U = 2.0 ** -24


def _operands(shape, n_classes, seed=0):
    gen = torch.Generator().manual_seed(7000 + seed)
    return torch.randn(shape, generator=gen), torch.randn((n_classes, shape[3]), generator=gen)


def _fp64(feat, w, cols, per_image, relu):
    """(reference, bound) [B, K, N] in fp64: (C + 8) 2^-24 sum_c |w| |feat|, the worst case of any fp32 summation order"""
    B, h, wd, C = feat.shape
    f, w64 = feat.double().reshape(B, h * wd, C), w.double()
    if per_image:
        ref = torch.einsum("bc,bpc->bp", w64[cols], f)[:, None]
        mag = torch.einsum("bc,bpc->bp", w64[cols].abs(), f.abs())[:, None]
    else:
        ref = torch.einsum("kc,bpc->bkp", w64[cols], f)
        mag = torch.einsum("kc,bpc->bkp", w64[cols].abs(), f.abs())
    return (ref.clamp_min(0.0) if relu else ref), (C + 8) * U * mag


def _check(feat, w, fd, wd, cols, per_image, relu, what):
    """one call into the middle of a larger sentinel-filled tensor against fp64; returns the device result [B, K, h, w]"""
    from scouter_amd import kernels as K
    B, h, wdt, C = feat.shape
    Kc = 1 if per_image else len(cols)
    ref, bound = _fp64(feat, w, cols, per_image, relu)
    big = torch.full((B + 2, Kc, h, wdt), SENTINEL, device="cuda")
    out = K.cam_fc(fd, wd, torch.tensor(cols, dtype=torch.int32).cuda(), big[1:B + 1], per_image=per_image, relu=relu)
    torch.cuda.synchronize()
    assert out.data_ptr() == big[1].data_ptr() and tuple(out.shape) == (B, Kc, h, wdt)
    assert bool((big[0] == SENTINEL).all()) and bool((big[B + 1] == SENTINEL).all())       # the neighbours are untouched
    got = out.reshape(B, Kc, h * wdt).cpu().double()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    print("cam_fc", tuple(feat.shape), what, "relu", relu, "max err %.3e, max err / bound %.3f"
          % (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.min()))
    if relu:
        assert float(got.min()) >= 0.0
    return out.clone()


# ------------------------------------------------------------------------------------------------------ 1: against fp64
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_cam_fc_kernel_against_fp64(shape):
    B = shape[0]
    for i, n in enumerate(N_CLASSES):
        feat, w = _operands(shape, n, seed=i)
        fd, wd = feat.cuda(), w.cuda()
        own = [(3 * b + n - 1) % n for b in range(B)]
        for relu in (False, True):
            for cols in ([0], [n - 1, 0], list(range(n))):
                _check(feat, w, fd, wd, cols, False, relu, "n_classes %d columns %s" % (n, cols if len(cols) < 3 else "all"))
            _check(feat, w, fd, wd, own, True, relu, "n_classes %d per-image %s" % (n, own))


# ------------------------------------------------------------------------------------------------------ 2: bit identities
@pytest.mark.parametrize("C", [65, 2048, 4100], ids=lambda c: "C%d" % c)
def test_cam_fc_bit_identities(C):
    """two calls; a per-image call and the matching columns of an all-classes call; [3, 1] column 1 and [1] column 0; an image at
    batch position 0 and 2 -- with one 2048-channel piece, three of them, and the scalar route"""
    from scouter_amd import kernels as K
    feat, w = _operands((3, 3, 5, C), 10, seed=C)
    feat[2] = feat[0]
    fd, wd = feat.cuda(), w.cuda()

    def run(cols, per_image=False, f=fd):
        B = f.shape[0]
        out = torch.full((B, 1 if per_image else len(cols), 3, 5), SENTINEL, device="cuda")
        return K.cam_fc(f, wd, torch.tensor(cols, dtype=torch.int32).cuda(), out, per_image=per_image)

    every = run(list(range(10)))
    assert torch.equal(every, run(list(range(10))))
    own = [7, 0, 4]
    per = run(own, per_image=True)
    for b, c in enumerate(own):
        assert torch.equal(per[b, 0], every[b, c]), (b, c)
    assert torch.equal(run([3, 1])[:, 1], run([1])[:, 0]) and torch.equal(run([3, 1])[:, 0], every[:, 3])
    assert torch.equal(every[0], every[2])                                   # the same image at batch position 0 and 2
    assert torch.equal(run(list(range(10)), f=fd[2:3].clone())[0], every[2])           # and alone (a copy: 16-byte aligned)
    assert not torch.equal(every[0], every[1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ 3: refusals
@pytest.mark.parametrize("bad", ["null", "misaligned", "c0", "per_image_k2"])
def test_cam_fc_kernel_refuses_bad_arguments(bad):
    """the library's error naming cam_fc, nothing launched, and a valid call afterwards is right"""
    from scouter_amd import _native
    from scouter_amd import kernels as K
    f, w = torch.ones((2, 3, 3, 8), device="cuda"), torch.ones((4, 8), device="cuda")
    cols = torch.tensor([1, 2], dtype=torch.int32).cuda()
    out = torch.full((2, 2, 3, 3), SENTINEL, device="cuda")
    message = {"null": "null pointer", "misaligned": "misaligned pointer", "c0": "C 0", "per_image_k2": "K 2 must be 1"}[bad]
    with pytest.raises(RuntimeError, match="cam_fc.*" + message):
        if bad == "null":
            _native.check(_native.lib().scouter_cam_fc_f32(f.data_ptr(), None, cols.data_ptr(), out.data_ptr(), 2, 9, 8, 4, 2, 0, 0,
                                                           None), "cam_fc")
        elif bad == "misaligned":
            big = torch.ones(2 * 9 * 8 + 4, device="cuda")
            K.cam_fc(big[1:1 + 144].view(2, 3, 3, 8), w, cols, out)
        elif bad == "c0":                                                    # (valid pointers: the count check itself answers)
            _native.check(_native.lib().scouter_cam_fc_f32(f.data_ptr(), w.data_ptr(), cols.data_ptr(), out.data_ptr(), 2, 9, 0, 4,
                                                           2, 0, 0, None), "cam_fc")
        else:
            _native.check(_native.lib().scouter_cam_fc_f32(f.data_ptr(), w.data_ptr(), cols.data_ptr(), out.data_ptr(), 2, 9, 8, 4,
                                                           2, 1, 0, None), "cam_fc")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    feat, wt = _operands((3, 2, 3, 65), 10, seed=1)
    _check(feat, wt, feat.cuda(), wt.cuda(), [9, 0], False, False, "after a refusal")


def test_cam_fc_wrapper_checks_shapes():
    from scouter_amd import kernels as K
    f, w = torch.ones((2, 3, 3, 8), device="cuda"), torch.ones((4, 8), device="cuda")
    cols = torch.tensor([1, 2], dtype=torch.int32).cuda()
    for args in ((f, w[:, :4].contiguous(), cols, torch.empty((2, 2, 3, 3), device="cuda")),
                 (f, w, cols, torch.empty((2, 3, 3, 3), device="cuda")),
                 (f, w, cols.long(), torch.empty((2, 2, 3, 3), device="cuda")),
                 (f.cpu(), w, cols, torch.empty((2, 2, 3, 3), device="cuda"))):
        with pytest.raises(RuntimeError):
            K.cam_fc(*args)
    with pytest.raises(RuntimeError):                                        # per-image columns are one an image
        K.cam_fc(f, w, torch.zeros(3, dtype=torch.int32).cuda(), torch.empty((2, 1, 3, 3), device="cuda"), per_image=True)


# ------------------------------------------------------------------------------------------------------ 4: the whole model
def test_fccam_on_the_fc_baseline():
    """fc_resnet18_mnist_64 (batch 4, 2 x 2 x 512 features), unfolded in training mode and folded in eval mode.

    Completeness.  z[b, k] = mean_p cam[b, k, p] + bias[k] is the model's logit, so log_softmax(z) is its output.  Two fp32 chains
    lie between the two sides: the model pools the features (N - 1 additions and a scaling) and contracts the pooled vector with
    the weights (C products and additions, the bias), at most (N + C + 4) roundings of terms |w| |feat| / N; fccam contracts first,
    within (C + 8) 2^-24 sum_c |w| |feat| per position, and the mean, the bias and the log-softmax of this side are taken in
    fp64.  With A[b, k] = mean_p sum_c |w[k, c]| |feat[b, p, c]| + |bias[k]| the logits differ by at most
    d = (2 C + N + 12) 2^-24 max_k A[b, k]; a log-softmax moves by at most twice the largest move of a logit; and the model's own
    fp32 log-softmax over n classes adds at most (n + 16) 2^-24 max(1, max |log_prob|).  bound = 2 d + that term."""
    from scouter_amd.tools.attribution import fccam
    m, P, images, cfg, arch = build("fc_resnet18_mnist_64")
    x = images.cuda()
    w64, b64 = m.backbone.fc.weight.detach().cpu().double(), m.backbone.fc.bias.detach().cpu().double()
    n = w64.shape[0]
    m.train()
    before = bn_buffers(m)
    for fold in (False, True):
        if fold:
            m.eval()
            m.set_inference_fold(True)
        fp = m.feature_pass(x)
        feat = fp.features
        B, h, wd, C = feat.shape
        N = h * wd
        f64 = feat.cpu().double().reshape(B, N, C)
        cam = fccam(m, x)
        torch.cuda.synchronize()
        assert m.training is (not fold)                                      # the caller's mode is back
        assert tuple(cam.shape) == (B, n, h, wd) and cam.dtype == torch.float32 and cam.is_cuda
        got = cam.reshape(B, n, N).cpu().double()
        ref = torch.einsum("kc,bpc->bkp", w64, f64)
        mag = torch.einsum("kc,bpc->bkp", w64.abs(), f64.abs())
        err = (got - ref).abs()
        print("fccam fold %s: max err %.3e, max err / bound %.3f" % (fold, float(err.max()), float((err / ((C + 8) * U * mag)).max())))
        assert float(ref.abs().max()) > 0 and bool((err <= (C + 8) * U * mag).all())
        # completeness against the model's own output
        logp = fp.log_probs.cpu().double()
        mine = torch.log_softmax(got.mean(dim=2) + b64, dim=1)
        A = mag.mean(dim=2) + b64.abs()
        bound = 2.0 * (2 * C + N + 12) * U * A.max(dim=1, keepdim=True).values + \
            (n + 16) * U * logp.abs().max(dim=1, keepdim=True).values.clamp_min(1.0)
        gap = (mine - logp).abs()
        print("fccam fold %s completeness: max |log_softmax(mean cam + bias) - log_probs| %.3e, max gap / bound %.2e"
              % (fold, float(gap.max()), float((gap / bound).max())))
        assert bool((gap <= bound).all()), (float(gap.max()), float(bound.min()))
        # a list and a tensor of classes: the columns of the call above, bit for bit; relu clamps
        two = fccam(m, x, classes=[3, 1])
        assert torch.equal(two[:, 0], cam[:, 3]) and torch.equal(two[:, 1], cam[:, 1])
        cls = (torch.arange(B) * 3 + 1) % n
        own = fccam(m, x, classes=cls)
        assert tuple(own.shape) == (B, 1, h, wd) and all(torch.equal(own[b, 0], cam[b, int(cls[b])]) for b in range(B))
        assert torch.equal(fccam(m, x, classes=[3], relu=True)[:, 0], cam[:, 3].clamp_min(0.0))
        for bad in ([n], [-1], torch.tensor([0] * (B - 1) + [n])):
            with pytest.raises(IndexError):
                fccam(m, x, classes=bad)
    after = bn_buffers(m)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in m.parameters())                       # no backward at all


def test_fccam_maps_and_the_slot_model():
    from scouter_amd import kernels as K
    from scouter_amd.tools.attribution import fccam, fccam_maps
    m, P, images, cfg, arch = build("fc_resnet18_mnist_64")
    x = images.cuda()
    maps = fccam_maps(m, x, min_level=0.2)
    assert maps.dtype == torch.uint8 and maps.is_cuda and tuple(maps.shape) == (4, 10, 64, 64) and bool(maps.any())
    assert torch.equal(maps, K.cam_maps(fccam(m, x), 64, 64, 0.2))
    small = fccam_maps(m, x, classes=[2, 5], size=(20, 30))
    assert tuple(small.shape) == (4, 2, 20, 30) and torch.equal(small, K.cam_maps(fccam(m, x, classes=[2, 5]), 20, 30, 0.0))
    slot, _, simages, _, _ = build("resnet18_mnist_64")
    for call in (fccam, fccam_maps):
        with pytest.raises(RuntimeError, match="use_slot false.*gradcam"):
            call(slot, simages.cuda())
