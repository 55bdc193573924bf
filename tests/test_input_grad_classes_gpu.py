"""input_gradients with a LongTensor [B] of classes (-m gpu): every image its own class, K = 1, one backward -- the form the
table tool's `grad` row calls.  Image b's gradient must be the gradient input_gradients gives the same image for the list
[classes[b]], and the refusals are those of the other methods: a class outside the outputs is an IndexError, a tensor that is
not a LongTensor [B] a ValueError.  (Before this form existed a tensor was iterated like a list; `.tolist()` still gives that.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gradcam_gpu import build                                          # noqa: E402


@pytest.mark.parametrize("case", ["resnet18_mnist_64", "fc_resnet18_mnist_64"])
def test_a_tensor_of_classes_gives_each_image_its_own_class(case):
    """Both sides are the same eval-mode forward and backward at the same batch shape, and no kernel on the way to the input
    gradient sums over images (BatchNorm uses its running statistics), so image b's values see the same operations in the same
    order whatever the seeds of the other rows are: the bound is 2^-20 max |gradient of the image| -- 16 units in the last place
    at the map's scale, room for a kernel that skips a zero row -- and bit equality is printed.  The gradient of another class
    differs by orders of magnitude more, so a seed at a wrong index cannot pass."""
    from scouter_amd.tools.attribution import input_gradients
    m, P, images, cfg, arch = build(case)
    x = images.cuda()
    B, n = x.shape[0], 10
    m.train()
    cls = (torch.arange(B) * 3 + 1) % n                                      # 1, 4, 7, 0: four different classes
    own = input_gradients(m, x, classes=cls)
    torch.cuda.synchronize()
    assert m.training
    assert tuple(own.shape) == (B, 1) + tuple(x.shape[1:]) and own.dtype == torch.float32 and own.is_cuda
    assert torch.equal(own, input_gradients(m, x, classes=cls.cuda()))       # two calls, the tensor on either device
    for b in range(B):
        c = int(cls[b])
        ref = input_gradients(m, x, classes=[c, (c + 1) % n])
        scale = float(ref[b, 0].abs().max())
        err = float((own[b, 0] - ref[b, 0]).abs().max())
        other = float((own[b, 0] - ref[b, 1]).abs().max())
        print("%s image %d class %d: max |tensor form - list form| %.3e (bit-equal %s), max |.| %.3e, against class %d %.3e"
              % (case, b, c, err, torch.equal(own[b, 0], ref[b, 0]), scale, (c + 1) % n, other))
        assert scale > 0 and err <= 2.0 ** -20 * scale, (b, err, scale)
        assert other > 2.0 ** -10 * scale, (b, other, scale)
    # what a tensor did before, a list still does: K columns for every image
    assert tuple(input_gradients(m, x, classes=cls.tolist()).shape) == (B, B) + tuple(x.shape[1:])


def test_a_tensor_of_classes_is_checked():
    from scouter_amd.tools.attribution import input_gradients
    m, P, images, cfg, arch = build("resnet18_mnist_64")
    x = images.cuda()
    B = x.shape[0]
    for bad in (torch.tensor([0] * (B - 1) + [10]), torch.tensor([-1] + [0] * (B - 1))):
        with pytest.raises(IndexError):
            input_gradients(m, x, classes=bad)
    for bad in (torch.tensor([0, 3]), torch.zeros(B + 1, dtype=torch.int64), torch.zeros(B, dtype=torch.int32),
                torch.zeros((B, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match="LongTensor"):
            input_gradients(m, x, classes=bad)
    after = input_gradients(m, x, classes=torch.zeros(B, dtype=torch.int64))    # a right call after the refusals
    assert bool(torch.isfinite(after).all()) and float(after.abs().max()) > 0
