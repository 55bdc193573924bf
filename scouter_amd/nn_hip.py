"""Layer primitives with EXPLICIT forward / backward over NHWC device tensors (the host side of the HIP path).

The reference leaves sequencing of the backward pass to torch.autograd over ~1400 tiny ATen kernels
(SURVEY.md section 2.2).  Here every layer has `fwd(x, save, ...) -> (y, ctx)` and `bwd(dy, ctx, ...) -> dx`
that launch the hand-written kernels directly; parameter gradients are written straight into one flat fp32
arena (GradArena) whose slices are exposed as `param.grad`, so the data-parallel all-reduce and the fused AdamW
see a single contiguous buffer.  Modules keep the reference's parameter / buffer names so state_dicts are
interchangeable; conv weights have the reference's logical (Cout, Cin/g, kh, kw) shape
over an HWIO physical layout."""
import math
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import kernels as K


class Act(nn.Module):
    """Placeholder for the reference's ReLU modules (keeps nn.Sequential indices, e.g. backbone.conv1.{0,1,3,4,6})."""

    def forward(self, x):   # pragma: no cover - activation is fused into the neighbouring kernel
        raise RuntimeError("activation is fused; call the parent module")


# bf16 storage of the gradients that only bf16-input convolution kernels read (Conv2d.grad_storage); SCOUTER_BF16_GRADS=0: fp32
GRAD_STORAGE_BF16 = os.environ.get("SCOUTER_BF16_GRADS", "1") != "0"

# The kernels of one convolution layer (Conv2d.route): a function of its shape and its (x3, precision, planes).
# fwd / dgrad: the kernel families of that pass in order of preference -- a call runs on the first one it fits
# (Conv2d._fwd_fits / _dgrad_fits), on the igemm kernels (kernels.conv2d_fwd / conv2d_dgrad) if it fits none; wgrad: the
# family of the weight gradient.  Families: "planes" (bf16x3 operand planes, csrc/conv_planes.hip), "xpw" (the persistent
# bf16x3 pointwise forward, csrc/conv_pw_persist_x3.h; SCOUTER_X3 bit 5), "xhalo" (the persistent resident-rows kernel,
# csrc/conv_xhalo.hip; bits 7 / 6), "x3" (the register-split bf16x3 GEMM, csrc/conv_x3.hip; bits 0 / 1 / 3 / 4) and
# "x3_fused" (the same GEMM with the fused BatchNorm-backward epilogue; bit 2).  split_fwd / split_dgrad: the layer takes
# forward / input-gradient weight planes from the model's one-launch split (SlotModel._split_items).  planes_in /
# planes_dy: number of operand planes the layer wants its input / output gradient in (0: a plain tensor).
ConvRoute = namedtuple("ConvRoute", "fwd dgrad wgrad split_fwd split_dgrad planes_in planes_dy")
# What Conv2d.fwd saves for bwd: the input (its shape only when the producer wrote planes only), the input-gradient weight
# planes, the operand planes of the input.
ConvCtx = namedtuple("ConvCtx", "x wd xp")
# What StemConv2d.fwd saves: the image's patch rows, and the image's shape (the input gradient's; the patch rows no longer
# have it).
StemCtx = namedtuple("StemCtx", "x shape")


# The INFERENCE variant (SlotModel.set_inference_fold: every BatchNorm folded into the convolution in front of it, so each
# layer is conv + bias [+ residual addend] [+ ReLU] in one kernel): fwd is the one forward family of the layer -- one with
# the bias + addend + ReLU epilogue.  The persistent pointwise forward ("xpw") has the plain epilogue only and the
# resident-rows kernel ("xhalo") takes no bias / addend, so in fp32 mode a layer whose training forward runs on a bf16x3
# family keeps fp32-grade bf16x3 arithmetic on the register-split GEMM ("x3", which takes all three); the plane layers (the
# 3x3 radix convolutions), whose producer is now a convolution epilogue that writes no planes, run on it as well, fed the
# fp32 tensor directly.  The other candidate, a K.planes_split pass in front of the plane kernel (FOLD_RADIX = "planes", kept
# for tools_dev/eval_fold_bench.py --radix), measured at BASELINE config 2's shapes (batch 70, 224^2; conv + bias + ReLU, us,
# x3 / split + planes): 64 -> 128 at 56^2 118 / 133, 128 -> 256 at 56^2 359 / 407 and at 28^2 106 / 105, 256 -> 512 at 28^2
# 387 / 360 and at 14^2 108 / 90, 512 -> 1024 at 14^2 384 / 345 and at 7^2 105 / 102 -- the plane kernel wins from 256
# channels on, the split pass costs more than that on the large maps: the whole folded forward 4.80 ms on x3, 4.88 ms on
# split + planes (3 windows each, spread 0.1 %).  So: x3.  Everything else -- strided
# layers, resnet18, the stem's 32 -> 32 convolution, the attention FCs, and every layer under precision "bf16" -- runs on
# "igemm" with the folded weights.  split: the layer wants three-way forward planes of its FOLDED weight.
InferRoute = namedtuple("InferRoute", "fwd split")
# What the model's fold leaves on a layer (Conv2d._fold): folded HWIO weight and bias (views of the model's flat buffer),
# the three-way forward planes / the bf16 transposed weight of the folded weight where the route / precision wants them.
FoldedConv = namedtuple("FoldedConv", "w b wf wt")
FOLD_RADIX = "x3"


def _infer_route(c):
    k = c.kernel_size
    if c.precision != "fp32" or isinstance(c, StemConv2d):
        return InferRoute("igemm", False)
    abi = K.x3_fwd_abi_ok(c.in_channels, c.out_channels, k, c.stride, c.padding, c.groups)
    r = c.route()
    if c.planes:
        if r.planes_in and FOLD_RADIX == "planes":
            return InferRoute("planes", True)
        return InferRoute("x3", True) if r.planes_in and abi else InferRoute("igemm", False)
    if abi and ("x3" in r.fwd or "xpw" in r.fwd):
        return InferRoute("x3", True)
    return InferRoute("igemm", False)


def _conv_route(c):
    k, g = c.kernel_size, c.groups
    cg, ng = c.in_channels // g, c.out_channels // g
    shape = (c.in_channels, c.out_channels, k, k, c.stride, c.padding, g, c.bias is not None)
    n = c._nplanes()
    planes_in = n if n and c.stride == 1 and cg % 32 == 0 and ng % 64 == 0 else 0
    planes_dy = n if n and c.stride == 1 and ng % 32 == 0 and cg % 64 == 0 else 0
    bits = c.x3 if c.precision == "fp32" else 0              # (the register-split kernels: fp32 precision only)
    halo_fwd, halo_dgrad = K.x3_halo_eligible(*shape)
    # (the resident-rows input gradient also serves plane layers: their gradient planes need 64 input channels per group)
    dgrad = ("xhalo",) if bits & 64 and halo_dgrad else ()
    if c.planes:
        wgrad = "planes" if planes_in and planes_dy and cg % 64 == 0 and ng % 64 == 0 and 2 * c.padding == k - 1 else "igemm"
        return ConvRoute(("planes",) if planes_in else (), ("planes",) if planes_dy else dgrad, wgrad, True,
                         bool(planes_dy or dgrad), planes_in, planes_dy)
    x3 = K.x3_eligible(*shape)
    # (the persistent forward serves 64 / 128 input channels always, 256 where the register-split GEMM does not: it wins from
    #  512 output channels on, tools_dev/xpw_fwd_bench.py)
    xpw = bits & 32 and K.xpw_fwd_eligible(*shape) and (c.in_channels <= 128 or not x3)
    fwd = ((("xpw",) if xpw else ()) + (("xhalo",) if bits & 128 and halo_fwd else ()) +
           (("x3",) if (bits & 1 and x3) or (bits & 16 and K.x3_conv_eligible(*shape)) else ()))
    dgrad += (("x3",) if bits & 2 and x3 else ()) + (("x3_fused",) if bits & 4 and x3 else ())
    wgrad = "x3" if bits & 8 and x3 and K.x3_wgrad_ok(c.in_channels, c.out_channels) else "igemm"
    # (the persistent forward splits its weight tile itself)
    return ConvRoute(fwd, dgrad, wgrad, fwd[:1] in (("xhalo",), ("x3",)), bool(dgrad), 0, 0)


class Conv2d(nn.Module):
    """nn.Conv2d(bias optional) -> scouter_conv2d_{fwd,dgrad,wgrad}_f32.  Per-group channels must be multiples of 32."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, groups=1, bias=False):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.groups = stride, padding, groups
        k = kernel_size
        w = torch.empty(k, k, in_channels // groups, out_channels)
        self.weight = nn.Parameter(w.permute(3, 2, 0, 1))          # logical OIHW, physical HWIO
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self._dw = self._db = None                                  # arena slices, set by GradArena
        self.precision = "fp32"                                     # per layer; SlotModel.set_precision (no global)
        self.use_side_stream = K.SIDE_STREAM_DEFAULT                # weight gradient on the side stream
        self.planes = 0                                             # 3: bf16x3 plane kernels (SlotModel.set_planes)
        self._wsplit = None                                         # (wf, wd) of this step, from the model's one-launch split
        self.x3 = 0                                                 # bits of kernels.X3_DEFAULT (SlotModel.set_x3): register-split bf16x3 GEMM
        self._routes = {}                                           # (x3, precision, planes) -> ConvRoute
        self._iroutes = {}                                          # (x3, precision, planes, FOLD_RADIX) -> InferRoute
        self._fold = None                                           # FoldedConv of the model's last fold (SlotModel._refold)
        self._capture = None                                        # test instrumentation, see BatchNorm2d
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")   # timm resnet.py:447-448
        if bias:
            bound = 1.0 / math.sqrt(in_channels // groups * k * k)
            nn.init.uniform_(self.bias, -bound, bound)

    def route(self):
        """This layer's ConvRoute for its current (x3, precision, planes)."""
        key = (self.x3, self.precision, self.planes)
        r = self._routes.get(key)
        if r is None:
            r = self._routes[key] = _conv_route(self)
        return r

    def infer_route(self):
        """This layer's InferRoute (the folded inference forward) for its current (x3, precision, planes)."""
        key = (self.x3, self.precision, self.planes, FOLD_RADIX)
        r = self._iroutes.get(key)
        if r is None:
            r = self._iroutes[key] = _infer_route(self)
        return r

    def fwd_folded(self, x, relu=False, addend=None):
        """[relu](conv'(x) + b' [+ addend]) with the BatchNorm behind this layer folded into (w', b') by the model's fold:
        one kernel, fp32 tensors in and out, nothing saved."""
        f = self._fold
        if f is None:
            raise RuntimeError("Conv2d.fwd_folded: the model has not folded this layer (SlotModel.set_inference_fold)")
        fam = self.infer_route().fwd
        k = self.kernel_size
        if fam != "igemm" and not K.x3_fwd_fits(*x.shape[:3], self.in_channels, self.out_channels, k, self.groups):
            fam = "igemm"                 # (past the 32-bit offset guards of the bf16x3 kernels, like Conv2d._fwd_fits in training)
        if fam == "x3":
            return K.conv2d_fwd_x3(x, f.wf, addend, relu, kh=k, pad=self.padding, groups=self.groups, bias=f.b)
        if fam == "planes":
            return K.conv2d_fwd_planes(K.planes_split(x, 3), f.wf, k, k, self.stride, self.padding, self.groups, f.b, addend,
                                       relu)
        return K.conv2d_fwd(x, f.w, f.b, addend, self.stride, self.padding, self.groups, relu, precision=self.precision,
                            wt=f.wt)

    def dgrad_folded(self, dy, xshape, addend=None, wd=None):
        """conv'^T(dy) [+ addend]: the input gradient of fwd_folded's convolution (SlotModel.image_pass), on the FOLDED weight,
        fp32 in and out.  wd: the input-gradient planes of the folded weight from the model's one-launch split -- with them the
        call runs on the bf16x3 family the layer's route offers for a plain fp32 gradient ("xhalo" / "x3") where that admits the
        shape; without them, and for every other layer, on the igemm kernels."""
        f = self._fold
        if f is None:
            raise RuntimeError("Conv2d.dgrad_folded: the model has not folded this layer (SlotModel.image_pass)")
        if self.precision != "fp32":
            raise NotImplementedError("Conv2d.dgrad_folded: precision %r has no folded input gradient" % (self.precision,))
        k = self.kernel_size
        xshape = tuple(xshape)
        fam = next((fm for fm in self.route().dgrad
                    if fm in ("xhalo", "x3") and self._dgrad_fits(fm, dy, None, wd, None, None, xshape)), "igemm")
        if fam != "igemm":
            return K.conv2d_dgrad_x3(dy, wd, xshape, addend, tile=7 if fam == "xhalo" else None, kh=k, pad=self.padding,
                                     groups=self.groups)
        return K.conv2d_dgrad(dy, f.w, xshape, addend, self.stride, self.padding, self.groups)

    def x3_mode(self):
        """True if a pass of this layer runs on a register-split kernel (SlotModel._x3_convs)."""
        r = self.route()
        return not self.planes and any(f in ("xhalo", "x3", "x3_fused") for f in r.fwd + r.dgrad + (r.wgrad,))

    def _x3_weights(self, want_fwd, want_dgrad):
        ws, self._wsplit = self._wsplit, None
        if ws is not None and (ws[0] is not None or not want_fwd) and (ws[1] is not None or not want_dgrad):
            return ws
        return K.planes_split_weight(K.hwio(self.weight), self.groups, 3, fwd=want_fwd, dgrad=want_dgrad)

    def _halo_fits(self, dgrad, shape):
        """The resident-rows kernel takes this pass on a B x H x W map (the library's width and byte guards, K.x3_halo_ok);
        past them the layer keeps the fp32 MFMA kernels it had before tile 7."""
        return K.x3_halo_ok(dgrad, *shape[:3], self.in_channels, self.out_channels, self.groups)

    def _fwd_fits(self, fam, x, relu, addend, out_dtype):
        """This forward call fits family `fam` of the route: fp32 tensors in and out; the persistent pointwise kernel has the
        plain epilogue only, the resident-rows kernel no addend."""
        if x.dtype != K.F32 or out_dtype not in (None, K.F32):
            return False
        if fam == "xpw":
            return addend is None and not relu
        if fam == "xhalo":
            return addend is None and self._halo_fits(False, x.shape)
        return fam == "x3"

    def _dgrad_fits(self, fam, dy, dyp, wd, post, dx_dtype, xshape):
        """This input-gradient call fits family `fam` of the route: the weight planes were saved; the plane kernel reads the
        gradient's planes, the register-split kernels an fp32 gradient -- with the fused BatchNorm-backward epilogue only
        where the GEMM is deep enough (K.X3_FUSED_MIN_K)."""
        if wd is None:
            return False
        if fam == "planes":
            return dyp is not None
        if dy is None or dy.dtype != K.F32:
            return False
        if fam == "xhalo":
            return dx_dtype in (None, K.F32) and self._halo_fits(True, xshape)
        fused = post is not None and K._fuse_wanted(post, self.kernel_size) and post.x_io() == 0
        return dyp is None and (fused and self.out_channels >= K.X3_FUSED_MIN_K if fam == "x3_fused" else not fused)

    # ---- bf16x3 operand planes (csrc/conv_planes.hip): the producer of this layer's input hands over a K.PlaneTensor
    def _nplanes(self):
        """3 exact bf16 planes per operand in fp32 mode (fp32-grade products), 1 (the RNE-rounded value: what the
        bf16-input kernels compute, without their in-flight conversion and with half the operand bytes) in bf16 mode."""
        return 0 if not self.planes else (self.planes if self.precision == "fp32" else 1)

    def planes_only(self, H, W, B=None):
        """True if forward, input gradient AND weight gradient of this layer all run on planes for an H x W map: its
        producers then need not write the fp32 copy of the tensor at all.  In bf16 mode (ONE plane = the bf16-stored
        tensor) that also holds when the gradients run on the bf16-input igemm kernels, which read that plane as a
        bf16-stored activation (32-channel groups: the first grouped layer; needs the batch size for their pixel rule)."""
        r = self.route()
        if not (self.bias is None and r.planes_in):
            return False
        # (the plane kernel's branch-free pixel walk needs maps that are not tiny: 32 // W + 1 < H)
        if r.wgrad == "planes" and 32 // W + 1 < H:
            return True
        return bool(B is not None and self._nplanes() == 1 and self._bf16_igemm(B, H, W))

    def _bf16_igemm(self, B, H, W):
        """The bf16-input igemm kernels run this layer for a B x H x W map (kernels.conv2d_fwd / conv2d_dgrad / conv2d_wgrad
        rules): they read bf16-stored operands and round fp32 ones to the same values."""
        cg, ng = self.in_channels // self.groups, self.out_channels // self.groups
        k = self.kernel_size
        return bool(GRAD_STORAGE_BF16 and self.precision == "bf16" and self.stride == 1 and 2 * self.padding == k - 1 and
                    B * H * W >= K.BF16_MIN_PIXELS and cg % 32 == 0 and ng % 32 == 0 and (k == 1 or 64 // W + 1 < H))

    def dy_plane_only(self, B, H, W):
        """bf16 mode, a plane layer whose input gradient does NOT run on planes (32-channel groups): its output gradient
        can still be handed over as ONE bf16 plane only -- the igemm kernels read it as a bf16-stored tensor."""
        return bool(self.planes and self._nplanes() == 1 and not self.route().planes_dy and self.bias is None and
                    self._bf16_igemm(B, H, W))

    def grad_storage(self, B, H, W):
        """Storage type for this layer's OUTPUT gradient (B x H x W output pixels): bf16 when both of its readers -- the
        input-gradient and the weight-gradient kernel -- are the bf16-input ones, which round an fp32 gradient to exactly
        the stored values (so this storage changes no result); None (fp32) otherwise."""
        return K.BF16 if not self.planes and self.bias is None and self._bf16_igemm(B, H, W) else None

    def act_storage(self, B, H, W):
        """Storage type for this layer's INPUT activation (B x H x W pixels) when nothing else reads it: bf16 when the
        forward and the weight-gradient kernel are the bf16-input ones (which round an fp32 input to exactly the stored
        values: no result changes); None (fp32) otherwise."""
        return K.BF16 if not self.planes and self._bf16_igemm(B, H, W) else None

    def fwd(self, x, save, relu=False, addend=None, bn_stats=False, out_dtype=None):
        """bn_stats=True (a train-mode BatchNorm follows): returns ((y, stats), ctx) -- see kernels.conv2d_fwd.
        out_dtype=torch.bfloat16: the output is STORED as bf16 (activation storage of the bf16 mode, kernels.conv2d_fwd)."""
        r = self.route()
        k = self.kernel_size
        want_wd = save and r.split_dgrad
        if isinstance(x, K.PlaneTensor):
            ws, self._wsplit = self._wsplit, None
            if ws is not None and ws[0] is not None and ws[0].shape[0] == x.planes.shape[0] and (ws[1] is not None or not want_wd):
                wf, wd = ws[0], (ws[1] if want_wd else None)        # split by SlotModel for the whole model in one launch
            else:
                wf, wd = K.planes_split_weight(K.hwio(self.weight), self.groups, x.planes.shape[0], fwd=True, dgrad=want_wd)
            y = K.conv2d_fwd_planes(x.planes, wf, k, k, self.stride, self.padding, self.groups, self.bias, addend, relu,
                                    bn_stats, out_dtype=out_dtype or K.F32)
            ctx = ConvCtx(x.f32 if x.f32 is not None else tuple(x.shape), wd,
                          x.planes if r.wgrad == "planes" or x.f32 is None else None)
        else:
            fam = next((f for f in r.fwd if self._fwd_fits(f, x, relu, addend, out_dtype)), "igemm")
            split = fam in ("xhalo", "x3")
            want_wd = want_wd and not self.planes           # (a plane layer fed a plain tensor: the igemm kernels)
            wf, wd = self._x3_weights(split, want_wd) if split or want_wd else (None, None)
            if split:
                y = K.conv2d_fwd_x3(x, wf, addend, relu, bn_stats, tile=7 if fam == "xhalo" else None, kh=k, pad=self.padding,
                                    groups=self.groups)
            else:
                y = K.conv2d_fwd(x, K.hwio(self.weight), self.bias, addend, self.stride, self.padding, self.groups, relu,
                                 bn_stats, precision=self.precision, out_dtype=out_dtype or K.F32,
                                 tile=5 if fam == "xpw" else None)
            ctx = ConvCtx(x, wd, None)
        if self._capture is not None and relu:
            self._capture[0][self._capture[1]] = y
        return y, (ctx if save else None)

    def bwd(self, dy, ctx, need_dx=True, addend=None, post=None, dx_dtype=None):
        """post (K.BnBwdFuse): the input gradient is the gradient of a BatchNorm(+ReLU) output -- its producer finishes
        that BatchNorm's backward reductions in the epilogue (only when dx is computed at all).  dx_dtype=torch.bfloat16:
        that masked gradient is stored as bf16 when the bf16-input kernel fuses (kernels.conv2d_dgrad; check dx.dtype)."""
        r = self.route()
        k = self.kernel_size
        x, wd, xp = ctx
        dyp = None
        if isinstance(dy, K.PlaneTensor):
            dy, dyp = dy.f32, dy.planes
        xshape = x if isinstance(x, tuple) else tuple(x.shape)       # (a shape only: the producer wrote planes only)
        xt = None if isinstance(x, tuple) else x
        if xt is None and xp is not None and xp.shape[0] == 1 and r.wgrad != "planes":
            xt = xp[0]                    # (bf16 mode: the one plane IS the bf16-stored activation of the igemm kernels)
        if dy is None and dyp is not None and dyp.shape[0] == 1 and wd is None:
            dy, dyp = dyp[0], None        # (likewise the output gradient, Conv2d.dy_plane_only)
        dev = dy.device if dy is not None else dyp.device
        fam = next((f for f in r.dgrad if self._dgrad_fits(f, dy, dyp, wd, post, dx_dtype, xshape)), "igemm") if need_dx else None
        dx = None
        if fam == "planes":               # (ahead of the weight gradient, like every input gradient that feeds the next layer)
            dx = K.conv2d_dgrad_planes(dyp, wd, xshape, k, k, self.stride, self.padding, self.groups, addend, post=post)
        if self._dw is not None or self._db is not None:
            # weight / bias gradients: off the critical path
            with K.side_stream(dev, xt, dy, xp, dyp, enabled=self.use_side_stream):
                # (the plane kernel's branch-free pixel walk needs maps that are not tiny: 32 // W + 1 < H)
                if (self._dw is not None and r.wgrad == "planes" and xp is not None and dyp is not None and
                        32 // xshape[2] + 1 < xshape[1]):
                    K.conv2d_wgrad_planes(xp, dyp, self._dw, self.padding, self.groups)
                elif (self._dw is not None and r.wgrad == "x3" and xt is not None and dy is not None and
                      xt.dtype == K.F32 and dy.dtype == K.F32):
                    K.conv2d_wgrad_x3(xt, dy, self._dw)      # (pointwise layer: register-split bf16x3 GEMM, csrc/conv_x3.hip)
                elif self._dw is not None:
                    if xt is None or dy is None:
                        raise RuntimeError("Conv2d.bwd: the fp32 operands were dropped (planes_only) but the weight "
                                           "gradient cannot run on planes for this shape")
                    K.conv2d_wgrad(xt, dy, self._dw, self.stride, self.padding, self.groups, precision=self.precision)
                if self._db is not None:
                    K.colsum(dy, self._db)
        if fam in (None, "planes"):
            return dx
        if fam != "igemm":
            # resident rows (tile 7), or the pointwise register-split GEMM, plain or with the fused BatchNorm-backward epilogue
            return K.conv2d_dgrad_x3(dy, wd, xshape, addend, post=post, tile=7 if fam == "xhalo" else None, kh=k,
                                     pad=self.padding, groups=self.groups)
        return K.conv2d_dgrad(dy, K.hwio(self.weight), xshape, addend, self.stride, self.padding, self.groups,
                              precision=self.precision, post=post, out_dtype=dx_dtype or K.F32)


class StemConv2d(Conv2d):
    """First convolution of the network (Cin = 1 or 3, NCHW image in): im2col into [M][Kpad] rows (zero padded to a
    multiple of 32) + the generic MFMA GEMM, for the forward and the weight gradient.  The input gradient (bwd(need_dx=True):
    d output / d image, NCHW fp32 -- what attribution maps read) is one direct fp32 kernel, kernels.stem_dgrad, whatever the
    precision."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding):
        nn.Module.__init__(self)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.groups = stride, padding, 1
        k = kernel_size
        self.kdim = k * k * in_channels
        self.kpad = (self.kdim + 31) // 32 * 32
        self.weight = nn.Parameter(torch.empty(k, k, in_channels, out_channels).permute(3, 2, 0, 1))
        self.bias = None
        self._dw = self._db = None
        self.precision = "fp32"
        self.use_side_stream = K.SIDE_STREAM_DEFAULT
        self.planes = 0
        self.x3 = 0
        self._routes = {}
        self._iroutes = {}
        self._fold = None
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")

    def fwd_folded(self, x_nchw, relu=False, addend=None):
        """Conv2d.fwd_folded for the stem: patch rows x the folded weight, which the fold keeps padded to `kpad` rows."""
        f = self._fold
        if f is None:
            raise RuntimeError("StemConv2d.fwd_folded: the model has not folded this layer (SlotModel.set_inference_fold)")
        if x_nchw.dim() != 4 or x_nchw.shape[1] != self.in_channels:
            raise RuntimeError("expected an NCHW image batch with %d channel(s), got shape %s"
                               % (self.in_channels, tuple(x_nchw.shape)))
        col = K.im2col_nchw(x_nchw, self.kernel_size, self.stride, self.padding, self.kpad)
        return K.conv2d_fwd(col, f.w, f.b, addend, 1, 0, 1, relu, precision=self.precision, wt=f.wt)

    def dgrad_folded(self, dy, xshape, addend=None, wd=None):
        """The image gradient (NCHW fp32) of fwd_folded's convolution: kernels.stem_dgrad on the folded weight, whose first
        `kdim` rows are the HWIO weight (the rest is the GEMM's zero padding)."""
        f = self._fold
        if f is None:
            raise RuntimeError("StemConv2d.dgrad_folded: the model has not folded this layer (SlotModel.image_pass)")
        if addend is not None:
            raise RuntimeError("StemConv2d.dgrad_folded: the image gradient takes no addend")
        k = self.kernel_size
        w = f.w.view(self.kpad, self.out_channels)[:self.kdim].view(k, k, self.in_channels, self.out_channels)
        return K.stem_dgrad(dy, w, xshape, k, self.stride, self.padding)

    def fwd(self, x_nchw, save, relu=False, addend=None, bn_stats=False):
        if x_nchw.dim() != 4 or x_nchw.shape[1] != self.in_channels:
            raise RuntimeError("expected an NCHW image batch with %d channel(s), got shape %s"
                               % (self.in_channels, tuple(x_nchw.shape)))
        col = K.im2col_nchw(x_nchw, self.kernel_size, self.stride, self.padding, self.kpad)
        wflat = K.hwio(self.weight).reshape(-1)
        wpad = K.pad_rows(wflat, wflat.numel(), self.kpad * self.out_channels).view(1, 1, self.kpad, self.out_channels)
        y = K.conv2d_fwd(col, wpad, None, addend, 1, 0, 1, relu, bn_stats, precision=self.precision)
        return y, (StemCtx(col, tuple(x_nchw.shape)) if save else None)

    def bwd(self, dy, ctx, need_dx=False, addend=None):
        """need_dx: returns the gradient of the image (NCHW fp32), computed on the compute stream ahead of the weight
        gradient on its side stream, like Conv2d.bwd."""
        dx = None
        if need_dx:
            if addend is not None:
                raise RuntimeError("StemConv2d.bwd: the image gradient takes no addend")
            dx = K.stem_dgrad(dy, K.hwio(self.weight), ctx.shape, self.kernel_size, self.stride, self.padding)
        if self._dw is not None:
            with K.side_stream(dy.device, ctx.x, dy, enabled=self.use_side_stream):
                dwpad = torch.empty((1, 1, self.kpad, self.out_channels), dtype=torch.float32, device=dy.device)
                K.conv2d_wgrad(ctx.x, dy, dwpad, precision=self.precision)
                n = self.kdim * self.out_channels
                K.axpby(dwpad.view(-1)[:n], None, 1.0, 0.0, out=self._dw.reshape(-1))
        return dx


class BatchNorm2d(nn.Module):
    """nn.BatchNorm2d (eps 1e-5, momentum 0.1) with ReLU / residual-add fused into the apply pass."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self._dg = self._db = None
        self._capture = None                 # test instrumentation: (dict, key) -> the ReLU'd output is stored there

    def fwd(self, x, save, relu=False, residual=None, tracked=None, planes=0, residual_bn=None, keep_f32=True,
            out_dtype=None):
        """x may be the (tensor, stats) pair a conv produced with bn_stats=True.  out_dtype=torch.bfloat16: the output is
        stored as bf16 (x / residual may be bf16-stored too: kernels.bn_fwd).  planes = 1 / 3: the output is a
        K.PlaneTensor (fp32 + bf16 operand planes for the plane convolution that consumes it).  residual_bn: `residual`
        is the raw output of the downsample convolution and this the saved block of ITS BatchNorm (stats_only): both
        BatchNorms are applied in this one pass."""
        stats = None
        if isinstance(x, tuple):
            x, stats = x
        if self.training and x.numel() == x.shape[-1]:     # torch.nn.functional.batch_norm's check (batch 1 on a 1x1 map)
            raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                             % (tuple(x.shape),))
        out = K.bn_fwd(x, self.weight, self.bias, self.running_mean, self.running_var, self.training, relu,
                       residual, self.momentum, self.eps, stats if self.training else None,
                       want_mask=bool(relu and save), planes=planes, residual_bn=residual_bn, keep_f32=keep_f32,
                       out_dtype=out_dtype or K.F32)
        if self.training and tracked is not None:
            tracked.append(self.num_batches_tracked)
        if self._capture is not None and relu:
            o = out[0].f32 if isinstance(out[0], K.PlaneTensor) else out[0]
            self._capture[0][self._capture[1]] = o if o is not None else K.bn_apply(x, out[1], True)
        # the backward takes the ReLU sign from a 1-bit/element mask, not from the 4-byte activation
        return out[0], ((x, out[2] if relu else None, out[1], self.training) if save else None)

    def stats_only(self, x, tracked=None, relu_follows=True):
        """Statistics / running-stat update without the apply pass -> (raw x, saved [4, C]); the consumer evaluates
        relu((x - mean) * scale + shift) itself (fused split attention, timm/models/layers/split_attn.py)."""
        stats = None
        if isinstance(x, tuple):
            x, stats = x
        if self.training and x.numel() == x.shape[-1]:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                             % (tuple(x.shape),))
        saved = K.bn_stats(x, self.weight, self.bias, self.running_mean, self.running_var, self.training,
                           self.momentum, self.eps, stats if self.training else None)
        if self.training and tracked is not None:
            tracked.append(self.num_batches_tracked)
        if self._capture is not None and relu_follows:   # test instrumentation: the activation the fused kernels see
            self._capture[0][self._capture[1]] = K.bn_apply(x, saved, True)
        return x, saved

    @staticmethod
    def fuse(ctx, *more):
        """K.BnBwdFuse for the kernel that produces this BatchNorm's output gradient (`more`: contexts of further
        BatchNorms fed by the same gradient -- the downsample branch)."""
        return K.BnBwdFuse(ctx[1], [(c[0], c[2]) for c in (ctx,) + more])

    def bwd(self, dy, ctx, want_gout=False, fused=None, dx_dtype=None):
        """fused = BnBwdFuse.ext(i): dy is already masked and its sums are reduced (by the producer's epilogue).
        dx_dtype=torch.bfloat16: dx is stored as bf16 (Conv2d.grad_storage of the convolution in front)."""
        x, mask, saved, training = ctx
        if fused is not None:
            return K.bn_bwd(dy, None, x, saved, training, self._dg, self._db, want_gout, ext=fused,
                            dx_dtype=dx_dtype or K.F32)
        return K.bn_bwd(dy, None, x, saved, training, self._dg, self._db, want_gout, mask=mask, dx_dtype=dx_dtype or K.F32)


class LinearParams(nn.Module):
    """Parameter holder with nn.Linear's names / init; the arithmetic runs in the HIP kernels of the owner."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        bound = 1.0 / math.sqrt(in_features)
        self.weight = nn.Parameter(torch.empty(out_features, in_features).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(out_features).uniform_(-bound, bound))
        self._g = {}

    def _bind_grad(self, leaf, seg):
        self._g[leaf] = seg.view(self.weight.shape) if leaf == "weight" else seg


class GradArena:
    """One flat fp32 buffer holding the gradient of every trainable parameter, in named_parameters() order.
    `param.grad` are views into it (conv weights with the parameter's own HWIO strides).  Parameters that never
    receive a gradient on this path (slot.to_q.*, reference slot_attention.py:52-53) are excluded, like the
    `find_unused_parameters=True` of the reference's DDP wrap (train.py:140)."""

    def __init__(self, model, exclude=("to_q",)):
        self.entries = []       # (name, param, offset, numel)
        off = 0
        for name, p in model.named_parameters():
            if not p.requires_grad or any(e in name for e in exclude):
                continue
            self.entries.append((name, p, off, p.numel()))
            off += (p.numel() + 3) // 4 * 4
        self.numel = off
        # (no trainable parameter -- a frozen model whose INPUT requires grad: an empty arena on the model's device)
        dev = self.entries[0][1].device if self.entries else self._model_device(model)
        self.flat = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        self.views = {}
        for name, p, o, n in self.entries:
            seg = self.flat[o:o + n]
            if p.dim() == 4:
                co, cg, kh, kw = p.shape
                self.views[name] = seg.view(kh, kw, cg, co).permute(3, 2, 0, 1)
            elif p.dim() == 2 and getattr(p, "_hip_transposed", False):
                self.views[name] = seg.view(p.shape[1], p.shape[0]).t()
            else:
                self.views[name] = seg.view(p.shape)
        self._bind(model)

    @staticmethod
    def _model_device(model):
        p = next(model.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def _bind(self, model):
        mods = dict(model.named_modules())
        for m in mods.values():      # (bindings of an earlier arena: a parameter frozen since then gets no gradient)
            if isinstance(m, Conv2d):
                m._dw = m._db = None
            elif isinstance(m, BatchNorm2d):
                m._dg = m._db = None
            elif isinstance(getattr(m, "_g", None), dict):
                m._g.clear()
        for name, p, o, n in self.entries:
            mod_name, _, leaf = name.rpartition(".")
            m = mods[mod_name]
            seg = self.flat[o:o + n]
            if isinstance(m, Conv2d):
                if leaf == "weight":
                    co, cg, kh, kw = p.shape
                    m._dw = seg.view(kh, kw, cg, co)
                else:
                    m._db = seg
            elif isinstance(m, BatchNorm2d):
                if leaf == "weight":
                    m._dg = seg
                else:
                    m._db = seg
            else:
                hook = getattr(m, "_bind_grad", None)
                if hook is None:
                    raise RuntimeError("no gradient binding for parameter %s" % name)
                hook(leaf, seg)

    def first_offset(self, prefix):
        """Arena offset of the first parameter whose name starts with `prefix` (None if there is none)."""
        for name, p, o, n in self.entries:
            if name.startswith(prefix):
                return o
        return None

    def attach(self):
        """Expose the arena slices as param.grad (PyTorch semantics: .grad holds the gradient of the last backward)."""
        for name, p, o, n in self.entries:
            p.grad = self.views[name]

    def matches(self, model):
        cur = [(n, p) for n, p in model.named_parameters() if p.requires_grad and "to_q" not in n]
        if not cur and not self.entries:
            return self._model_device(model) == self.flat.device
        return len(cur) == len(self.entries) and all(a[1] is b[1] and b[1].device == self.flat.device
                                                     for a, b in zip(cur, self.entries))
