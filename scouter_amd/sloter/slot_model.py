"""SlotModel on the MI355X HIP path -- mirrors sloter/slot_model.py:10-127 of the reference (same constructor
`args`, attributes, state_dict keys and return structure: `log_probs` or `[log_probs, [loss, nll, area_loss]]`).

The whole step (backbone -> conv1x1+ReLU -> sine PE -> fused xSlot -> log_softmax/NLL + lambda*area) is ONE autograd
node: the forward launches the HIP kernels layer by layer and records what each layer's hand-written backward
needs; `loss.backward()` then runs those backward kernels in reverse and writes every parameter gradient into a
flat arena (`param.grad` are views of it).  There is no ATen arithmetic on the path and no CPU fallback."""
from collections import OrderedDict

import os

import torch
import torch.nn as nn

from .. import kernels as K
from ..nn_hip import Conv2d, FoldedConv, GradArena, StemConv2d
from ..timm.models import create_model
from .utils.position_encode import build_position_encoding
from .utils.slot_attention import SlotAttention

# bf16 activation storage under --precision bf16 (SlotModel.set_activation_storage); SCOUTER_BF16_STORAGE=0: fp32 storage
BF16_STORAGE_DEFAULT = os.environ.get("SCOUTER_BF16_STORAGE", "1") != "0"
# the per-step weight-plane split on its own stream next to the stem (SlotModel._forward_impl); 0: on the compute stream
SPLIT_ASYNC = os.environ.get("SCOUTER_SPLIT_ASYNC", "1") != "0"


class Identical(nn.Module):
    def forward(self, x):
        return x


def load_backbone(args):
    """reference slot_model.py:18-52 (resnet-family branch; the other timm families are out of scope)."""
    # slot_model.py:19-22: a 3-channel model (pretrained weights when args.pre_trained: a LOCAL file, see
    # timm/models/helpers.py -- raises when it is absent rather than freezing random layers), then the MNIST stem swap
    bone = create_model(args.model, pretrained=bool(getattr(args, "pre_trained", False)), num_classes=args.num_classes)
    if args.dataset == "MNIST":
        from ..nn_hip import StemConv2d
        bone.conv1 = StemConv2d(1, 64, 3, 2, 1)                 # slot_model.py:23-24
    if args.use_slot:
        if getattr(args, "use_pre", False):
            checkpoint = torch.load(f"saved_model/{args.dataset}_no_slot_checkpoint.pth", map_location="cpu", weights_only=False)
            new_state_dict = OrderedDict((k[9:], v) for k, v in checkpoint["model"].items())   # strip `backbone.`
            bone.load_state_dict(new_state_dict)
            print("load pre dataset parameter over")
        if not getattr(args, "grad", False):
            if "res" not in args.model:
                raise RuntimeError("only the resnet / resnest backbones are built")
            bone.global_pool = Identical()
            bone.fc = Identical()
    return bone


class _FusedStep(torch.autograd.Function):
    """The single autograd node of the model.  `anchor` is a dummy leaf that ties the outputs into the graph;
    parameter gradients are delivered through the flat arena (param.grad views), not through autograd edges."""

    @staticmethod
    def forward(ctx, anchor, model, x, target):
        ctx.set_materialize_grads(False)
        logp, stats, state = model._forward_impl(x, target, save=True)
        ctx.model, ctx.state = model, state
        return logp, stats[0], stats[1], stats[2]

    @staticmethod
    def backward(ctx, g_logp, g_loss, g_nll, g_term):
        # (an input that requires grad: the walk goes on to the image and its gradient -- NCHW fp32, the input's shape -- is
        #  returned on x's edge; autograd casts it for an input of another floating type)
        dx = ctx.model._backward_impl(ctx.state, g_logp, g_loss, g_nll, g_term, need_input_grad=ctx.needs_input_grad[2])
        ctx.state = None
        return None, None, dx, None


def _seeded_head_backward(m, logp, hstate, seed):
    """d(sum seed * log_probs) / d features by one head backward (SlotModel._head_backward), nothing of the backbone; the head
    parameters that require grad get their `.grad` overwritten.  What FeaturePass.grad and ImagePass.grad share, refusals
    included."""
    if not torch.is_tensor(seed) or seed.shape != logp.shape or seed.dtype != torch.float32 or seed.device != logp.device:
        raise ValueError("seed must be an fp32 tensor of shape %s on %s" % (tuple(logp.shape), logp.device))
    arena = m.grad_arena()
    dfeat = m._head_backward(hstate, seed.contiguous(), None, None, None, need_dfeat=True, post=None)
    K.join_side_stream(dfeat.device)                     # (the head's parameter gradients ran on the side stream)
    head = "backbone.fc." if not m.use_slot else None
    for name, p, _, _ in arena.entries:
        if name.startswith(head) if head else not name.startswith("backbone."):
            p.grad = arena.views[name]
    return dfeat


class FeaturePass:
    """What SlotModel.feature_pass returns: the backbone's output, the model's output and the head's backward from one to
    the other."""

    def __init__(self, model, features, log_probs, hstate):
        self.features, self.log_probs = features, log_probs
        self._model, self._hstate = model, hstate

    @torch.no_grad()
    def grad(self, seed):
        """seed: fp32 [B, classes] on the device -> d(sum seed * log_probs) / d features, NHWC fp32 [B, h, w, channel]: one
        head backward (SlotModel._head_backward), nothing of the backbone.  Head parameters that require grad get their
        `.grad` overwritten, as in any backward of the model; the backbone's parameter gradients are not touched."""
        return _seeded_head_backward(self._model, self.log_probs, self._hstate, seed)


class ImagePass:
    """What SlotModel.image_pass returns: the model's output, the backbone's output, and the backward from the output to the
    IMAGE on the folded weights -- one forward, any number of gradients."""

    def __init__(self, model, features, log_probs, bstate, hstate, wds, gen):
        self.features, self.log_probs = features, log_probs
        self._model, self._bstate, self._hstate, self._wds, self._gen = model, bstate, hstate, wds, gen

    RULES = {"gradient": K.RULE_GRADIENT, "guided": K.RULE_GUIDED, "deconvnet": K.RULE_DECONVNET}

    def _check(self, rule):
        """the refusals of grad / grad_from that come before any launch -> the kernels' rule"""
        if not isinstance(rule, str) or rule not in self.RULES:
            raise ValueError("rule must be 'gradient', 'guided' or 'deconvnet', got %r" % (rule,))
        if self._model._fold_gen != self._gen:
            raise RuntimeError("ImagePass.grad: the model has folded its weights again since this pass; run image_pass again")
        return self.RULES[rule]

    @torch.no_grad()
    def grad(self, seed):
        """seed: fp32 [B, n_outputs] on the device -> d(sum seed * log_probs) / d x, NCHW fp32 in the shape of the pass's images:
        one head backward (as FeaturePass.grad, with its refusals and its effect on the head's `.grad`), then the backbone's
        input gradients on the folded weights (ResNet.image_bwd) -- no BatchNorm kernel, no backbone parameter gradient.  May be
        called any number of times; a pass whose model has folded again since (new weights in the same buffers) refuses.
        It is grad_from(feature_grad(seed)): its parameter list is pinned (tests/test_foldgrad_cpu.py), so the gradient under
        another ReLU rule is grad_from(feature_grad(seed), rule)."""
        self._check("gradient")
        return self.grad_from(self.feature_grad(seed))

    @torch.no_grad()
    def feature_grad(self, seed):
        """d(sum seed * log_probs) / d features, NHWC fp32 in the shape of `.features`: the head backward `grad` runs, with its
        refusals and its effect on the head's `.grad`.  The head keeps the plain rule under every `rule` of grad_from."""
        return _seeded_head_backward(self._model, self.log_probs, self._hstate, seed)

    @torch.no_grad()
    def grad_from(self, dfeat, rule="gradient"):
        """The backbone's backward alone: dfeat (NHWC fp32 in the shape of `.features`, not written) -> the gradient of the image,
        NCHW fp32.  rule is what the backward does where it meets a ReLU OF THE BACKBONE (the entries of relu_outputs() other
        than "conv1x1" and "maxpool"), with g the gradient arriving at the ReLU's output y:
            "gradient"    y > 0 ? g : 0               the derivative
            "guided"      (y > 0 and g > 0) ? g : 0   guided backpropagation (Springenberg et al. 2015)
            "deconvnet"   g > 0 ? g : 0               the deconvnet rule (Zeiler & Fergus 2014)
        The pool's gather, the radix softmax, the average pools and every convolution keep their ordinary backward.  Anything else
        is a ValueError, a stale pass a RuntimeError, both before any launch."""
        r = self._check(rule)
        if not torch.is_tensor(dfeat) or dfeat.shape != self.features.shape or dfeat.dtype != torch.float32 or \
                dfeat.device != self.features.device:
            raise ValueError("dfeat must be an fp32 tensor of shape %s on %s" % (tuple(self.features.shape), self.features.device))
        m = self._model
        return m.backbone.image_bwd(dfeat.contiguous(), self._bstate, self._wds, r)

    def relu_outputs(self):
        """{name: activation} whose signs the backward used, in the keys of the training path's capture: the name of the
        BatchNorm each ReLU follows (the split-attention gate's hidden activation under its `bn1`), `conv1x1` for the head's,
        and `maxpool` for the max-pool's window indices (uint8 NHWC).  For tests that pin an oracle to this pass's pattern."""
        m = self._model
        names = {mod: n for n, mod in m.named_modules()}
        with torch.no_grad():
            pairs, arg = m.backbone.image_relus(self._bstate)
        out = {names[bn]: t for bn, t in pairs}
        if m.use_slot:
            out["conv1x1"] = self._hstate[1]
        out["maxpool"] = arg
        return out


class SlotModel(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.use_slot = args.use_slot
        # "fp32" (parity path) or "bf16": convolution matrix inputs rounded to bf16, fp32 accumulation; the wide bottleneck
        # tensors stored as bf16 (set_activation_storage)
        self.precision = str(getattr(args, "precision", "fp32"))
        if self.precision not in ("fp32", "bf16"):
            raise ValueError("precision must be fp32 or bf16, got %r" % self.precision)
        self.backbone = load_backbone(args)
        self.set_precision(self.precision)
        self.set_planes(int(os.environ.get("SCOUTER_PLANES", "3")))
        self.set_x3(K.X3_DEFAULT)
        self._arena = None
        self._anchor = None
        self._split_device = None
        self.inference_fold = False          # set_inference_fold
        self._folder = None                  # K.BnFolder: table + the flat buffer of every folded weight / bias
        self._fold_splitter = K.PlaneWeightSplitter()
        self._fold_gen = 0                   # folds so far (ImagePass.grad: the folded buffers are rewritten in place)
        self._fold_stale = True              # (a property: going stale drops the folded weights' input-gradient planes)
        self._flatten_tracked()              # BatchNorm counters: views of one flat buffer, from construction on
        self._post_backward_hooks = []       # called with the GradArena after every backward (data-parallel reduce)
        self._grad_ready_hooks = []          # called (arena, lo, hi) as soon as arena.flat[lo:hi] is final
        self.last_stats = None               # device tensor [loss, nll, area**power, top1, area] of the last forward
        if not self.use_slot:                # FC baseline (slot_model.py:75-77): backbone + global pool + fc
            if args.pre_trained:
                self.dfs_freeze(self.backbone, args.freeze_layers)
            return
        self.feature_size = 9            # kept for attribute compatibility; the grid is derived from the features
        self.channel = args.channel
        self.slots_per_class = args.slots_per_class
        self.conv1x1 = Conv2d(self.channel, args.hidden_dim, 1, 1, 0, bias=True)
        if args.pre_trained:
            self.dfs_freeze(self.backbone, args.freeze_layers)
        self.slot = SlotAttention(args.num_classes, self.slots_per_class, args.hidden_dim, vis=args.vis,
                                  vis_id=args.vis_id, loss_status=args.loss_status, power=args.power,
                                  to_k_layer=args.to_k_layer)
        self.position_emb = build_position_encoding("sine", hidden_dim=args.hidden_dim)
        self.lambda_value = float(args.lambda_value)

    # ---- BatchNorm-folded inference
    def set_inference_fold(self, enabled):
        """enabled: an eval-mode forward that builds no training graph (model.eval() + torch.no_grad(), or no trainable
        parameter and an input that does not require grad) runs with every BatchNorm of the backbone folded into the convolution in front of it -- w' = w * s,
        b' = beta - running_mean * s (+ conv_bias * s), s = gamma / sqrt(running_var + eps), formed in fp64 by ONE launch
        (K.BnFolder) -- so a block is three convolutions with bias / ReLU / residual in their epilogues, the split-attention
        gate one launch, and no BatchNorm kernel runs (nn_hip.InferRoute, ResNet.features_fwd_folded).  Off (the default) and
        in every other case the forward is the layer-by-layer one.  The head is the same either way.
        The folded tensors are no parameters or buffers (state_dict() is untouched): they live in one flat buffer of the
        model and are rebuilt on the first folded forward after train() / eval(), load_state_dict, a move or cast of the
        module, set_precision / set_planes / set_x3, a training forward, or refold() -- call refold() after changing
        parameters in any other way (the fused optimizer and the BatchNorm kernels write through raw pointers, so tensor
        version counters do not see them).  Activations of the folded path are stored as fp32, also under precision "bf16"
        (whose convolutions still round their matrix inputs to bf16).  Measured: +1.3 % at batch 70 and
        1.8 x on single images in fp32; under precision "bf16" at batch 256 it is 17 % SLOWER than the unfolded path with its
        bf16 storage -- leave it off there.
        Autograd does not see the folded path: an input that requires grad (d output / d image, tools/attribution.py
        route="autograd") runs the unfolded eval forward, fold or no fold, and gets the same gradient.  The folded path's own
        backward is explicit -- image_pass(x).grad(seed), a gradient with respect to the image only -- and runs whether this
        switch is on or off."""
        self.inference_fold = bool(enabled)
        self._fold_stale = True

    @property
    def _fold_stale(self):
        return self.__dict__.get("_fold_is_stale", True)

    @_fold_stale.setter
    def _fold_stale(self, stale):
        self.__dict__["_fold_is_stale"] = bool(stale)
        if stale:                            # the planes image_pass split from the folded weights go with the fold
            self.__dict__["_fold_wd"] = None
            self.__dict__["_fold_dsplitter"] = None

    def refold(self):
        """The next folded forward folds the current parameters and running statistics again."""
        self._fold_stale = True

    def fold_pairs(self):
        """[(convolution name, BatchNorm name)] set_inference_fold folds: every BatchNorm of the backbone is in one pair."""
        names = {m: n for n, m in self.named_modules()}
        return [(names[c], names[b]) for c, b in self.backbone.fold_pairs()]

    def train(self, mode=True):
        self._fold_stale = True
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._fold_stale = True
        return super().load_state_dict(*args, **kwargs)

    def _refold(self):
        pairs = self.backbone.fold_pairs()
        items = [(K.hwio(c.weight), c.bias, b.weight, b.bias, b.running_mean, b.running_var, b.eps,
                  c.kpad if isinstance(c, StemConv2d) else 0) for c, b in pairs]
        if self._folder is None or self._folder.key != K.BnFolder.pointers(items):
            self._folder = K.BnFolder(items)
        outs = self._folder.run()
        split = [(c, w) for (c, _), (w, _) in zip(pairs, outs) if c.infer_route().split]
        planes = self._fold_splitter.run([(w, c.groups, True, False) for c, w in split], 3) if split else []
        wf = {c: p[0] for (c, _), p in zip(split, planes)}
        for (c, _), (w, b) in zip(pairs, outs):
            # (precision "bf16": the transposed bf16 weight the bf16-input forward reads, once per fold instead of per call)
            wt = K.weight_bf16t(w, c.groups) if c.precision == "bf16" else None
            c._fold = FoldedConv(w, b, wf.get(c), wt)
        self._fold_gen += 1
        self._fold_stale = False

    def _fold_dgrad_planes(self):
        """{layer: input-gradient planes of its FOLDED weight} for the layers whose route offers a bf16x3 input gradient for a
        plain fp32 gradient ("xhalo" / "x3"): one launch of a splitter of their own on the first image_pass after a fold --
        an inference-only user never pays for them -- and dropped with the fold (the _fold_stale setter)."""
        wds = self.__dict__.get("_fold_wd")
        if wds is None:
            convs = [c for c, _ in self.backbone.fold_pairs()
                     if not isinstance(c, StemConv2d) and any(f in ("xhalo", "x3") for f in c.route().dgrad)]
            wds = {}
            if convs:
                splitter = self.__dict__["_fold_dsplitter"] = K.PlaneWeightSplitter()
                outs = splitter.run([(c._fold.w, c.groups, False, True) for c in convs], 3)
                wds = {c: o[1] for c, o in zip(convs, outs)}
            self.__dict__["_fold_wd"] = wds
        return wds

    def _forward_folded(self, x, target):
        if not x.is_cuda:
            raise RuntimeError("scouter_amd.SlotModel runs on a HIP device (got a %s tensor); there is no CPU fallback" % x.device)
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        if self._fold_stale or self._folder is None:
            self._refold()
        feat = self.backbone.features_fwd_folded(x)
        logp, stats, _ = self._head_forward(feat, target, False)
        return logp, stats

    def set_precision(self, precision):
        """Matrix-input precision of the BACKBONE convolutions (the xSlot head incl. conv1x1 always runs in fp32).
        Stored on each layer object, so two models of different precision never share a switch."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be fp32 or bf16, got %r" % precision)
        self.precision = precision
        self._fold_stale = True
        for mod in self.backbone.modules():
            if isinstance(mod, Conv2d):
                mod.precision = precision
        self.set_activation_storage("bf16" if precision == "bf16" and BF16_STORAGE_DEFAULT else "fp32")

    def set_activation_storage(self, storage):
        """"bf16" (the default under precision "bf16"; SCOUTER_BF16_STORAGE=0 turns it off): every ResNeSt bottleneck but
        the last stores its 4x-wide tensors -- conv3 / downsample-convolution outputs and the block output -- as bf16 in
        HBM (half the bytes of the passes that dominate BASELINE configs[4]); arithmetic and every gradient stay fp32.
        The oracle emulates it with oracle.torch_oracle.ACTIVATION_STORAGE."""
        if storage not in ("fp32", "bf16"):
            raise ValueError("activation storage must be fp32 or bf16, got %r" % storage)
        if storage == "bf16" and self.precision != "bf16":
            raise ValueError("bf16 activation storage is an option of precision 'bf16'")
        from ..timm.models.resnest import ResNestBottleneck, GRAD_STREAM_BF16_DEFAULT
        blocks = [m for m in self.backbone.modules() if isinstance(m, ResNestBottleneck)]
        for i, blk in enumerate(blocks):
            blk.store_bf16 = storage == "bf16" and i + 1 < len(blocks)
            # the residual-stream gradient follows the activation storage (SCOUTER_BF16_GRAD_STREAM=0: fp32 under bf16 storage)
            blk.grad_stream_bf16 = storage == "bf16" and GRAD_STREAM_BF16_DEFAULT
        self.activation_storage = storage if blocks else "fp32"

    def set_planes(self, nplanes):
        """3 (default): the grouped 3x3 convolutions of the split-attention blocks run on the bf16 matrix cores over
        exact three-way bf16 splits of their fp32 operands (csrc/conv_planes.hip: six products per fp32 product, fp32
        accumulation -- the accuracy of the exact-fp32 MFMA kernel at 1.6x its speed); 0: every convolution on the fp32
        MFMA kernels.  Only layers whose shapes qualify switch (Conv2d.route: planes_in / planes_dy).  With precision="bf16" the
        same layers take ONE plane -- the RNE-rounded bf16 value the bf16-input kernels would form in flight -- from their
        producers: half the operand bytes, LDS-DMA instead of a conversion pass through registers."""
        if nplanes not in (0, 3):
            raise ValueError("planes must be 0 or 3")
        self._fold_stale = True
        from ..timm.models.layers.split_attn import SplitAttnConv2d
        for mod in self.backbone.modules():
            if isinstance(mod, SplitAttnConv2d):
                mod.conv.planes = nplanes
        self._plane_convs = [m for m in self.backbone.modules() if isinstance(m, Conv2d) and m.planes]
        self._wsplitter = K.PlaneWeightSplitter()

    def set_x3(self, bits):
        """Deep pointwise (1x1) convolutions of the backbone on the register-split bf16x3 GEMM (csrc/conv_x3.hip: fp32
        tensors in and out, fp32-grade products on the bf16 matrix cores): bit 0 forward, bit 1 plain input gradient, bit 2
        input gradient with the fused BatchNorm-backward epilogue, bit 3 weight gradient, bit 4 the forward of the 3x3
        layers with 32 input channels per group (kernels.x3_conv_eligible: the stem's 32 -> 64 convolution), bit 5 the forward of
        the short-K pointwise layers on the persistent bf16x3 kernel (nn_hip.Conv2d.route, csrc/conv_pw_persist_x3.h), bit 6
        the INPUT GRADIENT of the 3x3 layers with 32 input channels per group on the persistent resident-rows kernel
        (csrc/conv_xhalo.hip: both deep-stem convolutions and layer1's radix convolutions, plane
        layers whose gradient planes would need 64), bit 7 (opt-in) the FORWARD of the 3x3 layers with 32 output channels per
        group on the same kernel (the stem's 32 -> 32); 0: the exact-fp32 MFMA kernels.  Which layers qualify is a static function of their channels (kernels.x3_eligible,
        kernels.xpw_fwd_eligible), so the forward does not depend on batch or timing."""
        if bits & ~255:
            raise ValueError("x3 bits must be within 0..255")
        self._fold_stale = True
        self._convs = [m for m in self.backbone.modules() if isinstance(m, Conv2d) and not isinstance(m, StemConv2d)]
        for mod in self._convs:
            mod.x3 = int(bits)

    @property
    def _x3_convs(self):
        """The backbone layers with a pass on a register-split kernel (Conv2d.x3_mode)."""
        return [m for m in self._convs if m.x3_mode()]

    def _split_items(self, save):
        """[(layer, forward planes, input-gradient planes)] of this step's one-launch weight split (Conv2d.route): every plane
        layer, then the layers on the register-split kernels -- whose three-way planes are split in fp32 mode only."""
        convs = [c for c in self._plane_convs if c._nplanes()]
        xconvs = self._x3_convs if not convs or convs[0]._nplanes() == 3 else []
        items = [(c, c.route().split_fwd, bool(save and c.route().split_dgrad)) for c in convs + xconvs]
        return [(c, f, d) for c, f, d in items if f or d]

    def set_side_stream(self, enabled):
        """Weight gradients on the side stream (default) or serially on the compute stream (per-kernel timing)."""
        for mod in self.modules():
            if isinstance(mod, Conv2d) or hasattr(mod, "_param_grads"):        # (+ the xSlot head's parameter gradients)
                mod.use_side_stream = bool(enabled)

    def dfs_freeze(self, model, freeze_layer_num):
        """reference slot_model.py:79-94"""
        if freeze_layer_num == 0:
            return
        unfreeze_layers = ["layer4", "layer3", "layer2", "layer1"][:4 - freeze_layer_num]
        for name, child in model.named_children():
            if any(u in name for u in unfreeze_layers):
                continue
            for param in child.parameters():
                param.requires_grad = False
            self.dfs_freeze(child, freeze_layer_num)

    # ------------------------------------------------------------------------------------------------------------
    def grad_arena(self):
        if self._arena is None or not self._arena.matches(self):
            self._arena = GradArena(self)
        return self._arena

    def _fc_forward(self, feat, target, save):
        logits, cctx = self.backbone.classifier_fwd(feat, save)
        if target is not None and target.dtype != torch.int64:
            target = target.long()
        logp, stats = K.slot_loss_fwd(logits, target, None, 1.0, 0.0, 1.0)      # slot_model.py:117,124
        self.last_stats = stats
        return logp, stats, ((cctx, logp, stats, target) if save else None)

    def _fc_backward(self, hstate, g_logp, g_loss, g_nll, g_term, need_dfeat=True):
        cctx, logp, stats, target = hstate
        f32 = lambda g: None if g is None else g.float().contiguous()
        dlogits, _ = K.slot_loss_bwd(logp, target, stats, f32(g_loss), f32(g_nll), None, f32(g_logp), 1.0, 0.0, 1.0)
        return self.backbone.classifier_bwd(dlogits, cctx, need_dfeat)

    def _head_forward(self, feat, target, save):
        """feat: NHWC backbone features [B, h, w, channel] -> (log_probs, stats, head state)."""
        if not self.use_slot:
            return self._fc_forward(feat, target, save)
        if feat.shape[-1] != self.channel:
            raise RuntimeError("backbone produced %d channels, args.channel is %d" % (feat.shape[-1], self.channel))
        xmap, cctx = self.conv1x1.fwd(feat, save, relu=True)                  # slot_model.py:108-109
        B, h, w, d = xmap.shape
        PE = self.position_emb.table(h, w, feat.device)                       # slot_model.py:110-111
        so = self.slot.fwd(xmap.view(B, h * w, d), PE)                        # slot_model.py:116
        S, N = self.slot.num_slots, h * w
        if target is not None and target.dtype != torch.int64:
            target = target.long()
        logp, stats = K.slot_loss_fwd(so["logits"], target, so["area_part"], B * S * N, self.lambda_value,
                                      self.slot.power)                        # slot_model.py:117-121
        self.last_stats = stats
        if self.slot.vis:
            self.slot.save_vis()
        return logp, stats, ((cctx, xmap, PE, so, logp, stats, target) if save else None)

    def _head_backward(self, hstate, g_logp, g_loss, g_nll, g_term, need_dfeat=True, post=None):
        """post: the last backbone block's K.BnBwdFuse -- conv1x1's input-gradient epilogue finishes its reductions."""
        if not self.use_slot:
            return self._fc_backward(hstate, g_logp, g_loss, g_nll, g_term, need_dfeat)
        cctx, xmap, PE, so, logp, stats, target = hstate
        B, h, w, d = xmap.shape
        S, N = self.slot.num_slots, h * w
        f32 = lambda g: None if g is None else g.float().contiguous()
        dlogits, g_area = K.slot_loss_bwd(logp, target, stats, f32(g_loss), f32(g_nll), f32(g_term), f32(g_logp),
                                          B * S * N, self.lambda_value, self.slot.power)
        dX = self.slot.bwd(xmap.view(B, N, d), PE, so, dlogits, g_area)
        dxr = K.relu_bwd(dX.view(B, h, w, d), xmap)
        return self.conv1x1.bwd(dxr, cctx, need_dx=need_dfeat, post=post if need_dfeat else None)

    def _forward_impl(self, x, target, save):
        if not x.is_cuda:
            raise RuntimeError("scouter_amd.SlotModel runs on a HIP device (got a %s tensor); there is no CPU fallback "
                               "-- the CPU restatement lives in oracle/ and is test infrastructure only" % x.device)
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        tracked = []
        feat, bctx = self._backbone_forward(x, save, tracked)                 # NHWC [B, h, w, channel]
        logp, stats, hstate = self._head_forward(feat, target, save)
        if tracked:
            self._bump_tracked(tracked)                                       # BatchNorm num_batches_tracked
        return logp, stats, ((bctx, hstate) if save else None)

    def _backbone_forward(self, x, save, tracked):
        """This step's weight planes, then the layer-by-layer backbone forward -> (NHWC features, backbone state)."""
        items = self._split_items(save)
        if items:      # this step's weight planes of every plane convolution: one launch into persistent buffers ...
            # ... on its own stream NEXT TO the stem's kernels (the stem reads no planes; MFMA-bound next to a byte-moving
            # pass): the backbone joins it after the max-pool (`_post_stem_hooks`).  SCOUTER_SPLIT_ASYNC=0: on the compute stream
            hooks = getattr(self.backbone, "_post_stem_hooks", None)
            use_async = SPLIT_ASYNC and hooks is not None
            if use_async and not hooks:
                hooks.append(lambda: K.join_side_stream(self._split_device, "wsplit") if self._split_device is not None else None)
            self._split_device = x.device if use_async else None
            with K.side_stream(x.device, enabled=use_async, which="wsplit"):
                # (plane layers come first: their number of planes; the register-split layers take three)
                outs = self._wsplitter.run([(K.hwio(c.weight), c.groups, f, d) for c, f, d in items],
                                           items[0][0]._nplanes() or 3)
            for (c, f, d), o in zip(items, outs):
                c._wsplit = o
        return self.backbone.features_fwd(x, save, tracked)

    def feature_pass(self, x):
        """One eval-mode forward that keeps the backbone's output and the head's state: what a class activation map needs
        (tools/attribution.py gradcam).  Returns a FeaturePass: `.log_probs` [B, classes], `.features` (NHWC fp32
        [B, h, w, channel]) and `.grad(seed)` = d(sum seed * log_probs) / d features, any number of times.
        The model runs in eval mode (no BatchNorm buffer or counter moves; the caller's mode is restored); the backbone runs
        folded when set_inference_fold is on and layer by layer otherwise, and saves nothing either way -- the gradient never
        walks into it.  Works with use_slot on and off."""
        if not x.is_cuda:
            raise RuntimeError("scouter_amd.SlotModel runs on a HIP device (got a %s tensor); there is no CPU fallback" % x.device)
        if x.dim() != 4:
            raise ValueError("images must be [B, C, H, W], got shape %s" % (tuple(x.shape),))
        was_training = self.training
        if was_training:
            self.eval()
        try:
            with torch.no_grad():
                x = x.detach().contiguous()
                if x.dtype != torch.float32:
                    x = x.float()
                if self.inference_fold:
                    if self._fold_stale or self._folder is None:
                        self._refold()
                    feat = self.backbone.features_fwd_folded(x)
                else:
                    feat, _ = self._backbone_forward(x, False, [])
                logp, _, hstate = self._head_forward(feat, None, True)
        finally:
            if was_training:
                self.train(True)
        return FeaturePass(self, feat, logp, hstate)

    def image_pass(self, x):
        """One eval-mode forward on the BatchNorm-FOLDED weights that keeps what a gradient with respect to the image needs:
        every ReLU output, the max-pool's window indices, the split-attention vectors and the head's state -- no BatchNorm
        statistics, masks or convolution inputs of the training backward.  Returns an ImagePass: `.log_probs` [B, n_outputs],
        `.features` (NHWC fp32), `.grad(seed)` = d(sum seed * log_probs) / d x (NCHW fp32, any number of times) and
        `.relu_outputs()`.  The weights are folded again when stale, as in feature_pass, and the pass runs whether or not
        set_inference_fold is on: it has no unfolded form.  No BatchNorm buffer or counter moves, no backbone parameter gradient
        is computed or touched, the caller's mode is restored.  resnet18 / resnest26d / resnest50d, use_slot on and off, fp32:
        precision "bf16" is refused (DESIGN.md advises against the folded path there)."""
        if self.precision == "bf16":
            raise NotImplementedError('image_pass: precision "bf16" has no folded backward (fp32 only)')
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError("scouter_amd.SlotModel runs on a HIP device (got %s); there is no CPU fallback"
                               % (x.device if torch.is_tensor(x) else type(x).__name__,))
        if x.dim() != 4:
            raise ValueError("images must be [B, C, H, W], got shape %s" % (tuple(x.shape),))
        was_training = self.training
        if was_training:
            self.eval()
        try:
            with torch.no_grad():
                x = x.detach().contiguous()
                if x.dtype != torch.float32:
                    x = x.float()
                if self._fold_stale or self._folder is None:
                    self._refold()
                wds = self._fold_dgrad_planes()
                feat, bstate = self.backbone.image_fwd(x)
                logp, _, hstate = self._head_forward(feat, None, True)
                gen = self._fold_gen
        finally:
            if was_training:
                self.train(True)
        return ImagePass(self, feat, logp, bstate, hstate, wds, gen)

    def head_pass(self, features):
        """`feature_pass` without the backbone: NHWC fp32 `features` [n, h, w, channel] on the device -- the backbone's output, or
        anything of its shape, such as the noisy samples of tools/attribution.py information_bottleneck -- go through one
        eval-mode head forward.  Returns a FeaturePass whose `.features` are the tensor given and whose `.grad(seed)` is the
        gradient with respect to it, any number of times.  Works with use_slot on and off; the caller's mode is restored."""
        if not torch.is_tensor(features) or not features.is_cuda:
            raise RuntimeError("scouter_amd.SlotModel runs on a HIP device (got %s); there is no CPU fallback"
                               % (features.device if torch.is_tensor(features) else type(features).__name__,))
        if features.dim() != 4 or features.dtype != torch.float32:
            raise ValueError("features must be fp32 NHWC [n, h, w, channel], got %s %s" % (features.dtype, tuple(features.shape)))
        was_training = self.training
        if was_training:
            self.eval()
        try:
            with torch.no_grad():
                feat = features.detach().contiguous()
                logp, _, hstate = self._head_forward(feat, None, True)
        finally:
            if was_training:
                self.train(True)
        return FeaturePass(self, feat, logp, hstate)

    def loss_seed(self, loss):
        """A cached tensor of ones shaped like the scalar loss: `loss.backward(model.loss_seed(loss))` spares autograd the
        `ones_like` fill it launches for a bare `loss.backward()` (the last ATen kernel of the step; engine.py, bench.py)."""
        seed = getattr(self, "_loss_seed", None)
        if seed is None or seed.device != loss.device or seed.shape != loss.shape or seed.dtype != loss.dtype:
            seed = self._loss_seed = torch.ones_like(loss)
        return seed

    def _flatten_tracked(self):
        """Every BatchNorm's `num_batches_tracked` becomes a view of ONE flat int64 buffer (same buffer names / shapes in the
        state_dict).  Done at construction and after every `_apply` (module.to / .cuda), never during a step: buffer identity is
        stable from the first forward on, so references taken by EMA copies, external buffer lists or a captured hipGraph
        keep pointing at the counters that advance."""
        from ..nn_hip import BatchNorm2d
        bns = [m for m in self.modules() if isinstance(m, BatchNorm2d)]
        self._nbt_runs = {}
        if not bns:
            self._nbt_flat, self._nbt_index = None, {}
            return
        flat = torch.stack([m.num_batches_tracked.detach().reshape(()) for m in bns]).contiguous()
        for i, m in enumerate(bns):
            m._buffers["num_batches_tracked"] = flat[i]
        self._nbt_flat = flat
        self._nbt_index = {flat[i].data_ptr(): i for i in range(len(bns))}

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if hasattr(self, "_nbt_flat"):
            self._flatten_tracked()
        self._fold_stale = True
        return out

    def _bump_tracked(self, tracked):
        """num_batches_tracked += 1 for the train-mode BatchNorms of this forward (one launch of the library per contiguous run of
        counters in the flat buffer -- ONE when every BatchNorm trains -- instead of an ATen multi-tensor kernel); a BatchNorm
        that ran twice in the forward is counted twice."""
        key = tuple(t.data_ptr() for t in tracked)
        runs = self._nbt_runs.get(key)
        if runs is None:
            if any(p not in self._nbt_index for p in key):
                # a counter was re-assigned behind the model's back (module.num_batches_tracked = ...): flatten again and follow
                # this forward's tensors to their modules
                from ..nn_hip import BatchNorm2d
                by_ptr = {m.num_batches_tracked.data_ptr(): m for m in self.modules() if isinstance(m, BatchNorm2d)}
                mods = [by_ptr[p] for p in key]
                self._flatten_tracked()
                idx = [self._nbt_index[m.num_batches_tracked.data_ptr()] for m in mods]
            else:
                idx = [self._nbt_index[p] for p in key]
            count = {}
            for i in idx:
                count[i] = count.get(i, 0) + 1
            runs, order = [], sorted(count)
            for i in order:
                if runs and runs[-1][1] == i and runs[-1][2] == count[i]:
                    runs[-1][1] = i + 1
                else:
                    runs.append([i, i + 1, count[i]])
            self._nbt_runs[key] = runs
        for lo, hi, c in runs:
            K.iadd_i64(self._nbt_flat[lo:hi], c)

    def _backward_impl(self, state, g_logp, g_loss, g_nll, g_term, need_input_grad=False):
        """need_input_grad: the backbone backward runs whatever trains and goes on to the image (ResNet.features_bwd);
        returns its gradient (None otherwise).  The parameter gradients are the same bits either way: the extra launches
        come after their producers."""
        bctx, hstate = state
        arena = self.grad_arena()
        need = need_input_grad or self.backbone._first_trainable_stage() < 5
        last = self.backbone.last_fuse(bctx, need_input_grad) if need and self.use_slot else None
        dfeat = self._head_backward(hstate, g_logp, g_loss, g_nll, g_term, need_dfeat=need, post=last)
        # gradient ranges become final from the END of the arena (head, layer4) towards its start (stem)
        done_hi = [arena.numel]

        def stage_done(name):
            lo = arena.first_offset("backbone." + name + ".")
            if lo is not None and lo < done_hi[0]:
                K.join_side_stream(arena.flat.device)       # this stage's weight gradients ran on the side stream
                for hook in self._grad_ready_hooks:
                    hook(arena, lo, done_hi[0])
                done_hi[0] = lo
        dx = None
        if need:
            dx = self.backbone.features_bwd(dfeat, bctx, stage_done if self._grad_ready_hooks else None, own=last,
                                            need_input_grad=need_input_grad)
        K.join_side_stream(arena.flat.device)               # all weight gradients are in the arena from here on
        if self._grad_ready_hooks and done_hi[0] > 0:
            for hook in self._grad_ready_hooks:
                hook(arena, 0, done_hi[0])
        arena.attach()
        for hook in self._post_backward_hooks:
            hook(arena)
        return dx

    def forward(self, x, target=None):
        # (an input that requires grad takes the autograd route too -- in eval mode and with nothing trainable as well: the
        #  node's backward returns d output / d image)
        train_graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if train_graph:
            if self._anchor is None or self._anchor.device != x.device:
                self._anchor = torch.zeros(1, device=x.device, requires_grad=True)
            self.grad_arena()
            output, loss, nll, attn_loss = _FusedStep.apply(self._anchor, self, x, target)
        elif self.inference_fold and not self.training:
            output, stats = self._forward_folded(x, target)
            loss, nll, attn_loss = stats[0], stats[1], stats[2]
        else:
            output, stats, _ = self._forward_impl(x, target, save=False)
            loss, nll, attn_loss = stats[0], stats[1], stats[2]
        if self.training:
            self._fold_stale = True          # (running statistics moved; the optimizer step that follows moves the weights)
        if target is not None:
            return [output, [loss, nll, attn_loss]] if self.use_slot else [output, [loss]]
        return output
