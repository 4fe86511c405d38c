"""The 2-D backbone's head on this package's kernels (mvn/models/pose_resnet.py:266-291, 312-316;
DESIGN.md §4.16): the three ``ConvTranspose2d(Cin, 256, 4, stride=2, padding=1)`` + ``BatchNorm2d``
+ ``ReLU`` that take ``layer4``'s maps to the 256-channel feature maps, one ``deconv4s2`` launch
each (csrc/deconv_head.hip, bf16 MFMA), and ``final_layer`` through ``model.feature_conv``.
``deconv4s2_project`` is the last layer with the volumetric model's ``process_features`` behind it
in the same launch: the 256-channel maps are not written.

``DeconvHeadEval`` is the head alone, from ``layer4``'s output to ``(heatmaps, features)``;
``BackboneEval`` is the reference's ``PoseResNet.forward`` with its own trunk modules in front of
it.  By default the confidence heads and the ResNet trunk stay with torch;
``BackboneEval.from_reference(..., trunk="kernels")`` runs ``layer1`` .. ``layer4`` on ``resnet.TrunkEval``
 and ``confidences="kernels"`` the heads on ``confidence.ConfidenceHeadEval`` (§4.20).
Eval mode, inference-only.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from . import _ops
from .model import _feature_conv_params, feature_conv
from .op import _dtype_code
from .v2v import _bn_fold, _f64, _inference_only, _pack_mfma_a

COUT = _ops.DECONV_COUT
MIN_CIN, MAX_CIN = 32, 2048
MAX_PIXELS = (2 ** 31 - 1) // 4096       # H * W of one input image: its f32 output image stays below 2^31 bytes
FINAL_ROWS = _ops.FEATURE_COUT           # final_layer runs as feature_conv: at most 32 joints


class DeconvParams(NamedTuple):
    """What ``fold_deconv_block`` returns: packed bf16 weights and f32 scale / shift."""
    packed: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def _check_cin(what, cin):
    if cin % 32 != 0 or not MIN_CIN <= cin <= MAX_CIN:
        raise RuntimeError(f"{what}: the input channels must be a multiple of 32 in [{MIN_CIN}, {MAX_CIN}], got {cin}")


def pack_deconv4_weight(w):
    """(cin, 256, 4, 4) float64 ConvTranspose2d weight -> (16, cin / 32, 16, 64, 8) bf16 as mvn_deconv4s2
    reads it: [tap = ky*4 + kx][kp][m][lane][j] = w[32 kp + 8 (lane >> 4) + j][16 m + (lane & 15)][ky][kx]."""
    if w.dim() != 4 or tuple(w.shape[1:]) != (COUT, 4, 4):
        raise RuntimeError(f"expected a (Cin, {COUT}, 4, 4) ConvTranspose2d weight, got {tuple(w.shape)}")
    cin = w.shape[0]
    _check_cin("pack_deconv4_weight", cin)
    return _pack_mfma_a(w.permute(2, 3, 1, 0).reshape(16, COUT, cin))                # rows cout, K-slots cin


def _check_deconv(what, deconv, bn):
    """The layer is what mvn_deconv4s2 computes, or a RuntimeError naming what it is instead."""
    if not isinstance(deconv, nn.ConvTranspose2d):
        raise RuntimeError(f"{what}: expected a ConvTranspose2d, got {type(deconv).__name__}")
    if not isinstance(bn, nn.BatchNorm2d):
        raise RuntimeError(f"{what}: expected a BatchNorm2d behind the ConvTranspose2d, got {type(bn).__name__}")
    found = dict(kernel_size=tuple(deconv.kernel_size), stride=tuple(deconv.stride), padding=tuple(deconv.padding),
                 output_padding=tuple(deconv.output_padding), dilation=tuple(deconv.dilation), groups=deconv.groups,
                 out_channels=deconv.out_channels)
    want = dict(kernel_size=(4, 4), stride=(2, 2), padding=(1, 1), output_padding=(0, 0), dilation=(1, 1), groups=1,
                out_channels=COUT)
    bad = {k: v for k, v in found.items() if v != want[k]}
    if bad:
        raise RuntimeError(f"{what}: expected ConvTranspose2d(Cin, {COUT}, 4, stride=2, padding=1) with no output padding, "
                           "no dilation and one group, got " + ", ".join(f"{k}={v}" for k, v in bad.items()))
    _check_cin(what, deconv.in_channels)
    if bn.running_mean is None or tuple(bn.running_mean.shape) != (COUT,):
        raise RuntimeError(f"{what}: expected a BatchNorm2d({COUT}) with running statistics, got "
                           f"BatchNorm2d({bn.num_features}, track_running_stats={bn.track_running_stats})")


def fold_deconv_block(deconv, bn, device="cuda"):
    """``ConvTranspose2d(Cin, 256, 4, stride=2, padding=1)`` and the eval-mode ``BatchNorm2d`` behind it
    -> ``DeconvParams`` on ``device``: the weight rounded once to bf16 and packed
    (``pack_deconv4_weight``), BN and the deconv's bias (if any) folded in float64 and rounded once to
    f32.  Anything else raises and names what it found."""
    _check_deconv("fold_deconv_block", deconv, bn)
    s, shift = _bn_fold(deconv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, COUT)
    dev = torch.device(device)
    return DeconvParams(pack_deconv4_weight(_f64(deconv.weight)).to(dev), s.float().to(dev), shift.float().to(dev))


def _aligned(t):
    """``t`` contiguous at a 16-byte aligned address (torch's allocations are; a view at an odd offset is copied)."""
    t = t.contiguous()
    if _ops._tracing():                   # a traced tensor has no address; the recorded op gets fresh allocations
        return t
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _check_deconv_call(what, x_cl, p):
    """The input and parameter checks that ``deconv4s2`` and ``deconv4s2_project`` share."""
    if x_cl.dtype != torch.bfloat16:
        raise TypeError(f"{what}: x_cl must be bfloat16, got {x_cl.dtype}")
    if x_cl.dim() != 4:
        raise RuntimeError(f"{what}: x_cl must be (M, H, W, Cin), got {tuple(x_cl.shape)}")
    M, H, W, cin = x_cl.shape
    _check_cin(what, cin)
    if H < 1 or W < 1 or H * W > min(MAX_PIXELS, (2 ** 31 - 1) // (2 * cin)):
        raise RuntimeError(f"{what}: H and W must be at least 1 with one image below 2^31 bytes on both sides, got {H} x {W}")
    shape = (16, cin // 32, COUT // 16, 64, 8)
    if (tuple(p.packed.shape) != shape or p.packed.dtype != torch.bfloat16 or tuple(p.scale.shape) != (COUT,)
            or tuple(p.shift.shape) != (COUT,) or p.scale.dtype != torch.float32 or p.shift.dtype != torch.float32):
        raise RuntimeError(f"{what}: packed weights {shape}, scale and shift ({COUT},) must be what fold_deconv_block returns")


def deconv4s2(x_cl, params, out_layout="cl", out_dtype=None):
    """One launch of mvn_deconv4s2: x_cl (M, H, W, Cin) bfloat16 channels-last ->
    ``relu(bn(conv_transpose2d(x, w, stride=2, padding=1)))`` with ``params`` from ``fold_deconv_block``, as
    (M, 2H, 2W, 256) bfloat16 (``out_layout="cl"``, the next layer's input) or (M, 256, 2H, 2W) bfloat16 |
    float32 (``out_layout="nchw"``, ``out_dtype`` default bfloat16).  Cin is a multiple of 32 in
    [32, 2048].  bf16 operands, f32 accumulation, one rounding; the three outputs agree bit for bit
    (the f32 one after rounding).  GPU only; inference-only: under autograd use the modules themselves."""
    what = "deconv4s2"
    p = DeconvParams(*params)
    _inference_only(what, x_cl, *p, instead="the backbone's own deconv_layers, which autograd records")
    if out_layout not in ("cl", "nchw"):
        raise ValueError(f"{what}: out_layout must be 'cl' or 'nchw', got {out_layout!r}")
    out_dtype = torch.bfloat16 if out_dtype is None else out_dtype
    od = _dtype_code(out_dtype)
    if out_layout == "cl" and out_dtype != torch.bfloat16:
        raise TypeError(f"{what}: the channels-last output is bfloat16, got {out_dtype}")
    _check_deconv_call(what, x_cl, p)
    return _ops.call(_ops.deconv4s2, _aligned(x_cl), _aligned(p.packed), _aligned(p.scale), _aligned(p.shift),
                     out_layout == "nchw", od)


class ProjectionParams(NamedTuple):
    """What ``pack_projection`` returns: the packed bf16 hi | lo weight and the f32 bias."""
    packed: torch.Tensor
    bias: torch.Tensor


PROJ_SHAPE = (2, COUT // 32, FINAL_ROWS // 16, 64, 8)


def pack_projection(weight, bias=None, device="cuda"):
    """A ``Conv2d(256, 32, 1)`` weight, (32, 256) or (32, 256, 1, 1), and bias ((32,), None for zeros) ->
    ``ProjectionParams`` on ``device`` as mvn_deconv4s2_project reads them.  The float32 weight is split
    in float64 into two bfloat16 parts, ``hi = bf16(w)`` and ``lo = bf16(w - hi)`` (hi + lo is within
    2^-17 relative of w), packed (2, 8, 2, 64, 8):
    [part hi | lo][k][nt][lane][j] = part(w[16 nt + (lane & 15)][32 k + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)])."""
    if tuple(weight.shape) not in ((FINAL_ROWS, COUT), (FINAL_ROWS, COUT, 1, 1)):
        raise RuntimeError(f"pack_projection: weight must be ({FINAL_ROWS}, {COUT}) or ({FINAL_ROWS}, {COUT}, 1, 1), got "
                           f"{tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (FINAL_ROWS,):
        raise RuntimeError(f"pack_projection: bias must be ({FINAL_ROWS},), got {tuple(bias.shape)}")
    w = _f64(weight.detach().float()).reshape(FINAL_ROWS, COUT)
    hi = w.float().bfloat16()
    lo = (w - hi.double()).float().bfloat16()                    # the difference is exact in float64 and in float32
    parts = torch.stack((hi, lo)).reshape(2, FINAL_ROWS // 16, 16, COUT // 32, 2, 4, 4)   # [part][nt][n][k][j >> 2][g][j & 3]
    packed = parts.permute(0, 3, 1, 5, 2, 4, 6).reshape(PROJ_SHAPE).contiguous()          # [part][k][nt][g][n][j]
    dev = torch.device(device)
    b = torch.zeros(FINAL_ROWS) if bias is None else bias.detach().float().cpu().clone()
    return ProjectionParams(packed.to(dev), b.to(dev))


def deconv4s2_project(x_cl, params, proj, out_dtype=None):
    """One launch of mvn_deconv4s2_project: ``deconv4s2(x_cl, params, "nchw", bfloat16)`` followed by the
    256 -> 32 1x1 convolution of ``proj`` (``pack_projection``), without the 256-channel maps in between:
    x_cl (M, H, W, Cin) bfloat16 channels-last -> (M, 32, 2H, 2W) bfloat16 | float32 (``out_dtype``, default
    bfloat16).  The activation is what ``deconv4s2`` rounds to bfloat16, bit for bit; the projection is
    ``bias + sum a hi + sum a lo`` in f32 on the MFMA in one fixed order, rounded once for a bfloat16
    output.  The checks and errors of ``deconv4s2``.  GPU only; inference-only."""
    what = "deconv4s2_project"
    p, pr = DeconvParams(*params), ProjectionParams(*proj)
    _inference_only(what, x_cl, *p, *pr, instead="the backbone's own deconv_layers and the model's process_features, "
                    "which autograd records")
    out_dtype = torch.bfloat16 if out_dtype is None else out_dtype
    od = _dtype_code(out_dtype)
    _check_deconv_call(what, x_cl, p)
    if (tuple(pr.packed.shape) != PROJ_SHAPE or pr.packed.dtype != torch.bfloat16 or tuple(pr.bias.shape) != (FINAL_ROWS,)
            or pr.bias.dtype != torch.float32):
        raise RuntimeError(f"{what}: the packed projection {PROJ_SHAPE} and bias ({FINAL_ROWS},) must be what "
                           "pack_projection returns")
    return _ops.call(_ops.deconv4s2_project, _aligned(x_cl), _aligned(p.packed), _aligned(p.scale), _aligned(p.shift),
                     _aligned(pr.packed), _aligned(pr.bias), od)


def _final_layer_params(final_layer):
    """(weight (32, 256), bias (32,), J) of the reference's ``final_layer``, zero-padded to feature_conv's 32 rows."""
    what = "final_layer"
    if not isinstance(final_layer, nn.Conv2d):
        raise RuntimeError(f"{what}: expected a Conv2d({COUT}, J, 1), got {type(final_layer).__name__}")
    found = dict(kernel_size=tuple(final_layer.kernel_size), stride=tuple(final_layer.stride), padding=final_layer.padding,
                 dilation=tuple(final_layer.dilation), groups=final_layer.groups, in_channels=final_layer.in_channels)
    if isinstance(found["padding"], (tuple, list)):
        found["padding"] = tuple(found["padding"])
    want = dict(kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, in_channels=COUT)
    bad = {k: v for k, v in found.items() if v != want[k]}
    if bad:
        raise RuntimeError(f"{what}: expected Conv2d({COUT}, J, 1) with stride 1, padding 0, dilation 1 and one group, got "
                           + ", ".join(f"{k}={v}" for k, v in bad.items()))
    J = final_layer.out_channels
    if not 1 <= J <= FINAL_ROWS:
        raise RuntimeError(f"{what}: expected at most {FINAL_ROWS} joints, got out_channels={J}")
    w = torch.zeros(FINAL_ROWS, COUT)
    w[:J] = final_layer.weight.detach().float().cpu().reshape(J, COUT)
    b = torch.zeros(FINAL_ROWS)
    if final_layer.bias is not None:
        b[:J] = final_layer.bias.detach().float().cpu()
    return w, b, J


def _deconv_triples(deconv_layers):
    """The (ConvTranspose2d, BatchNorm2d, ReLU) triples of the reference's ``deconv_layers``."""
    what = "deconv_layers"
    if not isinstance(deconv_layers, nn.Sequential) or len(deconv_layers) == 0 or len(deconv_layers) % 3 != 0:
        n = f" of {len(deconv_layers)} modules" if isinstance(deconv_layers, nn.Sequential) else ""
        raise RuntimeError(f"{what}: expected a Sequential of (ConvTranspose2d, BatchNorm2d, ReLU) triples, got "
                           f"{type(deconv_layers).__name__}{n}")
    mods = list(deconv_layers)
    triples = [tuple(mods[i:i + 3]) for i in range(0, len(mods), 3)]
    for i, (d, b, r) in enumerate(triples):
        names = tuple(type(m).__name__ for m in (d, b, r))
        if not (isinstance(d, nn.ConvTranspose2d) and isinstance(b, nn.BatchNorm2d) and isinstance(r, nn.ReLU)):
            raise RuntimeError(f"{what}[{3 * i}:{3 * i + 3}]: expected (ConvTranspose2d, BatchNorm2d, ReLU), got {names}")
        _check_deconv(f"{what}[{3 * i}]", d, b)
        if i > 0 and d.in_channels != COUT:
            raise RuntimeError(f"{what}[{3 * i}]: expected {COUT} input channels behind a {COUT}-channel layer, got "
                               f"in_channels={d.in_channels}")
    return triples


def _no_heatmaps_with_project(heatmaps):
    if heatmaps:
        raise RuntimeError("DeconvHeadEval: project and heatmaps=True exclude each other: with the projection in the "
                           "last layer's launch the 256-channel map is not formed, so final_layer has nothing to read; "
                           "pass heatmaps=False, or keep the unfused head")


class DeconvHeadEval(nn.Module):
    """``deconv_layers`` and ``final_layer`` of the reference's ``PoseResNet`` (pose_resnet.py:312-316),
    eval mode: ``module(x)`` takes ``layer4``'s output (M, Cin, h, w), float32 or bfloat16 in any memory
    format, and returns ``(heatmaps (M, J, 8h, 8w) float32 or None, features (M, 256, 8h, 8w) in
    feature_dtype)`` for the usual three layers.

    1. the input as channels-last bfloat16: one cast-and-permute pass over this small tensor (a
       view when the trunk already runs bfloat16 channels_last), the only torch pass;
    2. one ``deconv4s2`` launch per layer, all but the last channels-last, the last NCHW in
       ``feature_dtype``;
    3. ``heatmaps``: ``model.feature_conv`` with ``final_layer``'s weight and bias zero-padded to 32 rows,
       sliced to the J joints and made contiguous (``heatmaps=False``: skipped, None returned).

    With ``project`` (a ``ProjectionParams``; ``from_reference(..., process_features=)`` packs the
    volumetric model's), the last layer runs ``deconv4s2_project`` and the module returns ``(None,
    features32 (M, 32, 8h, 8w) in feature_dtype)``: what ``model.feature_conv`` makes of the 256-channel
    maps, which are not formed.  ``heatmaps`` must then be False.

    Every layer runs on the kernel: none of them is slower there than in torch.  The
    parameters are copied: later changes to the backbone do not reach this module."""

    def __init__(self, params, final_weight, final_bias, joints, feature_dtype=torch.bfloat16, heatmaps=True,
                 project=None):
        super().__init__()
        _dtype_code(feature_dtype)
        if project is not None:
            _no_heatmaps_with_project(heatmaps)
        self.n_layers = len(params)
        for i, p in enumerate(params):
            p = DeconvParams(*p)
            self.register_buffer(f"packed{i}", p.packed)
            self.register_buffer(f"scale{i}", p.scale)
            self.register_buffer(f"shift{i}", p.shift)
        self.register_buffer("final_weight", final_weight)
        self.register_buffer("final_bias", final_bias)
        self.joints = int(joints)
        self.feature_dtype = feature_dtype
        self.heatmaps = bool(heatmaps)
        self.project = project is not None
        if self.project:
            project = ProjectionParams(*project)
            self.register_buffer("proj_packed", project.packed)
            self.register_buffer("proj_bias", project.bias)

    @classmethod
    def from_reference(cls, backbone, device="cuda", feature_dtype=torch.bfloat16, heatmaps=True,
                       process_features=None):
        """``backbone.deconv_layers`` (a Sequential of (ConvTranspose2d, BatchNorm2d, ReLU) triples, each
        k = 4, stride 2, padding 1, no output padding, no dilation, one group, 256 outputs) and
        ``backbone.final_layer`` (a Conv2d(256, J, 1), J <= 32); anything else raises and names what it
        found.  ``process_features``: the volumetric model's ``Sequential`` of one ``Conv2d(256, 32, 1)``
        (validated as ``VolumetricEval.from_reference`` does), run inside the last layer's launch."""
        project = None
        if process_features is not None:
            _no_heatmaps_with_project(heatmaps)
            pw, pb = _feature_conv_params(process_features)
            if pw.shape[1] != COUT:
                raise RuntimeError(f"process_features: expected Conv2d({COUT}, {FINAL_ROWS}, 1) behind the {COUT}-channel "
                                   f"head, got in_channels={pw.shape[1]}")
            project = pack_projection(pw, pb, device=device)
        triples = _deconv_triples(backbone.deconv_layers)
        w, b, J = _final_layer_params(backbone.final_layer)
        dev = torch.device(device)
        params = [fold_deconv_block(d, bn, device=dev) for d, bn, _ in triples]
        return cls(params, w.to(dev), b.to(dev), J, feature_dtype, heatmaps, project)

    def layer_params(self, i):
        return DeconvParams(getattr(self, f"packed{i}"), getattr(self, f"scale{i}"), getattr(self, f"shift{i}"))

    def forward(self, x):
        _inference_only("DeconvHeadEval", x, instead="the backbone's own modules, which autograd records")
        if x.dim() != 4:
            raise RuntimeError(f"DeconvHeadEval: x must be (M, Cin, h, w), got {tuple(x.shape)}")
        _dtype_code(x.dtype)
        h = x.permute(0, 2, 3, 1)
        if h.dtype != torch.bfloat16 or not h.is_contiguous():
            h = torch.empty(h.shape, dtype=torch.bfloat16, device=x.device).copy_(h)   # the one cast-and-permute pass
        last = self.n_layers - 1
        for i in range(self.n_layers):
            if i == last and self.project:
                h = deconv4s2_project(h, self.layer_params(i), (self.proj_packed, self.proj_bias), self.feature_dtype)
            elif i == last:
                h = deconv4s2(h, self.layer_params(i), "nchw", self.feature_dtype)
            else:
                h = deconv4s2(h, self.layer_params(i), "cl")
        heatmaps = None
        if self.heatmaps:
            heatmaps = feature_conv(h, self.final_weight, self.final_bias, out_dtype=torch.float32)[:, :self.joints]
            heatmaps = heatmaps.contiguous()
        return heatmaps, h


_TRUNK = ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4")


class BackboneEval(nn.Module):
    """The reference's ``PoseResNet.forward`` (pose_resnet.py:293-318), eval mode: its own trunk modules
    ``conv1`` ... ``layer4`` and optional ``alg_confidences`` / ``vol_confidences`` heads, kept as they are
    (or replaced on request: ``from_reference``) and called in the reference's order, then
    ``DeconvHeadEval``.  Returns the reference's 4-tuple
    ``(heatmaps, features, alg_confidences, vol_confidences)``, None where the backbone has no such
    head (or ``heatmaps=False``); with ``process_features`` (``DeconvHeadEval``) the features are the
    model's 32-channel ones.  The module adds no arithmetic of its own.  The trunk modules are
    the backbone's own objects (not copies) and must live on the device of the input; call under
    ``torch.no_grad()``."""

    def __init__(self, trunk, head, alg_confidences=None, vol_confidences=None, cast_for_confidences=False):
        super().__init__()
        self.trunk = trunk
        self.head = head
        self.alg_confidences = alg_confidences
        self.vol_confidences = vol_confidences
        self.cast_for_confidences = bool(cast_for_confidences)

    @classmethod
    def from_reference(cls, backbone, device="cuda", feature_dtype=torch.bfloat16, heatmaps=True,
                       process_features=None, trunk="torch", stem="torch", confidences="torch"):
        """``trunk="torch"`` (the default) keeps the backbone's own ``conv1`` ... ``layer4``; ``trunk="kernels"``
        runs ``layer1`` .. ``layer4`` through ``resnet.TrunkEval``, whose bfloat16
        channels-last output the head reads without a copy and the confidence heads, while they stay torch
        modules, get cast to their parameters' dtype.  ``stem`` is passed on to ``TrunkEval``: ``"kernels"``
        runs ``conv1, bn1, relu, maxpool`` as one launch too and needs ``trunk="kernels"``.
        ``confidences="torch"`` (the default) keeps the backbone's own ``alg_confidences`` and
        ``vol_confidences`` objects; ``"kernels"`` replaces each head the backbone has with a
        ``confidence.ConfidenceHeadEval``, which reads the kernel trunk's output as it is
        (no float32 cast is made then) and takes one cast-and-permute pass behind the torch trunk."""
        if trunk not in ("torch", "kernels"):
            raise ValueError(f"BackboneEval: trunk must be 'torch' or 'kernels', got {trunk!r}")
        if stem not in ("torch", "kernels"):
            raise ValueError(f"BackboneEval: stem must be 'torch' or 'kernels', got {stem!r}")
        if confidences not in ("torch", "kernels"):
            raise ValueError(f"BackboneEval: confidences must be 'torch' or 'kernels', got {confidences!r}")
        if stem == "kernels" and trunk != "kernels":
            raise ValueError("BackboneEval: stem='kernels' needs trunk='kernels': the kernel stem writes channels-last "
                             f"bfloat16 for TrunkEval, got trunk={trunk!r}")
        missing = [n for n in _TRUNK if not isinstance(getattr(backbone, n, None), nn.Module)]
        if missing:
            raise RuntimeError(f"BackboneEval: expected the trunk modules {', '.join(_TRUNK)}; {type(backbone).__name__} "
                               f"has no {', '.join(missing)}")
        if trunk == "kernels":
            from .resnet import TrunkEval
            trunk_module = TrunkEval.from_reference(backbone, device=device, stem=stem)
        else:
            trunk_module = nn.Sequential(*(getattr(backbone, n) for n in _TRUNK))
        head = DeconvHeadEval.from_reference(backbone, device, feature_dtype, heatmaps, process_features)
        alg, vol = getattr(backbone, "alg_confidences", None), getattr(backbone, "vol_confidences", None)
        if confidences == "kernels":
            from .confidence import ConfidenceHeadEval
            try:
                alg, vol = (None if h is None else ConfidenceHeadEval.from_reference(h, device=device) for h in (alg, vol))
            except RuntimeError as e:
                raise RuntimeError(f"BackboneEval: {e}") from None
        return cls(trunk_module, head, alg, vol,
                   cast_for_confidences=trunk == "kernels" and confidences == "torch")

    def forward(self, x):
        _inference_only("BackboneEval", x, instead="the backbone itself, which autograd records")
        x = self.trunk(x)
        xc = x
        if self.cast_for_confidences:     # one cast of the kernels' bfloat16 output for both heads
            heads = [h for h in (self.alg_confidences, self.vol_confidences) if h is not None]
            p = next((p for h in heads for p in h.parameters()), None)
            if p is not None and p.dtype != x.dtype:
                xc = x.to(p.dtype)
        alg = self.alg_confidences(xc) if self.alg_confidences is not None else None
        vol = self.vol_confidences(xc) if self.vol_confidences is not None else None
        heatmaps, features = self.head(x)
        return heatmaps, features, alg, vol
