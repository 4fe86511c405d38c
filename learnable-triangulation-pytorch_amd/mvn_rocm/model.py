"""The volumetric model after the backbone (mvn/models/triangulation.py:343-353) on this package's
kernels: ``process_features``, a ``Conv2d(256, 32, 1)``, as ``feature_conv``
(csrc/feature_conv.hip), and ``VolumetricEval``, the one call from the backbone's
feature maps to the joints: ``feature_conv``, ``v2v.unproject_channels_last`` and ``v2v.V2VEval``,
composed and nothing else.  ``VolumetricModelEval`` puts ``backbone.BackboneEval`` in front of it:
images to joints, with ``process_features`` optionally inside the head's last launch.
``AlgebraicModelEval`` is the algebraic model (triangulation.py:149-200) in one call: ``BackboneEval`` and
``multiview.triangulate_from_heatmaps``.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _ops
from .op import _dtype_code
from .v2v import V2VEval, _inference_only, unproject_channels_last

COUT = _ops.FEATURE_COUT
MIN_CIN, MAX_CIN = 32, 512
FUSED_DEFAULT = True          # VolumetricModelEval: the fused launch won every row of DESIGN.md §4.17


def _check_cin(what, cin):
    if cin % 32 != 0 or not MIN_CIN <= cin <= MAX_CIN:
        raise RuntimeError(f"{what}: the input channels must be a multiple of 32 in [{MIN_CIN}, {MAX_CIN}], got {cin}")


def feature_conv(x, weight, bias=None, out_dtype=None):
    """``F.conv2d(x, weight, bias)`` for a 1x1 convolution to 32 channels (mvn_feature_conv): x
    (M, Cin, H, W) or (B, N, Cin, H, W), float32 or bfloat16 -> the same leading dimensions with 32
    channels, in ``out_dtype`` (float32 | bfloat16, default ``x.dtype``).  ``weight`` is (32, Cin) or
    (32, Cin, 1, 1), ``bias`` (32,) or None for zeros; Cin is a multiple of 32 in [32, 512].

    The arithmetic is one f32 chain whatever the dtypes: ``acc = bias[co]``, then ``acc =
    fma(weight[co, ci], x[ci], acc)`` for ci ascending; a bfloat16 result is ``acc`` rounded to
    nearest-even, so ``out_dtype=torch.bfloat16`` equals ``feature_conv(...).to(torch.bfloat16)`` of the
    float32 result without its pass over the maps.  A non-contiguous ``x`` is copied.  GPU only;
    inference-only: under autograd use ``torch.nn.functional.conv2d``."""
    what = "feature_conv"
    _inference_only(what, x, weight, bias, instead="torch.nn.functional.conv2d, which autograd records")
    _dtype_code(x.dtype)
    od = _dtype_code(out_dtype if out_dtype is not None else x.dtype)
    if x.dim() not in (4, 5):
        raise RuntimeError(f"{what}: x must be (M, Cin, H, W) or (B, N, Cin, H, W), got {tuple(x.shape)}")
    cin, H, W = x.shape[-3:]
    _check_cin(what, cin)
    if tuple(weight.shape) not in ((COUT, cin), (COUT, cin, 1, 1)):
        raise RuntimeError(f"{what}: weight must be ({COUT}, {cin}) or ({COUT}, {cin}, 1, 1), got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (COUT,):
        raise RuntimeError(f"{what}: bias must be ({COUT},), got {tuple(bias.shape)}")
    w = _ops.f32c(weight.reshape(COUT, cin))
    b = _ops.f32c(bias) if bias is not None else None
    lead = x.shape[:-3]
    out = _ops.call(_ops.feature_conv, x.contiguous().view(math.prod(lead), cin, H, W), w, b, od)
    return out.view(*lead, COUT, H, W)


def _feature_conv_params(process_features):
    """(weight (32, Cin), bias or None) of the reference's ``process_features``: a ``Sequential`` of
    exactly one ``Conv2d`` that ``feature_conv`` computes; anything else raises naming what it is."""
    what = "process_features"
    if not isinstance(process_features, nn.Sequential) or len(process_features) != 1:
        n = f" of {len(process_features)} modules" if isinstance(process_features, nn.Sequential) else ""
        raise RuntimeError(f"{what}: expected a Sequential of exactly one Conv2d, got {type(process_features).__name__}{n}")
    conv = process_features[0]
    if not isinstance(conv, nn.Conv2d):
        raise RuntimeError(f"{what}: expected a Sequential of exactly one Conv2d, got one {type(conv).__name__}")
    found = dict(kernel_size=tuple(conv.kernel_size), stride=tuple(conv.stride), padding=conv.padding,
                 dilation=tuple(conv.dilation), groups=conv.groups, out_channels=conv.out_channels)
    want = dict(kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, out_channels=COUT)
    if isinstance(found["padding"], (tuple, list)):
        found["padding"] = tuple(found["padding"])
    bad = {k: v for k, v in found.items() if v != want[k]}
    if bad:
        raise RuntimeError(f"{what}: expected Conv2d(Cin, {COUT}, 1) with stride 1, padding 0, dilation 1 and one group, got "
                           + ", ".join(f"{k}={v}" for k, v in bad.items()))
    _check_cin(what, conv.in_channels)
    return conv.weight.detach().reshape(COUT, conv.in_channels), (conv.bias.detach() if conv.bias is not None else None)


class VolumetricEval(nn.Module):
    """``VolumetricTriangulationNet.forward`` (triangulation.py:245-355) from the backbone's outputs to
    the joints, eval mode, on this package's kernels:

    1. 'conf_norm' only: ``vol_confidences / vol_confidences.sum(dim=1, keepdim=True)``
       (triangulation.py:268-269), the reference's own torch expression on B*N*32 numbers;
    2. ``feature_conv`` into ``feature_dtype`` (process_features, :344-346);
    3. ``v2v.unproject_channels_last`` into a bfloat16 channels-last volume (:349);
    4. ``v2v.V2VEval`` with the model's ``volume_multiplier`` and ``volume_softmax`` (:352-353).

    The module adds no arithmetic of its own.  ``VolumetricEval.from_reference(model)`` once, then
    ``module(features, proj_matricies, coord_volumes, vol_confidences)`` per batch.  Inference-only."""

    def __init__(self, weight, bias, v2v, volume_aggregation_method="softmax", volume_multiplier=1.0,
                 volume_softmax=True, feature_dtype=torch.bfloat16, precision=None):
        super().__init__()
        _dtype_code(feature_dtype)
        self.register_buffer("weight", weight)
        self.register_buffer("bias", bias)
        self.v2v = v2v
        self.volume_aggregation_method = volume_aggregation_method
        self.volume_multiplier = float(volume_multiplier)
        self.volume_softmax = bool(volume_softmax)
        self.feature_dtype = feature_dtype
        self.precision = precision

    @classmethod
    def from_reference(cls, model, device="cuda", feature_dtype=torch.bfloat16, half_res="kernels", deep="kernels",
                       precision=None):
        """``model.process_features`` (a missing bias means zeros), ``model.volume_net`` through
        ``V2VEval.from_reference`` with ``half_res`` and ``deep``, and the model's
        ``volume_aggregation_method``, ``volume_multiplier`` and ``volume_softmax``.  The parameters are
        copied: later changes to ``model`` do not reach this module."""
        weight, bias = _feature_conv_params(model.process_features)
        dev = torch.device(device)
        return cls(weight.float().contiguous().clone().to(dev), bias.float().clone().to(dev) if bias is not None else None,
                   V2VEval.from_reference(model.volume_net, device=device, half_res=half_res, deep=deep),
                   model.volume_aggregation_method, model.volume_multiplier, model.volume_softmax, feature_dtype,
                   precision)

    def forward(self, features, proj_matricies, coord_volumes, vol_confidences=None):
        """features (B, N, Cin, H, W), proj_matricies (B, N, 3, 4), coord_volumes (B, V, V, V, 3) or a
        ``volumetric.Cuboids``, vol_confidences (B, N, 32) for 'conf*' aggregation ->
        (vol_keypoints_3d (B, J, 3), features (B, N, 32, H, W) in ``feature_dtype``, volumes
        (B, J, V, V, V), vol_confidences as the unprojection read them), the first four of the
        reference's return values."""
        _inference_only("VolumetricEval", features, vol_confidences,
                        instead="the model's own modules, which autograd records")
        if features.dim() != 5:
            raise RuntimeError(f"VolumetricEval: features must be (B, N, Cin, H, W), got {tuple(features.shape)}")
        if self.volume_aggregation_method == "conf_norm" and vol_confidences is None:
            raise TypeError("volume_aggregation_method 'conf_norm' needs vol_confidences")      # before any launch
        features = feature_conv(features, self.weight, self.bias, out_dtype=self.feature_dtype)
        return self.from_projected(features, proj_matricies, coord_volumes, vol_confidences)

    def from_projected(self, features32, proj_matricies, coord_volumes, vol_confidences=None):
        """Everything of ``forward`` behind ``feature_conv``: features32 (B, N, 32, H, W), already through
        ``process_features`` (``feature_conv``, or the head's ``deconv4s2_project``), and the other
        arguments and the four return values of ``forward``."""
        _inference_only("VolumetricEval", features32, vol_confidences,
                        instead="the model's own modules, which autograd records")
        if features32.dim() != 5 or features32.shape[2] != COUT:
            raise RuntimeError(f"VolumetricEval: features32 must be (B, N, {COUT}, H, W), got {tuple(features32.shape)}")
        features = features32
        method = self.volume_aggregation_method
        if method == "conf_norm":
            if vol_confidences is None:
                raise TypeError("volume_aggregation_method 'conf_norm' needs vol_confidences")
            vol_confidences = vol_confidences / vol_confidences.sum(dim=1, keepdim=True)
        volumes = unproject_channels_last(features, proj_matricies, coord_volumes, method, out_dtype=torch.bfloat16,
                                          vol_confidences=vol_confidences, precision=self.precision)
        vol_keypoints_3d, volumes = self.v2v(volumes, coord_volumes, self.volume_multiplier, self.volume_softmax)
        return vol_keypoints_3d, features, volumes, vol_confidences


class VolumetricModelEval(nn.Module):
    """``VolumetricTriangulationNet.forward`` (triangulation.py:245-355) from the images to the joints,
    eval mode: ``backbone.BackboneEval`` over ``model.backbone`` on the images as (B * N, 3, H, W), then

    - ``fused=True``: the head's last layer ran ``process_features`` in its own launch
      (``deconv4s2_project``), and ``VolumetricEval.from_projected`` takes the 32-channel features;
    - ``fused=False``: ``VolumetricEval.forward`` on the 256-channel features.

    ``module(images (B, N, 3, H, W), proj_matricies (B, N, 3, 4), coord_volumes (B, V, V, V, 3) or a
    volumetric.Cuboids)`` returns ``VolumetricEval``'s four values.  The projection matrices are the
    caller's, already at the feature maps' resolution (triangulation.py:271-278).  The module adds no
    arithmetic of its own; the backbone's heatmaps are not computed.  Inference-only."""

    def __init__(self, backbone, volumetric, fused):
        super().__init__()
        self.backbone = backbone
        self.volumetric = volumetric
        self.fused = bool(fused)

    @classmethod
    def from_reference(cls, model, device="cuda", feature_dtype=torch.bfloat16, half_res="kernels", deep="kernels",
                       precision=None, fused=FUSED_DEFAULT, trunk="torch", stem="torch", confidences="torch"):
        """``model.backbone`` through ``BackboneEval.from_reference`` (``heatmaps=False``; with ``fused`` it
        is given ``model.process_features``; ``trunk`` is passed on: ``"kernels"`` runs the ResNet stages on
        ``resnet.TrunkEval``, DESIGN.md §4.18, and with it ``stem="kernels"`` the stem in one launch, §4.19;
        ``confidences="kernels"`` runs the confidence heads on ``confidence.ConfidenceHeadEval``, §4.20)
        and the rest of ``model`` through ``VolumetricEval.from_reference``.  ``fused`` defaults to what was measured faster (DESIGN.md
        §4.17)."""
        from .backbone import BackboneEval
        vol = VolumetricEval.from_reference(model, device, feature_dtype, half_res, deep, precision)
        bb = BackboneEval.from_reference(model.backbone, device, feature_dtype, heatmaps=False,
                                         process_features=model.process_features if fused else None, trunk=trunk,
                                         stem=stem, confidences=confidences)
        return cls(bb, vol, fused)

    def forward(self, images, proj_matricies, coord_volumes):
        _inference_only("VolumetricModelEval", images, instead="the model itself, which autograd records")
        if images.dim() != 5:
            raise RuntimeError(f"VolumetricModelEval: images must be (B, N, 3, H, W), got {tuple(images.shape)}")
        B, N = images.shape[:2]
        _, features, _, vol_confidences = self.backbone(images.reshape(B * N, *images.shape[2:]))
        features = features.view(B, N, *features.shape[1:])
        if vol_confidences is not None:
            vol_confidences = vol_confidences.view(B, N, *vol_confidences.shape[1:])
        run = self.volumetric.from_projected if self.fused else self.volumetric
        return run(features, proj_matricies, coord_volumes, vol_confidences)


class AlgebraicModelEval(nn.Module):
    """``AlgebraicTriangulationNet.forward`` (triangulation.py:149-200) from the images to the joints, eval
    mode: ``backbone.BackboneEval`` (``heatmaps=True``) over ``model.backbone`` on the images as
    (B * N, 3, H, W), then ``multiview.triangulate_from_heatmaps`` on its heatmaps with the model's
    ``heatmap_multiplier`` and ``heatmap_softmax``, the images' (H, W) as ``image_shape`` and, with
    ``use_confidences``, the backbone's ``alg_confidences`` (without: None, the reference's all ones).

    ``module(images (B, N, 3, H, W), proj_matricies (B, N, 3, 4))`` returns the reference's 4-tuple:
    keypoints_3d (B, J, 3), keypoints_2d (B, N, J, 2) in image pixels, the normalised heatmaps
    (B, N, J, h, w) and the normalised confidences (B, N, J).  The module adds no arithmetic of its own.
    Inference-only."""

    def __init__(self, backbone, use_confidences, heatmap_softmax, heatmap_multiplier):
        super().__init__()
        if use_confidences and getattr(backbone, "alg_confidences", None) is None:
            raise RuntimeError("AlgebraicModelEval: use_confidences needs a backbone with an alg_confidences head, "
                               "got alg_confidences=None")
        self.backbone = backbone
        self.use_confidences = bool(use_confidences)
        self.heatmap_softmax = bool(heatmap_softmax)
        self.heatmap_multiplier = float(heatmap_multiplier)

    @classmethod
    def from_reference(cls, model, device="cuda", feature_dtype=torch.bfloat16, trunk="torch", stem="torch",
                       confidences="torch"):
        """``model.backbone`` through ``BackboneEval.from_reference`` with ``trunk``, ``stem`` and
        ``confidences`` passed on, and the model's ``use_confidences``,
        ``heatmap_softmax`` and ``heatmap_multiplier``.  ``use_confidences`` with a backbone that has no
        ``alg_confidences`` raises."""
        from .backbone import BackboneEval
        if model.use_confidences and getattr(model.backbone, "alg_confidences", None) is None:
            raise RuntimeError("AlgebraicModelEval: use_confidences needs a backbone with an alg_confidences head, "
                               f"{type(model.backbone).__name__} has none")
        bb = BackboneEval.from_reference(model.backbone, device, feature_dtype, heatmaps=True, trunk=trunk, stem=stem,
                                         confidences=confidences)
        return cls(bb, model.use_confidences, model.heatmap_softmax, model.heatmap_multiplier)

    def forward(self, images, proj_matricies):
        from .multiview import triangulate_from_heatmaps
        _inference_only("AlgebraicModelEval", images, instead="the model itself, which autograd records")
        if images.dim() != 5:
            raise RuntimeError(f"AlgebraicModelEval: images must be (B, N, 3, H, W), got {tuple(images.shape)}")
        B, N = images.shape[:2]
        heatmaps, _, alg_confidences, _ = self.backbone(images.reshape(B * N, *images.shape[2:]))
        return triangulate_from_heatmaps(heatmaps, proj_matricies, alg_confidences if self.use_confidences else None,
                                         image_shape=tuple(images.shape[3:]), heatmap_multiplier=self.heatmap_multiplier,
                                         heatmap_softmax=self.heatmap_softmax)
