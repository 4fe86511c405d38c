"""The 2-D backbone's ResNet trunk on this package's kernels (mvn/models/pose_resnet.py:57-95, 236-251,
293-310): ``layer1`` .. ``layer4`` of the reference's ``PoseResNet`` are ``Bottleneck``
blocks, each three convolutions with a BatchNorm behind them, a residual (the input itself, or a strided
1x1 ``downsample``) and ReLUs.  A block runs as three launches on bf16 channels-last tensors
(csrc/bottleneck.hip, bf16 MFMA, f32 accumulation, one rounding per convolution):

    conv1x1 (conv1 + bn1 + relu) -> conv3x3 (conv2 + bn2 + relu, the block's stride)
    -> conv1x1 (conv3 + bn3 + the residual + relu; the downsample runs inside this launch)

``TrunkEval`` is the whole trunk: by default the stem (``conv1, bn1, relu, maxpool``) stays the backbone's
own torch modules, one cast-and-permute pass makes its output channels-last bfloat16, and the four stages
run on the kernels.  With ``stem="kernels"`` the stem and that pass are one launch as well (csrc/stem.hip,
``StemEval``).  Eval mode, inference-only.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _lib, _ops
from .v2v import _bn_fold, _f64, _inference_only, _pack_mfma_a

MIN_C, MAX_C1, MAX_C3 = 64, 2048, 512
MAX_BYTES = 2 ** 31 - 1                   # of one tensor: one buffer resource


class ConvParams(NamedTuple):
    """One folded convolution: packed bf16 weights and f32 scale / shift."""
    packed: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


class BottleneckParams(NamedTuple):
    """What ``fold_bottleneck`` returns: the three folded convolutions, the folded ``downsample`` (None for
    the identity residual) and the block's stride (that of ``conv2`` and of the downsample)."""
    conv1: ConvParams
    conv2: ConvParams
    conv3: ConvParams
    downsample: Optional[ConvParams]
    stride: int


def _check_c(what, name, c, max_c):
    if c % 64 != 0 or not MIN_C <= c <= max_c:
        raise RuntimeError(f"{what}: {name} must be a multiple of 64 in [{MIN_C}, {max_c}], got {c}")


def pack_conv1x1_weight(w):
    """(cout, cin) or (cout, cin, 1, 1) float64 Conv2d weight -> (cin / 32, cout / 16, 64, 8) bf16 as mvn_conv1x1
    reads it: [kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]."""
    if not (w.dim() == 2 or (w.dim() == 4 and tuple(w.shape[2:]) == (1, 1))):
        raise RuntimeError(f"expected a (Cout, Cin) or (Cout, Cin, 1, 1) Conv2d weight, got {tuple(w.shape)}")
    cout, cin = w.shape[:2]
    _check_c("pack_conv1x1_weight", "Cin", cin, MAX_C1)
    _check_c("pack_conv1x1_weight", "Cout", cout, MAX_C1)
    return _pack_mfma_a(w.reshape(cout, cin))


def pack_conv3x3_weight(w):
    """(C, C, 3, 3) float64 Conv2d weight -> (9, C / 32, C / 16, 64, 8) bf16 as mvn_conv3x3 reads it:
    [tap = ky*3 + kx][kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != w.shape[1]:
        raise RuntimeError(f"expected a (C, C, 3, 3) Conv2d weight, got {tuple(w.shape)}")
    C = w.shape[0]
    _check_c("pack_conv3x3_weight", "C", C, MAX_C3)
    return _pack_mfma_a(w.permute(2, 3, 0, 1).reshape(9, C, C))


STEM_CIN, STEM_COUT, STEM_K = 3, 64, 7
STEM_ROW_SLOTS, STEM_K_SLOTS = 24, 192    # K-slots of a tap row (21 real) and of the whole packed K axis (168 real)


def pack_stem_weight(w):
    """(64, 3, 7, 7) float64 Conv2d weight -> (6, 4, 64, 8) bf16 as mvn_stem reads it:
    [kp][m][lane][j] = A[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j] with A (64, 192),
    A[co][24 ky + 3 kx + ci] = w[co][ci][ky][kx] and zero in every other slot (24 ky + 21 .. 24 ky + 23 and
    168 .. 191)."""
    if w.dim() != 4 or tuple(w.shape) != (STEM_COUT, STEM_CIN, STEM_K, STEM_K):
        raise RuntimeError(f"expected a ({STEM_COUT}, {STEM_CIN}, {STEM_K}, {STEM_K}) Conv2d weight, got {tuple(w.shape)}")
    rows = w.permute(0, 2, 3, 1).reshape(STEM_COUT, STEM_K, STEM_K * STEM_CIN)           # [co][ky][3 kx + ci]
    rows = nn.functional.pad(rows, (0, STEM_ROW_SLOTS - STEM_K * STEM_CIN)).reshape(STEM_COUT, STEM_K * STEM_ROW_SLOTS)
    return _pack_mfma_a(nn.functional.pad(rows, (0, STEM_K_SLOTS - STEM_K * STEM_ROW_SLOTS)))


# ----------------------------------------------------------------------------- the fold
def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _check_conv_bn(what, conv, bn, k, pad, strides):
    """``conv`` is a Conv2d(k, padding pad, stride in strides, no dilation, one group) with a BatchNorm2d with
    running statistics behind it, or a RuntimeError naming what it is instead.  Returns the stride."""
    if not isinstance(conv, nn.Conv2d):
        raise RuntimeError(f"{what}: expected a Conv2d, got {type(conv).__name__}")
    if not isinstance(bn, nn.BatchNorm2d):
        raise RuntimeError(f"{what}: expected a BatchNorm2d behind the Conv2d, got {type(bn).__name__}")
    found = dict(kernel_size=_pair(conv.kernel_size), padding=conv.padding if isinstance(conv.padding, str)
                 else _pair(conv.padding), dilation=_pair(conv.dilation), groups=conv.groups)
    want = dict(kernel_size=(k, k), padding=(pad, pad), dilation=(1, 1), groups=1)
    bad = {n: v for n, v in found.items() if v != want[n]}
    stride = _pair(conv.stride)
    if stride not in [(s, s) for s in strides]:
        bad["stride"] = stride
    if bad:
        raise RuntimeError(f"{what}: expected Conv2d(k={k}, padding={pad}, stride in {tuple(strides)}) with no dilation and "
                           "one group, got " + ", ".join(f"{n}={v}" for n, v in bad.items()))
    if bn.running_mean is None or bn.running_var is None or tuple(bn.running_mean.shape) != (conv.out_channels,):
        raise RuntimeError(f"{what}: expected a BatchNorm2d({conv.out_channels}) with running statistics, got "
                           f"BatchNorm2d({bn.num_features}, track_running_stats={bn.track_running_stats})")
    return stride[0]


def _fold_conv(conv, bn, pack, dev):
    s, shift = _bn_fold(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, conv.out_channels)
    return ConvParams(pack(_f64(conv.weight)).to(dev), s.float().to(dev), shift.float().to(dev))


_BLOCK_ATTRS = ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3")


def fold_bottleneck(block, device="cuda"):
    """The reference's eval-mode ``Bottleneck`` (attributes ``conv1/bn1/conv2/bn2/conv3/bn3/downsample/stride``:
    1x1, 3x3 with padding 1 carrying the stride, 1x1; ``downsample`` None or a Sequential of a 1x1 Conv2d
    with the block's stride and a BatchNorm2d) -> ``BottleneckParams`` on ``device``.  Weights are rounded
    once to bf16 and packed; each BatchNorm (and conv bias, if any) is folded in float64 and rounded once
    to f32.  A ``Bottleneck_CAFFE`` (stride on ``conv1``), a ``BasicBlock`` (no ``conv3``), dilation, groups
    or a BatchNorm without running statistics raises a RuntimeError naming what was found."""
    what = "fold_bottleneck"
    missing = [n for n in _BLOCK_ATTRS if not isinstance(getattr(block, n, None), nn.Module)]
    if missing or not hasattr(block, "downsample") or not hasattr(block, "stride"):
        missing += [n for n in ("downsample", "stride") if not hasattr(block, n)]
        raise RuntimeError(f"{what}: expected a Bottleneck with {', '.join(_BLOCK_ATTRS)}, downsample and stride; "
                           f"{type(block).__name__} has no {', '.join(missing)}")
    _check_conv_bn(f"{what}: conv1", block.conv1, block.bn1, 1, 0, (1,))
    stride = _check_conv_bn(f"{what}: conv2", block.conv2, block.bn2, 3, 1, (1, 2))
    _check_conv_bn(f"{what}: conv3", block.conv3, block.bn3, 1, 0, (1,))
    if _pair(block.stride) != (stride, stride):
        raise RuntimeError(f"{what}: expected the block's stride on conv2, got stride={block.stride} with "
                           f"conv2.stride={_pair(block.conv2.stride)}")
    cin, mid, cout = block.conv1.in_channels, block.conv1.out_channels, block.conv3.out_channels
    if (block.conv2.in_channels, block.conv2.out_channels, block.conv3.in_channels) != (mid, mid, mid):
        raise RuntimeError(f"{what}: expected conv2 and conv3 to take conv1's {mid} channels, got conv2 "
                           f"{block.conv2.in_channels} -> {block.conv2.out_channels} and conv3.in_channels="
                           f"{block.conv3.in_channels}")
    _check_c(what, "conv1.in_channels", cin, MAX_C1)
    _check_c(what, "conv2's channels", mid, MAX_C3)
    _check_c(what, "conv3.out_channels", cout, MAX_C1)
    dev = torch.device(device)
    ds = block.downsample
    down = None
    if ds is None:
        if stride != 1 or cin != cout:
            raise RuntimeError(f"{what}: expected a downsample for stride {stride} and {cin} -> {cout} channels, got None")
    else:
        if not isinstance(ds, nn.Sequential) or len(ds) != 2:
            raise RuntimeError(f"{what}: expected downsample to be None or a Sequential(Conv2d, BatchNorm2d), got "
                               f"{type(ds).__name__}" + (f" of {len(ds)} modules" if isinstance(ds, nn.Sequential) else ""))
        ds_stride = _check_conv_bn(f"{what}: downsample", ds[0], ds[1], 1, 0, (1, 2))
        if ds_stride != stride or (ds[0].in_channels, ds[0].out_channels) != (cin, cout):
            raise RuntimeError(f"{what}: expected downsample Conv2d({cin}, {cout}, 1, stride={stride}), got "
                               f"Conv2d({ds[0].in_channels}, {ds[0].out_channels}, 1, stride={ds_stride})")
        down = _fold_conv(ds[0], ds[1], pack_conv1x1_weight, dev)
    return BottleneckParams(_fold_conv(block.conv1, block.bn1, pack_conv1x1_weight, dev),
                            _fold_conv(block.conv2, block.bn2, pack_conv3x3_weight, dev),
                            _fold_conv(block.conv3, block.bn3, pack_conv1x1_weight, dev), down, stride)


def fold_stem(conv1, bn1, relu, maxpool, device="cuda"):
    """The reference's eval-mode stem (pose_resnet.py:205-209): ``Conv2d(3, 64, 7, stride=2, padding=3)`` with no
    dilation and one group, ``BatchNorm2d(64)`` with running statistics, ``nn.ReLU`` and
    ``MaxPool2d(kernel_size=3, stride=2, padding=1)`` with dilation 1, ``ceil_mode=False``,
    ``return_indices=False`` -> ``ConvParams`` on ``device``: the weight rounded once to bf16 and packed
    (``pack_stem_weight``), the BatchNorm (and a conv bias, if any) folded in float64 and rounded once to f32.
    Anything else raises a RuntimeError naming what was found."""
    what = "fold_stem"
    _check_conv_bn(f"{what}: conv1", conv1, bn1, STEM_K, 3, (2,))
    if (conv1.in_channels, conv1.out_channels) != (STEM_CIN, STEM_COUT):
        raise RuntimeError(f"{what}: expected conv1 to be Conv2d({STEM_CIN}, {STEM_COUT}, {STEM_K}), got "
                           f"Conv2d({conv1.in_channels}, {conv1.out_channels}, {STEM_K})")
    if not isinstance(relu, nn.ReLU):
        raise RuntimeError(f"{what}: expected an nn.ReLU behind bn1, got {type(relu).__name__}")
    if not isinstance(maxpool, nn.MaxPool2d):
        raise RuntimeError(f"{what}: expected a MaxPool2d behind the ReLU, got {type(maxpool).__name__}")
    found = dict(kernel_size=_pair(maxpool.kernel_size), stride=_pair(maxpool.stride), padding=_pair(maxpool.padding),
                 dilation=_pair(maxpool.dilation), ceil_mode=bool(maxpool.ceil_mode),
                 return_indices=bool(maxpool.return_indices))
    want = dict(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1), dilation=(1, 1), ceil_mode=False, return_indices=False)
    bad = {n: v for n, v in found.items() if v != want[n]}
    if bad:
        raise RuntimeError(f"{what}: expected MaxPool2d(kernel_size=3, stride=2, padding=1) with dilation 1, ceil_mode=False "
                           "and return_indices=False, got " + ", ".join(f"{n}={v}" for n, v in bad.items()))
    return _fold_conv(conv1, bn1, pack_stem_weight, torch.device(device))


# ----------------------------------------------------------------------------- launches
def _aligned(t):
    from .backbone import _aligned as aligned
    return aligned(t)


def _check_x(what, name, x, max_c):
    if x.dtype != torch.bfloat16:
        raise TypeError(f"{what}: {name} must be bfloat16, got {x.dtype}")
    if x.dim() != 4:
        raise RuntimeError(f"{what}: {name} must be (M, H, W, C) channels-last, got {tuple(x.shape)}")
    M, H, W, C = x.shape
    _check_c(what, f"the channels of {name}", C, max_c)
    if H < 1 or W < 1 or M * H * W * C * 2 > MAX_BYTES:
        raise RuntimeError(f"{what}: {name} must have H, W >= 1 and stay below 2^31 bytes, got {tuple(x.shape)}")


def _check_folded(what, name, p, shape, cout):
    if (tuple(p.packed.shape) != shape or p.packed.dtype != torch.bfloat16 or tuple(p.scale.shape) != (cout,)
            or tuple(p.shift.shape) != (cout,) or p.scale.dtype != torch.float32 or p.shift.dtype != torch.float32):
        raise RuntimeError(f"{what}: {name} must be packed bfloat16 weights {shape} with float32 scale and shift "
                           f"({cout},), got {tuple(p.packed.shape)} {p.packed.dtype}, {tuple(p.scale.shape)} {p.scale.dtype}, "
                           f"{tuple(p.shift.shape)} {p.shift.dtype}")


def conv1x1(x_cl, packed, scale, shift, skip=None, skip_params=None, skip_stride=1):
    """One launch of mvn_conv1x1: x_cl (M, H, W, Cin) bfloat16 channels-last ->
    ``relu(conv1x1(x) * scale + shift + skip term)`` as (M, H, W, Cout) bfloat16, ``packed`` from
    ``pack_conv1x1_weight``.  Without ``skip`` there is no residual; ``skip`` (M, H, W, Cout) alone is added
    as it is; ``skip`` (M, Hs, Ws, Cs) with ``skip_params = (packed, scale, shift)`` goes through its folded
    1x1 convolution at ``skip_stride`` 1 | 2 (H = (Hs - 1) // skip_stride + 1, the same for W).  Channel counts
    are multiples of 64 in [64, 2048].  A misaligned view is copied.  GPU only; inference-only."""
    what = "conv1x1"
    sp = ConvParams(*skip_params) if skip_params is not None else None
    _inference_only(what, x_cl, packed, scale, shift, skip, *(sp or ()),
                    instead="the backbone's own Bottleneck, which autograd records")
    _check_x(what, "x_cl", x_cl, MAX_C1)
    M, H, W, cin = x_cl.shape
    if scale.dim() != 1:
        raise RuntimeError(f"{what}: scale must be (Cout,), got {tuple(scale.shape)}")
    cout = scale.shape[0]
    _check_c(what, "Cout", cout, MAX_C1)
    _check_folded(what, "the weights", ConvParams(packed, scale, shift), (cin // 32, cout // 16, 64, 8), cout)
    if M * H * W * cout * 2 > MAX_BYTES:
        raise RuntimeError(f"{what}: the output must stay below 2^31 bytes, got {(M, H, W, cout)}")
    if skip is None:
        if sp is not None:
            raise RuntimeError(f"{what}: skip_params without skip")
        return _ops.call(_ops.conv1x1, _aligned(x_cl), _aligned(packed), _aligned(scale), _aligned(shift),
                         _lib.MVN_SKIP_NONE, None, None, None, None, 1)
    if sp is None:
        if skip.dtype != torch.bfloat16 or tuple(skip.shape) != (M, H, W, cout):
            raise RuntimeError(f"{what}: an identity skip must be bfloat16 {(M, H, W, cout)}, got {skip.dtype} "
                               f"{tuple(skip.shape)}")
        return _ops.call(_ops.conv1x1, _aligned(x_cl), _aligned(packed), _aligned(scale), _aligned(shift),
                         _lib.MVN_SKIP_IDENTITY, _aligned(skip), None, None, None, 1)
    if skip_stride not in (1, 2):
        raise ValueError(f"{what}: skip_stride must be 1 or 2, got {skip_stride!r}")
    _check_x(what, "skip", skip, MAX_C1)
    Ms, Hs, Ws, cs = skip.shape
    if Ms != M or (Hs - 1) // skip_stride + 1 != H or (Ws - 1) // skip_stride + 1 != W:
        raise RuntimeError(f"{what}: a pointwise skip at stride {skip_stride} must map onto {(M, H, W)}, got "
                           f"{tuple(skip.shape)}")
    _check_folded(what, "skip_params", sp, (cs // 32, cout // 16, 64, 8), cout)
    return _ops.call(_ops.conv1x1, _aligned(x_cl), _aligned(packed), _aligned(scale), _aligned(shift),
                     _lib.MVN_SKIP_POINTWISE, _aligned(skip), _aligned(sp.packed), _aligned(sp.scale),
                     _aligned(sp.shift), int(skip_stride))


def conv3x3(x_cl, packed, scale, shift, stride=1):
    """One launch of mvn_conv3x3: x_cl (M, H, W, C) bfloat16 channels-last ->
    ``relu(conv3x3(x, padding=1, stride) * scale + shift)`` as (M, (H - 1) // stride + 1, (W - 1) // stride + 1, C)
    bfloat16, ``packed`` from ``pack_conv3x3_weight``.  C is a multiple of 64 in [64, 512], stride 1 | 2.  A
    misaligned view is copied.  GPU only; inference-only."""
    what = "conv3x3"
    _inference_only(what, x_cl, packed, scale, shift, instead="the backbone's own Bottleneck, which autograd records")
    if stride not in (1, 2):
        raise ValueError(f"{what}: stride must be 1 or 2, got {stride!r}")
    _check_x(what, "x_cl", x_cl, MAX_C3)
    C = x_cl.shape[3]
    _check_folded(what, "the weights", ConvParams(packed, scale, shift), (9, C // 32, C // 16, 64, 8), C)
    return _ops.call(_ops.conv3x3, _aligned(x_cl), _aligned(packed), _aligned(scale), _aligned(shift), int(stride))


def stem(images, packed, scale, shift):
    """One launch of mvn_stem: images (M, 3, H, W) float32 or bfloat16 ->
    ``max_pool2d(relu(conv7x7(bf16(images), stride 2, padding 3) * scale + shift), 3, 2, 1)`` as
    (M, Hp, Wp, 64) bfloat16 channels-last, Hp = ((H - 1) // 2) // 2 + 1 and the same for W; ``packed`` from
    ``pack_stem_weight``.  A non-contiguous tensor (channels_last included) is made contiguous and a
    misaligned view of the weights is copied.  GPU only; inference-only."""
    what = "stem"
    _inference_only(what, images, packed, scale, shift, instead="the backbone's own conv1, bn1, relu and maxpool, "
                    "which autograd records")
    if images.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{what}: images must be float32 or bfloat16, got {images.dtype}")
    if images.dim() != 4 or images.shape[1] != STEM_CIN:
        raise RuntimeError(f"{what}: images must be (M, {STEM_CIN}, H, W), got {tuple(images.shape)}")
    M, _, H, W = images.shape
    if H < 1 or W < 1 or M * STEM_CIN * H * W * images.element_size() > MAX_BYTES:
        raise RuntimeError(f"{what}: images must have H, W >= 1 and stay below 2^31 bytes, got {tuple(images.shape)}")
    _check_folded(what, "the weights", ConvParams(packed, scale, shift), (STEM_K_SLOTS // 32, STEM_COUT // 16, 64, 8),
                  STEM_COUT)
    out_shape = (M, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1, STEM_COUT)
    if out_shape[0] * out_shape[1] * out_shape[2] * STEM_COUT * 2 > MAX_BYTES:
        raise RuntimeError(f"{what}: the output must stay below 2^31 bytes, got {out_shape}")
    return _ops.call(_ops.stem, images.contiguous(), _aligned(packed), _aligned(scale), _aligned(shift))


def bottleneck(x_cl, params):
    """An eval-mode Bottleneck in three launches: x_cl (M, H, W, Cin) bfloat16 channels-last -> (M, Ho, Wo, Cout)
    bfloat16 with ``params`` from ``fold_bottleneck``; the residual is x_cl itself, or x_cl through the
    folded downsample inside the last launch.  Inference-only."""
    p = BottleneckParams(*params)
    h = conv1x1(x_cl, *p.conv1)
    h = conv3x3(h, *p.conv2, stride=p.stride)
    if p.downsample is None:
        return conv1x1(h, *p.conv3, skip=x_cl)
    return conv1x1(h, *p.conv3, skip=x_cl, skip_params=p.downsample, skip_stride=p.stride)


class BottleneckCL(nn.Module):
    """Eval-mode replacement of a reference ``Bottleneck`` on a channels-last bfloat16 tensor:
    ``BottleneckCL.from_reference(block)(x_cl)``.  The parameters are copied."""

    _CONVS = ("conv1", "conv2", "conv3", "downsample")

    def __init__(self, params):
        super().__init__()
        p = BottleneckParams(*params)
        self.stride = int(p.stride)
        self.has_downsample = p.downsample is not None
        for name in self._CONVS:
            c = getattr(p, name)
            if c is None:
                continue
            c = ConvParams(*c)
            self.register_buffer(f"{name}_packed", c.packed)
            self.register_buffer(f"{name}_scale", c.scale)
            self.register_buffer(f"{name}_shift", c.shift)
        self.cin = p.conv1.packed.shape[0] * 32
        self.cout = p.conv3.scale.shape[0]

    @classmethod
    def from_reference(cls, block, device="cuda"):
        return cls(fold_bottleneck(block, device=device))

    def _conv(self, name):
        return ConvParams(getattr(self, f"{name}_packed"), getattr(self, f"{name}_scale"), getattr(self, f"{name}_shift"))

    @property
    def params(self):
        return BottleneckParams(self._conv("conv1"), self._conv("conv2"), self._conv("conv3"),
                                self._conv("downsample") if self.has_downsample else None, self.stride)

    def forward(self, x_cl):
        return bottleneck(x_cl, self.params)


_STEM = ("conv1", "bn1", "relu", "maxpool")
_LAYERS = ("layer1", "layer2", "layer3", "layer4")


class StemEval(nn.Module):
    """Eval-mode replacement of the reference's ``conv1, bn1, relu, maxpool`` in one launch (``stem``):
    ``StemEval.from_reference(backbone)(images (M, 3, H, W) float32 or bfloat16)`` returns the pooled map as
    (M, Hp, Wp, 64) bfloat16 channels-last, what the first ``BottleneckCL`` reads.  The parameters are copied."""

    def __init__(self, params):
        super().__init__()
        p = ConvParams(*params)
        self.register_buffer("packed", p.packed)
        self.register_buffer("scale", p.scale)
        self.register_buffer("shift", p.shift)

    @classmethod
    def from_reference(cls, backbone, device="cuda"):
        missing = [n for n in _STEM if not isinstance(getattr(backbone, n, None), nn.Module)]
        if missing:
            raise RuntimeError(f"StemEval: expected the stem modules {', '.join(_STEM)}; {type(backbone).__name__} has no "
                               f"{', '.join(missing)}")
        return cls(fold_stem(*(getattr(backbone, n) for n in _STEM), device=device))

    @property
    def params(self):
        return ConvParams(self.packed, self.scale, self.shift)

    def forward(self, images):
        return stem(images, *self.params)


class TrunkEval(nn.Module):
    """``conv1`` .. ``layer4`` of the reference's ``PoseResNet.forward`` (pose_resnet.py:293-310), eval mode:
    ``module(images (M, 3, H, W))`` returns ``layer4``'s output as an (M, C, h, w) bfloat16 tensor in
    channels_last memory format, a view of the last kernel's output, which ``DeconvHeadEval`` reads without
    a copy.

    1. the stem ``conv1, bn1, relu, maxpool``: the backbone's own modules (not copies), on the device and
       in the dtype of the input;
    2. one cast-and-permute pass: channels-last bfloat16;
    3. every ``Bottleneck`` of ``layer1`` .. ``layer4``: three launches (``bottleneck``).

    With ``stem="kernels"`` steps 1 and 2 are one launch of ``StemEval``, whose output the
    first block reads as it is.  The blocks' parameters are copied: later changes to the backbone do not reach
    them."""

    def __init__(self, stem, blocks):
        super().__init__()
        self.stem = stem
        self.blocks = nn.ModuleList(blocks)

    @classmethod
    def from_reference(cls, backbone, device="cuda", stem="torch"):
        """``backbone.conv1, bn1, relu, maxpool`` as they are (``stem="torch"``, the default) or folded into a
        ``StemEval`` (``stem="kernels"``), and ``backbone.layer1`` .. ``layer4``, each a Sequential of
        ``Bottleneck`` blocks whose channels chain; anything else raises and names what it found."""
        what = "TrunkEval"
        if stem not in ("torch", "kernels"):
            raise ValueError(f"{what}: stem must be 'torch' or 'kernels', got {stem!r}")
        missing = [n for n in _STEM + _LAYERS if not isinstance(getattr(backbone, n, None), nn.Module)]
        if missing:
            raise RuntimeError(f"{what}: expected the trunk modules {', '.join(_STEM + _LAYERS)}; {type(backbone).__name__} "
                               f"has no {', '.join(missing)}")
        blocks, c = [], getattr(backbone.conv1, "out_channels", None)
        for name in _LAYERS:
            layer = getattr(backbone, name)
            if not isinstance(layer, nn.Sequential) or len(layer) == 0:
                raise RuntimeError(f"{what}: expected {name} to be a Sequential of Bottleneck blocks, got "
                                   f"{type(layer).__name__}")
            for i, block in enumerate(layer):
                try:
                    b = BottleneckCL.from_reference(block, device=device)
                except RuntimeError as e:
                    raise RuntimeError(f"{what}: {name}[{i}]: {e}") from None
                if c is not None and b.cin != c:
                    raise RuntimeError(f"{what}: {name}[{i}]: expected {c} input channels behind a {c}-channel layer, got "
                                       f"conv1.in_channels={b.cin}")
                c = b.cout
                blocks.append(b)
        if stem == "kernels":
            try:
                return cls(StemEval.from_reference(backbone, device=device), blocks)
            except RuntimeError as e:
                raise RuntimeError(f"{what}: {e}") from None
        return cls(nn.Sequential(*(getattr(backbone, n) for n in _STEM)), blocks)

    def channels_last(self, x):
        """The stem and the one cast-and-permute pass, or the one launch of a ``StemEval``: images ->
        (M, h, w, C) bfloat16."""
        if isinstance(self.stem, StemEval):
            return self.stem(x)
        h = self.stem(x).permute(0, 2, 3, 1)
        return torch.empty(h.shape, dtype=torch.bfloat16, device=h.device).copy_(h)

    def forward(self, x):
        _inference_only("TrunkEval", x, instead="the backbone itself, which autograd records")
        if x.dim() != 4:
            raise RuntimeError(f"TrunkEval: x must be (M, 3, H, W), got {tuple(x.shape)}")
        h = self.channels_last(x)
        for block in self.blocks:
            h = block(h)
        return h.permute(0, 3, 1, 2)
