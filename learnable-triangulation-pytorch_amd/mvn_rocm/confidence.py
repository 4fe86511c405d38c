"""The 2-D backbone's confidence heads on this package's kernels (mvn/models/pose_resnet.py:140-174,
``GlobalAveragePoolingHead``).  A head is

    Conv2d(Cin, 512, 3, padding=1) + BatchNorm2d + MaxPool2d(2) + ReLU
    Conv2d(512, 256, 3, padding=1) + BatchNorm2d + MaxPool2d(2) + ReLU
    the mean over the pixels, Linear(256, 512) + ReLU + Linear(512, 256) + ReLU + Linear(256, n) + Sigmoid

and runs as three launches (csrc/confidence_head.hip): ``conv3x3_pool`` twice (bf16 MFMA, f32 accumulation;
bfloat16 out, then float32 out) and ``confidence_tail`` (f32 on the vector ALU).  ``ConfidenceHeadEval`` is
the head as a module; ``backbone.BackboneEval.from_reference(..., confidences="kernels")`` puts it in
place of the backbone's ``alg_confidences`` and ``vol_confidences``.  Eval mode, inference-only.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from . import _ops
from .op import _dtype_code
from .resnet import ConvParams, _aligned, _check_c, _check_conv_bn, _check_folded, _fold_conv, _pair
from .v2v import _inference_only, _pack_mfma_a

MIN_C, MAX_CIN, MAX_COUT = 64, 2048, 512
MAX_WIDTH, MAX_N = 512, 32                # of the tail's Linear layers
MAX_BYTES = 2 ** 31 - 1                   # of one tensor: one buffer resource
_INSTEAD = "the backbone's own confidence head, which autograd records"


class TailParams(NamedTuple):
    """What ``pack_confidence_tail`` returns: the packed float32 parameters and the widths (C0, C1, C2, n)."""
    packed: torch.Tensor
    widths: tuple


class ConfidenceHeadParams(NamedTuple):
    """What ``fold_confidence_head`` returns: the two folded convolutions and the packed tail."""
    conv1: ConvParams
    conv2: ConvParams
    tail: TailParams


def pack_conv3x3_pool_weight(w):
    """(Cout, Cin, 3, 3) float64 Conv2d weight -> (9, Cin / 32, Cout / 16, 64, 8) bf16 as mvn_conv3x3_pool reads it:
    [tap = ky*3 + kx][kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError(f"expected a (Cout, Cin, 3, 3) Conv2d weight, got {tuple(w.shape)}")
    cout, cin = w.shape[:2]
    _check_c("pack_conv3x3_pool_weight", "Cin", cin, MAX_CIN)
    _check_c("pack_conv3x3_pool_weight", "Cout", cout, MAX_COUT)
    return _pack_mfma_a(w.permute(2, 3, 0, 1).reshape(9, cout, cin))


def _tail_size(c0, c1, c2, n):
    return c0 * c1 + c1 + c1 * c2 + c2 + c2 * n + n


def pack_confidence_tail(linears):
    """Three ``(weight (out, in), bias (out,))`` pairs, Linear(C0, C1), Linear(C1, C2), Linear(C2, n) ->
    ``TailParams`` with one flat float32 tensor as mvn_confidence_tail reads it, each weight transposed to
    (in, out):

        packed[i * C1 + o]      = W1[o][i]        packed[O1 + o] = b1[o]     O1 = C0 C1
        packed[O2 + i * C2 + o] = W2[o][i]        packed[O3 + o] = b2[o]     O2 = O1 + C1,  O3 = O2 + C1 C2
        packed[O4 + i * n + o]  = W3[o][i]        packed[O5 + o] = b3[o]     O4 = O3 + C2,  O5 = O4 + C2 n

    C0, C1, C2 are multiples of 64 in [64, 512] and 1 <= n <= 32; the values are copied as float32."""
    what = "pack_confidence_tail"
    linears = list(linears)
    if len(linears) != 3:
        raise RuntimeError(f"{what}: expected three (weight, bias) pairs, got {len(linears)}")
    parts, widths = [], []
    for k, (w, b) in enumerate(linears):
        if w.dim() != 2 or b is None or tuple(b.shape) != (w.shape[0],):
            raise RuntimeError(f"{what}: Linear {k}: expected a weight (out, in) and a bias (out,), got "
                               f"{tuple(w.shape)} and {None if b is None else tuple(b.shape)}")
        if widths and w.shape[1] != widths[-1]:
            raise RuntimeError(f"{what}: Linear {k}: expected {widths[-1]} inputs behind a {widths[-1]}-wide layer, got "
                               f"in_features={w.shape[1]}")
        if not widths:
            widths.append(w.shape[1])
        widths.append(w.shape[0])
        parts += [w.detach().float().cpu().t().contiguous().reshape(-1), b.detach().float().cpu().reshape(-1)]
    c0, c1, c2, n = widths
    for name, c in (("C0", c0), ("C1", c1), ("C2", c2)):
        _check_c(what, name, c, MAX_WIDTH)
    if not 1 <= n <= MAX_N:
        raise RuntimeError(f"{what}: expected 1 to {MAX_N} outputs, got out_features={n}")
    return TailParams(torch.cat(parts).contiguous(), (c0, c1, c2, n))


# ----------------------------------------------------------------------------- the fold
_POOL_WANT = dict(kernel_size=(2, 2), stride=(2, 2), padding=(0, 0), dilation=(1, 1), ceil_mode=False, return_indices=False)


def _check_stage(what, conv, bn, pool, relu):
    _check_conv_bn(what, conv, bn, 3, 1, (1,))
    if not isinstance(pool, nn.MaxPool2d):
        raise RuntimeError(f"{what}: expected a MaxPool2d behind the BatchNorm2d, got {type(pool).__name__}")
    found = dict(kernel_size=_pair(pool.kernel_size), stride=_pair(pool.stride), padding=_pair(pool.padding),
                 dilation=_pair(pool.dilation), ceil_mode=bool(pool.ceil_mode), return_indices=bool(pool.return_indices))
    bad = {n: v for n, v in found.items() if v != _POOL_WANT[n]}
    if bad:
        raise RuntimeError(f"{what}: expected MaxPool2d(2) with stride 2, no padding, no dilation, ceil_mode=False and "
                           "return_indices=False, got " + ", ".join(f"{n}={v}" for n, v in bad.items()))
    if not isinstance(relu, nn.ReLU):
        raise RuntimeError(f"{what}: expected an nn.ReLU behind the MaxPool2d, got {type(relu).__name__}")


def fold_confidence_head(head, device="cuda"):
    """The reference's eval-mode ``GlobalAveragePoolingHead`` -> ``ConfidenceHeadParams`` on ``device``.
    ``head.features`` is a Sequential of (Conv2d k=3 stride 1 padding 1, no dilation, one group; BatchNorm2d
    with running statistics; MaxPool2d(2) with stride 2, no padding, no dilation, floor mode; ReLU), twice;
    ``head.head`` a Sequential of (Linear, ReLU, Linear, ReLU, Linear, Sigmoid); the widths chain, Cin a
    multiple of 64 in [64, 2048], the other widths multiples of 64 in [64, 512], at most 32 outputs.  The
    convolutions' weights are rounded once to bf16 and packed, their bias and BatchNorm folded in float64
    and rounded once to f32; the Linear layers stay float32.  The parameters are copied.  Anything else
    raises a RuntimeError naming what was found."""
    what = "fold_confidence_head"
    feats, lin = getattr(head, "features", None), getattr(head, "head", None)
    if not isinstance(feats, nn.Sequential) or len(feats) != 8:
        n = f" of {len(feats)} modules" if isinstance(feats, nn.Sequential) else ""
        raise RuntimeError(f"{what}: expected features to be a Sequential of (Conv2d, BatchNorm2d, MaxPool2d, ReLU) twice, "
                           f"got {type(feats).__name__}{n}")
    if not isinstance(lin, nn.Sequential) or len(lin) != 6:
        n = f" of {len(lin)} modules" if isinstance(lin, nn.Sequential) else ""
        raise RuntimeError(f"{what}: expected head to be a Sequential of (Linear, ReLU, Linear, ReLU, Linear, Sigmoid), "
                           f"got {type(lin).__name__}{n}")
    for s in (0, 1):
        _check_stage(f"{what}: features[{4 * s}:{4 * s + 4}]", *feats[4 * s:4 * s + 4])
    want = (nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear, nn.Sigmoid)
    if not all(isinstance(m, t) for m, t in zip(lin, want)):
        raise RuntimeError(f"{what}: expected head to be (Linear, ReLU, Linear, ReLU, Linear, Sigmoid), got "
                           f"({', '.join(type(m).__name__ for m in lin)})")
    c1, c2, linears = feats[0], feats[4], (lin[0], lin[2], lin[4])
    _check_c(what, "features[0].in_channels", c1.in_channels, MAX_CIN)
    _check_c(what, "features[0].out_channels", c1.out_channels, MAX_COUT)
    _check_c(what, "features[4].out_channels", c2.out_channels, MAX_WIDTH)
    if c2.in_channels != c1.out_channels:
        raise RuntimeError(f"{what}: expected features[4] to take features[0]'s {c1.out_channels} channels, got "
                           f"in_channels={c2.in_channels}")
    width = c2.out_channels
    for k, l in zip((0, 2, 4), linears):
        if l.in_features != width:
            raise RuntimeError(f"{what}: expected head[{k}] to take {width} inputs, got in_features={l.in_features}")
        if l.bias is None:
            raise RuntimeError(f"{what}: expected head[{k}] to have a bias, got bias=None")
        width = l.out_features
    try:
        tail = pack_confidence_tail([(l.weight, l.bias) for l in linears])
    except RuntimeError as e:
        raise RuntimeError(f"{what}: head: {e}") from None
    dev = torch.device(device)
    return ConfidenceHeadParams(_fold_conv(c1, feats[1], pack_conv3x3_pool_weight, dev),
                                _fold_conv(c2, feats[5], pack_conv3x3_pool_weight, dev),
                                TailParams(tail.packed.to(dev), tail.widths))


# ----------------------------------------------------------------------------- launches
def conv3x3_pool(x_cl, packed, scale, shift, out_dtype=None):
    """One launch of mvn_conv3x3_pool: x_cl (M, H, W, Cin) bfloat16 channels-last ->
    ``relu(max_pool2d(conv3x3(x, padding=1) * scale + shift, 2))`` as (M, H // 2, W // 2, Cout) bfloat16 |
    float32 (``out_dtype``, default bfloat16), ``packed`` from ``pack_conv3x3_pool_weight``, Cout =
    ``len(scale)``.  Cin is a multiple of 64 in [64, 2048], Cout in [64, 512]; H, W >= 2.  bf16 operands, f32
    accumulation in one fixed order (include/mvn_hip.h), one rounding; the float32 output rounded to bfloat16 is
    the bfloat16 output.  A misaligned view is copied.  GPU only; inference-only."""
    what = "conv3x3_pool"
    _inference_only(what, x_cl, packed, scale, shift, instead=_INSTEAD)
    od = _dtype_code(torch.bfloat16 if out_dtype is None else out_dtype)
    if x_cl.dtype != torch.bfloat16:
        raise TypeError(f"{what}: x_cl must be bfloat16, got {x_cl.dtype}")
    if x_cl.dim() != 4:
        raise RuntimeError(f"{what}: x_cl must be (M, H, W, Cin) channels-last, got {tuple(x_cl.shape)}")
    M, H, W, cin = x_cl.shape
    _check_c(what, "the channels of x_cl", cin, MAX_CIN)
    if scale.dim() != 1:
        raise RuntimeError(f"{what}: scale must be (Cout,), got {tuple(scale.shape)}")
    cout = scale.shape[0]
    _check_c(what, "Cout", cout, MAX_COUT)
    if H < 2 or W < 2 or M * H * W * cin * 2 > MAX_BYTES:
        raise RuntimeError(f"{what}: x_cl must have H, W >= 2 and stay below 2^31 bytes, got {tuple(x_cl.shape)}")
    _check_folded(what, "the weights", ConvParams(packed, scale, shift), (9, cin // 32, cout // 16, 64, 8), cout)
    if M * (H // 2) * (W // 2) * cout * 4 > MAX_BYTES:
        raise RuntimeError(f"{what}: the output must stay below 2^31 bytes, got {(M, H // 2, W // 2, cout)}")
    return _ops.call(_ops.conv3x3_pool, _aligned(x_cl), _aligned(packed), _aligned(scale), _aligned(shift), od)


def confidence_tail(pooled, params, sigmoid=True):
    """One launch of mvn_confidence_tail: pooled (M, h, w, C0) float32 channels-last (the second
    ``conv3x3_pool``'s float32 output) and ``params`` from ``pack_confidence_tail`` ->
    ``sigmoid(Linear3(relu(Linear2(relu(Linear1(mean over the pixels))))))`` as (M, n) float32, or the
    logits with ``sigmoid=False``.  The mean adds the pixels in ascending order and divides once; each Linear
    is ``acc = bias[o]``, then ``acc = fma(w[o, i], x[i], acc)`` for i ascending; the sigmoid is
    ``1 / (1 + exp(-z))`` in float32.  GPU only; inference-only."""
    what = "confidence_tail"
    p = TailParams(*params)
    _inference_only(what, pooled, p.packed, instead=_INSTEAD)
    if pooled.dtype != torch.float32:
        raise TypeError(f"{what}: pooled must be float32, got {pooled.dtype}")
    if pooled.dim() != 4:
        raise RuntimeError(f"{what}: pooled must be (M, h, w, C0) channels-last, got {tuple(pooled.shape)}")
    M, h, w, c0 = pooled.shape
    widths = tuple(int(v) for v in p.widths)
    if len(widths) != 4 or widths[0] != c0:
        raise RuntimeError(f"{what}: params are for widths {widths}, pooled has {c0} channels")
    for name, c in zip(("C0", "C1", "C2"), widths):
        _check_c(what, name, c, MAX_WIDTH)
    n = widths[3]
    if not 1 <= n <= MAX_N:
        raise RuntimeError(f"{what}: expected 1 to {MAX_N} outputs, got {n}")
    if h * w < 1 or M * h * w * c0 * 4 > MAX_BYTES:
        raise RuntimeError(f"{what}: pooled must have h w >= 1 and stay below 2^31 bytes, got {tuple(pooled.shape)}")
    if p.packed.dtype != torch.float32 or tuple(p.packed.shape) != (_tail_size(*widths),):
        raise RuntimeError(f"{what}: the packed parameters must be float32 ({_tail_size(*widths)},) as pack_confidence_tail "
                           f"returns them, got {p.packed.dtype} {tuple(p.packed.shape)}")
    return _ops.call(_ops.confidence_tail, pooled.contiguous(), p.packed.contiguous(), widths[1], widths[2], n,
                     bool(sigmoid))


class ConfidenceHeadEval(nn.Module):
    """Eval-mode replacement of a reference ``GlobalAveragePoolingHead`` in three launches:
    ``ConfidenceHeadEval.from_reference(head)(x (M, Cin, h, w))`` returns (M, n) float32.  h, w >= 4 (below
    that the second pool has no window, and torch raises as well).  A bfloat16 x in channels_last memory
    format, what ``resnet.TrunkEval`` returns, is read as it is; anything else takes one cast-and-permute
    pass.  The first stage writes bfloat16 (the second's operand), the second float32 (the tail's input).
    The parameters are copied: later changes to the head do not reach this module."""

    def __init__(self, params):
        super().__init__()
        p = ConfidenceHeadParams(*params)
        for name, c in (("conv1", ConvParams(*p.conv1)), ("conv2", ConvParams(*p.conv2))):
            self.register_buffer(f"{name}_packed", c.packed)
            self.register_buffer(f"{name}_scale", c.scale)
            self.register_buffer(f"{name}_shift", c.shift)
        tail = TailParams(*p.tail)
        self.register_buffer("tail_packed", tail.packed)
        self.widths = tuple(int(v) for v in tail.widths)
        self.cin = self.conv1_packed.shape[1] * 32

    @classmethod
    def from_reference(cls, head, device="cuda"):
        return cls(fold_confidence_head(head, device=device))

    def _conv(self, name):
        return ConvParams(getattr(self, f"{name}_packed"), getattr(self, f"{name}_scale"), getattr(self, f"{name}_shift"))

    @property
    def params(self):
        return ConfidenceHeadParams(self._conv("conv1"), self._conv("conv2"), TailParams(self.tail_packed, self.widths))

    def forward(self, x):
        what = "ConfidenceHeadEval"
        _inference_only(what, x, instead=_INSTEAD)
        if x.dim() != 4 or x.shape[1] != self.cin:
            raise RuntimeError(f"{what}: x must be (M, {self.cin}, h, w), got {tuple(x.shape)}")
        if x.shape[2] < 4 or x.shape[3] < 4:
            raise RuntimeError(f"{what}: x must have h, w >= 4 (two 2 x 2 pools), got {tuple(x.shape)}")
        h = x.permute(0, 2, 3, 1)
        if h.dtype != torch.bfloat16 or not h.is_contiguous():
            h = torch.empty(h.shape, dtype=torch.bfloat16, device=x.device).copy_(h)   # the one cast-and-permute pass
        p = self.params
        h = conv3x3_pool(h, *p.conv1, out_dtype=torch.bfloat16)
        h = conv3x3_pool(h, *p.conv2, out_dtype=torch.float32)
        return confidence_tail(h, p.tail, sigmoid=True)
