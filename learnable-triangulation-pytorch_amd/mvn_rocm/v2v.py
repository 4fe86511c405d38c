"""V2V front block on the GPU (BASELINE config 5).

``V2VModel.front_layers[0]`` is ``Basic3DBlock(32, 16, 7)`` (mvn/models/v2v.py:7-17,
145-146): Conv3d 32 -> 16, kernel 7, padding 3, BatchNorm3d, ReLU, applied to the
unprojected volume (triangulation.py:352).  In eval mode the block is one MFMA kernel
(csrc/v2v_front.hip) with the BatchNorm folded into a per-channel scale / shift, reading
the volume channels-last in bf16 straight from the unprojection
(``unproject_channels_last``): the unproject + view-softmax + front-block pipeline of
config 5 is two launches and one (B, V^3, 32) bf16 intermediate.

The other end of the V2V, its pointwise tail ``back_layers[1]``, ``back_layers[2]`` and
``output_layer`` (v2v.py:154-160), is ``v2v_head`` / ``V2VHead`` below (csrc/v2v_head.hip,
DESIGN.md §4.11), alone or in one call with the 3D soft-argmax behind it.

Between them, the five ``Res3DBlock``s that run at the full resolution (``front_layers[1..3]``,
``encoder_decoder.skip_res1``, ``back_layers[0]``; v2v.py:20-42) are ``v2v_conv3`` /
``res3d_block`` / ``Res3DBlockCL`` (csrc/v2v_res3d.hip), and ``V2VEval`` is the
whole eval-mode V2V with the soft-argmax, the pooled interior alone left to torch.  With
``half_res="kernels"`` the interior's first level and its boundaries run on kernels too:
``max_pool2_cl``, ``v2v_conv3_wide`` / ``res3d_block_wide`` / ``Res3DBlockWideCL`` and
``upsample2_add`` (csrc/v2v_interior.hip).  With ``deep="kernels"`` on top of it
the 128-channel levels below run on kernels as well, at any extent from 64 down to 1:
``v2v_conv3_deep`` / ``res3d_block_deep`` / ``Res3DBlockDeepCL``, ``upsample2_add_deep`` and
``v2v_interior_deep_cl`` (csrc/v2v_deep.hip), and ``V2VEval`` runs no torch module.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch
from torch import nn

from . import _lib
from ._ops import _require_gpu, _stream
from .op import _dtype_code, aggregation_code, unproject_inputs

CIN, COUT, KS = 32, 16, 7


def _f64(t):
    return t.detach().to(torch.float64).cpu()


def _bn_fold(bias, gamma, beta, mean, var, eps, channels):
    """float64 (scale, shift) of an eval-mode BatchNorm behind a conv with ``bias`` (or None):
    bn(conv(x) + bias) = conv(x) * scale + shift with scale = gamma / (var + eps) ** 0.5 and
    shift = (bias - mean) * scale + beta.  Every fold of this module goes through here."""
    s = _f64(gamma) / torch.sqrt(_f64(var) + eps)
    b = _f64(bias) if bias is not None else torch.zeros(channels, dtype=torch.float64)
    return s, (b - _f64(mean)) * s + _f64(beta)


def _pack_mfma_a(w):
    """(..., R, K) float64, R a multiple of 16 and K of 32 -> (..., K / 32, R / 16, 64, 8) bf16, the
    A fragments of v_mfma_f32_16x16x32_bf16 as every V2V kernel reads them:
    [kp][m][lane][j] = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j].  Each ``pack_*`` below is
    a reshape of its weight into rows and K-slots, this function, and at most a dropped ``kp``."""
    *lead, R, K = w.shape
    n = len(lead)
    p = w.reshape(*lead, R // 16, 16, K // 32, 4, 8)                                 # [m][lane & 15][kp][lane >> 4][j]
    p = p.permute(*range(n), n + 2, n, n + 3, n + 1, n + 4)                          # [kp][m][lane >> 4][lane & 15][j]
    return p.reshape(*lead, K // 32, R // 16, 64, 8).to(torch.float32).to(torch.bfloat16).contiguous()


def _pad_k(w):
    """The last axis zero-padded to a multiple of 32 K-slots."""
    return nn.functional.pad(w, (0, -w.shape[-1] % 32))


def fold_basic3d_block(weight, bias, bn_weight, bn_bias, running_mean, running_var, eps=1e-5, device="cuda"):
    """Eval-mode Basic3DBlock parameters -> (packed bf16 weights, scale, shift) on ``device``.

    y = relu(bn(conv(x) + bias)) = relu(conv(x) * s + ((bias - mean) * s + beta)), s the BatchNorm's
    scale, folded in float64 (``_bn_fold``).  The weights are rounded to bf16 (the
    kernel's MFMA operand type) and packed [tap][lane][8] as mvn_v2v_front expects."""
    w = _f64(weight)
    if tuple(w.shape) != (COUT, CIN, KS, KS, KS):
        raise RuntimeError(f"expected a ({COUT}, {CIN}, 7, 7, 7) Conv3d weight, got {tuple(w.shape)}")
    s, shift = _bn_fold(bias, bn_weight, bn_bias, running_mean, running_var, eps, COUT)
    packed = _pack_mfma_a(w.reshape(COUT, CIN, KS ** 3).permute(2, 0, 1))[:, 0, 0]    # [tap][lane][j]
    dev = torch.device(device)
    return packed.to(dev), s.float().to(dev), shift.float().to(dev)




def v2v_front(vol_cl, packed, scale, shift, out_dtype=torch.float32):
    """(B, V, V, V, 32) bf16 channels-last -> (B, 16, V, V, V) relu(bn(conv3d_7(x))).

    V is a multiple of 16 up to 256; a non-contiguous ``vol_cl`` is copied.  Non-finite voxels
    follow torch: the relu keeps a NaN as ``F.relu`` does, so a NaN or infinite input voxel
    reaches exactly its 7^3 neighbourhood (all 16 channels), as ``F.relu(bn(conv(x)))`` does,
    and nothing else."""
    if vol_cl.dtype != torch.bfloat16 or vol_cl.dim() != 5 or vol_cl.shape[-1] != CIN:
        raise RuntimeError(f"vol_cl must be (B, V, V, V, {CIN}) bfloat16, got {tuple(vol_cl.shape)} {vol_cl.dtype}")
    B, V = vol_cl.shape[0], vol_cl.shape[1]
    if tuple(vol_cl.shape[1:4]) != (V, V, V):
        raise RuntimeError("v2v_front needs a cubic volume")
    x = vol_cl.contiguous()
    _require_gpu(x, packed, scale, shift)
    od = _dtype_code(out_dtype)
    out = torch.empty((B, COUT, V, V, V), dtype=out_dtype, device=x.device)
    if out.numel() == 0:                  # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_v2v_front(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                     out.data_ptr(), od, B, V, _stream(x))
    _lib.check(code, "mvn_v2v_front")
    return out


def _inference_only(what, *tensors, instead=None):
    """The channels-last unprojection and the fused V2V front block have no backward: refuse
    a call autograd would record (ADVICE r5 — a 'conf*' training caller would otherwise get a
    volume without grad and lose the confidence gradient silently).  Training goes through
    ``op.unproject_heatmaps`` (differentiable in the features and the confidences)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is inference-only (no backward): call it under torch.no_grad(), or use "
                           + (instead or "mvn_rocm.op.unproject_heatmaps, which is differentiable in the features "
                              "and the confidences"))


def unproject_channels_last(heatmaps, proj_matricies, coord_volumes, volume_aggregation_method="softmax",
                            out_dtype=torch.bfloat16, align_corners=False, vol_confidences=None, precision=None):
    """unproject_heatmaps (op.py:99-163) written channels-last: (B, Vx, Vy, Vz, C).
    ``coord_volumes`` may be a ``volumetric.Cuboids`` (coordinates formed in-kernel);
    ``vol_confidences`` (B, N, C) is read for 'conf*' aggregation (op.py:147-148), as
    ``unproject_heatmaps``'s.  Inference-only: no backward (training: ``op.unproject_heatmaps``).
    ``precision`` as ``op.unproject_heatmaps``'s."""
    from .op import precision_code
    from .volumetric import Cuboids
    _inference_only("unproject_channels_last", heatmaps, vol_confidences)
    agg = aggregation_code(volume_aggregation_method)
    prec = precision_code(precision)
    cub = coord_volumes if isinstance(coord_volumes, Cuboids) else None
    feat, proj, conf = unproject_inputs(heatmaps, proj_matricies, vol_confidences, agg, volume_aggregation_method, cub)
    if conf is not None:
        _require_gpu(feat, conf)
    cptr = conf.data_ptr() if conf is not None else None
    if feat.dtype == torch.float32 and out_dtype == torch.bfloat16:
        # f32 maps into a bf16 volume: the kernels write f32 (no f32 -> bf16 instantiation,
        # mvn_hip.h), rounded to nearest-even by one device cast
        return unproject_channels_last(feat, proj, coord_volumes, volume_aggregation_method, torch.float32,
                                       align_corners, conf, precision).to(torch.bfloat16)
    fd, od = _dtype_code(feat.dtype), _dtype_code(out_dtype)
    B, N, C, H, W = feat.shape
    if N > 8:
        # the channels-last kernels take N <= 8 views (mvn_hip.h): more views go through the
        # NCDHW unprojection (any N) and one permute on the device
        from .op import unproject_heatmaps
        # written in out_dtype by the kernel itself (bf16 maps into an f32 volume keep f32
        # precision)
        vol = unproject_heatmaps(feat, proj, coord_volumes, volume_aggregation_method, conf,
                                 align_corners=align_corners, out_dtype=out_dtype, precision=precision)
        return vol.permute(0, 2, 3, 4, 1).contiguous()
    if cub is not None:
        # coordinates formed in-kernel from the per-frame cuboids (bit-identical)
        cub = coord_volumes
        _require_gpu(feat, proj, cub.params)
        V = cub.volume_size
        out = torch.empty((B, V, V, V, C), dtype=out_dtype, device=feat.device)
        if out.numel() == 0:
            return out
        code = _lib.load().mvn_unproject_precision(feat.data_ptr(), fd, proj.data_ptr(), None, cub.params.data_ptr(),
                                                   int(cub.transfer), cptr, out.data_ptr(), od, _lib.MVN_LAYOUT_NDHWC,
                                                   B, N, C, H, W, V, V, V, agg, int(align_corners), prec, _stream(feat))
        _lib.check(code, "mvn_unproject_precision")
        return out
    coords = coord_volumes.float().contiguous()
    if coords.dim() != 5 or coords.shape[0] != B or coords.shape[4] != 3:
        raise RuntimeError(f"coord_volumes must be ({B}, Vx, Vy, Vz, 3), got {tuple(coords.shape)}")
    _require_gpu(feat, proj, coords)
    Vx, Vy, Vz = coords.shape[1:4]
    out = torch.empty((B, Vx, Vy, Vz, C), dtype=out_dtype, device=feat.device)
    if out.numel() == 0:                  # empty batch: the empty volume, as unproject_heatmaps
        return out
    code = _lib.load().mvn_unproject_precision(feat.data_ptr(), fd, proj.data_ptr(), coords.data_ptr(), None, 0, cptr,
                                               out.data_ptr(), od, _lib.MVN_LAYOUT_NDHWC, B, N, C, H, W, Vx, Vy, Vz,
                                               agg, int(align_corners), prec, _stream(feat))
    _lib.check(code, "mvn_unproject_precision")
    return out


class Basic3DBlockFront(nn.Module):
    """Eval-mode replacement of Basic3DBlock(32, 16, 7) on a channels-last bf16 volume."""

    def __init__(self, packed, scale, shift):
        super().__init__()
        self.register_buffer("packed", packed)
        self.register_buffer("scale", scale)
        self.register_buffer("shift", shift)

    @classmethod
    def from_reference(cls, block, device="cuda"):
        conv, bn = block.block[0], block.block[1]
        return cls(*fold_basic3d_block(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                                       bn.running_var, bn.eps, device=device))

    def forward(self, vol_cl, out_dtype=torch.float32):
        return v2v_front(vol_cl, self.packed, self.scale, self.shift, out_dtype)


def unproject_v2v_front(heatmaps, proj_matricies, coord_volumes, packed, scale, shift,
                        volume_aggregation_method="softmax", out_dtype=torch.float32, group_frames=0,
                        align_corners=False, vol_confidences=None, precision=None):
    """Config 5 in one call (``mvn_unproject_v2v_front``): unproject_heatmaps (op.py:99-163)
    written channels-last bf16, then the front block relu(bn(conv3d_7)), pipelined over frame
    groups through a workspace of one group's intermediate (default: 8 frames at V = 64,
    within half of the MALL).  ``coord_volumes`` may be a ``volumetric.Cuboids``.  Equal to
    ``v2v_front(unproject_channels_last(...))`` bit for bit, NaN included: a NaN voxel coming out
    of the unprojection is NaN in its 7^3 neighbourhood of the result (``v2v_front``), not 0.
    'conf*' aggregation reads
    ``vol_confidences`` (B, N, C), as the volumetric model does (triangulation.py:349).
    Inference-only: no backward (the eval-mode BatchNorm fold is inference by construction).
    ``precision='fast'`` runs the two steps (the one-call C pipeline is the
    exact arithmetic)."""
    from .op import precision_code
    from .volumetric import Cuboids
    _inference_only("unproject_v2v_front", heatmaps, vol_confidences)
    agg = aggregation_code(volume_aggregation_method)
    fast = precision_code(precision) == _lib.MVN_PRECISION_FAST
    cub = coord_volumes if isinstance(coord_volumes, Cuboids) else None
    feat, proj, conf = unproject_inputs(heatmaps, proj_matricies, vol_confidences, agg, volume_aggregation_method, cub)
    fd, od = _dtype_code(feat.dtype), _dtype_code(out_dtype)
    B, N, C, H, W = feat.shape
    if C != CIN:
        raise RuntimeError(f"unproject_v2v_front needs {CIN} heatmap channels, got {C}")
    if N > 8 or B == 0 or fast:
        # more than 8 views (the channels-last kernels take N <= 8) or an empty batch: the two
        # steps, which handle both
        cl = unproject_channels_last(feat, proj, coord_volumes, volume_aggregation_method, align_corners=align_corners,
                                     vol_confidences=conf, precision=precision)
        return v2v_front(cl, packed, scale, shift, out_dtype)
    if cub is not None:
        coords, V = None, cub.volume_size
        _require_gpu(feat, proj, cub.params, packed, scale, shift)
    else:
        coords = coord_volumes.float().contiguous()
        if coords.dim() != 5 or coords.shape[0] != B or coords.shape[4] != 3 or len(set(coords.shape[1:4])) != 1:
            raise RuntimeError(f"coord_volumes must be ({B}, V, V, V, 3), got {tuple(coords.shape)}")
        V = coords.shape[1]
        _require_gpu(feat, proj, coords, packed, scale, shift)
    if conf is not None:
        _require_gpu(feat, conf)
    lib = _lib.load()
    ws = torch.empty(lib.mvn_unproject_v2v_front_workspace_bytes(int(group_frames), V), dtype=torch.uint8,
                     device=feat.device)
    out = torch.empty((B, COUT, V, V, V), dtype=out_dtype, device=feat.device)
    code = lib.mvn_unproject_v2v_front_ex(feat.data_ptr(), fd, proj.data_ptr(),
                                          coords.data_ptr() if coords is not None else None,
                                          cub.params.data_ptr() if cub is not None else None,
                                          int(cub.transfer) if cub is not None else 0, agg,
                                          conf.data_ptr() if conf is not None else None, int(align_corners),
                                          packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), od,
                                          ws.data_ptr(), ws.numel(), int(group_frames), B, N, C, H, W, V,
                                          _stream(feat))
    _lib.check(code, "mvn_unproject_v2v_front_ex")
    return out


# --------------------------------------------------------------------------- V2V head
# The pointwise tail of V2VModel (mvn/models/v2v.py:154-160): back_layers[1], back_layers[2]
# (Basic3DBlock(32, 32, 1)) and output_layer (Conv3d(32, J, 1)) as one kernel
# (csrc/v2v_head.hip), optionally with the 3D soft-argmax behind it.
HEAD_C = 32


def head_kslot(layer):
    """K-slot -> input channel of the packed weights of ``layer`` (0, 1, 2): the identity for the
    first layer; for the others slot 8g + j holds hidden channel 16 (j >> 2) + 4g + (j & 3), the
    channel an MFMA result leaves in that lane (mvn_hip.h, mvn_v2v_head)."""
    k = torch.arange(HEAD_C)
    if layer == 0:
        return k
    g, j = k // 8, k % 8
    return 16 * (j // 4) + 4 * g + (j % 4)


def _fold_conv_bn(conv, bn, what, ks, cout, cins):
    """(f64 weight, f64 scale, f64 shift) of an eval-mode Conv3d(cins -> cout, ks) + BatchNorm3d(cout)."""
    w = getattr(conv, "weight", None)
    want = " | ".join(map(str, cins))
    if not isinstance(conv, nn.Conv3d) or w.shape[0] != cout or w.shape[1] not in cins or tuple(w.shape[2:]) != (ks,) * 3:
        got = tuple(w.shape) if w is not None else type(conv).__name__
        raise RuntimeError(f"{what}: expected a ({cout}, {want}, {ks}, {ks}, {ks}) Conv3d weight, got {got}")
    pad = (ks - 1) // 2
    if tuple(conv.stride) != (1, 1, 1) or tuple(conv.padding) != (pad,) * 3 or tuple(conv.dilation) != (1, 1, 1):
        raise RuntimeError(f"{what}: expected stride 1, padding {pad} and no dilation")
    if bn.running_mean is None or tuple(bn.running_mean.shape) != (cout,):
        raise RuntimeError(f"{what}: expected a BatchNorm3d({cout}) with running statistics")
    return (_f64(w), *_bn_fold(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, cout))


def fold_v2v_head(block1, block2, output_conv, device="cuda"):
    """Two eval-mode ``Basic3DBlock(32, 32, 1)``-shaped modules (``.block[0]`` conv, ``.block[1]``
    BN) and a ``Conv3d(32, J, 1)`` -> (packed bf16 weights, scale_shift (2, 2, 32) f32, bias3 (J,)
    f32) on ``device``.  BN and the conv bias are folded in float64 as in ``fold_basic3d_block``;
    the weights are rounded to bf16 and packed [layer][m][lane][8] as mvn_v2v_head expects."""
    w1, s1, t1 = _fold_conv_bn(block1.block[0], block1.block[1], "block1", 1, HEAD_C, (HEAD_C,))
    w2, s2, t2 = _fold_conv_bn(block2.block[0], block2.block[1], "block2", 1, HEAD_C, (HEAD_C,))
    w3 = _f64(output_conv.weight)
    J = w3.shape[0]
    if w3.dim() != 5 or tuple(w3.shape[1:]) != (HEAD_C, 1, 1, 1) or not 1 <= J <= HEAD_C:
        raise RuntimeError(f"output_conv: expected a (J <= {HEAD_C}, {HEAD_C}, 1, 1, 1) Conv3d weight, "
                           f"got {tuple(w3.shape)}")
    w3p = torch.zeros(HEAD_C, HEAD_C, dtype=torch.float64)
    w3p[:J] = w3.reshape(J, HEAD_C)
    b3 = _f64(output_conv.bias) if output_conv.bias is not None else torch.zeros(J, dtype=torch.float64)
    # K-slot k of layer l reads input channel head_kslot(l)[k]
    layers = (w1.reshape(HEAD_C, HEAD_C), w2.reshape(HEAD_C, HEAD_C), w3p)
    packed = _pack_mfma_a(torch.stack([w[:, head_kslot(l)] for l, w in enumerate(layers)]))[:, 0]
    scale_shift = torch.stack([torch.stack([s1, t1]), torch.stack([s2, t2])]).float().contiguous()
    dev = torch.device(device)
    return packed.to(dev), scale_shift.to(dev), b3.float().to(dev)




def _head_input(what, x, packed, scale_shift, bias3, channels_last):
    """Checked, contiguous input of the head and its joint count."""
    _inference_only(what, x, packed, scale_shift, bias3,
                    instead="the model's own back_layers and output_layer, which autograd records")
    _dtype_code(x.dtype)
    ch = x.shape[-1] if channels_last else (x.shape[1] if x.dim() == 5 else -1)
    if x.dim() != 5 or ch != HEAD_C:
        want = f"(B, Vx, Vy, Vz, {HEAD_C})" if channels_last else f"(B, {HEAD_C}, Vx, Vy, Vz)"
        raise RuntimeError(f"{what}: x must be {want}, got {tuple(x.shape)}")
    if channels_last and x.dtype != torch.bfloat16:
        raise TypeError(f"{what}: a channels-last x must be bfloat16, got {x.dtype}")
    J = bias3.numel()
    if (tuple(packed.shape) != (3, 2, 64, 8) or packed.dtype != torch.bfloat16 or tuple(scale_shift.shape) != (2, 2, HEAD_C)
            or scale_shift.dtype != torch.float32 or bias3.dtype != torch.float32 or not 1 <= J <= HEAD_C):
        raise RuntimeError(f"{what}: packed, scale_shift, bias3 must be what fold_v2v_head returns")
    return x.contiguous(), packed.contiguous(), scale_shift.contiguous(), bias3.contiguous()


def v2v_head(x, packed, scale_shift, bias3, out_dtype=torch.float32, channels_last=False):
    """(B, 32, Vx, Vy, Vz) f32 | bf16 — or (B, Vx, Vy, Vz, 32) bf16 with ``channels_last`` — ->
    the logits (B, J, Vx, Vy, Vz) of back_layers[1], back_layers[2] and output_layer
    (v2v.py:154-160, eval mode), without the model's volume multiplier.  Inference-only."""
    from . import _ops
    od = _dtype_code(out_dtype)
    x, packed, scale_shift, bias3 = _head_input("v2v_head", x, packed, scale_shift, bias3, channels_last)
    return _ops.call(_ops.v2v_head, x, packed, scale_shift, bias3, od, bool(channels_last))


def v2v_head_softargmax(x, packed, scale_shift, bias3, coord_volumes, softmax=True, multiplier=1.0, out_dtype=None,
                        return_volumes=True, group_frames=0, channels_last=False):
    """``v2v_head`` then ``op.integrate_tensor_3d_with_coordinates(logits, coord_volumes, softmax,
    multiplier=multiplier)`` in one call (``mvn_v2v_head_softargmax``), pipelined over groups of
    ``group_frames`` frames through a workspace of one group's logits (default: within half of
    the MALL, 7 frames at 64^3 with J = 17).  Returns (keypoints (B, J, 3), volumes or None), the
    convention of ``op.integrate_tensor_3d_with_coordinates``; ``coord_volumes`` may be a
    ``volumetric.Cuboids``.  ``out_dtype`` (default float32) is the dtype of the returned
    volumes; a bfloat16 volume is formed from bfloat16 logits (the soft-argmax has no f32 ->
    bf16 form), everything else from float32 logits.  Equal bit for bit to the two steps with
    those logits.  Inference-only."""
    from . import _ops
    from .volumetric import Cuboids
    od = _dtype_code(out_dtype if out_dtype is not None else torch.float32)
    x, packed, scale_shift, bias3 = _head_input("v2v_head_softargmax", x, packed, scale_shift, bias3, channels_last)
    B, vol = _ops._head_dims(x, channels_last)
    if isinstance(coord_volumes, Cuboids):
        cub = coord_volumes
        if cub.shape != (B, *vol, 3):
            raise RuntimeError(f"cuboids {tuple(cub.shape)} do not match x {tuple(x.shape)}")
        coords, params, transfer = None, cub.params, cub.transfer
    else:
        coords, params, transfer = _ops.f32c(coord_volumes), None, False
        if tuple(coords.shape) != (B, *vol, 3):
            raise RuntimeError(f"coord_volumes {tuple(coords.shape)} does not match x {tuple(x.shape)}")
    xyz, out = _ops.call(_ops.v2v_head_softargmax, x, packed, scale_shift, bias3, coords, params, bool(transfer),
                         bool(softmax), float(multiplier), bool(return_volumes), od, int(group_frames),
                         bool(channels_last))
    return xyz, (out if return_volumes else None)


class V2VHead(nn.Module):
    """Eval-mode replacement of V2VModel's back_layers[1], back_layers[2] and output_layer with
    the 3D soft-argmax behind them: ``V2VHead.from_reference(m)(v2v_trunk(m, volumes),
    coord_volumes, volume_multiplier)`` replaces triangulation.py:352-353."""

    def __init__(self, packed, scale_shift, bias3):
        super().__init__()
        self.register_buffer("packed", packed)
        self.register_buffer("scale_shift", scale_shift)
        self.register_buffer("bias3", bias3)

    @classmethod
    def from_reference(cls, v2v_model, device="cuda"):
        return cls(*fold_v2v_head(v2v_model.back_layers[1], v2v_model.back_layers[2], v2v_model.output_layer,
                                  device=device))

    def forward(self, x, coord_volumes, multiplier=1.0, softmax=True):
        return v2v_head_softargmax(x, self.packed, self.scale_shift, self.bias3, coord_volumes, softmax=softmax,
                                   multiplier=multiplier)

    def forward_channels_last(self, x_cl, coord_volumes, multiplier=1.0, softmax=True):
        """``forward`` for a (B, Vx, Vy, Vz, 32) bf16 channels-last x."""
        return v2v_head_softargmax(x_cl, self.packed, self.scale_shift, self.bias3, coord_volumes, softmax=softmax,
                                   multiplier=multiplier, channels_last=True)


def v2v_trunk(v2v_model, x):
    """V2VModel.forward (v2v.py:164-169) up to the head: front_layers, encoder_decoder and
    back_layers[0], run with the model's own modules."""
    x = v2v_model.front_layers(x)
    x = v2v_model.encoder_decoder(x)
    return v2v_model.back_layers[0](x)


# --------------------------------------------------------------------------- Res3DBlocks and upsamples
# Res3DBlock (mvn/models/v2v.py:20-42) and Upsample3DBlock (:53-65) on channels-last bf16 volumes at
# the three channel widths of the V2V, each a 3x3x3 MFMA kernel of its own:
#   32   full resolution: front_layers[1..3], encoder_decoder.skip_res1, back_layers[0]
#        (csrc/v2v_res3d.hip)
#   64   first pooled level: encoder_pool1, encoder_res1, skip_res2, decoder_res1 and
#        decoder_upsample1 with the last ``+ skip_x1`` (csrc/v2v_interior.hip)
#   128  encoder_pool2 ... decoder_upsample2, at any extent D in [1, 64] (csrc/v2v_deep.hip,
#        DESIGN.md §4.14)
# One implementation of the folds, checks and calls serves all three through a ``_Level`` record;
# the public functions and modules of each width bind it.
RES_C = 32
WIDE_C = 64
UP_CIN, UP_COUT = 64, 32
DEEP_C = 128
DEEP_MAX_D = 64
SKIP_NONE, SKIP_IDENTITY, SKIP_POINTWISE = _lib.MVN_SKIP_NONE, _lib.MVN_SKIP_IDENTITY, _lib.MVN_SKIP_POINTWISE


class Res3DParams(NamedTuple):
    """What ``fold_res3d_block`` returns: the packed bf16 weights and f32 scale / shift of the two
    3x3x3 convs and, for a block with a 1x1x1 ``skip_con``, of the skip (else None: identity)."""
    packed1: torch.Tensor
    scale1: torch.Tensor
    shift1: torch.Tensor
    packed2: torch.Tensor
    scale2: torch.Tensor
    shift2: torch.Tensor
    skip_packed: Optional[torch.Tensor] = None
    skip_scale: Optional[torch.Tensor] = None
    skip_shift: Optional[torch.Tensor] = None


class UpsampleParams(NamedTuple):
    """What ``fold_upsample_block`` returns: packed bf16 weights and f32 scale / shift."""
    packed: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def _pack_taps(w):
    """(cout, cin, 3, 3, 3) float64 -> (27, K / 32, cout / 16, 64, 8) bf16, K = cin zero-padded to
    a multiple of 32, tap = (dx*3 + dy)*3 + dz."""
    cout, cin = w.shape[:2]
    return _pack_mfma_a(_pad_k(w.reshape(cout, cin, 27).permute(2, 0, 1)))            # rows cout, K-slots cin


def pack_conv3_weight(w):
    """(32, cin, 3, 3, 3) float64 -> (27, 2, 64, 8) bf16 as mvn_v2v_conv3 reads it:
    [tap = (dx*3 + dy)*3 + dz][m][lane][j] = w[16 m + (lane & 15)][8 (lane >> 4) + j][dx][dy][dz],
    zero where 8 (lane >> 4) + j >= cin (cin = 16: K zero-padded)."""
    return _pack_taps(w)[:, 0]


def pack_pointwise_skip_weight(w):
    """(32, 16) float64 -> (2, 64, 8) bf16: [m][lane][j] = w[16 m + (lane & 15)][8 (lane >> 4) + j],
    zero where 8 (lane >> 4) + j >= 16."""
    return _pack_mfma_a(_pad_k(w))[0]


def pack_conv3_wide_weight(w):
    """(64, cin, 3, 3, 3) float64, cin 32 | 64 -> (27, cin / 32, 4, 64, 8) bf16 as mvn_v2v_conv3_wide
    reads it: [tap = (dx*3 + dy)*3 + dz][kp][m][lane][j]
    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]."""
    return _pack_taps(w)


def pack_pointwise_skip_wide_weight(w):
    """(64, 32) float64 -> (4, 64, 8) bf16: [m][lane][j] = w[16 m + (lane & 15)][8 (lane >> 4) + j]."""
    return _pack_mfma_a(w)[0]


def pack_conv3_deep_weight(w):
    """(128, cin, 3, 3, 3) float64, cin 64 | 128 -> (27, cin / 32, 8, 64, 8) bf16 as mvn_v2v_conv3_deep
    reads it: [tap = (dx*3 + dy)*3 + dz][kp][m][lane][j]
    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]."""
    return _pack_taps(w)


def pack_pointwise_skip_deep_weight(w):
    """(128, 64) float64 -> (2, 8, 64, 8) bf16: [kp][m][lane][j]
    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]."""
    return _pack_mfma_a(w)


def pack_upsample_weight(w):
    """(64, 32, 2, 2, 2) float64 ConvTranspose3d weight -> (2, 16, 64, 8) bf16 as mvn_v2v_upsample2
    reads it: [kp][m][lane][j] = w[32 kp + 8 (lane >> 4) + j][16 (m & 1) + (lane & 15)][dx][dy][dz]
    with (dx*2 + dy)*2 + dz = m >> 1."""
    return pack_upsample_deep_weight(w)


def pack_upsample_deep_weight(w):
    """(128, cout, 2, 2, 2) float64 ConvTranspose3d weight, cout 64 | 128 -> (4, 8 cout / 16, 64, 8)
    bf16 as mvn_v2v_upsample2_deep reads it, with H = cout / 16 channel tiles per offset:
    [kp][m][lane][j] = w[32 kp + 8 (lane >> 4) + j][16 (m % H) + (lane & 15)][dx][dy][dz]
    with (dx*2 + dy)*2 + dz = m // H."""
    cin, cout = w.shape[:2]
    return _pack_mfma_a(w.reshape(cin, cout, 8).permute(2, 1, 0).reshape(8 * cout, cin))   # rows [offset][cout]


class _Level(NamedTuple):
    """One channel width of the Res3DBlock and upsample kernels: everything in which the folds,
    checks and calls of the three widths differ."""
    cout: int                  # a conv's output channels; it takes cout // 2 | cout, a pointwise skip cout // 2
    ax: str                    # the extent's letter in messages
    step: int                  # the extent is a multiple of ``step`` in [step, vmax]
    vmax: int
    conv_shape: dict           # a conv's input channels -> the shape of its packed weights
    skip_shape: tuple          # the shape of the packed pointwise-skip weights
    pack: Callable             # the packers of the two
    pack_skip: Callable
    op: str                    # the conv's custom op in ``_ops``, also its public name
    fold: str                  # the fold that messages cite
    up_couts: tuple = ()       # the upsample from this width: its output channels, op and fold
    up_op: str = ""
    up_fold: str = ""

    @property
    def cins(self):
        return (self.cout // 2, self.cout)


_RES = _Level(RES_C, "V", 16, 256, {16: (27, 2, 64, 8), 32: (27, 2, 64, 8)}, (2, 64, 8),
              pack_conv3_weight, pack_pointwise_skip_weight, "v2v_conv3", "fold_res3d_block")
_WIDE = _Level(WIDE_C, "V", 16, 128, {32: (27, 1, 4, 64, 8), 64: (27, 2, 4, 64, 8)}, (4, 64, 8),
               pack_conv3_wide_weight, pack_pointwise_skip_wide_weight, "v2v_conv3_wide", "fold_res3d_block_wide",
               (UP_COUT,), "v2v_upsample2", "fold_upsample_block")
_DEEP = _Level(DEEP_C, "D", 1, DEEP_MAX_D, {64: (27, 2, 8, 64, 8), 128: (27, 4, 8, 64, 8)}, (2, 8, 64, 8),
               pack_conv3_deep_weight, pack_pointwise_skip_deep_weight, "v2v_conv3_deep", "fold_res3d_block_deep",
               (64, 128), "v2v_upsample2_deep", "fold_upsample_block_deep")


def _one_of(values):
    return " | ".join(map(str, values))


def _fold_res3d(lv, block, device):
    """``fold_res3d_block*``: the two 3x3x3 convs and the 1x1x1 ``skip_con`` of a Res3DBlock with
    ``lv``'s channels, BN and biases folded in float64, as ``Res3DParams`` on ``device``."""
    rb, sk = getattr(block, "res_branch", None), getattr(block, "skip_con", None)
    if rb is None or sk is None or len(rb) != 5 or len(sk) not in (0, 2):
        raise RuntimeError("expected a module with Res3DBlock's res_branch of 5 modules and skip_con of 0 or 2, got "
                           + type(block).__name__)
    C, dev = lv.cout, torch.device(device)
    w1, s1, t1 = _fold_conv_bn(rb[0], rb[1], "res_branch[0]", 3, C, lv.cins)
    w2, s2, t2 = _fold_conv_bn(rb[3], rb[4], "res_branch[3]", 3, C, (C,))
    cin = w1.shape[1]
    skip = (None, None, None)
    if len(sk) == 2:
        ws, ss, ts = _fold_conv_bn(sk[0], sk[1], "skip_con[0]", 1, C, (C // 2,))
        if cin != C // 2:
            raise RuntimeError(f"a block with a 1x1x1 skip_con must take {C // 2} channels, got {cin}")
        skip = (lv.pack_skip(ws.reshape(C, C // 2)).to(dev), ss.float().to(dev), ts.float().to(dev))
    elif cin != C:
        raise RuntimeError(f"a block with an empty skip_con must take {C} channels, got {cin}")
    return Res3DParams(lv.pack(w1).to(dev), s1.float().to(dev), t1.float().to(dev),
                       lv.pack(w2).to(dev), s2.float().to(dev), t2.float().to(dev), *skip)


def _fold_upsample(lv, block, device):
    """``fold_upsample_block*``: the ConvTranspose3d(lv.cout, lv.up_couts, 2, stride 2) and the
    BatchNorm3d of an Upsample3DBlock, folded in float64, as ``UpsampleParams`` on ``device``."""
    seq = getattr(block, "block", None)
    if seq is None or len(seq) != 3 or not isinstance(seq[0], nn.ConvTranspose3d):
        raise RuntimeError("expected block = [ConvTranspose3d, BatchNorm3d, ReLU]")
    conv, bn = seq[0], seq[1]
    w = _f64(conv.weight)
    if w.dim() != 5 or w.shape[0] != lv.cout or w.shape[1] not in lv.up_couts or tuple(w.shape[2:]) != (2, 2, 2):
        raise RuntimeError(f"block[0]: expected a ({lv.cout}, {_one_of(lv.up_couts)}, 2, 2, 2) ConvTranspose3d weight, "
                           f"got {tuple(w.shape)}")
    cout = w.shape[1]
    if (tuple(conv.stride) != (2, 2, 2) or tuple(conv.padding) != (0, 0, 0) or tuple(conv.output_padding) != (0, 0, 0)
            or tuple(conv.dilation) != (1, 1, 1) or conv.groups != 1):
        raise RuntimeError("block[0]: expected stride 2, no padding, no output padding, no dilation, one group")
    if bn.running_mean is None or tuple(bn.running_mean.shape) != (cout,):
        raise RuntimeError(f"block[1]: expected a BatchNorm3d({cout}) with running statistics")
    s, shift = _bn_fold(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, cout)
    dev = torch.device(device)
    return UpsampleParams(pack_upsample_deep_weight(w).to(dev), s.float().to(dev), shift.float().to(dev))


def _volume(lv, what, x, name, channels, vmax=None):
    """Checked contiguous (B, V, V, V, C) bf16 volume of ``lv``'s kernels, C one of ``channels``."""
    a, vmax = lv.ax, vmax or lv.vmax
    if x.dtype != torch.bfloat16:
        raise TypeError(f"{what}: {name} must be bfloat16, got {x.dtype}")
    s = x.shape                                                 # one torch.Size per check: this runs per launch
    if len(s) != 5 or s[4] not in channels or not s[1] == s[2] == s[3]:
        raise RuntimeError(f"{what}: {name} must be (B, {a}, {a}, {a}, {_one_of(channels)}), got {tuple(s)}")
    V = s[1]
    if V % lv.step != 0 or not lv.step <= V <= vmax:
        rule = f"in [1, {vmax}]" if lv.step == 1 else f"a multiple of {lv.step} in [{lv.step}, {vmax}]"
        raise RuntimeError(f"{what}: {name}: {a} must be {rule}, got {V}")
    return x.contiguous()


def _folded(what, packed, scale, shift, shape, channels, fold):
    """Checked contiguous (packed weights, scale, shift) as ``fold`` returns them."""
    if (packed.shape != shape or packed.dtype != torch.bfloat16 or scale.shape != (channels,) or shift.shape != (channels,)
            or scale.dtype != torch.float32 or shift.dtype != torch.float32):
        raise RuntimeError(f"{what}: packed weights {shape}, scale and shift ({channels},) must be what {fold} returns")
    return packed.contiguous(), scale.contiguous(), shift.contiguous()


def _conv3(lv, x_cl, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift):
    """``v2v_conv3*``: the checks of one conv launch and the call of ``lv.op``."""
    from . import _ops
    what, C = lv.op, lv.cout
    _inference_only(what, x_cl, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift,
                    instead="the model's own Res3DBlock, which autograd records")
    x = _volume(lv, what, x_cl, "x_cl", lv.cins)
    packed, scale, shift = _folded(what, packed, scale, shift, lv.conv_shape[x.shape[4]], C, lv.fold)
    pw = (skip_packed, skip_scale, skip_shift)
    if skip is None:
        if any(t is not None for t in pw):
            raise RuntimeError(f"{what}: skip weights without a skip volume")
        mode = SKIP_NONE
    else:
        mode = SKIP_POINTWISE if skip_packed is not None else SKIP_IDENTITY
        skip = _volume(lv, what, skip, "skip", (C // 2,) if mode == SKIP_POINTWISE else (C,))
        if skip.shape[:4] != x.shape[:4]:
            raise RuntimeError(f"{what}: skip {tuple(skip.shape)} does not match x_cl {tuple(x.shape)}")
        if mode == SKIP_POINTWISE:
            if skip_scale is None or skip_shift is None:
                raise RuntimeError(f"{what}: a pointwise skip needs skip_packed, skip_scale and skip_shift")
            pw = _folded(what, skip_packed, skip_scale, skip_shift, lv.skip_shape, C, lv.fold)
        elif any(t is not None for t in pw):
            raise RuntimeError(f"{what}: an identity skip takes no skip_scale / skip_shift")
    return _ops.call(getattr(_ops, lv.op), x, packed, scale, shift, mode, skip, *pw)


def _res3d_two_launches(lv, what, x_cl, params):
    """``res3d_block_wide`` / ``_deep``: conv1, then conv2 with the block's input as its skip."""
    p = Res3DParams(*params)
    _inference_only(what, x_cl, *p, instead="the model's own Res3DBlock, which autograd records")
    pointwise = p.skip_packed is not None
    x = _volume(lv, what, x_cl, "x_cl", (lv.cout // 2,) if pointwise else (lv.cout,))
    h = _conv3(lv, x, p.packed1, p.scale1, p.shift1, None, None, None, None)
    if not pointwise and (p.skip_scale is not None or p.skip_shift is not None):
        raise RuntimeError(f"{what}: an identity skip takes no skip_scale / skip_shift")
    return _conv3(lv, h, p.packed2, p.scale2, p.shift2, x, p.skip_packed, p.skip_scale, p.skip_shift)


def _upsample2_add(lv, what, x_cl, params, skip):
    """``upsample2_add*``: the checks of one upsample launch and the call of ``lv.up_op``."""
    from . import _ops
    p = UpsampleParams(*params)
    _inference_only(what, x_cl, *p, skip, instead="the model's own Upsample3DBlock, which autograd records")
    x = _volume(lv, what, x_cl, "x_cl", (lv.cout,))
    cout = p.scale.shape[0] if p.scale.dim() == 1 else -1
    if cout not in lv.up_couts:
        raise RuntimeError(f"{what}: scale and shift must be ({_one_of(lv.up_couts)},), got {tuple(p.scale.shape)}")
    packed, scale, shift = _folded(what, p.packed, p.scale, p.shift, (lv.cout // 32, cout // 2, 64, 8), cout, lv.up_fold)
    if skip is not None:
        skip = _volume(lv, what, skip, "skip", (cout,), vmax=2 * lv.vmax)
        B, V = x.shape[:2]
        if skip.shape[:4] != (B, 2 * V, 2 * V, 2 * V):
            raise RuntimeError(f"{what}: skip {tuple(skip.shape)} does not match x_cl {tuple(x.shape)} upsampled")
    return _ops.call(getattr(_ops, lv.up_op), x, packed, scale, shift, skip)


class _Res3DBlockCL(nn.Module):
    """Base of the ``Res3DBlock*CL`` modules: the ``Res3DParams`` as buffers of their names;
    a subclass sets its fold and its forward."""
    _fold = None

    def __init__(self, params):
        super().__init__()
        for name, t in zip(Res3DParams._fields, Res3DParams(*params)):
            self.register_buffer(name, t)

    @classmethod
    def from_reference(cls, block, device="cuda"):
        return cls(cls._fold(block, device=device))

    @property
    def params(self):
        return Res3DParams(*(getattr(self, name) for name in Res3DParams._fields))


class _Upsample3DBlockCL(nn.Module):
    """Base of the ``Upsample3DBlock*CL`` modules: the ``UpsampleParams`` as buffers of their names."""
    _fold = None

    def __init__(self, params):
        super().__init__()
        for name, t in zip(UpsampleParams._fields, UpsampleParams(*params)):
            self.register_buffer(name, t)

    @classmethod
    def from_reference(cls, block, device="cuda"):
        return cls(cls._fold(block, device=device))

    @property
    def params(self):
        return UpsampleParams(self.packed, self.scale, self.shift)


# ---- 32 channels, full resolution
def fold_res3d_block(block, device="cuda"):
    """An eval-mode module with Res3DBlock's attributes (``res_branch[0..4]`` = conv, BN, ReLU,
    conv, BN; ``skip_con`` empty or [conv 1x1x1, BN]) with 16 | 32 -> 32 channels -> ``Res3DParams``
    on ``device``.  BN and the conv biases are folded in float64 as in ``fold_basic3d_block``; the
    weights are rounded to bf16 and packed as mvn_v2v_conv3 expects (``pack_conv3_weight``)."""
    return _fold_res3d(_RES, block, device)


def v2v_conv3(x_cl, packed, scale, shift, skip=None, skip_packed=None, skip_scale=None, skip_shift=None):
    """(B, V, V, V, 16 | 32) bf16 channels-last -> (B, V, V, V, 32) bf16: one launch of
    relu(bn(conv3d_3(x)) + skip term) (mvn_v2v_conv3, eval mode).  Without ``skip`` there is no
    residual; ``skip`` (B, V, V, V, 32) alone is added as it is (identity); ``skip`` (B, V, V, V, 16)
    with ``skip_packed``, ``skip_scale``, ``skip_shift`` goes through its folded 1x1x1 conv + BN.
    V is a multiple of 16 in [16, 256].  Non-finite voxels follow torch (mvn_hip.h).
    Inference-only."""
    return _conv3(_RES, x_cl, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift)


def res3d_block(x_cl, params, group_frames=0):
    """A whole eval-mode Res3DBlock (v2v.py:20-42) in one call (``mvn_v2v_res3d``): x_cl
    (B, V, V, V, 16 | 32) bf16 channels-last -> (B, V, V, V, 32) bf16, ``params`` from
    ``fold_res3d_block``.  conv1 writes one frame group's hidden volume into a workspace
    (``group_frames`` <= 0: the default, within half of the MALL, 8 frames at V = 64), conv2 reads
    it with the block's input as its skip.  Equal bit for bit to the two ``v2v_conv3`` launches on
    the whole batch.  Inference-only."""
    from . import _ops
    what, lv = "res3d_block", _RES
    p = Res3DParams(*params)
    _inference_only(what, x_cl, *p, instead="the model's own Res3DBlock, which autograd records")
    pointwise = p.skip_packed is not None
    x = _volume(lv, what, x_cl, "x_cl", (16,) if pointwise else (32,))
    c1 = _folded(what, p.packed1, p.scale1, p.shift1, lv.conv_shape[x.shape[4]], RES_C, lv.fold)
    c2 = _folded(what, p.packed2, p.scale2, p.shift2, lv.conv_shape[RES_C], RES_C, lv.fold)
    if pointwise:
        if p.skip_scale is None or p.skip_shift is None:
            raise RuntimeError(f"{what}: a pointwise skip needs skip_packed, skip_scale and skip_shift")
        sk = _folded(what, p.skip_packed, p.skip_scale, p.skip_shift, lv.skip_shape, RES_C, lv.fold)
    else:
        sk = (None, None, None)
    return _ops.call(_ops.v2v_res3d, x, *c1, *c2, *sk, int(group_frames))


class Res3DBlockCL(_Res3DBlockCL):
    """Eval-mode replacement of a full-resolution Res3DBlock(16 | 32, 32) on a channels-last bf16
    volume: ``Res3DBlockCL.from_reference(block)(x_cl)``."""
    _fold = staticmethod(fold_res3d_block)

    def forward(self, x_cl, group_frames=0):
        return res3d_block(x_cl, self.params, group_frames)


# ---- 64 channels, first pooled level
def max_pool2_cl(x_cl):
    """(B, V, V, V, C) bf16 channels-last -> (B, V/2, V/2, V/2, C): ``F.max_pool3d(x, 2, 2)`` bit
    for bit (mvn_v2v_maxpool2), NaN, infinities and signed zeros included.  V is even in [2, 256],
    C a multiple of 8 up to 128; a non-contiguous ``x_cl`` is copied.  Inference-only."""
    from . import _ops
    what = "max_pool2_cl"
    _inference_only(what, x_cl, instead="torch.nn.functional.max_pool3d, which autograd records")
    if x_cl.dtype != torch.bfloat16:
        raise TypeError(f"{what}: x_cl must be bfloat16, got {x_cl.dtype}")
    if x_cl.dim() != 5 or len(set(x_cl.shape[1:4])) != 1:
        raise RuntimeError(f"{what}: x_cl must be (B, V, V, V, C), got {tuple(x_cl.shape)}")
    V, C = x_cl.shape[1], x_cl.shape[4]
    if V % 2 != 0 or not 2 <= V <= 256:
        raise RuntimeError(f"{what}: V must be even in [2, 256], got {V}")
    if C % 8 != 0 or not 8 <= C <= 128:
        raise RuntimeError(f"{what}: C must be a multiple of 8 in [8, 128], got {C}")
    return _ops.call(_ops.v2v_maxpool2, x_cl.contiguous())


def fold_res3d_block_wide(block, device="cuda"):
    """An eval-mode module with Res3DBlock's attributes and 32 | 64 -> 64 channels (``skip_con``
    [conv 1x1x1, BN] for 32, empty for 64) -> ``Res3DParams`` on ``device``: folded in float64
    exactly as ``fold_res3d_block``, packed as mvn_v2v_conv3_wide expects
    (``pack_conv3_wide_weight``, ``pack_pointwise_skip_wide_weight``)."""
    return _fold_res3d(_WIDE, block, device)


def fold_upsample_block(block, device="cuda"):
    """An eval-mode module with Upsample3DBlock's attributes (``block[0..2]`` = ConvTranspose3d(64,
    32, 2, stride 2), BatchNorm3d(32), ReLU) -> ``UpsampleParams`` on ``device``: the ConvTranspose
    bias and the BN folded in float64, the weights rounded to bf16 and packed as
    mvn_v2v_upsample2 expects (``pack_upsample_weight``)."""
    return _fold_upsample(_WIDE, block, device)


def v2v_conv3_wide(x_cl, packed, scale, shift, skip=None, skip_packed=None, skip_scale=None, skip_shift=None):
    """(B, V, V, V, 32 | 64) bf16 channels-last -> (B, V, V, V, 64) bf16: one launch of
    relu(bn(conv3d_3(x)) + skip term) (mvn_v2v_conv3_wide, eval mode).  Without ``skip`` there is
    no residual; ``skip`` (B, V, V, V, 64) alone is added as it is (identity); ``skip``
    (B, V, V, V, 32) with ``skip_packed``, ``skip_scale``, ``skip_shift`` goes through its folded
    1x1x1 conv + BN.  V is a multiple of 16 in [16, 128].  Non-finite voxels follow torch
    (mvn_hip.h).  Inference-only."""
    return _conv3(_WIDE, x_cl, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift)


def res3d_block_wide(x_cl, params):
    """A whole eval-mode Res3DBlock(32 | 64, 64) as two ``v2v_conv3_wide`` launches: x_cl
    (B, V, V, V, 32 | 64) bf16 channels-last -> (B, V, V, V, 64) bf16, ``params`` from
    ``fold_res3d_block_wide``.  The hidden volume is a torch allocation (4.2 MB per frame at 32^3).
    Inference-only."""
    return _res3d_two_launches(_WIDE, "res3d_block_wide", x_cl, params)


class Res3DBlockWideCL(_Res3DBlockCL):
    """Eval-mode replacement of a Res3DBlock(32 | 64, 64) on a channels-last bf16 volume:
    ``Res3DBlockWideCL.from_reference(block)(x_cl)``."""
    _fold = staticmethod(fold_res3d_block_wide)

    def forward(self, x_cl):
        return res3d_block_wide(x_cl, self.params)


def upsample2_add(x_cl, params, skip=None):
    """(B, V, V, V, 64) bf16 channels-last -> (B, 2V, 2V, 2V, 32) bf16: an eval-mode
    Upsample3DBlock(64, 32) and the ``+ skip`` behind it in one launch (mvn_v2v_upsample2):
    bf16(relu(bn(conv_transpose(x))) + skip), the ReLU before the add, one rounding.  ``params``
    from ``fold_upsample_block``; ``skip`` (B, 2V, 2V, 2V, 32) bf16, or None for no add.  V is a
    multiple of 16 in [16, 128].  Inference-only."""
    return _upsample2_add(_WIDE, "upsample2_add", x_cl, params, skip)


class Upsample3DBlockCL(_Upsample3DBlockCL):
    """Eval-mode replacement of Upsample3DBlock(64, 32) with the ``+ skip`` behind it."""
    _fold = staticmethod(fold_upsample_block)

    def forward(self, x_cl, skip=None):
        return upsample2_add(x_cl, self.params, skip)


# ---- 128 channels, the levels below
def fold_res3d_block_deep(block, device="cuda"):
    """An eval-mode module with Res3DBlock's attributes and 64 | 128 -> 128 channels (``skip_con``
    [conv 1x1x1, BN] for 64, empty for 128) -> ``Res3DParams`` on ``device``: folded in float64
    exactly as ``fold_res3d_block_wide``, packed as mvn_v2v_conv3_deep expects
    (``pack_conv3_deep_weight``, ``pack_pointwise_skip_deep_weight``)."""
    return _fold_res3d(_DEEP, block, device)


def fold_upsample_block_deep(block, device="cuda"):
    """An eval-mode module with Upsample3DBlock's attributes (``block[0..2]`` = ConvTranspose3d(128,
    64 | 128, 2, stride 2), BatchNorm3d, ReLU) -> ``UpsampleParams`` on ``device``: the ConvTranspose
    bias and the BN folded in float64, the weights rounded to bf16 and packed as
    mvn_v2v_upsample2_deep expects (``pack_upsample_deep_weight``)."""
    return _fold_upsample(_DEEP, block, device)


def v2v_conv3_deep(x_cl, packed, scale, shift, skip=None, skip_packed=None, skip_scale=None, skip_shift=None):
    """(B, D, D, D, 64 | 128) bf16 channels-last -> (B, D, D, D, 128) bf16: one launch of
    relu(bn(conv3d_3(x)) + skip term) (mvn_v2v_conv3_deep, eval mode).  Without ``skip`` there is
    no residual; ``skip`` (B, D, D, D, 128) alone is added as it is (identity); ``skip``
    (B, D, D, D, 64) with ``skip_packed``, ``skip_scale``, ``skip_shift`` goes through its folded
    1x1x1 conv + BN.  D is any integer in [1, 64].  Non-finite voxels follow torch (mvn_hip.h);
    two calls on the same data return the same bits.  Inference-only."""
    return _conv3(_DEEP, x_cl, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift)


def res3d_block_deep(x_cl, params):
    """A whole eval-mode Res3DBlock(64 | 128, 128) as two ``v2v_conv3_deep`` launches: x_cl
    (B, D, D, D, 64 | 128) bf16 channels-last -> (B, D, D, D, 128) bf16, ``params`` from
    ``fold_res3d_block_deep``.  The hidden volume is a torch allocation (1 MB per frame at 16^3).
    Inference-only."""
    return _res3d_two_launches(_DEEP, "res3d_block_deep", x_cl, params)


class Res3DBlockDeepCL(_Res3DBlockCL):
    """Eval-mode replacement of a Res3DBlock(64 | 128, 128) on a channels-last bf16 volume:
    ``Res3DBlockDeepCL.from_reference(block)(x_cl)``."""
    _fold = staticmethod(fold_res3d_block_deep)

    def forward(self, x_cl):
        return res3d_block_deep(x_cl, self.params)


def upsample2_add_deep(x_cl, params, skip=None):
    """(B, D, D, D, 128) bf16 channels-last -> (B, 2D, 2D, 2D, cout) bf16, cout 64 | 128: an
    eval-mode Upsample3DBlock(128, cout) and the ``+ skip`` behind it in one launch
    (mvn_v2v_upsample2_deep): bf16(relu(bn(conv_transpose(x))) + skip), the ReLU before the add, one
    rounding.  ``params`` from ``fold_upsample_block_deep``; ``skip`` (B, 2D, 2D, 2D, cout) bf16, or
    None for no add.  D is any integer in [1, 64].  Inference-only."""
    return _upsample2_add(_DEEP, "upsample2_add_deep", x_cl, params, skip)


class Upsample3DBlockDeepCL(_Upsample3DBlockCL):
    """Eval-mode replacement of Upsample3DBlock(128, 64 | 128) with the ``+ skip`` behind it."""
    _fold = staticmethod(fold_upsample_block_deep)

    def forward(self, x_cl, skip=None):
        return upsample2_add_deep(x_cl, self.params, skip)




# the folded modules of ``V2VEval.deep`` in the order ``v2v_interior_deep_cl`` takes them
DEEP_RES = ("encoder_res2", "skip_res3", "encoder_res3", "skip_res4", "encoder_res4", "skip_res5", "encoder_res5",
            "mid_res", "decoder_res5", "decoder_res4", "decoder_res3", "decoder_res2")
DEEP_UP = ("decoder_upsample5", "decoder_upsample4", "decoder_upsample3", "decoder_upsample2")


def fold_deep_levels(encoder_decoder, device="cuda"):
    """The Res3DBlocks ``DEEP_RES`` and the upsamples ``DEEP_UP`` of an EncoderDecorder as
    ``Res3DBlockDeepCL`` and ``Upsample3DBlockDeepCL``, in that order: what ``v2v_interior_deep_cl``
    takes."""
    ed = encoder_decoder
    return ([Res3DBlockDeepCL.from_reference(getattr(ed, name), device=device) for name in DEEP_RES]
            + [Upsample3DBlockDeepCL.from_reference(getattr(ed, name), device=device) for name in DEEP_UP])


def v2v_interior_deep_cl(deep, e1_cl, s2_cl):
    """The data flow of ``v2v_interior_deep`` on channels-last bf16 volumes with the folded modules
    ``deep`` (``fold_deep_levels``): e1_cl (B, D, D, D, 64), ``encoder_res1``'s output, and s2_cl,
    ``skip_res2``'s output of the same shape -> (B, D, D, D, 64) with ``+ skip_x2`` already added:
    every ``+ skip`` is fused into the upsample before it.  D is a multiple of 16 up to 128 (four
    pools; the deepest level is D / 16).  No torch arithmetic: pools, ``res3d_block_deep`` and
    ``upsample2_add_deep`` only."""
    if len(deep) != len(DEEP_RES) + len(DEEP_UP):
        raise RuntimeError(f"expected the {len(DEEP_RES) + len(DEEP_UP)} modules of fold_deep_levels, got {len(deep)}")
    (encoder_res2, skip_res3, encoder_res3, skip_res4, encoder_res4, skip_res5, encoder_res5, mid_res,
     decoder_res5, decoder_res4, decoder_res3, decoder_res2, up5, up4, up3, up2) = deep
    x = encoder_res2(max_pool2_cl(e1_cl))
    s3 = skip_res3(x)
    x = encoder_res3(max_pool2_cl(x))
    s4 = skip_res4(x)
    x = encoder_res4(max_pool2_cl(x))
    s5 = skip_res5(x)
    x = encoder_res5(max_pool2_cl(x))
    x = mid_res(x)
    x = up5(decoder_res5(x), s5)
    x = up4(decoder_res4(x), s4)
    x = up3(decoder_res3(x), s3)
    return up2(decoder_res2(x), s2_cl)


def v2v_interior_deep(encoder_decoder, x):
    """EncoderDecorder.forward (v2v.py:108-132) from ``encoder_pool2`` through
    ``decoder_upsample2``: the levels below the first pooled one (16^3 and below at V = 64, 128
    channels), with the model's own modules.  x is ``encoder_res1``'s output (B, 64, V/2, V/2,
    V/2); the result has its shape and still lacks ``+ skip_x2``."""
    ed = encoder_decoder
    x = ed.encoder_res2(ed.encoder_pool2(x))
    s3 = ed.skip_res3(x)
    x = ed.encoder_res3(ed.encoder_pool3(x))
    s4 = ed.skip_res4(x)
    x = ed.encoder_res4(ed.encoder_pool4(x))
    s5 = ed.skip_res5(x)
    x = ed.encoder_res5(ed.encoder_pool5(x))
    x = ed.mid_res(x)
    x = ed.decoder_upsample5(ed.decoder_res5(x)) + s5
    x = ed.decoder_upsample4(ed.decoder_res4(x)) + s4
    x = ed.decoder_upsample3(ed.decoder_res3(x)) + s3
    return ed.decoder_upsample2(ed.decoder_res2(x))


def v2v_interior(encoder_decoder, x):
    """The pooled part of EncoderDecorder.forward (v2v.py:105-135): everything between skip_res1
    and the last ``+ skip_x1``, 32^3 and below at V = 64, with the model's own modules."""
    ed = encoder_decoder
    x = ed.encoder_res1(ed.encoder_pool1(x))
    s2 = ed.skip_res2(x)
    x = v2v_interior_deep(ed, x) + s2
    return ed.decoder_upsample1(ed.decoder_res1(x))


class V2VEval(nn.Module):
    """The whole eval-mode V2VModel (v2v.py:141-169) with the 3D soft-argmax behind it, every
    full-resolution layer on this package's kernels: ``V2VEval.from_reference(m)(vol_cl,
    coord_volumes, volume_multiplier)`` replaces triangulation.py:352-353 for the channels-last
    bf16 volume of ``unproject_channels_last``.  Data flow and what each torch glue step costs
    per frame at V = 64:

    1. ``v2v_front`` with bf16 output (B, 16, V, V, V), then one torch permute to channels-last:
       an extra read and write of the 16-channel volume (2 x 8.4 MB);
    2. ``front_layers[1..3]`` and ``encoder_decoder.skip_res1``: ``res3d_block`` (this kernel);
    3. the pooled interior (``encoder_pool1`` ... ``decoder_upsample1``, 32^3 and below) with the
       model's own torch modules in ``interior_dtype`` on an NCDHW view of the channels-last
       volume: the cast reads 16.8 MB of bf16 and writes the volume in ``interior_dtype``, and
       the modules make whatever layout copies their backend wants;
    4. ``+ skip_x1`` in ``interior_dtype`` and the cast back to channels-last bf16: two more
       passes over a 32-channel volume (read 33.6 MB + 16.8 MB, write 33.6 MB; read 33.6 MB,
       write 16.8 MB, for float32);
    5. ``back_layers[0]``: ``res3d_block``;
    6. ``v2v_head_softargmax(channels_last=True)``.

    With ``from_reference(..., half_res="kernels")`` steps 3 and 4 shrink to the levels below the
    first pooled one: ``max_pool2_cl``, ``encoder_res1``, ``skip_res2`` and ``decoder_res1`` as
    ``res3d_block_wide`` and ``decoder_upsample1`` with ``+ skip_x1`` as ``upsample2_add`` run on
    kernels, and the torch glue (cast to NCDHW ``interior_dtype``, ``+ skip_x2``,
    cast back) touches (B, V/2, V/2, V/2, 64) volumes only, an eighth of the traffic above.

    With ``deep="kernels"`` on top of that the levels below run on kernels too
    (``v2v_interior_deep_cl``: ``max_pool2_cl``, ``res3d_block_deep`` and ``upsample2_add_deep`` with
    every ``+ skip`` fused): steps 3 and 4 are gone, ``interior`` is None and no
    ``torch.nn`` module runs.  V is then a multiple of 32.

    The interior modules are a copy of the model's (its parameters frozen), so later changes to
    the model do not reach this module.  Inference-only."""

    def __init__(self, front, front_res, skip_res1, interior, back_res, head, interior_dtype=torch.float32,
                 half_res=None, deep=None):
        super().__init__()
        self.front, self.front_res, self.skip_res1 = front, nn.ModuleList(front_res), skip_res1
        self.interior, self.back_res, self.head = interior, back_res, head
        self.interior_dtype = interior_dtype
        # half_res="kernels": (encoder_res1, skip_res2, decoder_res1, decoder_upsample1) on the
        # kernels of the first pooled level; None: that level runs in ``interior`` (torch)
        self.half_res = nn.ModuleList(half_res) if half_res is not None else None
        # deep="kernels": the folded modules of ``fold_deep_levels`` (the 128-channel levels on
        # kernels, ``interior`` is None then); None: those levels run in ``interior`` (torch)
        self.deep = nn.ModuleList(deep) if deep is not None else None

    @classmethod
    def from_reference(cls, v2v_model, interior_dtype=torch.float32, device="cuda", half_res="torch", deep="torch"):
        """``half_res="torch"`` (the default) runs the whole pooled interior with the model's torch
        modules; ``"kernels"`` runs its first level (V/2, 64 channels) and both of its boundaries on
        this package's kernels and leaves the levels below to torch.
        ``deep="kernels"`` (with ``half_res="kernels"`` only) runs those levels on kernels as well
        (DESIGN.md §4.14): ``self.deep`` holds their folded modules, ``self.interior`` is None and no
        torch module is left."""
        import copy
        if half_res not in ("torch", "kernels"):
            raise ValueError(f"half_res must be 'torch' or 'kernels', got {half_res!r}")
        if deep not in ("torch", "kernels"):
            raise ValueError(f"deep must be 'torch' or 'kernels', got {deep!r}")
        if deep == "kernels" and half_res != "kernels":
            raise ValueError(f"deep='kernels' requires half_res='kernels', got half_res={half_res!r}")
        fl, ed = v2v_model.front_layers, v2v_model.encoder_decoder
        if len(fl) != 4:
            raise RuntimeError(f"expected front_layers of 4 modules, got {len(fl)}")
        interior = copy.deepcopy(ed).eval().to(device=device, dtype=interior_dtype).requires_grad_(False)
        del interior.skip_res1                              # runs on the kernel
        half = None
        if half_res == "kernels":
            half = [Res3DBlockWideCL.from_reference(ed.encoder_res1, device=device),
                    Res3DBlockWideCL.from_reference(ed.skip_res2, device=device),
                    Res3DBlockWideCL.from_reference(ed.decoder_res1, device=device),
                    Upsample3DBlockCL.from_reference(ed.decoder_upsample1, device=device)]
            for name in ("encoder_res1", "skip_res2", "decoder_res1", "decoder_upsample1"):
                delattr(interior, name)                     # run on the kernels
        deep_modules = None
        if deep == "kernels":
            deep_modules, interior = fold_deep_levels(ed, device=device), None
        return cls(Basic3DBlockFront.from_reference(fl[0], device=device),
                   [Res3DBlockCL.from_reference(fl[i], device=device) for i in (1, 2, 3)],
                   Res3DBlockCL.from_reference(ed.skip_res1, device=device), interior,
                   Res3DBlockCL.from_reference(v2v_model.back_layers[0], device=device),
                   V2VHead.from_reference(v2v_model, device=device), interior_dtype, half, deep_modules)

    def trunk(self, vol_cl):
        """(B, V, V, V, 32) bf16 unprojected volume -> the (B, V, V, V, 32) bf16 input of the head."""
        _inference_only("V2VEval", vol_cl, instead="the model's own modules, which autograd records")
        h = self.front(vol_cl, torch.bfloat16).permute(0, 2, 3, 4, 1).contiguous()
        for blk in self.front_res:
            h = blk(h)
        skip_x1 = self.skip_res1(h)
        if self.half_res is not None:
            # no torch pass over a full-resolution volume: the glue below touches (B, V/2, V/2,
            # V/2, 64) volumes only
            encoder_res1, skip_res2, decoder_res1, upsample1 = self.half_res
            e1 = encoder_res1(max_pool2_cl(h))
            s2 = skip_res2(e1)
            if self.deep is not None:
                # no torch arithmetic at all between the pool and back_layers[0]
                return self.back_res(upsample1(decoder_res1(v2v_interior_deep_cl(self.deep, e1, s2)), skip_x1))
            d = v2v_interior_deep(self.interior, e1.permute(0, 4, 1, 2, 3).to(self.interior_dtype))
            d = d + s2.permute(0, 4, 1, 2, 3)
            d1 = decoder_res1(d.permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous())
            return self.back_res(upsample1(d1, skip_x1))
        x = v2v_interior(self.interior, h.permute(0, 4, 1, 2, 3).to(self.interior_dtype))
        x = x + skip_x1.permute(0, 4, 1, 2, 3)
        return self.back_res(x.permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous())

    def forward(self, vol_cl, coord_volumes, multiplier=1.0, softmax=True):
        """(keypoints (B, J, 3), volumes (B, J, V, V, V)) as ``op.integrate_tensor_3d_with_coordinates``
        of the model's output times ``multiplier``."""
        return self.head.forward_channels_last(self.trunk(vol_cl), coord_volumes, multiplier, softmax)
