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
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._ops import _require_gpu, _stream
from .op import _dtype_code, aggregation_code, unproject_inputs

CIN, COUT, KS = 32, 16, 7


def fold_basic3d_block(weight, bias, bn_weight, bn_bias, running_mean, running_var, eps=1e-5, device="cuda"):
    """Eval-mode Basic3DBlock parameters -> (packed bf16 weights, scale, shift) on ``device``.

    y = relu(bn(conv(x) + bias)) = relu(conv(x) * s + ((bias - mean) * s + beta)),
    s = gamma / sqrt(var + eps), folded in float64.  The weights are rounded to bf16 (the
    kernel's MFMA operand type) and packed [tap][lane][8] as mvn_v2v_front expects."""
    w = weight.detach().to(torch.float64).cpu()
    if tuple(w.shape) != (COUT, CIN, KS, KS, KS):
        raise RuntimeError(f"expected a ({COUT}, {CIN}, 7, 7, 7) Conv3d weight, got {tuple(w.shape)}")
    s = bn_weight.detach().double().cpu() / torch.sqrt(running_var.detach().double().cpu() + eps)
    b = bias.detach().double().cpu() if bias is not None else torch.zeros(COUT, dtype=torch.float64)
    shift = (b - running_mean.detach().double().cpu()) * s + bn_bias.detach().double().cpu()
    wt = w.reshape(COUT, CIN, KS ** 3).permute(2, 0, 1)                 # [tap][cout][cin]
    lane = torch.arange(64)
    cout, kblk = lane % 16, lane // 16
    cin = kblk.view(64, 1) * 8 + torch.arange(8).view(1, 8)            # [lane][j]
    packed = wt[:, cout.view(64, 1).expand(64, 8), cin]                 # [tap][lane][j]
    packed = packed.to(torch.float32).to(torch.bfloat16).contiguous()
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


def _fold_bn(conv, bn, what):
    """(f64 weight (32, 32), f64 scale, f64 shift) of an eval-mode Conv3d(32, 32, 1) + BatchNorm3d."""
    w = conv.weight.detach().to(torch.float64).cpu()
    if tuple(w.shape) != (HEAD_C, HEAD_C, 1, 1, 1):
        raise RuntimeError(f"{what}: expected a ({HEAD_C}, {HEAD_C}, 1, 1, 1) Conv3d weight, got {tuple(w.shape)}")
    if bn.running_mean is None or tuple(bn.running_mean.shape) != (HEAD_C,):
        raise RuntimeError(f"{what}: expected a BatchNorm3d({HEAD_C}) with running statistics")
    s = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    b = conv.bias.detach().double().cpu() if conv.bias is not None else torch.zeros(HEAD_C, dtype=torch.float64)
    shift = (b - bn.running_mean.detach().double().cpu()) * s + bn.bias.detach().double().cpu()
    return w.reshape(HEAD_C, HEAD_C), s, shift


def fold_v2v_head(block1, block2, output_conv, device="cuda"):
    """Two eval-mode ``Basic3DBlock(32, 32, 1)``-shaped modules (``.block[0]`` conv, ``.block[1]``
    BN) and a ``Conv3d(32, J, 1)`` -> (packed bf16 weights, scale_shift (2, 2, 32) f32, bias3 (J,)
    f32) on ``device``.  BN and the conv bias are folded in float64 as in ``fold_basic3d_block``;
    the weights are rounded to bf16 and packed [layer][m][lane][8] as mvn_v2v_head expects."""
    w1, s1, t1 = _fold_bn(block1.block[0], block1.block[1], "block1")
    w2, s2, t2 = _fold_bn(block2.block[0], block2.block[1], "block2")
    w3 = output_conv.weight.detach().to(torch.float64).cpu()
    J = w3.shape[0]
    if w3.dim() != 5 or tuple(w3.shape[1:]) != (HEAD_C, 1, 1, 1) or not 1 <= J <= HEAD_C:
        raise RuntimeError(f"output_conv: expected a (J <= {HEAD_C}, {HEAD_C}, 1, 1, 1) Conv3d weight, "
                           f"got {tuple(w3.shape)}")
    w3p = torch.zeros(HEAD_C, HEAD_C, dtype=torch.float64)
    w3p[:J] = w3.reshape(J, HEAD_C)
    b3 = output_conv.bias.detach().double().cpu() if output_conv.bias is not None else torch.zeros(J, dtype=torch.float64)
    lane = torch.arange(64)
    row, k = lane % 16, (lane // 16).view(64, 1) * 8 + torch.arange(8).view(1, 8)    # [lane], [lane][j]
    packed = torch.empty(3, 2, 64, 8, dtype=torch.float64)
    for l, w in enumerate((w1, w2, w3p)):
        cin = head_kslot(l)[k]                                                       # [lane][j]
        for m in range(2):
            packed[l, m] = w[(16 * m + row).view(64, 1).expand(64, 8), cin]
    packed = packed.to(torch.float32).to(torch.bfloat16).contiguous()
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


def v2v_trunk(v2v_model, x):
    """V2VModel.forward (v2v.py:164-169) up to the head: front_layers, encoder_decoder and
    back_layers[0], run with the model's own modules."""
    x = v2v_model.front_layers(x)
    x = v2v_model.encoder_decoder(x)
    return v2v_model.back_layers[0](x)
