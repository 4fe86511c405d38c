"""PyTorch-ROCm custom ops over the libmvn_hip C ABI.

Each op is registered with ``torch.library.custom_op`` under the ``mvn_rocm``
namespace (``torch.ops.mvn_rocm.unproject`` …), launches on torch's current HIP
stream of the input's device, and has a fake (meta) kernel so it traces.  Inputs
must already live on the GPU: there is deliberately no CPU path.

Eager calls skip the dispatcher: ``call(op, *args)`` runs the op's own Python body
directly (the same ctypes launch) unless a tracer is active (torch.compile, or a
dispatch mode such as make_fx / FakeTensor), where the registered op is what must be
recorded.  The dispatcher round trip of a ``custom_op`` costs ~20 µs of host time per
call, on the order of the small launches it dispatches.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib

_DTYPE_CODE = {torch.float32: _lib.MVN_DTYPE_F32, torch.bfloat16: _lib.MVN_DTYPE_BF16}
_CODE_DTYPE = {v: k for k, v in _DTYPE_CODE.items()}


def _stream(t: Tensor) -> int:
    # the raw pointer of the device's current stream, without building a torch.cuda.Stream
    # object per call (host cost per op: the small-batch algebraic path is launch-bound)
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def f32c(t: Tensor) -> Tensor:
    """t as contiguous float32, with no dispatcher round trip when it already is."""
    return t if (t.dtype is torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _require_gpu(*tensors: Optional[Tensor]) -> None:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "mvn_rocm ops run on the MI355X only (got a tensor on "
                f"{t.device}); there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"mvn_rocm: tensors on different devices ({dev} vs {t.device})")


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _op(name: str):
    """Register fn as torch.ops.mvn_rocm.<name>, keeping the plain function as .eager."""
    def deco(fn):
        d = torch.library.custom_op(f"mvn_rocm::{name}", fn, mutates_args=())
        d.eager = fn
        return d
    return deco


def _tracing() -> bool:
    """Something records or transforms the call: torch.compile, a torch-dispatch mode,
    torch.jit.trace, or a functorch transform (vmap / grad / jvp wrap storage-less tensors)."""
    if torch.compiler.is_compiling() or torch._C._len_torch_dispatch_stack():
        return True
    if torch._C._get_tracing_state() is not None:
        return True
    try:
        return torch._C._functorch.peek_interpreter_stack() is not None
    except AttributeError:        # older torch: no functorch interpreter stack
        return False


def call(op, *args):
    """op(*args) — through the dispatcher only while something traces."""
    if _tracing():
        return op(*args)
    return op.eager(*args)


# --------------------------------------------------------------------------- unproject
@_op("unproject")
def unproject(feat: Tensor, proj: Tensor, coords: Tensor, conf: Optional[Tensor], agg: int,
              align_corners: bool, out_dtype: int, precision: int = 0) -> Tensor:
    """feat (B,N,C,H,W) f32|bf16, proj (B,N,3,4) f32, coords (B,Vx,Vy,Vz,3) f32,
    conf (B,N,C) f32 or None -> (B,C,Vx,Vy,Vz) of dtype code `out_dtype`; `precision`
    MVN_PRECISION_EXACT (the reference's rounding) or MVN_PRECISION_FAST."""
    _require_gpu(feat, proj, coords, conf)
    B, N, C, H, W = feat.shape
    Vx, Vy, Vz = coords.shape[1:4]
    out = torch.empty((B, C, Vx, Vy, Vz), dtype=_CODE_DTYPE[out_dtype], device=feat.device)
    if out.numel() == 0:                  # empty batch: the reference returns the empty volume
        return out
    lib = _lib.load()
    if precision == _lib.MVN_PRECISION_EXACT:
        code = lib.mvn_unproject(
            feat.data_ptr(), _DTYPE_CODE[feat.dtype], proj.data_ptr(), coords.data_ptr(), _ptr(conf),
            out.data_ptr(), out_dtype, B, N, C, H, W, Vx, Vy, Vz, agg, int(align_corners), _stream(feat))
    else:
        code = lib.mvn_unproject_precision(
            feat.data_ptr(), _DTYPE_CODE[feat.dtype], proj.data_ptr(), coords.data_ptr(), None, 0, _ptr(conf),
            out.data_ptr(), out_dtype, _lib.MVN_LAYOUT_NCDHW, B, N, C, H, W, Vx, Vy, Vz, agg, int(align_corners),
            int(precision), _stream(feat))
    _lib.check(code, "mvn_unproject")
    return out


@unproject.register_fake
def _(feat, proj, coords, conf, agg, align_corners, out_dtype, precision=0):
    B, N, C, H, W = feat.shape
    return feat.new_empty((B, C, *coords.shape[1:4]), dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- soft-argmax
@_op("softargmax3d")
def softargmax3d(vol: Tensor, coords: Tensor, softmax: bool, multiplier: float, return_volume: bool,
                 out_dtype: int) -> Tuple[Tensor, Tensor]:
    """vol (B,J,Vx,Vy,Vz) f32|bf16 (inner three dims contiguous; batch / joint strides
    arbitrary), coords (B,Vx,Vy,Vz,3) f32 -> (xyz (B,J,3) f32, normalised volume or an
    empty tensor when return_volume is False)."""
    _require_gpu(vol, coords)
    B, J, Vx, Vy, Vz = vol.shape
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=vol.device)
    if return_volume:
        out = torch.empty((B, J, Vx, Vy, Vz), dtype=_CODE_DTYPE[out_dtype], device=vol.device)
    else:
        out = torch.empty((0,), dtype=_CODE_DTYPE[out_dtype], device=vol.device)
    lib = _lib.load()
    ws_bytes = lib.mvn_softargmax3d_workspace_bytes(B, J, Vx, Vy, Vz)
    ws = torch.empty((ws_bytes + 15) // 16 * 4, dtype=torch.float32, device=vol.device)
    code = lib.mvn_softargmax3d(
        vol.data_ptr(), _DTYPE_CODE[vol.dtype], vol.stride(0), vol.stride(1), coords.data_ptr(),
        float(multiplier), int(softmax), xyz.data_ptr(), out.data_ptr() if return_volume else None,
        out_dtype, ws.data_ptr(), ws.numel() * 4, B, J, Vx, Vy, Vz, _stream(vol))
    _lib.check(code, "mvn_softargmax3d")
    return xyz, out


@softargmax3d.register_fake
def _(vol, coords, softmax, multiplier, return_volume, out_dtype):
    B, J = vol.shape[:2]
    xyz = vol.new_empty((B, J, 3), dtype=torch.float32)
    shape = tuple(vol.shape) if return_volume else (0,)
    return xyz, vol.new_empty(shape, dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- in-kernel coordinates
@_op("unproject_cuboid")
def unproject_cuboid(feat: Tensor, proj: Tensor, cuboids: Tensor, volume_size: int, transfer: bool,
                     conf: Optional[Tensor], agg: int, align_corners: bool, out_dtype: int,
                     precision: int = 0) -> Tensor:
    """unproject with coordinates formed in-kernel from cuboids (B, 18) f32 (V^3 grid)."""
    _require_gpu(feat, proj, cuboids, conf)
    B, N, C, H, W = feat.shape
    V = int(volume_size)
    out = torch.empty((B, C, V, V, V), dtype=_CODE_DTYPE[out_dtype], device=feat.device)
    if out.numel() == 0:
        return out
    code = _lib.load().mvn_unproject_precision(
        feat.data_ptr(), _DTYPE_CODE[feat.dtype], proj.data_ptr(), None, cuboids.data_ptr(), int(transfer), _ptr(conf),
        out.data_ptr(), out_dtype, _lib.MVN_LAYOUT_NCDHW, B, N, C, H, W, V, V, V, agg, int(align_corners),
        int(precision), _stream(feat))
    _lib.check(code, "mvn_unproject_cuboid")
    return out


@unproject_cuboid.register_fake
def _(feat, proj, cuboids, volume_size, transfer, conf, agg, align_corners, out_dtype, precision=0):
    B, N, C = feat.shape[:3]
    V = int(volume_size)
    return feat.new_empty((B, C, V, V, V), dtype=_CODE_DTYPE[out_dtype])


@_op("softargmax3d_cuboid")
def softargmax3d_cuboid(vol: Tensor, cuboids: Tensor, transfer: bool, softmax: bool, multiplier: float,
                        return_volume: bool, out_dtype: int) -> Tuple[Tensor, Tensor]:
    """softargmax3d with coordinates formed in-kernel from cuboids (B, 18) f32."""
    _require_gpu(vol, cuboids)
    B, J, V = vol.shape[:3]
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=vol.device)
    if return_volume:
        out = torch.empty(tuple(vol.shape), dtype=_CODE_DTYPE[out_dtype], device=vol.device)
    else:
        out = torch.empty((0,), dtype=_CODE_DTYPE[out_dtype], device=vol.device)
    lib = _lib.load()
    ws_bytes = lib.mvn_softargmax3d_workspace_bytes(B, J, V, V, V)
    ws = torch.empty((ws_bytes + 15) // 16 * 4, dtype=torch.float32, device=vol.device)
    code = lib.mvn_softargmax3d_cuboid(
        vol.data_ptr(), _DTYPE_CODE[vol.dtype], vol.stride(0), vol.stride(1), cuboids.data_ptr(), int(transfer),
        float(multiplier), int(softmax), xyz.data_ptr(), out.data_ptr() if return_volume else None,
        out_dtype, ws.data_ptr(), ws.numel() * 4, B, J, V, _stream(vol))
    _lib.check(code, "mvn_softargmax3d_cuboid")
    return xyz, out


@softargmax3d_cuboid.register_fake
def _(vol, cuboids, transfer, softmax, multiplier, return_volume, out_dtype):
    B, J = vol.shape[:2]
    shape = tuple(vol.shape) if return_volume else (0,)
    return vol.new_empty((B, J, 3), dtype=torch.float32), vol.new_empty(shape, dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- V2V head
def _head_dims(x: Tensor, channels_last: bool):
    """(B, (Vx, Vy, Vz)) of the head's input in either layout."""
    return x.shape[0], (tuple(x.shape[1:4]) if channels_last else tuple(x.shape[2:5]))


@_op("v2v_head")
def v2v_head(x: Tensor, packed: Tensor, scale_shift: Tensor, bias3: Tensor, out_dtype: int,
             channels_last: bool) -> Tensor:
    """x (B,32,Vx,Vy,Vz) f32|bf16, or (B,Vx,Vy,Vz,32) bf16 with channels_last -> logits
    (B,J,Vx,Vy,Vz) of dtype code `out_dtype`, J = bias3.numel() (csrc/v2v_head.hip)."""
    _require_gpu(x, packed, scale_shift, bias3)
    (B, (Vx, Vy, Vz)), J = _head_dims(x, channels_last), bias3.numel()
    out = torch.empty((B, J, Vx, Vy, Vz), dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if out.numel() == 0:                  # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_v2v_head(
        x.data_ptr(), _DTYPE_CODE[x.dtype], _lib.MVN_LAYOUT_NDHWC if channels_last else _lib.MVN_LAYOUT_NCDHW,
        packed.data_ptr(), scale_shift.data_ptr(), bias3.data_ptr(), out.data_ptr(), out_dtype, B, J, Vx, Vy, Vz,
        _stream(x))
    _lib.check(code, "mvn_v2v_head")
    return out


@v2v_head.register_fake
def _(x, packed, scale_shift, bias3, out_dtype, channels_last):
    B, vol = _head_dims(x, channels_last)
    return x.new_empty((B, bias3.numel(), *vol), dtype=_CODE_DTYPE[out_dtype])


@_op("v2v_head_softargmax")
def v2v_head_softargmax(x: Tensor, packed: Tensor, scale_shift: Tensor, bias3: Tensor, coords: Optional[Tensor],
                        cuboids: Optional[Tensor], transfer: bool, softmax: bool, multiplier: float,
                        return_volume: bool, out_dtype: int, group_frames: int,
                        channels_last: bool) -> Tuple[Tensor, Tensor]:
    """v2v_head then the 3D soft-argmax in one C call (mvn_v2v_head_softargmax): exactly one of
    coords (B,Vx,Vy,Vz,3) f32 and cuboids (B,18) f32 -> (xyz (B,J,3) f32, normalised volume or
    an empty tensor when return_volume is False)."""
    _require_gpu(x, packed, scale_shift, bias3, coords, cuboids)
    (B, (Vx, Vy, Vz)), J = _head_dims(x, channels_last), bias3.numel()
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=x.device)
    shape = (B, J, Vx, Vy, Vz) if return_volume else (0,)
    out = torch.empty(shape, dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if xyz.numel() == 0:
        return xyz, out
    lib = _lib.load()
    ws_bytes = lib.mvn_v2v_head_softargmax_workspace_bytes(int(group_frames), J, Vx, Vy, Vz)
    ws = torch.empty((ws_bytes + 15) // 16 * 4, dtype=torch.float32, device=x.device)
    code = lib.mvn_v2v_head_softargmax(
        x.data_ptr(), _DTYPE_CODE[x.dtype], _lib.MVN_LAYOUT_NDHWC if channels_last else _lib.MVN_LAYOUT_NCDHW,
        packed.data_ptr(), scale_shift.data_ptr(), bias3.data_ptr(), _ptr(coords), _ptr(cuboids), int(transfer),
        float(multiplier), int(softmax), xyz.data_ptr(), out.data_ptr() if return_volume else None, out_dtype,
        ws.data_ptr(), ws.numel() * 4, int(group_frames), B, J, Vx, Vy, Vz, _stream(x))
    _lib.check(code, "mvn_v2v_head_softargmax")
    return xyz, out


@v2v_head_softargmax.register_fake
def _(x, packed, scale_shift, bias3, coords, cuboids, transfer, softmax, multiplier, return_volume, out_dtype,
      group_frames, channels_last):
    B, vol = _head_dims(x, channels_last)
    J = bias3.numel()
    shape = (B, J, *vol) if return_volume else (0,)
    return x.new_empty((B, J, 3), dtype=torch.float32), x.new_empty(shape, dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- V2V Res3DBlock convs (32, 64, 128 channels)
def _conv3_op(name: str, cout: int, doc: str):
    """Register ``mvn_rocm::<name>`` and its fake: one 3x3x3 conv launch with ``cout`` output
    channels through the C entry point ``mvn_<name>``.  The three widths differ in nothing else."""
    entry = f"mvn_{name}"

    def conv3(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, skip_mode: int, skip: Optional[Tensor],
              skip_packed: Optional[Tensor], skip_scale: Optional[Tensor], skip_shift: Optional[Tensor]) -> Tensor:
        _require_gpu(x, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift)
        B, V, cin = x.shape[0], x.shape[1], x.shape[4]
        out = torch.empty((B, V, V, V, cout), dtype=torch.bfloat16, device=x.device)
        if out.numel() == 0:                  # empty batch: nothing to launch
            return out
        code = getattr(_lib.load(), entry)(
            x.data_ptr(), cin, packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), int(skip_mode), _ptr(skip),
            skip.shape[4] if skip is not None else 0, _ptr(skip_packed), _ptr(skip_scale), _ptr(skip_shift),
            out.data_ptr(), B, V, _stream(x))
        _lib.check(code, entry)
        return out

    conv3.__name__, conv3.__doc__ = name, doc
    op = _op(name)(conv3)

    @op.register_fake
    def _(x, packed, scale, shift, skip_mode, skip, skip_packed, skip_scale, skip_shift):
        return x.new_empty((*x.shape[:4], cout), dtype=torch.bfloat16)
    return op


v2v_conv3 = _conv3_op("v2v_conv3", 32, """x (B,V,V,V,cin) bf16, cin 16 | 32 -> (B,V,V,V,32) bf16:
    relu(bn(conv3d_3(x)) + skip term) (csrc/v2v_res3d.hip); skip (B,V,V,V,32) with MVN_SKIP_IDENTITY,
    (B,V,V,V,16) and its packed 1x1x1 weights, scale and shift with MVN_SKIP_POINTWISE.""")
v2v_conv3_wide = _conv3_op("v2v_conv3_wide", 64, """x (B,V,V,V,cin) bf16, cin 32 | 64 -> (B,V,V,V,64) bf16:
    relu(bn(conv3d_3(x)) + skip term) (csrc/v2v_interior.hip); skip (B,V,V,V,64) with MVN_SKIP_IDENTITY,
    (B,V,V,V,32) and its packed 1x1x1 weights, scale and shift with MVN_SKIP_POINTWISE.""")
v2v_conv3_deep = _conv3_op("v2v_conv3_deep", 128, """x (B,D,D,D,cin) bf16, cin 64 | 128, any D in [1, 64] ->
    (B,D,D,D,128) bf16: relu(bn(conv3d_3(x)) + skip term) (csrc/v2v_deep.hip); skip (B,D,D,D,128) with
    MVN_SKIP_IDENTITY, (B,D,D,D,64) and its packed 1x1x1 weights, scale and shift with MVN_SKIP_POINTWISE.""")


@_op("v2v_res3d")
def v2v_res3d(x: Tensor, packed1: Tensor, scale1: Tensor, shift1: Tensor, packed2: Tensor, scale2: Tensor,
              shift2: Tensor, skip_packed: Optional[Tensor], skip_scale: Optional[Tensor],
              skip_shift: Optional[Tensor], group_frames: int) -> Tensor:
    """A whole Res3DBlock in one C call (mvn_v2v_res3d): x (B,V,V,V,cin) bf16 -> (B,V,V,V,32) bf16;
    the identity skip (cin 32) without skip_packed, the pointwise one (cin 16) with it."""
    _require_gpu(x, packed1, scale1, shift1, packed2, scale2, shift2, skip_packed, skip_scale, skip_shift)
    B, V, cin = x.shape[0], x.shape[1], x.shape[4]
    out = torch.empty((B, V, V, V, 32), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:
        return out
    lib = _lib.load()
    ws_bytes = lib.mvn_v2v_res3d_workspace_bytes(int(group_frames), V)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    mode = _lib.MVN_SKIP_IDENTITY if skip_packed is None else _lib.MVN_SKIP_POINTWISE
    code = lib.mvn_v2v_res3d(
        x.data_ptr(), cin, packed1.data_ptr(), scale1.data_ptr(), shift1.data_ptr(), packed2.data_ptr(),
        scale2.data_ptr(), shift2.data_ptr(), mode, _ptr(skip_packed), _ptr(skip_scale), _ptr(skip_shift),
        out.data_ptr(), ws.data_ptr(), ws.numel(), int(group_frames), B, V, _stream(x))
    _lib.check(code, "mvn_v2v_res3d")
    return out


@v2v_res3d.register_fake
def _(x, packed1, scale1, shift1, packed2, scale2, shift2, skip_packed, skip_scale, skip_shift, group_frames):
    return x.new_empty((*x.shape[:4], 32), dtype=torch.bfloat16)


# --------------------------------------------------------------------------- V2V first pooled level
@_op("v2v_maxpool2")
def v2v_maxpool2(x: Tensor) -> Tensor:
    """x (B,V,V,V,C) bf16 -> (B,V/2,V/2,V/2,C) bf16: F.max_pool3d(x, 2, 2) channels-last
    (csrc/v2v_interior.hip)."""
    _require_gpu(x)
    B, V, C = x.shape[0], x.shape[1], x.shape[4]
    out = torch.empty((B, V // 2, V // 2, V // 2, C), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:                  # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_v2v_maxpool2(x.data_ptr(), out.data_ptr(), B, V, C, _stream(x))
    _lib.check(code, "mvn_v2v_maxpool2")
    return out


@v2v_maxpool2.register_fake
def _(x):
    B, V, C = x.shape[0], x.shape[1], x.shape[4]
    return x.new_empty((B, V // 2, V // 2, V // 2, C), dtype=torch.bfloat16)


@_op("v2v_upsample2")
def v2v_upsample2(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, skip: Optional[Tensor]) -> Tensor:
    """x (B,V,V,V,64) bf16 -> (B,2V,2V,2V,32) bf16: relu(bn(conv_transpose3d_2(x))) + skip
    (csrc/v2v_interior.hip); skip (B,2V,2V,2V,32) bf16 or None."""
    _require_gpu(x, packed, scale, shift, skip)
    B, V = x.shape[0], x.shape[1]
    out = torch.empty((B, 2 * V, 2 * V, 2 * V, 32), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:                  # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_v2v_upsample2(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                         _ptr(skip), out.data_ptr(), B, V, _stream(x))
    _lib.check(code, "mvn_v2v_upsample2")
    return out


@v2v_upsample2.register_fake
def _(x, packed, scale, shift, skip):
    B, V = x.shape[0], x.shape[1]
    return x.new_empty((B, 2 * V, 2 * V, 2 * V, 32), dtype=torch.bfloat16)


# --------------------------------------------------------------------------- V2V 128-channel levels
@_op("v2v_upsample2_deep")
def v2v_upsample2_deep(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, skip: Optional[Tensor]) -> Tensor:
    """x (B,D,D,D,128) bf16 -> (B,2D,2D,2D,cout) bf16, cout = scale.numel() (64 | 128):
    relu(bn(conv_transpose3d_2(x))) + skip (csrc/v2v_deep.hip); skip (B,2D,2D,2D,cout) bf16 or None."""
    _require_gpu(x, packed, scale, shift, skip)
    B, D, cout = x.shape[0], x.shape[1], scale.shape[0]
    out = torch.empty((B, 2 * D, 2 * D, 2 * D, cout), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:                  # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_v2v_upsample2_deep(x.data_ptr(), cout, packed.data_ptr(), scale.data_ptr(),
                                              shift.data_ptr(), _ptr(skip), out.data_ptr(), B, D, _stream(x))
    _lib.check(code, "mvn_v2v_upsample2_deep")
    return out


@v2v_upsample2_deep.register_fake
def _(x, packed, scale, shift, skip):
    B, D = x.shape[0], x.shape[1]
    return x.new_empty((B, 2 * D, 2 * D, 2 * D, scale.shape[0]), dtype=torch.bfloat16)


# --------------------------------------------------------------------------- feature conv (process_features)
FEATURE_COUT = 32             # csrc/feature_conv.hip: the 32 rows of one 32x32x2 f32 MFMA


@_op("feature_conv")
def feature_conv(x: Tensor, weight: Tensor, bias: Optional[Tensor], out_dtype: int) -> Tensor:
    """x (M,Cin,H,W) f32|bf16 contiguous, weight (32,Cin) f32, bias (32,) f32 or None (zeros) ->
    (M,32,H,W) of dtype code `out_dtype`: Conv2d(Cin, 32, 1) as an ascending fmaf chain
    (csrc/feature_conv.hip)."""
    _require_gpu(x, weight, bias)
    M, cin, H, W = x.shape
    out = torch.empty((M, FEATURE_COUT, H, W), dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if out.numel() == 0:                  # no image or no pixel: nothing to launch
        return out
    code = _lib.load().mvn_feature_conv(x.data_ptr(), _DTYPE_CODE[x.dtype], weight.data_ptr(), _ptr(bias),
                                        out.data_ptr(), out_dtype, M, cin, weight.shape[0], H, W, _stream(x))
    _lib.check(code, "mvn_feature_conv")
    return out


@feature_conv.register_fake
def _(x, weight, bias, out_dtype):
    M, cin, H, W = x.shape
    return x.new_empty((M, FEATURE_COUT, H, W), dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- backbone deconv head
DECONV_COUT = 256             # csrc/deconv_head.hip: every layer of the head has 256 output channels


def _deconv_out_shape(x: Tensor, nchw: bool):
    M, H, W, _ = x.shape
    return (M, DECONV_COUT, 2 * H, 2 * W) if nchw else (M, 2 * H, 2 * W, DECONV_COUT)


@_op("deconv4s2")
def deconv4s2(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, nchw: bool, out_dtype: int) -> Tensor:
    """x (M,H,W,Cin) bf16 channels-last -> relu(bn(conv_transpose2d_4s2(x))) as (M,2H,2W,256) bf16
    (nchw False) or (M,256,2H,2W) of dtype code `out_dtype` (nchw True) (csrc/deconv_head.hip)."""
    _require_gpu(x, packed, scale, shift)
    M, H, W, cin = x.shape
    out = torch.empty(_deconv_out_shape(x, nchw), dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_deconv4s2(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                     out.data_ptr(), _lib.MVN_LAYOUT_NCHW if nchw else _lib.MVN_LAYOUT_NHWC,
                                     out_dtype, M, cin, H, W, _stream(x))
    _lib.check(code, "mvn_deconv4s2")
    return out


@deconv4s2.register_fake
def _(x, packed, scale, shift, nchw, out_dtype):
    return x.new_empty(_deconv_out_shape(x, nchw), dtype=_CODE_DTYPE[out_dtype])


@_op("deconv4s2_project")
def deconv4s2_project(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, proj: Tensor, bias: Tensor,
                      out_dtype: int) -> Tensor:
    """x (M,H,W,Cin) bf16 channels-last -> the 256 -> 32 projection (proj packed hi | lo, bias (32,) f32) of
    relu(bn(conv_transpose2d_4s2(x))) rounded to bf16, as (M,32,2H,2W) of dtype code `out_dtype`; the
    256-channel map is not stored (csrc/deconv_head.hip)."""
    _require_gpu(x, packed, scale, shift, proj, bias)
    M, H, W, cin = x.shape
    out = torch.empty((M, FEATURE_COUT, 2 * H, 2 * W), dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_deconv4s2_project(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                             proj.data_ptr(), bias.data_ptr(), out.data_ptr(), out_dtype, M, cin, H, W,
                                             _stream(x))
    _lib.check(code, "mvn_deconv4s2_project")
    return out


@deconv4s2_project.register_fake
def _(x, packed, scale, shift, proj, bias, out_dtype):
    M, H, W, _ = x.shape
    return x.new_empty((M, FEATURE_COUT, 2 * H, 2 * W), dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- ResNet trunk (Bottleneck convolutions)
@_op("conv1x1")
def conv1x1(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, skip_mode: int, skip: Optional[Tensor],
            skip_packed: Optional[Tensor], skip_scale: Optional[Tensor], skip_shift: Optional[Tensor],
            skip_stride: int) -> Tensor:
    """x (M,H,W,Cin) bf16 channels-last -> relu(bn(conv1x1(x)) + skip term) as (M,H,W,Cout) bf16, Cout =
    len(scale); skip (M,H,W,Cout) with MVN_SKIP_IDENTITY, (M,Hs,Ws,Cs) with its packed 1x1 weights, scale,
    shift and stride with MVN_SKIP_POINTWISE (csrc/bottleneck.hip)."""
    _require_gpu(x, packed, scale, shift, skip, skip_packed, skip_scale, skip_shift)
    M, H, W, cin = x.shape
    cout = scale.shape[0]
    out = torch.empty((M, H, W, cout), dtype=torch.bfloat16, device=x.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    pw = int(skip_mode) == _lib.MVN_SKIP_POINTWISE
    code = _lib.load().mvn_conv1x1(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), int(skip_mode),
                                   _ptr(skip), _ptr(skip_packed), _ptr(skip_scale), _ptr(skip_shift),
                                   skip.shape[3] if pw else 0, skip.shape[1] if pw else 0, skip.shape[2] if pw else 0,
                                   int(skip_stride), out.data_ptr(), M, H, W, cin, cout, _stream(x))
    _lib.check(code, "mvn_conv1x1")
    return out


@conv1x1.register_fake
def _(x, packed, scale, shift, skip_mode, skip, skip_packed, skip_scale, skip_shift, skip_stride):
    return x.new_empty((*x.shape[:3], scale.shape[0]), dtype=torch.bfloat16)


def _conv3x3_out_shape(x: Tensor, stride: int):
    M, H, W, C = x.shape
    return (M, (H - 1) // stride + 1, (W - 1) // stride + 1, C)


@_op("conv3x3")
def conv3x3(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, stride: int) -> Tensor:
    """x (M,H,W,C) bf16 channels-last -> relu(bn(conv3x3(x, padding 1, stride))) as (M,Ho,Wo,C) bf16
    (csrc/bottleneck.hip)."""
    _require_gpu(x, packed, scale, shift)
    M, H, W, C = x.shape
    out = torch.empty(_conv3x3_out_shape(x, int(stride)), dtype=torch.bfloat16, device=x.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_conv3x3(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
                                   M, H, W, C, int(stride), _stream(x))
    _lib.check(code, "mvn_conv3x3")
    return out


@conv3x3.register_fake
def _(x, packed, scale, shift, stride):
    return x.new_empty(_conv3x3_out_shape(x, stride), dtype=torch.bfloat16)


# --------------------------------------------------------------------------- ResNet stem
STEM_COUT = 64


def _stem_out_shape(images: Tensor):
    M, _, H, W = images.shape
    return (M, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1, STEM_COUT)


@_op("stem")
def stem(images: Tensor, packed: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    """images (M,3,H,W) f32|bf16 contiguous NCHW -> maxpool(relu(bn(conv7x7(images, stride 2, padding 3))), 3, 2, 1)
    as (M,Hp,Wp,64) bf16 channels-last (csrc/stem.hip)."""
    _require_gpu(images, packed, scale, shift)
    M, _, H, W = images.shape
    out = torch.empty(_stem_out_shape(images), dtype=torch.bfloat16, device=images.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_stem(images.data_ptr(), _DTYPE_CODE[images.dtype], packed.data_ptr(), scale.data_ptr(),
                                shift.data_ptr(), out.data_ptr(), M, H, W, _stream(images))
    _lib.check(code, "mvn_stem")
    return out


@stem.register_fake
def _(images, packed, scale, shift):
    return images.new_empty(_stem_out_shape(images), dtype=torch.bfloat16)


# --------------------------------------------------------------------------- confidence heads
def _pool_out_shape(x: Tensor, scale: Tensor):
    M, H, W, _ = x.shape
    return (M, H // 2, W // 2, scale.shape[0])


@_op("conv3x3_pool")
def conv3x3_pool(x: Tensor, packed: Tensor, scale: Tensor, shift: Tensor, out_dtype: int) -> Tensor:
    """x (M,H,W,Cin) bf16 channels-last -> relu(maxpool2(bn(conv3x3(x, padding 1)))) as (M,H/2,W/2,Cout) of dtype
    code `out_dtype`, Cout = len(scale) (csrc/confidence_head.hip)."""
    _require_gpu(x, packed, scale, shift)
    M, H, W, cin = x.shape
    out = torch.empty(_pool_out_shape(x, scale), dtype=_CODE_DTYPE[out_dtype], device=x.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_conv3x3_pool(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                        out.data_ptr(), out_dtype, M, H, W, cin, scale.shape[0], _stream(x))
    _lib.check(code, "mvn_conv3x3_pool")
    return out


@conv3x3_pool.register_fake
def _(x, packed, scale, shift, out_dtype):
    return x.new_empty(_pool_out_shape(x, scale), dtype=_CODE_DTYPE[out_dtype])


@_op("confidence_tail")
def confidence_tail(pooled: Tensor, packed: Tensor, c1: int, c2: int, n: int, sigmoid: bool) -> Tensor:
    """pooled (M,h,w,C0) f32 channels-last, packed f32 (pack_confidence_tail) -> the sigmoid (or the logits) of
    Linear(C0,c1) relu Linear(c1,c2) relu Linear(c2,n) of the mean over the pixels, (M,n) f32
    (csrc/confidence_head.hip)."""
    _require_gpu(pooled, packed)
    M, h, w, c0 = pooled.shape
    out = torch.empty((M, n), dtype=torch.float32, device=pooled.device)
    if M == 0:                            # empty batch: nothing to launch
        return out
    code = _lib.load().mvn_confidence_tail(pooled.data_ptr(), packed.data_ptr(), out.data_ptr(), M, h * w, c0, int(c1),
                                           int(c2), int(n), _lib.MVN_ACT_SIGMOID if sigmoid else _lib.MVN_ACT_NONE,
                                           _stream(pooled))
    _lib.check(code, "mvn_confidence_tail")
    return out


@confidence_tail.register_fake
def _(pooled, packed, c1, c2, n, sigmoid):
    return pooled.new_empty((pooled.shape[0], n), dtype=torch.float32)


# --------------------------------------------------------------------------- 2D soft-argmax
@_op("softargmax2d")
def softargmax2d(hm: Tensor, softmax: bool, multiplier: float, return_maps: bool,
                 out_dtype: int) -> Tuple[Tensor, Tensor]:
    """hm (B,J,H,W) f32|bf16 contiguous -> (xy (B,J,2) f32, maps (B,J,H,W) or an empty tensor)."""
    _require_gpu(hm)
    B, J, H, W = hm.shape
    xy = torch.empty((B, J, 2), dtype=torch.float32, device=hm.device)
    if return_maps:
        maps = torch.empty((B, J, H, W), dtype=_CODE_DTYPE[out_dtype], device=hm.device)
    else:
        maps = torch.empty((0,), dtype=_CODE_DTYPE[out_dtype], device=hm.device)
    code = _lib.load().mvn_softargmax2d(hm.data_ptr(), _DTYPE_CODE[hm.dtype], float(multiplier), int(softmax),
                                        xy.data_ptr(), maps.data_ptr() if return_maps else None, out_dtype,
                                        B, J, H, W, _stream(hm))
    _lib.check(code, "mvn_softargmax2d")
    return xy, maps


@softargmax2d.register_fake
def _(hm, softmax, multiplier, return_maps, out_dtype):
    B, J = hm.shape[:2]
    shape = tuple(hm.shape) if return_maps else (0,)
    return hm.new_empty((B, J, 2), dtype=torch.float32), hm.new_empty(shape, dtype=_CODE_DTYPE[out_dtype])


# --------------------------------------------------------------------------- DLT
@_op("dlt")
def dlt(proj: Tensor, pts: Tensor, conf: Optional[Tensor]) -> Tensor:
    """proj (B,N,3,4) f32, pts (B,N,J,2) f32, conf (B,N,J) f32 or None -> (B,J,3) f32."""
    _require_gpu(proj, pts, conf)
    B, N, J = pts.shape[:3]
    out = torch.empty((B, J, 3), dtype=torch.float32, device=pts.device)
    if out.numel() == 0:                  # multiview.py:164-174 on an empty batch: (0, J, 3)
        return out
    code = _lib.load().mvn_dlt(proj.data_ptr(), pts.data_ptr(), _ptr(conf), out.data_ptr(), B, N, J,
                               _stream(pts))
    _lib.check(code, "mvn_dlt")
    return out


@dlt.register_fake
def _(proj, pts, conf):
    B, N, J = pts.shape[:3]
    return pts.new_empty((B, J, 3), dtype=torch.float32)


# --------------------------------------------------------------------------- algebraic model, one launch
ALGEBRAIC_MAX_VIEWS = 32      # csrc/algebraic.hip: LDS holds the views' points and confidences


@_op("algebraic_triangulate")
def algebraic_triangulate(hm: Tensor, proj: Tensor, conf: Optional[Tensor], softmax: bool, multiplier: float,
                          scale_x: float, scale_y: float, return_maps: bool,
                          out_dtype: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """hm (B,N,J,H,W) f32|bf16 contiguous, proj (B,N,3,4) f32, conf (B,N,J) f32 raw or None (ones)
    -> (xyz (B,J,3), kp2d (B,N,J,2) image px, xy (B,N,J,2) heatmap px, normalised conf (B,N,J),
    all f32, maps (B,N,J,H,W) or an empty tensor).  N <= ALGEBRAIC_MAX_VIEWS."""
    _require_gpu(hm, proj, conf)
    B, N, J, H, W = hm.shape
    dev = hm.device
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    kp2d = torch.empty((B, N, J, 2), dtype=torch.float32, device=dev)
    xy = torch.empty((B, N, J, 2), dtype=torch.float32, device=dev)
    cn = torch.empty((B, N, J), dtype=torch.float32, device=dev)
    if return_maps:
        maps = torch.empty((B, N, J, H, W), dtype=_CODE_DTYPE[out_dtype], device=dev)
    else:
        maps = torch.empty((0,), dtype=_CODE_DTYPE[out_dtype], device=dev)
    if xyz.numel() == 0:
        return xyz, kp2d, xy, cn, maps
    code = _lib.load().mvn_algebraic_triangulate(
        hm.data_ptr(), _DTYPE_CODE[hm.dtype], float(multiplier), int(softmax), proj.data_ptr(), _ptr(conf),
        float(scale_x), float(scale_y), xyz.data_ptr(), kp2d.data_ptr(), xy.data_ptr(), cn.data_ptr(),
        maps.data_ptr() if return_maps else None, out_dtype, B, N, J, H, W, _stream(hm))
    _lib.check(code, "mvn_algebraic_triangulate")
    return xyz, kp2d, xy, cn, maps


@algebraic_triangulate.register_fake
def _(hm, proj, conf, softmax, multiplier, scale_x, scale_y, return_maps, out_dtype):
    B, N, J = hm.shape[:3]
    f32 = dict(dtype=torch.float32)
    shape = tuple(hm.shape) if return_maps else (0,)
    return (hm.new_empty((B, J, 3), **f32), hm.new_empty((B, N, J, 2), **f32), hm.new_empty((B, N, J, 2), **f32),
            hm.new_empty((B, N, J), **f32), hm.new_empty(shape, dtype=_CODE_DTYPE[out_dtype]))


# --------------------------------------------------------------------------- RANSAC
@_op("reprojection_error")
def reprojection_error(points3d: Tensor, pts: Tensor, proj: Tensor) -> Tensor:
    """points3d (B,J,3) f32, pts (B,N,J,2) f32, proj (B,N,3,4) f32 -> (B,J,N) f32, half the
    pixel distance (multiview.py:177-184)."""
    _require_gpu(points3d, pts, proj)
    B, N, J = pts.shape[:3]
    out = torch.empty((B, J, N), dtype=torch.float32, device=pts.device)
    if out.numel() == 0:
        return out
    code = _lib.load().mvn_reprojection_error(points3d.data_ptr(), pts.data_ptr(), proj.data_ptr(),
                                              out.data_ptr(), B, N, J, _stream(pts))
    _lib.check(code, "mvn_reprojection_error")
    return out


@reprojection_error.register_fake
def _(points3d, pts, proj):
    B, N, J = pts.shape[:3]
    return pts.new_empty((B, J, N), dtype=torch.float32)


@_op("ransac")
def ransac(proj: Tensor, pts: Tensor, pairs: Tensor, epsilon: float,
           direct_optimization: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """proj (B,N,3,4) f32, pts (B,N,J,2) f32, pairs int32 (n_iters,2) or (B,J,n_iters,2)
    -> (xyz (B,J,3) f32, inlier masks (B,J) int32 (bit v: view v used), mean error (B,J) f32)."""
    _require_gpu(proj, pts, pairs)
    B, N, J = pts.shape[:3]
    xyz = torch.empty((B, J, 3), dtype=torch.float32, device=pts.device)
    mask = torch.empty((B, J), dtype=torch.int32, device=pts.device)
    err = torch.empty((B, J), dtype=torch.float32, device=pts.device)
    if mask.numel() == 0:
        return xyz, mask, err
    code = _lib.load().mvn_triangulate_ransac(proj.data_ptr(), pts.data_ptr(), pairs.data_ptr(),
                                              int(pairs.dim() == 4), pairs.shape[-2], float(epsilon),
                                              int(direct_optimization), xyz.data_ptr(), mask.data_ptr(),
                                              err.data_ptr(), B, N, J, _stream(pts))
    _lib.check(code, "mvn_triangulate_ransac")
    return xyz, mask, err


@ransac.register_fake
def _(proj, pts, pairs, epsilon, direct_optimization):
    B, N, J = pts.shape[:3]
    return (pts.new_empty((B, J, 3), dtype=torch.float32), pts.new_empty((B, J), dtype=torch.int32),
            pts.new_empty((B, J), dtype=torch.float32))
