"""The V2V's first pooled level (csrc/v2v_interior.hip): folding and packing, the C ABI's argument
checks, the Python layer's refusals and the ``v2v_interior`` refactor — no GPU needed (only
validation paths are called; they return before any HIP call)."""
import pytest
import torch
from torch import nn

from v2v_kit import (EncoderDecorder, Res3DBlock, Upsample3DBlock, V2VModel, bn_fold64, randomise, unpack_conv3,
                     unpack_skip, unpack_upsample as unpack_up, vol)

ARG, SHAPE = -1, -2
NONE, IDENTITY, POINTWISE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- C argument validation
def test_size_functions(lib):
    assert lib.mvn_v2v_conv3_wide_packed_weight_bytes(32) == 27 * 1 * 4 * 64 * 8 * 2 == 27 * 64 * 32 * 2
    assert lib.mvn_v2v_conv3_wide_packed_weight_bytes(64) == 27 * 2 * 4 * 64 * 8 * 2 == 27 * 64 * 64 * 2
    assert lib.mvn_v2v_conv3_wide_packed_weight_bytes(16) == 0 and lib.mvn_v2v_conv3_wide_packed_weight_bytes(128) == 0
    assert lib.mvn_v2v_conv3_wide_skip_packed_weight_bytes(32) == 4 * 64 * 8 * 2 == 64 * 32 * 2
    assert lib.mvn_v2v_conv3_wide_skip_packed_weight_bytes(16) == 0
    assert lib.mvn_v2v_conv3_wide_skip_packed_weight_bytes(64) == 0
    assert lib.mvn_v2v_upsample2_packed_weight_bytes() == 2 * 16 * 64 * 8 * 2 == 64 * 32 * 8 * 2


def _wide(lib, **k):
    mode = k.get("mode", NONE)
    skip = k.get("skip", None if mode == NONE else 1)
    pw = 1 if mode == POINTWISE else None
    return lib.mvn_v2v_conv3_wide(k.get("x", 1), k.get("cin", 64), k.get("w", 1), k.get("scale", 1), k.get("shift", 1),
                                  mode, skip, k.get("skip_cin", {NONE: 0, IDENTITY: 64, POINTWISE: 32}.get(mode, 0)),
                                  k.get("ws", pw), k.get("ss", pw), k.get("ts", pw), k.get("out", 1), k.get("B", 2),
                                  k.get("V", 32), None)


def test_conv3_wide_argument_validation(lib):
    """Every documented error code, with no device: the checks run before any HIP call."""
    for name in ("x", "w", "scale", "shift", "out"):
        assert _wide(lib, **{name: None}) == ARG
    assert _wide(lib, mode=3) == ARG and _wide(lib, mode=-1) == ARG
    assert _wide(lib, mode=NONE, skip=1) == ARG
    assert _wide(lib, mode=NONE, ws=1) == ARG and _wide(lib, mode=NONE, ss=1) == ARG
    assert _wide(lib, mode=IDENTITY, skip=None) == ARG
    assert _wide(lib, mode=IDENTITY, ws=1) == ARG and _wide(lib, mode=IDENTITY, ts=1) == ARG
    assert _wide(lib, mode=POINTWISE, skip=None) == ARG
    for name in ("ws", "ss", "ts"):
        assert _wide(lib, mode=POINTWISE, **{name: None}) == ARG
    for mode in (NONE, IDENTITY, POINTWISE):
        assert _wide(lib, mode=mode, B=0) == SHAPE and _wide(lib, mode=mode, B=-2) == SHAPE
        for V in (0, 8, 24, 40, 144, 256, -16):
            assert _wide(lib, mode=mode, V=V) == SHAPE
        for cin in (0, 16, 48, 128):
            assert _wide(lib, mode=mode, cin=cin) == SHAPE
    assert _wide(lib, mode=IDENTITY, skip_cin=32) == SHAPE
    assert _wide(lib, mode=POINTWISE, skip_cin=64) == SHAPE and _wide(lib, mode=POINTWISE, skip_cin=16) == SHAPE
    assert _wide(lib, x=None, V=24) == ARG                      # an argument error comes first


def test_old_conv3_keeps_its_shapes(lib):
    """The existing entry point is not widened: 64 channels and its other refusals stay."""
    assert lib.mvn_v2v_conv3(1, 64, 1, 1, 1, NONE, None, 0, None, None, None, 1, 2, 32, None) == SHAPE
    assert lib.mvn_v2v_conv3(1, 32, 1, 1, 1, IDENTITY, 1, 64, None, None, None, 1, 2, 32, None) == SHAPE
    assert lib.mvn_v2v_conv3_packed_weight_bytes(64) == 0


def test_upsample_and_pool_argument_validation(lib):
    up = lambda **k: lib.mvn_v2v_upsample2(k.get("x", 1), k.get("w", 1), k.get("scale", 1), k.get("shift", 1),   # noqa: E731
                                           k.get("skip", 1), k.get("out", 1), k.get("B", 2), k.get("V", 32), None)
    for name in ("x", "w", "scale", "shift", "out"):
        assert up(**{name: None}) == ARG
    assert up(B=0) == SHAPE
    for V in (0, 8, 24, 144, 256, -16):
        assert up(V=V) == SHAPE and up(V=V, skip=None) == SHAPE
    assert up(x=None, V=24) == ARG
    pool = lambda **k: lib.mvn_v2v_maxpool2(k.get("x", 1), k.get("out", 1), k.get("B", 2), k.get("V", 32),     # noqa: E731
                                            k.get("C", 32), None)
    assert pool(x=None) == ARG and pool(out=None) == ARG
    assert pool(B=0) == SHAPE
    for V in (0, 1, 3, 33, 258, -2):
        assert pool(V=V) == SHAPE
    for C in (0, 4, 12, 136, 256, -8):
        assert pool(C=C) == SHAPE


# ---------------------------------------------------------------- packing and folding
def unpack_wide(packed, cin):
    """The (64, cin, 3, 3, 3) weight from the documented layout of mvn_v2v_conv3_wide (mvn_hip.h):
    [tap][kp][m][lane][j] = W[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]."""
    return unpack_conv3(packed, 64, cin)


def unpack_wide_skip(packed):
    return unpack_skip(packed, 64, 32)


def unpack_upsample(packed):
    """The (64, 32, 2, 2, 2) ConvTranspose3d weight from mvn_v2v_upsample2's documented layout:
    [kp][m][lane][j] = W[32 kp + 8 (lane >> 4) + j][16 (m & 1) + (lane & 15)][dx][dy][dz],
    (dx*2 + dy)*2 + dz = m >> 1."""
    return unpack_up(packed, 64, 32)


@pytest.mark.parametrize("cin", (32, 64))
def test_fold_res3d_block_wide(cin):
    from mvn_rocm import v2v
    blk = randomise(Res3DBlock(cin, 64), seed=cin)
    p = v2v.fold_res3d_block_wide(blk, device="cpu")
    rb = blk.res_branch
    with torch.no_grad():
        for packed, scale, shift, conv, bn, ci in ((p.packed1, p.scale1, p.shift1, rb[0], rb[1], cin),
                                                   (p.packed2, p.scale2, p.shift2, rb[3], rb[4], 64)):
            assert packed.dtype == torch.bfloat16 and scale.dtype == shift.dtype == torch.float32
            assert packed.numel() * 2 == 27 * 64 * ci * 2
            assert torch.equal(unpack_wide(packed, ci), conv.weight.bfloat16().double())
            s, t = bn_fold64(conv, bn)
            assert torch.equal(scale, s.float()) and torch.equal(shift, t.float())
        if cin == 32:
            assert torch.equal(unpack_wide_skip(p.skip_packed), blk.skip_con[0].weight.view(64, 32).bfloat16().double())
            s, t = bn_fold64(blk.skip_con[0], blk.skip_con[1])
            assert torch.equal(p.skip_scale, s.float()) and torch.equal(p.skip_shift, t.float())
        else:
            assert p.skip_packed is None and p.skip_scale is None and p.skip_shift is None


def test_fold_res3d_block_wide_without_bias():
    from mvn_rocm import v2v
    blk = randomise(Res3DBlock(32, 64, bias=False), seed=5)
    p = v2v.fold_res3d_block_wide(blk, device="cpu")
    with torch.no_grad():
        s, t = bn_fold64(blk.res_branch[0], blk.res_branch[1])
    assert torch.equal(p.shift1, t.float()) and torch.equal(p.scale1, s.float())


def test_fold_upsample_block():
    from mvn_rocm import v2v
    blk = randomise(Upsample3DBlock(64, 32), seed=9)
    p = v2v.fold_upsample_block(blk, device="cpu")
    conv, bn = blk.block[0], blk.block[1]
    with torch.no_grad():
        assert p.packed.dtype == torch.bfloat16 and p.packed.numel() * 2 == 64 * 32 * 8 * 2
        assert torch.equal(unpack_upsample(p.packed), conv.weight.bfloat16().double())
        s, t = bn_fold64(conv, bn)
        assert torch.equal(p.scale, s.float()) and torch.equal(p.shift, t.float())
        assert float(conv.bias.abs().max()) > 0                 # the bias is in the fold


def test_folds_refuse_other_modules():
    from mvn_rocm import v2v
    for cin, cout in ((16, 32), (32, 32), (64, 128), (128, 64)):
        with pytest.raises(RuntimeError):
            v2v.fold_res3d_block_wide(randomise(Res3DBlock(cin, cout), 1), device="cpu")
    blk = randomise(Res3DBlock(64, 64), 1)
    blk.res_branch[0].stride = (2, 2, 2)
    with pytest.raises(RuntimeError, match="stride"):
        v2v.fold_res3d_block_wide(blk, device="cpu")
    blk = randomise(Res3DBlock(64, 64), 1)
    blk.res_branch[3].padding = (0, 0, 0)
    with pytest.raises(RuntimeError, match="padding"):
        v2v.fold_res3d_block_wide(blk, device="cpu")
    blk = randomise(Res3DBlock(32, 64), 1)
    blk.res_branch[1] = nn.BatchNorm3d(64, track_running_stats=False)
    with pytest.raises(RuntimeError, match="running statistics"):
        v2v.fold_res3d_block_wide(blk, device="cpu")
    blk = randomise(Res3DBlock(32, 64), 1)
    blk.skip_con = nn.Sequential()                              # 32 -> 64 cannot be an identity
    with pytest.raises(RuntimeError, match="empty skip_con"):
        v2v.fold_res3d_block_wide(blk, device="cpu")
    for cin, cout in ((128, 64), (64, 64), (32, 32)):
        with pytest.raises(RuntimeError):
            v2v.fold_upsample_block(randomise(Upsample3DBlock(cin, cout), 1), device="cpu")
    up = randomise(Upsample3DBlock(64, 32), 1)
    up.block[0].stride = (1, 1, 1)
    with pytest.raises(RuntimeError, match="stride"):
        v2v.fold_upsample_block(up, device="cpu")
    up = randomise(Upsample3DBlock(64, 32), 1)
    up.block[1] = nn.BatchNorm3d(32, track_running_stats=False)
    with pytest.raises(RuntimeError, match="running statistics"):
        v2v.fold_upsample_block(up, device="cpu")
    with pytest.raises(RuntimeError):
        v2v.fold_upsample_block(randomise(Res3DBlock(64, 64), 1), device="cpu")


# ---------------------------------------------------------------- the Python layer's refusals
def test_max_pool2_cl_refusals():
    from mvn_rocm import v2v
    with pytest.raises(TypeError, match="bfloat16"):
        v2v.max_pool2_cl(vol(1, 4, 32, torch.float32))
    with pytest.raises(RuntimeError, match=r"\(B, V, V, V, C\)"):
        v2v.max_pool2_cl(torch.zeros(1, 4, 4, 6, 32, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match=r"\(B, V, V, V, C\)"):
        v2v.max_pool2_cl(torch.zeros(4, 4, 4, 32, dtype=torch.bfloat16))
    for V in (3, 258):
        with pytest.raises(RuntimeError, match="even"):
            v2v.max_pool2_cl(vol(1, V, 8))
    for C in (4, 12, 136):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            v2v.max_pool2_cl(vol(1, 4, C))
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.max_pool2_cl(vol(1, 4, 32).requires_grad_())
    with pytest.raises(RuntimeError, match="MI355X only"):     # valid, on the CPU: no fallback
        v2v.max_pool2_cl(vol(1, 4, 32))


def test_conv3_wide_refusals():
    from mvn_rocm import v2v
    p = v2v.fold_res3d_block_wide(randomise(Res3DBlock(32, 64), 2), device="cpu")
    q = v2v.fold_res3d_block_wide(randomise(Res3DBlock(64, 64), 3), device="cpu")
    c1, c2, sk = (p.packed1, p.scale1, p.shift1), (p.packed2, p.scale2, p.shift2), (p.skip_packed, p.skip_scale, p.skip_shift)
    with pytest.raises(TypeError, match="bfloat16"):
        v2v.v2v_conv3_wide(vol(1, 16, 32, torch.float32), *c1)
    with pytest.raises(RuntimeError, match="32 | 64"):
        v2v.v2v_conv3_wide(vol(1, 16, 16), *c1)
    with pytest.raises(RuntimeError, match="32 | 64"):
        v2v.v2v_conv3_wide(torch.zeros(1, 16, 16, 32, 32, dtype=torch.bfloat16), *c1)
    for V in (8, 24, 144):
        with pytest.raises(RuntimeError, match="multiple of 16"):
            v2v.v2v_conv3_wide(vol(1, V, 32), *c1)
    with pytest.raises(RuntimeError, match="packed weights"):    # 32-channel weights, 64-channel volume
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c1)
    with pytest.raises(RuntimeError, match="packed weights"):
        v2v.v2v_conv3_wide(vol(1, 16, 32), c1[0], c1[1].double(), c1[2])
    # skip arguments that make no sense
    with pytest.raises(RuntimeError, match="without a skip volume"):
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, None, *sk)
    with pytest.raises(RuntimeError, match="identity skip takes no"):
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, vol(1, 16, 64), None, sk[1], None)
    with pytest.raises(RuntimeError, match="pointwise skip needs"):
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, vol(1, 16, 32), sk[0], None, sk[2])
    with pytest.raises(RuntimeError, match="skip must be"):      # identity skip with 32 channels
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, vol(1, 16, 32))
    with pytest.raises(RuntimeError, match="skip must be"):      # pointwise skip with 64 channels
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, vol(1, 16, 64), *sk)
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.v2v_conv3_wide(vol(2, 16, 64), *c2, vol(1, 16, 64))
    with pytest.raises(TypeError, match="skip must be bfloat16"):
        v2v.v2v_conv3_wide(vol(1, 16, 64), *c2, vol(1, 16, 64, torch.float32))
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.v2v_conv3_wide(vol(1, 16, 32).requires_grad_(), *c1)
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.v2v_conv3_wide(vol(1, 16, 32), c1[0], c1[1].clone().requires_grad_(), c1[2])
    with torch.no_grad():                                        # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="MI355X only"):
            v2v.v2v_conv3_wide(vol(1, 16, 32).requires_grad_(), *c1)
    # the block: the volume's channels must fit the parameters' skip kind
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.res3d_block_wide(vol(1, 16, 64), p)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.res3d_block_wide(vol(1, 16, 32), q)
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.res3d_block_wide(vol(1, 16, 64).requires_grad_(), q)
    with pytest.raises(RuntimeError, match="MI355X only"):
        v2v.res3d_block_wide(vol(1, 16, 64), q)


def test_upsample2_add_refusals():
    from mvn_rocm import v2v
    p = v2v.fold_upsample_block(randomise(Upsample3DBlock(64, 32), 4), device="cpu")
    with pytest.raises(TypeError, match="bfloat16"):
        v2v.upsample2_add(vol(1, 16, 64, torch.float32), p)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.upsample2_add(vol(1, 16, 32), p)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.upsample2_add(torch.zeros(1, 16, 16, 32, 64, dtype=torch.bfloat16), p)
    for V in (8, 24, 144):
        with pytest.raises(RuntimeError, match="multiple of 16"):
            v2v.upsample2_add(vol(1, V, 64), p)
    with pytest.raises(RuntimeError, match="packed weights"):
        v2v.upsample2_add(vol(1, 16, 64), (p.packed.view(16, 2, 64, 8), p.scale, p.shift))
    with pytest.raises(RuntimeError, match="skip must be"):
        v2v.upsample2_add(vol(1, 16, 64), p, vol(1, 32, 64))
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.upsample2_add(vol(1, 16, 64), p, vol(1, 16, 32))
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.upsample2_add(vol(2, 16, 64), p, vol(1, 32, 32))
    with pytest.raises(TypeError, match="skip must be bfloat16"):
        v2v.upsample2_add(vol(1, 16, 64), p, vol(1, 32, 32, torch.float32))
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.upsample2_add(vol(1, 16, 64), p, vol(1, 32, 32).requires_grad_())
    with pytest.raises(RuntimeError, match="MI355X only"):
        v2v.upsample2_add(vol(1, 16, 64), p, vol(1, 32, 32))


def test_ops_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import _ops  # noqa: F401
    with FakeTensorMode():
        x = torch.empty(2, 32, 32, 32, 32, dtype=torch.bfloat16)
        p = torch.ops.mvn_rocm.v2v_maxpool2(x)
        assert tuple(p.shape) == (2, 16, 16, 16, 32) and p.dtype == torch.bfloat16
        w = torch.empty(27, 1, 4, 64, 8, dtype=torch.bfloat16)
        s = torch.empty(64)
        y = torch.ops.mvn_rocm.v2v_conv3_wide(p, w, s, s, NONE, None, None, None, None)
        assert tuple(y.shape) == (2, 16, 16, 16, 64) and y.dtype == torch.bfloat16
        wu, su = torch.empty(2, 16, 64, 8, dtype=torch.bfloat16), torch.empty(32)
        u = torch.ops.mvn_rocm.v2v_upsample2(y, wu, su, su, x)
        assert tuple(u.shape) == (2, 32, 32, 32, 32) and u.dtype == torch.bfloat16


# ---------------------------------------------------------------- V2VEval and v2v_interior
def test_v2veval_refuses_an_unknown_half_res():
    from mvn_rocm import v2v
    m = randomise(V2VModel(32, 17), seed=11)
    with pytest.raises(ValueError, match="half_res"):
        v2v.V2VEval.from_reference(m, half_res="nonsense", device="cpu")


def test_v2veval_half_res_kernels_holds_the_folded_level():
    from mvn_rocm import v2v
    m = randomise(V2VModel(32, 17), seed=11)
    ev = v2v.V2VEval.from_reference(m, half_res="kernels", device="cpu")
    assert len(ev.half_res) == 4
    for name in ("skip_res1", "encoder_res1", "skip_res2", "decoder_res1", "decoder_upsample1"):
        assert not hasattr(ev.interior, name)
    assert hasattr(ev.interior, "encoder_res2") and hasattr(ev.interior, "decoder_upsample2")
    ev = v2v.V2VEval.from_reference(m, device="cpu")            # the default: everything pooled in torch
    assert ev.half_res is None and hasattr(ev.interior, "encoder_res1")


def test_v2v_interior_equals_the_encoder_decoder_minus_skip_res1():
    """``v2v_interior`` through ``v2v_interior_deep`` is EncoderDecorder.forward without the skip_res1
    branch, bit for bit on the CPU."""
    from mvn_rocm import v2v
    ed = randomise(EncoderDecorder(), seed=21)
    x = torch.randn(1, 32, 32, 32, 32, generator=torch.Generator().manual_seed(22))
    with torch.no_grad():
        got = v2v.v2v_interior(ed, x)
        want = ed(x) - ed.skip_res1(x)                          # not bit-exact: only a sanity scale
        e1 = ed.encoder_res1(ed.encoder_pool1(x))
        s2 = ed.skip_res2(e1)
        y = ed.encoder_res2(ed.encoder_pool2(e1))
        s3 = ed.skip_res3(y)
        y = ed.encoder_res3(ed.encoder_pool3(y))
        s4 = ed.skip_res4(y)
        y = ed.encoder_res4(ed.encoder_pool4(y))
        s5 = ed.skip_res5(y)
        y = ed.mid_res(ed.encoder_res5(ed.encoder_pool5(y)))
        y = ed.decoder_upsample5(ed.decoder_res5(y)) + s5
        y = ed.decoder_upsample4(ed.decoder_res4(y)) + s4
        y = ed.decoder_upsample3(ed.decoder_res3(y)) + s3
        deep = ed.decoder_upsample2(ed.decoder_res2(y))
        exact = ed.decoder_upsample1(ed.decoder_res1(deep + s2))
        assert torch.equal(v2v.v2v_interior_deep(ed, e1), deep)
    assert torch.equal(got, exact)
    assert torch.equal(got + ed.skip_res1(x).detach(), ed(x).detach())     # the stand-in's forward
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-5
