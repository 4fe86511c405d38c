"""The V2V's 128-channel levels (csrc/v2v_deep.hip): folding and packing, the C ABI's argument
checks, the Python layer's refusals and V2VEval's ``deep`` option — no GPU needed (only validation
paths are called; they return before any HIP call)."""
import pytest
import torch
from torch import nn

from v2v_kit import (Basic3DBlock, Res3DBlock, Upsample3DBlock, V2VModel, bn_fold64, randomise, unpack_conv3, unpack_skip,
                     unpack_upsample, vol)

ARG, SHAPE = -1, -2
NONE, IDENTITY, POINTWISE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- C argument validation
def test_size_functions(lib):
    assert lib.mvn_v2v_conv3_deep_packed_weight_bytes(64) == 27 * 2 * 8 * 64 * 8 * 2 == 442368
    assert lib.mvn_v2v_conv3_deep_packed_weight_bytes(128) == 27 * 4 * 8 * 64 * 8 * 2 == 884736
    for cin in (0, 16, 32, 96, 256, -64):
        assert lib.mvn_v2v_conv3_deep_packed_weight_bytes(cin) == 0
    assert lib.mvn_v2v_conv3_deep_skip_packed_weight_bytes(64) == 2 * 8 * 64 * 8 * 2 == 128 * 64 * 2
    for cin in (0, 32, 128):
        assert lib.mvn_v2v_conv3_deep_skip_packed_weight_bytes(cin) == 0
    assert lib.mvn_v2v_upsample2_deep_packed_weight_bytes(64) == 4 * 32 * 64 * 8 * 2 == 128 * 64 * 8 * 2
    assert lib.mvn_v2v_upsample2_deep_packed_weight_bytes(128) == 4 * 64 * 64 * 8 * 2 == 128 * 128 * 8 * 2
    for cout in (0, 32, 96, 256):
        assert lib.mvn_v2v_upsample2_deep_packed_weight_bytes(cout) == 0


def _deep(lib, **k):
    mode = k.get("mode", NONE)
    skip = k.get("skip", None if mode == NONE else 1)
    pw = 1 if mode == POINTWISE else None
    return lib.mvn_v2v_conv3_deep(k.get("x", 1), k.get("cin", 128), k.get("w", 1), k.get("scale", 1), k.get("shift", 1),
                                  mode, skip, k.get("skip_cin", {NONE: 0, IDENTITY: 128, POINTWISE: 64}.get(mode, 0)),
                                  k.get("ws", pw), k.get("ss", pw), k.get("ts", pw), k.get("out", 1), k.get("B", 2),
                                  k.get("D", 5), None)


def test_conv3_deep_argument_validation(lib):
    """Every documented error code, with no device: the checks run before any HIP call."""
    for name in ("x", "w", "scale", "shift", "out"):
        assert _deep(lib, **{name: None}) == ARG
    assert _deep(lib, mode=3) == ARG and _deep(lib, mode=-1) == ARG
    assert _deep(lib, mode=NONE, skip=1) == ARG
    assert _deep(lib, mode=NONE, ws=1) == ARG and _deep(lib, mode=NONE, ss=1) == ARG
    assert _deep(lib, mode=IDENTITY, skip=None) == ARG
    assert _deep(lib, mode=IDENTITY, ws=1) == ARG and _deep(lib, mode=IDENTITY, ts=1) == ARG
    assert _deep(lib, mode=POINTWISE, skip=None) == ARG
    for name in ("ws", "ss", "ts"):
        assert _deep(lib, mode=POINTWISE, **{name: None}) == ARG
    for mode in (NONE, IDENTITY, POINTWISE):
        assert _deep(lib, mode=mode, B=0) == SHAPE and _deep(lib, mode=mode, B=-2) == SHAPE
        for D in (0, 65, -1, 128):
            assert _deep(lib, mode=mode, D=D) == SHAPE
        for cin in (0, 32, 96, 256):
            assert _deep(lib, mode=mode, cin=cin) == SHAPE
    assert _deep(lib, mode=IDENTITY, skip_cin=64) == SHAPE
    assert _deep(lib, mode=POINTWISE, skip_cin=128) == SHAPE and _deep(lib, mode=POINTWISE, skip_cin=32) == SHAPE
    assert _deep(lib, B=2 ** 31 - 1, D=64) == SHAPE              # B * D^3 overflows
    assert _deep(lib, B=1024, D=64) == SHAPE                     # 8 B D^3 = 2^31: the upsampled voxel count overflows
    assert _deep(lib, x=None, D=0) == ARG                        # an argument error comes first
    assert _deep(lib, mode=5, cin=32) == ARG
    assert _deep(lib, mode=NONE, skip=1, D=65) == ARG


def test_wide_conv_is_not_widened(lib):
    """The existing entry point keeps its shapes: 128 channels and the small extents stay refused."""
    wide = lambda cin, V: lib.mvn_v2v_conv3_wide(1, cin, 1, 1, 1, NONE, None, 0, None, None, None, 1, 2, V, None)   # noqa: E731
    assert wide(128, 32) == SHAPE and wide(64, 8) == SHAPE and wide(64, 5) == SHAPE
    assert lib.mvn_v2v_conv3_wide_packed_weight_bytes(128) == 0
    assert lib.mvn_v2v_upsample2(1, 1, 1, 1, None, 1, 2, 8, None) == SHAPE


def test_upsample2_deep_argument_validation(lib):
    up = lambda **k: lib.mvn_v2v_upsample2_deep(k.get("x", 1), k.get("cout", 128), k.get("w", 1), k.get("scale", 1),   # noqa: E731
                                                k.get("shift", 1), k.get("skip", 1), k.get("out", 1), k.get("B", 2),
                                                k.get("D", 5), None)
    for name in ("x", "w", "scale", "shift", "out"):
        assert up(**{name: None}) == ARG
    assert up(B=0) == SHAPE and up(B=-1) == SHAPE
    for D in (0, 65, -1):
        assert up(D=D) == SHAPE and up(D=D, skip=None) == SHAPE
    for cout in (0, 32, 96, 256):
        assert up(cout=cout) == SHAPE
    assert up(B=1024, D=64) == SHAPE
    assert up(x=None, D=0) == ARG and up(out=None, cout=32) == ARG


# ---------------------------------------------------------------- packing and folding
def unpack_deep(packed, cin):
    """The (128, cin, 3, 3, 3) weight from the documented layout of mvn_v2v_conv3_deep (mvn_hip.h):
    [tap][kp][m][lane][j] = W[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]."""
    return unpack_conv3(packed, 128, cin)


def unpack_deep_skip(packed):
    assert tuple(packed.shape) == (2, 8, 64, 8)
    return unpack_skip(packed, 128, 64)


def unpack_upsample_deep(packed, cout):
    """The (128, cout, 2, 2, 2) ConvTranspose3d weight from mvn_v2v_upsample2_deep's documented
    layout, H = cout / 16: [kp][m][lane][j] = W[32 kp + 8 (lane >> 4) + j][16 (m % H) + (lane & 15)]
    [dx][dy][dz], (dx*2 + dy)*2 + dz = m // H."""
    return unpack_upsample(packed, 128, cout)


@pytest.mark.parametrize("cin", (64, 128))
def test_pack_functions_against_an_independent_unpack(cin):
    """Random weights through the three pack functions and back through the documented formulas."""
    from mvn_rocm import v2v
    g = torch.Generator().manual_seed(cin)
    w = torch.randn(128, cin, 3, 3, 3, generator=g).bfloat16().double()
    assert torch.equal(unpack_deep(v2v.pack_conv3_deep_weight(w), cin), w)
    ws = torch.randn(128, 64, generator=g).bfloat16().double()
    assert torch.equal(unpack_deep_skip(v2v.pack_pointwise_skip_deep_weight(ws)), ws)
    wu = torch.randn(128, cin, 2, 2, 2, generator=g).bfloat16().double()        # cout = cin: 64 | 128
    assert torch.equal(unpack_upsample_deep(v2v.pack_upsample_deep_weight(wu), cin), wu)


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "no_bias"))
@pytest.mark.parametrize("cin", (64, 128))
def test_fold_res3d_block_deep(cin, bias):
    from mvn_rocm import v2v
    blk = randomise(Res3DBlock(cin, 128, bias=bias), seed=cin)
    p = v2v.fold_res3d_block_deep(blk, device="cpu")
    assert isinstance(p, v2v.Res3DParams)
    rb = blk.res_branch
    with torch.no_grad():
        for packed, scale, shift, conv, bn, ci in ((p.packed1, p.scale1, p.shift1, rb[0], rb[1], cin),
                                                   (p.packed2, p.scale2, p.shift2, rb[3], rb[4], 128)):
            assert packed.dtype == torch.bfloat16 and scale.dtype == shift.dtype == torch.float32
            assert packed.numel() * 2 == 27 * 128 * ci * 2
            assert torch.equal(unpack_deep(packed, ci), conv.weight.bfloat16().double())
            s, t = bn_fold64(conv, bn)
            assert torch.equal(scale, s.float()) and torch.equal(shift, t.float())
            assert (conv.bias is not None) == bias
        if cin == 64:
            assert torch.equal(unpack_deep_skip(p.skip_packed), blk.skip_con[0].weight.view(128, 64).bfloat16().double())
            s, t = bn_fold64(blk.skip_con[0], blk.skip_con[1])
            assert torch.equal(p.skip_scale, s.float()) and torch.equal(p.skip_shift, t.float())
        else:
            assert p.skip_packed is None and p.skip_scale is None and p.skip_shift is None


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "no_bias"))
@pytest.mark.parametrize("cout", (64, 128))
def test_fold_upsample_block_deep(cout, bias):
    from mvn_rocm import v2v
    blk = Upsample3DBlock(128, cout)
    if not bias:
        blk.block[0] = nn.ConvTranspose3d(128, cout, 2, 2, bias=False)
    blk = randomise(blk, seed=9 + cout)
    p = v2v.fold_upsample_block_deep(blk, device="cpu")
    assert isinstance(p, v2v.UpsampleParams)
    conv, bn = blk.block[0], blk.block[1]
    with torch.no_grad():
        assert p.packed.dtype == torch.bfloat16 and p.packed.numel() * 2 == 128 * cout * 8 * 2
        assert torch.equal(unpack_upsample_deep(p.packed, cout), conv.weight.bfloat16().double())
        s, t = bn_fold64(conv, bn)
        assert torch.equal(p.scale, s.float()) and torch.equal(p.shift, t.float())
        if bias:
            assert float(conv.bias.abs().max()) > 0             # the bias is in the fold


def test_folds_refuse_other_modules():
    from mvn_rocm import v2v
    for cin, cout in ((16, 32), (32, 32), (32, 64), (64, 64), (128, 64)):
        with pytest.raises(RuntimeError, match="expected a"):
            v2v.fold_res3d_block_deep(randomise(Res3DBlock(cin, cout), 1), device="cpu")
    with pytest.raises(RuntimeError, match="Res3DBlock"):
        v2v.fold_res3d_block_deep(randomise(Basic3DBlock(128, 128, 3), 1), device="cpu")
    blk = randomise(Res3DBlock(128, 128), 1)
    blk.res_branch[0].stride = (2, 2, 2)
    with pytest.raises(RuntimeError, match="stride"):
        v2v.fold_res3d_block_deep(blk, device="cpu")
    blk = randomise(Res3DBlock(64, 128), 1)
    blk.res_branch[1] = nn.BatchNorm3d(128, track_running_stats=False)
    with pytest.raises(RuntimeError, match="running statistics"):
        v2v.fold_res3d_block_deep(blk, device="cpu")
    blk = randomise(Res3DBlock(64, 128), 1)
    blk.skip_con = nn.Sequential()                              # 64 -> 128 cannot be an identity
    with pytest.raises(RuntimeError, match="empty skip_con"):
        v2v.fold_res3d_block_deep(blk, device="cpu")
    for cin, cout in ((64, 32), (64, 64), (128, 32)):
        with pytest.raises(RuntimeError, match="ConvTranspose3d weight"):
            v2v.fold_upsample_block_deep(randomise(Upsample3DBlock(cin, cout), 1), device="cpu")
    up = randomise(Upsample3DBlock(128, 64), 1)
    up.block[0].stride = (1, 1, 1)
    with pytest.raises(RuntimeError, match="stride"):
        v2v.fold_upsample_block_deep(up, device="cpu")
    with pytest.raises(RuntimeError, match="ConvTranspose3d"):
        v2v.fold_upsample_block_deep(randomise(Basic3DBlock(128, 128, 3), 1), device="cpu")
    with pytest.raises(RuntimeError):
        v2v.fold_upsample_block_deep(randomise(Res3DBlock(128, 128), 1), device="cpu")


# ---------------------------------------------------------------- the Python layer's refusals
def test_conv3_deep_refusals():
    from mvn_rocm import v2v
    p = v2v.fold_res3d_block_deep(randomise(Res3DBlock(64, 128), 2), device="cpu")
    q = v2v.fold_res3d_block_deep(randomise(Res3DBlock(128, 128), 3), device="cpu")
    c1, c2, sk = (p.packed1, p.scale1, p.shift1), (p.packed2, p.scale2, p.shift2), (p.skip_packed, p.skip_scale, p.skip_shift)
    with pytest.raises(TypeError, match="x_cl must be bfloat16"):
        v2v.v2v_conv3_deep(vol(1, 5, 64, torch.float32), *c1)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.v2v_conv3_deep(vol(1, 5, 32), *c1)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.v2v_conv3_deep(torch.zeros(1, 5, 5, 6, 64, dtype=torch.bfloat16), *c1)
    with pytest.raises(RuntimeError, match=r"D must be in \[1, 64\]"):
        v2v.v2v_conv3_deep(vol(1, 65, 64), *c1)
    with pytest.raises(RuntimeError, match="packed weights"):    # 64-channel weights, 128-channel volume
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c1)
    with pytest.raises(RuntimeError, match="packed weights"):
        v2v.v2v_conv3_deep(vol(1, 5, 64), c1[0], c1[1].double(), c1[2])
    with pytest.raises(RuntimeError, match="without a skip volume"):
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, None, *sk)
    with pytest.raises(RuntimeError, match="identity skip takes no"):
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 5, 128), None, sk[1], None)
    with pytest.raises(RuntimeError, match="pointwise skip needs"):
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 5, 64), sk[0], None, sk[2])
    with pytest.raises(RuntimeError, match="skip must be"):      # identity skip with 64 channels
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 5, 64))
    with pytest.raises(RuntimeError, match="skip must be"):      # pointwise skip with 128 channels
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 5, 128), *sk)
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.v2v_conv3_deep(vol(2, 5, 128), *c2, vol(1, 5, 128))
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 4, 128))
    with pytest.raises(TypeError, match="skip must be bfloat16"):
        v2v.v2v_conv3_deep(vol(1, 5, 128), *c2, vol(1, 5, 128, torch.float32))
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.v2v_conv3_deep(vol(1, 5, 64).requires_grad_(), *c1)
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.v2v_conv3_deep(vol(1, 5, 64), c1[0], c1[1].clone().requires_grad_(), c1[2])
    with torch.no_grad():                                        # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="MI355X only"):
            v2v.v2v_conv3_deep(vol(1, 5, 64).requires_grad_(), *c1)
    for D in (1, 3, 7):                                          # valid, on the CPU: no fallback
        with pytest.raises(RuntimeError, match="MI355X only"):
            v2v.v2v_conv3_deep(vol(1, D, 128), *c2, vol(1, D, 128))
    # the block: the volume's channels must fit the parameters' skip kind
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.res3d_block_deep(vol(1, 5, 128), p)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.res3d_block_deep(vol(1, 5, 64), q)
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.res3d_block_deep(vol(1, 5, 128).requires_grad_(), q)
    with pytest.raises(RuntimeError, match="MI355X only"):
        v2v.Res3DBlockDeepCL(q)(vol(1, 5, 128))


@pytest.mark.parametrize("cout", (64, 128))
def test_upsample2_add_deep_refusals(cout):
    from mvn_rocm import v2v
    p = v2v.fold_upsample_block_deep(randomise(Upsample3DBlock(128, cout), 4), device="cpu")
    with pytest.raises(TypeError, match="x_cl must be bfloat16"):
        v2v.upsample2_add_deep(vol(1, 3, 128, torch.float32), p)
    with pytest.raises(RuntimeError, match="x_cl must be"):
        v2v.upsample2_add_deep(vol(1, 3, 64), p)
    with pytest.raises(RuntimeError, match="packed weights"):
        v2v.upsample2_add_deep(vol(1, 3, 128), (p.packed.view(-1, 4, 64, 8), p.scale, p.shift))
    with pytest.raises(RuntimeError, match="scale and shift"):
        v2v.upsample2_add_deep(vol(1, 3, 128), (p.packed, p.scale[:32], p.shift[:32]))
    with pytest.raises(RuntimeError, match="skip must be"):
        v2v.upsample2_add_deep(vol(1, 3, 128), p, vol(1, 6, 192 - cout))
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.upsample2_add_deep(vol(1, 3, 128), p, vol(1, 3, cout))
    with pytest.raises(RuntimeError, match="does not match"):
        v2v.upsample2_add_deep(vol(2, 3, 128), p, vol(1, 6, cout))
    with pytest.raises(TypeError, match="skip must be bfloat16"):
        v2v.upsample2_add_deep(vol(1, 3, 128), p, vol(1, 6, cout, torch.float32))
    with pytest.raises(RuntimeError, match="inference-only"):
        v2v.upsample2_add_deep(vol(1, 3, 128), p, vol(1, 6, cout).requires_grad_())
    with pytest.raises(RuntimeError, match="MI355X only"):
        v2v.Upsample3DBlockDeepCL(p)(vol(1, 3, 128), vol(1, 6, cout))


def test_ops_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import _ops  # noqa: F401
    with FakeTensorMode():
        s = torch.empty(128)
        for cin in (64, 128):
            x = torch.empty(3, 5, 5, 5, cin, dtype=torch.bfloat16)
            w = torch.empty(27, cin // 32, 8, 64, 8, dtype=torch.bfloat16)
            y = torch.ops.mvn_rocm.v2v_conv3_deep(x, w, s, s, NONE, None, None, None, None)
            assert tuple(y.shape) == (3, 5, 5, 5, 128) and y.dtype == torch.bfloat16
        for cout in (64, 128):
            wu, su = torch.empty(4, 8 * cout // 16, 64, 8, dtype=torch.bfloat16), torch.empty(cout)
            u = torch.ops.mvn_rocm.v2v_upsample2_deep(y, wu, su, su, None)
            assert tuple(u.shape) == (3, 10, 10, 10, cout) and u.dtype == torch.bfloat16


# ---------------------------------------------------------------- V2VEval
def test_v2veval_deep_option():
    """deep="kernels" needs half_res="kernels" and holds the folded 128-channel modules: the model has
    12 Res3DBlocks with 128 output channels (encoder_res2..5, mid_res, decoder_res5..2, skip_res3..5)
    and 4 upsamples that take 128 channels, 16 modules.  The other settings are structurally as before."""
    from mvn_rocm import v2v
    m = randomise(V2VModel(32, 17), seed=11)
    with pytest.raises(ValueError, match="deep.*half_res|half_res.*deep"):
        v2v.V2VEval.from_reference(m, half_res="torch", deep="kernels", device="cpu")
    with pytest.raises(ValueError, match="deep.*half_res|half_res.*deep"):
        v2v.V2VEval.from_reference(m, deep="kernels", device="cpu")
    with pytest.raises(ValueError, match="deep"):
        v2v.V2VEval.from_reference(m, half_res="kernels", deep="nonsense", device="cpu")
    ev = v2v.V2VEval.from_reference(m, half_res="kernels", deep="kernels", device="cpu")
    assert ev.interior is None and len(ev.half_res) == 4
    assert len(ev.deep) == len(v2v.DEEP_RES) + len(v2v.DEEP_UP) == 16
    assert sum(isinstance(d, v2v.Res3DBlockDeepCL) for d in ev.deep) == 12
    assert sum(isinstance(d, v2v.Upsample3DBlockDeepCL) for d in ev.deep) == 4
    assert ev.deep[0].skip_packed is not None and all(d.skip_packed is None for d in ev.deep[1:12])
    assert [d.scale.numel() for d in ev.deep[12:]] == [128, 128, 128, 64]
    assert not any(isinstance(mod, (nn.Conv3d, nn.ConvTranspose3d, nn.BatchNorm3d)) for mod in ev.modules())
    ev = v2v.V2VEval.from_reference(m, half_res="kernels", device="cpu")       # as before
    assert ev.deep is None and len(ev.half_res) == 4
    assert hasattr(ev.interior, "encoder_res2") and hasattr(ev.interior, "decoder_upsample2")
    assert not hasattr(ev.interior, "encoder_res1")
    ev = v2v.V2VEval.from_reference(m, device="cpu")                           # the default
    assert ev.deep is None and ev.half_res is None and hasattr(ev.interior, "encoder_res1")
