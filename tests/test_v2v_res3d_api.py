"""Full-resolution Res3DBlocks: folding and packing, the C ABI's argument checks and the Python
layer — no GPU needed (only validation paths are called; they return before any HIP call)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.fx.experimental.proxy_tensor import make_fx

from v2v_kit import IDENTITY, NONE, POINTWISE, Res3DBlock, V2VModel, randomise, unpack_conv3, unpack_skip as unpack_skip_w
from v2v_kit import bn_fold64 as fold64

CO = 32
ARG, SHAPE, WORKSPACE = -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- C argument validation
def test_size_functions(lib):
    assert lib.mvn_v2v_conv3_packed_weight_bytes(32) == lib.mvn_v2v_conv3_packed_weight_bytes(16) == 27 * 2 * 64 * 8 * 2
    assert lib.mvn_v2v_conv3_packed_weight_bytes(8) == 0 and lib.mvn_v2v_conv3_packed_weight_bytes(64) == 0
    assert lib.mvn_v2v_conv3_skip_packed_weight_bytes(16) == 2 * 64 * 8 * 2
    assert lib.mvn_v2v_conv3_skip_packed_weight_bytes(32) == 0
    per = lambda V: V ** 3 * 32 * 2                                                   # noqa: E731
    assert lib.mvn_v2v_res3d_workspace_bytes(3, 64) == 3 * per(64)
    # default: one group's hidden volume within 128 MiB, at most 64 frames
    assert (128 << 20) // per(64) == 8
    assert lib.mvn_v2v_res3d_workspace_bytes(0, 64) == lib.mvn_v2v_res3d_workspace_bytes(-1, 64) == 8 * per(64)
    assert lib.mvn_v2v_res3d_workspace_bytes(0, 16) == 64 * per(16)
    assert lib.mvn_v2v_res3d_workspace_bytes(0, 256) == 1 * per(256)
    assert lib.mvn_v2v_res3d_workspace_bytes(2, 24) == 0 and lib.mvn_v2v_res3d_workspace_bytes(2, 272) == 0
    assert lib.mvn_v2v_res3d_workspace_bytes(2, 0) == 0


def _conv3(lib, **k):
    mode = k.get("mode", NONE)
    skip = k.get("skip", None if mode == NONE else 1)
    pw = 1 if mode == POINTWISE else None
    return lib.mvn_v2v_conv3(k.get("x", 1), k.get("cin", 32), k.get("w", 1), k.get("scale", 1), k.get("shift", 1), mode,
                             skip, k.get("skip_cin", {NONE: 0, IDENTITY: 32, POINTWISE: 16}.get(mode, 0)),
                             k.get("ws", pw), k.get("ss", pw), k.get("ts", pw), k.get("out", 1), k.get("B", 2),
                             k.get("V", 32), None)


def test_conv3_argument_validation(lib):
    """Every documented error code, with no device: the checks run before any HIP call.  (A valid
    argument set is not tried: it would launch.)"""
    for name in ("x", "w", "scale", "shift", "out"):
        assert _conv3(lib, **{name: None}) == ARG
    assert _conv3(lib, mode=3) == ARG and _conv3(lib, mode=-1) == ARG                 # unknown skip mode
    # a skip pointer that contradicts the mode
    assert _conv3(lib, mode=NONE, skip=1) == ARG
    assert _conv3(lib, mode=NONE, ws=1) == ARG and _conv3(lib, mode=NONE, ss=1) == ARG
    assert _conv3(lib, mode=IDENTITY, skip=None) == ARG
    assert _conv3(lib, mode=IDENTITY, ws=1) == ARG and _conv3(lib, mode=IDENTITY, ts=1) == ARG
    assert _conv3(lib, mode=POINTWISE, skip=None) == ARG
    for name in ("ws", "ss", "ts"):
        assert _conv3(lib, mode=POINTWISE, **{name: None}) == ARG
    for mode in (NONE, IDENTITY, POINTWISE):
        assert _conv3(lib, mode=mode, B=0) == SHAPE and _conv3(lib, mode=mode, B=-2) == SHAPE
        for V in (0, 8, 24, 40, 272, 512, -16):
            assert _conv3(lib, mode=mode, V=V) == SHAPE
        for cin in (0, 8, 24, 64):
            assert _conv3(lib, mode=mode, cin=cin) == SHAPE
    assert _conv3(lib, mode=IDENTITY, skip_cin=16) == SHAPE
    assert _conv3(lib, mode=POINTWISE, skip_cin=32) == SHAPE
    assert _conv3(lib, mode=POINTWISE, cin=16, skip_cin=8) == SHAPE
    # an argument error is reported before a shape error
    assert _conv3(lib, x=None, V=24) == ARG


def _res3d(lib, **k):
    mode = k.get("mode", IDENTITY)
    cin = k.get("cin", 32 if mode == IDENTITY else 16)
    pw = 1 if mode == POINTWISE else None
    G, V = k.get("G", 2), k.get("V", 32)
    ws_bytes = k.get("wsb", lib.mvn_v2v_res3d_workspace_bytes(G, V if V in range(16, 257, 16) else 16))
    return lib.mvn_v2v_res3d(k.get("x", 1), cin, k.get("w1", 1), k.get("s1", 1), k.get("t1", 1), k.get("w2", 1),
                             k.get("s2", 1), k.get("t2", 1), mode, k.get("ws", pw), k.get("ss", pw), k.get("ts", pw),
                             k.get("out", 1), k.get("work", 1), ws_bytes, G, k.get("B", 3), V, None)


def test_res3d_argument_validation(lib):
    for mode in (IDENTITY, POINTWISE):
        for name in ("x", "w1", "s1", "t1", "w2", "s2", "t2", "out"):
            assert _res3d(lib, mode=mode, **{name: None}) == ARG
        assert _res3d(lib, mode=mode, B=0) == SHAPE
        for V in (0, 8, 24, 272):
            assert _res3d(lib, mode=mode, V=V) == SHAPE
        assert _res3d(lib, mode=mode, cin=8) == SHAPE
        assert _res3d(lib, mode=mode, work=None) == WORKSPACE
        assert _res3d(lib, mode=mode, wsb=lib.mvn_v2v_res3d_workspace_bytes(2, 32) - 1) == WORKSPACE
        # the default group (64 frames at 32^3) needs its own, larger workspace
        assert _res3d(lib, mode=mode, G=0, wsb=lib.mvn_v2v_res3d_workspace_bytes(2, 32)) == WORKSPACE
    assert _res3d(lib, mode=NONE, cin=32) == ARG and _res3d(lib, mode=3) == ARG          # a block has a skip
    assert _res3d(lib, mode=IDENTITY, ws=1) == ARG and _res3d(lib, mode=POINTWISE, ss=None) == ARG
    assert _res3d(lib, mode=IDENTITY, cin=16) == SHAPE and _res3d(lib, mode=POINTWISE, cin=32) == SHAPE


# ---------------------------------------------------------------- packing and folding
def unpack3(packed):
    """The (32, 32, 3, 3, 3) weight from the documented layout of mvn_v2v_conv3 (mvn_hip.h):
    [tap = (dx*3 + dy)*3 + dz][m][lane][j] = W[16 m + (lane & 15)][8 (lane >> 4) + j][dx][dy][dz]."""
    return unpack_conv3(packed, CO)


def unpack_skip(packed):
    return unpack_skip_w(packed, CO)


def bf16r(t):
    return t.float().to(torch.bfloat16).double()


@pytest.mark.parametrize("cin,bias", ((16, True), (32, True), (32, False), (16, False)))
def test_fold_and_pack(cin, bias):
    """fold_res3d_block against a float64 fold written out here: unpacking under the documented
    layout gives the bf16-rounded weights (K-slots >= cin zero), scale and shift are the fold
    rounded to f32; a block with an empty skip_con has no skip parameters; a conv without bias."""
    from mvn_rocm import v2v
    block = randomise(Res3DBlock(cin, CO, bias=bias), seed=3 + cin)
    p = v2v.fold_res3d_block(block, device="cpu")
    rb = block.res_branch
    for packed, scale, shift, conv, bn, c in ((p.packed1, p.scale1, p.shift1, rb[0], rb[1], cin),
                                              (p.packed2, p.scale2, p.shift2, rb[3], rb[4], 32)):
        assert tuple(packed.shape) == (27, 2, 64, 8) and packed.dtype == torch.bfloat16
        W = unpack3(packed)
        assert torch.equal(W[:, :c], bf16r(conv.weight.detach())) and not bool(W[:, c:].any())
        s, t = fold64(conv, bn)
        assert scale.dtype == torch.float32 and torch.equal(scale, s.float()) and torch.equal(shift, t.float())
    if cin == 32:
        assert p.skip_packed is None and p.skip_scale is None and p.skip_shift is None
    else:
        assert tuple(p.skip_packed.shape) == (2, 64, 8) and p.skip_packed.dtype == torch.bfloat16
        Ws = unpack_skip(p.skip_packed)
        assert torch.equal(Ws[:, :16], bf16r(block.skip_con[0].weight.detach().view(CO, 16))) and not bool(Ws[:, 16:].any())
        s, t = fold64(block.skip_con[0], block.skip_con[1])
        assert torch.equal(p.skip_scale, s.float()) and torch.equal(p.skip_shift, t.float())


def test_fold_refuses_wrong_shapes():
    from mvn_rocm import v2v
    with pytest.raises(RuntimeError, match="Conv3d weight"):
        v2v.fold_res3d_block(Res3DBlock(32, 64), device="cpu")
    with pytest.raises(RuntimeError, match="Conv3d weight"):
        v2v.fold_res3d_block(Res3DBlock(8, 32), device="cpu")
    b = Res3DBlock(32, 32)
    b.res_branch[0] = nn.Conv3d(32, 32, 5, 1, 2)
    with pytest.raises(RuntimeError, match="Conv3d weight"):
        v2v.fold_res3d_block(b, device="cpu")
    b = Res3DBlock(32, 32)
    b.res_branch[3] = nn.Conv3d(32, 32, 3, 2, 1)
    with pytest.raises(RuntimeError, match="stride 1"):
        v2v.fold_res3d_block(b, device="cpu")
    b = Res3DBlock(16, 32)
    b.skip_con = nn.Sequential()
    with pytest.raises(RuntimeError, match="empty skip_con"):
        v2v.fold_res3d_block(b, device="cpu")
    b = Res3DBlock(32, 32)
    b.res_branch = nn.Sequential(*list(b.res_branch)[:3])
    with pytest.raises(RuntimeError, match="res_branch of 5"):
        v2v.fold_res3d_block(b, device="cpu")
    b = Res3DBlock(32, 32)
    b.res_branch[1] = nn.BatchNorm3d(32, track_running_stats=False)
    with pytest.raises(RuntimeError, match="running statistics"):
        v2v.fold_res3d_block(b, device="cpu")


@pytest.mark.parametrize("cin", (16, 32))
def test_packed_dataflow_reproduces_conv3d(cin):
    """The kernel's MFMA dataflow replayed on the CPU from the packed buffers alone, on integer
    data: per tap, A = packed[tap][m] as 16 rows x 32 K-slots (lane (r, g) holds slots 8 g .. 8 g + 7
    of row r), B = the tap-shifted zero-padded input with K-slot 8 g + j = channel 8 g + j (zeros
    for the slots >= cin), D row r of half m = output channel 16 m + r.  Equal to conv3d exactly;
    the same for the pointwise skip's packed weights."""
    from mvn_rocm import v2v
    g = torch.Generator().manual_seed(cin)
    V = 6
    x = torch.randint(-4, 5, (1, cin, V, V, V), generator=g).double()
    w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).double()
    A = v2v.pack_conv3_weight(w).double().view(27, 2, 4, 16, 8)            # [tap][m][g][row][j]
    xp = F.pad(x[0], (1, 1, 1, 1, 1, 1))
    D = torch.zeros(2, 16, V, V, V, dtype=torch.float64)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                sh = xp[:, dx:dx + V, dy:dy + V, dz:dz + V]                   # input voxel (x + dx - 1, ...)
                frag = torch.zeros(32, V, V, V, dtype=torch.float64)
                frag[:cin] = sh
                D += torch.einsum("mgrj,gjxyz->mrxyz", A[(dx * 3 + dy) * 3 + dz], frag.view(4, 8, V, V, V))
    assert torch.equal(D.view(CO, V, V, V), F.conv3d(x, w, padding=1)[0])
    ws = torch.randint(-4, 5, (CO, 16), generator=g).double()
    skip = torch.randint(-4, 5, (16, V, V, V), generator=g).double()
    As = v2v.pack_pointwise_skip_weight(ws).double().view(2, 4, 16, 8)
    frag = torch.zeros(32, V, V, V, dtype=torch.float64)
    frag[:16] = skip
    Ds = torch.einsum("mgrj,gjxyz->mrxyz", As, frag.view(4, 8, V, V, V))
    assert torch.equal(Ds.view(CO, V, V, V), F.conv3d(skip[None], ws.view(CO, 16, 1, 1, 1))[0])


# ---------------------------------------------------------------- Python checks
def _params(cin):
    from mvn_rocm import v2v
    return v2v.fold_res3d_block(randomise(Res3DBlock(cin, CO), 3), device="cpu")


def test_python_refusals():
    from mvn_rocm import v2v
    p32, p16 = _params(32), _params(16)
    x = torch.zeros(1, 16, 16, 16, 32, dtype=torch.bfloat16)
    x16 = torch.zeros(1, 16, 16, 16, 16, dtype=torch.bfloat16)
    c1 = (p32.packed1, p32.scale1, p32.shift1)
    with pytest.raises(RuntimeError, match="v2v_conv3 is inference-only"):
        v2v.v2v_conv3(x, p32.packed1, p32.scale1.clone().requires_grad_(), p32.shift1)
    with pytest.raises(RuntimeError, match="res3d_block is inference-only"):
        v2v.res3d_block(x.float().requires_grad_(), p32)
    with torch.no_grad():
        for bad in (x.float(), x.half()):
            with pytest.raises(TypeError, match="bfloat16"):
                v2v.v2v_conv3(bad, *c1)
            with pytest.raises(TypeError, match="bfloat16"):
                v2v.res3d_block(bad, p32)
        with pytest.raises(TypeError, match="skip must be bfloat16"):
            v2v.v2v_conv3(x, *c1, x.float())
        for bad in (x[..., :8], x[:, :, :, :8], x[0], torch.zeros(1, 24, 24, 24, 32, dtype=torch.bfloat16)):
            with pytest.raises(RuntimeError, match="x_cl must be|multiple of 16"):
                v2v.v2v_conv3(bad, *c1)
        with pytest.raises(RuntimeError, match="x_cl must be"):
            v2v.res3d_block(x16, p32)                                  # an identity block takes 32 channels
        with pytest.raises(RuntimeError, match="x_cl must be"):
            v2v.res3d_block(x, p16)                                    # a pointwise block takes 16
        with pytest.raises(RuntimeError, match="skip must be"):
            v2v.v2v_conv3(x, *c1, x16)                                 # identity skip: 32 channels
        with pytest.raises(RuntimeError, match="skip must be"):
            v2v.v2v_conv3(x, *c1, x, p16.skip_packed, p16.skip_scale, p16.skip_shift)
        with pytest.raises(RuntimeError, match="does not match"):
            v2v.v2v_conv3(x, *c1, torch.zeros(2, 16, 16, 16, 32, dtype=torch.bfloat16))
        with pytest.raises(RuntimeError, match="without a skip volume"):
            v2v.v2v_conv3(x, *c1, None, p16.skip_packed, p16.skip_scale, p16.skip_shift)
        with pytest.raises(RuntimeError, match="fold_res3d_block"):
            v2v.v2v_conv3(x, p32.packed1.float(), p32.scale1, p32.shift1)
        with pytest.raises(RuntimeError, match="fold_res3d_block"):
            v2v.v2v_conv3(x, p32.packed1, p32.scale1[:16], p32.shift1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.v2v_conv3(x, *c1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.v2v_conv3(x, *c1, x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.res3d_block(x16, p16)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.Res3DBlockCL(p32)(x)


def test_fake_ops_trace():
    """Under make_fx with fake tensors both functions record their torch.ops.mvn_rocm op, with
    the shapes and dtypes of the real ones (no GPU, no library call)."""
    from mvn_rocm import v2v
    p32, p16 = _params(32), _params(16)
    x16 = torch.zeros(2, 16, 16, 16, 16, dtype=torch.bfloat16)

    def path(x16, *flat):
        a, b = v2v.Res3DParams(*flat[:9]), v2v.Res3DParams(*flat[9:], None, None, None)
        h = v2v.v2v_conv3(x16, a.packed1, a.scale1, a.shift1)
        y = v2v.v2v_conv3(h, a.packed2, a.scale2, a.shift2, x16, a.skip_packed, a.skip_scale, a.skip_shift)
        z = v2v.v2v_conv3(y, b.packed1, b.scale1, b.shift1, y)
        return h, y, z, v2v.res3d_block(x16, a, 1), v2v.res3d_block(z, b)

    with torch.no_grad():
        gm = make_fx(path, tracing_mode="fake")(x16, *p16, *p32[:6])
    targets = {str(n.target) for n in gm.graph.nodes if n.op == "call_function"}
    assert "mvn_rocm.v2v_conv3.default" in targets and "mvn_rocm.v2v_res3d.default" in targets, targets
    metas = [o.meta["val"] for o in [n for n in gm.graph.nodes if n.op == "output"][0].args[0]]
    assert [tuple(m.shape) for m in metas] == [(2, 16, 16, 16, 32)] * 5
    assert all(m.dtype == torch.bfloat16 for m in metas)


# ---------------------------------------------------------------- the modules
def test_modules_from_reference():
    from mvn_rocm import v2v
    block = randomise(Res3DBlock(16, CO), 8)
    mod = v2v.Res3DBlockCL.from_reference(block, device="cpu")
    want = v2v.fold_res3d_block(block, device="cpu")
    assert not list(mod.parameters()) and set(dict(mod.named_buffers())) == set(v2v.Res3DParams._fields)
    for a, b in zip(mod.params, want):
        assert torch.equal(a, b)
    ident = v2v.Res3DBlockCL.from_reference(randomise(Res3DBlock(32, CO), 9), device="cpu")
    assert ident.skip_packed is None and set(dict(ident.named_buffers())) == set(v2v.Res3DParams._fields[:6])
    m = randomise(V2VModel(32, 5), 10)
    ev = v2v.V2VEval.from_reference(m, device="cpu")
    assert len(ev.front_res) == 3 and ev.interior_dtype == torch.float32
    assert not hasattr(ev.interior, "skip_res1") and hasattr(m.encoder_decoder, "skip_res1")     # the model is untouched
    assert not any(p.requires_grad for p in ev.parameters())
    for blk, ref in ((ev.front_res[0], m.front_layers[1]), (ev.front_res[2], m.front_layers[3]),
                     (ev.skip_res1, m.encoder_decoder.skip_res1), (ev.back_res, m.back_layers[0])):
        for a, b in zip(blk.params, v2v.fold_res3d_block(ref, device="cpu")):
            assert (a is None and b is None) or torch.equal(a, b)
    half = v2v.V2VEval.from_reference(m, interior_dtype=torch.bfloat16, device="cpu")
    assert next(half.interior.parameters()).dtype == torch.bfloat16
    # the interior is the model's forward between skip_res1 and the last add (f32 on the CPU)
    x = torch.randn(1, 32, 32, 32, 32, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ed = m.encoder_decoder
        assert torch.equal(v2v.v2v_interior(ev.interior, x) + ed.skip_res1(x), ed(x))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ev(torch.zeros(1, 32, 32, 32, 32, dtype=torch.bfloat16), torch.zeros(1, 32, 32, 32, 3))
