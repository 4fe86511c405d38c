"""V2V head: folding and packing, the C ABI's argument checks and the Python layer — no GPU
needed (only validation paths are called; they return before any HIP call)."""
import pytest
import torch
from torch import nn
from torch.fx.experimental.proxy_tensor import make_fx

from test_gpu_v2v_head import C, bf16r, make_head, restate, unpack, exceed, CAP, LOOSE
from v2v_kit import Basic3DBlock


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- folding and packing
@pytest.mark.parametrize("J", (1, 17, 32))
def test_fold_and_pack(J):
    """Unpacking `packed` under the documented layout gives the bf16-rounded W1..W3 (rows >= J of
    W3 zero); scale_shift and bias3 are the float64 fold rounded to f32."""
    from mvn_rocm import v2v
    b1, b2, out = make_head(J, 3)
    packed, ss, b3 = v2v.fold_v2v_head(b1, b2, out, device="cpu")
    assert packed.shape == (3, 2, 64, 8) and packed.dtype == torch.bfloat16
    assert ss.shape == (2, 2, C) and ss.dtype == torch.float32 and b3.shape == (J,) and b3.dtype == torch.float32
    for l, conv in enumerate((b1.block[0], b2.block[0], out)):
        W = torch.zeros(C, C, dtype=torch.float64)
        W[:conv.weight.shape[0]] = bf16r(conv.weight.detach().reshape(-1, C))
        assert torch.equal(unpack(packed, l), W)
    for l, blk in enumerate((b1, b2)):
        conv, bn = blk.block[0], blk.block[1]
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t = (conv.bias.detach().double() - bn.running_mean.double()) * s + bn.bias.detach().double()
        assert torch.equal(ss[l, 0], s.float()) and torch.equal(ss[l, 1], t.float())
    assert torch.equal(b3, out.bias.detach())
    assert torch.equal(v2v.head_kslot(0), torch.arange(C))
    assert sorted(v2v.head_kslot(1).tolist()) == list(range(C))          # a permutation


def test_fold_refuses_wrong_shapes():
    from mvn_rocm import v2v
    b1, b2, out = make_head(17, 3)
    with pytest.raises(RuntimeError, match="Conv3d weight"):
        v2v.fold_v2v_head(Basic3DBlock(C, 16, 1), b2, out, device="cpu")
    with pytest.raises(RuntimeError, match="Conv3d weight"):
        v2v.fold_v2v_head(b1, Basic3DBlock(C, C, 3), out, device="cpu")
    with pytest.raises(RuntimeError, match="output_conv"):
        v2v.fold_v2v_head(b1, b2, nn.Conv3d(16, 17, 1), device="cpu")
    with pytest.raises(RuntimeError, match="output_conv"):
        v2v.fold_v2v_head(b1, b2, nn.Conv3d(C, 33, 1), device="cpu")


def test_packed_dataflow_is_the_restatement():
    """The kernel's register dataflow, replayed on the CPU from `packed` alone: a lane's 8 MFMA
    results (tile m, register i -> channel 16 m + 4 g + i) are its next B operand in the order
    (m, i), which is K-slots 8 g .. 8 g + 7.  Equal to the restatement up to f64 summation
    order, and to the stock modules up to the bf16 roundings."""
    from mvn_rocm import v2v
    J = 17
    b1, b2, out = make_head(J, 5)
    packed, ss, b3 = v2v.fold_v2v_head(b1, b2, out, device="cpu")
    x = torch.randn(1, C, 50, generator=torch.Generator().manual_seed(1))
    A = packed.double().view(3, 2, 4, 16, 8)                  # [layer][m][g'][row][j]
    frag = bf16r(x)[0].view(4, 8, 50)                         # layer 1's B operand: [g][j][voxel] = channel 8 g + j
    for l in range(3):
        D = torch.einsum("mgrj,gjv->mrv", A[l], frag)        # [m][row][voxel]
        if l < 2:
            D = D.view(2, 4, 4, 50)                           # [m][g][i][voxel]: row = 4 g + i
            s = ss[l, 0].double().view(2, 4, 4, 1)            # channel 16 m + 4 g + i
            t = ss[l, 1].double().view(2, 4, 4, 1)
            h = bf16r(torch.relu(D * s + t))
            frag = h.permute(1, 0, 2, 3).reshape(4, 8, 50)    # [g][j = 4 m + i][voxel]
    y = D.reshape(C, 50)[:J] + b3.double().view(J, 1)
    ref = restate(x, packed, ss, b3)[0]
    assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    with torch.no_grad():
        stock = out(b2(b1(x.view(1, C, 50, 1, 1)))).view(J, 50).double()
    assert float((y - stock).abs().max()) <= 2.0 ** -5 * float(stock.abs().max())   # three bf16 roundings deep


def test_cap_evidence_on_the_cpu_pair():
    """The restatement in f32 against f64 at 32,768 voxels (unit-normal input, Xavier-scale
    weights): the share of voxels over the tight bar stays far under the 0.5 % cap."""
    from mvn_rocm import v2v
    params = v2v.fold_v2v_head(*make_head(17, 51), device="cpu")
    x = torch.randn(1, C, 32768, generator=torch.Generator().manual_seed(17))
    frac, worst = exceed(restate(x, *params, dtype=torch.float32), restate(x, *params))
    assert frac <= CAP / 5 and worst <= LOOSE, (frac, worst)


# ---------------------------------------------------------------- C argument validation
def test_size_functions(lib):
    assert lib.mvn_v2v_head_packed_weight_bytes(17) == 3 * 2 * 64 * 8 * 2
    assert lib.mvn_v2v_head_packed_weight_bytes(1) == lib.mvn_v2v_head_packed_weight_bytes(32) == 6144
    assert lib.mvn_v2v_head_packed_weight_bytes(0) == 0 and lib.mvn_v2v_head_packed_weight_bytes(33) == 0

    def formula(G, J, Vx, Vy, Vz):
        return (G * J * Vx * Vy * Vz * 4 + 15) // 16 * 16 + lib.mvn_softargmax3d_workspace_bytes(G, J, Vx, Vy, Vz)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(2, 17, 64, 64, 64) == formula(2, 17, 64, 64, 64)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(3, 1, 3, 5, 7) == formula(3, 1, 3, 5, 7)
    # default: one group's f32 logits within 128 MiB: 7 frames at 64^3 with J = 17; at most 64
    assert (128 << 20) // (17 * 64 ** 3 * 4) == 7
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(0, 17, 64, 64, 64) == formula(7, 17, 64, 64, 64)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(-1, 17, 64, 64, 64) == formula(7, 17, 64, 64, 64)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(0, 17, 8, 8, 8) == formula(64, 17, 8, 8, 8)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(0, 32, 128, 128, 128) == formula(1, 32, 128, 128, 128)
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(2, 0, 8, 8, 8) == 0
    assert lib.mvn_v2v_head_softargmax_workspace_bytes(2, 17, 8, 0, 8) == 0


def _head(lib, **k):
    return lib.mvn_v2v_head(k.get("x", 1), k.get("xd", 0), k.get("xl", 0), k.get("w", 1), k.get("ss", 1),
                            k.get("b3", 1), k.get("out", 1), k.get("od", 0), k.get("B", 2), k.get("J", 17),
                            k.get("Vx", 8), k.get("Vy", 8), k.get("Vz", 8), None)


def test_head_argument_validation(lib):
    for name in ("x", "w", "ss", "b3", "out"):
        assert _head(lib, **{name: None}) == -1
    assert _head(lib, xl=2) == -1 and _head(lib, xl=-1) == -1              # unknown layout
    assert _head(lib, xd=0, xl=1) == -3                                    # f32 channels-last
    assert _head(lib, xd=2) == -3 and _head(lib, od=5) == -3               # unknown dtypes
    assert _head(lib, J=0) == -2 and _head(lib, J=33) == -2
    assert _head(lib, B=0) == -2 and _head(lib, Vy=0) == -2 and _head(lib, Vz=-3) == -2
    assert _head(lib, Vx=2048, Vy=2048, Vz=2048) == -2                     # voxel count past 2^30
    assert _head(lib, B=2 ** 31 - 1, Vx=1024, Vy=1024, Vz=1024) == -2      # element count overflows


def _one_call(lib, **k):
    ws = lib.mvn_v2v_head_softargmax_workspace_bytes(k.get("G", 2), k.get("J", 17), 8, 8, k.get("Vz", 8))
    return lib.mvn_v2v_head_softargmax(k.get("x", 1), k.get("xd", 0), k.get("xl", 0), k.get("w", 1), k.get("ss", 1),
                                       k.get("b3", 1), k.get("coords", 1), k.get("cub", None), k.get("tr", 0), 1.0,
                                       k.get("sm", 1), k.get("xyz", 1), k.get("vol", None), k.get("od", 0),
                                       k.get("ws", 1), k.get("wsb", ws), k.get("G", 2), k.get("B", 3),
                                       k.get("J", 17), 8, 8, k.get("Vz", 8), None)


def test_one_call_argument_validation(lib):
    for name in ("x", "w", "ss", "b3", "xyz"):
        assert _one_call(lib, **{name: None}) == -1
    assert _one_call(lib, coords=None) == -1                               # neither coordinate source
    assert _one_call(lib, cub=1) == -1                                     # both
    assert _one_call(lib, xl=3) == -1 and _one_call(lib, sm=2) == -1 and _one_call(lib, tr=2) == -1
    assert _one_call(lib, xd=0, xl=1) == -3 and _one_call(lib, xd=7) == -3 and _one_call(lib, od=2) == -3
    assert _one_call(lib, J=0) == -2 and _one_call(lib, J=33) == -2 and _one_call(lib, B=0) == -2
    assert _one_call(lib, coords=None, cub=1, Vz=16) == -2                 # cuboids need a cubic volume
    assert _one_call(lib, ws=None) == -5
    ws = lib.mvn_v2v_head_softargmax_workspace_bytes(2, 17, 8, 8, 8)
    assert _one_call(lib, wsb=ws - 1) == -5
    # the default group (64 frames at 8^3) needs its own, larger workspace
    assert _one_call(lib, G=0, wsb=ws) == -5


# ---------------------------------------------------------------- Python checks
def _params(J=17):
    from mvn_rocm import v2v
    return v2v.fold_v2v_head(*make_head(J, 3), device="cpu")


def test_python_refusals():
    from mvn_rocm import v2v
    params = _params()
    x, coords = torch.zeros(1, C, 4, 4, 4), torch.zeros(1, 4, 4, 4, 3)
    with pytest.raises(RuntimeError, match="v2v_head is inference-only"):
        v2v.v2v_head(x.clone().requires_grad_(), *params)
    with pytest.raises(RuntimeError, match="v2v_head_softargmax is inference-only"):
        v2v.v2v_head_softargmax(x.clone().requires_grad_(), *params, coords)
    with torch.no_grad():
        with pytest.raises(TypeError, match="float32 and bfloat16"):
            v2v.v2v_head(x.half(), *params)
        with pytest.raises(TypeError, match="float32 and bfloat16"):
            v2v.v2v_head(x, *params, out_dtype=torch.float16)
        with pytest.raises(TypeError, match="float32 and bfloat16"):
            v2v.v2v_head_softargmax(x.half(), *params, coords)
        with pytest.raises(TypeError, match="channels-last"):
            v2v.v2v_head(x.permute(0, 2, 3, 4, 1), *params, channels_last=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.v2v_head(x, *params)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            v2v.v2v_head_softargmax(x, *params, coords)
        with pytest.raises(RuntimeError, match="x must be"):
            v2v.v2v_head(torch.zeros(1, 16, 4, 4, 4), *params)
        with pytest.raises(RuntimeError, match="does not match"):
            v2v.v2v_head_softargmax(x, *params, torch.zeros(1, 4, 4, 5, 3))
        with pytest.raises(RuntimeError, match="fold_v2v_head"):
            v2v.v2v_head(x, params[0].float(), params[1], params[2])


def test_fake_ops_trace():
    """Under make_fx with fake tensors both functions record their torch.ops.mvn_rocm op, with
    the shapes and dtypes of the real ones (no GPU, no library call)."""
    from mvn_rocm import v2v
    params = _params(17)
    x, coords = torch.randn(2, C, 3, 5, 7), torch.randn(2, 3, 5, 7, 3)

    def path(x, coords, *p):
        y = v2v.v2v_head(x, *p)
        y16 = v2v.v2v_head(x.to(torch.bfloat16).permute(0, 2, 3, 4, 1), *p, out_dtype=torch.bfloat16, channels_last=True)
        kp, vol = v2v.v2v_head_softargmax(x, *p, coords, multiplier=2.0)
        kp2, none = v2v.v2v_head_softargmax(x, *p, coords, softmax=False, out_dtype=torch.bfloat16,
                                            return_volumes=False, group_frames=1)
        assert none is None
        return y, y16, kp, vol, kp2

    with torch.no_grad():
        gm = make_fx(path, tracing_mode="fake")(x, coords, *params)
    targets = {str(n.target) for n in gm.graph.nodes if n.op == "call_function"}
    assert "mvn_rocm.v2v_head.default" in targets and "mvn_rocm.v2v_head_softargmax.default" in targets, targets
    outs = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    metas = [o.meta["val"] for o in outs]
    assert [tuple(m.shape) for m in metas] == [(2, 17, 3, 5, 7), (2, 17, 3, 5, 7), (2, 17, 3), (2, 17, 3, 5, 7), (2, 17, 3)]
    assert [m.dtype for m in metas] == [torch.float32, torch.bfloat16, torch.float32, torch.float32, torch.float32]


# ---------------------------------------------------------------- V2VHead and v2v_trunk
class _StandIn(nn.Module):
    """The reference V2VModel's attribute names (v2v.py:141-160), from torch.nn."""

    def __init__(self, J):
        super().__init__()
        b1, b2, out = make_head(J, 9)
        self.front_layers = nn.Sequential(nn.Conv3d(4, C, 1))
        self.encoder_decoder = nn.Sequential(nn.ReLU())
        self.back_layers = nn.Sequential(nn.Conv3d(C, C, 3, padding=1), b1, b2)
        self.output_layer = out


def test_from_reference_and_trunk():
    from mvn_rocm import v2v
    m = _StandIn(5).eval()
    head = v2v.V2VHead.from_reference(m, device="cpu")
    want = v2v.fold_v2v_head(m.back_layers[1], m.back_layers[2], m.output_layer, device="cpu")
    assert set(dict(head.named_buffers())) == {"packed", "scale_shift", "bias3"} and not list(head.parameters())
    for name, t in zip(("packed", "scale_shift", "bias3"), want):
        assert torch.equal(getattr(head, name), t)
    x = torch.randn(1, 4, 4, 4, 4, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        trunk = v2v.v2v_trunk(m, x)
        assert torch.equal(trunk, m.back_layers[0](m.encoder_decoder(m.front_layers(x))))
        # trunk + stock tail = the model's own forward (v2v.py:164-169)
        full = m.output_layer(m.back_layers(m.encoder_decoder(m.front_layers(x))))
        assert torch.equal(m.output_layer(m.back_layers[2](m.back_layers[1](trunk))), full)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            head(trunk, torch.zeros(1, 4, 4, 4, 3), 2.0)
