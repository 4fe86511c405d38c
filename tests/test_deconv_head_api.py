"""The backbone's deconv head (csrc/deconv_head.hip, mvn_rocm/backbone.py) without a GPU: the packed
weight layout against include/mvn_hip.h, the fold against float64, every MVN_ERR_ARG path of the C
entry (the checks run before any HIP call), ``from_reference``'s refusals on stand-in modules, the
autograd refusal, the fake kernel and the traced op."""
import pytest
import torch
from torch import nn

from deconv_kit import COUT, index_weight, randomise2d, unpack_by_loops, unpack_deconv4
from v2v_kit import bf16r

OK, ARG = 0, -1
F32, BF16 = 0, 1
NCHW, NHWC = 0, 1
A = 4096                         # a 16-byte aligned stand-in address: the checks never dereference it


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- packing and folding
@pytest.mark.parametrize("cin", (32, 64, 2048))
def test_pack_round_trip_by_the_documented_layout(cin, lib):
    from mvn_rocm import backbone
    w = index_weight(cin) if cin < 2048 else bf16r(torch.randn(cin, COUT, 4, 4, generator=torch.Generator().manual_seed(1)))
    packed = backbone.pack_deconv4_weight(w.double())
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous()
    assert packed.numel() * 2 == lib.mvn_deconv4s2_packed_weight_bytes(cin)
    assert torch.equal(unpack_deconv4(packed, cin), w.double())
    picks = [(0, 0, 0, 0, 0), (15, cin // 32 - 1, 15, 63, 7), (6, 0, 3, 17, 5), (9, cin // 32 - 1, 8, 40, 2)]
    for (ci, co, ky, kx), v in unpack_by_loops(packed, cin, picks):
        assert v == float(w[ci, co, ky, kx])


def test_pack_rounds_once_to_bf16():
    from mvn_rocm import backbone
    w = torch.randn(32, COUT, 4, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    assert torch.equal(unpack_deconv4(backbone.pack_deconv4_weight(w), 32), w.float().bfloat16().double())


def test_packed_weight_bytes(lib):
    assert lib.mvn_deconv4s2_packed_weight_bytes(256) == 16 * 8 * 16 * 64 * 8 * 2
    for cin in (0, 16, 48, 2080, -32):
        assert lib.mvn_deconv4s2_packed_weight_bytes(cin) == 0


@pytest.mark.parametrize("cin", (32, 48))
def test_pack_refuses_other_shapes(cin):
    from mvn_rocm import backbone
    bad = torch.zeros(32, 128, 4, 4) if cin == 32 else torch.zeros(48, COUT, 4, 4)
    with pytest.raises(RuntimeError, match="expected a|multiple of 32"):
        backbone.pack_deconv4_weight(bad.double())


@pytest.mark.parametrize("bias", (False, True), ids=("no_bias", "bias"))
def test_fold_against_float64(bias):
    from mvn_rocm import backbone
    d, bn = nn.ConvTranspose2d(64, COUT, 4, 2, 1, bias=bias), nn.BatchNorm2d(COUT)
    randomise2d(nn.Sequential(d, bn), seed=3)
    p = backbone.fold_deconv_block(d, bn, device="cpu")
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    b = d.bias.detach().double() if bias else torch.zeros(COUT, dtype=torch.float64)
    t = (b - bn.running_mean.double()) * s + bn.bias.detach().double()
    assert torch.equal(p.scale, s.float()) and torch.equal(p.shift, t.float())
    assert p.scale.dtype == torch.float32 and tuple(p.packed.shape) == (16, 2, 16, 64, 8)
    assert torch.equal(unpack_deconv4(p.packed, 64), d.weight.detach().float().bfloat16().double())


# ---------------------------------------------------------------- C argument validation
def _deconv(lib, **k):
    return lib.mvn_deconv4s2(k.get("x", A), k.get("w", A), k.get("scale", A), k.get("shift", A), k.get("out", A),
                             k.get("layout", NHWC), k.get("od", BF16), k.get("n", 2), k.get("cin", 256), k.get("H", 5),
                             k.get("W", 7), None)


def test_argument_validation(lib):
    """Every refusal is MVN_ERR_ARG and comes before any HIP call (there is no device here)."""
    for name in ("x", "w", "scale", "shift", "out"):
        assert _deconv(lib, **{name: None}) == ARG
    for cin in (0, 16, 48, 2080, -32, 4096):
        assert _deconv(lib, cin=cin) == ARG
    assert _deconv(lib, H=0) == ARG and _deconv(lib, W=0) == ARG and _deconv(lib, H=-1) == ARG
    assert _deconv(lib, n=-1) == ARG
    for layout in (-1, 2, 7):
        assert _deconv(lib, layout=layout) == ARG
    for od in (-1, 2, 7):
        assert _deconv(lib, od=od, layout=NCHW) == ARG
    assert _deconv(lib, layout=NHWC, od=F32) == ARG                      # the channels-last output is bf16
    # an image over the buffer limit: the f32 output image of H * W input pixels is 4096 H W bytes
    assert _deconv(lib, H=1024, W=512) == ARG                            # 2^31 bytes
    assert _deconv(lib, H=724, W=724, n=0) == OK                         # 524,176 pixels: just below
    assert _deconv(lib, H=725, W=724) == ARG
    assert _deconv(lib, cin=2048, H=512, W=512, n=0) == OK               # 2^30 bytes of input
    assert _deconv(lib, cin=2048, H=1024, W=512) == ARG                  # 2^31 bytes of input
    assert _deconv(lib, H=2 ** 30, W=2 ** 30) == ARG                     # H * W itself beyond int
    assert _deconv(lib, n=2 ** 40, H=1, W=1) == ARG                      # more blocks than an int counts
    # element-aligned (odd) pointers: the kernel's loads and stores are 16 bytes wide
    for name in ("x", "w", "scale", "shift", "out"):
        assert _deconv(lib, **{name: A + 2}) == ARG
    # an empty batch is nothing to do, but its errors come first
    assert _deconv(lib, n=0) == OK and _deconv(lib, n=0, layout=NCHW, od=F32) == OK
    assert _deconv(lib, n=0, x=None) == ARG and _deconv(lib, n=0, cin=48) == ARG and _deconv(lib, n=0, H=0) == ARG


# ---------------------------------------------------------------- the Python wrapper
def _params(cin=64):
    return (torch.zeros(16, cin // 32, 16, 64, 8, dtype=torch.bfloat16), torch.ones(COUT), torch.zeros(COUT))


def test_wrapper_refusals():
    from mvn_rocm import backbone
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        backbone.deconv4s2(x, _params())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        backbone.deconv4s2(x, _params(), "nchw", torch.float32)
    with pytest.raises(TypeError, match="x_cl must be bfloat16"):
        backbone.deconv4s2(x.float(), _params())
    with pytest.raises(RuntimeError, match="x_cl must be"):
        backbone.deconv4s2(x[0], _params())
    with pytest.raises(ValueError, match="out_layout"):
        backbone.deconv4s2(x, _params(), "nhwc")
    with pytest.raises(TypeError, match="channels-last output is bfloat16"):
        backbone.deconv4s2(x, _params(), "cl", torch.float32)
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        backbone.deconv4s2(x, _params(), "nchw", torch.float16)
    for cin in (16, 48, 2080):
        with pytest.raises(RuntimeError, match="multiple of 32"):
            backbone.deconv4s2(torch.zeros(1, 2, 2, cin, dtype=torch.bfloat16), _params())
    with pytest.raises(RuntimeError, match="fold_deconv_block returns"):
        backbone.deconv4s2(x, _params(32))
    with pytest.raises(RuntimeError, match="fold_deconv_block returns"):
        backbone.deconv4s2(x, (_params()[0], torch.ones(128), torch.zeros(128)))
    with pytest.raises(RuntimeError, match="at least 1"):
        backbone.deconv4s2(torch.zeros(1, 0, 5, 64, dtype=torch.bfloat16), _params())


def test_autograd_is_refused():
    from mvn_rocm import backbone
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    pk, sc, sh = _params()
    with pytest.raises(RuntimeError, match="inference-only.*deconv_layers"):
        backbone.deconv4s2(x.clone().requires_grad_(), (pk, sc, sh))
    with pytest.raises(RuntimeError, match="inference-only"):
        backbone.deconv4s2(x, (pk, sc.clone().requires_grad_(), sh))
    with torch.no_grad():                                      # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            backbone.deconv4s2(x.clone().requires_grad_(), (pk, sc, sh))
    head = backbone.DeconvHeadEval.from_reference(stand_in(), device="cpu")
    with pytest.raises(RuntimeError, match="inference-only"):
        head(torch.zeros(1, 64, 3, 4).requires_grad_())
    with pytest.raises(RuntimeError, match="x must be"):
        head(torch.zeros(64, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(1, 64, 3, 4))


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import backbone
    with FakeTensorMode():
        x = torch.empty(3, 5, 7, 64, dtype=torch.bfloat16)
        p = (torch.empty(16, 2, 16, 64, 8, dtype=torch.bfloat16), torch.empty(COUT), torch.empty(COUT))
        y = backbone.deconv4s2(x, p)
        assert tuple(y.shape) == (3, 10, 14, COUT) and y.dtype == torch.bfloat16
        y = backbone.deconv4s2(x, p, "nchw")
        assert tuple(y.shape) == (3, COUT, 10, 14) and y.dtype == torch.bfloat16
        y = backbone.deconv4s2(x, p, "nchw", torch.float32)
        assert tuple(y.shape) == (3, COUT, 10, 14) and y.dtype == torch.float32
        y = backbone.deconv4s2(x[:0], p, "nchw")
        assert tuple(y.shape) == (0, COUT, 10, 14)


def test_make_fx_records_the_op():
    """As tests/test_ops_tracing.py: the eager bypass must not hide the op from a tracer."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import backbone

    def two_layers(x, pk1, pk2, sc, sh):
        return backbone.deconv4s2(backbone.deconv4s2(x, (pk1, sc, sh)), (pk2, sc, sh), "nchw", torch.float32)

    gm = make_fx(two_layers, tracing_mode="fake")(torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16), _params(64)[0],
                                                  _params(COUT)[0], torch.ones(COUT), torch.zeros(COUT))
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.deconv4s2.default) == 2
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    assert tuple(out.meta["val"].shape) == (2, COUT, 12, 20) and out.meta["val"].dtype == torch.float32


# ---------------------------------------------------------------- from_reference
class StandIn(nn.Module):
    """The attributes of the reference's PoseResNet that the head reads."""

    def __init__(self, deconv_layers, final_layer):
        super().__init__()
        self.deconv_layers = deconv_layers
        self.final_layer = final_layer


def triple(cin, **k):
    cout = k.pop("cout", COUT)
    return [nn.ConvTranspose2d(cin, cout, k.pop("k", 4), stride=k.pop("stride", 2), padding=1, bias=False, **k),
            nn.BatchNorm2d(cout), nn.ReLU(True)]


def stand_in(layers=None, final=None, seed=5):
    layers = layers if layers is not None else triple(64) + triple(COUT) + triple(COUT)
    net = StandIn(layers if isinstance(layers, nn.Module) else nn.Sequential(*layers),
                  final if final is not None else nn.Conv2d(COUT, 17, 1))
    return randomise2d(net, seed)


def _swapped():
    t = triple(64)
    return [t[0], t[2], t[1]]


@pytest.mark.parametrize("layers, final, found", [
    (triple(64, k=3), None, r"kernel_size=\(3, 3\)"),
    (triple(64, stride=1), None, r"stride=\(1, 1\)"),
    (triple(64, k=3, output_padding=1), None, r"output_padding=\(1, 1\)"),
    (triple(64, cout=128), None, "out_channels=128"),
    (triple(64, dilation=2), None, r"dilation=\(2, 2\)"),
    (triple(64, groups=2), None, "groups=2"),
    (triple(48), None, "got 48"),
    (None, nn.Conv2d(COUT, 33, 1), "out_channels=33"),
    (None, nn.Conv2d(COUT, 17, 3, padding=1), r"kernel_size=\(3, 3\)"),
    (None, nn.Linear(COUT, 17), "Linear"),
    ([triple(64)[0], nn.ReLU(True), nn.ReLU(True)], None, r"\('ConvTranspose2d', 'ReLU', 'ReLU'\)"),
    (triple(64)[:1] + triple(64)[2:], None, "Sequential of 2 modules"),
    (_swapped(), None, r"\('ConvTranspose2d', 'ReLU', 'BatchNorm2d'\)"),
    (triple(64) + triple(64), None, "in_channels=64"),
    (nn.ModuleList(triple(64)), None, "ModuleList"),
], ids=["k3", "stride1", "output_padding1", "cout128", "dilation2", "groups2", "cin48", "J33", "final3x3", "final_linear",
        "no_bn", "bn_dropped", "wrong_order", "second_cin64", "not_sequential"])
def test_from_reference_refuses_and_names_what_it_found(layers, final, found):
    from mvn_rocm import backbone
    with pytest.raises(RuntimeError, match=found):
        backbone.DeconvHeadEval.from_reference(stand_in(layers, final), device="cpu")


def test_from_reference_refuses_a_bn_without_statistics():
    from mvn_rocm import backbone
    t = triple(64)
    t[1] = nn.BatchNorm2d(COUT, track_running_stats=False)
    with pytest.raises(RuntimeError, match="running statistics"):
        backbone.DeconvHeadEval.from_reference(stand_in(t), device="cpu")


def test_from_reference_reads_the_backbone():
    from mvn_rocm import backbone
    net = stand_in()
    head = backbone.DeconvHeadEval.from_reference(net, device="cpu")
    assert head.n_layers == 3 and head.joints == 17 and head.feature_dtype == torch.bfloat16 and head.heatmaps
    for i, cin in enumerate((64, COUT, COUT)):
        p = head.layer_params(i)
        want = backbone.fold_deconv_block(net.deconv_layers[3 * i], net.deconv_layers[3 * i + 1], device="cpu")
        assert tuple(p.packed.shape) == (16, cin // 32, 16, 64, 8)
        assert all(torch.equal(a, b) for a, b in zip(p, want))
    fl = net.final_layer
    assert tuple(head.final_weight.shape) == (32, COUT) and tuple(head.final_bias.shape) == (32,)
    assert torch.equal(head.final_weight[:17], fl.weight.detach().view(17, COUT)) and not head.final_weight[17:].any()
    assert torch.equal(head.final_bias[:17], fl.bias.detach()) and not head.final_bias[17:].any()
    # the default leaves no torch layer in the module
    assert not any(isinstance(m, (nn.ConvTranspose2d, nn.BatchNorm2d, nn.Conv2d)) for m in head.modules())
    h2 = backbone.DeconvHeadEval.from_reference(net, device="cpu", feature_dtype=torch.float32, heatmaps=False)
    assert h2.feature_dtype == torch.float32 and not h2.heatmaps
    assert h2.packed0.data_ptr() != head.packed0.data_ptr() and not h2.packed0.requires_grad      # copies
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        backbone.DeconvHeadEval.from_reference(net, device="cpu", feature_dtype=torch.float16)
    no_bias = stand_in(final=nn.Conv2d(COUT, 5, 1, bias=False))
    h3 = backbone.DeconvHeadEval.from_reference(no_bias, device="cpu")
    assert h3.joints == 5 and not h3.final_bias.any()


def test_backbone_eval_refuses_a_backbone_without_a_trunk():
    from mvn_rocm import backbone
    with pytest.raises(RuntimeError, match="has no conv1"):
        backbone.BackboneEval.from_reference(stand_in(), device="cpu")
