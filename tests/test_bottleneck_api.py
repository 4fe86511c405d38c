"""The ResNet trunk's kernels (csrc/bottleneck.hip, mvn_rocm/resnet.py) without a GPU: the packed weight layouts
against include/mvn_hip.h, the fold against float64, every MVN_ERR_ARG path of the two C entries (the checks
run before any HIP call), the refusals of ``fold_bottleneck`` and ``TrunkEval.from_reference`` on stand-in
modules, the autograd refusal, the fake kernels and the traced ops, and ``trunk="torch"`` as today's
``BackboneEval``."""
import pytest
import torch
from torch import nn

from bottleneck_kit import (Bottleneck, StandInTrunkBackbone, element1, element3, index_weight1, index_weight3, make_block,
                            stand_in_backbone, unpack_conv1x1, unpack_conv3x3)
from deconv_kit import randomise2d
from v2v_kit import IDENTITY, NONE, POINTWISE

OK, ARG = 0, -1
A = 4096                         # a 16-byte aligned stand-in address: the checks never dereference it


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- packing and folding
@pytest.mark.parametrize("cout, cin", ((64, 64), (256, 64), (64, 2048), (2048, 512)))
def test_conv1x1_pack_round_trip_by_the_documented_layout(cout, cin, lib):
    from mvn_rocm import resnet
    w = index_weight1(cout, cin)
    for shaped in (w, w.view(cout, cin, 1, 1)):
        packed = resnet.pack_conv1x1_weight(shaped.double())
        assert packed.dtype == torch.bfloat16 and packed.is_contiguous()
        assert packed.numel() * 2 == lib.mvn_conv1x1_packed_weight_bytes(cin, cout)
        assert torch.equal(unpack_conv1x1(packed, cout, cin), w.double())
    for pick in ((0, 0, 0, 0), (cin // 32 - 1, cout // 16 - 1, 63, 7), (1, 3, 17, 5), (cin // 32 - 1, 2, 40, 2)):
        (co, ci), v = element1(packed, *pick)
        assert v == float(w[co, ci])


@pytest.mark.parametrize("C", (64, 192, 512))
def test_conv3x3_pack_round_trip_by_the_documented_layout(C, lib):
    from mvn_rocm import resnet
    w = index_weight3(C)
    packed = resnet.pack_conv3x3_weight(w.double())
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous()
    assert packed.numel() * 2 == lib.mvn_conv3x3_packed_weight_bytes(C)
    assert torch.equal(unpack_conv3x3(packed, C), w.double())
    for pick in ((0, 0, 0, 0, 0), (8, C // 32 - 1, C // 16 - 1, 63, 7), (5, 1, 3, 17, 5), (2, C // 32 - 1, 2, 40, 2)):
        (co, ci, ky, kx), v = element3(packed, *pick)
        assert v == float(w[co, ci, ky, kx])


def test_packs_round_once_to_bf16():
    from mvn_rocm import resnet
    g = torch.Generator().manual_seed(2)
    w = torch.randn(128, 64, generator=g, dtype=torch.float64)
    assert torch.equal(unpack_conv1x1(resnet.pack_conv1x1_weight(w), 128, 64), w.float().bfloat16().double())
    w = torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64)
    assert torch.equal(unpack_conv3x3(resnet.pack_conv3x3_weight(w), 64), w.float().bfloat16().double())


def test_packed_weight_bytes(lib):
    assert lib.mvn_conv1x1_packed_weight_bytes(256, 64) == 8 * 4 * 64 * 8 * 2
    assert lib.mvn_conv3x3_packed_weight_bytes(128) == 9 * 4 * 8 * 64 * 8 * 2
    for c in (0, 32, 96, 2112, -64):
        assert lib.mvn_conv1x1_packed_weight_bytes(c, 64) == 0 and lib.mvn_conv1x1_packed_weight_bytes(64, c) == 0
    for c in (0, 32, 96, 576, 1024, -64):
        assert lib.mvn_conv3x3_packed_weight_bytes(c) == 0


def test_packs_refuse_other_shapes():
    from mvn_rocm import resnet
    for bad in (torch.zeros(64, 64, 3, 3), torch.zeros(64), torch.zeros(96, 64), torch.zeros(64, 32), torch.zeros(4096, 64)):
        with pytest.raises(RuntimeError, match="expected a|multiple of 64"):
            resnet.pack_conv1x1_weight(bad.double())
    for bad in (torch.zeros(64, 64, 1, 1), torch.zeros(64, 128, 3, 3), torch.zeros(96, 96, 3, 3), torch.zeros(1024, 1024, 3, 3)):
        with pytest.raises(RuntimeError, match="expected a|multiple of 64"):
            resnet.pack_conv3x3_weight(bad.double())


def _fold64(conv, bn):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64)
    return s.float(), ((b - bn.running_mean.double()) * s + bn.bias.detach().double()).float()


@pytest.mark.parametrize("inplanes, planes, stride", ((64, 64, 1), (256, 64, 1), (256, 128, 2)), ids=("down_s1", "identity", "down_s2"))
def test_fold_against_float64(inplanes, planes, stride):
    from mvn_rocm import resnet
    block = make_block(inplanes, planes, stride, seed=3)
    if stride == 2:                                               # a conv bias is not required, and is folded when there
        block.conv2 = nn.Conv2d(planes, planes, 3, stride=2, padding=1, bias=True)
        randomise2d(block, seed=4)
    p = resnet.fold_bottleneck(block, device="cpu")
    assert p.stride == stride and (p.downsample is None) == (block.downsample is None)
    pairs = [(p.conv1, block.conv1, block.bn1, unpack_conv1x1), (p.conv2, block.conv2, block.bn2, None),
             (p.conv3, block.conv3, block.bn3, unpack_conv1x1)]
    if block.downsample is not None:
        pairs.append((p.downsample, block.downsample[0], block.downsample[1], unpack_conv1x1))
    for got, conv, bn, unpack in pairs:
        s, t = _fold64(conv, bn)
        assert torch.equal(got.scale, s) and torch.equal(got.shift, t) and got.scale.dtype == torch.float32
        want = conv.weight.detach().float().bfloat16().double()
        if unpack is None:
            assert torch.equal(unpack_conv3x3(got.packed, planes), want)
        else:
            assert torch.equal(unpack(got.packed, conv.out_channels, conv.in_channels), want.view(conv.out_channels, -1))


# ---------------------------------------------------------------- C argument validation
def _c1(lib, **k):
    mode = k.get("mode", NONE)
    skip = k.get("skip", A if mode != NONE else None)
    pw = A if mode == POINTWISE else None
    return lib.mvn_conv1x1(k.get("x", A), k.get("w", A), k.get("scale", A), k.get("shift", A), mode, skip, k.get("ws", pw),
                           k.get("scs", pw), k.get("shs", pw), k.get("cs", 256), k.get("Hs", 5), k.get("Ws", 9),
                           k.get("stride", 2), k.get("out", A), k.get("n", 2), k.get("H", 3), k.get("W", 5), k.get("cin", 64),
                           k.get("cout", 256), None)


def test_conv1x1_argument_validation(lib):
    """Every refusal is MVN_ERR_ARG and comes before any HIP call (there is no device here)."""
    for mode in (NONE, IDENTITY, POINTWISE):
        assert _c1(lib, mode=mode, n=0) == OK
        for name in ("x", "w", "scale", "shift", "out"):
            assert _c1(lib, mode=mode, **{name: None}) == ARG
            assert _c1(lib, mode=mode, **{name: A + 2}) == ARG
    for mode in (-1, 3, 7):
        assert _c1(lib, mode=mode, n=0) == ARG
    # skip arguments that contradict the mode
    assert _c1(lib, mode=NONE, skip=A, n=0) == ARG and _c1(lib, mode=NONE, ws=A, n=0) == ARG
    assert _c1(lib, mode=NONE, scs=A, n=0) == ARG and _c1(lib, mode=NONE, shs=A, n=0) == ARG
    assert _c1(lib, mode=IDENTITY, skip=None, n=0) == ARG and _c1(lib, mode=IDENTITY, ws=A, n=0) == ARG
    for name in ("skip", "ws", "scs", "shs"):
        assert _c1(lib, mode=POINTWISE, n=0, **{name: None}) == ARG
        assert _c1(lib, mode=POINTWISE, n=0, **{name: A + 2}) == ARG
    assert _c1(lib, mode=IDENTITY, skip=A + 2, n=0) == ARG
    for c in (0, 32, 96, 2112, -64, 4096):
        assert _c1(lib, cin=c, n=0) == ARG and _c1(lib, cout=c, n=0) == ARG and _c1(lib, mode=POINTWISE, cs=c, n=0) == ARG
    assert _c1(lib, cin=2048, cout=2048, n=0) == OK
    assert _c1(lib, H=0) == ARG and _c1(lib, W=0) == ARG and _c1(lib, H=-1) == ARG and _c1(lib, n=-1) == ARG
    # the pointwise skip's geometry: H = (Hs - 1) / s + 1, W = (Ws - 1) / s + 1, s in {1, 2}
    for s in (0, 3, -1):
        assert _c1(lib, mode=POINTWISE, stride=s, n=0) == ARG
    assert _c1(lib, mode=POINTWISE, Hs=5, Ws=9, n=0) == OK and _c1(lib, mode=POINTWISE, Hs=6, Ws=10, n=0) == OK
    assert _c1(lib, mode=POINTWISE, Hs=7, n=0) == ARG and _c1(lib, mode=POINTWISE, Ws=8, n=0) == ARG
    assert _c1(lib, mode=POINTWISE, Hs=0, n=0) == ARG and _c1(lib, mode=POINTWISE, Ws=0, n=0) == ARG
    assert _c1(lib, mode=POINTWISE, stride=1, Hs=3, Ws=5, n=0) == OK and _c1(lib, mode=POINTWISE, stride=1, n=0) == ARG
    # every tensor below 2^31 bytes: x, out and the pointwise skip
    assert _c1(lib, n=1, H=4096, W=4096, cin=64, cout=64) == ARG                     # 2^31 bytes of x
    assert _c1(lib, n=1, H=2048, W=2048, cin=64, cout=2048) == ARG                   # 2^34 bytes of out
    assert _c1(lib, n=1, H=2048, W=2048, cin=2048, cout=64) == ARG
    assert _c1(lib, n=2 ** 40, H=1, W=1) == ARG and _c1(lib, n=1, H=2 ** 30, W=2 ** 30) == ARG
    assert _c1(lib, n=2 ** 20, H=64, W=64, cin=64, cout=64) == ARG
    assert _c1(lib, mode=POINTWISE, n=2 ** 12, H=16, W=16, Hs=32, Ws=32, cin=64, cout=64, cs=2048) == ARG   # the skip alone
    # an empty batch is nothing to do, but its errors come first
    assert _c1(lib, n=0, x=None) == ARG and _c1(lib, n=0, cin=96) == ARG and _c1(lib, n=0, H=0) == ARG


def _c3(lib, **k):
    return lib.mvn_conv3x3(k.get("x", A), k.get("w", A), k.get("scale", A), k.get("shift", A), k.get("out", A), k.get("n", 2),
                           k.get("H", 5), k.get("W", 7), k.get("C", 64), k.get("stride", 2), None)


def test_conv3x3_argument_validation(lib):
    assert _c3(lib, n=0) == OK and _c3(lib, n=0, stride=1, C=512) == OK
    for name in ("x", "w", "scale", "shift", "out"):
        assert _c3(lib, **{name: None}) == ARG and _c3(lib, **{name: A + 2}) == ARG
    for c in (0, 32, 96, 576, 1024, -64):
        assert _c3(lib, C=c, n=0) == ARG
    for s in (0, 3, -1):
        assert _c3(lib, stride=s, n=0) == ARG
    assert _c3(lib, H=0) == ARG and _c3(lib, W=0) == ARG and _c3(lib, W=-3) == ARG and _c3(lib, n=-1) == ARG
    assert _c3(lib, n=1, H=4096, W=4096, C=64) == ARG                                # 2^31 bytes of x
    assert _c3(lib, n=0, H=4096, W=2048, C=64, stride=1) == OK                       # 2^30 bytes: allowed
    assert _c3(lib, n=1, H=2048, W=2048, C=512, stride=2) == ARG                     # 2^32 bytes of x
    assert _c3(lib, n=2 ** 40, H=1, W=1) == ARG and _c3(lib, n=1, H=2 ** 30, W=2 ** 30) == ARG
    assert _c3(lib, n=0, x=None) == ARG and _c3(lib, n=0, C=96) == ARG and _c3(lib, n=0, H=0) == ARG


# ---------------------------------------------------------------- the Python wrappers
def _p1(cin=64, cout=256):
    return (torch.zeros(cin // 32, cout // 16, 64, 8, dtype=torch.bfloat16), torch.ones(cout), torch.zeros(cout))


def _p3(C=64):
    return (torch.zeros(9, C // 32, C // 16, 64, 8, dtype=torch.bfloat16), torch.ones(C), torch.zeros(C))


def test_wrapper_refusals():
    from mvn_rocm import resnet
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet.conv1x1(x, *_p1())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet.conv3x3(x, *_p3())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet.conv1x1(x, *_p1(), skip=torch.zeros(2, 3, 5, 256, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet.conv1x1(x, *_p1(), skip=torch.zeros(2, 5, 9, 128, dtype=torch.bfloat16), skip_params=_p1(128), skip_stride=2)
    for fn, p in ((resnet.conv1x1, _p1()), (resnet.conv3x3, _p3())):
        with pytest.raises(TypeError, match="x_cl must be bfloat16"):
            fn(x.float(), *p)
        with pytest.raises(RuntimeError, match="x_cl must be"):
            fn(x[0], *p)
        with pytest.raises(RuntimeError, match="multiple of 64"):
            fn(torch.zeros(1, 2, 2, 96, dtype=torch.bfloat16), *p)
        with pytest.raises(RuntimeError, match="H, W >= 1"):
            fn(torch.zeros(1, 0, 5, 64, dtype=torch.bfloat16), *p)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        resnet.conv3x3(torch.zeros(1, 2, 2, 1024, dtype=torch.bfloat16), *_p3())
    with pytest.raises(RuntimeError, match="packed bfloat16 weights"):
        resnet.conv1x1(x, *_p1(128))
    with pytest.raises(RuntimeError, match="packed bfloat16 weights"):
        resnet.conv3x3(x, *_p3(128))
    with pytest.raises(ValueError, match="stride must be 1 or 2"):
        resnet.conv3x3(x, *_p3(), stride=3)
    with pytest.raises(RuntimeError, match="identity skip"):
        resnet.conv1x1(x, *_p1(), skip=torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="skip_params without skip"):
        resnet.conv1x1(x, *_p1(), skip_params=_p1())
    sk = torch.zeros(2, 5, 9, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="skip_stride must be 1 or 2"):
        resnet.conv1x1(x, *_p1(), skip=sk, skip_params=_p1(128), skip_stride=3)
    with pytest.raises(RuntimeError, match="must map onto"):
        resnet.conv1x1(x, *_p1(), skip=sk, skip_params=_p1(128), skip_stride=1)
    with pytest.raises(RuntimeError, match="skip_params must be"):
        resnet.conv1x1(x, *_p1(), skip=sk, skip_params=_p1(64), skip_stride=2)


def test_autograd_is_refused():
    from mvn_rocm import resnet
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    pk, sc, sh = _p1()
    with pytest.raises(RuntimeError, match="inference-only.*Bottleneck"):
        resnet.conv1x1(x.clone().requires_grad_(), pk, sc, sh)
    with pytest.raises(RuntimeError, match="inference-only"):
        resnet.conv1x1(x, pk, sc.clone().requires_grad_(), sh)
    with pytest.raises(RuntimeError, match="inference-only"):
        resnet.conv1x1(x, pk, sc, sh, skip=torch.zeros(2, 3, 5, 256, dtype=torch.bfloat16).requires_grad_())
    with pytest.raises(RuntimeError, match="inference-only.*Bottleneck"):
        resnet.conv3x3(x.clone().requires_grad_(), *_p3())
    with torch.no_grad():                                         # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            resnet.conv3x3(x.clone().requires_grad_(), *_p3())
    block = resnet.BottleneckCL.from_reference(make_block(64, 64), device="cpu")
    with pytest.raises(RuntimeError, match="inference-only"):
        block(x.clone().requires_grad_())
    trunk = resnet.TrunkEval.from_reference(stand_in_backbone(), device="cpu")
    with pytest.raises(RuntimeError, match="inference-only"):
        trunk(torch.zeros(1, 3, 40, 56).requires_grad_())
    with pytest.raises(RuntimeError, match="x must be"):
        trunk(torch.zeros(3, 40, 56))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            trunk(torch.zeros(1, 3, 40, 56))


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import resnet
    with FakeTensorMode():
        x = torch.empty(3, 5, 9, 64, dtype=torch.bfloat16)
        p1 = (torch.empty(2, 16, 64, 8, dtype=torch.bfloat16), torch.empty(256), torch.empty(256))
        p3 = (torch.empty(9, 2, 4, 64, 8, dtype=torch.bfloat16), torch.empty(64), torch.empty(64))
        y = resnet.conv1x1(x, *p1)
        assert tuple(y.shape) == (3, 5, 9, 256) and y.dtype == torch.bfloat16
        assert tuple(resnet.conv1x1(x, *p1, skip=y).shape) == (3, 5, 9, 256)
        z = resnet.conv3x3(x, *p3, stride=2)
        assert tuple(z.shape) == (3, 3, 5, 64) and z.dtype == torch.bfloat16
        assert tuple(resnet.conv3x3(x, *p3).shape) == (3, 5, 9, 64)
        assert tuple(resnet.conv1x1(z, *p1, skip=x, skip_params=p1, skip_stride=2).shape) == (3, 3, 5, 256)
        assert tuple(resnet.conv3x3(x[:0], *p3, stride=2).shape) == (0, 3, 5, 64)


def test_make_fx_records_the_ops():
    """As tests/test_ops_tracing.py: the eager bypass must not hide the ops from a tracer."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import resnet
    params = resnet.fold_bottleneck(make_block(64, 64, 2), device="cpu")

    def block(x, c1, c2, c3, down):
        return resnet.bottleneck(x, resnet.BottleneckParams(c1, c2, c3, down, params.stride))

    gm = make_fx(block, tracing_mode="fake")(torch.zeros(2, 5, 9, 64, dtype=torch.bfloat16), tuple(params.conv1),
                                             tuple(params.conv2), tuple(params.conv3), tuple(params.downsample))
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.conv1x1.default) == 2 and targets.count(torch.ops.mvn_rocm.conv3x3.default) == 1
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    out = out[0] if isinstance(out, (list, tuple)) else out
    assert tuple(out.meta["val"].shape) == (2, 3, 5, 256) and out.meta["val"].dtype == torch.bfloat16


# ---------------------------------------------------------------- fold_bottleneck's refusals
class BasicBlock(nn.Module):
    """The shape of the reference's BasicBlock: two 3x3 convolutions, no conv3."""

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
        self.conv2, self.bn2 = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
        self.downsample, self.stride = None, 1


def _caffe():
    b = make_block(256, 64, 2)
    b.conv1 = nn.Conv2d(256, 64, 1, stride=2, bias=False)        # the stride on conv1
    b.conv2 = nn.Conv2d(64, 64, 3, stride=1, padding=1, bias=False)
    return b


def _widens():
    b = make_block(256, 64)
    b.conv2, b.bn2 = nn.Conv2d(64, 128, 3, padding=1, bias=False), nn.BatchNorm2d(128)
    return b


def _with(attr, module, inplanes=256, planes=64, stride=1):
    b = make_block(inplanes, planes, stride)
    setattr(b, attr, module)
    return b


def _down(conv, bn=None, inplanes=64, planes=64, stride=1):
    b = make_block(inplanes, planes, stride)
    b.downsample = nn.Sequential(conv, bn if bn is not None else nn.BatchNorm2d(conv.out_channels))
    return b


@pytest.mark.parametrize("block, found", [
    (BasicBlock(), "BasicBlock has no conv3, bn3"),
    (_caffe(), r"conv1: .*stride=\(2, 2\)"),
    (_with("conv2", nn.Conv2d(64, 64, 3, padding=2, dilation=2, bias=False)), r"conv2: .*dilation=\(2, 2\)"),
    (_with("conv2", nn.Conv2d(64, 64, 3, padding=1, groups=32, bias=False)), "conv2: .*groups=32"),
    (_with("conv2", nn.Conv2d(64, 64, 5, padding=1, bias=False)), r"conv2: .*kernel_size=\(5, 5\)"),
    (_with("conv2", nn.Conv2d(64, 64, 3, padding=0, bias=False)), r"conv2: .*padding=\(0, 0\)"),
    (_with("conv2", nn.Conv2d(64, 64, 3, stride=4, padding=1, bias=False)), r"conv2: .*stride=\(4, 4\)"),
    (_with("conv3", nn.Conv2d(64, 256, 3, padding=1, bias=False)), r"conv3: .*kernel_size=\(3, 3\)"),
    (_with("conv1", nn.Linear(256, 64)), "conv1: expected a Conv2d, got Linear"),
    (_with("bn2", nn.GroupNorm(8, 64)), "conv2: expected a BatchNorm2d behind the Conv2d, got GroupNorm"),
    (_with("bn3", nn.BatchNorm2d(256, track_running_stats=False)), "conv3: .*running statistics"),
    (_with("bn1", nn.BatchNorm2d(128)), r"conv1: .*BatchNorm2d\(128"),
    (_widens(), "conv2 64 -> 128"),
    (_with("conv1", nn.Conv2d(96, 64, 1, bias=False), 96), "conv1.in_channels must be a multiple of 64.*got 96"),
    (_with("stride", 2), "stride=2 with conv2.stride"),
    (_with("downsample", None, 64, 64), "expected a downsample for stride 1 and 64 -> 256 channels, got None"),
    (_with("downsample", nn.Conv2d(64, 256, 1), 64, 64), "got Conv2d"),
    (_with("downsample", nn.Sequential(nn.Conv2d(64, 256, 1)), 64, 64), "Sequential of 1 modules"),
    (_down(nn.Conv2d(64, 256, 3, padding=1, bias=False)), r"downsample: .*kernel_size=\(3, 3\)"),
    (_down(nn.Conv2d(64, 256, 1, stride=2, bias=False)), r"stride=1\), got Conv2d\(64, 256, 1, stride=2\)"),
    (_down(nn.Conv2d(64, 128, 1, bias=False)), r"got Conv2d\(64, 128, 1, stride=1\)"),
    (_down(nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256, track_running_stats=False)), "downsample: .*running statistics"),
], ids=["basic_block", "caffe", "dilation", "groups", "k5", "padding0", "stride4", "conv3_3x3", "linear", "group_norm",
        "bn_no_stats", "bn_width", "conv2_widens", "cin96", "stride_attr", "no_downsample", "downsample_conv", "downsample_short",
        "downsample_3x3", "downsample_stride", "downsample_width", "downsample_bn_no_stats"])
def test_fold_bottleneck_refuses_and_names_what_it_found(block, found):
    from mvn_rocm import resnet
    with pytest.raises(RuntimeError, match=found):
        resnet.fold_bottleneck(block, device="cpu")


# ---------------------------------------------------------------- TrunkEval.from_reference
def _backbone(**changes):
    net = StandInTrunkBackbone()
    for name, value in changes.items():
        if value is None:
            delattr(net, name)
        else:
            setattr(net, name, value)
    return randomise2d(net, seed=6)


@pytest.mark.parametrize("net, found", [
    (_backbone(layer3=None), "has no layer3"),
    (_backbone(maxpool=None, conv1=None), "has no conv1, maxpool"),
    (_backbone(layer2=nn.Identity()), "expected layer2 to be a Sequential of Bottleneck blocks, got Identity"),
    (_backbone(layer2=nn.Sequential()), "expected layer2 to be a Sequential"),
    (_backbone(layer2=nn.Sequential(BasicBlock())), r"layer2\[0\]: .*BasicBlock has no conv3"),
    (_backbone(layer4=nn.Sequential(_caffe())), r"layer4\[0\]: .*conv1: .*stride=\(2, 2\)"),
    (_backbone(layer2=nn.Sequential(make_block(128, 64, 2))), r"layer2\[0\]: expected 256 input channels.*in_channels=128"),
    (_backbone(conv1=nn.Conv2d(3, 128, 7, stride=2, padding=3, bias=False)), r"layer1\[0\]: expected 128 input channels"),
], ids=["no_layer3", "no_stem", "identity_layer", "empty_layer", "basic_block", "caffe", "channel_chain", "stem_width"])
def test_trunk_eval_refuses_and_names_what_it_found(net, found):
    from mvn_rocm import resnet
    with pytest.raises(RuntimeError, match=found):
        resnet.TrunkEval.from_reference(net, device="cpu")


def test_trunk_eval_reads_the_backbone():
    from mvn_rocm import resnet
    net = stand_in_backbone()
    trunk = resnet.TrunkEval.from_reference(net, device="cpu")
    assert [type(m) for m in trunk.stem] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d]
    assert all(a is b for a, b in zip(trunk.stem, (net.conv1, net.bn1, net.relu, net.maxpool)))
    blocks = net.blocks()
    assert len(trunk.blocks) == len(blocks) == 6
    assert [b.stride for b in trunk.blocks] == [1, 1, 2, 2, 1, 2]
    assert [b.has_downsample for b in trunk.blocks] == [True, False, True, True, False, True]
    for got, block in zip(trunk.blocks, blocks):
        want = resnet.fold_bottleneck(block, device="cpu")
        for name in ("conv1", "conv2", "conv3", "downsample"):
            g, w = getattr(got.params, name), getattr(want, name)
            assert (g is None) == (w is None)
            if g is not None:
                assert all(torch.equal(a, b) for a, b in zip(g, w))
                assert g.packed.data_ptr() != w.packed.data_ptr() and not g.packed.requires_grad      # copies
    # no torch layer is left in the stages
    assert not any(isinstance(m, (nn.Conv2d, nn.BatchNorm2d)) for b in trunk.blocks for m in b.modules())


# ---------------------------------------------------------------- BackboneEval(trunk=)
def test_trunk_torch_builds_todays_backbone_eval():
    from mvn_rocm import backbone, resnet
    net = stand_in_backbone()
    default = backbone.BackboneEval.from_reference(net, device="cpu")
    named = backbone.BackboneEval.from_reference(net, device="cpu", trunk="torch")
    for be in (default, named):
        assert type(be.trunk) is nn.Sequential and len(be.trunk) == 8 and not be.cast_for_confidences
        names = ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4")
        assert all(m is getattr(net, n) for m, n in zip(be.trunk, names))                         # the backbone's own modules
        assert be.alg_confidences is net.alg_confidences and be.vol_confidences is net.vol_confidences
    for a, b in zip(default.head.buffers(), named.head.buffers()):
        assert torch.equal(a, b)
    kernels = backbone.BackboneEval.from_reference(net, device="cpu", trunk="kernels")
    assert isinstance(kernels.trunk, resnet.TrunkEval) and kernels.cast_for_confidences
    assert kernels.vol_confidences is net.vol_confidences
    with pytest.raises(ValueError, match="trunk must be 'torch' or 'kernels'"):
        backbone.BackboneEval.from_reference(net, device="cpu", trunk="hip")
    # the f32 trunk on the CPU computes what the backbone's own modules compute: the module adds no arithmetic
    x = torch.randn(1, 3, 40, 56, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        assert torch.equal(default.trunk(x), net.trunk(x))


def test_volumetric_model_eval_passes_the_trunk_through():
    from bottleneck_kit import stand_in_trunk_model
    from mvn_rocm import model, resnet
    net = stand_in_trunk_model()
    assert type(model.VolumetricModelEval.from_reference(net, device="cpu").backbone.trunk) is nn.Sequential
    me = model.VolumetricModelEval.from_reference(net, device="cpu", trunk="kernels")
    assert isinstance(me.backbone.trunk, resnet.TrunkEval)
