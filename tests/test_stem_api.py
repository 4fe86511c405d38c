"""The ResNet stem's kernel (csrc/stem.hip, mvn_rocm/resnet.py) without a GPU: the packed weight
layout against include/mvn_hip.h, the fold against float64, every MVN_ERR_ARG path of the C entry (the checks
run before any HIP call), the refusals of ``fold_stem``, of the wrapper and of the three ``from_reference``
signatures, the autograd refusal, the fake kernel and the traced op, and ``stem="torch"`` as the parent's
modules."""
import pytest
import torch
from torch import nn

from bottleneck_kit import StandInTrunkBackbone, stand_in_backbone, stand_in_trunk_model
from deconv_kit import randomise2d
from stem_kit import CIN, COUT, KS, element, index_weight, slot_of, unpack_stem

OK, ARG = 0, -1
A = 4096                         # a 16-byte aligned stand-in address: the checks never dereference it
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- packing and folding
def test_pack_round_trip_by_the_documented_layout(lib):
    from mvn_rocm import resnet
    w = index_weight()
    packed = resnet.pack_stem_weight(w.double())
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous() and tuple(packed.shape) == (6, 4, 64, 8)
    assert packed.numel() * 2 == lib.mvn_stem_packed_weight_bytes() == 24576
    got, pad_nonzero = unpack_stem(packed)
    assert torch.equal(got, w.double())
    assert not bool(pad_nonzero.any())                            # 24 ky + 21 .. + 23 and 168 .. 191 are zeros
    assert int((packed != 0).sum()) == COUT * CIN * KS * KS
    # a few elements by the literal formula: A[co][24 ky + 3 kx + ci] = w[co][ci][ky][kx]
    for pick, (ci, ky, kx) in (((0, 0, 0, 0), (0, 0, 0)), ((0, 3, 17, 5), (1, 0, 4)), ((1, 1, 40, 2), (2, 2, 0)),
                               ((4, 2, 63, 7), (0, 6, 5)), ((5, 3, 15, 4), (2, 6, 6))):
        (co, k), v = element(packed, *pick)
        assert k == slot_of(ci, ky, kx) and v == float(w[co, ci, ky, kx])
    for pick in ((0, 0, 32, 5), (0, 1, 47, 7), (5, 0, 16, 0), (5, 3, 63, 7), (2, 2, 49, 6)):   # pad slots: k = 21, 23, 168, 191, 94
        (co, k), v = element(packed, *pick)
        assert (k % 24 >= 21 or k >= 168) and v == 0.0


def test_pack_rounds_once_to_bf16_and_refuses_other_shapes():
    from mvn_rocm import resnet
    w = torch.randn(COUT, CIN, KS, KS, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    assert torch.equal(unpack_stem(resnet.pack_stem_weight(w))[0], w.float().bfloat16().double())
    for bad in (torch.zeros(64, 4, 7, 7), torch.zeros(64, 3, 3, 3), torch.zeros(32, 3, 7, 7), torch.zeros(64, 147),
                torch.zeros(64, 3, 7, 7, 1)):
        with pytest.raises(RuntimeError, match=r"expected a \(64, 3, 7, 7\) Conv2d weight, got \(" + str(bad.shape[0])):
            resnet.pack_stem_weight(bad.double())


def _stem_modules(bias=False, seed=3):
    net = nn.Sequential()
    net.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=bias)
    net.bn1 = nn.BatchNorm2d(64)
    net.relu = nn.ReLU(inplace=True)
    net.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    return randomise2d(net, seed=seed)


@pytest.mark.parametrize("bias", (False, True), ids=("no_bias", "bias"))
def test_fold_against_float64(bias):
    from mvn_rocm import resnet
    net = _stem_modules(bias)
    p = resnet.fold_stem(net.conv1, net.bn1, net.relu, net.maxpool, device="cpu")
    bn = net.bn1
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    b = net.conv1.bias.detach().double() if bias else torch.zeros(64, dtype=torch.float64)
    t = (b - bn.running_mean.double()) * s + bn.bias.detach().double()
    assert bias == bool((b != 0).any())
    assert torch.equal(p.scale, s.float()) and torch.equal(p.shift, t.float())
    assert p.scale.dtype == p.shift.dtype == torch.float32 and p.packed.dtype == torch.bfloat16
    assert torch.equal(unpack_stem(p.packed)[0], net.conv1.weight.detach().float().bfloat16().double())
    se = resnet.StemEval.from_reference(net, device="cpu")
    assert all(torch.equal(a, b) for a, b in zip(se.params, p)) and not se.packed.requires_grad
    assert sorted(n for n, _ in se.named_buffers()) == ["packed", "scale", "shift"] and not list(se.parameters())


def _with(**changes):
    net = _stem_modules()
    for name, module in changes.items():
        setattr(net, name, module)
    return net


@pytest.mark.parametrize("net, found", [
    (_with(conv1=nn.Conv2d(4, 64, 7, stride=2, padding=3, bias=False)), r"got Conv2d\(4, 64, 7\)"),
    (_with(conv1=nn.Conv2d(3, 128, 7, stride=2, padding=3, bias=False), bn1=nn.BatchNorm2d(128)), r"got Conv2d\(3, 128, 7\)"),
    (_with(conv1=nn.Conv2d(3, 64, 3, stride=2, padding=3, bias=False)), r"conv1: .*kernel_size=\(3, 3\)"),
    (_with(conv1=nn.Conv2d(3, 64, 7, stride=1, padding=3, bias=False)), r"conv1: .*stride=\(1, 1\)"),
    (_with(conv1=nn.Conv2d(3, 64, 7, stride=2, padding=2, bias=False)), r"conv1: .*padding=\(2, 2\)"),
    (_with(conv1=nn.Conv2d(3, 64, 7, stride=2, padding=3, dilation=2, bias=False)), r"conv1: .*dilation=\(2, 2\)"),
    (_with(conv1=nn.Conv2d(3, 63, 7, stride=2, padding=3, groups=3, bias=False), bn1=nn.BatchNorm2d(63)), "conv1: .*groups=3"),
    (_with(conv1=nn.Linear(3, 64)), "conv1: expected a Conv2d, got Linear"),
    (_with(bn1=nn.GroupNorm(8, 64)), "expected a BatchNorm2d behind the Conv2d, got GroupNorm"),
    (_with(bn1=nn.BatchNorm2d(64, track_running_stats=False)), "running statistics.*track_running_stats=False"),
    (_with(bn1=nn.BatchNorm2d(32)), r"BatchNorm2d\(32"),
    (_with(relu=nn.LeakyReLU()), "expected an nn.ReLU behind bn1, got LeakyReLU"),
    (_with(maxpool=nn.AvgPool2d(3, 2, 1)), "expected a MaxPool2d behind the ReLU, got AvgPool2d"),
    (_with(maxpool=nn.MaxPool2d(3, 2, 1, ceil_mode=True)), "got ceil_mode=True"),
    (_with(maxpool=nn.MaxPool2d(2, 2, 1)), r"got kernel_size=\(2, 2\)"),
    (_with(maxpool=nn.MaxPool2d(3, 1, 1)), r"got stride=\(1, 1\)"),
    (_with(maxpool=nn.MaxPool2d(3, 2, 0)), r"got padding=\(0, 0\)"),
    (_with(maxpool=nn.MaxPool2d(3, 2, 1, dilation=2)), r"got dilation=\(2, 2\)"),
    (_with(maxpool=nn.MaxPool2d(3, 2, 1, return_indices=True)), "got return_indices=True"),
], ids=["cin4", "cout128", "k3", "stride1", "padding2", "dilation", "groups", "linear", "group_norm", "bn_no_stats", "bn_width",
        "leaky", "avg_pool", "ceil_mode", "pool_k2", "pool_s1", "pool_p0", "pool_dilation", "pool_indices"])
def test_fold_stem_refuses_and_names_what_it_found(net, found):
    from mvn_rocm import resnet
    with pytest.raises(RuntimeError, match="fold_stem: .*" + found):
        resnet.fold_stem(net.conv1, net.bn1, net.relu, net.maxpool, device="cpu")
    with pytest.raises(RuntimeError, match=found):
        resnet.StemEval.from_reference(net, device="cpu")


# ---------------------------------------------------------------- C argument validation
def _c(lib, **k):
    return lib.mvn_stem(k.get("images", A), k.get("dtype", F32), k.get("w", A), k.get("scale", A), k.get("shift", A),
                        k.get("out", A), k.get("n", 2), k.get("H", 40), k.get("W", 56), None)


def test_stem_argument_validation(lib):
    """Every refusal is MVN_ERR_ARG and comes before any HIP call (there is no device here)."""
    for dtype in (F32, BF16):
        assert _c(lib, dtype=dtype, n=0) == OK
    for name in ("images", "w", "scale", "shift", "out"):
        assert _c(lib, **{name: None}) == ARG and _c(lib, n=0, **{name: None}) == ARG
    for name in ("w", "scale", "shift", "out"):                   # 16-byte alignment
        for off in (2, 4, 8):
            assert _c(lib, n=0, **{name: A + off}) == ARG
    # the images need the alignment of their element only: a row of odd W is not aligned anyway
    assert _c(lib, n=0, images=A + 4) == OK and _c(lib, n=0, images=A + 2) == ARG
    assert _c(lib, n=0, dtype=BF16, images=A + 2) == OK and _c(lib, n=0, dtype=BF16, images=A + 1) == ARG
    for dtype in (-1, 2, 7):
        assert _c(lib, dtype=dtype, n=0) == ARG
    assert _c(lib, H=0) == ARG and _c(lib, W=0) == ARG and _c(lib, H=-1) == ARG and _c(lib, W=-3) == ARG and _c(lib, n=-1) == ARG
    assert _c(lib, n=0, H=1, W=1) == OK
    # every tensor below 2^31 bytes: the images (f32 twice the bytes of bf16) and the output
    assert _c(lib, n=1, H=2 ** 14, W=2 ** 14) == ARG                               # 3 * 2^28 * 4 bytes
    assert _c(lib, n=1, dtype=BF16, H=2 ** 14, W=2 ** 14) == ARG and _c(lib, n=2 ** 40, H=1, W=1) == ARG
    assert _c(lib, n=1, H=2 ** 30, W=2 ** 30) == ARG and _c(lib, n=2 ** 20, H=32, W=32) == ARG
    assert _c(lib, n=2 ** 25, dtype=BF16, H=1, W=1) == ARG                         # the output alone: 2^25 * 64 * 2 bytes
    assert _c(lib, n=2 ** 24, dtype=BF16, H=1, W=1, images=None) == ARG
    # an empty batch is nothing to do, but its errors come first
    assert _c(lib, n=0, images=None) == ARG and _c(lib, n=0, H=0) == ARG and _c(lib, n=0, dtype=5) == ARG


# ---------------------------------------------------------------- the Python wrapper
def _p():
    return (torch.zeros(6, 4, 64, 8, dtype=torch.bfloat16), torch.ones(64), torch.zeros(64))


def test_wrapper_refusals():
    from mvn_rocm import resnet
    x = torch.zeros(2, 3, 9, 11)
    for images in (x, x.bfloat16(), x.to(memory_format=torch.channels_last)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            resnet.stem(images, *_p())
    for dtype in (torch.float16, torch.float64, torch.uint8):
        with pytest.raises(TypeError, match=f"images must be float32 or bfloat16, got {dtype}"):
            resnet.stem(x.to(dtype), *_p())
    for bad in (x[0], torch.zeros(2, 4, 9, 11), torch.zeros(2, 1, 9, 11), torch.zeros(2, 3, 9, 11, 1)):
        with pytest.raises(RuntimeError, match=r"images must be \(M, 3, H, W\), got \(" + str(bad.shape[0])):
            resnet.stem(bad, *_p())
    for bad in (torch.zeros(1, 3, 0, 5), torch.zeros(1, 3, 5, 0)):
        with pytest.raises(RuntimeError, match="H, W >= 1"):
            resnet.stem(bad, *_p())
    with pytest.raises(RuntimeError, match="below 2\\^31 bytes"):
        resnet.stem(torch.empty(1, 3, 2 ** 14, 2 ** 14, device="meta"), *_p())
    pk, sc, sh = _p()
    for bad in ((pk.float(), sc, sh), (pk[:5], sc, sh), (pk, sc[:32], sh), (pk, sc, sh.double()), (pk, sc.bfloat16(), sh)):
        with pytest.raises(RuntimeError, match="packed bfloat16 weights"):
            resnet.stem(x, *bad)


def test_autograd_is_refused():
    from mvn_rocm import resnet
    x = torch.zeros(2, 3, 9, 11)
    pk, sc, sh = _p()
    with pytest.raises(RuntimeError, match="inference-only.*conv1, bn1, relu and maxpool"):
        resnet.stem(x.clone().requires_grad_(), pk, sc, sh)
    with pytest.raises(RuntimeError, match="inference-only"):
        resnet.stem(x, pk, sc.clone().requires_grad_(), sh)
    with torch.no_grad():                                         # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            resnet.stem(x.clone().requires_grad_(), pk, sc, sh)
    se = resnet.StemEval.from_reference(stand_in_backbone(), device="cpu")
    with pytest.raises(RuntimeError, match="inference-only"):
        se(x.clone().requires_grad_())
    trunk = resnet.TrunkEval.from_reference(stand_in_backbone(), device="cpu", stem="kernels")
    with pytest.raises(RuntimeError, match="inference-only"):
        trunk(torch.zeros(1, 3, 40, 56).requires_grad_())
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            trunk(torch.zeros(1, 3, 40, 56))


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import resnet
    with FakeTensorMode():
        p = (torch.empty(6, 4, 64, 8, dtype=torch.bfloat16), torch.empty(64), torch.empty(64))
        for (M, H, W), want in (((3, 40, 56), (3, 10, 14, 64)), ((1, 1, 1), (1, 1, 1, 64)), ((2, 37, 51), (2, 10, 13, 64)),
                                ((2, 35, 34), (2, 9, 9, 64)), ((4, 384, 384), (4, 96, 96, 64)), ((0, 7, 9), (0, 2, 3, 64))):
            for dtype in (torch.float32, torch.bfloat16):
                y = resnet.stem(torch.empty(M, 3, H, W, dtype=dtype), *p)
                assert tuple(y.shape) == want and y.dtype == torch.bfloat16


def test_fake_shapes_are_torchs():
    """The output extent of the contract is that of torch's conv and pool."""
    net = _stem_modules()
    from stem_kit import out_hw
    for H, W in ((1, 1), (2, 3), (7, 9), (37, 51), (38, 50), (35, 34), (67, 70)):
        with torch.no_grad():
            y = net.maxpool(net.relu(net.bn1(net.conv1(torch.zeros(1, 3, H, W)))))
        assert tuple(y.shape[2:]) == out_hw(H, W)[2:]


def test_make_fx_records_the_op():
    """As tests/test_ops_tracing.py: the eager bypass must not hide the op from a tracer."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import resnet
    p = resnet.fold_stem(*(getattr(stand_in_backbone(), n) for n in ("conv1", "bn1", "relu", "maxpool")), device="cpu")
    gm = make_fx(lambda x, pk, sc, sh: resnet.stem(x, pk, sc, sh), tracing_mode="fake")(torch.zeros(2, 3, 40, 56), *p)
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.stem.default) == 1
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    out = out[0] if isinstance(out, (list, tuple)) else out
    assert tuple(out.meta["val"].shape) == (2, 10, 14, 64) and out.meta["val"].dtype == torch.bfloat16


# ---------------------------------------------------------------- the three from_reference signatures
def test_stem_torch_is_the_default_and_builds_the_parents_modules():
    from mvn_rocm import backbone, model, resnet
    net = stand_in_backbone()
    for trunk in (resnet.TrunkEval.from_reference(net, device="cpu"), resnet.TrunkEval.from_reference(net, device="cpu", stem="torch")):
        assert type(trunk.stem) is nn.Sequential
        assert [type(m) for m in trunk.stem] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d]
        assert all(a is b for a, b in zip(trunk.stem, (net.conv1, net.bn1, net.relu, net.maxpool)))
        assert len(trunk.blocks) == 6
    for be in (backbone.BackboneEval.from_reference(net, device="cpu"),
               backbone.BackboneEval.from_reference(net, device="cpu", trunk="torch", stem="torch")):
        assert type(be.trunk) is nn.Sequential and len(be.trunk) == 8 and be.trunk[0] is net.conv1
    be = backbone.BackboneEval.from_reference(net, device="cpu", trunk="kernels")
    assert type(be.trunk.stem) is nn.Sequential and be.trunk.stem[0] is net.conv1
    mnet = stand_in_trunk_model()
    assert type(model.VolumetricModelEval.from_reference(mnet, device="cpu").backbone.trunk) is nn.Sequential
    me = model.VolumetricModelEval.from_reference(mnet, device="cpu", trunk="kernels")
    assert type(me.backbone.trunk.stem) is nn.Sequential and me.backbone.trunk.stem[3] is mnet.backbone.maxpool


def test_stem_kernels_replaces_the_stem_and_the_cast_pass():
    from mvn_rocm import backbone, model, resnet
    net = stand_in_backbone()
    want = resnet.fold_stem(net.conv1, net.bn1, net.relu, net.maxpool, device="cpu")
    default = resnet.TrunkEval.from_reference(net, device="cpu")
    trunk = resnet.TrunkEval.from_reference(net, device="cpu", stem="kernels")
    assert isinstance(trunk.stem, resnet.StemEval)
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(trunk.stem.params, want))
    assert not any(isinstance(m, (nn.Conv2d, nn.BatchNorm2d, nn.MaxPool2d, nn.ReLU)) for m in trunk.modules())   # no torch layer is left
    for a, b in zip(trunk.blocks, default.blocks):                # the stages are the default's
        assert all(torch.equal(x, y) for x, y in zip(a.buffers(), b.buffers()))
    be = backbone.BackboneEval.from_reference(net, device="cpu", trunk="kernels", stem="kernels")
    assert isinstance(be.trunk.stem, resnet.StemEval) and be.cast_for_confidences
    me = model.VolumetricModelEval.from_reference(stand_in_trunk_model(), device="cpu", trunk="kernels", stem="kernels")
    assert isinstance(me.backbone.trunk.stem, resnet.StemEval)


def test_from_reference_value_errors():
    from mvn_rocm import backbone, model, resnet
    net, mnet = stand_in_backbone(), stand_in_trunk_model()
    for bad in ("hip", "kernel", None, True):
        with pytest.raises(ValueError, match="TrunkEval: stem must be 'torch' or 'kernels', got"):
            resnet.TrunkEval.from_reference(net, device="cpu", stem=bad)
        with pytest.raises(ValueError, match="BackboneEval: stem must be 'torch' or 'kernels', got"):
            backbone.BackboneEval.from_reference(net, device="cpu", trunk="kernels", stem=bad)
        with pytest.raises(ValueError, match="stem must be 'torch' or 'kernels', got"):
            model.VolumetricModelEval.from_reference(mnet, device="cpu", trunk="kernels", stem=bad)
    # the kernel stem writes channels-last bfloat16 for TrunkEval: it cannot feed the torch stages
    for kwargs in (dict(stem="kernels"), dict(trunk="torch", stem="kernels")):
        with pytest.raises(ValueError, match="kernel stem writes channels-last bfloat16 for TrunkEval"):
            backbone.BackboneEval.from_reference(net, device="cpu", **kwargs)
        with pytest.raises(ValueError, match="kernel stem writes channels-last bfloat16 for TrunkEval"):
            model.VolumetricModelEval.from_reference(mnet, device="cpu", **kwargs)
    with pytest.raises(ValueError, match="trunk must be"):
        backbone.BackboneEval.from_reference(net, device="cpu", trunk="hip", stem="kernels")


def test_trunk_eval_names_a_stem_it_cannot_fold():
    from mvn_rocm import resnet
    net = randomise2d(StandInTrunkBackbone(), seed=6)
    net.maxpool = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    assert type(resnet.TrunkEval.from_reference(net, device="cpu").stem) is nn.Sequential       # the torch stem takes it
    with pytest.raises(RuntimeError, match="TrunkEval: fold_stem: .*ceil_mode=True"):
        resnet.TrunkEval.from_reference(net, device="cpu", stem="kernels")
