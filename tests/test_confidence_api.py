"""The confidence heads' Python surface without a GPU (mvn_rocm/confidence.py): the packers
against the documented layouts, ``fold_confidence_head``'s fold and refusals, the fake kernels, the
``confidences=`` switch of ``BackboneEval`` and ``AlgebraicModelEval``'s construction."""
import copy

import pytest
import torch
from torch import nn

from confidence_kit import (GlobalAveragePoolingHead, StandInAlgebraicModel, element_pool, index_weight_pool, random_tail,
                            small_head, stand_in_backbone, tail_element, tail_offsets, unpack_pool, unpack_tail)


# ----------------------------------------------------------------------------- packers
@pytest.mark.parametrize("cout, cin", ((64, 64), (128, 192), (512, 2048)))
def test_pool_weight_round_trips_and_matches_the_element_formula(cout, cin):
    from mvn_rocm import _lib, confidence
    w = index_weight_pool(cout, cin)
    packed = confidence.pack_conv3x3_pool_weight(w.double())
    assert tuple(packed.shape) == (9, cin // 32, cout // 16, 64, 8) and packed.dtype == torch.bfloat16
    assert packed.numel() * 2 == _lib.load().mvn_conv3x3_pool_packed_weight_bytes(cin, cout)
    assert torch.equal(unpack_pool(packed, cout, cin), w.double())
    g = torch.Generator().manual_seed(cout + cin)
    for _ in range(200):
        tap, kp, m, lane, j = (int(torch.randint(0, n, (1,), generator=g)) for n in packed.shape)
        (co, ci, ky, kx), v = element_pool(packed, tap, kp, m, lane, j)
        assert v == float(w[co, ci, ky, kx])


def test_pool_weight_is_rounded_once_to_bf16_and_refuses_other_shapes():
    from mvn_rocm import confidence
    w = torch.randn(64, 64, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(unpack_pool(confidence.pack_conv3x3_pool_weight(w), 64, 64), w.float().bfloat16().double())
    for bad in (torch.zeros(64, 64, 1, 1), torch.zeros(64, 96, 3, 3), torch.zeros(576, 64, 3, 3), torch.zeros(64, 2112, 3, 3)):
        with pytest.raises(RuntimeError):
            confidence.pack_conv3x3_pool_weight(bad.double())
    assert tuple(confidence.pack_conv3x3_pool_weight(torch.zeros(512, 2048, 3, 3).double()).shape) == (9, 64, 32, 64, 8)


@pytest.mark.parametrize("widths", ((64, 64, 64, 1), (64, 128, 64, 5), (256, 512, 256, 32)))
def test_tail_round_trips_and_matches_the_element_formula(widths):
    from mvn_rocm import _lib, confidence
    c0, c1, c2, n = widths
    _, linears = random_tail((1, 1) + widths, seed=sum(widths))
    p = confidence.pack_confidence_tail(linears)
    assert p.widths == widths and p.packed.dtype == torch.float32
    assert p.packed.numel() * 4 == _lib.load().mvn_confidence_tail_packed_bytes(*widths) == tail_offsets(*widths)[5] * 4
    for (W, b), (Wu, bu) in zip(linears, unpack_tail(p.packed, widths)):
        assert torch.equal(W, Wu) and torch.equal(b, bu)
    g = torch.Generator().manual_seed(3)
    for layer, (W, _) in enumerate(linears, start=1):
        for _ in range(100):
            o, i = int(torch.randint(0, W.shape[0], (1,), generator=g)), int(torch.randint(0, W.shape[1], (1,), generator=g))
            assert tail_element(p.packed, widths, layer, i, o) == float(W[o, i])


def test_tail_packer_refusals():
    from mvn_rocm import confidence
    mk = lambda o, i: (torch.zeros(o, i), torch.zeros(o))
    with pytest.raises(RuntimeError, match="three"):
        confidence.pack_confidence_tail([mk(64, 64), mk(64, 64)])
    with pytest.raises(RuntimeError, match="in_features=128"):
        confidence.pack_confidence_tail([mk(64, 64), mk(64, 128), mk(5, 64)])
    with pytest.raises(RuntimeError, match="out_features=33"):
        confidence.pack_confidence_tail([mk(64, 64), mk(64, 64), mk(33, 64)])
    with pytest.raises(RuntimeError, match="C1"):
        confidence.pack_confidence_tail([mk(96, 64), mk(64, 96), mk(5, 64)])
    with pytest.raises(RuntimeError, match="C0"):
        confidence.pack_confidence_tail([mk(64, 576), mk(64, 64), mk(5, 64)])
    assert _lib_bytes(64, 64, 64, 33) == 0 and _lib_bytes(64, 64, 64, 0) == 0 and _lib_bytes(64, 96, 64, 5) == 0


def _lib_bytes(*widths):
    from mvn_rocm import _lib
    return _lib.load().mvn_confidence_tail_packed_bytes(*widths)


def test_size_functions_refuse_channels_outside_the_sets():
    from mvn_rocm import _lib
    f = _lib.load().mvn_conv3x3_pool_packed_weight_bytes
    assert f(2048, 512) == 9 * 64 * 32 * 64 * 16
    assert f(32, 64) == f(64, 32) == f(2112, 64) == f(64, 576) == f(96, 64) == 0


# ----------------------------------------------------------------------------- the fold
def test_fold_equals_the_float64_fold_with_the_conv_bias():
    from mvn_rocm import confidence
    head = small_head()
    p = confidence.fold_confidence_head(head, device="cpu")
    for conv, bn, folded in ((head.features[0], head.features[1], p.conv1), (head.features[4], head.features[5], p.conv2)):
        assert conv.bias is not None and float(conv.bias.detach().abs().max()) > 0
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        t = (conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()
        assert torch.equal(folded.scale, s.float()) and torch.equal(folded.shift, t.float())
        assert torch.equal(unpack_pool(folded.packed, conv.out_channels, conv.in_channels),
                           conv.weight.detach().bfloat16().double())
    assert p.tail.widths == (64, 128, 64, 5)
    for lin, (W, b) in zip((head.head[0], head.head[2], head.head[4]), unpack_tail(p.tail.packed, p.tail.widths)):
        assert torch.equal(W, lin.weight.detach()) and torch.equal(b, lin.bias.detach())


def test_fold_copies_the_parameters():
    from mvn_rocm import confidence
    head = copy.deepcopy(small_head())
    p = confidence.fold_confidence_head(head, device="cpu")
    before = [t.clone() for t in (p.conv1.packed, p.conv1.scale, p.conv2.shift, p.tail.packed)]
    with torch.no_grad():
        for q in head.parameters():
            q.add_(1.0)
        head.features[1].running_var.add_(1.0)
    for b, t in zip(before, (p.conv1.packed, p.conv1.scale, p.conv2.shift, p.tail.packed)):
        assert torch.equal(b, t)


def _head(**kw):
    return GlobalAveragePoolingHead(64, kw.pop("n", 5), 64, 64, 128, 64).eval()


def _with(head, path, index, module):
    getattr(head, path)[index] = module
    return head


REFUSALS = {
    "a_1x1_conv": (lambda: _with(_head(), "features", 0, nn.Conv2d(64, 64, 1)), r"features\[0:4\].*kernel_size=\(1, 1\)"),
    "stride_2": (lambda: _with(_head(), "features", 4, nn.Conv2d(64, 64, 3, stride=2, padding=1)),
                 r"features\[4:8\].*stride=\(2, 2\)"),
    "maxpool_3": (lambda: _with(_head(), "features", 2, nn.MaxPool2d(3)), r"features\[0:4\].*kernel_size=\(3, 3\)"),
    "ceil_mode": (lambda: _with(_head(), "features", 6, nn.MaxPool2d(2, ceil_mode=True)), r"features\[4:8\].*ceil_mode=True"),
    "no_sigmoid": (lambda: _with(_head(), "head", 5, nn.Identity()), r"Sigmoid\), got \(.*Identity\)"),
    "widths_do_not_chain": (lambda: _with(_head(), "head", 2, nn.Linear(64, 64)), r"head\[2\].*in_features=64"),
    "conv_widths_do_not_chain": (lambda: _with(_head(), "features", 4, nn.Conv2d(128, 64, 3, padding=1)), r"in_channels=128"),
    "n_33": (lambda: _head(n=33), r"out_features=33"),
    "bn_without_running_statistics": (lambda: _with(_head(), "features", 1, nn.BatchNorm2d(64, track_running_stats=False)),
                                      r"running statistics.*track_running_stats=False"),
    "cin_96": (lambda: GlobalAveragePoolingHead(96, 5, 64, 64, 128, 64), r"in_channels must be a multiple of 64"),
    "a_relu_for_the_pool": (lambda: _with(_head(), "features", 2, nn.ReLU()), r"expected a MaxPool2d.*got ReLU"),
    "seven_feature_modules": (lambda: _truncated(), r"of 7 modules"),
}


def _truncated():
    h = _head()
    h.features = nn.Sequential(*list(h.features)[:7])
    return h


@pytest.mark.parametrize("name", REFUSALS)
def test_fold_refuses_by_name(name):
    from mvn_rocm import confidence
    make, pattern = REFUSALS[name]
    with pytest.raises(RuntimeError, match=pattern):
        confidence.fold_confidence_head(make(), device="cpu")
    with pytest.raises(RuntimeError, match=pattern):
        confidence.ConfidenceHeadEval.from_reference(make(), device="cpu")


# ----------------------------------------------------------------------------- fake kernels, tracing
def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import confidence
    with FakeTensorMode():
        x = torch.empty(3, 5, 7, 128, dtype=torch.bfloat16)
        p = (torch.empty(9, 4, 16, 64, 8, dtype=torch.bfloat16), torch.empty(256), torch.empty(256))
        y = confidence.conv3x3_pool(x, *p)
        assert tuple(y.shape) == (3, 2, 3, 256) and y.dtype == torch.bfloat16
        z = confidence.conv3x3_pool(x, *p, out_dtype=torch.float32)
        assert tuple(z.shape) == (3, 2, 3, 256) and z.dtype == torch.float32
        assert tuple(confidence.conv3x3_pool(x[:0], *p).shape) == (0, 2, 3, 256)
        widths = (256, 512, 256, 17)
        tail = confidence.TailParams(torch.empty(tail_offsets(*widths)[5]), widths)
        c = confidence.confidence_tail(z, tail)
        assert tuple(c.shape) == (3, 17) and c.dtype == torch.float32
        assert tuple(confidence.confidence_tail(z, tail, sigmoid=False).shape) == (3, 17)


def test_make_fx_records_the_ops():
    """As tests/test_ops_tracing.py: the eager bypass must not hide the ops from a tracer."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import confidence
    p = confidence.fold_confidence_head(small_head(), device="cpu")

    def head(x, c1, c2, tail_packed):
        return confidence.ConfidenceHeadEval((c1, c2, confidence.TailParams(tail_packed, p.tail.widths)))(x)

    gm = make_fx(head, tracing_mode="fake")(torch.zeros(2, 64, 5, 6), tuple(p.conv1), tuple(p.conv2), p.tail.packed)
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.conv3x3_pool.default) == 2
    assert targets.count(torch.ops.mvn_rocm.confidence_tail.default) == 1
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    out = out[0] if isinstance(out, (list, tuple)) else out
    assert tuple(out.meta["val"].shape) == (2, 5) and out.meta["val"].dtype == torch.float32


# ----------------------------------------------------------------------------- argument checks
def test_cpu_tensors_raise():
    from mvn_rocm import confidence
    p = confidence.fold_confidence_head(small_head(), device="cpu")
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        confidence.conv3x3_pool(x, *p.conv1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        confidence.confidence_tail(torch.zeros(1, 1, 1, 64), p.tail)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        confidence.ConfidenceHeadEval(p)(torch.zeros(1, 64, 4, 4))


def test_wrapper_argument_checks():
    from mvn_rocm import confidence
    p = confidence.fold_confidence_head(small_head(), device="cpu")
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bfloat16"):
        confidence.conv3x3_pool(x.float(), *p.conv1)
    with pytest.raises(TypeError):
        confidence.conv3x3_pool(x, *p.conv1, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        confidence.conv3x3_pool(x[:, :1], *p.conv1)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        confidence.conv3x3_pool(torch.zeros(1, 4, 4, 96, dtype=torch.bfloat16), *p.conv1)
    with pytest.raises(RuntimeError, match="packed"):
        confidence.conv3x3_pool(torch.zeros(1, 4, 4, 128, dtype=torch.bfloat16), *p.conv1)
    with pytest.raises(TypeError, match="float32"):
        confidence.confidence_tail(torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16), p.tail)
    with pytest.raises(RuntimeError, match="128 channels"):
        confidence.confidence_tail(torch.zeros(1, 1, 1, 128), p.tail)
    with pytest.raises(RuntimeError, match="pack_confidence_tail"):
        confidence.confidence_tail(torch.zeros(1, 1, 1, 64), confidence.TailParams(p.tail.packed[:-1], p.tail.widths))
    m = confidence.ConfidenceHeadEval(p)
    with pytest.raises(RuntimeError, match="h, w >= 4"):
        m(torch.zeros(1, 64, 3, 4))
    with pytest.raises(RuntimeError, match=r"\(M, 64, h, w\)"):
        m(torch.zeros(1, 128, 4, 4))
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 64, 4, 4, requires_grad=True))


# ----------------------------------------------------------------------------- the switches
def test_bad_confidences_switch_is_a_value_error():
    from mvn_rocm import backbone, model
    bb = stand_in_backbone()
    with pytest.raises(ValueError, match="confidences must be 'torch' or 'kernels'"):
        backbone.BackboneEval.from_reference(bb, device="cpu", confidences="hip")
    with pytest.raises(ValueError, match="confidences"):
        model.AlgebraicModelEval.from_reference(StandInAlgebraicModel(bb, True, True, 100.0), device="cpu", confidences="")


def test_default_keeps_the_backbones_own_heads():
    from mvn_rocm import backbone, confidence
    bb = stand_in_backbone()
    be = backbone.BackboneEval.from_reference(bb, device="cpu")
    assert be.alg_confidences is bb.alg_confidences and be.vol_confidences is bb.vol_confidences
    assert not be.cast_for_confidences
    be = backbone.BackboneEval.from_reference(bb, device="cpu", trunk="kernels")
    assert be.alg_confidences is bb.alg_confidences and be.vol_confidences is bb.vol_confidences and be.cast_for_confidences
    be = backbone.BackboneEval.from_reference(bb, device="cpu", trunk="kernels", stem="kernels", confidences="kernels")
    assert isinstance(be.alg_confidences, confidence.ConfidenceHeadEval) and be.alg_confidences.widths == (256, 512, 256, 17)
    assert isinstance(be.vol_confidences, confidence.ConfidenceHeadEval) and be.vol_confidences.widths == (256, 512, 256, 32)
    assert not be.cast_for_confidences
    assert not any(isinstance(m, (nn.Conv2d, nn.Linear, nn.BatchNorm2d)) for m in be.modules())
    be = backbone.BackboneEval.from_reference(stand_in_backbone(17, False), device="cpu", confidences="kernels")
    assert be.alg_confidences is None and isinstance(be.vol_confidences, confidence.ConfidenceHeadEval)


def test_algebraic_model_refuses_use_confidences_without_a_head():
    from mvn_rocm import model
    bb = stand_in_backbone(17, False)
    with pytest.raises(RuntimeError, match="use_confidences needs a backbone with an alg_confidences head"):
        model.AlgebraicModelEval.from_reference(StandInAlgebraicModel(bb, True, True, 100.0), device="cpu")
    m = model.AlgebraicModelEval.from_reference(StandInAlgebraicModel(bb, False, False, 1.0), device="cpu")
    assert m.use_confidences is False and m.heatmap_softmax is False and m.heatmap_multiplier == 1.0
    m = model.AlgebraicModelEval.from_reference(StandInAlgebraicModel(stand_in_backbone(), True, True, 100.0), device="cpu")
    assert m.use_confidences and m.heatmap_softmax and m.heatmap_multiplier == 100.0
    with pytest.raises(RuntimeError, match=r"\(B, N, 3, H, W\)"):
        m(torch.zeros(6, 3, 64, 96), torch.zeros(2, 3, 3, 4))
