"""mvn_deconv4s2_project and what is built on it (csrc/deconv_head.hip, mvn_rocm/backbone.py,
mvn_rocm/model.py) without a GPU: the packed projection against the element formula
of include/mvn_hip.h, the hi | lo split against float64, every MVN_ERR_ARG path of the C entry (the
checks run before any HIP call), the refusals of ``from_reference`` and of ``project`` with
``heatmaps=True``, the autograd refusal, the fake kernel and the traced op."""
import pytest
import torch
from torch import nn

from deconv_kit import COUT
from deconv_project_kit import (PACKED_SHAPE, ROWS, StandInBackbone, index_projection, split, stand_in_model,
                                unpack_projection)

OK, ARG = 0, -1
F32, BF16 = 0, 1
A = 4096                         # a 16-byte aligned stand-in address: the checks never dereference it


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


def random_weight(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(ROWS, COUT, generator=g) * (2.0 / 288) ** 0.5, torch.randn(ROWS, generator=g)


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("kind", ("index", "random", "conv_shape"))
def test_pack_round_trip_by_the_documented_formula(kind, lib):
    from mvn_rocm import backbone
    w, b = (index_projection(), None) if kind == "index" else random_weight(3)
    p = backbone.pack_projection(w.view(ROWS, COUT, 1, 1) if kind == "conv_shape" else w, b, device="cpu")
    assert isinstance(p, backbone.ProjectionParams)
    assert tuple(p.packed.shape) == PACKED_SHAPE and p.packed.dtype == torch.bfloat16 and p.packed.is_contiguous()
    assert p.packed.numel() * 2 == lib.mvn_deconv4s2_project_weight_bytes() == 32768
    assert p.bias.dtype == torch.float32 and tuple(p.bias.shape) == (ROWS,)
    assert torch.equal(p.bias, torch.zeros(ROWS) if b is None else b)
    hi, lo = split(w)
    got_hi, got_lo = unpack_projection(p.packed)
    assert torch.equal(got_hi, hi) and torch.equal(got_lo, lo)
    # the formula read literally for a few (part, k, nt, lane, j)
    for part, k, nt, lane, j in ((0, 0, 0, 0, 0), (1, 7, 1, 63, 7), (0, 3, 1, 17, 5), (1, 5, 0, 40, 2), (0, 6, 0, 15, 4)):
        row, col = 16 * nt + (lane & 15), 32 * k + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
        assert float(p.packed[part, k, nt, lane, j]) == float((hi, lo)[part][row, col])


def test_the_split_against_float64():
    """hi is w rounded once to bf16, lo the float64 remainder rounded once; hi + lo is within 2^-17
    relative of w (half a bf16 ulp of the remainder, which is at most half a bf16 ulp of w)."""
    from mvn_rocm import backbone
    w, _ = random_weight(4)
    hi, lo = unpack_projection(backbone.pack_projection(w, device="cpu").packed)
    assert torch.equal(hi, w.bfloat16().double())
    assert torch.equal(lo, (w.double() - hi).float().bfloat16().double())
    assert bool((lo != 0).any())
    assert bool(((hi + lo - w.double()).abs() <= 2.0 ** -17 * w.double().abs()).all())
    exact = torch.randint(-4, 5, (ROWS, COUT)).float()
    hi, lo = unpack_projection(backbone.pack_projection(exact, device="cpu").packed)
    assert torch.equal(hi, exact.double()) and not bool(lo.any())


def test_pack_refuses_other_shapes():
    from mvn_rocm import backbone
    for bad in (torch.zeros(17, COUT), torch.zeros(ROWS, 128), torch.zeros(ROWS, COUT, 3, 3), torch.zeros(COUT, ROWS)):
        with pytest.raises(RuntimeError, match="weight must be"):
            backbone.pack_projection(bad, device="cpu")
    with pytest.raises(RuntimeError, match="bias must be"):
        backbone.pack_projection(torch.zeros(ROWS, COUT), torch.zeros(17), device="cpu")


# ---------------------------------------------------------------- C argument validation
NAMES = ("x", "w", "scale", "shift", "proj", "bias", "out")


def _project(lib, **k):
    return lib.mvn_deconv4s2_project(*(k.get(n, A) for n in NAMES), k.get("od", BF16), k.get("n", 2), k.get("cin", 256),
                                     k.get("H", 5), k.get("W", 7), None)


def test_argument_validation(lib):
    """Every refusal is MVN_ERR_ARG and comes before any HIP call (there is no device here)."""
    for name in NAMES:
        assert _project(lib, **{name: None}) == ARG
    for cin in (0, 16, 48, 2080, -32, 4096):
        assert _project(lib, cin=cin) == ARG
    assert _project(lib, H=0) == ARG and _project(lib, W=0) == ARG and _project(lib, H=-1) == ARG
    assert _project(lib, n=-1) == ARG
    for od in (-1, 2, 7):
        assert _project(lib, od=od) == ARG
    # the size guards of mvn_deconv4s2
    assert _project(lib, H=1024, W=512) == ARG
    assert _project(lib, H=724, W=724, n=0) == OK
    assert _project(lib, H=725, W=724) == ARG
    assert _project(lib, cin=2048, H=512, W=512, n=0) == OK
    assert _project(lib, cin=2048, H=1024, W=512) == ARG
    assert _project(lib, H=2 ** 30, W=2 ** 30) == ARG
    assert _project(lib, n=2 ** 40, H=1, W=1) == ARG
    for name in NAMES:
        assert _project(lib, **{name: A + 2}) == ARG
        assert _project(lib, **{name: A + 8}) == ARG
    # an empty batch is nothing to do, but its errors come first
    assert _project(lib, n=0) == OK and _project(lib, n=0, od=F32) == OK
    assert _project(lib, n=0, bias=None) == ARG and _project(lib, n=0, cin=48) == ARG and _project(lib, n=0, H=0) == ARG


# ---------------------------------------------------------------- the Python wrapper
def _params(cin=64):
    return (torch.zeros(16, cin // 32, 16, 64, 8, dtype=torch.bfloat16), torch.ones(COUT), torch.zeros(COUT))


def _proj():
    return (torch.zeros(PACKED_SHAPE, dtype=torch.bfloat16), torch.zeros(ROWS))


def test_wrapper_refusals():
    """The checks and errors of deconv4s2, and the projection's own."""
    from mvn_rocm import backbone
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        backbone.deconv4s2_project(x, _params(), _proj())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        backbone.deconv4s2_project(x, _params(), _proj(), torch.float32)
    with pytest.raises(TypeError, match="x_cl must be bfloat16"):
        backbone.deconv4s2_project(x.float(), _params(), _proj())
    with pytest.raises(RuntimeError, match="x_cl must be"):
        backbone.deconv4s2_project(x[0], _params(), _proj())
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        backbone.deconv4s2_project(x, _params(), _proj(), torch.float16)
    for cin in (16, 48, 2080):
        with pytest.raises(RuntimeError, match="multiple of 32"):
            backbone.deconv4s2_project(torch.zeros(1, 2, 2, cin, dtype=torch.bfloat16), _params(), _proj())
    with pytest.raises(RuntimeError, match="fold_deconv_block returns"):
        backbone.deconv4s2_project(x, _params(32), _proj())
    with pytest.raises(RuntimeError, match="at least 1"):
        backbone.deconv4s2_project(torch.zeros(1, 0, 5, 64, dtype=torch.bfloat16), _params(), _proj())
    with pytest.raises(RuntimeError, match="pack_projection returns"):
        backbone.deconv4s2_project(x, _params(), (torch.zeros(ROWS, COUT, dtype=torch.bfloat16), torch.zeros(ROWS)))
    with pytest.raises(RuntimeError, match="pack_projection returns"):
        backbone.deconv4s2_project(x, _params(), (_proj()[0], torch.zeros(17)))
    with pytest.raises(RuntimeError, match="pack_projection returns"):
        backbone.deconv4s2_project(x, _params(), (_proj()[0].float(), torch.zeros(ROWS)))


def test_autograd_is_refused():
    from mvn_rocm import backbone, model
    x = torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="inference-only.*process_features"):
        backbone.deconv4s2_project(x.clone().requires_grad_(), _params(), _proj())
    with pytest.raises(RuntimeError, match="inference-only"):
        backbone.deconv4s2_project(x, _params(), (_proj()[0], torch.zeros(ROWS).requires_grad_()))
    with torch.no_grad():                                      # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            backbone.deconv4s2_project(x.clone().requires_grad_(), _params(), _proj())
    net = stand_in_model()
    head = backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu", heatmaps=False,
                                                  process_features=net.process_features)
    with pytest.raises(RuntimeError, match="inference-only"):
        head(torch.zeros(1, 64, 3, 4).requires_grad_())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(1, 64, 3, 4))
    ev = model.VolumetricModelEval.from_reference(net, device="cpu", fused=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        ev(torch.zeros(1, 2, 3, 12, 16).requires_grad_(), None, None)
    with pytest.raises(RuntimeError, match="images must be"):
        ev(torch.zeros(2, 3, 12, 16), None, None)


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import backbone
    with FakeTensorMode():
        x = torch.empty(3, 5, 7, 64, dtype=torch.bfloat16)
        p = (torch.empty(16, 2, 16, 64, 8, dtype=torch.bfloat16), torch.empty(COUT), torch.empty(COUT))
        pr = (torch.empty(PACKED_SHAPE, dtype=torch.bfloat16), torch.empty(ROWS))
        y = backbone.deconv4s2_project(x, p, pr)
        assert tuple(y.shape) == (3, ROWS, 10, 14) and y.dtype == torch.bfloat16
        y = backbone.deconv4s2_project(x, p, pr, torch.float32)
        assert tuple(y.shape) == (3, ROWS, 10, 14) and y.dtype == torch.float32
        y = backbone.deconv4s2_project(x[:0], p, pr)
        assert tuple(y.shape) == (0, ROWS, 10, 14)


def test_make_fx_records_the_op():
    """As tests/test_ops_tracing.py: the eager bypass must not hide the op from a tracer."""
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import backbone

    def two_layers(x, pk1, pk2, sc, sh, pp, pb):
        return backbone.deconv4s2_project(backbone.deconv4s2(x, (pk1, sc, sh)), (pk2, sc, sh), (pp, pb), torch.float32)

    gm = make_fx(two_layers, tracing_mode="fake")(torch.zeros(2, 3, 5, 64, dtype=torch.bfloat16), _params(64)[0],
                                                  _params(COUT)[0], torch.ones(COUT), torch.zeros(COUT), *_proj())
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.deconv4s2.default) == 1
    assert targets.count(torch.ops.mvn_rocm.deconv4s2_project.default) == 1
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    assert tuple(out.meta["val"].shape) == (2, ROWS, 12, 20) and out.meta["val"].dtype == torch.float32


# ---------------------------------------------------------------- from_reference
@pytest.mark.parametrize("pf, found", [
    (nn.Sequential(nn.Conv2d(COUT, ROWS, 3, padding=1)), r"kernel_size=\(3, 3\)"),
    (nn.Sequential(nn.Conv2d(COUT, 16, 1)), "out_channels=16"),
    (nn.Sequential(nn.Conv2d(COUT, ROWS, 1), nn.ReLU()), "Sequential of 2 modules"),
    (nn.Conv2d(COUT, ROWS, 1), "got Conv2d"),
    (nn.Sequential(nn.Linear(COUT, ROWS)), "Linear"),
    (nn.Sequential(nn.Conv2d(128, ROWS, 1)), "in_channels=128"),
    (nn.Sequential(nn.Conv2d(48, ROWS, 1)), "got 48"),
], ids=["3x3", "cout16", "two_modules", "bare_conv", "linear", "cin128", "cin48"])
def test_from_reference_refuses_and_names_what_it_found(pf, found):
    from mvn_rocm import backbone
    net = stand_in_model()
    with pytest.raises(RuntimeError, match=found):
        backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu", heatmaps=False, process_features=pf)
    with pytest.raises(RuntimeError, match=found):
        backbone.BackboneEval.from_reference(net.backbone, device="cpu", heatmaps=False, process_features=pf)


def test_project_with_heatmaps_is_refused_and_says_why():
    from mvn_rocm import backbone
    net = stand_in_model()
    why = "256-channel map is not formed.*final_layer has nothing to read"
    with pytest.raises(RuntimeError, match=why):
        backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu", process_features=net.process_features)
    with pytest.raises(RuntimeError, match=why):
        backbone.BackboneEval.from_reference(net.backbone, device="cpu", heatmaps=True, process_features=net.process_features)
    pr = backbone.pack_projection(torch.zeros(ROWS, COUT), device="cpu")
    with pytest.raises(RuntimeError, match=why):
        backbone.DeconvHeadEval([_params()], torch.zeros(ROWS, COUT), torch.zeros(ROWS), 17, project=pr)


def test_from_reference_reads_the_model():
    from mvn_rocm import backbone, model
    net = stand_in_model()
    conv = net.process_features[0]
    plain = backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu")
    assert not plain.project and not hasattr(plain, "proj_packed") and plain.heatmaps        # nothing changes without the keyword
    head = backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu", heatmaps=False,
                                                  process_features=net.process_features)
    assert head.project and not head.heatmaps
    want = backbone.pack_projection(conv.weight, conv.bias, device="cpu")
    assert torch.equal(head.proj_packed, want.packed) and torch.equal(head.proj_bias, conv.bias.detach())
    assert not head.proj_packed.requires_grad and not head.proj_bias.requires_grad
    for i in range(3):
        assert all(torch.equal(a, b) for a, b in zip(head.layer_params(i), plain.layer_params(i)))
    no_bias = nn.Sequential(nn.Conv2d(COUT, ROWS, 1, bias=False))
    h2 = backbone.DeconvHeadEval.from_reference(net.backbone, device="cpu", heatmaps=False, process_features=no_bias)
    assert not h2.proj_bias.any()
    for fused in (True, False):
        ev = model.VolumetricModelEval.from_reference(net, device="cpu", feature_dtype=torch.float32, fused=fused)
        assert ev.fused == fused and ev.backbone.head.project == fused and not ev.backbone.head.heatmaps
        assert ev.backbone.head.feature_dtype == torch.float32 and ev.volumetric.feature_dtype == torch.float32
        assert ev.backbone.trunk[0] is net.backbone.conv1
        assert torch.equal(ev.volumetric.weight, conv.weight.detach().view(ROWS, COUT))
    assert model.VolumetricModelEval.from_reference(net, device="cpu").fused == model.FUSED_DEFAULT


def test_from_projected_checks_its_features():
    from mvn_rocm import model
    ev = model.VolumetricEval.from_reference(stand_in_model(), device="cpu")
    with pytest.raises(RuntimeError, match="features32 must be"):
        ev.from_projected(torch.zeros(2, 3, COUT, 8, 8), None, None)
    with pytest.raises(RuntimeError, match="features32 must be"):
        ev.from_projected(torch.zeros(6, ROWS, 8, 8), None, None)
    ev.volume_aggregation_method = "conf_norm"
    with pytest.raises(TypeError, match="needs vol_confidences"):
        ev.from_projected(torch.zeros(2, 3, ROWS, 8, 8), None, None)
    with pytest.raises(TypeError, match="needs vol_confidences"):
        ev(torch.zeros(2, 3, COUT, 8, 8), None, None)
