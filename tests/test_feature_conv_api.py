"""The feature convolution (csrc/feature_conv.hip, mvn_rocm/model.py): the C ABI's argument checks,
the Python wrapper's refusals and fake kernel, ``VolumetricEval.from_reference`` on a stand-in net
and the exact-fma reference that the GPU tests compare against — no GPU needed (only validation
paths are called; they return before any HIP call)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
from torch import nn

from v2v_kit import V2VModel, randomise

OK, ARG, SHAPE = 0, -1, -2
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from mvn_rocm import _lib
    return _lib.load()


# ---------------------------------------------------------------- the exact f32 fma in numpy
def fma32(a, b, c):
    """The correctly rounded float32 fma(a, b, c), elementwise with broadcasting, for finite normal
    operands.  The product of two float32 is exact in float64; TwoSum gives the float64 sum s and
    its error; where the sum is inexact and s's last mantissa bit is 0, s moves to its neighbour
    on the error's side: round-to-odd, after which the cast to float32 rounds once.  (The plain
    ``float32(float64(a) * b + c)`` rounds twice and is wrong about once in 2^29 operations.)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def fma_chain(x, w, b):
    """mvn_feature_conv's contract restated: x (n, Cin, P) f32, w (32, Cin) f32, b (32,) f32 ->
    (n, 32, P) f32 with acc = b[co], then acc = fma32(w[co, ci], x[n, ci, p], acc), ci ascending."""
    x, w, b = (np.asarray(v, np.float32) for v in (x, w, b))
    acc = np.broadcast_to(b[None, :, None], (x.shape[0], w.shape[0], x.shape[2])).astype(np.float32)
    for ci in range(w.shape[1]):
        acc = fma32(w[None, :, ci, None], x[:, None, ci, :], acc)
    return acc


def round_fraction_to_f32(v):
    """A Fraction rounded to the nearest float32, ties to even (normal range)."""
    if v == 0:
        return np.float32(0.0)
    sign, v = (-1.0 if v < 0 else 1.0), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    scaled = v / Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * math.ldexp(n, e - 23))


def near_tie_triples(rng, count):
    """a * b + c within 2^-70 of a float32 rounding tie of c in [1, 2): a = 2^-24 (1 + m 2^-23),
    b = k (1 - m 2^-23) (k odd), so a * b = k 2^-24 (1 - m^2 2^-46): the float64 sum lands on the
    tie exactly and a second rounding goes the wrong way for half of them."""
    m = rng.integers(1, 1 << 10, count).astype(np.float64)
    k = rng.choice([1.0, 3.0, 5.0, 7.0], count)
    a = (2.0 ** -24 * (1 + m * 2.0 ** -23)).astype(np.float32)
    b = (k * (1 - m * 2.0 ** -23)).astype(np.float32)
    c = (1 + rng.integers(0, 1 << 23, count) * 2.0 ** -23).astype(np.float32)
    flip = rng.choice([1.0, -1.0], count).astype(np.float32)
    return a * flip, b, c * flip


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(5)
    n = 2000
    a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    c = c * (a * b != 0)                                    # keep the sum in the products' range
    ta, tb, tc = near_tie_triples(rng, n)
    # cancellation: c close to -a*b
    ca, cb = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    cc = -(ca.astype(np.float64) * cb).astype(np.float32)
    a, b, c = np.concatenate([a, ta, ca]), np.concatenate([b, tb, cb]), np.concatenate([c, tc, cc])
    got = fma32(a, b, c)
    want = np.array([round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the near ties are what the helper is for: the twice-rounded expression misses some of them
    naive = (ta.astype(np.float64) * tb + tc).astype(np.float32)
    assert (naive.view(np.uint32) != want[n:2 * n].view(np.uint32)).any()


def test_fma_chain_matches_a_scalar_loop():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 32, 3)).astype(np.float32)
    w = (rng.standard_normal((32, 32)) / 16).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32)
    got = fma_chain(x, w, b)
    for n, co, p in ((0, 0, 0), (1, 31, 2), (0, 17, 1)):
        acc = Fraction(float(b[co]))
        for ci in range(32):
            acc = Fraction(float(round_fraction_to_f32(Fraction(float(w[co, ci])) * Fraction(float(x[n, ci, p])) + acc)))
        assert np.float32(float(acc)) == got[n, co, p]


# ---------------------------------------------------------------- C argument validation
def _conv(lib, **k):
    return lib.mvn_feature_conv(k.get("x", 1), k.get("xd", F32), k.get("w", 1), k.get("b", 1), k.get("out", 1),
                                k.get("od", F32), k.get("n", 2), k.get("cin", 256), k.get("cout", 32), k.get("H", 5),
                                k.get("W", 7), None)


def test_argument_validation(lib):
    """Every documented error code, with no device: the checks run before any HIP call."""
    for name in ("x", "w", "out"):
        assert _conv(lib, **{name: None}) == ARG
    for code in (-1, 2, 7):
        assert _conv(lib, xd=code) == ARG and _conv(lib, od=code) == ARG
    for cout in (0, 16, 31, 33, 64):
        assert _conv(lib, cout=cout) == SHAPE
    for cin in (0, 16, 48, 544, -32, 1024):
        assert _conv(lib, cin=cin) == SHAPE
    assert _conv(lib, n=-1) == SHAPE and _conv(lib, H=-1) == SHAPE and _conv(lib, W=-3) == SHAPE
    # nothing to do: MVN_OK without a launch (there is no device here)
    assert _conv(lib, H=0) == OK and _conv(lib, W=0) == OK and _conv(lib, n=0) == OK
    assert _conv(lib, H=0, b=None) == OK
    assert _conv(lib, H=0, x=None) == ARG and _conv(lib, H=0, cin=48) == SHAPE      # errors come first
    # one image's maps above 2^31 - 1 bytes
    assert _conv(lib, cin=256, H=2048, W=1024) == SHAPE                  # 256 * 2^21 * 4 = 2^31
    assert _conv(lib, cin=512, H=1024, W=1024, xd=F32) == SHAPE
    assert _conv(lib, cin=512, H=2048, W=1024, xd=BF16) == SHAPE         # 2^31 bytes of bf16
    assert _conv(lib, cin=32, H=2 ** 30, W=2 ** 30) == SHAPE             # H * W itself beyond int
    assert _conv(lib, n=2 ** 40, H=1, W=1) == SHAPE                      # more tiles than an int counts


# ---------------------------------------------------------------- the Python wrapper
def test_wrapper_refusals():
    from mvn_rocm import model
    x, w, b = torch.zeros(2, 64, 5, 7), torch.zeros(32, 64), torch.zeros(32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.feature_conv(x, w, b)
    for wt in (w, w.view(32, 64, 1, 1)):                       # both weight shapes reach the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.feature_conv(x, wt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.feature_conv(x.view(1, 2, 64, 5, 7).bfloat16(), w, b, out_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="inference-only.*conv2d"):
        model.feature_conv(x.clone().requires_grad_(), w, b)
    with pytest.raises(RuntimeError, match="inference-only"):
        model.feature_conv(x, w.clone().requires_grad_(), b)
    with torch.no_grad():                                      # allowed under no_grad: reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.feature_conv(x.clone().requires_grad_(), w, b)
    for bad in (torch.zeros(32, 32), torch.zeros(16, 64), torch.zeros(64, 32), torch.zeros(32, 64, 3, 3),
                torch.zeros(32, 64, 1), torch.zeros(32 * 64)):
        with pytest.raises(RuntimeError, match="weight must be"):
            model.feature_conv(x, bad, b)
    with pytest.raises(RuntimeError, match="bias must be"):
        model.feature_conv(x, w, torch.zeros(64))
    with pytest.raises(RuntimeError, match="x must be"):
        model.feature_conv(x[0], w, b)
    for cin in (16, 48, 544):
        with pytest.raises(RuntimeError, match="multiple of 32"):
            model.feature_conv(torch.zeros(1, cin, 2, 2), torch.zeros(32, cin))
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        model.feature_conv(x.half(), w, b)
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        model.feature_conv(x, w, b, out_dtype=torch.float16)


def test_fake_kernel_keeps_the_leading_dimensions():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvn_rocm import model
    with FakeTensorMode():
        w, b = torch.empty(32, 256), torch.empty(32)
        y = model.feature_conv(torch.empty(6, 256, 17, 23), w, b)
        assert tuple(y.shape) == (6, 32, 17, 23) and y.dtype == torch.float32
        y = model.feature_conv(torch.empty(2, 3, 256, 17, 23), w.view(32, 256, 1, 1), None, out_dtype=torch.bfloat16)
        assert tuple(y.shape) == (2, 3, 32, 17, 23) and y.dtype == torch.bfloat16
        y = model.feature_conv(torch.empty(2, 3, 256, 4, 4, dtype=torch.bfloat16), w)
        assert tuple(y.shape) == (2, 3, 32, 4, 4) and y.dtype == torch.bfloat16
        y = model.feature_conv(torch.empty(0, 3, 256, 4, 4), w)
        assert tuple(y.shape) == (0, 3, 32, 4, 4)
        y = torch.ops.mvn_rocm.feature_conv(torch.empty(5, 64, 3, 3), torch.empty(32, 64), None, BF16)
        assert tuple(y.shape) == (5, 32, 3, 3) and y.dtype == torch.bfloat16


def test_make_fx_records_the_op():
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import model
    gm = make_fx(lambda x, w, b: model.feature_conv(x, w, b, out_dtype=torch.bfloat16), tracing_mode="fake")(
        torch.zeros(2, 3, 64, 5, 7), torch.zeros(32, 64, 1, 1), torch.zeros(32))
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert torch.ops.mvn_rocm.feature_conv.default in targets
    out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
    assert tuple(out.meta["val"].shape) == (2, 3, 32, 5, 7) and out.meta["val"].dtype == torch.bfloat16


# ---------------------------------------------------------------- VolumetricEval.from_reference
class StandInNet(nn.Module):
    """The attributes of VolumetricTriangulationNet that VolumetricEval reads (triangulation.py:203-242)."""

    def __init__(self, process_features, J=5, method="softmax", multiplier=3.0, softmax=True):
        super().__init__()
        self.process_features = process_features
        self.volume_net = V2VModel(32, J)
        self.volume_aggregation_method = method
        self.volume_multiplier = multiplier
        self.volume_softmax = softmax


def stand_in_net(conv=None, seed=7, **k):
    g = torch.Generator().manual_seed(seed)
    conv = conv if conv is not None else nn.Conv2d(256, 32, 1)
    pf = conv if isinstance(conv, nn.Sequential) else nn.Sequential(conv)
    with torch.no_grad():
        for p in pf.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    net = StandInNet(pf, **k)
    randomise(net.volume_net, seed=seed)
    return net.eval()


@pytest.mark.parametrize("conv, found", [
    (nn.Conv2d(256, 32, 3, padding=1), r"kernel_size=\(3, 3\)"),
    (nn.Conv2d(256, 32, 1, stride=2), r"stride=\(2, 2\)"),
    (nn.Conv2d(256, 32, 1, groups=2), "groups=2"),
    (nn.Conv2d(256, 16, 1), "out_channels=16"),
    (nn.Conv2d(256, 32, 1, padding=1), r"padding=\(1, 1\)"),
    (nn.Conv2d(256, 32, 1, dilation=2), r"dilation=\(2, 2\)"),
    (nn.Sequential(nn.Conv2d(256, 32, 1), nn.ReLU()), "Sequential of 2 modules"),
    (nn.Sequential(nn.Linear(256, 32)), "Linear"),
    (nn.Conv2d(48, 32, 1), "got 48"),
], ids=["3x3", "stride2", "groups2", "cout16", "padding1", "dilation2", "two_modules", "linear", "cin48"])
def test_from_reference_refuses_and_names_what_it_found(conv, found):
    from mvn_rocm import model
    with pytest.raises(RuntimeError, match=found):
        model.VolumetricEval.from_reference(stand_in_net(conv), device="cpu")


def test_from_reference_refuses_a_bare_conv():
    from mvn_rocm import model
    net = stand_in_net()
    net.process_features = net.process_features[0]
    with pytest.raises(RuntimeError, match="Sequential of exactly one Conv2d, got Conv2d"):
        model.VolumetricEval.from_reference(net, device="cpu")


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "no_bias"))
def test_from_reference_reads_the_model(bias):
    from mvn_rocm import model, v2v
    net = stand_in_net(nn.Conv2d(256, 32, 1, bias=bias), method="conf_norm", multiplier=2.5, softmax=False)
    ev = model.VolumetricEval.from_reference(net, device="cpu", feature_dtype=torch.float32, precision="fast")
    conv = net.process_features[0]
    assert tuple(ev.weight.shape) == (32, 256) and torch.equal(ev.weight, conv.weight.detach().view(32, 256))
    assert (ev.bias is None) == (not bias)
    if bias:
        assert torch.equal(ev.bias, conv.bias.detach())
    assert not ev.weight.requires_grad and ev.weight.data_ptr() != conv.weight.data_ptr()      # a copy
    assert (ev.volume_aggregation_method, ev.volume_multiplier, ev.volume_softmax) == ("conf_norm", 2.5, False)
    assert ev.feature_dtype == torch.float32 and ev.precision == "fast"
    # the default: the whole V2V on kernels, no torch module left
    assert isinstance(ev.v2v, v2v.V2VEval) and ev.v2v.interior is None and len(ev.v2v.deep) == 16
    assert not any(isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose3d, nn.BatchNorm3d)) for m in ev.modules())
    assert model.VolumetricEval.from_reference(net, device="cpu").feature_dtype == torch.bfloat16
    ev = model.VolumetricEval.from_reference(net, device="cpu", half_res="torch", deep="torch")
    assert ev.v2v.half_res is None and ev.v2v.deep is None
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        model.VolumetricEval.from_reference(net, device="cpu", feature_dtype=torch.float16)


def test_volumetric_eval_refusals():
    from mvn_rocm import model
    ev = model.VolumetricEval.from_reference(stand_in_net(method="conf_norm"), device="cpu")
    f, P, cv = torch.zeros(1, 2, 256, 4, 4), torch.zeros(1, 2, 3, 4), torch.zeros(1, 32, 32, 32, 3)
    with pytest.raises(RuntimeError, match="inference-only"):
        ev(f.clone().requires_grad_(), P, cv, torch.ones(1, 2, 32))
    with pytest.raises(RuntimeError, match="inference-only"):
        ev(f, P, cv, torch.ones(1, 2, 32).requires_grad_())
    with pytest.raises(TypeError, match="needs vol_confidences"):
        ev(f, P, cv)
    with pytest.raises(RuntimeError, match="features must be"):
        ev(f[0], P, cv, torch.ones(1, 2, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev(f, P, cv, torch.ones(1, 2, 32))
