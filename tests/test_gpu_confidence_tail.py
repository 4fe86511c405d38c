"""mvn_confidence_tail on the GPU (csrc/confidence_head.hip): the logits against the contract's
chain of exact f32 fmas bit for bit, integer data against integer arithmetic, one-hot inputs with index weights
through every slot of the transposed layout, a NaN image, the sigmoid against float64 on the kernel's own
logits, the C entry's argument errors and the dispatcher (tests/confidence_kit.py)."""
import numpy as np
import pytest
import torch

from confidence_kit import TAIL_SHAPES, random_tail, shape_id, tail_logits
from v2v_kit import assert_same_bits

pytestmark = pytest.mark.gpu

EXP_ULPS = 1                                   # include/mvn_hip.h: expf of the HIP device library, 1 ulp
SIGMOID_BAR = (EXP_ULPS + 2) * 2.0 ** -24      # the exp, one add and one division beside it


def run(device, pooled, linears, sigmoid):
    """pooled (M, hw, C0) f32 on the CPU -> the kernel's (M, n) on the CPU."""
    from mvn_rocm import confidence
    p = confidence.pack_confidence_tail(linears)
    M, hw, c0 = pooled.shape
    return confidence.confidence_tail(pooled.view(M, hw, 1, c0).to(device), (p.packed.to(device), p.widths), sigmoid=sigmoid).cpu()


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=shape_id)
def test_logits_equal_the_fma_chain_bit_for_bit(device, shape):
    pooled, linears = random_tail(shape, seed=sum(shape))
    got = run(device, pooled, linears, sigmoid=False)
    assert tuple(got.shape) == (shape[0], shape[5]) and got.dtype == torch.float32
    assert_same_bits(got, torch.from_numpy(tail_logits(pooled.numpy(), [(W.numpy(), b.numpy()) for W, b in linears])))


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=shape_id)
def test_integer_data_is_exact(device, shape):
    """Small integers whose sums stay below 2^24 (asserted): the chain rounds nowhere, so the logits are the
    integer arithmetic's."""
    pooled, linears = random_tail(shape, seed=sum(shape) + 1, integers=True)
    v = pooled.double().mean(1)
    assert bool((v == v.round()).all())
    for k, (W, b) in enumerate(linears):
        assert float((v.abs() @ W.double().abs().t() + b.double().abs()).max()) < 2.0 ** 24
        v = v @ W.double().t() + b.double()
        if k < 2:
            v = v.clamp_min(0.0)
    got = run(device, pooled, linears, sigmoid=False)
    assert bool((got.double() == v).all()) and bool((v != 0).any())


# ----------------------------------------------------------------------------- every slot of the transposed layout
def _sel(out, inn, d):
    """W (out, in) with W[o][o + d] = 1 where that exists: the layer passes x[o + d] on to output o."""
    W = torch.zeros(out, inn)
    o = torch.arange(out)
    ok = (o + d >= 0) & (o + d < inn)
    W[o[ok], (o + d)[ok]] = 1.0
    return W


def _index(out, inn):
    """Positive f32 weights, each slot its own value."""
    W = 1.0 + (torch.arange(out).view(-1, 1) * inn + torch.arange(inn).view(1, -1)).double() * 2.0 ** -18
    assert W.unique().numel() == out * inn
    return W.float()


def _starts(width, n):
    return sorted({min(t, width - n) for t in range(0, width, n)})


@pytest.mark.parametrize("widths", ((64, 128, 64, 5), (256, 512, 256, 32)), ids=shape_id)
@pytest.mark.parametrize("layer", (1, 2, 3))
def test_one_hot_inputs_read_every_weight_slot(device, widths, layer):
    """Image m holds v_m in channel m of its one pixel and zeros elsewhere.  The layer under test has index
    weights and no bias, the other two pass selected entries on (weights 0 / 1, no bias: exact), so every logit
    is one product v_m W[o][i], rounded once, of a known slot; the launches together show every slot."""
    c0, c1, c2, n = widths
    g = torch.Generator().manual_seed(layer + sum(widths))
    v = 1.0 + torch.rand(c0, generator=g)
    pooled = torch.diag(v).view(c0, 1, c0)
    zeros = lambda k: torch.zeros(k)
    m, q = torch.arange(c0).view(-1, 1), torch.arange(n).view(1, -1)
    dims = {1: (c1, c0), 2: (c2, c1), 3: (n, c2)}[layer]
    Wx = _index(*dims)
    covered = torch.zeros(dims, dtype=torch.bool)
    if layer == 1:       # z[q] = x1[q + t]: W1[q + t][m]
        launches = [((Wx, _sel(c2, c1, t - min(t, c2 - n)), _sel(n, c2, min(t, c2 - n))), q + t + 0 * m, m + 0 * q)
                    for t in _starts(c1, n)]
    elif layer == 2:     # x1 hot at m + s, z[q] = x2[q + t]: W2[q + t][m + s]
        launches = [((_sel(c1, c0, -s), Wx, _sel(n, c2, t)), q + t + 0 * m, m + s + 0 * q)
                    for s in range(0, c1, c0) for t in _starts(c2, n)]
    else:                # x1 hot at m, x2 hot at m + s: W3[q][m + s]
        launches = [((_sel(c1, c0, 0), _sel(c2, c1, -s), Wx), q + 0 * m, m + s + 0 * q) for s in range(0, c2, min(c0, c1))]
    for (W1, W2, W3), o_idx, i_idx in launches:
        ok = i_idx < dims[1]
        if layer == 3:
            ok = ok & (m < c1)
        want = torch.where(ok, (Wx.double()[o_idx, i_idx.clamp_max(dims[1] - 1)] * v.double().view(-1, 1)).float(), torch.zeros(()))
        got = run(device, pooled, [(W1, zeros(c1)), (W2, zeros(c2)), (W3, zeros(n))], sigmoid=False)
        assert_same_bits(got, want)
        covered[o_idx[ok], i_idx[ok]] = True
    assert bool(covered.all()), f"{int((~covered).sum())} of {covered.numel()} slots of layer {layer} were never read"


# ----------------------------------------------------------------------------- non-finite values
def test_a_nan_stays_in_its_image(device):
    shape = (5, 6, 64, 128, 64, 5)
    pooled, linears = random_tail(shape, seed=3)
    clean = run(device, pooled, linears, sigmoid=True)
    dirty = pooled.clone()
    dirty[2, 4, 17] = float("nan")
    got = run(device, dirty, linears, sigmoid=True)
    assert bool(torch.isnan(got[2]).all())                        # every Linear is dense: the NaN reaches every output
    keep = [0, 1, 3, 4]
    assert_same_bits(got[keep], clean[keep])
    logits = run(device, dirty, linears, sigmoid=False)
    assert bool(torch.isnan(logits[2]).all()) and bool(torch.isfinite(logits[keep]).all())


# ----------------------------------------------------------------------------- the sigmoid
def test_sigmoid_against_float64_on_the_kernels_own_logits(device):
    """Logits spread over [-20, 20] (asserted): 1 / (1 + exp(-z)) in f32 against the float64 sigmoid of the very
    logits the kernel computed, within (e + 2) 2^-24 relative, e the documented error of the exp in ulps."""
    shape = (64, 2, 64, 64, 64, 32)
    pooled, linears = random_tail(shape, seed=9)
    (W3, _) = linears[2]
    linears[2] = (W3, torch.linspace(-20.0, 20.0, 32))
    z = run(device, pooled, linears, sigmoid=False)
    s = run(device, pooled, linears, sigmoid=True)
    assert float(z.min()) < -19.0 and float(z.max()) > 19.0 and z.unique().numel() > 1000
    hist = torch.histc(z.clamp(-20, 20), bins=8, min=-20, max=20)
    assert int(hist.min()) > 50                                   # every eighth of the range is populated
    ref = 1.0 / (1.0 + torch.exp(-z.double()))
    rel = ((s.double() - ref).abs() / ref)
    worst = float(rel.max())
    print(f"sigmoid: worst relative error {worst / 2.0 ** -24:.3f} x 2^-24, {worst / SIGMOID_BAR:.3f} of the bar "
          f"(at z = {float(z.flatten()[int(rel.argmax())]):.3f})")
    assert bool((s > 0).all()) and bool((s <= 1).all())
    assert worst <= SIGMOID_BAR


# ----------------------------------------------------------------------------- the C entry, the dispatcher
def test_c_entry_argument_errors_and_the_empty_batch(device):
    from mvn_rocm import _lib, confidence
    from mvn_rocm._ops import _stream
    shape = (5, 6, 64, 128, 64, 5)
    pooled, linears = random_tail(shape, seed=4)
    p = confidence.pack_confidence_tail(linears)
    x, pk = pooled.to(device), p.packed.to(device)
    out = torch.zeros(5 * 5 + 4, dtype=torch.float32, device=device)
    fn = _lib.load().mvn_confidence_tail
    ptr = lambda t: None if t is None else t.data_ptr()
    call = lambda x_, pk_, out_, M, hw, c0, c1, c2, n, act: fn(ptr(x_), ptr(pk_), ptr(out_), M, hw, c0, c1, c2, n, act, _stream(pk))
    ok = (x, pk, out, 5, 6, 64, 128, 64, 5, _lib.MVN_ACT_NONE)
    for i in range(3):                                               # a null pointer
        assert call(*(None if j == i else a for j, a in enumerate(ok))) == -1
    for name, args in dict(M=(x, pk, out, -1, 6, 64, 128, 64, 5, 0), hw=(x, pk, out, 5, 0, 64, 128, 64, 5, 0),
                           c0=(x, pk, out, 5, 6, 96, 128, 64, 5, 0), c1=(x, pk, out, 5, 6, 64, 576, 64, 5, 0),
                           c2=(x, pk, out, 5, 6, 64, 128, 32, 5, 0), n0=(x, pk, out, 5, 6, 64, 128, 64, 0, 0),
                           n33=(x, pk, out, 5, 6, 64, 128, 64, 33, 0), act=(x, pk, out, 5, 6, 64, 128, 64, 5, 2),
                           bytes=(x, pk, out, 2 ** 20, 8, 64, 128, 64, 5, 0)).items():
        assert call(*args) == -1, name
    torch.cuda.synchronize()
    assert not bool(out.any())                                       # refused before any launch
    assert call(x, pk, out, 0, 6, 64, 128, 64, 5, 0) == 0            # the empty batch: MVN_OK, no launch
    torch.cuda.synchronize()
    assert not bool(out.any())
    y = confidence.confidence_tail(x.view(5, 2, 3, 64)[:0], (pk, p.widths))
    assert tuple(y.shape) == (0, 5) and y.dtype == torch.float32
    assert call(*ok) == 0
    torch.cuda.synchronize()
    assert_same_bits(out[:25].view(5, 5), run(device, pooled, linears, sigmoid=False))
    assert not bool(out[25:].any())


def test_the_op_runs_through_the_dispatcher_and_replays_from_a_graph(device):
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import confidence
    shape = (3, 9, 256, 512, 256, 17)
    pooled, linears = random_tail(shape, seed=6)
    p = confidence.pack_confidence_tail(linears)
    x, pk = pooled.view(3, 3, 3, 256).to(device), p.packed.to(device)
    want = run(device, pooled, linears, sigmoid=True)
    assert_same_bits(torch.ops.mvn_rocm.confidence_tail(x, pk, 512, 256, 17, True), want)
    gm = make_fx(lambda x, pk: confidence.confidence_tail(x, (pk, p.widths)), tracing_mode="real")(x, pk)
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.confidence_tail.default) == 1
    assert_same_bits(gm(x, pk), want)
