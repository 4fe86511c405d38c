"""mvn_feature_conv / model.feature_conv (csrc/feature_conv.hip) on the MI355X:
the bit-exact contract (an ascending f32 fma chain from the bias), both load paths, every dtype pair,
the operand maps of the f32 MFMA, non-finite values, guard bands and the reference's recorded chain.

Shapes (n_images, Cin, H, W), the smallest at which the kernel can still go wrong:
  (1, 32, 1, 1)      one pixel
  (2, 32, 1, 3)      a row shorter than any vector; the second image only element-aligned
  (1, 64, 5, 7)      one full 32-pixel accumulator plus 3 pixels
  (3, 256, 17, 23)   the model's Cin, odd H*W: every image base and channel row misaligned; four 128-pixel tiles
  (2, 256, 8, 16)    the vector path, whole 128-pixel tiles only
  (1, 256, 16, 16)   H*W = Cin (the one-hot maps); two tiles
  (1, 512, 4, 8)     the largest Cin (64 KB of LDS); a quarter tile on the vector path
  (1, 256, 96, 96)   one image of the model's own shape (integer test only)
"""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_bits_equal, assert_parity_with_nans, max_rel
from test_feature_conv_api import fma_chain

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = list(itertools.product((F32, BF16), (F32, BF16)))
DT_IDS = [f"{'f32' if a is F32 else 'bf16'}-{'f32' if b is F32 else 'bf16'}" for a, b in DTYPES]
SHAPES = [(1, 32, 1, 1), (2, 32, 1, 3), (1, 64, 5, 7), (3, 256, 17, 23), (2, 256, 8, 16), (1, 256, 16, 16),
          (1, 512, 4, 8), (1, 256, 96, 96)]
CHAIN_SHAPES = [(2, 32, 1, 3), (1, 64, 5, 7), (3, 256, 17, 23), (2, 256, 8, 16)]
CODE = {F32: 0, BF16: 1}


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def bf16_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def assert_equal_out(got, ref32, out_dtype):
    """got (on the device) equals the f32 reference bit for bit, or its nearest-even bf16 rounding."""
    assert got.dtype == out_dtype and tuple(got.shape) == tuple(ref32.shape)
    if out_dtype is F32:
        assert_bits_equal(got.cpu().numpy(), ref32.numpy())
    else:
        g, r = bf16_bits(got), bf16_bits(ref32.bfloat16())
        bad = g != r
        assert not bad.any(), f"{int(bad.sum())} of {bad.size} bf16 elements differ in their bits"


def conv_cpu(x, w, b):
    """F.conv2d in f32 on the CPU of the values the kernel reads."""
    return F.conv2d(x.float(), w.float().view(32, -1, 1, 1), b)


def run(device, x, w, b, out_dtype):
    from mvn_rocm import model
    return model.feature_conv(x.to(device), w.to(device), b.to(device) if b is not None else None, out_dtype=out_dtype)


def integer_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, cin, H, W = shape
    return (torch.randint(-4, 5, shape, generator=g).float(), torch.randint(-4, 5, (32, cin), generator=g).float(),
            torch.randint(-4, 5, (32,), generator=g).float())


@functools.lru_cache(maxsize=None)
def random_case(shape, in_dtype):
    """Standard normal x (rounded to in_dtype), w / 16, normal b; the exact-fma chain and the float64
    sum of magnitudes S = |b| + sum |w x|, computed once per case."""
    g = torch.Generator().manual_seed(sum(shape) + (in_dtype is BF16))
    n, cin, H, W = shape
    x = torch.randn(shape, generator=g).to(in_dtype)
    w, b = torch.randn(32, cin, generator=g) / 16, torch.randn(32, generator=g)
    for t in (x.float(), w, b):                             # normal range: nothing flushes anywhere
        assert float(t.abs().min()) > 2.0 ** -60
    xs = x.float().numpy().reshape(n, cin, H * W)
    chain = torch.from_numpy(fma_chain(xs, w.numpy(), b.numpy()).reshape(n, 32, H, W))
    S = np.abs(b.double().numpy())[None, :, None] + np.einsum("oc,ncp->nop", np.abs(w.double().numpy()),
                                                               np.abs(xs.astype(np.float64)))
    return x, w, b, chain, S.reshape(n, 32, H, W)


# ---------------------------------------------------------------- 1. integers
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_integers_are_exact(device, shape, in_dtype, out_dtype):
    """x, w, b integers in [-4, 4]: every partial sum is exact in f32 in any order, so the result is
    F.conv2d's on the CPU bit for bit."""
    x, w, b = integer_case(shape, seed=shape[1] + shape[3])
    assert_equal_out(run(device, x.to(in_dtype), w, b, out_dtype), conv_cpu(x, w, b), out_dtype)


@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(3, 256, 17, 23), (2, 256, 8, 16)], ids=ids([(3, 256, 17, 23), (2, 256, 8, 16)]))
def test_element_aligned_pointers_take_the_element_path(device, shape, in_dtype, out_dtype):
    """A contiguous x whose data pointer is only element-aligned (a view from element 1 of a flat
    buffer), then the same for out through the C entry point: the same bits as the aligned call."""
    from mvn_rocm import _lib, model
    x, w, b = integer_case(shape, seed=3)
    n, cin, H, W = shape
    xd, wd, bd = x.to(in_dtype).to(device), w.to(device), b.to(device)
    want = model.feature_conv(xd, wd, bd, out_dtype=out_dtype)
    flat = torch.zeros(xd.numel() + 1, dtype=in_dtype, device=device)
    xo = flat[1:].view(shape)
    xo.copy_(xd)
    assert xo.is_contiguous() and xo.data_ptr() == flat.data_ptr() + xd.element_size()
    got = model.feature_conv(xo, wd, bd, out_dtype=out_dtype)
    assert torch.equal(got.view(torch.int32 if out_dtype is F32 else torch.int16),
                       want.view(torch.int32 if out_dtype is F32 else torch.int16))
    assert_equal_out(got, conv_cpu(x, w, b), out_dtype)
    # out one element into its buffer; the element before and the ones after keep their sentinel
    es = want.element_size()
    buf = torch.full((want.numel() + 2,), -7.0, dtype=out_dtype, device=device)
    code = _lib.load().mvn_feature_conv(xd.data_ptr(), CODE[in_dtype], wd.data_ptr(), bd.data_ptr(), buf.data_ptr() + es,
                                        CODE[out_dtype], n, cin, 32, H, W, torch.cuda.current_stream().cuda_stream)
    assert code == 0
    torch.cuda.synchronize()
    assert float(buf[0]) == -7.0 and float(buf[-1]) == -7.0
    assert torch.equal(buf[1:-1].view(want.shape), want)


# ---------------------------------------------------------------- 2. operand maps
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(1, 256, 16, 16), (1, 512, 4, 8)], ids=ids([(1, 256, 16, 16), (1, 512, 4, 8)]))
def test_one_hot_maps_read_every_weight_slot(device, shape, in_dtype, out_dtype):
    """w[co, ci] = co Cin + ci + 1 (asymmetric), x one-hot in channel (p + shift) mod Cin at pixel p, a
    distinct integer bias per channel: y[co, p] = w[co, (p + shift) mod Cin] + b[co].  The shifts
    cover every ci, so every (co, ci) slot of the A operand is read by some pixel."""
    n, cin, H, W = shape
    P = H * W
    w = (torch.arange(32)[:, None] * cin + torch.arange(cin)[None, :] + 1).float()
    b = (torch.arange(32) * 3 - 40).float()
    seen = torch.zeros(cin, dtype=torch.bool)
    for shift in range(0, cin, P):
        ch = (torch.arange(P) + shift) % cin
        seen[ch] = True
        x = torch.zeros(1, cin, P)
        x[0, ch, torch.arange(P)] = 1.0
        want = (w[:, ch] + b[:, None]).view(1, 32, H, W)
        assert_equal_out(run(device, x.view(shape).to(in_dtype), w, b, out_dtype), want, out_dtype)
    assert bool(seen.all())


@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(1, 256, 16, 16), (1, 512, 4, 8)], ids=ids([(1, 256, 16, 16), (1, 512, 4, 8)]))
def test_one_hot_weights_read_every_map_slot(device, shape, in_dtype, out_dtype):
    """The roles swapped: x[ci, p] = (7 ci + p) mod 251 (asymmetric, exact in bf16), w one-hot in
    channel (5 co + shift) mod Cin: y[co, p] = x[(5 co + shift) mod Cin, p] + b[co].  The shifts
    0, 16, ... over 32 rows stepping by 5 cover every ci, so every (ci, p) slot of the B operand is read."""
    n, cin, H, W = shape
    P = H * W
    x = ((7 * torch.arange(cin)[:, None] + torch.arange(P)[None, :]) % 251).float().view(1, cin, P)
    b = (torch.arange(32) * 3 - 40).float()
    seen = torch.zeros(cin, dtype=torch.bool)
    for shift in range(0, cin, 16):
        ch = (5 * torch.arange(32) + shift) % cin
        seen[ch] = True
        w = torch.zeros(32, cin)
        w[torch.arange(32), ch] = 1.0
        want = (x[0, ch] + b[:, None]).view(1, 32, H, W)
        assert_equal_out(run(device, x.view(shape).to(in_dtype), w, b, out_dtype), want, out_dtype)
    assert bool(seen.all())


# ---------------------------------------------------------------- 3. the chain, 4. the true semantics
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=ids(CHAIN_SHAPES))
def test_random_data_equal_the_fma_chain(device, shape, in_dtype, out_dtype):
    """The contract itself: acc = b[co], acc = fma(w[co, ci], x[ci, p], acc) for ci ascending, every
    fma correctly rounded (test_feature_conv_api.fma32); a bf16 result is its nearest-even rounding."""
    x, w, b, chain, _ = random_case(shape, in_dtype)
    assert_equal_out(run(device, x, w, b, out_dtype), chain, out_dtype)


@pytest.mark.parametrize("in_dtype", (F32, BF16), ids=("f32", "bf16"))
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=ids(CHAIN_SHAPES))
def test_random_data_against_torch(device, shape, in_dtype):
    """|y - F.conv2d (f32, CPU)| <= 2 Cin 2^-24 S with S = |b| + sum |w x| in float64: each side is
    within Cin 2^-24 S of the exact sum whatever its order of summation."""
    x, w, b, chain, S = random_case(shape, in_dtype)
    ref = conv_cpu(x, w, b).double().numpy()
    bar = 2 * shape[1] * 2.0 ** -24 * S
    got = run(device, x, w, b, F32).cpu().double().numpy()
    ratio = float((np.abs(got - ref) / bar).max())
    print(f"feature_conv vs torch at {shape} {in_dtype}: {ratio:.3f} of the bar, max-rel {max_rel(got, ref):.2e}; "
          f"the chain alone {float((np.abs(chain.double().numpy() - ref) / bar).max()):.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------- 5. non-finite values
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
def test_nonfinite_values_reach_their_own_pixel(device, in_dtype, out_dtype):
    """(1, 64, 5, 7): a NaN at one (ci, p) makes exactly the 32 outputs of p NaN; +inf gives +-inf by
    the weight's sign; inf times a zero weight gives NaN.  Integer data otherwise, so every other
    element is the CPU conv's bit for bit."""
    shape = (1, 64, 5, 7)
    x, w, b = integer_case(shape, seed=11)
    w[w == 0] = 1.0
    w[5, 9] = 0.0                                               # inf * 0 at (co 5, ci 9)
    x = x.view(1, 64, 35)
    x[0, 3, 33] = float("nan")                                  # the tile's tail
    x[0, 9, 2] = float("inf")
    x[0, 20, 17] = float("-inf")
    x = x.view(shape)
    ref = conv_cpu(x, w, b)
    r = ref.view(32, 35)
    assert bool(r[:, 33].isnan().all()) and int(r.isnan().sum()) == 32 + 1 and bool(r[5, 2].isnan())
    others = [co for co in range(32) if co != 5]
    assert bool((r[others, 2] == torch.sign(w[others, 9]) * float("inf")).all())
    assert bool((r[:, 17] == -torch.sign(w[:, 20]) * float("inf")).all())
    got = run(device, x.to(in_dtype), w, b, out_dtype)
    assert got.dtype == out_dtype
    want = ref if out_dtype is F32 else ref.bfloat16().float()
    assert_parity_with_nans(got.float().cpu().numpy(), want.numpy(), "sum")


# ---------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("in_dtype, out_dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(3, 256, 17, 23), (2, 32, 1, 3), (1, 512, 4, 8), (2, 256, 8, 16)],
                         ids=ids([(3, 256, 17, 23), (2, 32, 1, 3), (1, 512, 4, 8), (2, 256, 8, 16)]))
def test_guard_bands_stay_untouched(device, shape, in_dtype, out_dtype):
    """out is a window inside a larger buffer of a sentinel bit pattern, x a window between NaN
    bands: every byte outside out's window is unchanged, and nothing of x's bands reaches it.  The
    first two shapes take the element path, the last two the vector path (a quarter tile, whole tiles)."""
    from mvn_rocm import _lib
    n, cin, H, W = shape
    x, w, b = integer_case(shape, seed=5)
    band = 4096
    xb = torch.full((x.numel() + 2 * band,), float("nan"), dtype=in_dtype, device=device)
    xb[band:band + x.numel()] = x.to(in_dtype).flatten().to(device)
    ob = torch.full((n * 32 * H * W + 2 * band,), -1.5, dtype=out_dtype, device=device).view(torch.uint8)
    ob.fill_(0xA5)
    es_in, es_out = xb.element_size(), 4 if out_dtype is F32 else 2
    wd, bd = w.to(device), b.to(device)
    code = _lib.load().mvn_feature_conv(xb.data_ptr() + band * es_in, CODE[in_dtype], wd.data_ptr(), bd.data_ptr(),
                                        ob.data_ptr() + band * es_out, CODE[out_dtype], n, cin, 32, H, W,
                                        torch.cuda.current_stream().cuda_stream)
    assert code == 0
    torch.cuda.synchronize()
    lo, hi = band * es_out, (band + n * 32 * H * W) * es_out
    assert bool((ob[:lo] == 0xA5).all()) and bool((ob[hi:] == 0xA5).all())
    got = ob[lo:hi].view(out_dtype).view(n, 32, H, W)
    assert_equal_out(got, conv_cpu(x, w, b), out_dtype)


# ---------------------------------------------------------------- 7. small cases
def test_small_cases(device):
    from mvn_rocm import model
    shape = (3, 256, 17, 23)
    x, w, b, _, _ = random_case(shape, F32)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    for od in (F32, BF16):
        view = torch.int32 if od is F32 else torch.int16
        y1, y2 = model.feature_conv(xd, wd, bd, out_dtype=od), model.feature_conv(xd, wd, bd, out_dtype=od)
        assert torch.equal(y1.view(view), y2.view(view))                               # two calls, equal bits
        y5 = model.feature_conv(xd.view(1, 3, 256, 17, 23), wd.view(32, 256, 1, 1), bd, out_dtype=od)
        assert tuple(y5.shape) == (1, 3, 32, 17, 23) and torch.equal(y5.view(view).view(y1.shape), y1.view(view))
        y0 = model.feature_conv(xd, wd, None, out_dtype=od)
        assert torch.equal(y0.view(view), model.feature_conv(xd, wd, torch.zeros_like(bd), out_dtype=od).view(view))
        assert not torch.equal(y0.view(view), y1.view(view))
    assert model.feature_conv(xd, wd, bd).dtype == F32 and model.feature_conv(xd.bfloat16(), wd, bd).dtype == BF16
    e = model.feature_conv(xd[:0], wd, bd)
    assert tuple(e.shape) == (0, 32, 17, 23) and e.device == xd.device
    e = model.feature_conv(xd.view(1, 3, 256, 17, 23)[:, :0], wd, bd, out_dtype=BF16)
    assert tuple(e.shape) == (1, 0, 32, 17, 23) and e.dtype == BF16
    # a non-contiguous x is copied
    xt = xd.transpose(2, 3)
    assert not xt.is_contiguous()
    assert torch.equal(model.feature_conv(xt, wd, bd), model.feature_conv(xt.contiguous(), wd, bd))
    # a weight whose pointer is only element-aligned (the scalar staging of the LDS image)
    wf = torch.zeros(wd.numel() + 1, device=device)
    wo = wf[1:].view(32, 256)
    wo.copy_(wd)
    assert torch.equal(model.feature_conv(xd, wo, bd), model.feature_conv(xd, wd, bd))


# ---------------------------------------------------------------- 8. the reference's recorded chain
def test_reference_chain(device, golden):
    """tests/golden/chains.npz: vol_features in channels 0..31 of a 256-channel zero tensor through the
    pass-through weight and zero bias of make_golden.py:289-292 is vol_features bit for bit; its
    unprojection matches the recorded volume within the 1e-5 of test_gpu_configs.py."""
    from mvn_rocm import model, op, volumetric
    d = golden("chains.npz")
    f32 = torch.from_numpy(d["vol_features"])
    B, N, C, H, W = f32.shape
    feats = torch.zeros(B, N, 256, H, W)
    feats[:, :, :32] = f32
    w = torch.zeros(32, 256)
    w[torch.arange(32), torch.arange(32)] = 1.0
    got = model.feature_conv(feats.to(device), w.view(32, 256, 1, 1).to(device), torch.zeros(32, device=device))
    assert_bits_equal(got.cpu().numpy(), d["vol_features"])
    side, V = float(d["vol_side"]), d["vol_coords"].shape[1]
    cv = volumetric.build_coord_volumes(d["vol_base"], side, V, d["vol_thetas"], "mpii", False, device=device)
    vol = op.unproject_heatmaps(got, torch.from_numpy(d["vol_proj"]).to(device), cv, "softmax")
    sub = (slice(None), slice(None), slice(None, None, 4), slice(None, None, 4), slice(None, None, 4))
    assert max_rel(vol.cpu().numpy()[sub], d["vol_unprojected_sub"]) <= 1e-5
