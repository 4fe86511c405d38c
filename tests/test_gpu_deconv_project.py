"""mvn_deconv4s2_project on the GPU (csrc/deconv_head.hip): the head's last layer
with the 256 -> 32 projection in the same launch, against the contract of include/mvn_hip.h restated on
the CPU (tests/deconv_project_kit.py) and against the unfused pair of launches: data on which no order
of accumulation rounds bit for bit, every slot of the packed projection, random data within the
contract's bound, the borders and seams (tiles are 4 rows x 16 columns of input pixels), non-finite
pixels, guard bands, determinism, the wrapper's copy of a misaligned view and the empty batch."""
import functools

import pytest
import torch

from deconv_kit import (COUT, SMALL, DeconvCase, banded_out, cl2d, deconv, integer_case, parity_case, random_case,
                        shape_id)
from deconv_project_kit import (GAMMA, ROWS, abs_sum, exact_projection, index_projection, integer_projection, project64,
                                split)
from v2v_kit import BAND, assert_same_bits, banded, bits

pytestmark = pytest.mark.gpu

# SMALL: one pixel, sizes below a tile, more than one row tile, Cin = 2048; the added shape: the row
# seam 4 | 5, the column seam 16 | 17, the scalar store path and a clipped tile
SHAPES = SMALL + ((1, 32, 5, 17),)
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = ("f32", "bf16")


def want(ref32, dtype):
    return ref32 if dtype == torch.float32 else ref32.bfloat16()


def run(case, w, b, device, dtype, x_dev=None):
    from mvn_rocm import backbone
    xd = cl2d(case.x, device) if x_dev is None else x_dev
    return backbone.deconv4s2_project(xd, case.params(device), backbone.pack_projection(w, b, device=device), dtype)


def unfused(case, w, b, device, dtype, x_dev=None):
    """The parent's two launches: the NCHW bf16 map, then feature_conv."""
    from mvn_rocm import model
    a = case.run(device, "nchw", torch.bfloat16, x_dev)
    return model.feature_conv(a, w.to(device), b.to(device), out_dtype=dtype), a


@functools.lru_cache(maxsize=None)
def exact_case(shape):
    """(the deconv's integer case, the integer projection, the CPU value), computed once."""
    case, ref, _ = parity_case(shape)
    w, b = integer_projection(seed=5 + sum(shape))
    out32, _ = exact_projection(ref, w, b)
    return case, w, b, out32


# ----------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_exact_data_bit_equal_to_the_cpu_and_to_the_unfused_pair(device, shape):
    """Every term of every projection sum is a multiple of 1/4 and |bias| + the sum of |a w| is below
    2^22 (asserted on the CPU), so no order of accumulation rounds: the launch must return the bits of
    ``bias + sum bf16(ref) w``, and those of feature_conv on the NCHW bf16 map."""
    case, w, b, out32 = exact_case(shape)
    xd = cl2d(case.x, device)
    for dtype in DTYPES:
        got = run(case, w, b, device, dtype, xd)
        assert got.dtype == dtype and tuple(got.shape) == (shape[0], ROWS, 2 * shape[2], 2 * shape[3])
        assert_same_bits(got, want(out32, dtype))
        assert_same_bits(got, unfused(case, w, b, device, dtype, xd)[0])


# ----------------------------------------------------------------------------- every slot of the packed projection
def test_every_slot_of_the_packed_projection(device):
    """An identity deconv weight and 256 unit impulses, impulse k in channel k at every second pixel:
    each output pixel has one active channel or none (asserted: at most one product per output), so
    the f32 output is hi[p, k] + lo[p, k] in every impulse's 4 x 4 box and +0 elsewhere; with a weight
    that encodes its own (p, c) index in 16 significant bits (lo != 0) all 32 x 256 slots of both
    parts are read (asserted on the CPU)."""
    H = W = 32
    wd = torch.zeros(COUT, COUT, 4, 4)
    wd[torch.arange(COUT), torch.arange(COUT)] = 1.0
    ys, xs = torch.meshgrid(torch.arange(0, H, 2), torch.arange(0, W, 2), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    assert ys.numel() == COUT
    k = torch.arange(COUT)
    x = torch.zeros(1, COUT, H, W)
    x[0, k, ys, xs] = 1.0
    hits = deconv((x != 0).sum(1, keepdim=True).double(), torch.ones(1, 1, 4, 4, dtype=torch.float64))
    assert float(hits.max()) == 1.0
    case = DeconvCase(x, wd, torch.ones(COUT), torch.zeros(COUT))
    a, _ = case.reference()                                          # (1, 256, 64, 64): ones in the boxes
    assert bool(((a == 0) | (a == 1)).all()) and float(a.sum(1).max()) == 1.0
    assert bool((a.sum((0, 2, 3)) >= 9).all())                       # every channel is active somewhere
    w = index_projection()
    hi, lo = split(w)
    expect = torch.einsum("pc,mchw->mphw", hi + lo, a.double()).float()      # one term per output: exact
    active = a[0].sum(0) > 0
    read = torch.zeros(ROWS, COUT, dtype=torch.bool)
    ch = a[0].argmax(0)[active]
    read[:, ch] = True
    assert bool(read.all())
    assert bool((expect[0][:, active] == w[:, ch]).all()) and not bool(expect[0][:, ~active].any())
    got = run(case, w, torch.zeros(ROWS), device, torch.float32)
    assert_same_bits(got, expect)
    assert not bool(torch.signbit(got.cpu()[0][:, ~active]).any())   # +0 elsewhere


# ----------------------------------------------------------------------------- random data
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_random_data_within_the_contract_bound(device, shape):
    """a from the unfused NCHW bf16 launch (the same bits by the contract); ref = bias + sum a (hi + lo)
    in float64; bar gamma S (+ 2^-8 |ref| for a bf16 output), gamma = (2 256 + 4) 2^-24, S = |bias| +
    sum |a| (|hi| + |lo|); against the unsplit f32 weight the bar is wider by 2^-17 S.  The same sum in
    f32 on the CPU must sit at 0.05 of gamma S or below.  Measured: DESIGN.md §4.17."""
    case = random_case(shape, seed=sum(shape))
    g = torch.Generator().manual_seed(17 + sum(shape))
    w = torch.randn(ROWS, COUT, generator=g) * (2.0 / 288) ** 0.5
    b = 0.1 * torch.randn(ROWS, generator=g)
    assert bool((w.bfloat16().float() != w).any())
    hi, lo = split(w)
    xd = cl2d(case.x, device)
    _, a_dev = unfused(case, w, b, device, torch.float32, xd)
    a = a_dev.cpu().float()
    ref, S = project64(a, hi, lo, b), abs_sum(a, hi, lo, b)
    ref_w = torch.einsum("pc,mchw->mphw", w.double(), a.double()) + b.double().view(1, -1, 1, 1)
    cpu32 = torch.einsum("pc,mchw->mphw", (hi + lo).float(), a) + b.view(1, -1, 1, 1)
    cpu_frac = float(((cpu32.double() - ref).abs() / (GAMMA * S)).max())
    assert bool(((ref - ref_w).abs() <= 2.0 ** -17 * S).all())       # the split's own error
    for dtype in DTYPES:
        got = run(case, w, b, device, dtype, xd).cpu().double()
        half_ulp = 2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0
        frac = float(((got - ref).abs() / (GAMMA * S + half_ulp)).max())
        frac_w = float(((got - ref_w).abs() / (GAMMA * S + half_ulp + 2.0 ** -17 * S)).max())
        print(f"{shape_id(shape)} {dtype}: worst |got - ref| / bar = {frac:.4f}; against the unsplit weight {frac_w:.4f}; "
              f"the f32 CPU sum at {cpu_frac:.4f} of gamma S")
        assert cpu_frac <= 0.05, "the f32 CPU sum is not far inside gamma S: the bar is no bound for these inputs"
        assert frac <= 1.0
        assert frac_w <= 1.0


# ----------------------------------------------------------------------------- borders
@pytest.mark.parametrize("shape", ((1, 32, 1, 6), (1, 32, 6, 1), (1, 32, 2, 16), (1, 64, 2, 17), (1, 32, 3, 8),
                                   (1, 32, 3, 6)), ids=shape_id)
def test_borders_bit_equal(device, shape):
    """H = 1, W = 1, the image's edge on and next to the column seam (W = 16, 17), W % 4 zero (16-byte
    stores) and non-zero (single elements): exact data, the CPU value's bits."""
    case = integer_case(shape, seed=9 + shape[2] + 3 * shape[3])
    ref, _ = case.reference()
    w, b = integer_projection(seed=shape[3])
    out32, _ = exact_projection(ref, w, b)
    for dtype in DTYPES:
        assert_same_bits(run(case, w, b, device, dtype), want(out32, dtype))


# ----------------------------------------------------------------------------- non-finite pixels
H_NF, W_NF = 9, 20               # 3 row tiles (seams 3 | 4, 7 | 8), 2 column tiles (seam 15 | 16)
# (iy, ix, channel or None for all, value): a corner, either side of the row seam 3 | 4 and of the column
# seam 15 | 16; boxes pairwise disjoint (two pixels apart along an axis)
NF_PIXELS = ((0, 0, None, float("nan")), (8, 19, 7, float("inf")), (3, 4, 3, float("nan")), (4, 12, 17, float("-inf")),
             (3, 15, 5, float("inf")), (6, 16, 9, float("-inf")), (8, 0, 2, float("nan")), (0, 17, 30, float("inf")))


def box(iy, ix):
    return slice(max(2 * iy - 1, 0), min(2 * iy + 2, 2 * H_NF - 1) + 1), slice(max(2 * ix - 1, 0), min(2 * ix + 2, 2 * W_NF - 1) + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nonfinite_pixels_reach_exactly_their_boxes(device, dtype):
    """A NaN, +inf and -inf at single input pixels: every pixel of each clipped 4 x 4 box is non-finite
    in all 32 channels (the CPU asserts that each has a non-finite activation: the 256 channels' weights
    have both signs, so an infinity survives the ReLU somewhere); everything else equals the clean
    run bit for bit."""
    clean = integer_case((1, 32, H_NF, W_NF), seed=77)
    w, b = integer_projection(seed=78)
    x = clean.x.clone()
    inside = torch.zeros(2 * H_NF, 2 * W_NF, dtype=torch.bool)
    for iy, ix, ch, v in NF_PIXELS:
        bx = box(iy, ix)
        assert not bool(inside[bx].any()), "the test's boxes overlap"
        inside[bx] = True
        x[0, slice(None) if ch is None else ch, iy, ix] = v
    case = DeconvCase(x, clean.w, clean.scale, clean.shift)
    r = deconv(x, clean.w).double() * clean.scale.double().view(1, -1, 1, 1) + clean.shift.double().view(1, -1, 1, 1)
    a = torch.where(r <= 0, torch.zeros_like(r), r)
    bad = ~torch.isfinite(a[0])
    assert bool((bad.any(0) == inside).all())                        # a non-finite activation in every box pixel, none outside
    got_clean = run(clean, w, b, device, dtype).cpu()
    got = run(case, w, b, device, dtype).cpu()
    assert bool(torch.isfinite(got_clean.float()).all())
    assert not bool(torch.isfinite(got.float()[0][:, inside]).any())
    assert (bits(got)[0][:, ~inside.numpy()] == bits(got_clean)[0][:, ~inside.numpy()]).all()


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", ((2, 32, 3, 5), (1, 64, 5, 7), (2, 256, 12, 12), (1, 32, 5, 17)), ids=shape_id)
def test_no_reads_or_writes_outside_the_tensors(device, shape, dtype):
    """NaN bands around x, sentinel bands and a sentinel fill around out (C entry, caller's buffers)."""
    from mvn_rocm import _lib, backbone
    from mvn_rocm._ops import _stream
    M, cin, H, W = shape
    case, w, b, out32 = exact_case(shape)
    big_x, xin = banded(cl2d(case.x, device))
    big_o, out, sentinel = banded_out((M, ROWS, 2 * H, 2 * W), dtype, device)
    pk, sc, sh = case.params(device)
    pr = backbone.pack_projection(w, b, device=device)
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = _lib.load().mvn_deconv4s2_project(xin.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                             pr.packed.data_ptr(), pr.bias.data_ptr(), out.data_ptr(),
                                             _lib.MVN_DTYPE_BF16 if dtype == torch.bfloat16 else _lib.MVN_DTYPE_F32, M,
                                             cin, H, W, _stream(xin))
    _lib.check(code, "mvn_deconv4s2_project")
    torch.cuda.synchronize()
    n = out.numel()
    assert bool((big_o[:BAND] == sentinel).all()) and bool((big_o[BAND + n:] == sentinel).all())
    assert not bool((big_o[BAND:BAND + n] == sentinel).any())
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(out, want(out32, dtype))


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_same_bits_on_every_run_and_for_every_batch(device, dtype):
    """Random data (sums that round): two runs agree, and image 0 of M = 2 equals the image run alone."""
    case = random_case((2, 256, 12, 12), seed=11)
    g = torch.Generator().manual_seed(12)
    w, b = torch.randn(ROWS, COUT, generator=g) * (2.0 / 288) ** 0.5, 0.1 * torch.randn(ROWS, generator=g)
    xd = cl2d(case.x, device)
    y1, y2 = run(case, w, b, device, dtype, xd), run(case, w, b, device, dtype, xd)
    assert_same_bits(y1, y2)
    alone = run(case, w, b, device, dtype, xd[:1].contiguous())
    assert_same_bits(y1[:1], alone)


# ----------------------------------------------------------------------------- misaligned views, empty batch
def test_a_misaligned_view_equals_the_aligned_call(device):
    """The C entry takes 16-byte aligned pointers only; the wrapper copies a view at an odd element offset."""
    from mvn_rocm import _lib, backbone
    from mvn_rocm._ops import _stream
    shape = (2, 32, 3, 5)
    case, w, b, out32 = exact_case(shape)
    xd, params = cl2d(case.x, device), case.params(device)
    pr = backbone.pack_projection(w, b, device=device)
    buf = torch.zeros(xd.numel() + 8, dtype=torch.bfloat16, device=device)
    odd = buf[1:1 + xd.numel()].view(xd.shape)
    odd.copy_(xd)
    assert odd.data_ptr() % 16 == 2
    bias_buf = torch.zeros(ROWS + 4, device=device)
    odd_bias = bias_buf[1:1 + ROWS]
    odd_bias.copy_(pr.bias)
    assert odd_bias.data_ptr() % 16 == 4
    for dtype in DTYPES:
        assert_same_bits(backbone.deconv4s2_project(odd, params, (pr.packed, odd_bias), dtype), want(out32, dtype))
    out = torch.zeros(2 * ROWS * 6 * 10 + 8, dtype=torch.bfloat16, device=device)
    args = dict(x=xd.data_ptr(), bias=pr.bias.data_ptr(), out=out.data_ptr())
    for name, ptr in (("x", odd.data_ptr()), ("bias", odd_bias.data_ptr()), ("out", out[1:].data_ptr())):
        k = dict(args, **{name: ptr})
        code = _lib.load().mvn_deconv4s2_project(k["x"], params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(),
                                                 pr.packed.data_ptr(), k["bias"], k["out"], _lib.MVN_DTYPE_BF16, 2, 32, 3, 5,
                                                 _stream(xd))
        assert code == -1
    torch.cuda.synchronize()
    assert not bool(out.any())                                           # refused before any launch


def test_empty_batch(device):
    from mvn_rocm import backbone
    case, w, b, _ = exact_case((2, 32, 3, 5))
    x = torch.zeros(0, 3, 5, 32, dtype=torch.bfloat16, device=device)
    pr = backbone.pack_projection(w, b, device=device)
    y = backbone.deconv4s2_project(x, case.params(device), pr)
    assert tuple(y.shape) == (0, ROWS, 6, 10) and y.dtype == torch.bfloat16
    y = backbone.deconv4s2_project(x, case.params(device), pr, torch.float32)
    assert tuple(y.shape) == (0, ROWS, 6, 10) and y.dtype == torch.float32
