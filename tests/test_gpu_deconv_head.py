"""mvn_deconv4s2 on the GPU (csrc/deconv_head.hip) against
``F.conv_transpose2d(stride=2, padding=1)`` on the CPU: operands for which the kernel's f32
arithmetic is exact in any order (integers, impulse lattices) bit for bit, random data within the
contract's own bound, the borders, non-finite pixels either side of every tile seam (tiles are
4 rows x 16 columns of input pixels), guard bands, the agreement of the three outputs, the
wrapper's copy of a misaligned view, determinism and the empty batch."""
import pytest
import torch

from deconv_kit import (COUT, SHAPES, SMALL, DeconvCase, banded_out, check_bound, cl2d, deconv, index_weight,
                        integer_case, nchw, parity_case, random_case, shape_id)
from v2v_kit import BAND, assert_same_bits, banded, bf16_full, bits

LAYOUTS = (("cl", torch.bfloat16), ("nchw", torch.bfloat16), ("nchw", torch.float32))
LAYOUT_IDS = ("cl", "nchw_bf16", "nchw_f32")


def as_nchw(y, layout):
    return nchw(y) if layout == "cl" else y.cpu()


def want(ref32, dtype):
    return ref32 if dtype == torch.float32 else ref32.bfloat16()


# ----------------------------------------------------------------------------- integer data
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_integer_data_bit_equal_to_the_cpu_deconv(device, shape):
    """Every sum is exact in f32 (asserted: the sum of |x w| is below 2^24), so the kernel must return
    the CPU deconv's bits in both layouts and both NCHW dtypes."""
    case, ref, _ = parity_case(shape)
    xd, params = cl2d(case.x, device), case.params(device)
    from mvn_rocm import backbone
    for layout, dtype in LAYOUTS:
        got = backbone.deconv4s2(xd, params, layout, dtype)
        assert got.dtype == dtype
        assert_same_bits(as_nchw(got, layout), want(ref, dtype))


# ----------------------------------------------------------------------------- impulse lattices
def lattice_launches(cin, M, H, W, rounds, g):
    """Impulses at every second pixel of both axes (the 4 x 4 output boxes of two input pixels two
    apart are disjoint), four offsets per round, one channel each, channels counted on across the
    launches; full-significand bf16 values."""
    k = 0
    for _ in range(rounds):
        for oy in (0, 1):
            for ox in (0, 1):
                ys, xs = torch.arange(oy, H, 2), torch.arange(ox, W, 2)
                if ys.numel() == 0 or xs.numel() == 0:
                    continue
                mm, yy, xx = (t.reshape(-1) for t in torch.meshgrid(torch.arange(M), ys, xs, indexing="ij"))
                n = mm.numel()
                ch = (k + torch.arange(n)) % cin
                k += n
                yield mm, yy, xx, ch, bf16_full((n,), g)


@pytest.mark.gpu
@pytest.mark.parametrize("cin, M, H, W, rounds", [(32, 2, 5, 7, 3), (64, 1, 9, 18, 3), (256, 2, 12, 12, 4),
                                                  (2048, 2, 34, 35, 3)], ids=lambda v: str(v))
def test_impulse_lattices_read_every_weight_slot(device, cin, M, H, W, rounds):
    """At most one product per output (asserted), so the output IS that product times the scale,
    rounded once; with a weight that encodes its own index the launches together must read every
    (ci, co, ky, kx) slot (asserted on the CPU: every (ci, ky, kx) is hit by an unclipped tap, and
    every impulse reaches all 256 co) and write every parity."""
    from mvn_rocm import backbone
    g = torch.Generator().manual_seed(cin + H)
    w = index_weight(cin)
    scale = 0.75 + 0.5 * torch.rand(COUT, generator=g)
    scale = scale * torch.where(torch.arange(COUT) % 3 == 1, -1.0, 1.0)
    params = DeconvCase(torch.zeros(1, cin, 1, 1), w, scale, torch.zeros(COUT)).params(device)
    covered = torch.zeros(cin, 4, 4, dtype=torch.bool)
    parities = set()
    for mm, yy, xx, ch, val in lattice_launches(cin, M, H, W, rounds, g):
        x = torch.zeros(M, cin, H, W)
        x[mm, ch, yy, xx] = val
        hits = deconv((x != 0).sum(1, keepdim=True).double(), torch.ones(1, 1, 4, 4, dtype=torch.float64))
        assert float(hits.max()) == 1.0
        acc = torch.zeros(M, COUT, 2 * H, 2 * W, dtype=torch.float64)
        for ky in range(4):
            for kx in range(4):
                oy, ox = 2 * yy - 1 + ky, 2 * xx - 1 + kx
                ok = (oy >= 0) & (oy < 2 * H) & (ox >= 0) & (ox < 2 * W)
                acc[mm[ok], :, oy[ok], ox[ok]] = val[ok].double()[:, None] * w[ch[ok], :, ky, kx].double()
                covered[ch[ok], ky, kx] = True
                parities |= set(zip((oy[ok] % 2).tolist(), (ox[ok] % 2).tolist()))
        assert int((acc != 0).sum()) == int(hits.sum()) * COUT
        r = (acc * scale.double().view(1, -1, 1, 1)).float()
        ref = torch.where(r <= 0, torch.zeros_like(r), r)
        xd = cl2d(x, device)
        assert_same_bits(nchw(backbone.deconv4s2(xd, params, "cl")), ref.bfloat16())
        assert_same_bits(backbone.deconv4s2(xd, params, "nchw", torch.float32).cpu(), ref)
    assert bool(covered.all()), f"{int((~covered).sum())} (ci, ky, kx) slots were never read"
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ----------------------------------------------------------------------------- random data
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL, ids=shape_id)
def test_random_data_within_the_contract_bound(device, shape):
    case = random_case(shape, seed=sum(shape))
    xd, params = cl2d(case.x, device), case.params(device)
    from mvn_rocm import backbone
    check_bound(case, nchw(backbone.deconv4s2(xd, params, "cl")).float(), f"{shape_id(shape)} cl")
    check_bound(case, backbone.deconv4s2(xd, params, "nchw", torch.bfloat16).cpu().float(), f"{shape_id(shape)} nchw bf16")
    check_bound(case, backbone.deconv4s2(xd, params, "nchw", torch.float32).cpu(), f"{shape_id(shape)} nchw f32",
                f32_out=True)


# ----------------------------------------------------------------------------- borders
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((2, 32, 1, 1), (1, 32, 1, 6), (1, 32, 6, 1), (1, 64, 2, 17), (1, 32, 5, 16)),
                         ids=shape_id)
def test_borders_take_one_or_two_taps(device, shape):
    """Rows and columns 0 and 2H - 1 / 2W - 1 have one tap along their axis: with all-positive
    operands their sums are strictly smaller than a full 2 x 2 sum could be, and equal to the CPU
    deconv's.  H = 1 and W = 1 have every output on a border.  Column tiles end at 16: W = 16 and
    17 put the image's edge on and next to the seam."""
    M, cin, H, W = shape
    g = torch.Generator().manual_seed(7 + H + W)
    x = torch.randint(1, 5, (M, cin, H, W), generator=g).float()
    w = torch.randint(1, 5, (cin, COUT, 4, 4), generator=g).float()
    case = DeconvCase(x, w, torch.ones(COUT), torch.zeros(COUT))
    ref, _ = case.reference()
    taps = deconv(torch.ones(1, 1, H, W), torch.ones(1, 1, 4, 4))[0, 0]
    assert taps[0, 0] == 1 and taps[-1, -1] == 1 and float(taps.max()) == min(2, H) * min(2, W)
    for layout, dtype in LAYOUTS:
        got = as_nchw(case.run(device, layout, dtype), layout)
        for sl in ((..., 0, slice(None)), (..., -1, slice(None)), (..., slice(None), 0), (..., slice(None), -1)):
            assert_same_bits(got[sl], want(ref, dtype)[sl])
        assert_same_bits(got, want(ref, dtype))


# ----------------------------------------------------------------------------- non-finite pixels
H_NF, W_NF = 9, 20               # 3 row tiles (seams 3 | 4, 7 | 8), 2 column tiles (seam 15 | 16)
# (iy, ix, channel or None for all, value): boxes pairwise disjoint (two pixels apart along an axis)
NF_PIXELS = ((0, 0, None, float("nan")), (8, 19, None, float("nan")), (3, 4, 3, float("nan")),
             (4, 12, 17, float("nan")), (3, 15, 5, float("inf")), (6, 16, 9, float("-inf")),
             (5, 1, 0, float("inf")), (8, 4, 11, float("nan")), (0, 19, 30, float("inf")), (8, 0, 2, float("-inf")))
ZERO_W_CHANNEL = 0               # w[0] is zero at one tap: the +inf of pixel (5, 1) meets it as inf * 0


def box(iy, ix):
    return slice(max(2 * iy - 1, 0), min(2 * iy + 2, 2 * H_NF - 1) + 1), slice(max(2 * ix - 1, 0), min(2 * ix + 2, 2 * W_NF - 1) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout, dtype", LAYOUTS, ids=LAYOUT_IDS)
def test_nonfinite_pixels_reach_exactly_their_boxes(device, layout, dtype):
    """A NaN, +inf, -inf and inf * 0 at single input pixels, in the corners and either side of every
    tile seam: outside the clipped 4 x 4 boxes the output equals the clean run's, bit for bit; inside,
    it follows the CPU deconv (NaN where it has NaN, its bits elsewhere); a NaN pixel fills its box."""
    clean = integer_case((1, 32, H_NF, W_NF), seed=77)
    clean.w[ZERO_W_CHANNEL, :, 2, 1] = 0.0
    x = clean.x.clone()
    inside = torch.zeros(2 * H_NF, 2 * W_NF, dtype=torch.bool)
    for iy, ix, ch, v in NF_PIXELS:
        b = box(iy, ix)
        assert not bool(inside[b].any()), "the test's boxes overlap"
        inside[b] = True
        x[0, slice(None) if ch is None else ch, iy, ix] = v
    case = DeconvCase(x, clean.w, clean.scale, clean.shift)
    ref_clean, _ = clean.reference()
    r = deconv(x, clean.w).double() * clean.scale.double().view(1, -1, 1, 1) + clean.shift.double().view(1, -1, 1, 1)
    ref = torch.where(r <= 0, torch.zeros_like(r), r).float()
    assert bool(torch.isnan(ref[0, :, 11, 2]).all())                     # inf * 0 at tap (ky, kx) = (2, 1) of pixel (5, 1)
    got = as_nchw(case.run(device, layout, dtype), layout)
    assert_same_bits(got[..., ~inside], want(ref_clean, dtype)[..., ~inside])
    nan = torch.isnan(ref)
    assert bool((torch.isnan(got.float()) == nan).all())
    assert not bool(nan[..., ~inside].any())
    assert (bits(got)[~nan.numpy()] == bits(want(ref, dtype))[~nan.numpy()]).all()
    for iy, ix, ch, v in NF_PIXELS:
        if v != v:
            assert bool(torch.isnan(got.float()[0][(slice(None),) + box(iy, ix)]).all())


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.gpu
@pytest.mark.parametrize("layout, dtype", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", ((2, 32, 3, 5), (1, 64, 5, 7), (2, 256, 12, 12)), ids=shape_id)
def test_no_reads_or_writes_outside_the_tensors(device, shape, layout, dtype):
    """NaN bands around x, sentinel bands and a sentinel fill around out (C entry, caller's buffers):
    a read outside x would put a NaN into the result, a write outside out would break a band, and an
    unwritten element would keep the sentinel."""
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    M, cin, H, W = shape
    case, ref, _ = parity_case(shape)
    big_x, xin = banded(cl2d(case.x, device))
    oshape = (M, 2 * H, 2 * W, COUT) if layout == "cl" else (M, COUT, 2 * H, 2 * W)
    big_o, out, sentinel = banded_out(oshape, dtype, device)
    pk, sc, sh = case.params(device)
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = _lib.load().mvn_deconv4s2(xin.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(),
                                     _lib.MVN_LAYOUT_NHWC if layout == "cl" else _lib.MVN_LAYOUT_NCHW,
                                     _lib.MVN_DTYPE_BF16 if dtype == torch.bfloat16 else _lib.MVN_DTYPE_F32, M, cin, H, W,
                                     _stream(xin))
    _lib.check(code, "mvn_deconv4s2")
    torch.cuda.synchronize()
    n = out.numel()
    assert bool((big_o[:BAND] == sentinel).all()) and bool((big_o[BAND + n:] == sentinel).all())
    assert not bool((big_o[BAND:BAND + n] == sentinel).any())
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(as_nchw(out, layout), want(ref, dtype))


# ----------------------------------------------------------------------------- the three outputs agree
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_layouts_agree_bit_for_bit(device, shape):
    """Random data (sums that round): channels-last == NCHW bf16 after the permute, and NCHW f32
    rounded to bf16 == NCHW bf16."""
    case = random_case(shape, seed=3 + sum(shape))
    xd, params = cl2d(case.x, device), case.params(device)
    from mvn_rocm import backbone
    y_cl = backbone.deconv4s2(xd, params, "cl")
    y_bf = backbone.deconv4s2(xd, params, "nchw", torch.bfloat16)
    y_f32 = backbone.deconv4s2(xd, params, "nchw", torch.float32)
    assert_same_bits(nchw(y_cl), y_bf.cpu())
    assert_same_bits(y_f32.bfloat16().cpu(), y_bf.cpu())
    assert bool((y_f32.cpu() != y_bf.cpu().float()).any())               # the f32 result does hold more bits


# ----------------------------------------------------------------------------- misaligned views
@pytest.mark.gpu
def test_a_misaligned_view_equals_the_aligned_call(device):
    """The C entry takes 16-byte aligned pointers only (MVN_ERR_ARG otherwise, tests/test_deconv_head_api.py):
    the kernel has no element-aligned path.  The wrapper copies a view at an odd element offset."""
    from mvn_rocm import _lib, backbone
    from mvn_rocm._ops import _stream
    shape = (2, 32, 3, 5)
    case, ref, _ = parity_case(shape)
    xd, params = cl2d(case.x, device), case.params(device)
    buf = torch.zeros(xd.numel() + 8, dtype=torch.bfloat16, device=device)
    odd = buf[1:1 + xd.numel()].view(xd.shape)
    odd.copy_(xd)
    assert odd.data_ptr() % 16 == 2
    for layout, dtype in LAYOUTS:
        assert_same_bits(as_nchw(backbone.deconv4s2(odd, params, layout, dtype), layout), want(ref, dtype))
    out = torch.zeros(2 * 6 * 10 * COUT + 8, dtype=torch.bfloat16, device=device)
    code = _lib.load().mvn_deconv4s2(odd.data_ptr(), params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(),
                                     out.data_ptr(), _lib.MVN_LAYOUT_NHWC, _lib.MVN_DTYPE_BF16, 2, 32, 3, 5, _stream(xd))
    assert code == -1
    code = _lib.load().mvn_deconv4s2(xd.data_ptr(), params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(),
                                     out[1:].data_ptr(), _lib.MVN_LAYOUT_NHWC, _lib.MVN_DTYPE_BF16, 2, 32, 3, 5, _stream(xd))
    assert code == -1
    torch.cuda.synchronize()
    assert not bool(out.any())                                           # refused before any launch


# ----------------------------------------------------------------------------- determinism, empty batch
@pytest.mark.gpu
@pytest.mark.parametrize("layout, dtype", LAYOUTS, ids=LAYOUT_IDS)
def test_two_runs_give_the_same_bits(device, layout, dtype):
    case = random_case((2, 256, 12, 12), seed=11)
    xd = cl2d(case.x, device)
    a, b = case.run(device, layout, dtype, xd), case.run(device, layout, dtype, xd)
    assert_same_bits(a, b)


@pytest.mark.gpu
def test_empty_batch(device):
    from mvn_rocm import backbone
    case, _, _ = parity_case((2, 32, 3, 5))
    params = case.params(device)
    x = torch.zeros(0, 3, 5, 32, dtype=torch.bfloat16, device=device)
    y = backbone.deconv4s2(x, params)
    assert tuple(y.shape) == (0, 6, 10, COUT) and y.dtype == torch.bfloat16
    y = backbone.deconv4s2(x, params, "nchw", torch.float32)
    assert tuple(y.shape) == (0, COUT, 6, 10) and y.dtype == torch.float32
