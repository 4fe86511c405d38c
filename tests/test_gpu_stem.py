"""mvn_stem on the GPU (csrc/stem.hip) against ``F.conv2d`` and ``F.max_pool2d`` on the CPU:
operands for which the kernel's f32 arithmetic is exact in any order (integers, impulses) bit for bit, random
data within the contract's own bound, the rounding of f32 images, non-finite pixels in the corners, either
side of every tile seam (tests/stem_kit.py: the block seam 7 | 8 and the fragment seams 16 k - 1 | 16 k) and in
the interior, guard bands, determinism, odd element offsets and the empty batch."""
import pytest
import torch

from deconv_kit import nchw
from stem_kit import (CIN, COUT, DTYPE_IDS, DTYPES, INTERIOR_SHAPE, KS, SEAM_SHAPE, SHAPES, TILE, StemCase, check_bound,
                      conv7, fragment_seam_pixels, index_weight, integer_case, out_hw, parity_case, pool3, random_case,
                      relu64, shape_id)
from v2v_kit import BAND, SENTINEL, assert_same_bits, banded, bf16_full, bits

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- integer data
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_integer_data_bit_equal_to_the_cpu(device, shape, dtype):
    """Every sum is exact in f32 (asserted: the sum of |x w| is at most 147 * 16 < 2^24), so the kernel must
    return the CPU restatement's bits, from f32 and from bf16 images."""
    case, ref = parity_case(shape)
    got = case.run(device, dtype)
    M, H, W = shape
    assert tuple(got.shape) == (M, *out_hw(H, W)[2:], COUT) and got.dtype == torch.bfloat16
    assert_same_bits(nchw(got), ref)


def test_pad_slots_carry_nothing_whatever_they_hold(device):
    """The K-slots 24 ky + 21 .. 23 lie on the pixel right of the footprint and 168 .. 191 on more of the last
    tap row: with ones in every pad slot of the packed weight, dense integer images still give the reference's
    bits, because the kernel clears the pixel operand there."""
    from mvn_rocm import resnet
    case, ref = parity_case(SEAM_SHAPE)
    packed = resnet.pack_stem_weight(case.w.double())
    pads = resnet.pack_stem_weight(torch.ones(COUT, CIN, KS, KS, dtype=torch.float64)) == 0
    assert int(pads.sum()) == COUT * (192 - 147)
    dirty = torch.where(pads, torch.ones_like(packed), packed)
    assert_same_bits(nchw(case.run(device, packed=dirty.to(device))), ref)


# ----------------------------------------------------------------------------- index weight, impulses
def _lattice(M, H, W, oy, ox, rot, g):
    """Impulses eleven apart in both axes from (oy, ox): the 11 x 11 input pixels under the 3 x 3 convolution
    pixels of a pool window hold one at the most.  One channel each, counted on along the lattice from ``rot``."""
    ys, xs = torch.arange(oy, H, 11), torch.arange(ox, W, 11)
    mm, yy, xx = (t.reshape(-1) for t in torch.meshgrid(torch.arange(M), ys, xs, indexing="ij"))
    ch = (rot + mm + (yy // 11) * 2 + (xx // 11)) % CIN
    return mm, yy, xx, ch, bf16_full((mm.numel(),), g).abs()


OFFSETS = ((0, 0), (4, 7))


def test_impulses_read_every_weight_slot(device):
    """Impulses on a lattice give at most one product per convolution output and one impulse per pool window
    (asserted).  The weight encodes its own (co, ci, ky, kx) and is masked to the taps with (ky >> 1) % 3 == ry
    and (kx >> 1) % 3 == rx: the three convolution rows of a pool window see the impulse through taps ky, ky - 2,
    ky - 4, so a window holds one non-zero product per channel at the most (asserted) and the pooled output IS that product times the
    (positive) scale, rounded once: bit-equal to the CPU.  Over the nine masks, three channel rotations and two
    lattices every one of the 64 * 147 slots gives an output (asserted on the CPU: every (ci, ky, kx) is met by
    an unclipped tap under the mask that keeps it, in all 64 rows), and every output element is written
    non-zero in some launch (asserted)."""
    M, H, W = 2, 37, 51
    Hc, Wc, Hp, Wp = out_hw(H, W)
    g = torch.Generator().manual_seed(5)
    w = index_weight()
    scale = 0.75 + 0.5 * torch.rand(COUT, generator=g)
    covered = torch.zeros(CIN, KS, KS, dtype=torch.bool)
    written = torch.zeros(M, COUT, Hp, Wp, dtype=torch.bool)
    taps = torch.arange(KS)
    for (oy, ox) in OFFSETS:
        for rot in range(CIN):
            mm, yy, xx, ch, val = _lattice(M, H, W, oy, ox, rot, g)
            x = torch.zeros(M, CIN, H, W)
            x[mm, ch, yy, xx] = val
            hits = conv7((x != 0).sum(1, keepdim=True).double(), torch.ones(1, 1, KS, KS, dtype=torch.float64))
            assert float(hits.max()) == 1.0
            for ry in range(3):
                for rx in range(3):
                    keep = (((taps >> 1) % 3 == ry).view(-1, 1) & ((taps >> 1) % 3 == rx).view(1, -1))
                    wm = w * keep.view(1, 1, KS, KS)
                    acc = conv7(x.double(), wm.double())          # one product per output: exact
                    a = relu64((acc * scale.double().view(1, -1, 1, 1)).float())
                    in_window = torch.nn.functional.avg_pool2d((a != 0).double(), 3, 2, 1, count_include_pad=True) * 9
                    assert float(in_window.max()) <= 1.0 + 1e-9
                    ref = pool3(a).bfloat16()
                    written |= ref != 0
                    for ky in taps[(taps >> 1) % 3 == ry].tolist():
                        for kx in taps[(taps >> 1) % 3 == rx].tolist():
                            ny, nx = yy + 3 - ky, xx + 3 - kx    # 2 (cy, cx)
                            ok = (ny >= 0) & (nx >= 0) & (ny % 2 == 0) & (nx % 2 == 0) & (ny // 2 < Hc) & (nx // 2 < Wc)
                            covered[ch[ok], ky, kx] = True
                    case = StemCase(x, wm, scale, torch.zeros(COUT))
                    assert_same_bits(nchw(case.run(device)), ref)
    assert bool(covered.all()), f"{int((~covered).sum())} (ci, ky, kx) slots are never read"
    assert bool(written.all())


# ----------------------------------------------------------------------------- random data
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_random_data_within_the_contract_bound(device, shape, dtype):
    case = random_case(shape, seed=sum(shape))
    check_bound(case, nchw(case.run(device, dtype)).float(), f"stem {shape_id(shape)} {dtype}")


@pytest.mark.parametrize("shape", ((2, 37, 51), SEAM_SHAPE), ids=shape_id)
def test_f32_images_are_rounded_once_to_bf16(device, shape):
    """f32 images with their low mantissa bits set (ties and near-ties among them) give the bits of the same
    images rounded to bf16 on the host, nearest-even, and passed as bf16."""
    case = random_case(shape, seed=21, exact_inputs=False)
    x = case.x.clone()
    flat = x.view(-1).view(torch.int32)
    flat[0::5] = (flat[0::5] & ~0xFFFF) | 0x8000                  # exact ties: to even
    flat[1::5] |= 0x7FFF                                          # just below a tie
    flat[2::5] = (flat[2::5] & ~0xFFFF) | 0x8001                  # just above
    assert not bool((x.bfloat16().float() == x).all())
    case = StemCase(x, case.w, case.scale, case.shift)
    assert_same_bits(case.run(device, torch.float32), case.run(device, images=x.bfloat16().to(device)))
    check_bound(case, nchw(case.run(device)).float(), f"stem {shape_id(shape)} unrounded f32")


# ----------------------------------------------------------------------------- non-finite values
NAN, INF = float("nan"), float("inf")
ZERO_W = (0, 3, 3)               # w[:, 0, 3, 3] is zero: an inf in channel 0 meets it at the centre tap as inf * 0


def _footprint(H, W, y, x):
    """(Hp, Wp) bool: the pooled outputs that input pixel (y, x) reaches, by the contract's formula."""
    Hc, Wc, Hp, Wp = out_hw(H, W)

    def axis(n_c, n_p, v):
        hit = torch.zeros(n_p, dtype=torch.bool)
        for p in range(n_p):
            hit[p] = any(0 <= c < n_c and abs(2 * c - v) <= 3 for c in (2 * p - 1, 2 * p, 2 * p + 1))
        return hit
    return axis(Hc, Hp, y).view(-1, 1) & axis(Wc, Wp, x).view(1, -1)


def _seam_pixels(H, W):
    """Input pixels under the convolution pixels either side of every fragment seam of the first tile and of the
    block seam 7 | 8 in both axes (stem_kit), those of the map only."""
    Hc, Wc, _, _ = out_hw(H, W)
    conv = [cp for k in range(1, 19) for cp in fragment_seam_pixels(k)]
    conv += [(2 * TILE - 2, 5), (2 * TILE, 5), (5, 2 * TILE - 2), (5, 2 * TILE), (2 * TILE - 1, 2 * TILE - 1)]
    return [(2 * cy, 2 * cx) for cy, cx in conv if 0 <= cy < Hc and 0 <= cx < Wc and 2 * cy < H and 2 * cx < W]


def _nonfinite_groups(M, H, W):
    """Lists of (image, channel or None, y, x, value): the four corners and one interior pixel of each parity in
    the first, the seam pixels dealt over the others so that a launch keeps clean outputs between them."""
    first = [(0, None, 0, 0, NAN), (0, 1, 0, W - 1, INF), (0, 2, H - 1, 0, -INF), (0, None, H - 1, W - 1, NAN),
             (M - 1, 0, 12, 20, NAN), (M - 1, 1, 13, 9, INF), (M - 1, 0, 20, 13, INF), (M - 1, 2, 21, 27, -INF)]
    groups = [first]
    values = (NAN, INF, -INF, INF)
    seams = _seam_pixels(H, W)
    for start in range(6):
        groups.append([(i % M, (None, 0, 1, 2)[i % 4], y, x, values[i % 4]) for i, (y, x) in enumerate(seams[start::6])])
    return groups


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nonfinite_pixels_reach_exactly_their_footprints(device, dtype):
    """A NaN, +inf, -inf and inf * 0 at single input pixels: each reaches exactly the pooled outputs whose window
    holds a convolution pixel with the input pixel under its 7 x 7 taps, in its own image.  Outside the
    footprints the clean run's bits; inside, the CPU restatement's (NaN where it has NaN, inf * 0 included);
    a NaN pixel fills its footprint in all 64 channels.  The pad K-slots lie on the pixel right of the taps:
    a NaN there must not come through.  A -inf and whatever the ReLU removes do not survive the pool."""
    M, H, W = SEAM_SHAPE
    clean = integer_case(SEAM_SHAPE, seed=93)
    clean.w[:, ZERO_W[0], ZERO_W[1], ZERO_W[2]] = 0.0
    ref_clean = clean.reference()
    for group in _nonfinite_groups(M, H, W):
        x = clean.x.clone()
        inside = torch.zeros(M, *out_hw(H, W)[2:], dtype=torch.bool)
        for n, ch, y, xx, v in group:
            x[n, slice(None) if ch is None else ch, y, xx] = v
            inside[n] |= _footprint(H, W, y, xx)
        assert bool(inside.any()) and not bool(inside.all())
        case = StemCase(x, clean.w, clean.scale, clean.shift)
        ref = pool3(relu64(case.pre_relu())).float()
        nan = torch.isnan(ref)
        inside_c = inside.unsqueeze(1).expand_as(nan)
        assert not bool(nan[~inside_c].any())
        got = nchw(case.run(device, dtype))
        assert (bits(got)[~inside_c.numpy()] == bits(ref_clean)[~inside_c.numpy()]).all()
        assert bool((torch.isnan(got.float()) == nan).all())
        assert (bits(got)[~nan.numpy()] == bits(ref.bfloat16())[~nan.numpy()]).all()
        assert not bool((got.float()[~nan] < 0).any())            # -inf and the negatives are gone
        for n, ch, y, xx, v in group:
            if v != v:
                assert bool(torch.isnan(got.float()[n][:, _footprint(H, W, y, xx)]).all())
    # an inf in channel 0 under the zero weight of the centre tap is a NaN at that convolution pixel
    x = clean.x.clone()
    x[0, 0, 12, 20] = INF
    assert bool(torch.isnan(StemCase(x, clean.w, clean.scale, clean.shift).pre_relu()[0, :, 6, 10]).all())


# ----------------------------------------------------------------------------- guard bands
def _banded_images(x, dtype, device):
    n = x.numel()
    big = torch.full((BAND + n + BAND,), NAN, dtype=dtype, device=device)
    view = big[BAND:BAND + n].view(x.shape)
    view.copy_(x.to(dtype))
    return big, view


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 2, 3), (2, 37, 51), SEAM_SHAPE, INTERIOR_SHAPE), ids=shape_id)
def test_no_reads_or_writes_outside_the_tensors(device, shape, dtype):
    """NaN bands around the images, sentinel bands and a sentinel fill around out (C entry, caller's buffers): a
    read outside the images would put a NaN into the result, a write outside out would break a band, and an
    unwritten element would keep the sentinel."""
    from mvn_rocm import _lib, resnet
    from mvn_rocm._ops import _DTYPE_CODE, _stream
    M, H, W = shape
    case, ref = parity_case(shape)
    big_x, xin = _banded_images(case.x, dtype, device)
    big_o, out = banded(((M, *out_hw(H, W)[2:], COUT), device))
    pk = resnet.pack_stem_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    code = _lib.load().mvn_stem(xin.data_ptr(), _DTYPE_CODE[dtype], pk.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                out.data_ptr(), M, H, W, _stream(xin))
    _lib.check(code, "mvn_stem")
    torch.cuda.synchronize()
    n = out.numel()
    assert bool((big_o[:BAND] == SENTINEL).all()) and bool((big_o[BAND + n:] == SENTINEL).all())
    assert not bool((big_o[BAND:BAND + n] == SENTINEL).any())
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(nchw(out), ref)


# ----------------------------------------------------------------------------- determinism, views, empty batch
def test_two_runs_give_the_same_bits(device):
    for shape in (SEAM_SHAPE, (3, 40, 56)):
        case = random_case(shape, seed=14)
        for dtype in DTYPES:
            xd = case.x.to(dtype).to(device)
            assert_same_bits(case.run(device, images=xd), case.run(device, images=xd))


def _odd_view(t):
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    odd = buf[1:1 + t.numel()].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 16 == t.element_size()
    return odd


def test_views_at_odd_offsets_and_other_strides(device):
    """Images at an odd element offset go through the wrapper as they are (the kernel needs the element's
    alignment only), a channels_last or sliced tensor is made contiguous, misaligned weights are copied; the C
    entry refuses a misaligned out, packed weight, scale or shift before any launch."""
    from mvn_rocm import _lib, resnet
    from mvn_rocm._ops import _DTYPE_CODE, _stream
    shape = (2, 37, 51)
    M, H, W = shape
    case, ref = parity_case(shape)
    pk = resnet.pack_stem_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    for dtype in DTYPES:
        xd = case.x.to(dtype).to(device)
        assert_same_bits(nchw(case.run(device, images=_odd_view(xd))), ref)
        assert_same_bits(nchw(case.run(device, images=xd.to(memory_format=torch.channels_last))), ref)
        wide = torch.zeros(M, CIN, H, W + 3, dtype=dtype, device=device)
        wide[..., :W] = xd
        assert_same_bits(nchw(case.run(device, images=wide[..., :W])), ref)
    assert_same_bits(nchw(resnet.stem(case.x.to(device), _odd_view(pk), _odd_view(sc), _odd_view(sh))), ref)
    out = torch.zeros(M * 10 * 13 * COUT + 8, dtype=torch.bfloat16, device=device)
    xd = case.x.to(device)
    lib = _lib.load()

    def c(x, w, s, t, o):
        return lib.mvn_stem(x.data_ptr(), _DTYPE_CODE[x.dtype], w.data_ptr(), s.data_ptr(), t.data_ptr(), o.data_ptr(), M, H, W,
                            _stream(xd))
    assert c(xd, pk, sc, sh, out[1:]) == -1 and c(xd, _odd_view(pk), sc, sh, out) == -1
    assert c(xd, pk, _odd_view(sc), sh, out) == -1 and c(xd, pk, sc, _odd_view(sh), out) == -1
    torch.cuda.synchronize()
    assert not bool(out.any())                                    # refused before any launch
    assert c(_odd_view(xd), pk, sc, sh, out) == 0                 # the images need their element's alignment only
    torch.cuda.synchronize()
    assert_same_bits(nchw(out[:M * 10 * 13 * COUT].view(M, 10, 13, COUT)), ref)


def test_empty_batch(device):
    from mvn_rocm import resnet
    case, _ = parity_case((2, 2, 3))
    pk = resnet.pack_stem_weight(case.w.double()).to(device)
    for dtype in DTYPES:
        y = resnet.stem(torch.zeros(0, 3, 37, 51, dtype=dtype, device=device), pk, case.scale.to(device), case.shift.to(device))
        assert tuple(y.shape) == (0, 10, 13, COUT) and y.dtype == torch.bfloat16
