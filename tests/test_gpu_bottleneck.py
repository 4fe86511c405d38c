"""mvn_conv1x1 and mvn_conv3x3 on the GPU (csrc/bottleneck.hip) against ``F.conv2d`` on the
CPU: operands for which the kernels' f32 arithmetic is exact in any order (integers, impulses) bit for
bit, random data within the contract's own bound, non-finite pixels either side of every tile seam
(tests/bottleneck_kit.py: flat pixels 16 k, 64 k, 256 k), guard bands, determinism, the wrapper's copy of
a misaligned view and the empty batch."""
import pytest
import torch
import torch.nn.functional as F

from bottleneck_kit import (CONV1_SHAPES, CONV3_SHAPES, POINTWISE_CASES, Conv1Case, Conv3Case, check_bound, conv1, conv3,
                            index_weight1, index_weight3, integer_conv1, integer_conv3, parity_conv1, parity_conv3,
                            random_conv1, random_conv3, relu64, shape_id)
from deconv_kit import cl2d, nchw
from v2v_kit import BAND, IDENTITY, NONE, POINTWISE, SENTINEL, assert_same_bits, banded, bf16_full, bits

pytestmark = pytest.mark.gpu

MODES = (NONE, IDENTITY)
MODE_IDS = ("none", "identity")
PW_IDS = [f"{shape_id(s)}_from_{cs}x{hs}x{ws}_s{st}" for s, cs, st, hs, ws in POINTWISE_CASES]


# ----------------------------------------------------------------------------- integer data
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=shape_id)
def test_conv1x1_integer_data_bit_equal_to_the_cpu(device, shape, mode):
    """Every sum is exact in f32 (asserted: the sum of |x w| is below 2^24), so the kernel must return the CPU
    restatement's bits, the skip term included."""
    case, ref, _ = parity_conv1(shape, mode)
    assert_same_bits(nchw(case.run(device)), ref.bfloat16())


@pytest.mark.parametrize("shape, cs, stride, Hs, Ws", POINTWISE_CASES, ids=PW_IDS)
def test_conv1x1_pointwise_skip_integer_data_bit_equal_to_the_cpu(device, shape, cs, stride, Hs, Ws):
    case, ref, _ = parity_conv1(shape, POINTWISE, (cs, stride, Hs, Ws))
    assert_same_bits(nchw(case.run(device)), ref.bfloat16())


@pytest.mark.parametrize("shape", CONV3_SHAPES, ids=shape_id)
def test_conv3x3_integer_data_bit_equal_to_the_cpu(device, shape):
    case, ref, _ = parity_conv3(shape)
    got = case.run(device)
    M, C, H, W, s = shape
    assert tuple(got.shape) == (M, (H - 1) // s + 1, (W - 1) // s + 1, C)
    assert_same_bits(nchw(got), ref.bfloat16())


# ----------------------------------------------------------------------------- index weights, impulses
def _signed_scale(g, n):
    return (0.75 + 0.5 * torch.rand(n, generator=g)) * torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0)


def _impulse_reference(acc64, scale):
    """One product per output at the most, so the output is that product times the scale: one f32 rounding
    (the fma with a zero shift), relu, one bf16 rounding."""
    r = (acc64 * scale.double().view(1, -1, 1, 1)).float()
    return torch.where(r <= 0, torch.zeros_like(r), r).bfloat16()


@pytest.mark.parametrize("shape", ((1, 256, 9, 15, 64), (1, 2048, 20, 18, 64), (2, 64, 3, 5, 2048)), ids=shape_id)
def test_conv1x1_impulses_read_every_weight_slot(device, shape):
    """One non-zero channel per pixel, the channels counted on across the pixels and the launches: every output
    is one product, the weight encodes its own (co, ci), and the launches together read every (co, ci) slot
    and write every output (asserted on the CPU)."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(cin + cout)
    w, scale = index_weight1(cout, cin), _signed_scale(g, cout)
    P = M * H * W
    covered, k = torch.zeros(cin, dtype=torch.bool), 0
    for _ in range(-(-cin // P)):
        ch = (k + torch.arange(P)) % cin
        k += P
        x = torch.zeros(P, cin)
        x[torch.arange(P), ch] = bf16_full((P,), g)
        x = x.view(M, H, W, cin).permute(0, 3, 1, 2).contiguous()
        assert int((x != 0).sum(1).max()) == 1 and int((x != 0).sum(1).min()) == 1    # every pixel, so every output
        covered[ch] = True
        case = Conv1Case(x, w, scale, torch.zeros(cout))
        assert_same_bits(nchw(case.run(device)), _impulse_reference(conv1(x.double(), w.double()), scale))
    assert bool(covered.all())                                    # every ci meets all cout rows of w


@pytest.mark.parametrize("stride, Hs, Ws", ((1, 9, 15), (2, 17, 29), (2, 18, 30)), ids=("s1", "s2_odd", "s2_even"))
def test_conv1x1_pointwise_impulses_read_every_skip_weight_slot(device, stride, Hs, Ws):
    """The same through the fused downsample: impulses in x at the even flat pixels and in the skip tensor at the
    sources of the odd ones, so every output is still one product; w and w_s encode their indices with
    different values."""
    M, cin, H, W, cout, cs = 1, 64, 9, 15, 128, 256
    g = torch.Generator().manual_seed(stride + Hs)
    w, ws = index_weight1(cout, cin), index_weight1(cout, cs) * 2.0 ** 20
    scale, scale_s = _signed_scale(g, cout), _signed_scale(g, cout)
    P = H * W
    even, odd = torch.arange(0, P, 2), torch.arange(1, P, 2)
    covered, covered_s = torch.zeros(cin, dtype=torch.bool), torch.zeros(cs, dtype=torch.bool)
    for rnd in range(4):                                          # 4 x 67 odd pixels >= the 256 channels of the skip
        x = torch.zeros(P, cin)
        ch = (rnd * even.numel() + torch.arange(even.numel())) % cin
        x[even, ch] = bf16_full((even.numel(),), g)
        covered[ch] = True
        skip = torch.zeros(Hs, Ws, cs)
        chs = (rnd * odd.numel() + torch.arange(odd.numel())) % cs
        skip[stride * (odd // W), stride * (odd % W), chs] = bf16_full((odd.numel(),), g)
        covered_s[chs] = True
        x = x.view(1, H, W, cin).permute(0, 3, 1, 2).contiguous()
        skip = skip.permute(2, 0, 1).unsqueeze(0).contiguous()
        case = Conv1Case(x, w, scale, torch.zeros(cout), POINTWISE, skip, ws, scale_s, torch.zeros(cout), stride)
        a, b = conv1(x.double(), w.double()), conv1(case.skip_sampled().double(), ws.double())
        assert not bool(((a != 0) & (b != 0)).any()) and bool(((a != 0) | (b != 0)).all())
        # each term is rounded by its own fma; the other term is +0 or -0, which the add and the relu absorb
        r = (a * scale.double().view(1, -1, 1, 1)).float() + (b * scale_s.double().view(1, -1, 1, 1)).float()
        ref = torch.where(r <= 0, torch.zeros_like(r), r).bfloat16()
        assert_same_bits(nchw(case.run(device)), ref)
    assert bool(covered.all()) and bool(covered_s.all())


def lattice3(C, M, H, W, rounds, g):
    """Impulses at every third pixel of both axes (the footprints of two input pixels three apart are disjoint
    at stride 1 and 2), nine offsets per round, one channel each, the channels counted on across the launches."""
    k = 0
    for _ in range(rounds):
        for oy in range(3):
            for ox in range(3):
                ys, xs = torch.arange(oy, H, 3), torch.arange(ox, W, 3)
                if ys.numel() == 0 or xs.numel() == 0:
                    continue
                mm, yy, xx = (t.reshape(-1) for t in torch.meshgrid(torch.arange(M), ys, xs, indexing="ij"))
                n = mm.numel()
                ch = (k + torch.arange(n)) % C
                k += n + 1                                        # + 1: a channel moves on to other parities
                yield mm, yy, xx, ch, bf16_full((n,), g)


def lattice3_coverage(C, M, H, W, stride, rounds, g=None):
    """(covered (C, 3, 3): channel ci met tap (ky, kx) unclipped, written (Ho, Wo): the output was non-zero in
    some launch) of ``lattice3``, on the CPU."""
    g = g or torch.Generator().manual_seed(0)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    covered, written = torch.zeros(C, 3, 3, dtype=torch.bool), torch.zeros(Ho, Wo, dtype=torch.bool)
    for mm, yy, xx, ch, _ in lattice3(C, M, H, W, rounds, g):
        for ky in range(3):
            for kx in range(3):
                ny, nx = yy + 1 - ky, xx + 1 - kx                # stride * (oy, ox)
                ok = (ny >= 0) & (nx >= 0) & (ny % stride == 0) & (nx % stride == 0) & (ny // stride < Ho) & (nx // stride < Wo)
                covered[ch[ok], ky, kx] = True
                written[ny[ok] // stride, nx[ok] // stride] = True
    return covered, written


def sparse_conv3(mm, yy, xx, ch, val, w, M, H, W, stride):
    """The 3x3 convolution of the impulses ``val`` at (mm, ch, yy, xx), one product per output: float64, exact."""
    C, Ho, Wo = w.shape[0], (H - 1) // stride + 1, (W - 1) // stride + 1
    acc = torch.zeros(M, C, Ho, Wo, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            ny, nx = yy + 1 - ky, xx + 1 - kx                    # stride * (oy, ox)
            ok = (ny >= 0) & (nx >= 0) & (ny % stride == 0) & (nx % stride == 0) & (ny // stride < Ho) & (nx // stride < Wo)
            acc[mm[ok], :, ny[ok] // stride, nx[ok] // stride] = val[ok].double()[:, None] * w[:, ch[ok], ky, kx].double().t()
    return acc


@pytest.mark.parametrize("C, M, H, W, stride, rounds", [(64, 2, 20, 18, 1, 2), (64, 2, 20, 18, 2, 2), (128, 2, 20, 18, 2, 4),
                                                        (512, 2, 20, 18, 1, 3)], ids=lambda v: str(v))
def test_conv3x3_impulse_lattices_read_every_weight_slot(device, C, M, H, W, stride, rounds):
    """At most one product per output (asserted), so the output is that product times the scale, rounded once;
    with a weight that encodes its own (co, ci, ky, kx) the launches together must read every slot (asserted
    on the CPU: every (ci, ky, kx) is met by an unclipped tap, and every impulse reaches all co) and write
    every output pixel."""
    g = torch.Generator().manual_seed(C + H + stride)
    w, scale = index_weight3(C), _signed_scale(g, C)
    covered, written = lattice3_coverage(C, M, H, W, stride, rounds)
    assert bool(covered.all()), f"{int((~covered).sum())} (ci, ky, kx) slots are never read"
    assert bool(written.all())
    for mm, yy, xx, ch, val in lattice3(C, M, H, W, rounds, g):
        x = torch.zeros(M, C, H, W)
        x[mm, ch, yy, xx] = val
        hits = conv3((x != 0).sum(1, keepdim=True).double(), torch.ones(1, 1, 3, 3, dtype=torch.float64), stride)
        assert float(hits.max()) == 1.0
        acc = sparse_conv3(mm, yy, xx, ch, val, w, M, H, W, stride)
        assert int((acc != 0).sum()) == int(hits.sum()) * C
        if C == 64:                                               # the sparse restatement against F.conv2d
            assert torch.equal(acc, conv3(x.double(), w.double(), stride))
        case = Conv3Case(x, w, scale, torch.zeros(C), stride)
        assert_same_bits(nchw(case.run(device)), _impulse_reference(acc, scale))


# ----------------------------------------------------------------------------- random data
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=shape_id)
def test_conv1x1_random_data_within_the_contract_bound(device, shape, mode):
    case = random_conv1(shape, mode, seed=sum(shape) + mode)
    check_bound(case, nchw(case.run(device)).float(), f"conv1x1 {shape_id(shape)} mode {mode}")


@pytest.mark.parametrize("shape, cs, stride, Hs, Ws", POINTWISE_CASES, ids=PW_IDS)
def test_conv1x1_pointwise_skip_random_data_within_the_contract_bound(device, shape, cs, stride, Hs, Ws):
    case = random_conv1(shape, POINTWISE, seed=sum(shape) + cs, pointwise=(cs, stride, Hs, Ws))
    check_bound(case, nchw(case.run(device)).float(), f"conv1x1 {shape_id(shape)} pointwise from {cs} at stride {stride}")


@pytest.mark.parametrize("shape", CONV3_SHAPES, ids=shape_id)
def test_conv3x3_random_data_within_the_contract_bound(device, shape):
    case = random_conv3(shape, seed=sum(shape))
    check_bound(case, nchw(case.run(device)).float(), f"conv3x3 {shape_id(shape)}")


# ----------------------------------------------------------------------------- non-finite values
NAN, INF = float("nan"), float("inf")
# flat pixels of a 17 x 17 map: the corners and either side of the seams 15 | 16, 63 | 64, 255 | 256
NF_FLAT = ((0, None, NAN), (288, None, NAN), (15, 3, INF), (16, 5, NAN), (63, 9, -INF), (64, 0, INF), (255, 17, NAN),
           (256, 30, -INF))
ZERO_W_CHANNEL = 0               # w[:, 0] is zero: the +inf in channel 0 of pixel 64 meets it as inf * 0


def _same_outside_and_follows_inside(got, ref_clean, ref, inside):
    """Outside ``inside`` (H, W) the clean run's bits; inside, NaN where the CPU has NaN and its bits elsewhere."""
    want_clean, want = ref_clean.bfloat16(), ref.bfloat16()
    assert_same_bits(got[..., ~inside], want_clean[..., ~inside])
    nan = torch.isnan(ref)
    assert bool((torch.isnan(got.float()) == nan).all())
    assert not bool(nan[..., ~inside].any())
    assert (bits(got)[~nan.numpy()] == bits(want)[~nan.numpy()]).all()


@pytest.mark.parametrize("mode", (NONE, IDENTITY, POINTWISE), ids=("none", "identity", "pointwise"))
def test_conv1x1_nonfinite_pixels_reach_exactly_their_pixel(device, mode):
    """A NaN, +inf, -inf and inf * 0 at single pixels of x, in the corners and either side of every tile seam:
    each reaches its own output pixel only.  With a skip, non-finite skip pixels too: an identity skip's at its
    own element; a stride-2 pointwise skip's at the one output that reads it, and at none where the stride
    passes over it."""
    shape = (1, 64, 17, 17, 128)
    clean = integer_conv1(shape, mode, seed=91, pointwise=(64, 2, 33, 34))
    clean.w[:, ZERO_W_CHANNEL] = 0.0
    x = clean.x.clone()
    inside = torch.zeros(17 * 17, dtype=torch.bool)
    for p, ch, v in NF_FLAT:
        x[0, slice(None) if ch is None else ch, p // 17, p % 17] = v
        inside[p] = True
    skip = None if clean.skip is None else clean.skip.clone()
    if mode == IDENTITY:
        for p, v in ((1, NAN), (17, INF), (254, -INF), (257, NAN)):
            skip[0, 7, p // 17, p % 17] = v
            inside[p] = True
    if mode == POINTWISE:
        skip[0, 3, 1, 0] = NAN                                    # odd row: no output reads it
        skip[0, 5, 32, 33] = INF                                  # odd column
        for p, v in ((2, NAN), (14, INF), (258, NAN)):
            skip[0, 11, 2 * (p // 17), 2 * (p % 17)] = v
            inside[p] = True
    inside = inside.view(17, 17)
    case = Conv1Case(x, clean.w, clean.scale, clean.shift, mode, skip, clean.skip_w, clean.skip_scale, clean.skip_shift,
                     clean.skip_stride)
    ref_clean, _ = clean.reference()
    ref = relu64(case.pre_relu()).float()
    assert bool(torch.isnan(ref[0, :, 64 // 17, 64 % 17]).all())  # inf * 0
    got = nchw(case.run(device))
    _same_outside_and_follows_inside(got, ref_clean, ref, inside)
    for p, ch, v in NF_FLAT:
        if v != v:
            assert bool(torch.isnan(got.float()[0, :, p // 17, p % 17]).all())


# input pixels of a 20 x 18 map: the corners, and the pixels whose outputs lie either side of the flat seams
# (stride 1: 15 | 16 = (0, 15) | (0, 16), 63 | 64 = (3, 9) | (3, 10), 255 | 256 = (14, 3) | (14, 4))
NF_PIXELS3 = ((0, 0, None, NAN), (19, 17, None, NAN), (0, 15, 3, INF), (0, 16, 5, -INF), (3, 9, 9, NAN), (3, 10, 0, INF),
              (14, 3, 17, NAN), (14, 4, 30, -INF), (9, 17, 2, INF), (19, 0, 6, NAN), (7, 0, 1, -INF))


@pytest.mark.parametrize("stride", (1, 2))
def test_conv3x3_nonfinite_pixels_reach_exactly_their_boxes(device, stride):
    """The same for the 3x3: input pixel (iy, ix) reaches exactly the outputs (oy, ox) with |stride oy - iy| <= 1
    and |stride ox - ix| <= 1, clipped.  Outside the boxes the clean run's bits; inside, the CPU convolution's
    (NaN where it has NaN, inf * 0 included); a NaN pixel fills its box."""
    H, W = 20, 18
    clean = integer_conv3((1, 64, H, W, stride), seed=92)
    clean.w[:, ZERO_W_CHANNEL, 1, 2] = 0.0
    x = clean.x.clone()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    oy, ox = torch.arange(Ho).view(-1, 1), torch.arange(Wo).view(1, -1)
    inside = torch.zeros(Ho, Wo, dtype=torch.bool)
    boxes = []
    for iy, ix, ch, v in NF_PIXELS3:
        x[0, slice(None) if ch is None else ch, iy, ix] = v
        b = ((stride * oy - iy).abs() <= 1) & ((stride * ox - ix).abs() <= 1)
        boxes.append(b)
        inside |= b
    case = Conv3Case(x, clean.w, clean.scale, clean.shift, stride)
    ref_clean, _ = clean.reference()
    ref = relu64(case.pre_relu()).float()
    # the +inf of pixel (3, 10) channel 0 meets the zero weight at tap (1, 2): output (3, 9) at stride 1
    if stride == 1:
        assert bool(torch.isnan(ref[0, :, 3, 9]).all())
    got = nchw(case.run(device))
    _same_outside_and_follows_inside(got, ref_clean, ref, inside)
    for (iy, ix, ch, v), b in zip(NF_PIXELS3, boxes):
        if v != v:
            assert bool(torch.isnan(got.float()[0][:, b]).all())


# ----------------------------------------------------------------------------- guard bands
def _banded_out(shape, device):
    big, out = banded((shape, device))
    return big, out


def _bands_ok(big_o, n, *big_ins):
    assert bool((big_o[:BAND] == SENTINEL).all()) and bool((big_o[BAND + n:] == SENTINEL).all())
    assert not bool((big_o[BAND:BAND + n] == SENTINEL).any())
    for big, m in big_ins:
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + m:]).all())


@pytest.mark.parametrize("shape, mode, pw", [((3, 64, 3, 5, 256), NONE, None), ((1, 256, 9, 15, 64), IDENTITY, None),
                                             ((1, 64, 17, 17, 128), IDENTITY, None), ((3, 64, 3, 5, 256), POINTWISE, (256, 2, 5, 9)),
                                             ((1, 64, 17, 17, 128), POINTWISE, (64, 2, 33, 34))],
                         ids=("45_none", "135_identity", "289_identity", "45_pointwise", "289_pointwise"))
def test_conv1x1_no_reads_or_writes_outside_the_tensors(device, shape, mode, pw):
    """NaN bands around x and skip, sentinel bands and a sentinel fill around out (C entry, caller's buffers): a
    read outside an operand would put a NaN into the result, a write outside out would break a band, and an
    unwritten element would keep the sentinel."""
    from mvn_rocm import _lib, resnet
    from mvn_rocm._ops import _stream
    M, cin, H, W, cout = shape
    case, ref, _ = parity_conv1(shape, mode, pw)
    big_x, xin = banded(cl2d(case.x, device))
    big_o, out = _banded_out((M, H, W, cout), device)
    pk = resnet.pack_conv1x1_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    ins = [(big_x, xin.numel())]
    sk = spk = ssc = ssh = None
    cs = Hs = Ws = 0
    if mode != NONE:
        big_s, sk = banded(cl2d(case.skip, device))
        ins.append((big_s, sk.numel()))
    if mode == POINTWISE:
        cs, _, Hs, Ws = pw
        spk = resnet.pack_conv1x1_weight(case.skip_w.double()).to(device)
        ssc, ssh = case.skip_scale.to(device), case.skip_shift.to(device)
    ptr = lambda t: None if t is None else t.data_ptr()
    code = _lib.load().mvn_conv1x1(xin.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), mode, ptr(sk), ptr(spk),
                                   ptr(ssc), ptr(ssh), cs, Hs, Ws, case.skip_stride, out.data_ptr(), M, H, W, cin, cout,
                                   _stream(xin))
    _lib.check(code, "mvn_conv1x1")
    torch.cuda.synchronize()
    _bands_ok(big_o, out.numel(), *ins)
    assert_same_bits(nchw(out), ref.bfloat16())


@pytest.mark.parametrize("shape", ((2, 64, 1, 1, 2), (1, 64, 5, 7, 2), (3, 64, 4, 5, 1), (1, 64, 20, 18, 1), (2, 192, 5, 7, 2)),
                         ids=shape_id)
def test_conv3x3_no_reads_or_writes_outside_the_tensors(device, shape):
    from mvn_rocm import _lib, resnet
    from mvn_rocm._ops import _stream
    M, C, H, W, s = shape
    case, ref, _ = parity_conv3(shape)
    big_x, xin = banded(cl2d(case.x, device))
    big_o, out = _banded_out((M, (H - 1) // s + 1, (W - 1) // s + 1, C), device)
    pk = resnet.pack_conv3x3_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    code = _lib.load().mvn_conv3x3(xin.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), M, H, W, C,
                                   s, _stream(xin))
    _lib.check(code, "mvn_conv3x3")
    torch.cuda.synchronize()
    _bands_ok(big_o, out.numel(), (big_x, xin.numel()))
    assert_same_bits(nchw(out), ref.bfloat16())


# ----------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits(device):
    c1 = random_conv1((1, 64, 17, 17, 128), POINTWISE, seed=12, pointwise=(64, 2, 33, 34))
    xd, sd = cl2d(c1.x, device), cl2d(c1.skip, device)
    assert_same_bits(c1.run(device, xd, sd), c1.run(device, xd, sd))
    c1 = random_conv1((1, 2048, 2, 3, 512), IDENTITY, seed=13)
    xd, sd = cl2d(c1.x, device), cl2d(c1.skip, device)
    assert_same_bits(c1.run(device, xd, sd), c1.run(device, xd, sd))
    for shape in ((1, 64, 20, 18, 1), (1, 512, 3, 4, 1), (1, 128, 12, 12, 2)):
        c3 = random_conv3(shape, seed=14)
        xd = cl2d(c3.x, device)
        assert_same_bits(c3.run(device, xd), c3.run(device, xd))


# ----------------------------------------------------------------------------- misaligned views
def _odd_view(t):
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    odd = buf[1:1 + t.numel()].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 16 == 2
    return odd


def test_a_misaligned_view_equals_the_aligned_call(device):
    """The C entries take 16-byte aligned pointers only (MVN_ERR_ARG otherwise): the kernels have no
    element-aligned path.  The wrappers copy a view at an odd element offset."""
    from mvn_rocm import _lib, resnet
    from mvn_rocm._ops import _stream
    shape = (3, 64, 3, 5, 256)
    case, ref, _ = parity_conv1(shape, IDENTITY)
    xd, sd = cl2d(case.x, device), cl2d(case.skip, device)
    assert_same_bits(nchw(case.run(device, _odd_view(xd), _odd_view(sd))), ref.bfloat16())
    pk = resnet.pack_conv1x1_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    out = torch.zeros(45 * 256 + 8, dtype=torch.bfloat16, device=device)
    lib = _lib.load()

    def c1(x, skip, o):
        return lib.mvn_conv1x1(x.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), IDENTITY, skip.data_ptr(), None,
                               None, None, 0, 0, 0, 1, o.data_ptr(), 3, 3, 5, 64, 256, _stream(xd))
    assert c1(_odd_view(xd), sd, out) == -1 and c1(xd, _odd_view(sd), out) == -1 and c1(xd, sd, out[1:]) == -1

    shape3 = (1, 64, 5, 7, 2)
    case3, ref3, _ = parity_conv3(shape3)
    x3 = cl2d(case3.x, device)
    assert_same_bits(nchw(case3.run(device, _odd_view(x3))), ref3.bfloat16())
    pk3 = resnet.pack_conv3x3_weight(case3.w.double()).to(device)
    sc3, sh3 = case3.scale.to(device), case3.shift.to(device)

    def c3(x, o):
        return lib.mvn_conv3x3(x.data_ptr(), pk3.data_ptr(), sc3.data_ptr(), sh3.data_ptr(), o.data_ptr(), 1, 5, 7, 64, 2,
                               _stream(xd))
    assert c3(_odd_view(x3), out) == -1 and c3(x3, out[1:]) == -1
    torch.cuda.synchronize()
    assert not bool(out.any())                                    # refused before any launch


# ----------------------------------------------------------------------------- empty batch
def test_empty_batch(device):
    from mvn_rocm import resnet
    case, _, _ = parity_conv1((3, 64, 3, 5, 256), IDENTITY)
    pk = resnet.pack_conv1x1_weight(case.w.double()).to(device)
    x = torch.zeros(0, 3, 5, 64, dtype=torch.bfloat16, device=device)
    y = resnet.conv1x1(x, pk, case.scale.to(device), case.shift.to(device))
    assert tuple(y.shape) == (0, 3, 5, 256) and y.dtype == torch.bfloat16
    y = resnet.conv1x1(x, pk, case.scale.to(device), case.shift.to(device), skip=y)
    assert tuple(y.shape) == (0, 3, 5, 256)
    case3, _, _ = parity_conv3((1, 64, 5, 7, 2))
    pk3 = resnet.pack_conv3x3_weight(case3.w.double()).to(device)
    y = resnet.conv3x3(torch.zeros(0, 5, 7, 64, dtype=torch.bfloat16, device=device), pk3, case3.scale.to(device),
                       case3.shift.to(device), stride=2)
    assert tuple(y.shape) == (0, 3, 4, 64) and y.dtype == torch.bfloat16
