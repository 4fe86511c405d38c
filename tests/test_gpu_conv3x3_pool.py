"""mvn_conv3x3_pool on the GPU (csrc/confidence_head.hip) against ``F.conv2d`` and
``F.max_pool2d`` on the CPU: operands for which the kernel's f32 arithmetic is exact in any order bit for bit,
for both output types; random data within the contract's own bound carried
through the maximum; index weights; non-finite pixels; guard bands; the C entry's argument errors and the
dispatcher (tests/confidence_kit.py)."""
import pytest
import torch
import torch.nn.functional as F

from confidence_kit import (POOL_SHAPES, SUBSET, PoolCase, check_pool_bound, conv3,
                            index_weight_pool, integer_pool, nchw, parity_pool, pool, random_pool, relu64, shape_id)
from deconv_kit import banded_out, cl2d
from v2v_kit import BAND, assert_same_bits, banded, bf16_full, bits

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float32)
DTYPE_IDS = ("bf16", "f32")


def _as(ref, dtype):
    return ref.bfloat16() if dtype == torch.bfloat16 else ref


# ----------------------------------------------------------------------------- integer data
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=shape_id)
def test_integer_data_bit_equal_to_the_cpu(device, shape):
    """Every sum is exact in f32 (asserted: the sum of |x w| is below 2^24, the fma exact), so the kernel must
    return the CPU restatement's bits, as bf16 and as f32; the f32 output rounded
    is the bf16 output."""
    case, ref = parity_pool(shape)
    M, _, H, W, cout = shape
    xd = cl2d(case.x, device)
    got16 = case.run(device, torch.bfloat16, xd)
    got32 = case.run(device, torch.float32, xd)
    assert tuple(got16.shape) == tuple(got32.shape) == (M, H // 2, W // 2, cout)
    assert got16.dtype == torch.bfloat16 and got32.dtype == torch.float32
    assert_same_bits(nchw(got32), ref)
    assert_same_bits(nchw(got16), ref.bfloat16())
    assert_same_bits(got32.bfloat16(), got16)


# ----------------------------------------------------------------------------- random data
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=shape_id)
def test_random_data_within_the_contract_bound(device, shape):
    case = random_pool(shape, seed=sum(shape))
    xd = cl2d(case.x, device)
    got32 = case.run(device, torch.float32, xd)
    got16 = case.run(device, torch.bfloat16, xd)
    check_pool_bound(case, nchw(got32), f"conv3x3_pool {shape_id(shape)} f32", f32_out=True)
    check_pool_bound(case, nchw(got16).float(), f"conv3x3_pool {shape_id(shape)} bf16", f32_out=False)
    assert_same_bits(got32.bfloat16(), got16)


def test_two_runs_give_the_same_bits(device):
    for shape in ((1, 64, 18, 20, 64), (1, 512, 6, 6, 256)):
        case = random_pool(shape, seed=14)
        xd = cl2d(case.x, device)
        assert_same_bits(case.run(device, torch.float32, xd), case.run(device, torch.float32, xd))


# ----------------------------------------------------------------------------- index weights
def _lattice(M, H, W, cin, rounds, g):
    """Positive impulses at every fourth pixel of both axes (the windows that two of them reach are disjoint: input
    row 4 k + a reaches the windows 2 k + (a - 1) // 2 .. 2 k + (a + 1) // 2), sixteen offsets per round, one channel
    each, the channels counted on across the launches.  A window's winner is the conv pixel with the highest tap
    (the weight's exponent grows with it): tap row 1 wins from an even input row, 0 and 2 from an odd one."""
    k = 0
    for _ in range(rounds):
        for oy in range(4):
            for ox in range(4):
                ys, xs = torch.arange(oy, H, 4), torch.arange(ox, W, 4)
                if ys.numel() == 0 or xs.numel() == 0:
                    continue
                mm, yy, xx = (t.reshape(-1) for t in torch.meshgrid(torch.arange(M), ys, xs, indexing="ij"))
                n = mm.numel()
                ch = (k + torch.arange(n)) % cin
                k += n + 1                                        # + 1: a channel moves on to other offsets
                yield mm, yy, xx, ch, bf16_full((n,), g).abs()


@pytest.mark.parametrize("shape, rounds, every_slot", (((1, 64, 18, 20, 64), 6, True), ((1, 192, 4, 4, 128), 6, False)),
                         ids=("1x64x18x20x64", "1x192x4x4x128"))
def test_impulse_lattices_read_every_weight_slot(device, shape, rounds, every_slot):
    """One-hot input pixels: every conv pixel holds one product at the most (asserted), so r_q is that product
    times the scale, rounded once, and the pooled output the largest of its window.  The weight encodes its own
    (co, ci, ky, kx) and the scale has the weight's sign, so every product is positive and the winner of a window
    is visible; the launches together must show every slot as a winner (counted on the CPU, asserted).  The second shape (not one of POOL_SHAPES: 6 K-steps per tap, two channel groups, one
    impulse per launch) shows every tap in every block of 32 input x 64 output channels instead."""
    M, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    w = index_weight_pool(cout, cin)
    scale = (0.75 + 0.5 * torch.rand(cout, generator=g)) * torch.sign(w[:, 0, 0, 0])
    covered = torch.zeros(cout, cin, 3, 3, dtype=torch.bool)
    ones = torch.ones(1, 1, 3, 3, dtype=torch.float64)
    for mm, yy, xx, ch, val in _lattice(M, H, W, cin, rounds, g):
        x = torch.zeros(M, cin, H, W)
        x[mm, ch, yy, xx] = val
        assert float(conv3((x != 0).sum(1, keepdim=True).double(), ones).max()) == 1.0
        r = (conv3(x.double(), w.double()) * scale.double().view(1, -1, 1, 1)).float()       # one product, one rounding
        assert bool((r >= 0).all())
        ref, idx = F.max_pool2d(r, 2, return_indices=True)
        ref = relu64(ref)                                            # a window of -0 gives +0
        # the winner's conv pixel -> the impulse that it saw and the tap between them
        ci_map = torch.full((M, H + 2, W + 2), -1, dtype=torch.long)
        iy_map, ix_map = ci_map.clone(), ci_map.clone()
        for dy in range(3):
            for dx in range(3):
                ci_map[mm, yy + dy, xx + dx], iy_map[mm, yy + dy, xx + dx], ix_map[mm, yy + dy, xx + dx] = ch, yy, xx
        oy, ox = idx // W, idx % W                                   # (M, cout, Hp, Wp) conv pixels
        n_i = torch.arange(M).view(M, 1, 1, 1).expand_as(idx)
        co_i = torch.arange(cout).view(1, cout, 1, 1).expand_as(idx)
        ci = ci_map[n_i, oy + 1, ox + 1]
        ky, kx = iy_map[n_i, oy + 1, ox + 1] - oy + 1, ix_map[n_i, oy + 1, ox + 1] - ox + 1
        won = ref > 0
        assert bool((ci[won] >= 0).all())
        covered[co_i[won], ci[won], ky[won], kx[won]] = True
        case = PoolCase(x, w, scale, torch.zeros(cout))
        assert_same_bits(nchw(case.run(device, torch.float32)), ref)
    if every_slot:
        assert bool(covered.all()), f"{int((~covered).sum())} of {covered.numel()} (co, ci, ky, kx) slots never won a window"
    else:
        blocks = covered.view(cout // 64, 64, cin // 32, 32, 3, 3).any(3).any(1)          # (group, K-step of a tap, ky, kx)
        assert bool(blocks.all()), f"{int((~blocks).sum())} of {blocks.numel()} (group, kp, ky, kx) blocks never won a window"


# ----------------------------------------------------------------------------- non-finite values, the ReLU's zero
NAN, INF = float("nan"), float("inf")


def _footprint(H, W, iy, ix):
    """The windows (py, px) whose four conv pixels' taps reach input pixel (iy, ix): 2 py - 1 <= iy <= 2 py + 2."""
    py, px = torch.arange(H // 2).view(-1, 1), torch.arange(W // 2).view(1, -1)
    return (2 * py - 1 <= iy) & (iy <= 2 * py + 2) & (2 * px - 1 <= ix) & (ix <= 2 * px + 2)


# (shape, image, iy, ix): corners, the dropped odd row and column, pixels whose windows lie either side of
# the 16-window seam, the last pixel of an image whose neighbour shares the tile
NF_CASES = (((2, 64, 3, 3, 64), 1, 2, 2), ((2, 64, 3, 3, 64), 0, 0, 0), ((3, 64, 4, 6, 64), 1, 3, 5), ((3, 64, 4, 6, 64), 2, 2, 1),
            ((1, 64, 18, 20, 64), 0, 3, 11), ((1, 64, 18, 20, 64), 0, 17, 19), ((1, 192, 4, 4, 64), 0, 1, 2))


@pytest.mark.parametrize("shape, n, iy, ix", NF_CASES, ids=lambda v: shape_id(v) if isinstance(v, tuple) else str(v))
def test_a_nan_pixel_fills_exactly_its_windows(device, shape, n, iy, ix):
    """One NaN input pixel (every channel) makes NaN exactly the pooled outputs whose windows' footprints hold it,
    in every output channel, and leaves every other output's bits as they were."""
    M, cin, H, W, cout = shape
    clean, ref = parity_pool(shape)
    x = clean.x.clone()
    x[n, :, iy, ix] = NAN
    inside = torch.zeros(M, H // 2, W // 2, dtype=torch.bool)
    inside[n] = _footprint(H, W, iy, ix)
    assert bool(inside.any())
    got = nchw(PoolCase(x, clean.w, clean.scale, clean.shift).run(device, torch.float32))
    nan = torch.isnan(got)
    assert bool((nan == inside.view(M, 1, H // 2, W // 2).expand_as(nan)).all())
    assert (bits(got)[~nan.numpy()] == bits(ref)[~nan.numpy()]).all()


@pytest.mark.parametrize("shape, n, iy, ix", NF_CASES[2:6], ids=lambda v: shape_id(v) if isinstance(v, tuple) else str(v))
def test_an_infinite_pixel_follows_the_cpu_inside_its_windows(device, shape, n, iy, ix):
    """+inf in one channel of one pixel: inside the footprint the CPU's values (+inf where the window's largest
    r is +inf, NaN where the infinity meets a zero weight, what the ReLU leaves of -inf), outside the clean bits."""
    M, cin, H, W, cout = shape
    clean, ref_clean = parity_pool(shape)
    x = clean.x.clone()
    x[n, 5, iy, ix] = INF
    case = PoolCase(x, clean.w, clean.scale, clean.shift)
    ref = relu64(pool(case.pre_pool())).float()
    inside = torch.zeros(M, 1, H // 2, W // 2, dtype=torch.bool)
    inside[n, 0] = _footprint(H, W, iy, ix)
    changed = (bits(ref) != bits(ref_clean)) & ~(torch.isnan(ref) & torch.isnan(ref_clean)).numpy()
    assert not changed[~inside.expand_as(ref).numpy()].any() and bool(torch.isinf(ref).any()) and bool(torch.isnan(ref).any())
    for dtype in DTYPES:
        got = nchw(case.run(device, dtype))
        nan = torch.isnan(ref)
        assert bool((torch.isnan(got) == nan).all())
        assert (bits(got)[~nan.numpy()] == bits(_as(ref, dtype))[~nan.numpy()]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_window_of_negative_values_gives_plus_zero(device, dtype):
    """Positive inputs and weights under a negative scale: all four r_q of every window are negative, and the
    output is +0 (all bits clear), not -0 and not the largest negative value."""
    g = torch.Generator().manual_seed(7)
    x = torch.randint(1, 5, (2, 64, 4, 6), generator=g).float()
    w = torch.randint(1, 5, (64, 64, 3, 3), generator=g).float()
    scale = torch.full((64,), -0.5)
    scale[::2] = 0.5                                                 # the even channels stay positive
    case = PoolCase(x, w, scale, torch.zeros(64))
    ref = case.reference()
    assert bool((ref[:, 1::2] == 0).all()) and bool((ref[:, ::2] > 0).all()) and bool((case.pre_pool()[:, 1::2] < 0).all())
    got = nchw(case.run(device, dtype))
    assert_same_bits(got, _as(ref, dtype))
    assert not bits(got[:, 1::2]).any()


# ----------------------------------------------------------------------------- guard bands, the C entry
def _c_call(x, pk, sc, sh, out, out_code, M, H, W, cin, cout):
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    ptr = lambda t: None if t is None else t.data_ptr()
    stream = _stream(next(t for t in (x, pk, sc, sh, out) if t is not None))
    return _lib.load().mvn_conv3x3_pool(ptr(x), ptr(pk), ptr(sc), ptr(sh), ptr(out), out_code, M, H, W, cin, cout, stream)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", SUBSET, ids=shape_id)
def test_no_reads_or_writes_outside_the_tensors(device, shape, dtype):
    """NaN bands around x, sentinel bands and a sentinel fill around out (C entry, caller's buffers): a read
    outside x would put a NaN into the result, a write outside out would break a band, an unwritten element
    would keep the sentinel."""
    from mvn_rocm import _lib, confidence
    M, cin, H, W, cout = shape
    case, ref = parity_pool(shape)
    big_x, xin = banded(cl2d(case.x, device))
    big_o, out, sentinel = banded_out((M, H // 2, W // 2, cout), dtype, device)
    pk = confidence.pack_conv3x3_pool_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    code = _c_call(xin, pk, sc, sh, out, _lib.MVN_DTYPE_BF16 if dtype == torch.bfloat16 else _lib.MVN_DTYPE_F32, M, H, W,
                   cin, cout)
    _lib.check(code, "mvn_conv3x3_pool")
    torch.cuda.synchronize()
    n = out.numel()
    assert bool((big_o[:BAND] == sentinel).all()) and bool((big_o[BAND + n:] == sentinel).all())
    assert not bool((big_o[BAND:BAND + n] == sentinel).any())
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(nchw(out), _as(ref, dtype))


def test_c_entry_argument_errors_and_the_empty_batch(device):
    from mvn_rocm import _lib, confidence
    shape = (2, 64, 3, 3, 64)
    case, ref = parity_pool(shape)
    x = cl2d(case.x, device)
    pk = confidence.pack_conv3x3_pool_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    out = torch.zeros(2 * 64 + 8, dtype=torch.float32, device=device)
    BF, F32 = _lib.MVN_DTYPE_BF16, _lib.MVN_DTYPE_F32
    ok = (x, pk, sc, sh, out, F32, 2, 3, 3, 64, 64)
    for i in range(5):                                               # a null pointer
        assert _c_call(*(None if j == i else a for j, a in enumerate(ok))) == -1
    bad = dict(out_code=((x, pk, sc, sh, out, 7, 2, 3, 3, 64, 64), {}),
               M=((x, pk, sc, sh, out, F32, -1, 3, 3, 64, 64), {}), H=((x, pk, sc, sh, out, F32, 2, 1, 3, 64, 64), {}),
               W=((x, pk, sc, sh, out, F32, 2, 3, 1, 64, 64), {}), cin=((x, pk, sc, sh, out, F32, 2, 3, 3, 96, 64), {}),
               cin_max=((x, pk, sc, sh, out, F32, 2, 3, 3, 2112, 64), {}), cout=((x, pk, sc, sh, out, F32, 2, 3, 3, 64, 32), {}),
               cout_max=((x, pk, sc, sh, out, F32, 2, 3, 3, 64, 576), {}),
               bytes_in=((x, pk, sc, sh, out, F32, 2 ** 20, 32, 32, 64, 64), {}),           # 2^31 bytes of bf16 input
               bytes_out=((x, pk, sc, sh, out, F32, 2 ** 17, 8, 8, 64, 512), {}),            # 2^32 bytes of f32 output
               x_off=((x.view(-1)[1:], pk, sc, sh, out, F32, 1, 3, 3, 64, 64), {}),
               scale_off=((x, pk, sc[1:], sh, out, F32, 2, 3, 3, 64, 64), {}), out_off=((x, pk, sc, sh, out[1:], F32, 2, 3, 3, 64, 64), {}))
    for name, (args, kw) in bad.items():
        assert _c_call(*args, **kw) == -1, name
    torch.cuda.synchronize()
    assert not bool(out.any())                                       # refused before any launch
    assert _c_call(x, pk, sc, sh, out, F32, 0, 3, 3, 64, 64) == 0    # the empty batch: MVN_OK, no launch
    torch.cuda.synchronize()
    assert not bool(out.any())
    y = confidence.conv3x3_pool(x[:0], pk, sc, sh, out_dtype=torch.float32)
    assert tuple(y.shape) == (0, 1, 1, 64) and y.dtype == torch.float32
    assert _c_call(x, pk, sc, sh, out, F32, 2, 3, 3, 64, 64) == 0
    torch.cuda.synchronize()
    assert_same_bits(nchw(out[:128].view(2, 1, 1, 64)), ref)


def _odd_view(t):
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    odd = buf[1:1 + t.numel()].view(t.shape)
    odd.copy_(t)
    assert odd.data_ptr() % 16 != 0
    return odd


def test_a_misaligned_view_equals_the_aligned_call(device):
    case, ref = parity_pool((3, 64, 4, 6, 64))
    got = case.run(device, torch.float32, x_dev=_odd_view(cl2d(case.x, device)))
    assert_same_bits(nchw(got), ref)


# ----------------------------------------------------------------------------- the dispatcher
def test_the_op_runs_through_the_dispatcher_and_replays_from_a_graph(device):
    from torch.fx.experimental.proxy_tensor import make_fx
    from mvn_rocm import _lib, confidence
    case, ref = parity_pool((1, 64, 5, 7, 128))
    x = cl2d(case.x, device)
    pk = confidence.pack_conv3x3_pool_weight(case.w.double()).to(device)
    sc, sh = case.scale.to(device), case.shift.to(device)
    y = torch.ops.mvn_rocm.conv3x3_pool(x, pk, sc, sh, _lib.MVN_DTYPE_F32)
    assert_same_bits(nchw(y), ref)

    def f(x, pk, sc, sh):
        return confidence.conv3x3_pool(x, pk, sc, sh, out_dtype=torch.bfloat16)

    gm = make_fx(f, tracing_mode="real")(x, pk, sc, sh)
    targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count(torch.ops.mvn_rocm.conv3x3_pool.default) == 1
    assert_same_bits(nchw(gm(x, pk, sc, sh)), ref.bfloat16())
