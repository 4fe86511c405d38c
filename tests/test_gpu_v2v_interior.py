"""The V2V's first pooled level on kernels (csrc/v2v_interior.hip): the channels-last 2x2x2 max
pool, the 64-channel 3x3x3 conv + folded BN + skip + ReLU, the fused upsample + skip add, the wide
block and V2VEval(half_res="kernels") (MI355X only).

The method is tests/v2v_kit.py's, on its 64-channel record: operands for which the kernel's f32
arithmetic is exact in any summation order (integers in [-4, 4], power-of-two scales, shifts in quarters; impulse
lattices with one product per output), compared bit for bit with the arithmetic contract of
include/mvn_hip.h restated in float64, plus random data against that restatement with the
contract's own bound.  Reads nothing outside the repository.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_parity_with_nans
from v2v_kit import (BAND, E2E_MULT, E2E_SIDE, IDENTITY, INF_VOXELS, MODE_NAME, N_BOX, NAN_VOXELS, NONE, POINTWISE,
                     UP_WIDE, WIDE, Res3DBlock, assert_same_bits, banded, bands_intact, bf16_full, bf16_operand_model, bf16r,
                     bits, box_mask, chain, chain_kernels, check_bound, cl, e2e_case, lattice_input, lattice_reference, ncdhw,
                     per_channel, randomise, stand_in_model)

CO = 64
SKIP_C = {NONE: 0, IDENTITY: 64, POINTWISE: 32}
# the method of tests/v2v_kit.py on the 64-channel level and its upsample
WideCase, pack_wide, exact_scale_shift = WIDE.case, WIDE.pack, WIDE.exact_scale_shift
integer_case, parity_case, random_case = WIDE.integer_case, WIDE.parity_case, WIDE.random_case
UpCase = UP_WIDE.case


def up_integer_case(B, V, seed, negative_pre):
    return UP_WIDE.integer_case(B, V, 32, seed, negative_pre)


# ----------------------------------------------------------------------------- pool
def pool_reference_bits(x_cl):
    """F.max_pool3d(x, 2, 2) on the CPU on the bf16 values held in f32 (NCDHW, contiguous); the
    result's bf16 bits are the upper halves of the f32 words (a max only selects)."""
    x = x_cl.cpu().float().permute(0, 4, 1, 2, 3).contiguous()
    y = F.max_pool3d(x, 2, 2).permute(0, 2, 3, 4, 1).contiguous()
    w = y.view(torch.int32).numpy().view(np.uint32)
    assert not (w & 0xFFFF).any()
    return (w >> 16).astype(np.uint16)


POOL_SHAPES = ((1, 2, 32), (3, 6, 32), (2, 16, 32), (1, 32, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("B,V,C", POOL_SHAPES)
def test_pool_equals_torch_bit_for_bit(device, B, V, C):
    """Random bf16 data, an all-negative volume (its largest value, never 0), signed zeros among
    small integers (ties: the first in scan order wins), and guard bands around input and output."""
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    g = torch.Generator().manual_seed(B * 100 + V + C)
    rnd = torch.randn(B, V, V, V, C, generator=g).bfloat16()
    neg = -(torch.rand(B, V, V, V, C, generator=g) + 0.01).bfloat16()
    small = torch.randint(-2, 3, (B, V, V, V, C), generator=g).float()
    small = torch.where((small == 0) & (torch.rand(small.shape, generator=g) < 0.5), -torch.zeros_like(small), small)
    small = small.bfloat16()
    assert int((bits(small) == 0x8000).sum()) > 0 and int((bits(small) == 0).sum()) > 0
    lib = _lib.load()
    for name, x in (("random", rnd), ("negative", neg), ("signed zeros", small)):
        ref = pool_reference_bits(x)
        if name == "negative":
            assert (ref & 0x8000).all() and (ref != 0x8000).all()
        big_x, xin = banded(x.to(device))
        big_o, out = banded(((B, V // 2, V // 2, V // 2, C), device))
        assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        _lib.check(lib.mvn_v2v_maxpool2(xin.data_ptr(), out.data_ptr(), B, V, C, _stream(xin)), "mvn_v2v_maxpool2")
        torch.cuda.synchronize()
        assert bands_intact(big_o, out.numel(), True), name
        assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
        assert (bits(out) == ref).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("B,V,C", POOL_SHAPES)
def test_pool_nonfinite_values_in_every_window_position(device, B, V, C):
    """NaN, +inf and -inf in each of the 8 window positions (one window each, the rest of the
    window finite; and whole windows of -inf): NaN gives NaN, +inf wins, -inf loses unless alone."""
    from mvn_rocm import v2v
    g = torch.Generator().manual_seed(7 * V + C)
    x = torch.randn(B, V, V, V, C, generator=g).bfloat16()
    Vo = V // 2
    nwin = Vo ** 3
    for k, val in enumerate((float("nan"), float("inf"), float("-inf"))):
        for p in range(8):
            wdx = (8 * k + p) % nwin                              # the window that takes this value
            wx, wy, wz = wdx // (Vo * Vo), (wdx // Vo) % Vo, wdx % Vo
            x[(k + p) % B, 2 * wx + (p >> 2), 2 * wy + ((p >> 1) & 1), 2 * wz + (p & 1), (5 * p + k) % C] = val
    x[B - 1, V - 2:, V - 2:, V - 2:, C - 1] = float("-inf")      # a window of -inf alone
    ref = pool_reference_bits(x)
    assert (ref == 0x7FC0).any() and (ref == 0x7F80).any() and ref[B - 1, -1, -1, -1, C - 1] == 0xFF80
    y = v2v.max_pool2_cl(x.to(device))
    assert tuple(y.shape) == (B, Vo, Vo, Vo, C) and y.dtype == torch.bfloat16
    assert (bits(y) == ref).all()


@pytest.mark.gpu
def test_pool_empty_batch_and_noncontiguous_input(device):
    from mvn_rocm import v2v
    y = v2v.max_pool2_cl(torch.zeros(0, 4, 4, 4, 8, dtype=torch.bfloat16, device=device))
    assert tuple(y.shape) == (0, 2, 2, 2, 8)
    x = torch.randn(2, 32, 6, 6, 6, generator=torch.Generator().manual_seed(1)).bfloat16()
    view = x.to(device).permute(0, 2, 3, 4, 1)
    assert not view.is_contiguous()
    assert (bits(v2v.max_pool2_cl(view)) == pool_reference_bits(view.contiguous())).all()


# (cin, mode): the issue's four and the one Res3DBlock(32, 64)'s second conv takes
WIDE_KINDS = ((32, NONE), (32, POINTWISE), (64, NONE), (64, IDENTITY), (64, POINTWISE))
WIDE_IDS = [f"{c}_{MODE_NAME[m]}" for c, m in WIDE_KINDS]


# ----------------------------------------------------------------------------- wide conv: exact parity
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", WIDE_KINDS, ids=WIDE_IDS)
@pytest.mark.parametrize("B,V", ((1, 16), (3, 16), (1, 32)))
def test_wide_exact_parity_integer_inputs(device, B, V, cin, mode):
    """Every element equals the CPU reference bit for bit.  Partial sums stay below
    27 * 64 * 16 + 32 * 16 < 2^24.  The x column is cut into segments of 2 tiles at these sizes
    (fewer than 256 blocks), so every segment start but the first loads its halo mid-volume."""
    case, ref, r = parity_case(B, V, cin, mode)
    assert all(not torch.equal(case.x[0], case.x[f]) for f in range(1, B))
    partial = float(F.conv3d(case.x.abs(), case.w.abs(), None, padding=1).max())
    print(f"largest sum of |x w|: {partial:.0f}")
    assert partial <= 27 * cin * 16
    pos = r[r > 0].float()
    low = bits(pos) & 0xFFFF
    assert pos.numel() >= 0.25 * r.numel()
    assert (low != 0).sum() >= 0.10 * pos.numel() and (low == 0x8000).any()     # rounding and ties are tested
    y = case.run(device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, V, V, V, CO)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
def test_wide_exact_parity_twelve_tiles_per_column(device):
    """(B, V) = (2, 48), 64 -> 64 with the identity skip: 12 tiles per column in segments of 3 (36
    columns: halved twice), one period of the 6-slot x-slice ring per block, and tiles with
    neighbours on every side in every axis."""
    case, ref, _ = parity_case(2, 48, 64, IDENTITY)
    assert_same_bits(ncdhw(case.run(device)), ref)


@pytest.mark.gpu
def test_wide_whole_column_walk(device):
    """32 frames at V = 32 are 256 columns, so no column is cut: each block walks its 8 tiles, 2 2/3
    periods of the x-slice ring, the staged slices of every tile but the last in use.  The frames
    repeat two frames of data, so the CPU reference is two frames' conv."""
    case, ref, _ = parity_case(2, 32, 32, NONE)
    xd = cl(case.x, device).repeat(16, 1, 1, 1, 1)
    y = case.run(device, xd)
    assert tuple(y.shape) == (32, 32, 32, 32, CO)
    assert_same_bits(ncdhw(y), ref.repeat(16, 1, 1, 1, 1))


# ----------------------------------------------------------------------------- wide conv: impulses
LATTICE_B, LATTICE_V, LATTICE_OFFS = 2, 16, (0, 2)


@pytest.mark.parametrize("cin", (32, 64))
def test_wide_impulse_lattices_cover_every_packing_slot(cin):
    """No GPU: together the lattice cases read every (tap, ci) of the weights for all 64 outputs,
    which is every slot of the packed layout.  An impulse at p in channel ci reaches output p - d + 1
    through tap d, if that output is inside the volume."""
    V = LATTICE_V
    hit = torch.zeros(27, cin, dtype=torch.bool)
    for off in LATTICE_OFFS:
        x = lattice_input(cin, off, torch.Generator().manual_seed(1))
        for _, ci, px, py, pz in (x != 0).nonzero().tolist():
            for tap in range(27):
                d = (tap // 9, (tap // 3) % 3, tap % 3)
                if all(0 <= p + 1 - t < V for p, t in zip((px, py, pz), d)):
                    hit[tap, ci] = True
    assert bool(hit.all())


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (32, 64))
@pytest.mark.parametrize("off", LATTICE_OFFS)
def test_wide_impulse_lattice_full_mantissa(device, cin, off):
    """One product per output (asserted), 8-bit x 8-bit significands, V = 16: pins the
    (tap, ci, co) <-> packed-weight map, the channel-chunk swizzle and the border clipping one
    product at a time; the two offsets together read every packing slot (asserted above)."""
    g = torch.Generator().manual_seed(7 * LATTICE_V + off + cin)
    w = (torch.randn((CO, cin, 3, 3, 3), generator=g) * 0.05).bfloat16().float()
    scale = torch.randn(CO, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    x = lattice_input(cin, off, g)
    r32 = lattice_reference(x, w, scale, 1)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    y = WideCase(x, w, scale, torch.zeros(CO)).run(device)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
def test_wide_impulse_pointwise_skip_weights(device):
    """The pointwise skip's packed weights one product at a time: x is zero, every skip voxel has
    one of its 32 channels set."""
    B, V = 2, 16
    g = torch.Generator().manual_seed(99)
    ws = (torch.randn((CO, 32), generator=g) * 0.3).bfloat16().float()
    scale_s = torch.randn(CO, generator=g)
    scale_s[0], scale_s[1] = -scale_s[0].abs(), scale_s[1].abs()
    chs = torch.randint(0, 32, (B, 1, V, V, V), generator=g)
    assert len(set(chs.flatten().tolist())) == 32
    skip = torch.zeros(B, 32, V, V, V).scatter_(1, chs, bf16_full((B, 1, V, V, V), g))
    r32 = lattice_reference(skip, ws.view(CO, 32, 1, 1, 1), scale_s, 0)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    for cin in (32, 64):
        w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).float()
        case = WideCase(torch.zeros(B, cin, V, V, V), w, exact_scale_shift(3)[0], torch.zeros(CO), POINTWISE, skip, ws,
                        scale_s, torch.zeros(CO))
        assert_same_bits(ncdhw(case.run(device)), ref)


@pytest.mark.gpu
def test_wide_v128_sparse_impulses(device):
    """The largest volume the entry takes (V = 128, B = 1, 64 -> 64): (gy * V + gz) * 8 + c fills
    the staging descriptor's 17 bits and a frame is 2^28 bytes.  Sparse impulses (corners, faces,
    tile seams, the last voxels) with integer weights; the reference is each impulse's clipped
    3^3 x 64 block of weights, everything else relu(shift) = 0 — every element is compared."""
    from mvn_rocm import v2v
    V, cin = 128, 64
    g = torch.Generator().manual_seed(128)
    w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).float()
    scale = exact_scale_shift(5)[0]
    pts = [(0, 0, 0), (127, 127, 127), (127, 0, 64), (0, 127, 15), (63, 64, 16), (64, 63, 111), (3, 8, 127),
           (4, 7, 0), (100, 120, 124), (124, 124, 4), (31, 95, 47), (96, 32, 80)]
    pts += [tuple(int(v) for v in torch.randint(0, 43, (3,), generator=g) * 3) for _ in range(20)]
    pts = sorted(set(pts))
    for i, p in enumerate(pts):
        for q in pts[:i]:
            assert max(abs(a - b) for a, b in zip(p, q)) >= 3      # disjoint 3^3 boxes: one product per output
    x = torch.zeros(1, V, V, V, cin, dtype=torch.bfloat16, device=device)
    ref = torch.zeros(1, V, V, V, CO, dtype=torch.bfloat16, device=device)
    for n, (px, py, pz) in enumerate(pts):
        ch, val = (7 * n + 3) % cin, float((n % 4) + 1)
        x[0, px, py, pz, ch] = val
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    ox, oy, oz = px + 1 - dx, py + 1 - dy, pz + 1 - dz        # tap (dx, dy, dz) reads voxel o + d - 1
                    if 0 <= ox < V and 0 <= oy < V and 0 <= oz < V:
                        r = val * w[:, ch, dx, dy, dz] * scale
                        ref[0, ox, oy, oz] = torch.where(r <= 0, torch.zeros_like(r), r).bfloat16().to(device)
    y = v2v.v2v_conv3_wide(x, pack_wide(w, device), scale.to(device), torch.zeros(CO, device=device))
    same = torch.equal(y.view(torch.int16), ref.view(torch.int16))
    nbad = 0 if same else int((y.view(torch.int16) != ref.view(torch.int16)).sum())
    assert int((ref != 0).sum()) > 1000
    del x, y, ref
    torch.cuda.empty_cache()
    assert same, f"{nbad} elements differ in their bits"


# ----------------------------------------------------------------------------- wide conv: frames, borders
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((64, IDENTITY), (32, POINTWISE)), ids=("identity", "pointwise"))
def test_wide_frames_do_not_mix(device, cin, mode):
    """In a B = 3 call each frame equals its own B = 1 call bit for bit."""
    case, ref, _ = parity_case(3, 16, cin, mode)
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_same_bits(ncdhw(y), ref)
    for f in range(3):
        assert_same_bits(case.run(device, xd[f:f + 1].clone(), sd[f:f + 1].clone()), y[f:f + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (32, 64))
def test_wide_borders_are_zero_padding(device, cin):
    """All-ones frame between two NaN frames, weights of ones: exactly the clipped tap count x Cin
    at faces, edges and corners; a tap that reached into a neighbouring frame would show as NaN."""
    V = 32
    x = torch.full((3, cin, V, V, V), float("nan"))
    x[1] = 1.0
    y = ncdhw(WideCase(x, torch.ones(CO, cin, 3, 3, 3), torch.ones(CO), torch.zeros(CO)).run(device)).float()
    n = torch.full((V,), 3.0)
    n[0] = n[-1] = 2.0
    want = (n.view(V, 1, 1) * n.view(1, V, 1) * n.view(1, 1, V) * cin).expand(CO, V, V, V)
    assert torch.equal(y[1], want)
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[2]).all())


# ----------------------------------------------------------------------------- wide conv: non-finite voxels
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (32, 64))
def test_wide_nonfinite_input_voxels_follow_torch(device, cin):
    """A NaN input voxel is NaN in exactly its clipped 3^3 box, all 64 channels; +-inf voxels
    (positive weights, scales of both signs) come out +inf or 0; the clean frame equals its run
    alone."""
    V = 32
    case = integer_case(3, V, cin, NONE, seed=77 + cin)
    for n, (px, py, pz) in enumerate(NAN_VOXELS):
        case.x[0, (5 * n + 2) % cin, px, py, pz] = float("nan")
    g = torch.Generator().manual_seed(78)
    for px, py, pz, ch, val in INF_VOXELS:
        case.x[2, ch, px, py, pz] = val
        case.w[:, ch] = torch.randint(1, 5, (CO, 3, 3, 3), generator=g).float()       # no 0 * inf
    ref, _ = case.reference()
    ref = ref.float()
    nan_ref = torch.isnan(ref).numpy()
    assert (nan_ref[0] == box_mask(V, NAN_VOXELS, 1)[None]).all() and not nan_ref[1:].any()
    assert torch.isinf(ref[2]).any() and not torch.isinf(ref[:2]).any()
    xd = cl(case.x, device)
    y = case.run(device, xd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert int(torch.isnan(y).sum()) == CO * N_BOX
    assert_same_bits(case.run(device, xd[1:2].clone()), y[1:2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (IDENTITY, POINTWISE), ids=("identity", "pointwise"))
def test_wide_nonfinite_skip_voxels_reach_their_own_voxel(device, mode):
    V = 32
    case = integer_case(3, V, 64, mode, seed=91 + mode)
    sc = SKIP_C[mode]
    for n, (px, py, pz) in enumerate(NAN_VOXELS):
        case.skip[0, (5 * n + 2) % sc, px, py, pz] = float("nan")
    for px, py, pz, ch, val in INF_VOXELS:
        case.skip[2, ch, px, py, pz] = val
    if mode == POINTWISE:
        g = torch.Generator().manual_seed(92)
        for *_, ch, _ in INF_VOXELS:
            case.ws[:, ch] = torch.randint(1, 5, (CO,), generator=g).float()           # no 0 * inf
    ref, _ = case.reference()
    ref = ref.float()
    nan_ref = torch.isnan(ref).numpy()
    if mode == IDENTITY:
        assert int(nan_ref.sum()) == len(NAN_VOXELS) and not nan_ref[1:].any()
    else:
        assert (nan_ref[0] == box_mask(V, NAN_VOXELS, 0)[None]).all() and not nan_ref[1:].any()
    assert torch.isinf(ref[2]).any() and not torch.isinf(ref[:2]).any()
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])


# ----------------------------------------------------------------------------- wide conv: guards
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((64, IDENTITY), (32, POINTWISE), (64, POINTWISE)),
                         ids=("identity", "pointwise32", "pointwise64"))
def test_wide_no_reads_or_writes_outside_the_tensors(device, cin, mode):
    """The C entry on slices of larger buffers (V = 16, B = 2: every tile touches the border): the
    NaN bands around x and skip must not reach the result, the sentinel bands around the output must
    be intact, with no sentinel left inside it."""
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    B, V = 2, 16
    case, ref, _ = parity_case(3, V, cin, mode)
    a = case.args(device, cl(case.x[:B], device), cl(case.skip[:B], device))
    big_x, xin = banded(a[0])
    big_s, sin = banded(a[4])
    big_o, out = banded(((B, V, V, V, CO), device))
    pw = a[5:] if mode == POINTWISE else [None] * 3
    assert xin.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = _lib.load().mvn_v2v_conv3_wide(xin.data_ptr(), cin, a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), mode,
                                          sin.data_ptr(), SKIP_C[mode],
                                          *[t.data_ptr() if t is not None else None for t in pw], out.data_ptr(), B, V,
                                          _stream(xin))
    _lib.check(code, "mvn_v2v_conv3_wide")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref[:B])
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())


# ----------------------------------------------------------------------------- wide conv: random data
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((32, POINTWISE), (64, IDENTITY)), ids=("32to64_pointwise", "64to64_identity"))
@pytest.mark.parametrize("V", (16, 32))
def test_wide_random_data_against_float64_restatement(device, V, cin, mode):
    """conv1 (skip NONE) and conv2 (the block's skip) on random bf16 data against the float64
    restatement with the kernel's own roundings; conv2's restatement reads the hidden volume the
    GPU wrote.  Measured on the MI355X: 0.824-0.926 of the bar."""
    B = 2 if V == 16 else 1
    c1 = random_case(B, V, cin, NONE, seed=10 * V + cin)
    xd = cl(c1.x, device)
    h = c1.run(device, xd)
    check_bound(c1, ncdhw(h).float(), f"wide conv1 V={V} cin={cin}")
    c2 = random_case(B, V, 64, mode, seed=10 * V + cin + 1, x=ncdhw(h).float())
    c2.skip = c1.x
    y = c2.run(device, h, xd)
    check_bound(c2, ncdhw(y).float(), f"wide conv2 V={V} {MODE_NAME[mode]}")


# ----------------------------------------------------------------------------- upsample
@pytest.mark.gpu
@pytest.mark.parametrize("negative_pre", (False, True), ids=("mixed", "negative_pre_positive_skip"))
@pytest.mark.parametrize("B,V", ((1, 16), (3, 16), (1, 32)))
def test_upsample_exact_parity_integer_inputs(device, B, V, negative_pre):
    case = up_integer_case(B, V, 300 * B + V + int(negative_pre), negative_pre)
    assert float(F.conv_transpose3d(case.x.abs(), case.w.abs(), None, stride=2).max()) <= 64 * 16
    ref, pre = case.reference()
    if negative_pre:
        assert bool((pre <= 0).all()) and float((pre < 0).double().mean()) > 0.9
        assert torch.equal(ref.float(), case.skip)               # relu first: the skip alone
        late = torch.where(pre + case.skip.double() <= 0, torch.zeros_like(pre), pre + case.skip.double())
        assert float((late.float() != ref.float()).float().mean()) > 0.5      # a ReLU after the add differs
    else:
        assert 0.2 < float((pre > 0).double().mean()) < 0.8
        assert not bool((torch.signbit(pre) & (pre == 0)).any())
    y = case.run(device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, 2 * V, 2 * V, 2 * V, 32)
    assert_same_bits(ncdhw(y), ref)
    case.skip = None                                            # the skip = NULL form: no add
    assert_same_bits(ncdhw(case.run(device)), case.reference()[0])


@pytest.mark.gpu
def test_upsample_one_hot_channel_lattice(device):
    """Voxel v carries only channel v mod 64, full-significand weights: one product per output, and
    the 16^3 voxels of a frame hit every (ci, co, dx, dy, dz) weight."""
    B, V = 2, 16
    g = torch.Generator().manual_seed(17)
    w = (torch.randn((64, 32, 2, 2, 2), generator=g) * 0.2).bfloat16().float()
    scale = torch.randn(32, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    ch = ((torch.arange(B * V ** 3).view(B, 1, V, V, V) + 7 * torch.arange(B).view(B, 1, 1, 1, 1)) % 64)
    x = torch.zeros(B, 64, V, V, V).scatter_(1, ch, bf16_full((B, 1, V, V, V), g))
    assert int((x != 0).sum(dim=1).max()) == 1 and len(set(ch.flatten().tolist())) == 64
    r32 = (F.conv_transpose3d(x.double(), w.double(), None, stride=2) * per_channel(scale)).float()
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    y = UpCase(x, w, scale, torch.zeros(32)).run(device)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
def test_upsample_nonfinite_voxels(device):
    """A non-finite input voxel reaches exactly its own 2x2x2 outputs (all 32 channels for a NaN),
    a non-finite skip voxel exactly itself; the clean frame equals its run alone."""
    B, V = 3, 16
    case = up_integer_case(B, V, 55, False)
    vox = ((0, 0, 0), (15, 15, 15), (3, 8, 15), (4, 7, 0), (8, 8, 8))
    for n, (px, py, pz) in enumerate(vox):
        case.x[0, (11 * n + 2) % 64, px, py, pz] = float("nan")
    case.x[0, 5, 10, 2, 3] = float("inf")
    case.w[5] = case.w[5].abs() + 1.0                            # no 0 * inf
    case.skip[2, 7, 31, 0, 17] = float("nan")
    case.skip[2, 9, 5, 6, 7] = float("inf")
    case.skip[2, 11, 20, 21, 22] = float("-inf")
    ref, _ = case.reference()
    ref = ref.float()
    nan_ref = torch.isnan(ref).numpy()
    own = np.zeros((2 * V,) * 3, bool)
    for px, py, pz in vox:
        own[2 * px:2 * px + 2, 2 * py:2 * py + 2, 2 * pz:2 * pz + 2] = True
    assert (nan_ref[0] == own[None]).all() and not nan_ref[1].any() and int(nan_ref[2].sum()) == 1
    assert int(torch.isinf(ref[2]).sum()) == 2 and not torch.isinf(ref[1]).any()
    inf0 = torch.isinf(ref[0]).any(dim=0).numpy()
    assert inf0.any() and inf0[20:22, 4:6, 6:8].sum() == inf0.sum()
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])


@pytest.mark.gpu
def test_upsample_no_reads_or_writes_outside_the_tensors(device):
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    B, V = 2, 16
    case = up_integer_case(B, V, 66, False)
    ref, _ = case.reference()
    big_x, xin = banded(cl(case.x, device))
    big_s, sin = banded(cl(case.skip, device))
    big_o, out = banded(((B, 2 * V, 2 * V, 2 * V, 32), device))
    w, sc, sh = case.params(device)
    code = _lib.load().mvn_v2v_upsample2(xin.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), sin.data_ptr(),
                                         out.data_ptr(), B, V, _stream(xin))
    _lib.check(code, "mvn_v2v_upsample2")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref)
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("V", (16, 32))
def test_upsample_random_data_against_float64_restatement(device, V):
    """Random bf16 data: |got - ref| <= 2^-8 |ref| + (64 + 4) 2^-24 S, S the sum of the absolute
    terms (half a bf16 ulp of the result plus the f32 summation, fma and add roundings).  Measured
    on the MI355X: 0.993 and 0.994 of the bar, nearly all of it the half ulp of the one bf16
    rounding."""
    B = 2 if V == 16 else 1
    g = torch.Generator().manual_seed(V)
    x = bf16r(torch.randn(B, 64, V, V, V, generator=g))
    w = bf16r(torch.randn(64, 32, 2, 2, 2, generator=g) * 0.15)
    scale = (0.75 + 0.5 * torch.rand(32, generator=g)) * torch.where(torch.arange(32) % 5 == 2, -1.0, 1.0)
    case = UpCase(x, w, scale, 0.2 * torch.randn(32, generator=g), bf16r(torch.randn(B, 32, 2 * V, 2 * V, 2 * V, generator=g)))
    _, ref = case.pre_round(exact=False)
    S = F.conv_transpose3d(x.double().abs(), w.double().abs(), None, stride=2) * per_channel(scale).abs() \
        + per_channel(case.shift).abs() + case.skip.double().abs()
    bar = 2.0 ** -8 * ref.abs() + (64 + 4) * 2.0 ** -24 * S
    got = ncdhw(case.run(device)).double()
    frac = float(((got - ref).abs() / bar).max())
    print(f"upsample V={V}: worst |got - ref| / bar = {frac:.4f}")
    assert frac <= 1.0


# ----------------------------------------------------------------------------- wide block
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (32, 64), ids=("32to64_pointwise", "64to64_identity"))
def test_wide_block_equals_the_two_launches(device, cin):
    """res3d_block_wide and Res3DBlockWideCL.from_reference of a stand-in block (Xavier weights,
    randomised BN, conv biases) equal conv1 (skip NONE) then conv2 (the block's skip) bit for bit,
    and stay within the block-level bar of the float64 restatement of the stock block on the
    kernel's operands: conv2's bar on the hidden volume the GPU wrote (conv1 checked the same way)."""
    from mvn_rocm import v2v
    B, V = 2, 16
    block = randomise(Res3DBlock(cin, CO), seed=40 + cin)
    p = v2v.fold_res3d_block_wide(block, device=device)
    assert (p.skip_packed is None) == (cin == 64)
    x = bf16r(torch.randn(B, cin, V, V, V, generator=torch.Generator().manual_seed(cin)))
    xd = cl(x, device)
    h = v2v.v2v_conv3_wide(xd, p.packed1, p.scale1, p.shift1)
    two = v2v.v2v_conv3_wide(h, p.packed2, p.scale2, p.shift2, xd, p.skip_packed, p.skip_scale, p.skip_shift)
    assert_same_bits(v2v.res3d_block_wide(xd, p), two)
    assert_same_bits(v2v.Res3DBlockWideCL.from_reference(block, device=device)(xd), two)
    pc = v2v.fold_res3d_block_wide(block, device="cpu")
    rb = block.res_branch
    with torch.no_grad():
        c1 = WideCase(x, bf16r(rb[0].weight), pc.scale1, pc.shift1)
        check_bound(c1, ncdhw(h).float(), f"block conv1 cin={cin}")
        c2 = WideCase(ncdhw(h).float(), bf16r(rb[3].weight), pc.scale2, pc.shift2, POINTWISE if cin == 32 else IDENTITY, x)
        if cin == 32:
            c2.ws, c2.scale_s, c2.shift_s = bf16r(block.skip_con[0].weight.view(CO, 32)), pc.skip_scale, pc.skip_shift
        check_bound(c2, ncdhw(two).float(), f"block conv2 cin={cin}")
        stock = block(x)
    err = float((ncdhw(two).float() - stock).abs().max() / stock.abs().max())
    print(f"wide block against the stock f32 modules: {err:.3e} of max|ref|")
    assert err <= 2.0 ** -6                 # as the 32-channel block: two bf16 roundings deep
    empty = torch.zeros((0, V, V, V, cin), dtype=torch.bfloat16, device=device)
    assert tuple(v2v.res3d_block_wide(empty, p).shape) == (0, V, V, V, CO)
    view = x.bfloat16().to(device).permute(0, 2, 3, 4, 1)       # NCDHW storage: copied
    assert not view.is_contiguous()
    assert_same_bits(v2v.res3d_block_wide(view, p), two)


# ----------------------------------------------------------------------------- wiring
@pytest.mark.gpu
def test_v2veval_half_res_wiring(device):
    """V = 32, B = 2, the stand-in model: with half_res="kernels" trunk equals the chain written out
    here and forward equals v2v_head_softargmax on it, bit for bit; with half_res="torch" trunk
    still equals the existing chain."""
    from mvn_rocm import v2v, volumetric
    B, V = 2, 32
    m = stand_in_model()
    ev = v2v.V2VEval.from_reference(m, device=device, half_res="kernels")
    vol = bf16r(torch.randn(B, V, V, V, 32, generator=torch.Generator().manual_seed(9))).bfloat16().to(device)
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0], [-150.0, 40.0, 1000.0]]), 2500.0, V,
                                            theta=[0.0, 0.7], device=device)
    with torch.no_grad():
        want = chain_kernels(m, ev, vol)
        got = ev.trunk(vol)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, V, V, V, 32)
        assert_same_bits(got, want)
        kp, out = ev(vol, coords, 3.0)
        kp_w, out_w = v2v.v2v_head_softargmax(want, *v2v.fold_v2v_head(m.back_layers[1], m.back_layers[2], m.output_layer,
                                                                       device=device),
                                              coords, multiplier=3.0, channels_last=True)
        assert_same_bits(kp, kp_w)
        assert_same_bits(out, out_w)
        evt = v2v.V2VEval.from_reference(m, device=device, half_res="torch")
        old = chain(m, evt, vol)
        assert_same_bits(evt.trunk(vol), old)
        assert_same_bits(v2v.V2VEval.from_reference(m, device=device).trunk(vol), old)      # the default
    assert not torch.equal(got, old)                              # the two paths round differently


# ----------------------------------------------------------------------------- semantics
@pytest.mark.gpu
def test_v2veval_half_res_against_the_f32_modules(device):
    """The case of test_v2veval_against_the_f32_modules (V = 32, B = 1, blob input, multiplier 10):
    trunk error / max|ref| and joints error / cuboid side against the f32 CPU stand-in, in one run,
    for half_res="kernels", half_res="torch" and the CPU stand-in with bf16 conv operands.  The bar:
    err_kernels <= 2 x max(err_torch, err_bf16_cpu) for both quantities (both yardsticks come from
    code that is older than the half-resolution kernels; 2 is the margin of the test this mirrors).
    Measured on the MI355X, trunk / joints: kernels 6.263e-3 / 9.682e-3, torch
    6.630e-3 / 5.979e-3, bf16 operands on the CPU 4.179e-3 / 9.090e-3.  The trunk is no worse than
    with the torch level; the joints move from the torch path's 0.66 x to 1.07 x of what bf16
    operands alone cost (the 64-channel blocks round their outputs to bf16 where the torch path
    kept f32, and the fused upsample rounds once), 0.53 of the bar."""
    from mvn_rocm import v2v
    from oracle import restate_torch
    m = stand_in_model()
    x, coords = e2e_case(device)
    cc = coords.cpu()
    with torch.no_grad():
        def cpu(model):
            t = model.back_layers[0](model.encoder_decoder(model.front_layers(x)))
            logits = model.output_layer(model.back_layers[2](model.back_layers[1](t)))
            kp, _ = restate_torch.integrate_tensor_3d_with_coordinates(logits * E2E_MULT, cc, softmax=True)
            return t, kp
        t_ref, kp_ref = cpu(m)
        t_b, kp_b = cpu(bf16_operand_model(m))
        vol = x.bfloat16().permute(0, 2, 3, 4, 1).contiguous().to(device)
        res = {}
        for how in ("kernels", "torch"):
            ev = v2v.V2VEval.from_reference(m, device=device, half_res=how)
            t = ncdhw(ev.trunk(vol)).float()
            kp, _ = ev(vol, coords, E2E_MULT)
            res[how] = (float((t - t_ref).abs().max() / t_ref.abs().max()),
                        float((kp.cpu() - kp_ref).abs().max()) / E2E_SIDE)
    res["bf16_cpu"] = (float((t_b - t_ref).abs().max() / t_ref.abs().max()), float((kp_b - kp_ref).abs().max()) / E2E_SIDE)
    for how, (tr, jo) in res.items():
        print(f"half-res semantics, {how}: trunk {tr:.3e} of max|ref|, joints {jo:.3e} of the side")
    for q in (0, 1):
        assert res["kernels"][q] <= 2 * max(res["torch"][q], res["bf16_cpu"][q])
