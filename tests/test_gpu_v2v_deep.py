"""The V2V's 128-channel levels on kernels (csrc/v2v_deep.hip): the 3x3x3 conv with
128 output channels and the 128-channel upsample at any extent D in [1, 64], the block, and
V2VEval(half_res="kernels", deep="kernels") (MI355X only).

The method is tests/v2v_kit.py's, on its 128-channel record: operands for which the kernel's f32
arithmetic is exact in any summation order (integers in [-4, 4]: sums stay below 27 * 128 * 16 < 2^24; scales
+-2^k, shifts multiples of 1/4), compared bit for bit against torch on the CPU.

The kernels flatten the voxels of all frames into groups of 16, so the shapes are the small ones
at which a group spans z-rows, x-slices and frames, and the last group is ragged: (B, D) = (1, 1),
(3, 1), (2, 2), (3, 3), (1, 4), (3, 5), (2, 8), (1, 16), with 1, 3, 16, 81, 64, 375, 1024 and 4096
voxels.  The conv picks its wave tile (voxel groups x channel tiles = 1 x 2, 2 x 4 or 4 x 4) by
the number of groups: all of the above run 1 x 2, so (1, 26) and (1, 33) (1099 and 2247 groups, both
ragged in the group and in the tile) run the other two.  Reads nothing outside the repository.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_parity_with_nans
from v2v_kit import (BAND, DEEP, E2E_MULT, E2E_SIDE, IDENTITY, MODE_NAME, NONE, POINTWISE, UP_DEEP, Res3DBlock,
                     Upsample3DBlock, assert_same_bits, banded, bands_intact, bf16_full, bf16_operand_model, bf16r, bits,
                     box_mask, chain_deep, chain_kernels, check_bound, cl, e2e_case, lattice_input, lattice_reference,
                     ncdhw, per_channel, randomise, stand_in_model)

CO = 128
SKIP_C = {NONE: 0, IDENTITY: 128, POINTWISE: 64}
# the method of tests/v2v_kit.py on the 128-channel level and its upsample
DeepCase, pack_deep, exact_scale_shift = DEEP.case, DEEP.pack, DEEP.exact_scale_shift
integer_case, parity_case, random_case = DEEP.integer_case, DEEP.parity_case, DEEP.random_case
UpCase, up_integer_case = UP_DEEP.case, UP_DEEP.integer_case
SHAPES = ((1, 1), (3, 1), (2, 2), (3, 3), (1, 4), (3, 5), (2, 8), (1, 16))
DEEP_KINDS = ((64, NONE), (64, POINTWISE), (128, NONE), (128, IDENTITY), (128, POINTWISE))
DEEP_IDS = [f"{c}_{MODE_NAME[m]}" for c, m in DEEP_KINDS]


# ----------------------------------------------------------------------------- conv: exact parity
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", DEEP_KINDS, ids=DEEP_IDS)
@pytest.mark.parametrize("B,D", SHAPES)
def test_deep_exact_parity_integer_inputs(device, B, D, cin, mode):
    """Every element equals the CPU reference bit for bit; sums of |x w| stay below 2^24 (asserted
    on the CPU), so the accumulation order cannot matter."""
    case, ref, r = parity_case(B, D, cin, mode)
    assert all(not torch.equal(case.x[0], case.x[f]) for f in range(1, B))
    partial = case.abs_sum()
    print(f"largest sum of |x w|: {partial:.0f}")
    assert partial <= 27 * cin * 16 < 2 ** 24
    if B * D ** 3 >= 64:
        pos = r[r > 0].float()
        assert pos.numel() >= 0.25 * r.numel() and ((bits(pos) & 0xFFFF) != 0).any()    # the bf16 rounding is tested
    y = case.run(device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, D, D, D, CO)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,cin,mode", ((1, 26, 128, IDENTITY), (1, 33, 64, POINTWISE)), ids=("tile2x4", "tile4x4"))
def test_deep_exact_parity_larger_wave_tiles(device, B, D, cin, mode):
    """17,576 and 35,937 voxels: 1099 and 2247 groups, where the launch takes the 2 x 4 and the
    4 x 4 wave tile (from 1024 and 2048 groups on).  Neither count is a multiple of 16, nor the group
    counts of the tile's 2 or 4 groups: the last wave's last groups are partly or wholly past the end."""
    case, ref, _ = parity_case(B, D, cin, mode)
    n = B * D ** 3
    assert n % 16 != 0 and -(-n // 16) % (2 if D == 26 else 4) != 0
    assert (1024 <= -(-n // 16) < 2048) == (D == 26)
    assert_same_bits(ncdhw(case.run(device)), ref)


# ----------------------------------------------------------------------------- conv: impulses
LATTICE_B, LATTICE_D, LATTICE_OFFS = 2, 16, (0, 2)


def skip_lattice(g):
    """Every voxel of a (2, 5^3) skip volume carries one of its 64 channels."""
    B, D = 2, 5
    chs = (torch.arange(B * D ** 3).view(B, 1, D, D, D) * 3 + 1) % 64
    return chs, torch.zeros(B, 64, D, D, D).scatter_(1, chs, bf16_full((B, 1, D, D, D), g))


def up_lattice(B, D, g):
    """Voxel v carries only channel (v + 7 b) mod 128."""
    ch = (torch.arange(B * D ** 3).view(B, 1, D, D, D) + 7 * torch.arange(B).view(B, 1, 1, 1, 1)) % 128
    return ch, torch.zeros(B, 128, D, D, D).scatter_(1, ch, bf16_full((B, 1, D, D, D), g))


def test_deep_impulse_lattices_cover_every_weight_slot():
    """No GPU: the lattice cases below read every (tap, ci) of the conv's weights for all 128
    outputs (an impulse at p in channel ci reaches output p - d + 1 through tap d, if that output is
    inside the volume), every (kp, ci) of the pointwise skip's 64 input channels and every
    (offset, ci) of the upsample's 128 (each voxel writes all 8 offsets and every output channel):
    together with all output channels being compared, every slot of the three packed layouts."""
    D = LATTICE_D
    for cin in (64, 128):
        hit = torch.zeros(27, cin, dtype=torch.bool)
        for off in LATTICE_OFFS:
            x = lattice_input(cin, off, torch.Generator().manual_seed(1))
            for _, ci, px, py, pz in (x != 0).nonzero().tolist():
                for tap in range(27):
                    d = (tap // 9, (tap // 3) % 3, tap % 3)
                    if all(0 <= p + 1 - t < D for p, t in zip((px, py, pz), d)):
                        hit[tap, ci] = True
        assert bool(hit.all())
    chs, skip = skip_lattice(torch.Generator().manual_seed(1))
    assert set(chs.flatten().tolist()) == set(range(64)) and int((skip != 0).sum(dim=1).min()) == 1
    ch, x = up_lattice(2, 5, torch.Generator().manual_seed(1))
    assert set(ch.flatten().tolist()) == set(range(128)) and int((x != 0).sum(dim=1).min()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (64, 128))
@pytest.mark.parametrize("off", LATTICE_OFFS)
def test_deep_impulse_lattice_full_mantissa(device, cin, off):
    """One product per output (asserted), 8-bit x 8-bit significands: pins the (tap, ci, co) <->
    packed-weight map and the border clipping one product at a time."""
    g = torch.Generator().manual_seed(7 * LATTICE_D + off + cin)
    w = (torch.randn((CO, cin, 3, 3, 3), generator=g) * 0.05).bfloat16().float()
    scale = torch.randn(CO, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    x = lattice_input(cin, off, g)
    r32 = lattice_reference(x, w, scale, 1)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    assert_same_bits(ncdhw(DeepCase(x, w, scale, torch.zeros(CO)).run(device)), ref)


@pytest.mark.gpu
def test_deep_impulse_pointwise_skip_weights(device):
    """The pointwise skip's packed weights one product at a time: x is zero, every skip voxel has
    one of its 64 channels set."""
    g = torch.Generator().manual_seed(99)
    ws = (torch.randn((CO, 64), generator=g) * 0.3).bfloat16().float()
    scale_s = torch.randn(CO, generator=g)
    scale_s[0], scale_s[1] = -scale_s[0].abs(), scale_s[1].abs()
    _, skip = skip_lattice(g)
    B, D = skip.shape[0], skip.shape[2]
    r32 = lattice_reference(skip, ws.view(CO, 64, 1, 1, 1), scale_s, 0)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    for cin in (64, 128):
        w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).float()
        case = DeepCase(torch.zeros(B, cin, D, D, D), w, exact_scale_shift(3, CO)[0], torch.zeros(CO), POINTWISE, skip,
                        ws, scale_s, torch.zeros(CO))
        assert_same_bits(ncdhw(case.run(device)), ref)


@pytest.mark.gpu
def test_deep_d64_sparse_impulses(device):
    """The largest extent the entry takes (D = 64, B = 1, 128 -> 128; 262,144 voxels, the 4 x 4 wave
    tile).  Sparse impulses (corners, faces, the last voxels, group seams) with integer weights; the
    reference is formed analytically, each impulse's clipped 3^3 x 128 block of weights, everything
    else relu(shift) = 0, and every element is compared."""
    from mvn_rocm import v2v
    D, cin = 64, 128
    g = torch.Generator().manual_seed(64)
    w = torch.randint(-4, 5, (CO, cin, 3, 3, 3), generator=g).float()
    scale = exact_scale_shift(5, CO)[0]
    pts = [(0, 0, 0), (63, 63, 63), (63, 0, 32), (0, 63, 15), (31, 32, 16), (32, 31, 47), (3, 8, 63), (4, 7, 0),
           (50, 60, 60), (60, 56, 4), (15, 47, 23), (48, 16, 40)]
    for _ in range(20):
        p = tuple(int(v) for v in torch.randint(0, 21, (3,), generator=g) * 3)
        if all(max(abs(a - b) for a, b in zip(p, q)) >= 3 for q in pts):
            pts.append(p)
    pts = sorted(set(pts))
    assert len(pts) >= 20
    for i, p in enumerate(pts):
        for q in pts[:i]:
            assert max(abs(a - b) for a, b in zip(p, q)) >= 3      # disjoint 3^3 boxes: one product per output
    x = torch.zeros(1, D, D, D, cin, dtype=torch.bfloat16, device=device)
    ref = torch.zeros(1, D, D, D, CO, dtype=torch.bfloat16, device=device)
    for n, (px, py, pz) in enumerate(pts):
        ch, val = (7 * n + 3) % cin, float((n % 4) + 1)
        x[0, px, py, pz, ch] = val
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    ox, oy, oz = px + 1 - dx, py + 1 - dy, pz + 1 - dz        # tap (dx, dy, dz) reads voxel o + d - 1
                    if 0 <= ox < D and 0 <= oy < D and 0 <= oz < D:
                        r = val * w[:, ch, dx, dy, dz] * scale
                        ref[0, ox, oy, oz] = torch.where(r <= 0, torch.zeros_like(r), r).bfloat16().to(device)
    y = v2v.v2v_conv3_deep(x, pack_deep(w, device), scale.to(device), torch.zeros(CO, device=device))
    nbad = int((y.view(torch.int16) != ref.view(torch.int16)).sum())
    assert int((ref != 0).sum()) > 1000
    assert nbad == 0, f"{nbad} elements differ in their bits"


# ----------------------------------------------------------------------------- conv: frames, borders
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((128, IDENTITY), (64, POINTWISE)), ids=("identity", "pointwise"))
@pytest.mark.parametrize("D", (1, 2, 3))
def test_deep_frames_do_not_mix(device, D, cin, mode):
    """B = 3 with all frames inside one or two 16-voxel groups: each frame equals its own B = 1 call,
    and perturbing one frame (input and skip) leaves the other two with their bits."""
    case, ref, _ = parity_case(3, D, cin, mode)
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_same_bits(ncdhw(y), ref)
    for f in range(3):
        assert_same_bits(case.run(device, xd[f:f + 1].clone(), sd[f:f + 1].clone()), y[f:f + 1])
    for f in range(3):
        xp, sp = xd.clone(), sd.clone()
        xp[f] = xp[f] + 1
        sp[f] = sp[f] - 2
        yp = case.run(device, xp, sp)
        keep = [k for k in range(3) if k != f]
        assert_same_bits(yp[keep], y[keep])
        assert not torch.equal(yp[f], y[f])


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (64, 128))
@pytest.mark.parametrize("D", (1, 2, 3, 5))
def test_deep_borders_are_zero_padding(device, D, cin):
    """All-ones frame between two NaN frames, weights of ones: exactly the count of in-volume taps
    x Cin per voxel; a tap that reached into a neighbouring frame would show as NaN."""
    x = torch.full((3, cin, D, D, D), float("nan"))
    x[1] = 1.0
    y = ncdhw(DeepCase(x, torch.ones(CO, cin, 3, 3, 3), torch.ones(CO), torch.zeros(CO)).run(device)).float()
    n = torch.tensor([float(min(i + 1, D - 1) - max(i - 1, 0) + 1) for i in range(D)])
    want = (n.view(D, 1, 1) * n.view(1, D, 1) * n.view(1, 1, D) * cin).expand(CO, D, D, D)
    assert float(want.max()) == min(D, 3) ** 3 * cin
    assert torch.equal(y[1], want)
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[2]).all())


# ----------------------------------------------------------------------------- conv: non-finite voxels
def special_voxels(D):
    """(corner, edge, interior) voxels with 3^3 boxes that stay apart only at D = 5; at D = 3 they overlap."""
    return ((0, 0, 0), (D - 1, D // 2, D - 1), (D // 2, D // 2, D // 2))


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (64, 128))
@pytest.mark.parametrize("D", (3, 5))
def test_deep_nonfinite_input_voxels_follow_torch(device, D, cin):
    """B = 2.  Frame 0: a NaN in a corner, an edge and an interior voxel is NaN in exactly their 3^3
    boxes clipped to the frame, all 128 channels, and nowhere in frame 1.  Frame 1: +inf and -inf
    voxels (positive weights on their channels, scales of both signs) come out as torch's.  Compared
    with torch on the CPU, NaN positions equal and everything else bit for bit."""
    for value in (float("nan"), float("inf"), float("-inf")):
        case = integer_case(2, D, cin, NONE, seed=77 + cin + D)
        vox = special_voxels(D)
        f = 0 if value != value else 1
        g = torch.Generator().manual_seed(78)
        for n, (px, py, pz) in enumerate(vox):
            ch = (5 * n + 2) % cin
            case.x[f, ch, px, py, pz] = value
            if value == value:
                case.w[:, ch] = torch.randint(1, 5, (CO, 3, 3, 3), generator=g).float()      # no 0 * inf
        ref = case.reference()[0].float()
        nan_ref = torch.isnan(ref).numpy()
        if value != value:
            assert (nan_ref[0] == box_mask(D, vox, 1)[None]).all() and not nan_ref[1].any()
        else:
            assert torch.isinf(ref[1]).any() and not torch.isinf(ref[0]).any() and not nan_ref[0].any()
        xd = cl(case.x, device)
        y = case.run(device, xd)
        assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
        clean = 1 - f
        assert_same_bits(case.run(device, xd[clean:clean + 1].clone()), y[clean:clean + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (IDENTITY, POINTWISE), ids=("identity", "pointwise"))
@pytest.mark.parametrize("D", (3, 5))
def test_deep_nonfinite_skip_voxels_reach_their_own_voxel(device, D, mode):
    vox = special_voxels(D)
    sc = SKIP_C[mode]
    for value in (float("nan"), float("inf"), float("-inf")):
        case = integer_case(2, D, 128, mode, seed=91 + mode + D)
        g = torch.Generator().manual_seed(92)
        for n, (px, py, pz) in enumerate(vox):
            ch = (5 * n + 2) % sc
            case.skip[0, ch, px, py, pz] = value
            if mode == POINTWISE and value == value:
                case.ws[:, ch] = torch.randint(1, 5, (CO,), generator=g).float()             # no 0 * inf
        ref = case.reference()[0].float()
        bad = (~torch.isfinite(ref)).numpy()
        assert not bad[1].any()
        if mode == IDENTITY:                                     # the element itself: NaN, +inf, or relu(-inf) = 0
            assert int(torch.isnan(ref).sum()) == (len(vox) if value != value else 0)
            assert int(torch.isinf(ref).sum()) == (len(vox) if value == float("inf") else 0)
            for n, (px, py, pz) in enumerate(vox):
                assert value != float("-inf") or float(ref[0, (5 * n + 2) % sc, px, py, pz]) == 0.0
        else:
            assert (bad[0].any(axis=0) == box_mask(D, vox, 0)).all()
        xd, sd = cl(case.x, device), cl(case.skip, device)
        y = case.run(device, xd, sd)
        assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
        assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])


# ----------------------------------------------------------------------------- conv: guards
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((128, IDENTITY), (64, POINTWISE)), ids=("identity", "pointwise"))
@pytest.mark.parametrize("B,D", ((3, 3), (3, 5)))
def test_deep_no_reads_or_writes_outside_the_tensors(device, B, D, cin, mode):
    """The C entry on slices of larger poisoned buffers (81 and 375 voxels: a ragged last group):
    the NaN bands around x and skip must not reach the result, the sentinel bands around the output
    must be intact, with no sentinel left inside it."""
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    case, ref, _ = parity_case(B, D, cin, mode)
    a = case.args(device)
    big_x, xin = banded(a[0])
    big_s, sin = banded(a[4])
    big_o, out = banded(((B, D, D, D, CO), device))
    pw = a[5:] if mode == POINTWISE else [None] * 3
    assert xin.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = _lib.load().mvn_v2v_conv3_deep(xin.data_ptr(), cin, a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), mode,
                                          sin.data_ptr(), SKIP_C[mode],
                                          *[t.data_ptr() if t is not None else None for t in pw], out.data_ptr(), B, D,
                                          _stream(xin))
    _lib.check(code, "mvn_v2v_conv3_deep")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref)
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())


# ----------------------------------------------------------------------------- conv: random data
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((64, POINTWISE), (128, IDENTITY)), ids=("64to128_pointwise", "128to128_identity"))
@pytest.mark.parametrize("D", (5, 16))
def test_deep_random_data_against_float64_restatement(device, D, cin, mode):
    """conv1 (skip NONE) and conv2 (the block's skip) on random bf16 data against the float64
    restatement with the kernel's own roundings; conv2's restatement reads the hidden volume the
    GPU wrote.  Measured on the MI355X: 0.642-0.829 of the bar, the worst conv1
    64 -> 128 at D = 16."""
    B = 2
    c1 = random_case(B, D, cin, NONE, seed=10 * D + cin)
    xd = cl(c1.x, device)
    h = c1.run(device, xd)
    check_bound(c1, ncdhw(h).float(), f"deep conv1 D={D} cin={cin}")
    c2 = random_case(B, D, 128, mode, seed=10 * D + cin + 1, x=ncdhw(h).float())
    c2.skip = c1.x
    y = c2.run(device, h, xd)
    check_bound(c2, ncdhw(y).float(), f"deep conv2 D={D} {MODE_NAME[mode]}")


# ----------------------------------------------------------------------------- upsample
@pytest.mark.gpu
@pytest.mark.parametrize("negative_pre", (False, True), ids=("mixed", "negative_pre_positive_skip"))
@pytest.mark.parametrize("cout", (64, 128))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("D", (1, 2, 3, 5, 8, 16))
def test_deep_upsample_exact_parity_integer_inputs(device, D, B, cout, negative_pre):
    """With the skip and without it (skip = NULL), bit for bit against torch on the CPU."""
    case = up_integer_case(B, D, cout, 300 * B + D + cout + int(negative_pre), negative_pre)
    assert float(F.conv_transpose3d(case.x.abs(), case.w.abs(), None, stride=2).max()) <= 128 * 16 < 2 ** 24
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
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, 2 * D, 2 * D, 2 * D, cout)
    assert_same_bits(ncdhw(y), ref)
    case.skip = None                                            # the skip = NULL form: no add
    assert_same_bits(ncdhw(case.run(device)), case.reference()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cout", (64, 128))
def test_deep_upsample_one_hot_channel_lattice(device, cout):
    """Voxel v carries only channel v mod 128, full-significand weights: one product per output,
    and the 250 voxels of the two 5^3 frames hit every (ci, co, dx, dy, dz) weight."""
    B, D = 2, 5
    g = torch.Generator().manual_seed(17 + cout)
    w = (torch.randn((128, cout, 2, 2, 2), generator=g) * 0.2).bfloat16().float()
    scale = torch.randn(cout, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    _, x = up_lattice(B, D, g)
    r32 = (F.conv_transpose3d(x.double(), w.double(), None, stride=2) * per_channel(scale)).float()
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    assert_same_bits(ncdhw(UpCase(x, w, scale, torch.zeros(cout)).run(device)), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("cout", (64, 128))
@pytest.mark.parametrize("D", (3, 5))
def test_deep_upsample_nonfinite_voxels(device, D, cout):
    """B = 2: a non-finite input voxel of frame 0 reaches exactly its own 2x2x2 outputs (all channels
    for a NaN), a non-finite skip voxel exactly itself; the clean frame equals its run alone."""
    vox = special_voxels(D)
    for value in (float("nan"), float("inf"), float("-inf")):
        case = up_integer_case(2, D, cout, 55 + D + cout, False)
        for n, (px, py, pz) in enumerate(vox):
            ch = (11 * n + 2) % 128
            case.x[0, ch, px, py, pz] = value
            case.w[ch] = case.w[ch].abs() + 1.0                  # no 0 * inf
        ref = case.reference()[0].float()
        bad = (~torch.isfinite(ref)).numpy()
        own = np.zeros((2 * D,) * 3, bool)
        for px, py, pz in vox:
            own[2 * px:2 * px + 2, 2 * py:2 * py + 2, 2 * pz:2 * pz + 2] = True
        assert not bad[1].any() and (bad[0].any(axis=0) == own).all()
        if value != value:
            assert (torch.isnan(ref[0]).numpy() == own[None]).all()
        xd, sd = cl(case.x, device), cl(case.skip, device)
        y = case.run(device, xd, sd)
        assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
        assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])
        case = up_integer_case(2, D, cout, 56 + D + cout, False)
        for n, (px, py, pz) in enumerate(vox):
            case.skip[0, (3 * n + 1) % cout, 2 * px + 1, 2 * py, 2 * pz + 1] = value
        ref = case.reference()[0].float()
        assert int((~torch.isfinite(ref)).sum()) == len(vox) and bool(torch.isfinite(ref[1]).all())
        assert_parity_with_nans(ncdhw(case.run(device)).float().numpy(), ref.numpy(), "sum")


@pytest.mark.gpu
@pytest.mark.parametrize("cout", (64, 128))
@pytest.mark.parametrize("B,D", ((3, 3), (3, 5)))
def test_deep_upsample_no_reads_or_writes_outside_the_tensors(device, B, D, cout):
    from mvn_rocm import _lib
    from mvn_rocm._ops import _stream
    case = up_integer_case(B, D, cout, 66 + D, False)
    ref, _ = case.reference()
    big_x, xin = banded(cl(case.x, device))
    big_s, sin = banded(cl(case.skip, device))
    big_o, out = banded(((B, 2 * D, 2 * D, 2 * D, cout), device))
    w, sc, sh = case.params(device)
    code = _lib.load().mvn_v2v_upsample2_deep(xin.data_ptr(), cout, w.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                              sin.data_ptr(), out.data_ptr(), B, D, _stream(xin))
    _lib.check(code, "mvn_v2v_upsample2_deep")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref)
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cout", (64, 128))
@pytest.mark.parametrize("D", (5, 16))
def test_deep_upsample_random_data_against_float64_restatement(device, D, cout):
    """Random bf16 data: |got - ref| <= 2^-8 |ref| + (128 + 4) 2^-24 S, S the sum of the absolute
    terms (half a bf16 ulp of the result plus the f32 summation, fma and add roundings).  Measured
    on the MI355X: 0.984-0.991 of the bar, nearly all of it the half ulp of the one
    bf16 rounding."""
    B = 2
    g = torch.Generator().manual_seed(D + cout)
    x = bf16r(torch.randn(B, 128, D, D, D, generator=g))
    w = bf16r(torch.randn(128, cout, 2, 2, 2, generator=g) * 0.1)
    scale = (0.75 + 0.5 * torch.rand(cout, generator=g)) * torch.where(torch.arange(cout) % 5 == 2, -1.0, 1.0)
    case = UpCase(x, w, scale, 0.2 * torch.randn(cout, generator=g),
                  bf16r(torch.randn(B, cout, 2 * D, 2 * D, 2 * D, generator=g)))
    _, ref = case.pre_round(exact=False)
    S = F.conv_transpose3d(x.double().abs(), w.double().abs(), None, stride=2) * per_channel(scale).abs() \
        + per_channel(case.shift).abs() + case.skip.double().abs()
    bar = 2.0 ** -8 * ref.abs() + (128 + 4) * 2.0 ** -24 * S
    got = ncdhw(case.run(device)).double()
    frac = float(((got - ref).abs() / bar).max())
    print(f"deep upsample D={D} cout={cout}: worst |got - ref| / bar = {frac:.4f}")
    assert frac <= 1.0


# ----------------------------------------------------------------------------- block, determinism
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (64, 128), ids=("64to128_pointwise", "128to128_identity"))
def test_deep_block_equals_the_two_launches(device, cin):
    """res3d_block_deep and Res3DBlockDeepCL.from_reference of a stand-in block equal conv1 (skip
    NONE) then conv2 (the block's skip) bit for bit, for an empty batch and a non-contiguous view
    too, and stay within two bf16 roundings of the stock f32 block."""
    from mvn_rocm import v2v
    B, D = 2, 5
    block = randomise(Res3DBlock(cin, CO), seed=40 + cin)
    p = v2v.fold_res3d_block_deep(block, device=device)
    assert (p.skip_packed is None) == (cin == 128)
    x = bf16r(torch.randn(B, cin, D, D, D, generator=torch.Generator().manual_seed(cin)))
    xd = cl(x, device)
    h = v2v.v2v_conv3_deep(xd, p.packed1, p.scale1, p.shift1)
    two = v2v.v2v_conv3_deep(h, p.packed2, p.scale2, p.shift2, xd, p.skip_packed, p.skip_scale, p.skip_shift)
    assert_same_bits(v2v.res3d_block_deep(xd, p), two)
    assert_same_bits(v2v.Res3DBlockDeepCL.from_reference(block, device=device)(xd), two)
    with torch.no_grad():
        stock = block(x)
    err = float((ncdhw(two).float() - stock).abs().max() / stock.abs().max())
    print(f"deep block against the stock f32 modules: {err:.3e} of max|ref|")
    assert err <= 2.0 ** -6                 # as the 32- and 64-channel blocks: two bf16 roundings deep
    empty = torch.zeros((0, D, D, D, cin), dtype=torch.bfloat16, device=device)
    assert tuple(v2v.res3d_block_deep(empty, p).shape) == (0, D, D, D, CO)
    up = v2v.fold_upsample_block_deep(randomise(Upsample3DBlock(128, 64), seed=3), device=device)
    assert tuple(v2v.upsample2_add_deep(torch.zeros((0, D, D, D, 128), dtype=torch.bfloat16, device=device), up).shape) \
        == (0, 2 * D, 2 * D, 2 * D, 64)
    view = x.bfloat16().to(device).permute(0, 2, 3, 4, 1)       # NCDHW storage: copied
    assert not view.is_contiguous()
    assert_same_bits(v2v.res3d_block_deep(view, p), two)


@pytest.mark.gpu
def test_deep_two_calls_give_the_same_bits(device):
    """(3, 5): the same conv (identity and pointwise) and the same upsample twice."""
    for cin, mode in ((128, IDENTITY), (64, POINTWISE)):
        case, _, _ = parity_case(3, 5, cin, mode)
        a = case.args(device)
        from mvn_rocm import v2v
        assert_same_bits(v2v.v2v_conv3_deep(*a), v2v.v2v_conv3_deep(*a))
    c = random_case(3, 5, 128, IDENTITY, seed=5)
    assert_same_bits(c.run(device), c.run(device))
    up = up_integer_case(3, 5, 128, 9, False)
    assert_same_bits(up.run(device), up.run(device))


# ----------------------------------------------------------------------------- wiring
@pytest.mark.gpu
def test_v2veval_deep_wiring(device):
    """V = 32, B = 2, the stand-in model (deep extents 8, 4, 2, 1): with deep="kernels" trunk equals
    the chain written out here and forward equals v2v_head_softargmax on it, bit for bit; with
    deep="torch" trunk still equals the half-resolution chain."""
    from mvn_rocm import v2v, volumetric
    B, V = 2, 32
    m = stand_in_model()
    ev = v2v.V2VEval.from_reference(m, device=device, half_res="kernels", deep="kernels")
    assert ev.interior is None and len(ev.deep) == 16 and len(ev.half_res) == 4
    vol = bf16r(torch.randn(B, V, V, V, 32, generator=torch.Generator().manual_seed(9))).bfloat16().to(device)
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0], [-150.0, 40.0, 1000.0]]), 2500.0, V,
                                            theta=[0.0, 0.7], device=device)
    with torch.no_grad():
        want = chain_deep(m, vol)
        got = ev.trunk(vol)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, V, V, V, 32)
        assert_same_bits(got, want)
        kp, out = ev(vol, coords, 3.0)
        kp_w, out_w = v2v.v2v_head_softargmax(want, *v2v.fold_v2v_head(m.back_layers[1], m.back_layers[2], m.output_layer,
                                                                       device=device),
                                              coords, multiplier=3.0, channels_last=True)
        assert_same_bits(kp, kp_w)
        assert_same_bits(out, out_w)
        evt = v2v.V2VEval.from_reference(m, device=device, half_res="kernels", deep="torch")
        assert evt.deep is None and len(evt.half_res) == 4
        old = chain_kernels(m, evt, vol)
        assert_same_bits(evt.trunk(vol), old)
        assert_same_bits(v2v.V2VEval.from_reference(m, device=device, half_res="kernels").trunk(vol), old)   # the default
    assert not torch.equal(got, old)                              # the two paths round differently


# ----------------------------------------------------------------------------- semantics
@pytest.mark.gpu
def test_v2veval_deep_against_the_f32_modules(device):
    """The case of test_v2veval_half_res_against_the_f32_modules (V = 32, B = 1, blob input,
    multiplier 10): trunk error / max|ref| and joints error / cuboid side against the f32 CPU
    stand-in, in one run, for deep="kernels", for half_res="kernels" alone and for the CPU stand-in
    with bf16 conv operands.  The bar: err_deep <= 2 x max(err_half_res_kernels, err_bf16_cpu) for
    both quantities (both yardsticks come from code older than the deep kernels; 2 is the margin of
    the test this mirrors).  Measured on the MI355X, trunk / joints: deep 6.263e-3 /
    8.224e-3, half_res="kernels" alone 6.263e-3 / 9.682e-3, bf16 operands on the CPU 4.179e-3 /
    9.090e-3: 0.50 and 0.42 of the bar."""
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
            ev = v2v.V2VEval.from_reference(m, device=device, half_res="kernels", deep=how)
            t = ncdhw(ev.trunk(vol)).float()
            kp, _ = ev(vol, coords, E2E_MULT)
            res["deep" if how == "kernels" else "half_res"] = (float((t - t_ref).abs().max() / t_ref.abs().max()),
                                                               float((kp.cpu() - kp_ref).abs().max()) / E2E_SIDE)
    res["bf16_cpu"] = (float((t_b - t_ref).abs().max() / t_ref.abs().max()), float((kp_b - kp_ref).abs().max()) / E2E_SIDE)
    for how, (tr, jo) in res.items():
        print(f"deep semantics, {how}: trunk {tr:.3e} of max|ref|, joints {jo:.3e} of the side")
    for q in (0, 1):
        assert res["deep"][q] <= 2 * max(res["half_res"][q], res["bf16_cpu"][q])
