"""Full-resolution Res3DBlocks (csrc/v2v_res3d.hip): one 3x3x3 conv + folded BN + residual + ReLU
per launch on channels-last bf16 volumes, the one-call block, and V2VEval (MI355X only).

Most tests give the kernel operands for which its f32 arithmetic is exact in any summation
order, and compare bits (as tests/test_gpu_v2v_front_edges.py does for the front block):

* integers in [-4, 4] as inputs, weights and skip: every partial sum is an integer below
  27 * 32 * 16 = 13,824 < 2^24, so torch's f32 conv3d on the CPU is exact (guarded); ``scale`` is
  a per-channel power of two of either sign, ``shift`` a multiple of 1/4, so neither fma nor the
  residual add rounds; the only rounding left is f32 -> bf16, nearest-even, ties included;
* an impulse lattice of stride 3 with full 8-bit significands: every output receives at most
  one product (asserted), exact in f32; ``product * scale`` rounds once to f32, then to bf16.

The reference is r in float64 per the arithmetic contract of mvn_v2v_conv3 (include/mvn_hip.h),
+0 where r <= 0 (NaN kept), cast to f32, then ``.bfloat16()``; the tests assert r holds no -0.
The case builders, the reference and the bound are tests/v2v_kit.py's, on its 32-channel record.

Tiles are 4 x 8 x 16 (x, y, z); a block walks a column of V / 4 tiles along x through a ring of
6 x-slices whose slot pattern repeats every 3 tiles; the grid is B * (V / 8) * (V / 16) blocks.
Reads nothing outside the repository.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_parity_with_nans
from v2v_kit import (BAND, E2E_MULT, E2E_SIDE, IDENTITY, INF_VOXELS, J, N_BOX, NAN_VOXELS, NONE, POINTWISE, RES3D,
                     Res3DBlock, assert_same_bits, banded, bands_intact, bf16_full, bf16_operand_model, bf16r, bits,
                     box_mask, chain, check_bound, cl, e2e_case, lattice_reference, ncdhw, randomise, stand_in_model)

CO = 32
MODES = {"none": NONE, "identity": IDENTITY, "pointwise": POINTWISE}
SKIP_C = {NONE: 0, IDENTITY: 32, POINTWISE: 16}
# the method of tests/v2v_kit.py on the 32-channel level
Case, pack3, packs, exact_scale_shift = RES3D.case, RES3D.pack, RES3D.pack_skip, RES3D.exact_scale_shift
integer_case, parity_case, random_case = RES3D.integer_case, RES3D.parity_case, RES3D.random_case


# ----------------------------------------------------------------------------- 1. exact parity
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES.values(), ids=MODES.keys())
@pytest.mark.parametrize("cin", (16, 32))
@pytest.mark.parametrize("B,V", ((1, 16), (3, 16), (1, 32), (1, 48), (2, 48)))
def test_exact_parity_integer_inputs(device, B, V, cin, mode):
    """Every element equals the CPU reference bit for bit, every skip mode and Cin, frames of
    different data.  Grids of 2, 6, 8, 18 and 36 blocks: (1, 16) and (3, 16) have fewer blocks
    than XCDs; (3, 16), (1, 48) and (2, 48) take xcd_remap's ragged branch (6, 18, 36 are no
    multiples of 8); V = 48 has 3 z-tiles, 6 y-tiles and 12 x-tiles, so a tile with neighbours on
    both sides in every axis; the 6-slot x-slice ring repeats every 3 tiles, so V = 16 (4 tiles)
    already passes one period and V = 48 (12 tiles) four."""
    case, ref, r = parity_case(B, V, cin, mode)
    assert all(not torch.equal(case.x[0], case.x[f]) for f in range(1, B))
    finite = torch.where(torch.isfinite(case.x), case.x, torch.zeros_like(case.x))
    partial = float(F.conv3d(finite.abs(), case.w.abs(), None, padding=1).max())
    print(f"largest sum of |x w|: {partial:.0f}")
    assert partial <= 27 * cin * 16
    # what the reference must hold for the comparison to test the relu and the bf16 rounding
    pos = r[r > 0].float()
    low = bits(pos) & 0xFFFF
    assert pos.numel() >= 0.25 * r.numel()
    assert (low != 0).sum() >= 0.10 * pos.numel()               # more than 8 significant bits
    assert (low == 0x8000).any()                                # an exact tie
    y = case.run(device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, V, V, V, CO)
    assert_same_bits(ncdhw(y), ref)


# ----------------------------------------------------------------------------- 2. impulse lattice
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
@pytest.mark.parametrize("B,V,off", ((2, 16, 0), (2, 16, 2), (1, 48, 1)))
def test_impulse_lattice_full_mantissa(device, B, V, off, cin):
    """One product per output, 8-bit x 8-bit significands: pins the tap <-> packed-weight map,
    the channel-chunk swizzle and the border clipping one product at a time, bit for bit."""
    g = torch.Generator().manual_seed(7 * V + off + cin)
    w = (torch.randn((CO, cin, 3, 3, 3), generator=g) * 0.05).bfloat16().float()
    scale = torch.randn(CO, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    x = torch.zeros((B, cin, V, V, V))
    pts = torch.arange(off, V, 3)
    n = pts.numel()
    ch = (torch.arange(B * n ** 3).view(B, n, n, n) * 5 + 11 * torch.arange(B).view(B, 1, 1, 1)) % cin
    sub = torch.zeros(B, cin, n, n, n).scatter_(1, ch.unsqueeze(1), bf16_full((B, 1, n, n, n), g))
    x[:, :, off::3, off::3, off::3] = sub
    assert int((x != 0).sum()) == B * n ** 3 and len(set(ch.flatten().tolist())) == cin      # every channel used
    r32 = lattice_reference(x, w, scale, 1)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8                      # both relu branches
    y = Case(x, w, scale, torch.zeros(CO)).run(device)
    assert_same_bits(ncdhw(y), ref)


@pytest.mark.gpu
def test_impulse_pointwise_skip_weights(device):
    """The pointwise skip's packed weights one product at a time: x is zero, every skip voxel has
    one of its 16 channels set."""
    B, V = 2, 16
    g = torch.Generator().manual_seed(99)
    ws = (torch.randn((CO, 16), generator=g) * 0.3).bfloat16().float()
    scale_s = torch.randn(CO, generator=g)
    scale_s[0], scale_s[1] = -scale_s[0].abs(), scale_s[1].abs()
    ch = torch.randint(0, 16, (B, 1, V, V, V), generator=g)
    skip = torch.zeros(B, 16, V, V, V).scatter_(1, ch, bf16_full((B, 1, V, V, V), g))
    r32 = lattice_reference(skip, ws.view(CO, 16, 1, 1, 1), scale_s, 0)
    ref = torch.where(r32 <= 0, torch.zeros_like(r32), r32).bfloat16()
    assert 0.2 < float((ref > 0).float().mean()) < 0.8
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    case = Case(torch.zeros(B, 32, V, V, V), w, *exact_scale_shift(3)[:1], torch.zeros(CO), POINTWISE, skip, ws, scale_s,
                torch.zeros(CO))
    assert_same_bits(ncdhw(case.run(device)), ref)


# ----------------------------------------------------------------------------- 3. frames, borders
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((32, IDENTITY), (16, POINTWISE), (16, NONE)), ids=("identity", "pointwise", "none16"))
def test_frames_do_not_mix(device, cin, mode):
    """In a B = 3 call each frame equals its own B = 1 call bit for bit."""
    case, ref, _ = parity_case(3, 16, cin, mode)
    xd = cl(case.x, device)
    sd = cl(case.skip, device) if mode != NONE else None
    y = case.run(device, xd, sd)
    assert_same_bits(ncdhw(y), ref)
    for f in range(3):
        alone = case.run(device, xd[f:f + 1].clone(), sd[f:f + 1].clone() if sd is not None else None)
        assert_same_bits(alone, y[f:f + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
def test_borders_are_zero_padding(device, cin):
    """All-ones frame between two NaN frames, weights of ones, scale 1, shift 0: exactly the
    clipped tap count x Cin at faces, edges and corners — a tap that reached past the volume
    into a neighbouring frame (or anything else) would show as NaN or a wrong count."""
    V = 32
    x = torch.full((3, cin, V, V, V), float("nan"))
    x[1] = 1.0
    case = Case(x, torch.ones(CO, cin, 3, 3, 3), torch.ones(CO), torch.zeros(CO))
    y = ncdhw(case.run(device)).float()
    n = torch.full((V,), 3.0)
    n[0] = n[-1] = 2.0
    want = (n.view(V, 1, 1) * n.view(1, V, 1) * n.view(1, 1, V) * cin).expand(CO, V, V, V)
    assert set(want.unique().tolist()) == {8.0 * cin, 12.0 * cin, 18.0 * cin, 27.0 * cin}
    assert torch.equal(y[1], want)
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[2]).all())


# ----------------------------------------------------------------------------- 4. random data
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((16, POINTWISE), (32, IDENTITY)), ids=("16to32_pointwise", "32to32_identity"))
@pytest.mark.parametrize("V", (16, 32))
def test_random_data_against_float64_restatement(device, V, cin, mode):
    """conv1 (skip NONE) and conv2 (the block's skip) on random bf16 data against the float64
    restatement with the kernel's own roundings; conv2's restatement reads the hidden volume the
    GPU wrote.  Measured on the MI355X: see DESIGN.md §4.12."""
    B = 2
    c1 = random_case(B, V, cin, NONE, seed=10 * V + cin)
    xd = cl(c1.x, device)
    h = c1.run(device, xd)
    check_bound(c1, ncdhw(h).float(), f"conv1 V={V} cin={cin}")
    c2 = random_case(B, V, 32, mode, seed=10 * V + cin + 1, x=ncdhw(h).float())
    c2.skip = c1.x
    y = c2.run(device, h, xd)
    check_bound(c2, ncdhw(y).float(), f"conv2 V={V} {('none', 'identity', 'pointwise')[mode]}")


# ----------------------------------------------------------------------------- 5. non-finite voxels
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32))
def test_nonfinite_input_voxels_follow_torch(device, cin):
    """A NaN input voxel is NaN in exactly its clipped 3^3 box, all 32 channels; +-inf voxels
    (positive weights, scales of both signs) come out +inf or 0; every other element is
    bit-equal, and the clean frame equals its run alone."""
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
    box = box_mask(V, NAN_VOXELS, 1)
    assert box.sum() == N_BOX                                     # pairwise disjoint boxes
    assert (nan_ref[0] == box[None]).all() and not nan_ref[1:].any()
    inf_ref = torch.isinf(ref).numpy()
    assert not inf_ref[:2].any() and inf_ref[2].any() and bool((ref[torch.isinf(ref)] > 0).all())
    for (px, py, pz, _, val) in INF_VOXELS:
        at = ref[2, :, px, py, pz]
        assert bool((torch.isinf(at) == ((case.scale > 0) == (val > 0))).all()) and bool((at[~torch.isinf(at)] == 0).all())
    xd = cl(case.x, device)
    y = case.run(device, xd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert int(torch.isnan(y).sum()) == CO * N_BOX
    assert_same_bits(case.run(device, xd[1:2].clone()), y[1:2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (IDENTITY, POINTWISE), ids=("identity", "pointwise"))
def test_nonfinite_skip_voxels_reach_their_own_voxel(device, mode):
    """Under an IDENTITY / POINTWISE skip a non-finite skip voxel reaches exactly its own voxel."""
    V = 32
    case = integer_case(3, V, 32, mode, seed=91 + mode)
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
    own = box_mask(V, NAN_VOXELS, 0)
    if mode == IDENTITY:          # the NaN sits in one channel of the 32 and stays there
        assert int(nan_ref.sum()) == len(NAN_VOXELS) and not nan_ref[1:].any()
    else:                         # the 1x1x1 conv spreads it over all 32 channels of the voxel
        assert (nan_ref[0] == own[None]).all() and not nan_ref[1:].any()
    assert not torch.isinf(ref[:2]).any() and torch.isinf(ref[2]).any()
    # identity: only the +inf voxel stays infinite (-inf is below the relu); pointwise: both, in
    # the channels whose scale has the matching sign
    assert int(torch.isinf(ref).any(dim=1).sum()) == (1 if mode == IDENTITY else len(INF_VOXELS))
    xd, sd = cl(case.x, device), cl(case.skip, device)
    y = case.run(device, xd, sd)
    assert_parity_with_nans(ncdhw(y).float().numpy(), ref.numpy(), "sum")
    assert_same_bits(case.run(device, xd[1:2].clone(), sd[1:2].clone()), y[1:2])


# ----------------------------------------------------------------------------- 6. stray reads, writes
@pytest.mark.gpu
@pytest.mark.parametrize("cin,mode", ((32, IDENTITY), (16, POINTWISE)), ids=("identity", "pointwise"))
def test_no_reads_or_writes_outside_the_tensors(device, cin, mode):
    """The C entries on slices of larger buffers (V = 16, B = 2: every tile touches the border):
    the NaN bands around x and skip must not reach the result, and the sentinel bands around the
    output and around the workspace (passed at exactly its advertised size) must be intact, with
    no sentinel left inside the output."""
    from mvn_rocm import _lib, v2v
    from mvn_rocm._ops import _stream
    lib = _lib.load()
    B, V = 2, 16
    # one launch
    case, ref, _ = parity_case(3, V, 32, mode)
    big_x, xin = banded(cl(case.x[:B], device))
    big_s, sin = banded(cl(case.skip[:B], device))
    big_o, out = banded(((B, V, V, V, CO), device))
    w, sc, sh = pack3(case.w, device), case.scale.to(device), case.shift.to(device)
    pw = [packs(case.ws, device), case.scale_s.to(device), case.shift_s.to(device)] if mode == POINTWISE else [None] * 3
    assert xin.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = lib.mvn_v2v_conv3(xin.data_ptr(), 32, w.data_ptr(), sc.data_ptr(), sh.data_ptr(), mode, sin.data_ptr(),
                             SKIP_C[mode], *[t.data_ptr() if t is not None else None for t in pw], out.data_ptr(), B, V,
                             _stream(xin))
    _lib.check(code, "mvn_v2v_conv3")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True)
    assert_same_bits(ncdhw(out), ref[:B])
    for big, n in ((big_x, xin.numel()), (big_s, sin.numel())):
        assert bool(torch.isnan(big[:BAND]).all()) and bool(torch.isnan(big[BAND + n:]).all())
    # the one-call block: cin -> 32 with the block's own skip
    params = v2v.fold_res3d_block(randomise(Res3DBlock(cin, CO), 5), device=device)
    x = bf16r(torch.randn(3, cin, V, V, V, generator=torch.Generator().manual_seed(6)))
    big_x, xin = banded(cl(x, device))
    big_o, out = banded(((3, V, V, V, CO), device))
    ws_bytes = lib.mvn_v2v_res3d_workspace_bytes(2, V)
    assert ws_bytes == 2 * V ** 3 * CO * 2
    big_w, ws = banded(((ws_bytes // 2,), device))
    ptr = [t.data_ptr() if t is not None else None for t in params]
    code = lib.mvn_v2v_res3d(xin.data_ptr(), cin, *ptr[:6], IDENTITY if cin == 32 else POINTWISE, *ptr[6:],
                             out.data_ptr(), ws.data_ptr(), ws_bytes, 2, 3, V, _stream(xin))
    _lib.check(code, "mvn_v2v_res3d")
    torch.cuda.synchronize()
    assert bands_intact(big_o, out.numel(), True) and bands_intact(big_w, ws.numel(), False)
    assert bool(torch.isnan(big_x[:BAND]).all()) and bool(torch.isnan(big_x[BAND + xin.numel():]).all())
    assert_same_bits(out, v2v.res3d_block(cl(x, device), params, 2))
    assert not bool(torch.isnan(out).any())


# ----------------------------------------------------------------------------- 7. V = 256
PERIOD = 11           # coprime to every power of two: an address off by 2^k voxels changes the data


def periodic_map(V, S):
    """Index into the S^3 conv of the same periodic pattern that equals output q of the V^3 conv
    (V = S mod 11, S >= 15): the 2 voxels at either border keep their distance to it, the
    interior (no border within 1 voxel of the window) repeats with the period."""
    q = np.arange(V)
    return np.where(q < 2, q, np.where(q >= V - 2, S - (V - q), 2 + (q - 2) % PERIOD))


def periodic_volume(pat, V):
    i = torch.arange(V) % PERIOD
    return pat[:, i][:, :, i][:, :, :, i].unsqueeze(0)


def test_periodic_map_on_the_cpu():
    """The index map of the V = 256 test, at V = 32 against a direct conv (no GPU)."""
    V, S = 32, 21
    assert V % PERIOD == S % PERIOD and S >= 15
    g = torch.Generator().manual_seed(256)
    pat = torch.randint(-4, 5, (32, PERIOD, PERIOD, PERIOD), generator=g).float()
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    scale, shift = exact_scale_shift(256)
    full, _ = Case(periodic_volume(pat, V), w, scale, shift).reference()
    small, _ = Case(periodic_volume(pat, S), w, scale, shift).reference()
    m = torch.from_numpy(periodic_map(V, S))
    assert_same_bits(full, small[:, :, m][:, :, :, m][:, :, :, :, m])


@pytest.mark.gpu
def test_v256_whole_volume(device):
    """The largest volume the entry takes (512 blocks of 64 tiles; (gy * V + gz) * 4 + c fills
    the staging descriptor's 18 bits, gx * V * V * 64 reaches 2^30), every element checked: the
    input repeats an integer pattern with period 11 per axis, so the reference is a 25^3 CPU conv
    expanded through periodic_map (asserted on the CPU above).  About 3 GiB on the device."""
    from mvn_rocm import v2v
    V, S = 256, 25
    assert V % PERIOD == S % PERIOD and S >= 15
    g = torch.Generator().manual_seed(256)
    pat = torch.randint(-4, 5, (32, PERIOD, PERIOD, PERIOD), generator=g).float()
    w = torch.randint(-4, 5, (CO, 32, 3, 3, 3), generator=g).float()
    scale, shift = exact_scale_shift(256)
    ref_s, _ = Case(periodic_volume(pat, S), w, scale, shift).reference()
    assert float((ref_s > 0).float().mean()) > 0.25
    i = (torch.arange(V) % PERIOD).to(device)
    pcl = pat.bfloat16().permute(1, 2, 3, 0).contiguous().to(device)
    x = pcl.index_select(0, i).index_select(1, i).index_select(2, i).unsqueeze(0)
    assert tuple(x.shape) == (1, V, V, V, 32) and x.is_contiguous()
    y = v2v.v2v_conv3(x, pack3(w, device), scale.to(device), shift.to(device))
    del x
    m = torch.from_numpy(periodic_map(V, S)).to(device)
    ref = ref_s.permute(0, 2, 3, 4, 1).contiguous().to(device).index_select(1, m).index_select(2, m).index_select(3, m)
    assert y.shape == ref.shape
    same = torch.equal(y.view(torch.int16), ref.view(torch.int16))
    nbad = 0 if same else int((y.view(torch.int16) != ref.view(torch.int16)).sum())
    del y, ref
    torch.cuda.empty_cache()
    assert same, f"{nbad} elements differ in their bits"


# ----------------------------------------------------------------------------- 8. one-call block
@pytest.mark.gpu
@pytest.mark.parametrize("cin", (16, 32), ids=("16to32_pointwise", "32to32_identity"))
def test_one_call_block_equals_the_two_launches(device, cin):
    """res3d_block for group_frames 0, 1 and 2 (ragged) at B = 3 equals conv1 (skip NONE) then
    conv2 (the block's skip) on the whole batch bit for bit; Res3DBlockCL.from_reference of a
    stand-in block with non-trivial BN statistics and conv biases equals res3d_block with the
    folded parameters, and stays near the stock block in f32."""
    from mvn_rocm import v2v
    B, V = 3, 16
    block = randomise(Res3DBlock(cin, CO), seed=40 + cin)
    p = v2v.fold_res3d_block(block, device=device)
    assert (p.skip_packed is None) == (cin == 32)
    x = bf16r(torch.randn(B, cin, V, V, V, generator=torch.Generator().manual_seed(cin)))
    xd = cl(x, device)
    h = v2v.v2v_conv3(xd, p.packed1, p.scale1, p.shift1)
    two = v2v.v2v_conv3(h, p.packed2, p.scale2, p.shift2, xd, p.skip_packed, p.skip_scale, p.skip_shift)
    for gf in (0, 1, 2):
        assert_same_bits(v2v.res3d_block(xd, p, gf), two)
    mod = v2v.Res3DBlockCL.from_reference(block, device=device)
    assert_same_bits(mod(xd), two)
    with torch.no_grad():
        stock = block(x)
    err = float((ncdhw(two).float() - stock).abs().max() / stock.abs().max())
    print(f"block against the stock f32 modules: {err:.3e} of max|ref|")
    assert err <= 2.0 ** -6                 # two bf16 roundings deep (weights, hidden volume, output)


@pytest.mark.gpu
def test_empty_batch_and_noncontiguous_input(device):
    """An empty batch returns the empty volume without a launch; a non-contiguous view is copied."""
    from mvn_rocm import v2v
    case, ref, _ = parity_case(1, 16, 32, IDENTITY)
    p = v2v.fold_res3d_block(randomise(Res3DBlock(32, CO), 1), device=device)
    empty = torch.zeros((0, 16, 16, 16, 32), dtype=torch.bfloat16, device=device)
    c1 = (p.packed1, p.scale1, p.shift1)
    for y in (v2v.v2v_conv3(empty, *c1), v2v.v2v_conv3(empty, *c1, empty), v2v.res3d_block(empty, p)):
        assert tuple(y.shape) == (0, 16, 16, 16, 32) and y.dtype == torch.bfloat16
    view = case.x.bfloat16().to(device).permute(0, 2, 3, 4, 1)            # NCDHW storage
    sview = case.skip.bfloat16().to(device).permute(0, 2, 3, 4, 1)
    assert not view.is_contiguous()
    assert_same_bits(ncdhw(case.run(device, view, sview)), ref)


# ----------------------------------------------------------------------------- 9, 10. V2VEval
@pytest.mark.gpu
def test_v2veval_wiring(device):
    """trunk and forward equal, bit for bit, the same chain written out here (V = 32, B = 2); the
    interior runs the stand-in's own modules (V2VEval's copy of them: the same parameters)."""
    from mvn_rocm import v2v, volumetric
    import copy
    B, V = 2, 32
    m = stand_in_model()
    ev = v2v.V2VEval.from_reference(m, device=device)
    md = copy.deepcopy(m).to(device)
    own = [p for n, p in md.encoder_decoder.named_parameters() if not n.startswith("skip_res1.")]
    mine = list(ev.interior.parameters())
    assert len(mine) == len(own) and all(torch.equal(a, b) for a, b in zip(mine, own))
    vol = bf16r(torch.randn(B, V, V, V, 32, generator=torch.Generator().manual_seed(9))).bfloat16().to(device)
    coords = volumetric.build_coord_volumes(np.array([[10.0, -20.0, 900.0], [-150.0, 40.0, 1000.0]]), 2500.0, V,
                                            theta=[0.0, 0.7], device=device)
    with torch.no_grad():
        want = chain(m, ev, vol)
        got = ev.trunk(vol)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, V, V, V, 32)
        assert_same_bits(got, want)
        kp, out = ev(vol, coords, 3.0)
        kp_w, out_w = v2v.v2v_head_softargmax(want, *v2v.fold_v2v_head(m.back_layers[1], m.back_layers[2], m.output_layer,
                                                                       device=device),
                                              coords, multiplier=3.0, channels_last=True)
    assert tuple(kp.shape) == (B, J, 3) and tuple(out.shape) == (B, J, V, V, V)
    assert_same_bits(kp, kp_w)
    assert_same_bits(out, out_w)


# measured on the MI355X (see test_v2veval_against_the_f32_modules): the bars are twice these
E2E_TRUNK_MEASURED = 6.630e-3
E2E_JOINTS_MEASURED = 5.979e-3


def e2e_measure(device, mult=None):
    """(trunk error / max|ref|, joints error / cuboid side) of V2VEval and of the bf16-operand CPU
    stand-in, both against the f32 stand-in on the CPU followed by torch's soft-argmax."""
    from mvn_rocm import v2v
    from oracle import restate_torch
    mult = E2E_MULT if mult is None else mult
    m = stand_in_model()
    x, coords = e2e_case(device)
    cc = coords.cpu()
    with torch.no_grad():
        def cpu(model):
            t = model.back_layers[0](model.encoder_decoder(model.front_layers(x)))
            logits = model.output_layer(model.back_layers[2](model.back_layers[1](t)))
            kp, _ = restate_torch.integrate_tensor_3d_with_coordinates(logits * mult, cc, softmax=True)
            return t, kp, logits
        t_ref, kp_ref, logits = cpu(m)
        t_b, kp_b, _ = cpu(bf16_operand_model(m))
        ev = v2v.V2VEval.from_reference(m, device=device)
        vol = x.bfloat16().permute(0, 2, 3, 4, 1).contiguous().to(device)
        t = ncdhw(ev.trunk(vol)).float()
        kp, _ = ev(vol, coords, mult)
    peak = float(((logits * mult).amax(dim=(2, 3, 4)) - (logits * mult).mean(dim=(2, 3, 4))).min())
    den = float(t_ref.abs().max())
    res = dict(peak=peak,
               trunk=float((t - t_ref).abs().max()) / den, joints=float((kp.cpu() - kp_ref).abs().max()) / E2E_SIDE,
               trunk_bf16_cpu=float((t_b - t_ref).abs().max()) / den,
               joints_bf16_cpu=float((kp_b - kp_ref).abs().max()) / E2E_SIDE)
    print("V2VEval against the f32 stand-in: " + ", ".join(f"{k} {v:.3e}" for k, v in res.items()))
    return res


@pytest.mark.gpu
def test_v2veval_against_the_f32_modules(device):
    """The true semantics: the stand-in V2VModel (Xavier weights, randomised BN statistics) in f32
    on the CPU followed by torch's soft-argmax (oracle/restate_torch.py), against V2VEval on the
    GPU at V = 32, B = 1.  Input: synth.blob_volumes (peak 10, sigma 3 voxels, unit noise) in the
    first 17 of the 32 channels, 0.1 x unit noise in the rest, rounded to bf16; multiplier 10, which
    puts every joint's largest logit 10.2 or more above its mean (the height of the blobs).
    Measured on the MI355X: trunk max error 6.630e-3 of max|ref|, joints 5.979e-3 of the 2500 mm
    cuboid side (14.9 mm).  The same stand-in on the CPU with every conv operand rounded to bf16
    (bf16_operand_model), the cost of bf16 operands alone: trunk 4.179e-3, joints 9.090e-3 — the
    joints match it (0.66 x), the trunk is 1.59 x above it (V2VEval also rounds each block's
    output, the skip it re-reads and the front block's output to bf16).  With multiplier 40 (peaks
    41 above the mean, a near-argmax) both are 4 % of the side: 3.978e-2 against 3.725e-2.  The
    bars are twice the measured values, the margin of test_end_to_end_against_the_f32_modules."""
    res = e2e_measure(device)
    assert res["peak"] > 4.0                          # peaked logits: each joint's peak well above its mean
    assert res["trunk"] <= 2 * E2E_TRUNK_MEASURED
    assert res["joints"] <= 2 * E2E_JOINTS_MEASURED
