"""The V2V front block (csrc/v2v_front.hip) at its edges, without a tolerance (MI355X only).

The other GPU tests of this kernel feed it random normal data and accept 1e-4 of the largest
output on every element.  Here the conv gets inputs for which f32 accumulation is exact in any
order, so every output element, both output dtypes, must equal a CPU reference bit for bit:

* integers in [-4, 4] (exact in bf16) as inputs and weights: every partial sum is an integer
  below 343 * 32 * 16 = 175,616 < 2^24, so torch's f32 conv3d on the CPU is exact; `scale` is a
  per-channel power of two of either sign and `shift` a multiple of 1/4, so the fma rounds
  nothing either (and would round once, as the float64 reference cast to f32 does);
* an impulse lattice of stride 7 with full 8-bit significands: every output receives at most
  one product, which f32 holds exactly, and `product * scale` rounds once.

The reference is r = conv * scale + shift in float64, +0 where r <= 0 and r otherwise (NaN
kept), cast to f32, and torch's .bfloat16() of that for bf16 output.  It is not torch.relu,
which returns -0 for -0 on the CPU; the tests assert that r holds no -0 at all.

Shapes: grids below 8 blocks and not a multiple of 8 (xcd_remap's ragged branch), nTx = 12 (the
x-slice ring of 10 slots through two periods and every wrap), nTz = 3 (a z-tile with two
neighbours), V = 256 (the staging descriptor's 18-bit field full, slice offsets up to 2^30).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_bits_equal, assert_parity_with_nans

pytestmark = pytest.mark.gpu

CI, CO, KS, PAD = 32, 16, 7, 3
DTYPES = (torch.float32, torch.bfloat16)


# ----------------------------------------------------------------------------- helpers
def bits(t):
    """The bit pattern of an f32 / bf16 tensor as a numpy unsigned array (on the host)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    assert t.dtype == torch.bfloat16
    return t.view(torch.int16).numpy().view(np.uint16)


def assert_same_bits(got, want):
    a, b = bits(got), bits(want)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ in their bits"


def channels_last(x, device):
    """(B, 32, V, V, V) f32 holding bf16-exact values -> the kernel's (B, V, V, V, 32) bf16 input."""
    xb = x.bfloat16()
    same = (xb.float() == x) | torch.isnan(x)
    assert bool(same.all()), "the test's input is not exact in bf16"
    return xb.permute(0, 2, 3, 4, 1).contiguous().to(device)


def pack(w, device):
    """The packed bf16 weights of fold_basic3d_block (identity BatchNorm: only the packing)."""
    from mvn_rocm import v2v
    one, zero = torch.ones(CO), torch.zeros(CO)
    packed, _, _ = v2v.fold_basic3d_block(w, None, one, zero, zero, one, 0.0, device=device)
    return packed


def exact_scale_shift(seed):
    """Per-channel scale = +-2^k (k in -2..1, both signs present) and shift = a multiple of 1/4
    (never -0): conv * scale + shift is exact in f32 for the integer conv."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 2, (CO,), generator=g).float()
    sign = torch.where(torch.arange(CO) % 3 == 1, -1.0, 1.0)
    scale = sign * torch.exp2(k)
    shift = torch.randint(-8, 9, (CO,), generator=g).float() / 4 + 0.0
    assert not bool((torch.signbit(shift) & (shift == 0)).any())
    return scale, shift


def integer_case(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, CI, V, V, V), generator=g).float()
    w = torch.randint(-4, 5, (CO, CI, KS, KS, KS), generator=g).float()
    return x, w


def reference(x, w, scale, shift):
    """(f32 reference, float64 pre-relu r) of relu(conv3d_7(x) * scale + shift) on the CPU; the
    conv in f32, which the exactness guard shows to be exact for these operands."""
    finite = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    assert float(F.conv3d(finite.abs(), w.abs(), None, padding=PAD).max()) < 2.0 ** 24
    conv = F.conv3d(x, w, None, padding=PAD)
    r = conv.double() * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    assert not bool((torch.signbit(r) & (r == 0)).any()), "the pre-relu reference holds a -0"
    y = torch.where(r <= 0, torch.zeros_like(r), r)            # a NaN is neither: kept
    return y.float(), r


def as_dtype(ref32, dtype):
    return ref32 if dtype == torch.float32 else ref32.bfloat16()


@functools.lru_cache(maxsize=None)
def parity_case(B, V):
    """Inputs and CPU reference of the exact-parity test, computed once per shape."""
    x, w = integer_case(B, V, seed=1000 * B + V)
    scale, shift = exact_scale_shift(seed=V)
    ref, _ = reference(x, w, scale, shift)
    return x, w, scale, shift, ref


# ----------------------------------------------------------------------------- a. exact parity
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("B,V", ((1, 16), (3, 16), (1, 32), (1, 48), (2, 48)))
def test_exact_parity_integer_inputs(device, B, V, dtype):
    """Grids of 4, 12, 16, 36 and 72 blocks (fewer than 8; ragged xcd_remap; nTx = 12 and
    nTz = 3 at V = 48), frames of different data: every element equals the CPU reference bit
    for bit, f32 and bf16 (nearest-even of values needing more than 8 bits, ties among them)."""
    from mvn_rocm import v2v
    x, w, scale, shift, ref = parity_case(B, V)
    assert all(not torch.equal(x[0], x[f]) for f in range(1, B))
    # what the reference must hold for the comparison to test the relu and the bf16 rounding
    pos = ref[ref > 0]
    low = bits(pos) & 0xFFFF
    assert pos.numel() >= 0.25 * ref.numel()
    assert (low != 0).sum() >= 0.10 * pos.numel()               # not representable in bf16
    assert (low == 0x8000).any()                                # an exact tie
    y = v2v.v2v_front(channels_last(x, device), pack(w, device), scale.to(device), shift.to(device), dtype)
    assert y.dtype == dtype and tuple(y.shape) == (B, CO, V, V, V)
    if dtype == torch.float32:
        assert_bits_equal(y.cpu().numpy(), ref.numpy())
    else:
        assert np.array_equal(bits(y), bits(ref.bfloat16()))


# ----------------------------------------------------------------------------- b. impulse lattice
def lattice_case(B, V, off, seed):
    """x is zero except one channel at each voxel of the lattice g = off (mod 7) per axis (the
    channel cycles through all 32, the value is a full-mantissa bf16), so every output holds at
    most one product.  The reference is formed product by product in float64: output o = l + d
    (|d| <= 3 per axis, inside the volume) of lattice voxel l takes tap k = 3 - d."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn((CO, CI, KS, KS, KS), generator=g) * 0.02).bfloat16().float()
    scale = torch.randn(CO, generator=g)
    scale[0], scale[1] = -scale[0].abs(), scale[1].abs()
    x = torch.zeros((B, CI, V, V, V))
    w64, s64 = w.double().numpy(), scale.double().numpy().reshape(CO, 1, 1, 1)
    r = np.zeros((B, CO, V, V, V), np.float64)
    pts = range(off, V, KS)
    n = 0
    for b in range(B):
        for lx in pts:
            for ly in pts:
                for lz in pts:
                    ch = (n + 11 * b) % CI
                    n += 1
                    val = torch.randn((), generator=g).bfloat16().float()
                    assert abs(float(val)) > 2.0 ** -100             # a normal bf16
                    x[b, ch, lx, ly, lz] = val
                    o = [np.arange(max(l - PAD, 0), min(l + PAD, V - 1) + 1) for l in (lx, ly, lz)]
                    k = [l - oo + PAD for l, oo in zip((lx, ly, lz), o)]
                    blk = w64[:, ch][np.ix_(np.arange(CO), k[0], k[1], k[2])] * float(val)
                    r[np.ix_([b], np.arange(CO), o[0], o[1], o[2])] = (blk * s64)[None]
    ref = np.where(r <= 0, 0.0, r).astype(np.float32)
    return x, w, scale, ref


@pytest.mark.parametrize("V,off", ((16, 0), (16, 3), (48, 0), (48, 5)))
def test_impulse_lattice_full_mantissa(device, V, off):
    """One product per output, 8-bit x 8-bit significands: pins the tap <-> packed-weight map,
    the channel-chunk swizzle and the border clipping one product at a time, bit for bit."""
    from mvn_rocm import v2v
    B = 2 if V == 16 else 1
    x, w, scale, ref = lattice_case(B, V, off, seed=7 * V + off)
    assert (ref > 0).mean() > 0.2                                # both relu branches, mostly covered
    y = v2v.v2v_front(channels_last(x, device), pack(w, device), scale.to(device), torch.zeros(CO, device=device))
    assert_bits_equal(y.cpu().numpy(), ref)


# ----------------------------------------------------------------------------- c. V = 256
PERIOD = 11           # coprime to every power of two: an address off by 2^k voxels changes the data


def periodic_map(V, S):
    """Index into the S^3 conv of the same periodic pattern that equals output q of the V^3 conv
    (V = S mod 11, S >= 28): the 14 voxels at either border keep their distance to it, the
    interior (no border within 3 voxels of the window) repeats with the period."""
    q = np.arange(V)
    return np.where(q < 14, q, np.where(q >= V - 14, S - (V - q), 3 + (q - 3) % PERIOD))


def periodic_volume(pat, V):
    i = torch.arange(V) % PERIOD
    return pat[:, i][:, :, i][:, :, :, i].unsqueeze(0)


def test_v256_whole_volume(device):
    """The largest volume the entry point takes (1024 blocks of 64 tiles; (gy*V + gz)*4 + c
    fills the descriptor's 18 bits, gx * V*V*64 reaches 2^30), every element checked: the input
    repeats a random integer pattern with period 11 per axis, so the reference is a 36^3 CPU conv
    expanded through periodic_map.  About 3 GiB on the device, freed at the end.
    Measured on the MI355X: 0.24 s for the whole test (three CPU convs included)."""
    from mvn_rocm import v2v
    V, S = 256, 36
    assert V % PERIOD == S % PERIOD and S >= 28
    g = torch.Generator().manual_seed(256)
    pat = torch.randint(-4, 5, (CI, PERIOD, PERIOD, PERIOD), generator=g).float()
    w = torch.randint(-4, 5, (CO, CI, KS, KS, KS), generator=g).float()
    scale, shift = exact_scale_shift(seed=256)
    # the map itself, on the CPU at V = 64 against a 31^3 conv
    full, _ = reference(periodic_volume(pat, 64), w, scale, shift)
    small, _ = reference(periodic_volume(pat, 31), w, scale, shift)
    m = torch.from_numpy(periodic_map(64, 31))
    assert_bits_equal(full.numpy(), small[:, :, m][:, :, :, m][:, :, :, :, m].numpy())
    ref36, _ = reference(periodic_volume(pat, S), w, scale, shift)
    assert (ref36 > 0).float().mean() > 0.25
    # the periodic input, built channels-last on the device
    i = (torch.arange(V) % PERIOD).to(device)
    pcl = pat.bfloat16().permute(1, 2, 3, 0).contiguous().to(device)
    x = pcl.index_select(0, i).index_select(1, i).index_select(2, i).unsqueeze(0)
    assert tuple(x.shape) == (1, V, V, V, CI) and x.is_contiguous()
    y = v2v.v2v_front(x, pack(w, device), scale.to(device), shift.to(device))
    del x
    m = torch.from_numpy(periodic_map(V, S)).to(device)
    ref = ref36.to(device).index_select(2, m).index_select(3, m).index_select(4, m)
    assert y.shape == ref.shape
    same = torch.equal(y.view(torch.int32), ref.view(torch.int32))
    nbad = 0 if same else int((y.view(torch.int32) != ref.view(torch.int32)).sum())
    del y, ref
    torch.cuda.empty_cache()
    assert same, f"{nbad} elements differ in their bits"


# ----------------------------------------------------------------------------- d. non-finite voxels
# frame 0: one NaN voxel-channel each, 7^3 boxes pairwise disjoint: both corners, either side of
# the x seam 9 | 10 (and ring wrap), of the y seam 3 | 4 and of the z seam 15 | 16
NAN_VOXELS = ((0, 0, 0), (31, 31, 31), (9, 16, 5), (10, 16, 26), (24, 3, 8), (24, 4, 24), (20, 27, 15), (4, 27, 16))
INF_VOXELS = ((12, 12, 12, 5, float("inf")), (22, 20, 7, 21, float("-inf")))      # x, y, z, channel, value


def box_mask(V, voxels):
    m = np.zeros((V, V, V), bool)
    for x, y, z in voxels:
        m[max(x - PAD, 0):x + PAD + 1, max(y - PAD, 0):y + PAD + 1, max(z - PAD, 0):z + PAD + 1] = True
    return m


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    V = 32
    x, w = integer_case(3, V, seed=77)
    for n, (px, py, pz) in enumerate(NAN_VOXELS):
        x[0, (5 * n + 2) % CI, px, py, pz] = float("nan")
    g = torch.Generator().manual_seed(78)
    for px, py, pz, ch, val in INF_VOXELS:
        x[2, ch, px, py, pz] = val
        w[:, ch] = torch.randint(1, 5, (CO, KS, KS, KS), generator=g).float()     # no 0 * inf
    scale, shift = exact_scale_shift(seed=79)
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    ref, _ = reference(x, w, scale, shift)
    return x, w, scale, shift, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_nonfinite_voxels_follow_torch(device, dtype):
    """relu keeps a NaN as F.relu does: a NaN input voxel is NaN in exactly its clipped 7^3 box,
    all 16 channels; +-inf voxels (positive weights, scales of both signs) come out +inf or 0;
    every other element is bit-equal, and the clean frame equals its run alone.
    (With fmaxf in the epilogue the kernel returned 0 at every one of the 34,976 NaN elements
    and this test failed, in the NaN mask alone: 'NaN at 34976 differing elements'.)"""
    from mvn_rocm import v2v
    x, w, scale, shift, ref = nonfinite_case()
    V = x.shape[2]
    # the reference itself: NaN exactly in the boxes, infinities only in frame 2
    nan_ref = torch.isnan(ref).numpy()
    box = box_mask(V, NAN_VOXELS)
    assert box.sum() == 2 * 4 ** 3 + 6 * 7 ** 3                   # pairwise disjoint boxes
    assert (nan_ref[0] == box[None]).all() and not nan_ref[1:].any()
    assert int(nan_ref.sum()) == CO * (2 * 4 ** 3 + 6 * 7 ** 3) == 34976
    inf_ref = torch.isinf(ref).numpy()
    assert not inf_ref[:2].any() and (ref[inf_ref] > 0).all()
    for (px, py, pz, _, val) in INF_VOXELS:
        at = ref[2, :, px, py, pz]
        assert bool((torch.isinf(at) == ((scale > 0) == (val > 0))).all()) and bool((at[~torch.isinf(at)] == 0).all())
    xd, packed, sc, sh = channels_last(x, device), pack(w, device), scale.to(device), shift.to(device)
    y = v2v.v2v_front(xd, packed, sc, sh, dtype)
    want = as_dtype(ref, dtype)
    assert_parity_with_nans(y.float().cpu().numpy(), want.float().numpy(), "sum")
    assert int(torch.isnan(y).sum()) == 34976
    alone = v2v.v2v_front(xd[1:2].clone(), packed, sc, sh, dtype)
    assert_same_bits(alone, y[1:2])


# ----------------------------------------------------------------------------- e. stray reads, writes
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_no_reads_or_writes_outside_the_tensors(device, dtype):
    """The C entry point on slices of larger buffers (V = 16, B = 2: every tile touches the
    border): 64 KiB of NaN on both sides of the input must not reach the result (the zero
    padding comes from the buffer resource's range check), and 64 KiB of a sentinel on both
    sides of the output must be intact, with no sentinel left inside it."""
    from mvn_rocm import _lib, v2v
    from mvn_rocm._ops import _stream
    from mvn_rocm.op import _dtype_code
    B, V = 2, 16
    x, w, scale, shift, ref = parity_case(B, V)
    xd, packed, sc, sh = channels_last(x, device), pack(w, device), scale.to(device), shift.to(device)
    plain = v2v.v2v_front(xd, packed, sc, sh, dtype)
    assert_same_bits(plain, as_dtype(ref, dtype))
    gin = 64 * 1024 // 2
    big_in = torch.full((gin + xd.numel() + gin,), float("nan"), dtype=torch.bfloat16, device=device)
    xin = big_in[gin:gin + xd.numel()].view(xd.shape)
    xin.copy_(xd)
    esize = 4 if dtype == torch.float32 else 2
    ity, sentinel = (torch.int32, 0x7FA5A5A5) if dtype == torch.float32 else (torch.int16, 0x7FA5)
    gout, n = 64 * 1024 // esize, plain.numel()
    big_out = torch.full((gout + n + gout,), sentinel, dtype=ity, device=device).view(dtype)
    out = big_out[gout:gout + n].view(plain.shape)
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    code = _lib.load().mvn_v2v_front(xin.data_ptr(), packed.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(),
                                     _dtype_code(dtype), B, V, _stream(xin))
    _lib.check(code, "mvn_v2v_front")
    torch.cuda.synchronize()
    raw = big_out.view(ity)
    assert bool((raw[:gout] == sentinel).all()) and bool((raw[gout + n:] == sentinel).all())
    assert not bool((raw[gout:gout + n] == sentinel).any())
    assert_same_bits(out, plain)
    assert bool(torch.isnan(big_in[:gin]).all()) and bool(torch.isnan(big_in[gin + xd.numel():]).all())


# ----------------------------------------------------------------------------- f. the wrapper
def test_wrapper_noncontiguous_input_and_its_checks(device):
    from mvn_rocm import _lib, v2v
    B, V = 1, 16
    x, w, scale, shift, ref = parity_case(B, V)
    packed, sc, sh = pack(w, device), scale.to(device), shift.to(device)
    ncdhw = x.bfloat16().to(device)                              # (B, 32, V, V, V)
    view = ncdhw.permute(0, 2, 3, 4, 1)
    assert not view.is_contiguous()
    assert_same_bits(v2v.v2v_front(view, packed, sc, sh), v2v.v2v_front(view.contiguous(), packed, sc, sh))
    assert_same_bits(v2v.v2v_front(view, packed, sc, sh), ref)
    cl = view.contiguous()
    with pytest.raises(RuntimeError, match="bfloat16"):
        v2v.v2v_front(cl.float(), packed, sc, sh)
    with pytest.raises(RuntimeError, match="bfloat16"):
        v2v.v2v_front(cl[..., :31], packed, sc, sh)
    with pytest.raises(RuntimeError, match="cubic"):
        v2v.v2v_front(cl[:, :, :, :8], packed, sc, sh)
    with pytest.raises(_lib.MvnError, match="mvn_v2v_front"):
        v2v.v2v_front(torch.zeros((1, 24, 24, 24, CI), dtype=torch.bfloat16, device=device), packed, sc, sh)


# ----------------------------------------------------------------------------- g. one call, small
@pytest.mark.parametrize("coords_kind", ("volume", "cuboids"))
def test_one_call_pipeline_small_with_a_nan_pixel(device, coords_kind):
    """unproject_v2v_front at V = 32, B = 3 in groups of 2 (ragged), 1 and the default, bf16
    features, 'sum' aggregation, one NaN feature pixel of frame 1 where the volume's centre
    projects: bit-identical, NaN included, to v2v_front(unproject_channels_last(...)); the NaN
    stays in a part of its frame."""
    from mvn_rocm import synth, v2v
    B, V = 3, 32
    vb = synth.volumetric_batch(B, volume=V, dtype=torch.bfloat16, device=device, seed=59)
    coords = vb.cuboids(device) if coords_kind == "cuboids" else vb.coords
    P = vb.proj[1, 0].double().cpu()
    uvw = P @ torch.cat([vb.base_points[1].double().cpu(), torch.ones(1, dtype=torch.float64)])
    u, v = int(uvw[0] / uvw[2]), int(uvw[1] / uvw[2])
    H, W = vb.features.shape[-2:]
    assert 0 <= u < W and 0 <= v < H
    feat = vb.features.clone()
    feat[1, 0, 7, v, u] = float("nan")
    g = torch.Generator().manual_seed(59)
    w = torch.randn((CO, CI, KS, KS, KS), generator=g) * 0.02
    packed, scale, shift = v2v.fold_basic3d_block(w, torch.randn(CO, generator=g) * 0.1, torch.rand(CO, generator=g) + 0.5,
                                                  torch.randn(CO, generator=g) * 0.1, torch.zeros(CO), torch.ones(CO),
                                                  device=device)
    cl = v2v.unproject_channels_last(feat, vb.proj, coords, "sum")
    ref = v2v.v2v_front(cl, packed, scale, shift, torch.float32)
    nan = torch.isnan(ref)
    assert 0 < int(nan[1].sum()) < nan[1].numel()
    assert not bool(nan[0].any()) and not bool(nan[2].any())
    for gf in (2, 1, 0):
        got = v2v.unproject_v2v_front(feat, vb.proj, coords, packed, scale, shift, "sum", torch.float32, gf)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), gf
