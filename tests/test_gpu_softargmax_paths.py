"""The forward 3D soft-argmax (csrc/softargmax.hip) on every path of its pass 1, at the joint
counts, alignments, strides and partial counts where the three launches take other code, and on
non-finite voxels.  MI355X only.

Pass 1 takes, per wave: A, the buffer-descriptor ring (full 1,024-voxel chunk, `vec_ok`, J <= 64,
frame and joint stride below 2^31 bytes); B, the pointer ring (the same chunks otherwise); C, the
generic path (`vec_ok` false or a partial chunk).  `_paths` restates that rule from the launch
code, and every case asserts the paths it was built for before it runs.

Every call goes through the C ABI on buffers the test owns: the volume is an `as_strided` view
of a flat buffer whose other elements are NaN (a read outside the view poisons the result), and
out_xyz, out_vol and the workspace (handed over with exactly its required size) lie between
guards of a NaN with its own payload, which must be unchanged, bit for bit, after the call and
must not remain anywhere inside an output.

Reference: the C oracle (double accumulation) on the same values, for bf16 on the bf16-rounded
ones; for the non-finite cases torch on the CPU (softmax / relu, then einsum: op.py:89-94) in
float64.  Bars, the project's own (tests/test_gpu_parity.py), applied PER (frame, joint):
coordinates and f32 volumes <= 1e-5 of the joint's denominator, bf16 volumes rtol 2^-8 per
element.  A joint's denominator is max |ref| of the joint; for relu-mode coordinates, whose
signed terms cancel, the float64 sum of relu(x_i) * max_c |coords_i,c|.  Every test prints its
worst error as a fraction of its bar (DESIGN.md records them)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import capi
from oracle.backward_cases import bf16_round, max_rel_per

pytestmark = pytest.mark.gpu

GUARD = 64                   # sentinel elements in front of every owned buffer
GUARD_AFTER = 64 + 4096      # and behind it: more than one finalize block's 4,096 voxels
SENTINEL = {torch.float32: 0x7FC12345, torch.bfloat16: 0x7FE5}      # quiet NaNs, own payloads
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
# (volume dtype, out_vol dtype or None for out_vol = NULL)
VARIANTS = (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", None))
VARIANT_IDS = ["f32-f32", "bf16-bf16", "bf16-f32", "f32-null"]
WITH_VOLUME = VARIANTS[:3]
MODES = (True, False)
MODE_IDS = ["softmax", "relu"]
BAR = 1e-5
BF16_RTOL = 2.0 ** -8
CUBE = (16, 16, 16)          # 4,096 voxels: four full pass-1 chunks


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _owned(n, dtype, device, offset=0):
    """(buffer, its n live elements starting `offset` elements past the front guard); every
    element holds the sentinel."""
    buf = torch.empty(GUARD + offset + n + GUARD_AFTER, dtype=dtype, device=device)
    _bits(buf).fill_(SENTINEL[dtype])
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _assert_guards(buf, offset, n, what):
    b, s = _bits(buf), SENTINEL[buf.dtype]
    front, back = b[:GUARD + offset], b[GUARD + offset + n:]
    assert bool((front == s).all()), f"{what}: {int((front != s).sum())} elements in front of the buffer were written"
    assert bool((back == s).all()), f"{what}: {int((back != s).sum())} elements past the end of the buffer were written"
    left = int((b[GUARD + offset:GUARD + offset + n] == s).sum())
    assert left == 0, f"{what}: {left} of {n} elements were not written"


def _paths(ptr, bstride, jstride, esize, nvox, J, out_ptr):
    """The pass-1 paths a launch takes (softargmax.hip: `launch`'s vec_ok, the two ring
    conditions of softargmax_partials), as a sorted string of A / B / C."""
    vec_ok = (ptr % 16 == 0 and (bstride * esize) % 16 == 0 and (jstride * esize) % 16 == 0 and nvox % 8 == 0
              and (out_ptr is None or out_ptr % 16 == 0))
    if not vec_ok:
        return "C"
    frame_bytes = ((J - 1) * jstride + nvox) * esize
    taken = set()
    if nvox >= 1024:
        taken.add("A" if J <= 64 and frame_bytes < 2 ** 31 and jstride * esize < 2 ** 31 else "B")
    if nvox % 1024:
        taken.add("C")
    return "".join(sorted(taken))


def _place(vals, dtype, device, offset=0, jstride=None, bstride=None):
    """vals (B, J, nvox) float32 on the CPU -> a (B, J, nvox) view with the given element offset
    and strides of a flat device buffer that is NaN everywhere else.  Default strides: joints
    contiguous, frames 32 elements apart from each other's end (rounded to 16 bytes)."""
    B, J, n = vals.shape
    js = n if jstride is None else jstride
    bs = (J * js + 32 + 7) // 8 * 8 if bstride is None else bstride
    assert js >= n and bs >= (J - 1) * js + n
    flat = torch.full((offset + (B - 1) * bs + (J - 1) * js + n,), float("nan"), dtype=dtype, device=device)
    view = torch.as_strided(flat, (B, J, n), (bs, js, 1), offset)
    view.copy_(vals.to(dtype))
    return view


def _run(view, shape, coords, softmax, mult, out, expect, out_offset=0, cuboids=None):
    """mvn_softargmax3d (mvn_softargmax3d_cuboid with `cuboids` (B, 18)) on owned buffers ->
    (xyz (B, J, 3) float32, out_vol (B, J, Vx, Vy, Vz) as float32 or None), both numpy."""
    from mvn_rocm import _lib
    lib = _lib.load()
    dev = view.device
    B, J, n = view.shape
    Vx, Vy, Vz = shape
    assert n == Vx * Vy * Vz and view.stride(2) == 1
    out_dtype = DTYPES[out] if out else None
    xyz_buf, xyz = _owned(B * J * 3, torch.float32, dev)
    ws_bytes = lib.mvn_softargmax3d_workspace_bytes(B, J, Vx, Vy, Vz)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws_buf, ws = _owned(ws_bytes // 4, torch.float32, dev)
    assert ws.data_ptr() % 16 == 0
    vol_buf, vol = _owned(B * J * n, out_dtype, dev, out_offset) if out else (None, None)
    code = {torch.float32: _lib.MVN_DTYPE_F32, torch.bfloat16: _lib.MVN_DTYPE_BF16}
    out_ptr = vol.data_ptr() if out else None
    took = _paths(view.data_ptr(), view.stride(0), view.stride(1), view.element_size(), n, J, out_ptr)
    assert took == expect, f"the case was built for path {expect} and takes {took}"
    head = (view.data_ptr(), code[view.dtype], view.stride(0), view.stride(1))
    tail = (float(mult), int(softmax), xyz.data_ptr(), out_ptr, code[out_dtype or view.dtype], ws.data_ptr(), ws_bytes, B, J)
    stream = torch.cuda.current_stream().cuda_stream
    if cuboids is None:
        _lib.check(lib.mvn_softargmax3d(*head, coords.data_ptr(), *tail, Vx, Vy, Vz, stream), "mvn_softargmax3d")
    else:
        assert Vx == Vy == Vz
        _lib.check(lib.mvn_softargmax3d_cuboid(*head, cuboids.data_ptr(), 0, *tail, Vx, stream), "mvn_softargmax3d_cuboid")
    torch.cuda.synchronize()
    # the workspace's own elements need not all be written (it is sized for the smallest chunk)
    b, s = _bits(ws_buf), SENTINEL[torch.float32]
    assert bool((b[:GUARD] == s).all()) and bool((b[GUARD + ws_bytes // 4:] == s).all()), "workspace overrun"
    _assert_guards(xyz_buf, 0, B * J * 3, "out_xyz")
    if out:
        _assert_guards(vol_buf, out_offset, B * J * n, "out_vol")
    return (xyz.view(B, J, 3).cpu().numpy(),
            vol.view(B, J, Vx, Vy, Vz).float().cpu().numpy() if out else None)


# ---------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def _coords(shape, B):
    """(B, Vx, Vy, Vz, 3) float32 on the CPU: a corner of synth's rotated coordinate volume."""
    from mvn_rocm import synth
    c = synth.volumetric_batch(B, n_views=2, channels=1, heatmap=8, volume=max(shape), seed=5).coords
    return c[:, :shape[0], :shape[1], :shape[2]].contiguous()


@functools.lru_cache(maxsize=None)
def _coords_on(shape, B, device):
    return _coords(shape, B).to(device)


@functools.lru_cache(maxsize=None)
def _values(shape, B, J, vol_dt):
    """(B, J, nvox) float32 on the CPU, 3 * randn, bf16-rounded for a bf16 volume."""
    g = torch.Generator().manual_seed(7919 * J + int(np.prod(shape)) + B)
    v = 3.0 * torch.randn((B, J, int(np.prod(shape))), generator=g)
    return bf16_round(v) if vol_dt == "bf16" else v


def _relu_denominator(vals, coords, mult):
    """(B, J) float64: sum_i relu(mult * x_i) * max_c |coords_i,c| (non-finite terms left out)."""
    B, J, n = vals.shape
    x = (np.asarray(vals, np.float32) * np.float32(mult)).astype(np.float64)
    x = np.where(np.isfinite(x) & (x > 0), x, 0.0)
    cmax = np.abs(np.asarray(coords, np.float64)).reshape(B, n, 3).max(-1)
    return np.einsum("bjn,bn->bj", x, cmax)


@functools.lru_cache(maxsize=None)
def _oracle(shape, B, J, vol_dt, softmax, mult):
    vals, coords = _values(shape, B, J, vol_dt), _coords(shape, B)
    xyz, vol = capi.softargmax3d(vals.view(B, J, *shape).numpy(), coords.numpy(), softmax, mult)
    den = _relu_denominator(vals.numpy(), coords.numpy(), mult)
    for a in (xyz, vol, den):
        a.setflags(write=False)
    return xyz, vol, den


def _assert_within_bars(xyz, vol, ref_xyz, ref_vol, relu_den, softmax, out, what):
    """The per-(frame, joint) bars of the module docstring on finite references."""
    if softmax:
        rx = max_rel_per(xyz, ref_xyz, 2)
    else:
        err = np.abs(np.asarray(xyz, np.float64) - ref_xyz).max(-1)
        rx = err / np.where(relu_den > 0, relu_den, 1.0)
    line = f"{what}: worst joint / bar: xyz {rx.max() / BAR:.3f}"
    rv = None
    if out == "f32":
        rv = max_rel_per(vol, ref_vol, 2) / BAR
    elif out == "bf16":
        r64 = np.asarray(ref_vol, np.float64)
        rv = (np.abs(vol - r64) / (BF16_RTOL * np.abs(r64) + 1e-30)).reshape(r64.shape[0], r64.shape[1], -1).max(-1)
    if rv is not None:
        line += f", vol {rv.max():.3f}"
    print(line)
    assert not np.isnan(xyz).any(), what
    assert (rx <= BAR).all(), (what, rx / BAR)
    if rv is not None:
        assert not np.isnan(vol).any(), what
        assert (rv <= 1.0).all(), (what, rv)


def _check_case(device, shape, B, J, vol_dt, out, softmax, mult, expect, what, out_offset=0, **layout):
    vals = _values(shape, B, J, vol_dt)
    view = _place(vals, DTYPES[vol_dt], device, **layout)
    xyz, vol = _run(view, shape, _coords_on(shape, B, device), softmax, mult, out, expect, out_offset)
    ref_xyz, ref_vol, den = _oracle(shape, B, J, vol_dt, softmax, mult)
    _assert_within_bars(xyz, vol, ref_xyz, ref_vol, den, softmax, out, what)
    return xyz, vol


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits"


# ---------------------------------------------------------------- joint counts on path A
# ring depth PF = 4 (f32) / 8 (bf16): fewer joints than the ring, exactly the ring, one more; the
# flush's last lane (64)
@pytest.mark.parametrize("J", (1, 3, 4, 5, 8, 9, 63, 64))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_path_a_joint_counts(device, variant, softmax, J):
    _check_case(device, CUBE, 2, J, *variant, softmax, 1.0, "A", f"path A, J={J}")


# ---------------------------------------------------------------- path B: more than 64 joints
@pytest.mark.parametrize("J", (65, 67, 130))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_path_b_joint_counts(device, variant, softmax, J):
    _check_case(device, CUBE, 2, J, *variant, softmax, 1.0, "B", f"path B, J={J}")


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_path_b_through_the_cuboid_entry(device, variant, softmax):
    """J = 67 with the coordinates formed in-kernel: the bits of the call on the materialised
    coordinate volume (mvn_coord_volumes), and the oracle on that volume."""
    from mvn_rocm import synth, volumetric
    vol_dt, out = variant
    B, J, V = 2, 67, 16
    vb = synth.volumetric_batch(B, n_views=2, channels=1, heatmap=8, volume=V, seed=5)
    cub = volumetric.build_cuboids(vb.base_points64, synth.CUBOID_SIDE, V, vb.thetas, device=device)
    coords = cub.coord_volumes()
    vals = _values(CUBE, B, J, vol_dt)
    view = _place(vals, DTYPES[vol_dt], device)
    xa, va = _run(view, CUBE, None, softmax, 1.3, out, "B", cuboids=cub.params)
    xb, vb_ = _run(view, CUBE, coords, softmax, 1.3, out, "B")
    _same_bits(xa, xb, "cuboid entry xyz")
    if out:
        _same_bits(va, vb_, "cuboid entry volume")
    cn = coords.cpu().numpy()
    ref_xyz, ref_vol = capi.softargmax3d(vals.view(B, J, V, V, V).numpy(), cn, softmax, 1.3)
    _assert_within_bars(xa, va, ref_xyz, ref_vol, _relu_denominator(vals.numpy(), cn, 1.3), softmax, out,
                        "path B, cuboid entry, J=67")


# ---------------------------------------------------------------- path independence
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", WITH_VOLUME, ids=VARIANT_IDS[:3])
def test_a_joint_has_the_same_bits_on_every_path(device, variant, softmax):
    """The three paths share reduce_values and give each lane the same voxels: joints 0, 63 and
    64 of a J = 65 call (path B) equal the same data as a J = 1 call (path A) and as a J = 1
    call on a copy one element off 16-byte alignment (path C), bit for bit."""
    vol_dt, out = variant
    B, J = 2, 65
    vals = _values(CUBE, B, J, vol_dt)
    coords = _coords_on(CUBE, B, device)
    xyz, vol = _run(_place(vals, DTYPES[vol_dt], device), CUBE, coords, softmax, 1.3, out, "B")
    for j in (0, 63, 64):
        one = vals[:, j:j + 1].contiguous()
        xa, va = _run(_place(one, DTYPES[vol_dt], device), CUBE, coords, softmax, 1.3, out, "A")
        xc, vc = _run(_place(one, DTYPES[vol_dt], device, offset=1), CUBE, coords, softmax, 1.3, out, "C")
        _same_bits(xyz[:, j:j + 1], xa, f"joint {j}: path B against path A, xyz")
        _same_bits(vol[:, j:j + 1], va, f"joint {j}: path B against path A, volume")
        _same_bits(xa, xc, f"joint {j}: path A against path C, xyz")
        _same_bits(va, vc, f"joint {j}: path A against path C, volume")


# ---------------------------------------------------------------- vec_ok == false
def _odd(vol_dt):
    """An element count that is not a multiple of 16 bytes and keeps 4-byte alignment."""
    return 1 if vol_dt == "f32" else 4


def _misalignments():
    """(id, variant, layout of _check_case) of each single cause of vec_ok == false on 16^3, J = 5."""
    n, J = 4096, 5
    out = []
    for variant, vid in zip(VARIANTS, VARIANT_IDS):
        vol_dt = variant[0]
        js = n + _odd(vol_dt)
        out.append((f"base+1-{vid}", variant, dict(offset=1)))
        out.append((f"jstride-{vid}", variant, dict(jstride=js, bstride=(J * js + 32 + 7) // 8 * 8)))
        out.append((f"bstride-{vid}", variant, dict(bstride=J * n + 32 + _odd(vol_dt))))
        if variant[1]:
            out.append((f"out+1-{vid}", variant, dict(out_offset=1)))
    return out


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", _misalignments(), ids=lambda c: c[0])
def test_each_cause_of_the_generic_path(device, case, softmax):
    what, variant, layout = case
    _check_case(device, CUBE, 2, 5, *variant, softmax, 1.0, "C", f"path C, {what}", **layout)


@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_voxel_count_not_a_multiple_of_8(device, variant, softmax):
    """9 x 11 x 13 = 1,287 voxels: one full and one partial chunk, every run through the scalar
    tails of load_run / store_run."""
    _check_case(device, (9, 11, 13), 2, 5, *variant, softmax, 1.0, "C", "path C, 9x11x13")


# ---------------------------------------------------------------- a ring path and C in one launch
@pytest.mark.parametrize("J,expect", ((5, "AC"), (65, "BC")))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_full_and_partial_chunks_in_one_launch(device, variant, softmax, J, expect):
    """10 x 12 x 20 = 2,400 voxels, aligned: two full chunks and 352 voxels more."""
    _check_case(device, (10, 12, 20), 2, J, *variant, softmax, 1.0, expect, f"paths {expect}, 10x12x20, J={J}")


# ---------------------------------------------------------------- the combine's 4-at-a-time loop
# npart 1, 63, 65 (no round), 200 (lanes 0-7 take a round, the others the tail only), 264 (every
# lane a round, lanes 0-7 a tail)
@pytest.mark.parametrize("shape,npart", (((8, 8, 16), 1), ((32, 32, 63), 63), ((40, 52, 32), 65),
                                         ((64, 64, 50), 200), ((64, 64, 66), 264)),
                         ids=lambda v: str(v) if isinstance(v, int) else "x".join(map(str, v)))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
def test_combine_partial_counts(device, softmax, shape, npart):
    assert (int(np.prod(shape)) + 1023) // 1024 == npart
    _check_case(device, shape, 1, 2, "f32", "f32", softmax, 1.0, "A", f"combine, npart={npart}")


# ---------------------------------------------------------------- strides at the 2^31-byte limits
@pytest.mark.parametrize("limit", ("jstride_bytes_2^31", "frame_bytes_below_2^31"))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("vol_dt", ("f32", "bf16"))
def test_joint_strides_at_the_2_31_byte_limits(device, vol_dt, softmax, limit):
    """Two joints 2^31 bytes apart (the pointer ring), and at the largest 16-byte-aligned stride
    that keeps the frame below 2^31 bytes (the buffer-descriptor ring at its limit: 32-bit
    offsets), on an uninitialised buffer of a little over 2 GiB of which only the joints' 4,096
    voxels are written: both equal the contiguous call bit for bit."""
    dtype = DTYPES[vol_dt]
    esize, n, J = (4 if vol_dt == "f32" else 2), 4096, 2
    vals = _values(CUBE, 1, J, vol_dt)
    coords = _coords_on(CUBE, 1, device)
    ref_xyz, ref_vol = _run(_place(vals, dtype, device), CUBE, coords, softmax, 1.0, vol_dt, "A")
    oxyz, ovol, den = _oracle(CUBE, 1, J, vol_dt, softmax, 1.0)
    _assert_within_bars(ref_xyz, ref_vol, oxyz, ovol, den, softmax, vol_dt, f"2^31, contiguous, {vol_dt}")
    if limit == "jstride_bytes_2^31":
        js, expect = 2 ** 31 // esize, "B"
    else:
        js, expect = (2 ** 31 - n * esize - 16) // esize, "A"
        assert (js * esize) % 16 == 0 and (js + n) * esize < 2 ** 31 <= (js + 16 // esize + n) * esize
    flat = torch.empty((js + n,), dtype=dtype, device=device)
    try:
        view = torch.as_strided(flat, (1, J, n), (J * js, js, 1), 0)
        view.copy_(vals.to(dtype))
        xyz, vol = _run(view, CUBE, coords, softmax, 1.0, vol_dt, expect)
    finally:
        del flat
        view = None
        torch.cuda.empty_cache()
    _same_bits(xyz, ref_xyz, f"{limit}: xyz against the contiguous call")
    _same_bits(vol, ref_vol, f"{limit}: volume against the contiguous call")


# ---------------------------------------------------------------- multiplier
@pytest.mark.parametrize("mult", (-1.3, 0.0))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_negative_and_zero_multiplier(device, variant, softmax, mult):
    _check_case(device, CUBE, 2, 5, *variant, softmax, mult, "A", f"multiplier {mult}")


# ---------------------------------------------------------------- non-finite voxels
def _torch_reference(vals, coords, softmax, mult):
    """op.py:89-94 on the CPU in float64, on the float32 products x * mult -> (xyz, volumes)."""
    B, J, n = vals.shape
    v = (vals.float() * torch.tensor(mult, dtype=torch.float32)).double()
    p = F.softmax(v, dim=2) if softmax else F.relu(v)
    xyz = torch.einsum("bnv,bvc->bnc", p, coords.double().view(B, n, 3))
    return xyz.numpy(), p.numpy()


def _assert_follows_torch(got, ref, bar_of_joint, what):
    """NaN and +-inf at the same elements; the finite elements of every (frame, joint) within
    bar_of_joint(got, ref, finite mask, b, j) -> error / bar."""
    ref32 = np.asarray(ref, np.float64).astype(np.float32)
    assert (np.isnan(got) == np.isnan(ref32)).all(), \
        f"{what}: NaN at {int((np.isnan(got) != np.isnan(ref32)).sum())} other elements than torch"
    inf = np.isinf(ref32)
    assert (np.isinf(got) == inf).all() and (got[inf] == ref32[inf]).all(), f"{what}: infinities differ from torch"
    B, J = got.shape[:2]
    worst = 0.0
    for b in range(B):
        for j in range(J):
            fin = np.isfinite(ref32[b, j])
            if fin.any():
                r = bar_of_joint(np.asarray(got[b, j], np.float64), np.asarray(ref[b, j], np.float64), fin, b, j)
                worst = max(worst, r)
                assert r <= 1.0, (what, b, j, r)
    return worst


NONFINITE_LAYOUTS = {"A": (4, dict()), "B": (66, dict()), "C": (4, dict(offset=1))}


@pytest.mark.parametrize("path", tuple(NONFINITE_LAYOUTS))
@pytest.mark.parametrize("softmax", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_nonfinite_voxels_follow_torch(device, variant, softmax, path):
    """Frame 1: one NaN voxel in joint 1, one +inf voxel in joint 2.  torch's softmax makes both
    joints NaN throughout; torch's relu keeps the NaN and the +inf at their voxels and the
    coordinates take them through the einsum.  Joint 0 and frame 0 are clean: finite, and the
    bits of the call without the two voxels."""
    vol_dt, out = variant
    B = 2
    J, layout = NONFINITE_LAYOUTS[path]
    clean = _values(CUBE, B, J, vol_dt)
    vals = clean.clone()
    vals[1, 1, 1500] = float("nan")
    vals[1, 2, 3000] = float("inf")
    coords, dtype = _coords(CUBE, B), DTYPES[vol_dt]
    cdev = _coords_on(CUBE, B, device)
    xyz, vol = _run(_place(vals, dtype, device, **layout), CUBE, cdev, softmax, 1.0, out, path)
    xyz0, vol0 = _run(_place(clean, dtype, device, **layout), CUBE, cdev, softmax, 1.0, out, path)
    ref_xyz, ref_vol = _torch_reference(vals, coords, softmax, 1.0)
    den = _relu_denominator(vals.numpy(), coords.numpy(), 1.0)

    def xyz_bar(g, r, fin, b, j):
        d = np.abs(r[fin]).max() if softmax else den[b, j]
        return np.abs(g[fin] - r[fin]).max() / (d if d > 0 else 1.0) / BAR

    def vol_bar(g, r, fin, b, j):
        if out == "bf16":
            return (np.abs(g[fin] - r[fin]) / (BF16_RTOL * np.abs(r[fin]) + 1e-30)).max()
        d = np.abs(r[fin]).max()
        return np.abs(g[fin] - r[fin]).max() / (d if d > 0 else 1.0) / BAR

    what = f"non-finite, path {path}"
    wx = _assert_follows_torch(xyz, ref_xyz, xyz_bar, what + " xyz")
    wv = _assert_follows_torch(vol, ref_vol.reshape(vol.shape), vol_bar, what + " volume") if out else 0.0
    print(f"{what}: worst finite joint / bar: xyz {wx:.3f}, vol {wv:.3f}")
    # what torch does, spelled out: the reference above must show it too
    bad = (1, 2) if softmax else (1,)
    assert np.isnan(ref_xyz[1, list(bad)]).all() and np.isnan(xyz[1, list(bad)]).all()
    if not softmax:
        assert not np.isfinite(xyz[1, 2]).any()
        if out:
            flat = vol.reshape(B, J, -1)
            assert np.isnan(flat[1, 1, 1500]) and np.isnan(flat[1, 1]).sum() == 1
            assert flat[1, 2, 3000] == np.inf and np.isinf(flat[1, 2]).sum() == 1
    others = [(b, j) for b in range(B) for j in range(J) if not (b == 1 and j in (1, 2))]
    for b, j in others:
        assert np.isfinite(xyz[b, j]).all()
        _same_bits(xyz[b, j], xyz0[b, j], f"{what}: clean joint ({b}, {j}) xyz")
        if out:
            assert np.isfinite(vol[b, j]).all()
            _same_bits(vol[b, j], vol0[b, j], f"{what}: clean joint ({b}, {j}) volume")
