"""The V2V head (csrc/v2v_head.hip) at its edges, without a tolerance.

tests/test_gpu_v2v_head.py feeds the kernel random normal data, where an f32 sum taken in another
order can push a hidden activation across a bf16 rounding boundary, and therefore accepts a share
of voxels off the bar.  The head is pointwise, so here it gets operands for which the kernel has
no freedom at all, and every logit, f32 and bf16, must equal a float64 reference bit for bit:

* integer family: x integers in [-3, 3], dense integer weights in [-2, 2], scale1 in +-{1/2, 1, 2},
  scale2 in +-{1/8, 1/4}, shifts multiples of 1/4 in [-2, 2], integer output bias.  Every product is
  a multiple of the layer's input quantum 2^-q and sum |w||h| * 2^q < 2^24, so every f32 partial
  sum is exact in any order; scale is a power of two, so acc * scale + shift rounds once (the fma),
  as the float64 value cast to f32 does.  The hidden activations need more than 8 significant bits
  often enough, ties included, to pin both bf16 roundings (the guards below count them).
* one product per sum: every row of W1, W2, W3 has one nonzero with a full 8-bit significand, x
  is arbitrary bf16 with full significands, scale +-2^k, shift and bias nonzero.  Each accumulation
  is one 16-bit product, exact in f32, and the hidden roundings see arbitrary low bits: this pins
  every significand bit of the packed weights and the K-slot permutation of layers 2 and 3.

The parameters go through the real fold (BatchNorm with running_var + eps an exact power of four
— eps = 2^-20, since torch's batch_norm refuses eps = 0 and the modules themselves are run below
— and weight a power of two) and the test asserts that the folded scale_shift is exactly what was
meant.
The reference is computed from the modules' own weights: h = bf16(x); per layer r = W h * scale +
shift in float64, y = +0 where r <= 0 and r otherwise (NaN kept), cast to f32, .bfloat16(); logits
= W3 h2 + b3 cast to f32, and .bfloat16() of that for bf16 logits.  It asserts its own exactness
conditions (above; no -0 in r or in the logits) before it returns.

Which test covers which edge of the kernel (blocks of 2048 voxels, 4 waves x 8 chunks of 64):

  test_tiny_frames              S = 1, 2, 3 (the S - 1 clamp of the per-element path), S = 4 (VEC,
                                vc clamps to 0 in every lane), S = 5, 8
  test_loop_and_grid[8x16x16]   S = 2048: one full block, all 8 iterations of the `it` loop
  test_loop_and_grid[12x12x15]  S = 2160: a second block, wave 0 full, wave 1 with 48 voxels, waves
                                2-3 leave at `base >= S`; VEC
  test_loop_and_grid[13x13x13]  S = 2197: the same grid per element, odd frames misaligned
  test_loop_and_grid[2x2x457]   S = 1828: `vn < S` fails after iteration 6 for waves 1-3 only, wave
                                0 goes on to a 36-voxel chunk; VEC
  test_loop_and_grid[7x9x29]    S = 1827: the same per element
  test_every_j                  J = 1, 4, 15, 16, 17, 31, 32: the bias3 clamp and the `two` switch
  test_one_product_per_sum      packed significand bits, kslot, RNE of arbitrary low bits
  test_misaligned_pointers      the per-element path chosen by a pointer alone (S % 4 == 0)
  test_full_size_channels_last  64^3, B = 2, J = 17, channels-last bf16: the whole volume
  test_beyond_2_31_bytes        V = 256, x of 4 GiB: byte offsets past 2^31
  test_nonfinite_with_zero_weights   NaN and +-inf voxels, 0 * inf included
  test_one_call_ragged_and_multiblock   mvn_v2v_head_softargmax off the aligned 8^3 case

In the f32 layout x carries sub-ulp offsets (quarter ulps, ties among them) that round-to-
nearest-even must remove, so the kernel's own conversion of x is pinned too.  The tests without a
gpu mark need no GPU: they check that the data make the comparison bite.  Reads nothing outside
the repository.
"""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from conftest import assert_bits_equal
from test_gpu_v2v_head import C, LAYOUTS, as_layout, run_head
from v2v_kit import Basic3DBlock

DTYPES = (torch.float32, torch.bfloat16)
JS = (1, 4, 15, 16, 17, 31, 32)


# ----------------------------------------------------------------------------- helpers
def bits(t):
    """The bit pattern of an f32 / bf16 tensor as a numpy unsigned array (on the host)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    assert t.dtype == torch.bfloat16
    return t.view(torch.int16).numpy().view(np.uint16)


def assert_same_bits(got, want):
    if got.dtype == torch.float32:
        return assert_bits_equal(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    a, b = bits(got), bits(want)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} bf16 elements differ in their bits"


def vid(vol):
    return "x".join(map(str, vol))


def has_neg_zero(t):
    return bool((torch.signbit(t) & (t == 0)).any())


def quantum(t):
    """The smallest q >= 0 with t * 2^q an integer at every finite element."""
    t = t[torch.isfinite(t)]
    for q in range(64):
        s = t * 2.0 ** q
        if bool((s == s.round()).all()):
            return q
    raise AssertionError("no binary quantum")


def exact_sum(a, b):
    """a + b in float64 and whether it is exact at every finite element (TwoSum's error term)."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return s, bool((err[torch.isfinite(s)] == 0).all())


# ----------------------------------------------------------------------------- parameters
EPS = 2.0 ** -20      # torch's batch_norm refuses eps = 0; running_var + EPS is an exact power of four instead


def build_modules(W, scale, shift, b3, conv_bias, mean):
    """Eval-mode (block1, block2, output_conv) whose fold is exactly `scale` (+-2^k) and `shift`:
    running_var = 4^a - eps (a cycles through -1, 0, 1; exact in f32, and running_var + eps is
    exactly 4^a in f32 and in float64), weight = +-2^(k + a), and bias = shift - (conv_bias -
    running_mean) * scale.  All (2, 32) float64, W[l] float64."""
    blocks = [Basic3DBlock(C, C, 1), Basic3DBlock(C, C, 1)]
    out = nn.Conv3d(C, W[2].shape[0], 1)
    a = (torch.arange(C) % 3 - 1).double()
    with torch.no_grad():
        for l, blk in enumerate(blocks):
            conv, bn = blk.block[0], blk.block[1]
            conv.weight.copy_(W[l].view(C, C, 1, 1, 1))
            conv.bias.copy_(conv_bias[l])
            bn.eps = EPS
            bn.running_var.copy_(torch.exp2(2 * a) - EPS)
            assert torch.equal(bn.running_var.double() + EPS, torch.exp2(2 * a))
            bn.weight.copy_(scale[l] * torch.exp2(a))
            bn.running_mean.copy_(mean[l])
            beta = shift[l] - (conv_bias[l] - mean[l]) * scale[l]
            assert torch.equal(beta.float().double(), beta)
            bn.bias.copy_(beta)
        out.weight.copy_(W[2].view(-1, C, 1, 1, 1))
        out.bias.copy_(b3)
        for conv, w in zip((blocks[0].block[0], blocks[1].block[0], out), W):    # nothing was rounded
            assert torch.equal(conv.weight.double().view(w.shape), w)
            assert torch.equal(conv.weight.bfloat16().float(), conv.weight)
    for m in (*blocks, out):
        m.eval()
    return blocks[0], blocks[1], out


def make_head(W, scale, shift, b3, conv_bias, mean, family):
    mods = build_modules(W, scale, shift, b3, conv_bias, mean)
    return SimpleNamespace(W=W, scale=scale, shift=shift, b3=b3, modules=mods, J=W[2].shape[0], family=family)


@functools.lru_cache(maxsize=None)
def integer_head(J, seed):
    """Dense integer weights in [-2, 2], scale1 in +-{1/2, 1, 2}, scale2 in +-{1/8, 1/4} (negative
    on every fifth channel), shifts multiples of 1/4 in [-2, 2] (never -0), integer conv biases,
    running means and output bias."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    W = [ri(-2, 2, (C, C)), ri(-2, 2, (C, C)), ri(-2, 2, (J, C))]
    sign = torch.where(torch.arange(C) % 5 == 2, -1.0, 1.0).double()
    scale = torch.stack([sign * torch.exp2(ri(-1, 1, (C,))), sign.roll(1) * torch.exp2(ri(-3, -2, (C,)))])
    shift = ri(-8, 8, (2, C)) / 4 + 0.0
    assert not has_neg_zero(shift)
    return make_head(W, scale, shift, ri(-3, 3, (J,)), ri(-1, 1, (2, C)), ri(-1, 1, (2, C)), "integer")


def full8(g, shape, klo, khi):
    """Random values +-(128 + n) / 128 * 2^k, n in 0..127, k in klo..khi: full 8-bit significands."""
    n = torch.randint(0, 128, shape, generator=g).double()
    k = torch.randint(klo, khi + 1, shape, generator=g).double()
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return s * (128 + n) / 128 * torch.exp2(k)


@functools.lru_cache(maxsize=None)
def single_head(J, seed):
    """One nonzero per row of W1, W2, W3, in a random column (columns repeat), of either sign,
    with a full 8-bit significand; scale +-2^k, shift and output bias nonzero, 8-bit too."""
    g = torch.Generator().manual_seed(seed)
    W = []
    for rows in (C, C, J):
        w = torch.zeros(rows, C, dtype=torch.float64)
        w[torch.arange(rows), torch.randint(0, C, (rows,), generator=g)] = full8(g, (rows,), -2, 2)
        W.append(w)
    sgn = torch.randint(0, 2, (2, C), generator=g).double() * 2 - 1
    scale = sgn * torch.exp2(torch.randint(-2, 3, (2, C), generator=g).double())
    zero = torch.zeros(2, C, dtype=torch.float64)
    return make_head(W, scale, full8(g, (2, C), -3, 1), full8(g, (J,), -3, 1), zero, zero, "single")


def fold_checked(head, device):
    """fold_v2v_head of the modules; the fold must hold exactly the intended values."""
    from mvn_rocm import v2v
    packed, ss, b3 = v2v.fold_v2v_head(*head.modules, device=device)
    want = torch.stack([head.scale, head.shift], dim=1)                      # (2, 2, 32)
    assert torch.equal(want.float().double(), want)
    assert torch.equal(ss.cpu().double(), want), "the fold is not the exact scale and shift this test intends"
    assert not has_neg_zero(ss.cpu())
    assert torch.equal(b3.cpu().double(), head.b3)
    return packed, ss, b3


@functools.lru_cache(maxsize=None)
def device_params(kind, J, seed, device):
    return fold_checked(HEADS[kind](J, seed), device)


# ----------------------------------------------------------------------------- the reference
def reference(x, head):
    """x (B, 32, S) f32 as the kernel reads it -> SimpleNamespace(f32 = logits (B, J, S) f32,
    bf16 = their .bfloat16(), r = [r1, r2] float64 pre-activations, y = [y1, y2] the f32
    activations before their bf16 rounding).  Asserts the conditions under which the kernel has
    no freedom to differ."""
    h = x.float().bfloat16().double()
    rs, ys = [], []
    for l in range(3):
        W = head.W[l]
        hf = torch.where(torch.isfinite(h), h, torch.zeros_like(h))
        if head.family == "integer":
            assert torch.equal(W, W.round())
            mass = torch.einsum("oc,bcs->bos", W.abs(), hf.abs()).max()
            assert float(mass) * 2.0 ** quantum(hf) < 2.0 ** 24, f"layer {l + 1}: partial sums may round in f32"
        else:
            assert bool(((W != 0).sum(dim=1) == 1).all())                    # one 8-bit x 8-bit product
            assert torch.equal(W.float().bfloat16().double(), W)
        if bool(torch.isfinite(h).all()):
            acc = torch.einsum("oc,bcs->bos", W, h)
        else:                                                                # every product formed: 0 * inf is NaN
            acc = (W.view(1, -1, C, 1) * h.unsqueeze(1)).sum(dim=2)
        if l == 2:
            logits, exact = exact_sum(acc, head.b3.view(1, -1, 1))
            assert exact and not has_neg_zero(logits)
            break
        r, exact = exact_sum(acc * head.scale[l].view(1, C, 1), head.shift[l].view(1, C, 1))
        assert exact and not has_neg_zero(r), f"layer {l + 1}: r is not exact in float64, or holds a -0"
        y = torch.where(r <= 0, torch.zeros_like(r), r).float()             # a NaN is neither: kept
        h = y.bfloat16().double()
        rs.append(r)
        ys.append(y)
    f32 = logits.float()
    return SimpleNamespace(f32=f32, bf16=f32.bfloat16(), r=rs, y=ys)


def restate_f32(x, head, order):
    """The same in f32 throughout, the channels accumulated one by one in `order`."""
    h = x.float().bfloat16().float()
    for l in range(3):
        W = head.W[l].float()
        acc = torch.zeros(h.shape[0], W.shape[0], h.shape[2])
        for c in order:
            acc += W[:, c].view(1, -1, 1) * h[:, c:c + 1]
        if l == 2:
            return acc + head.b3.float().view(1, -1, 1)
        r = acc * head.scale[l].float().view(1, C, 1) + head.shift[l].float().view(1, C, 1)    # the product is exact
        h = torch.where(r <= 0, torch.zeros_like(r), r).bfloat16().float()


def through_the_modules(x, head):
    """The nn modules themselves in f32 (v2v.py:154-160), rounded to bf16 between them."""
    b1, b2, out = head.modules
    B, _, S = x.shape
    with torch.no_grad():
        h = x.float().bfloat16().float().view(B, C, S, 1, 1)
        h = b1(h).bfloat16().float()
        h = b2(h).bfloat16().float()
        return out(h).view(B, -1, S)


# ----------------------------------------------------------------------------- the data
def sub_ulp(xb, g, ks):
    """xb (bf16-exact f32) plus k quarter-ulps away from zero, k drawn from `ks`: what an f32 x
    holds below bf16's last bit."""
    _, e = torch.frexp(xb)
    quarter = torch.exp2(e.float() - 1 - 7 - 2)                              # ulp(xb) / 4 for 8-bit significands
    k = torch.tensor(ks, dtype=torch.float32)[torch.randint(0, len(ks), xb.shape, generator=g)]
    return torch.where(xb == 0, xb, xb + torch.sign(xb) * k * quarter)


@functools.lru_cache(maxsize=None)
def make_case(kind, vol, B, J, seed=0):
    """Inputs and CPU reference, computed once per case and shared.  `x` (B, 32, S) is what the
    f32 layout is fed (sub-ulp offsets included), `seen` its bf16 rounding."""
    S = vol[0] * vol[1] * vol[2]
    head = HEADS[kind](J, 1000 + J + seed)
    g = torch.Generator().manual_seed(7 * S + 31 * J + B + seed)
    if kind == "integer":
        seen = torch.randint(-3, 4, (B, C, S), generator=g).float()
        # -1/4, +1/4 and +1/2 ulp (a tie; 1, 2 and 3 have even significands) all round back
        x = sub_ulp(seen, g, (-1.0, 0.0, 1.0, 2.0))
        assert torch.equal(x.bfloat16().float(), seen)
    else:
        x = sub_ulp(full8(g, (B, C, S), -4, 4).float(), g, (-2.0, -1.0, 0.0, 1.0, 2.0))
        seen = x.bfloat16().float()
    assert B == 1 or all(not torch.equal(seen[0], seen[f]) for f in range(1, B))
    ref = reference(seen, head)
    return SimpleNamespace(kind=kind, vol=vol, B=B, J=J, S=S, head=head, x=x, seen=seen, ref=ref, seed=1000 + J + seed)


HEADS = {"integer": integer_head, "single": single_head}


def low16(t):
    return bits(t.float()) & 0xFFFF


# ----------------------------------------------------------------------------- guards (no GPU)
LOOP_VOLUMES = ((8, 16, 16), (12, 12, 15), (13, 13, 13), (2, 2, 457), (7, 9, 29))
GUARDED = tuple(("integer", v, 2, 17) for v in LOOP_VOLUMES) + (("integer", (64, 64, 64), 2, 17),)


@pytest.mark.parametrize("key", GUARDED, ids=lambda k: vid(k[1]))
def test_integer_data_make_the_comparison_bite(key):
    """On the reference alone: both relu branches, both hidden roundings and the output rounding
    are exercised, exact ties included, and f32 in another channel order gives the same bits."""
    case = make_case(*key)
    ref = case.ref
    for r in ref.r:
        assert float((r > 0).double().mean()) >= 0.25
    assert (low16(ref.y[0]) != 0).any()                                      # h1 rounds somewhere
    assert (low16(ref.y[1]) != 0).mean() >= 0.05                             # h2 at >= 5 % of its values
    low = low16(ref.f32)
    assert (low != 0).mean() >= 0.10
    assert (low == 0x8000).any()                                             # an exact tie
    if case.S <= 4096:
        shuffled = torch.randperm(C, generator=torch.Generator().manual_seed(case.S)).tolist()
        for order in (range(C - 1, -1, -1), shuffled):
            assert_bits_equal(restate_f32(case.seen, case.head, order).numpy(), ref.f32.numpy())
    # the f32 layout's sub-ulp offsets are there, ties among them
    assert float((case.x != case.seen).float().mean()) > 0.5 and (low16(case.x) == 0x8000).any()


@pytest.mark.parametrize("vol", ((4, 4, 5), (3, 5, 7)), ids=vid)
def test_single_product_data_make_the_comparison_bite(vol):
    """Hidden activations and logits with arbitrary low bits; every weight column's significand
    differs from a power of two in most rows."""
    case = make_case("single", vol, 2, 17)
    ref = case.ref
    for r, y in zip(ref.r, ref.y):
        assert float((r > 0).double().mean()) >= 0.25
        assert (low16(y) != 0).mean() >= 0.10                                # a zero input leaves the 8-bit shift
    assert (low16(ref.f32) != 0).mean() >= 0.10
    assert_bits_equal(restate_f32(case.seen, case.head, range(C - 1, -1, -1)).numpy(), ref.f32.numpy())
    for W in case.head.W:
        nz = W[W != 0].float()
        assert ((bits(nz) >> 16) & 0x7F != 0).mean() > 0.9                   # low significand bits set


@pytest.mark.parametrize("J", (1, 17, 32))
def test_reference_equals_the_modules_on_integer_data(J):
    """b1, round to bf16, b2, round to bf16, out — the stock modules in f32 — give the reference's
    bits, and the fold of those modules is exact: the restatement is v2v.py:154-160."""
    case = make_case("integer", (13, 13, 13), 2, J)
    packed, ss, b3 = fold_checked(case.head, "cpu")
    assert_bits_equal(through_the_modules(case.seen, case.head).numpy(), case.ref.f32.numpy())
    # the packed weights are the modules' under the documented K-slots, bit for bit
    from mvn_rocm import v2v
    lane, j = torch.arange(64).view(64, 1), torch.arange(8).view(1, 8)
    for l in range(3):
        Wp = torch.zeros(C, C, dtype=torch.float64)
        Wp[:case.head.W[l].shape[0]] = case.head.W[l]
        for m in range(2):
            want = Wp[(16 * m + lane % 16).expand(64, 8), v2v.head_kslot(l)[8 * (lane // 16) + j]]
            assert torch.equal(packed[l, m].double(), want)


def test_single_product_fold_is_exact():
    fold_checked(single_head(17, 1017), "cpu")


# ----------------------------------------------------------------------------- GPU: logits, bit for bit
def check_case(device, case, layout):
    params = device_params(case.kind, case.J, case.seed, device)
    x_dev, cl, seen = as_layout(case.x, case.vol, layout, device)
    assert torch.equal(seen.bfloat16().float(), case.seen)
    for dtype in DTYPES:
        got = run_head(x_dev, params, cl, dtype)
        assert got.dtype == dtype and tuple(got.shape) == (case.B, case.J, case.S)
        assert_same_bits(got, case.ref.f32 if dtype == torch.float32 else case.ref.bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("vol", ((1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 2, 2), (1, 1, 5), (2, 2, 2)), ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tiny_frames(device, layout, vol):
    """S = 1, 2, 3, 4, 5, 8 with B = 3: every lane but the first few reads a clamped voxel."""
    check_case(device, make_case("integer", vol, 3, 17), layout)
    check_case(device, make_case("single", vol, 3, 17), layout)


@pytest.mark.gpu
@pytest.mark.parametrize("vol", LOOP_VOLUMES, ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_loop_and_grid(device, layout, vol):
    """S = 2048, 2160, 2197, 1828, 1827 (module docstring), B = 2."""
    check_case(device, make_case("integer", vol, 2, 17), layout)


@pytest.mark.gpu
@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("vol", ((4, 4, 5), (3, 5, 7)), ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_j(device, layout, vol, J):
    """J at and around 16 and 32, at a VEC shape with a ragged chunk and at an odd S; the output
    bias differs per joint, so a joint reading its neighbour's bias differs."""
    case = make_case("integer", vol, 2, J)
    assert J == 1 or case.head.b3.unique().numel() > 1
    check_case(device, case, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("J", (17, 32))
@pytest.mark.parametrize("vol", ((4, 4, 5), (3, 5, 7), (12, 12, 15)), ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_product_per_sum(device, layout, vol, J):
    check_case(device, make_case("single", vol, 2, J), layout)


# ----------------------------------------------------------------------------- GPU: pointers
def call_abi(x, layout, params, out_ptr, out_dtype, B, J, vol, x_ptr=None):
    from mvn_rocm import _lib, _ops
    code = _lib.load().mvn_v2v_head(x_ptr if x_ptr is not None else x.data_ptr(), _ops._DTYPE_CODE[x.dtype],
                                    _lib.MVN_LAYOUT_NDHWC if layout == "ndhwc_bf16" else _lib.MVN_LAYOUT_NCDHW,
                                    params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(), out_ptr,
                                    _ops._DTYPE_CODE[out_dtype], B, J, *vol, _ops._stream(x))
    _lib.check(code, "mvn_v2v_head")


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("vol", ((4, 4, 5), (12, 12, 15)), ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_misaligned_pointers(device, layout, vol, out_dtype):
    """S % 4 == 0 through the C ABI with x moved inside its allocation (f32: 4 and 8 bytes, bf16: 2)
    and `out` moved by one element, alone and together: the logits are the reference's and the
    aligned run's bits (so both bf16 conversions meet the same ties), the sentinels are intact."""
    case = make_case("integer", vol, 2, 17)
    params = device_params(case.kind, case.J, case.seed, device)
    x_dev, _, _ = as_layout(case.x, vol, layout, device)
    want = case.ref.f32 if out_dtype == torch.float32 else case.ref.bf16
    n, es = want.numel(), x_dev.element_size()
    aligned = run_head(x_dev, params, layout == "ndhwc_bf16", out_dtype)
    assert_same_bits(aligned, want)
    x_offsets = (0, 1, 2) if es == 4 else (0, 1)                             # in elements
    ran = 0
    for xo in x_offsets:
        xbuf = torch.zeros(x_dev.numel() + 8, dtype=x_dev.dtype, device=device)
        xbuf[xo:xo + x_dev.numel()].copy_(x_dev.reshape(-1))
        for oo in (0, 1):
            if xo == 0 and oo == 0:
                continue
            pad = 64 + oo
            big = torch.full((pad + n + 300,), -768.0, dtype=out_dtype, device=device)
            x_ptr, out_ptr = xbuf.data_ptr() + xo * es, big.data_ptr() + pad * big.element_size()
            assert xbuf.data_ptr() % 16 == 0 and big.data_ptr() % 16 == 0
            assert (x_ptr % 16 != 0) == (xo != 0) and (out_ptr % 16 != 0) == (oo != 0)
            call_abi(x_dev, layout, params, out_ptr, out_dtype, case.B, case.J, vol, x_ptr=x_ptr)
            torch.cuda.synchronize()
            assert bool((big[:pad] == -768.0).all()) and bool((big[pad + n:] == -768.0).all()), (xo, oo)
            assert_same_bits(big[pad:pad + n].view(want.shape), want)
            ran += 1
    assert ran == 2 * len(x_offsets) - 1


# ----------------------------------------------------------------------------- GPU: full size
@pytest.mark.gpu
def test_full_size_channels_last(device):
    """64^3, B = 2, J = 17, channels-last bf16 (what V2VEval feeds the head), integer family: all
    2 * 17 * 262,144 logits, f32 and bf16, no cap."""
    check_case(device, make_case("integer", (64, 64, 64), 2, 17), "ndhwc_bf16")


PERIOD = 61           # odd: an address off by any power of two reads another voxel vector


@pytest.mark.gpu
def test_beyond_2_31_bytes(device):
    """V = 256, NCDHW f32, J = 2, B = 2: x is 4 GiB, frame 1 begins at byte 2^31 and channel rows
    16 and up of either frame lie 2^30 bytes and more into it.  Voxel v of frame b holds vector
    v % 61 of the frame's table of 61 voxel vectors, so the expected logits are the reference of
    the table gathered the same way, compared as int32 on the device.
    Measured on the MI355X: 0.12 s for the whole test with B = 2, so B stays 2
    (profiles/v2v_head_exact.txt)."""
    t0 = time.perf_counter()
    B, J, V = 2, 2, 256
    S = V ** 3
    case = make_case("integer", (1, 1, PERIOD), B, J)
    params = device_params(case.kind, case.J, case.seed, device)
    idx = torch.arange(S, device=device) % PERIOD
    x = torch.empty((B, C, V, V, V), dtype=torch.float32, device=device)
    assert x.numel() * 4 == 1 << 32
    table = case.x.to(device)
    for b in range(B):
        torch.index_select(table[b], 1, idx, out=x[b].view(C, S))
    got = run_head(x, params, False)
    del x
    want = case.ref.f32.to(device).index_select(2, idx)
    assert got.shape == want.shape == (B, J, S)
    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
    nbad = 0 if same else int((got.view(torch.int32) != want.view(torch.int32)).sum())
    del got, want, idx
    torch.cuda.empty_cache()
    print(f"V = 256, B = {B}: {time.perf_counter() - t0:.2f} s for the whole test")
    assert same, f"{nbad} logits differ in their bits"


# ----------------------------------------------------------------------------- GPU: NaN and inf
IN_POS, IN_NEG = 5, 20              # the input channels that carry +inf and -inf
H1_POS, H1_NEG = 9, 22              # the one hidden channel each of them turns into +inf
H2_POS, H2_NEG = (3, 17), (11, 30)  # the two channels of h2 that H1_POS / H1_NEG turn into +inf


@functools.lru_cache(maxsize=None)
def nonfinite_head(J, seed):
    """The integer family with four weight columns free of zeros, so that an infinite input does
    not turn its whole voxel into NaN on the way: +inf in channel IN_POS (-inf in IN_NEG) leaves
    h1 = +inf in channel H1_POS (H1_NEG) and 0 elsewhere, that leaves h2 = +inf in two channels,
    and the dense W3 — zeros included — makes NaN (0 * inf, inf - inf), +inf and -inf of them."""
    base = integer_head(J, seed)
    W = [w.clone() for w in base.W]
    g = torch.Generator().manual_seed(seed + 1)

    def column(l, col, positive_rows, sign_elsewhere):
        mag = torch.randint(1, 3, (C,), generator=g).double()
        eff = torch.full((C,), float(sign_elsewhere), dtype=torch.float64)
        eff[list(positive_rows)] = -float(sign_elsewhere)
        W[l][:, col] = eff * mag * torch.sign(base.scale[l])                 # sign(W * scale) = eff

    column(0, IN_POS, (H1_POS,), -1)        # +inf * W * scale: +inf in row H1_POS, -inf elsewhere
    column(0, IN_NEG, (H1_NEG,), +1)        # -inf * W * scale: the same for H1_NEG
    column(1, H1_POS, H2_POS, -1)
    column(1, H1_NEG, H2_NEG, -1)
    zero = torch.zeros(2, C, dtype=torch.float64)
    return make_head(W, base.scale, base.shift, base.b3, zero, zero, "integer")


HEADS["nonfinite"] = nonfinite_head


@functools.lru_cache(maxsize=None)
def nonfinite_case(vol):
    B, J = 2, 17
    S = vol[0] * vol[1] * vol[2]
    clean = make_case("integer", vol, B, J)
    head = nonfinite_head(J, clean.seed)
    nan, inf = float("nan"), float("inf")
    # (frame, channel, voxel, value): the first and the last voxel of a frame, the first block's last
    # chunk, and the second block's waves 0 and 1
    spots = ((0, 3, 0, nan), (0, IN_POS, S - 1, inf), (0, IN_NEG, 2047, -inf), (1, 30, 2048 + 5, nan),
             (1, IN_NEG, 2048 + 64 + 41, -inf), (1, IN_POS, 1000, inf))
    x = clean.x.clone()
    for b, ch, v, val in spots:
        x[b, ch, v] = val
    ref = reference(x.bfloat16().float(), head)
    return SimpleNamespace(kind="nonfinite", vol=vol, B=B, J=J, S=S, head=head, x=x, ref=ref, spots=spots,
                           seed=clean.seed)


@pytest.mark.parametrize("vol", ((13, 13, 13), (12, 12, 15)), ids=vid)
def test_nonfinite_reference_holds_nan_and_both_infinities(vol):
    """On the reference alone: a NaN voxel is NaN in every logit; an infinite voxel holds NaN and
    infinities side by side, both signs occurring; every other voxel is finite."""
    case = nonfinite_case(vol)
    ref = case.ref.f32
    special = torch.zeros(case.B, case.S, dtype=torch.bool)
    signs = set()
    for b, _, v, val in case.spots:
        special[b, v] = True
        at = ref[b, :, v]
        if val != val:
            assert bool(torch.isnan(at).all())
        else:
            assert bool(torch.isnan(at).any()) and bool(torch.isinf(at).any()) and not bool(torch.isfinite(at).any())
            signs |= set(torch.sign(at[torch.isinf(at)]).tolist())
    assert signs == {1.0, -1.0}
    assert torch.equal(~torch.isfinite(ref).any(dim=1), special)


@pytest.mark.gpu
@pytest.mark.parametrize("vol", ((13, 13, 13), (12, 12, 15)), ids=vid)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nonfinite_with_zero_weights(device, layout, vol):
    """NaN, +inf and -inf voxels (the last voxel of a frame and the second block among them): the
    NaN, +inf and -inf masks are those of torch on the CPU with the same operands, and every other
    logit is bit-equal, f32 and bf16."""
    case = nonfinite_case(vol)
    params = device_params("nonfinite", case.J, case.seed, device)
    x_dev, cl, _ = as_layout(case.x, vol, layout, device)
    for dtype in DTYPES:
        got = run_head(x_dev, params, cl, dtype).cpu()
        want = case.ref.f32 if dtype == torch.float32 else case.ref.bf16
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.isposinf(got), torch.isposinf(want))
        assert torch.equal(torch.isneginf(got), torch.isneginf(want))
        keep = ~torch.isnan(want)
        assert np.array_equal(bits(got)[keep.numpy()], bits(want)[keep.numpy()])


# ----------------------------------------------------------------------------- GPU: one call
ONE_CALL = (((3, 5, 7), "dense", 1), ((3, 5, 7), "dense", 2), ((12, 12, 15), "dense", 2), ((5, 5, 5), "cuboids", 2))


@pytest.mark.gpu
@pytest.mark.parametrize("vol,kind,group_frames", ONE_CALL, ids=lambda p: vid(p) if isinstance(p, tuple) else str(p))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_call_ragged_and_multiblock(device, layout, vol, kind, group_frames):
    """v2v_head_softargmax == v2v_head then the soft-argmax, bit for bit, at S = 105 (per element,
    groups start misaligned), S = 2160 (two blocks per frame) and 5^3 with Cuboids; B = 3 in groups
    of 1 and 2 (a ragged last group); both modes; f32 volumes, bf16 volumes and none.  The logits
    that feed the soft-argmax are the reference's."""
    from mvn_rocm import op, v2v, volumetric
    B, J = 3, 17
    case = make_case("integer", vol, B, J)
    params = device_params(case.kind, case.J, case.seed, device)
    x_dev, cl, _ = as_layout(case.x, vol, layout, device)
    if kind == "cuboids":
        base = np.array([[10.0, -20.0, 900.0], [-150.0, 40.0, 1000.0], [60.0, 5.0, 1100.0]])
        coords = volumetric.build_cuboids(base, 2500.0, vol[0], theta=[0.0, 0.7, 2.1], device=device)
    else:
        coords = (torch.randn((B, *vol, 3), generator=torch.Generator().manual_seed(3)) * 500.0).to(device)
    with torch.no_grad():
        for softmax in (True, False):
            for vol_dtype in (torch.float32, torch.bfloat16, None):
                ld = torch.bfloat16 if vol_dtype == torch.bfloat16 else torch.float32
                logits = v2v.v2v_head(x_dev, *params, out_dtype=ld, channels_last=cl)
                assert_same_bits(logits.reshape(B, J, -1), case.ref.bf16 if ld == torch.bfloat16 else case.ref.f32)
                kp_ref, vol_ref = op.integrate_tensor_3d_with_coordinates(logits, coords, softmax, multiplier=2.0 ** -6,
                                                                          return_volumes=vol_dtype is not None)
                kp, out = v2v.v2v_head_softargmax(x_dev, *params, coords, softmax=softmax, multiplier=2.0 ** -6,
                                                  out_dtype=vol_dtype, return_volumes=vol_dtype is not None,
                                                  group_frames=group_frames, channels_last=cl)
                assert bool(torch.isfinite(kp_ref).all())
                assert_bits_equal(kp.cpu().numpy(), kp_ref.cpu().numpy())
                if vol_dtype is None:
                    assert out is None and vol_ref is None
                else:
                    assert out.dtype == vol_dtype and tuple(out.shape) == (B, J, *vol)
                    assert_same_bits(out, vol_ref)
