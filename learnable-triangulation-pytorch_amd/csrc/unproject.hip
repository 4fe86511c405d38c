// Fused volumetric unprojection for gfx950.
//
// Replaces mvn/utils/op.py:99-163 (unproject_heatmaps).  The reference runs a
// Python loop over batch x view (op.py:107,113) issuing ~10 ATen launches per
// (b, v): a K=4 sgemm projection (multiview.py:80-101), depth mask / divide
// (op.py:121-124), [-1,1] normalisation (op.py:127-130), F.grid_sample bilinear
// with zero padding (op.py:134), masking (op.py:138) and a view aggregation
// (op.py:147-161).  Here one kernel does all of it: each lane owns one voxel,
// computes the N view projections once, then walks the channels writing each
// channel plane of the output coalesced (64 consecutive voxels per wave).
//
// Numerics (parity mode, compiled with -ffp-contract=off):
//   projection  r = fma(1, P3, fma(z, P2, fma(y, P1, x*P0)))   (MKL K=4 sgemm order)
//   sampling    fma(v_se,se, fma(v_sw,sw, fma(v_ne,ne, v_nw*nw)))  (ATen CPU grid sampler, §8a a1.5)
// so 'sum' / 'max' / 'conf' are bit-exact with the torch CPU reference and
// 'softmax' differs only by exp() rounding (<= 1e-6 rel).
#include "unproject_common.hpp"

namespace mvn {
namespace {

using namespace unproj;

constexpr int kUnprojBlock = 256;
constexpr int kMaxRegViews = 8;   // views whose geometry is held in registers

// ---- register-resident geometry, N <= 8 ----------------------------------
template <int AGG, typename TIn, typename TOut>
__global__ __launch_bounds__(kUnprojBlock) void unproject_regviews(
    const TIn* __restrict__ feat, const float* __restrict__ P, const float* __restrict__ coords,
    const float* __restrict__ conf, TOut* __restrict__ out, int N, int C, int H, int W, int nvox,
    int align_corners) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kUnprojBlock + threadIdx.x;
  if (i >= nvox) return;
  const float* cp = coords + (size_t(b) * nvox + i) * 3;
  const float x = cp[0], y = cp[1], z = cp[2];

  Taps t[kMaxRegViews];
#pragma unroll
  for (int v = 0; v < kMaxRegViews; ++v)
    if (v < N) t[v] = view_taps(P + (size_t(b) * N + v) * 12, x, y, z, H, W, align_corners);

  const size_t HW = size_t(H) * W;
  const TIn* fb = feat + size_t(b) * N * C * HW;
  TOut* ob = out + size_t(b) * C * nvox + i;
  for (int c = 0; c < C; ++c) {
    float s[kMaxRegViews];
#pragma unroll
    for (int v = 0; v < kMaxRegViews; ++v)
      if (v < N) s[v] = sample(fb + (size_t(v) * C + c) * HW, t[v]);

    const float* cf = AGG == MVN_AGG_CONF ? conf + size_t(b) * N * C + c : nullptr;
    store_elem(ob + size_t(c) * nvox, aggregate<AGG, kMaxRegViews>(s, N, cf, C));
  }
}

// ---- generic N (> 8): geometry recomputed per channel -------------------
template <int AGG, typename TIn, typename TOut>
__global__ __launch_bounds__(kUnprojBlock) void unproject_anyviews(
    const TIn* __restrict__ feat, const float* __restrict__ P, const float* __restrict__ coords,
    const float* __restrict__ conf, TOut* __restrict__ out, int N, int C, int H, int W, int nvox,
    int align_corners) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kUnprojBlock + threadIdx.x;
  if (i >= nvox) return;
  const float* cp = coords + (size_t(b) * nvox + i) * 3;
  const float x = cp[0], y = cp[1], z = cp[2];
  const size_t HW = size_t(H) * W;
  const TIn* fb = feat + size_t(b) * N * C * HW;
  const float* Pb = P + size_t(b) * N * 12;
  TOut* ob = out + size_t(b) * C * nvox + i;
  for (int c = 0; c < C; ++c) {
    float r = 0.f, m = -INFINITY, den = 0.f, num = 0.f;
    for (int v = 0; v < N; ++v) {
      const Taps t = view_taps(Pb + v * 12, x, y, z, H, W, align_corners);
      const float s = sample(fb + (size_t(v) * C + c) * HW, t);
      if constexpr (AGG == MVN_AGG_SUM) {
        r = v == 0 ? s : r + s;
      } else if constexpr (AGG == MVN_AGG_MAX) {
        r = (v == 0 || max_takes(s, r)) ? s : r;
      } else if constexpr (AGG == MVN_AGG_CONF) {
        const float p = s * conf[(size_t(b) * N + v) * C + c];
        r = v == 0 ? p : r + p;
      } else {  // online softmax over views
        if (s > m) {
          const float k = __expf(m - s);
          den *= k;
          num *= k;
          m = s;
        }
        const float e = __expf(s - m);
        den += e;
        num = __builtin_fmaf(s, e, num);
      }
    }
    if constexpr (AGG == MVN_AGG_SOFTMAX) r = num / den;
    store_elem(ob + size_t(c) * nvox, r);
  }
}

// Kernel choice: the tiled LDS-staged kernel (unproject_tiled.hip) for N <= 8 views, the
// register-geometry kernel above when a test forces it (mvn_debug_set_unproject), and the
// any-N kernel for more than 8 views.
template <int AGG, typename TIn, typename TOut>
int launch_agg(const UnprojCall& c) {
  if (c.N <= kMaxRegViews && !unproject_force_simple()) return launch_tiled<AGG, TIn, TOut>(c);
  if (c.cub) return MVN_ERR_SHAPE;     // in-kernel coordinates: the tiled kernel only (N <= 8)
  if (c.out_cl) return MVN_ERR_ARG;    // channels-last output: the tiled kernel only (N <= 8)
  const int nvox = c.Vx * c.Vy * c.Vz;
  const dim3 grid((nvox + kUnprojBlock - 1) / kUnprojBlock, c.B);
  const auto kernel = c.N <= kMaxRegViews ? unproject_regviews<AGG, TIn, TOut> : unproject_anyviews<AGG, TIn, TOut>;
  kernel<<<grid, kUnprojBlock, 0, c.s>>>(static_cast<const TIn*>(c.feat), c.P, c.coords, c.conf,
                                         static_cast<TOut*>(c.out), c.N, c.C, c.H, c.W, nvox, c.align_corners);
  return launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

// Validation common to the public entry points, then the dtype and aggregation dispatch.
int unproject_entry(const void* feat, int feat_dtype, const float* proj, const float* coords, const float* cub,
                    int transfer, const float* conf, void* out, int out_dtype, int out_layout, int B, int N, int C,
                    int H, int W, int Vx, int Vy, int Vz, int agg, int align_corners, int precision,
                    void* stream) {
  if (!feat || !proj || !(coords || cub) || !out) return MVN_ERR_ARG;
  if (precision != MVN_PRECISION_EXACT && precision != MVN_PRECISION_FAST) return MVN_ERR_ARG;
  if (agg < MVN_AGG_SUM || agg > MVN_AGG_CONF) return MVN_ERR_ARG;
  if (agg == MVN_AGG_CONF && !conf) return MVN_ERR_ARG;
  if (align_corners != 0 && align_corners != 1) return MVN_ERR_ARG;
  if (transfer != 0 && transfer != 1) return MVN_ERR_ARG;
  if (out_layout != MVN_LAYOUT_NCDHW && out_layout != MVN_LAYOUT_NDHWC) return MVN_ERR_ARG;
  if (B <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Vx <= 0 || Vy <= 0 || Vz <= 0) return MVN_ERR_SHAPE;
  const long long nvox = (long long)Vx * Vy * Vz;
  if (nvox > (1LL << 30) || (long long)H * W > (1LL << 30) || B > 65535) return MVN_ERR_SHAPE;
  UnprojCall c;
  c.feat = feat; c.P = proj; c.coords = coords; c.cub = cub; c.transfer = transfer; c.conf = conf; c.out = out;
  c.B = B; c.N = N; c.C = C; c.H = H; c.W = W; c.Vx = Vx; c.Vy = Vy; c.Vz = Vz;
  c.align_corners = align_corners;
  c.out_cl = out_layout == MVN_LAYOUT_NDHWC;
  c.fast = precision == MVN_PRECISION_FAST;
  c.s = static_cast<hipStream_t>(stream);
  return with_dtypes<false>(feat_dtype, out_dtype, [&](auto tin, auto tout) {
    return with_agg(agg, [&](auto a) {
      return launch_agg<decltype(a)::value, typename decltype(tin)::type, typename decltype(tout)::type>(c);
    });
  });
}

}  // namespace
}  // namespace mvn

extern "C" int mvn_unproject_ex(const void* feat, int feat_dtype, const float* proj, const float* coords,
                                const float* conf, void* out, int out_dtype, int out_layout, int B, int N, int C,
                                int H, int W, int Vx, int Vy, int Vz, int agg, int align_corners, void* stream) {
  if (!coords) return MVN_ERR_ARG;
  return mvn::unproject_entry(feat, feat_dtype, proj, coords, nullptr, 0, conf, out, out_dtype, out_layout, B, N, C,
                              H, W, Vx, Vy, Vz, agg, align_corners, MVN_PRECISION_EXACT, stream);
}

extern "C" int mvn_unproject_cuboid(const void* feat, int feat_dtype, const float* proj, const float* cuboids,
                                    int transfer_cmu, const float* conf, void* out, int out_dtype, int out_layout,
                                    int B, int N, int C, int H, int W, int V, int agg, int align_corners,
                                    void* stream) {
  if (!cuboids) return MVN_ERR_ARG;
  if (N > mvn::kMaxRegViews) return MVN_ERR_SHAPE;
  return mvn::unproject_entry(feat, feat_dtype, proj, nullptr, cuboids, transfer_cmu, conf, out, out_dtype,
                              out_layout, B, N, C, H, W, V, V, V, agg, align_corners, MVN_PRECISION_EXACT, stream);
}

extern "C" int mvn_unproject_precision(const void* feat, int feat_dtype, const float* proj, const float* coords,
                                       const float* cuboids, int transfer_cmu, const float* conf, void* out,
                                       int out_dtype, int out_layout, int B, int N, int C, int H, int W, int Vx,
                                       int Vy, int Vz, int agg, int align_corners, int precision, void* stream) {
  if ((coords == nullptr) == (cuboids == nullptr)) return MVN_ERR_ARG;     // exactly one coordinate source
  if (cuboids && (N > mvn::kMaxRegViews || Vx != Vy || Vx != Vz)) return MVN_ERR_SHAPE;
  return mvn::unproject_entry(feat, feat_dtype, proj, coords, cuboids, cuboids ? transfer_cmu : 0, conf, out,
                              out_dtype, out_layout, B, N, C, H, W, Vx, Vy, Vz, agg, align_corners, precision, stream);
}

extern "C" int mvn_unproject(const void* feat, int feat_dtype, const float* proj, const float* coords,
                             const float* conf, void* out, int out_dtype, int B, int N, int C, int H,
                             int W, int Vx, int Vy, int Vz, int agg, int align_corners, void* stream) {
  return mvn_unproject_ex(feat, feat_dtype, proj, coords, conf, out, out_dtype, MVN_LAYOUT_NCDHW, B, N, C, H, W,
                          Vx, Vy, Vz, agg, align_corners, stream);
}
