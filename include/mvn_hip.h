/*
 * mvn_hip.h — C ABI of libmvn_hip.so, the MI355X (gfx950) implementation of the
 * volumetric / algebraic triangulation hot path of learnable-triangulation-pytorch.
 *
 * The reference has no FFI layer: its boundary is three module-level Python
 * functions that the models call by attribute lookup.  Each entry
 * point below replaces exactly one of them and is what a ctypes / torch custom-op
 * binding on the reference side would call:
 *
 *   mvn_unproject        <- mvn/utils/op.py:99-163   unproject_heatmaps(...)
 *   mvn_softargmax3d     <- mvn/utils/op.py:84-96    integrate_tensor_3d_with_coordinates(...)
 *   mvn_dlt              <- mvn/utils/multiview.py:162-174 triangulate_batch_of_points(...)
 *                           (+ its per-point solver multiview.py:132-159)
 *   mvn_softargmax2d     <- mvn/utils/op.py:11-47    integrate_tensor_2d(...)  (the algebraic
 *                           path's producer of the DLT's 2D points)
 *   mvn_coord_volumes    <- mvn/models/triangulation.py:280-341 (the per-frame coordinate-
 *                           volume loop feeding unproject and soft-argmax)
 *   mvn_unproject_cuboid, mvn_softargmax3d_cuboid
 *                        <- op.py:99-163 / op.py:84-96 fed by triangulation.py:280-341: the
 *                           coordinate volume formed in-kernel from the per-frame cuboid
 *   mvn_nearest_voxel    <- mvn/models/loss.py:63-67 (VolumetricCELoss's distance volume +
 *                           argmin)
 *   mvn_v2v_front        <- mvn/models/v2v.py:7-17, 145-146 (V2VModel.front_layers[0] =
 *                           Basic3DBlock(32, 16, 7), eval mode; BASELINE config 5)
 *   mvn_v2v_head         <- mvn/models/v2v.py:154-160 (back_layers[1], back_layers[2] and
 *                           output_layer: the pointwise tail, eval mode), and with the 3D
 *                           soft-argmax behind it mvn_v2v_head_softargmax
 *   mvn_v2v_conv3, mvn_v2v_res3d
 *                        <- mvn/models/v2v.py:20-42 (Res3DBlock at the full resolution:
 *                           front_layers[1..3], skip_res1, back_layers[0]; eval mode)
 *   mvn_v2v_maxpool2, mvn_v2v_conv3_wide, mvn_v2v_upsample2
 *                        <- mvn/models/v2v.py:45-65, 105-135 (the encoder-decoder's first pooled
 *                           level: encoder_pool1, encoder_res1, skip_res2, decoder_res1 and
 *                           decoder_upsample1 with the last `+ skip_x1`; eval mode)
 *   mvn_v2v_conv3_deep, mvn_v2v_upsample2_deep
 *                        <- mvn/models/v2v.py:20-42, 53-65, 108-132 (the 128-channel levels below:
 *                           encoder_res2 ... decoder_upsample2 with their `+ skip`s; eval mode)
 *   mvn_triangulate_ransac <-mvn/models/triangulation.py:54-128 (the RANSAC baseline's host
 *                           loop: hypotheses, inlier DLT, Huber refinement)
 *   mvn_reprojection_error <- mvn/utils/multiview.py:177-184 calc_reprojection_error_matrix(...)
 *   mvn_algebraic_triangulate <- mvn/models/triangulation.py:164-191 (AlgebraicTriangulationNet's
 *                           forward after the backbone: mvn_softargmax2d, the confidence
 *                           normalisation, the upscale and mvn_dlt in one launch)
 *   mvn_feature_conv       <- mvn/models/triangulation.py:238-240, :345 process_features,
 *                           Conv2d(256, 32, 1)
 *   mvn_deconv4s2          <- mvn/models/pose_resnet.py:266-291 (one ConvTranspose2d(k = 4, stride 2)
 *                           + BatchNorm2d + ReLU of the backbone's deconv head; eval mode)
 *   mvn_deconv4s2_project  <- the head's last layer (as mvn_deconv4s2) and process_features,
 *                           mvn/models/triangulation.py:238-240, :345, in one launch
 *   mvn_conv1x1, mvn_conv3x3 <- mvn/models/pose_resnet.py:57-95 (the Bottleneck of the ResNet trunk's
 *                           layer1 .. layer4: its three convolutions with their BatchNorms, the
 *                           residual with its downsample, and the ReLUs; eval mode)
 *   mvn_stem               <- mvn/models/pose_resnet.py:205-209, 294-297 (conv1 + bn1 + relu + maxpool
 *                           of the ResNet; eval mode)
 *   mvn_conv3x3_pool, mvn_confidence_tail <- mvn/models/pose_resnet.py:140-174 (GlobalAveragePoolingHead:
 *                           a 3x3 convolution + BatchNorm2d + MaxPool2d(2) + ReLU stage, and the mean
 *                           with the three Linear layers and the Sigmoid; eval mode)
 *
 * Conventions
 *   - Every buffer is caller-owned device memory (hipMalloc / torch), contiguous,
 *     row-major in the reference's own tensor layout.  Nothing is retained after
 *     return; nothing is allocated (soft-argmax takes a caller workspace).
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Every call
 *     is stream-ordered and asynchronous: no host synchronisation, capturable in a
 *     hipGraph.
 *   - Return value: MVN_OK (0) or a negative MVN_ERR_* code.  Argument checks run
 *     before any HIP call, so they are safe without a GPU.
 *   - Functions are reentrant; the library keeps no mutable global state apart from
 *     the test-only knobs of mvn_debug_set_unproject (atomics).
 */
#ifndef MVN_HIP_H
#define MVN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------- */
#define MVN_OK              0
#define MVN_ERR_ARG        -1   /* null pointer / bad enum / bad flag            */
#define MVN_ERR_SHAPE      -2   /* non-positive or overflowing extent            */
#define MVN_ERR_DTYPE      -3   /* unsupported dtype combination                 */
#define MVN_ERR_LAUNCH     -4   /* hipLaunchKernel / hipGetLastError failed      */
#define MVN_ERR_WORKSPACE  -5   /* workspace missing or too small                */

/* ---- dtypes ------------------------------------------------------------ */
#define MVN_DTYPE_F32   0
#define MVN_DTYPE_BF16  1

/* ---- volume layouts ------------------------------------------------------ */
#define MVN_LAYOUT_NCDHW 0     /* (B, C, Vx, Vy, Vz): the reference's unproject output */
#define MVN_LAYOUT_NDHWC 1     /* (B, Vx, Vy, Vz, C): channels-last (V2V front input)  */

/* ---- unprojection arithmetic -------------------------------------------- */
#define MVN_PRECISION_EXACT 0  /* the reference's f32 op order: sum / max / conf* bit-exact,
                                  softmax <= 1e-5 (the default of every other entry point)  */
#define MVN_PRECISION_FAST  1  /* joints within north_star's 1e-4, the volume within the
                                  project's own bars (below): reciprocal
                                  projection, max-free view softmax, and for bf16 maps bf16
                                  bilinear weights on v_dot2 pixel pairs                    */

/* ---- view aggregation (op.py:147-161) ---------------------------------- */
#define MVN_AGG_SUM      0     /* 'sum'                                           */
#define MVN_AGG_MAX      1     /* 'max'                                           */
#define MVN_AGG_SOFTMAX  2     /* 'softmax'                                       */
#define MVN_AGG_CONF     3     /* any string starting with 'conf' (op.py:147)     */

/* Library version, (major << 16) | (minor << 8) | patch. */
int mvn_version(void);

/* Static message for an MVN_* return code. */
const char* mvn_strerror(int code);

/*
 * Unprojection of N views of C-channel maps into a C x Vx x Vy x Vz volume.
 * Replaces mvn/utils/op.py:99-163 (unproject_heatmaps).
 *
 *   feat    (B, N, C, H, W)     feat_dtype (f32 | bf16)
 *   proj    (B, N, 3, 4)        f32, heatmap-resolution projection matrices
 *   coords  (B, Vx, Vy, Vz, 3)  f32 world coordinates per voxel
 *   conf    (B, N, C)           f32, read only when agg == MVN_AGG_CONF (else may be NULL)
 *   out     (B, C, Vx, Vy, Vz)  out_dtype (f32 | bf16)
 *   align_corners: 0 = torch>=1.3 grid_sample default (the importable oracle),
 *                  1 = torch 1.0.1 semantics (requirements.txt:20 pins 1.0.1).
 */
int mvn_unproject(const void* feat, int feat_dtype,
                  const float* proj, const float* coords, const float* conf,
                  void* out, int out_dtype,
                  int B, int N, int C, int H, int W, int Vx, int Vy, int Vz,
                  int agg, int align_corners, void* stream);

/*
 * 3D soft-argmax over voxel world coordinates.
 * Replaces mvn/utils/op.py:84-96 (integrate_tensor_3d_with_coordinates), with the
 * caller's `volumes * volume_multiplier` (triangulation.py:353) fused as `multiplier`.
 *
 *   vol       element (b, j, i) at vol[b*vol_bstride + j*vol_jstride + i], i < Vx*Vy*Vz
 *             (strides in elements, so a channel slice of an unprojected volume
 *             needs no copy); vol_dtype f32 | bf16
 *   coords    (B, Vx, Vy, Vz, 3) f32
 *   out_xyz   (B, J, 3) f32
 *   out_vol   (B, J, Vx, Vy, Vz) contiguous, out_dtype f32 | bf16; NULL = do not
 *             write the normalised volume
 *   softmax   1 = softmax over the flattened volume (op.py:89),
 *             0 = relu with no mass normalisation (op.py:91, reference quirk)
 *   NaN       follows torch in both modes.  softmax: a joint holding a NaN (or +inf) voxel is
 *             NaN in coordinates and volume.  relu keeps a NaN as F.relu does (relu(NaN) = NaN,
 *             not 0): the voxel is NaN in out_vol and the joint's coordinates are NaN; a +inf
 *             voxel stays +inf.  Other joints are untouched.  mvn_softargmax3d_backward masks
 *             like torch's relu backward (x <= 0), so a NaN voxel receives its gradient.
 *   workspace >= mvn_softargmax3d_workspace_bytes(B, J, Vx, Vy, Vz) bytes of
 *             device memory, 16-byte aligned; contents need no initialisation.
 */
size_t mvn_softargmax3d_workspace_bytes(int B, int J, int Vx, int Vy, int Vz);

int mvn_softargmax3d(const void* vol, int vol_dtype,
                     int64_t vol_bstride, int64_t vol_jstride,
                     const float* coords, float multiplier, int softmax,
                     float* out_xyz, void* out_vol, int out_dtype,
                     void* workspace, size_t workspace_bytes,
                     int B, int J, int Vx, int Vy, int Vz, void* stream);

/*
 * Confidence-weighted linear (DLT) triangulation of a batch of points.
 * Replaces mvn/utils/multiview.py:162-174 (triangulate_batch_of_points) and its
 * per-point solver multiview.py:132-159.  The 2N x 4 design matrix is formed in
 * f32 exactly as the reference forms it (multiview.py:150-152); its null vector is
 * found in f64 (streaming Givens QR + one-sided Jacobi SVD).
 *
 *   proj  (B, N, 3, 4) f32     image-resolution projection matrices
 *   pts   (B, N, J, 2) f32     2D points, pixels
 *   conf  (B, N, J)    f32     per-view confidences; NULL = all ones (multiview.py:147-148)
 *   out   (B, J, 3)    f32
 */
int mvn_dlt(const float* proj, const float* pts, const float* conf, float* out,
            int B, int N, int J, void* stream);

/*
 * mvn_unproject with a selectable output layout: out_layout = MVN_LAYOUT_NCDHW is exactly
 * mvn_unproject; MVN_LAYOUT_NDHWC writes (B, Vx, Vy, Vz, C) (C % 4 == 0, N <= 8), the
 * input layout of mvn_v2v_front.
 */
int mvn_unproject_ex(const void* feat, int feat_dtype,
                     const float* proj, const float* coords, const float* conf,
                     void* out, int out_dtype, int out_layout,
                     int B, int N, int C, int H, int W, int Vx, int Vy, int Vz,
                     int agg, int align_corners, void* stream);

/*
 * mvn_unproject / mvn_unproject_ex / mvn_unproject_cuboid with a selectable arithmetic
 * (op.py:99-163).  Exactly one of coords (B, Vx, Vy, Vz, 3) and cuboids (B, 18; then
 * Vx = Vy = Vz, N <= 8) is non-NULL.  precision = MVN_PRECISION_EXACT is bit-identical
 * to those entry points; MVN_PRECISION_FAST computes the same function with the 3D joints
 * within north_star's 1e-4 (the only bound north_star sets) and the volume within bars the
 * project sets itself (f32 maps: <= 1e-4 max-rel of the volume, measured 2-4e-5; bf16 maps: one
 * bf16 ulp + 2^-8 max|ref|, 2^-7 for softmax; validity masks unchanged), measured in DESIGN.md §4.1a.
 */
int mvn_unproject_precision(const void* feat, int feat_dtype,
                            const float* proj, const float* coords, const float* cuboids, int transfer_cmu,
                            const float* conf, void* out, int out_dtype, int out_layout,
                            int B, int N, int C, int H, int W, int Vx, int Vy, int Vz,
                            int agg, int align_corners, int precision, void* stream);

/*
 * V2V front block, eval mode: Conv3d(32 -> 16, k = 7, pad = 3) + BatchNorm3d + ReLU
 * (v2v.py:7-17) on bf16 MFMA, f32 accumulation.
 *   vol_cl         (B, V, V, V, 32) bf16 channels-last (mvn_unproject_ex NDHWC output)
 *   weight_packed  mvn_v2v_front_packed_weight_bytes() bytes: bf16 weights as
 *                  [tap = (dx*7 + dy)*7 + dz][lane 0..63][j 0..7] = W[lane & 15][8*(lane >> 4) + j][dx][dy][dz]
 *   scale, shift   (16) f32: BN folded, y = relu(conv * scale + shift)
 *   out            (B, 16, V, V, V) out_dtype (f32 | bf16);  V % 16 == 0, V <= 256
 * NaN follows torch: relu keeps a NaN (F.relu(NaN) = NaN, not 0), so a NaN or infinite input
 * voxel reaches exactly its 7^3 neighbourhood (clipped at the volume border) in all 16 output
 * channels, as F.relu(bn(conv(x))) does: NaN there for a NaN voxel; for an infinite one
 * +inf or 0 by the sign of weight * scale (NaN where 0 * inf or inf - inf meet), and no other
 * voxel or frame changes.  Checked before any HIP call: a NULL pointer (MVN_ERR_ARG), B < 1 or
 * a V that is not a multiple of 16 in [16, 256] (MVN_ERR_SHAPE), another out_dtype
 * (MVN_ERR_DTYPE).
 */
size_t mvn_v2v_front_packed_weight_bytes(void);
int mvn_v2v_front(const void* vol_cl, const void* weight_packed, const float* scale, const float* shift,
                  void* out, int out_dtype, int B, int V, void* stream);

/*
 * Config 5 in one call: unprojection written channels-last bf16 (as mvn_unproject_ex with
 * MVN_LAYOUT_NDHWC, or mvn_unproject_cuboid when `cuboids` is given instead of `coords`)
 * followed by mvn_v2v_front, pipelined over groups of `group_frames` frames (<= 0: the
 * default, one group's intermediate within half of the 256 MiB MALL: 8 frames at V = 64)
 * through `workspace` (>= mvn_unproject_v2v_front_workspace_bytes(group_frames, V) bytes).
 * Replaces triangulation.py:349-352 up to V2VModel.front_layers[0] (v2v.py:145-146).
 *   C == 32, V % 16 == 0, 1 <= N <= 8 views (the channels-last kernels), B >= 1
 *   (MVN_ERR_SHAPE otherwise; mvn_rocm.v2v.unproject_v2v_front routes more views and empty
 *   batches through the two calls); exactly one of coords / cuboids non-NULL.
 *   out (B, 16, V, V, V) out_dtype.  Bit-identical to the two calls on the whole batch.
 * mvn_unproject_v2v_front takes agg != MVN_AGG_CONF; mvn_unproject_v2v_front_ex also takes
 * MVN_AGG_CONF with conf (B, N, C) f32 — the volumetric model's vol_confidences whenever
 * volume_aggregation_method starts with 'conf' (triangulation.py:268-269, 349; op.py:147-148)
 * — and ignores conf otherwise.
 */
size_t mvn_unproject_v2v_front_workspace_bytes(int group_frames, int V);
int mvn_unproject_v2v_front(const void* feat, int feat_dtype, const float* proj, const float* coords,
                            const float* cuboids, int transfer_cmu, int agg, int align_corners,
                            const void* weight_packed, const float* scale, const float* shift, void* out,
                            int out_dtype, void* workspace, size_t workspace_bytes, int group_frames,
                            int B, int N, int C, int H, int W, int V, void* stream);
int mvn_unproject_v2v_front_ex(const void* feat, int feat_dtype, const float* proj, const float* coords,
                               const float* cuboids, int transfer_cmu, int agg, const float* conf,
                               int align_corners, const void* weight_packed, const float* scale,
                               const float* shift, void* out, int out_dtype, void* workspace,
                               size_t workspace_bytes, int group_frames, int B, int N, int C, int H, int W,
                               int V, void* stream);

/*
 * V2V head, eval mode: the pointwise tail of V2VModel (v2v.py:154-160) in one kernel on bf16
 * MFMA with f32 accumulation.  Per voxel, with 32 -> 32 -> 32 -> J channels (1 <= J <= 32):
 *   h1 = relu(bn1(W1 x + b1))    back_layers[1] = Basic3DBlock(32, 32, 1)
 *   h2 = relu(bn2(W2 h1 + b2))   back_layers[2] = Basic3DBlock(32, 32, 1)
 *   y  = W3 h2 + b3              output_layer   = Conv3d(32, J, 1)
 * x is rounded to bf16 (nearest-even) when it arrives as f32; h = relu(acc * scale + shift) is
 * formed in f32 (one fma) and rounded to bf16 as the next layer's operand; y = acc + bias3 in
 * f32.  relu keeps a NaN (as F.relu): a NaN or infinite input voxel makes all J logits of that
 * voxel NaN or infinite, as torch does, and touches no other voxel.
 *   x              x_layout MVN_LAYOUT_NCDHW: (B, 32, Vx, Vy, Vz), x_dtype f32 | bf16;
 *                  MVN_LAYOUT_NDHWC: (B, Vx, Vy, Vz, 32), bf16 only
 *   weight_packed  mvn_v2v_head_packed_weight_bytes(J) = 3 * 2 * 64 * 8 * 2 bytes: bf16 weights as
 *                  [layer l 0..2][m 0..1][lane 0..63][j 0..7] = W_(l+1)[16 m + (lane & 15)][kslot_l(8 (lane >> 4) + j)]
 *                  with kslot_0(k) = k (the input channel) and, for l = 1, 2,
 *                  kslot_l(8 g + j) = 16 (j >> 2) + 4 g + (j & 3) (the hidden channel an MFMA
 *                  leaves in that lane); rows >= J of W_3 are zero
 *   scale_shift    [2 layers][scale 32 | shift 32] f32: BN and conv bias folded,
 *                  h = relu(conv * scale + shift)
 *   bias3          (J) f32
 *   out            (B, J, Vx, Vy, Vz) out_dtype (f32 | bf16): the logits, without the model's
 *                  volume_multiplier (mvn_softargmax3d fuses it)
 * The volume need not be cubic.  When Vx*Vy*Vz is no multiple of 4, or x or out is not 16-byte
 * aligned, loads and stores are per element (the same result).
 * MVN_ERR_ARG for a null pointer or an unknown layout; MVN_ERR_DTYPE for an unknown dtype or f32
 * with NDHWC; MVN_ERR_SHAPE for J outside 1..32, a non-positive extent or an overflowing element
 * count.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_v2v_head_packed_weight_bytes(int J);
int mvn_v2v_head(const void* x, int x_dtype, int x_layout, const void* weight_packed,
                 const float* scale_shift, const float* bias3, void* out, int out_dtype,
                 int B, int J, int Vx, int Vy, int Vz, void* stream);

/*
 * The end of the volumetric forward in one call: mvn_v2v_head into logits held in `workspace`,
 * then mvn_softargmax3d (coords) or mvn_softargmax3d_cuboid (cuboids; then Vx = Vy = Vz) on
 * them, over groups of `group_frames` frames (<= 0: the default, one group's f32 logits within
 * half of the 256 MiB MALL, at most 64: 7 frames at 64^3 with J = 17).  Replaces
 * triangulation.py:352-353 from back_layers[1] on.  Exactly one of coords (B, Vx, Vy, Vz, 3) and
 * cuboids (B, MVN_CUBOID_FLOATS) is non-NULL.
 *   multiplier, softmax, out_xyz (B, J, 3) f32, out_vol (B, J, Vx, Vy, Vz) out_dtype or NULL
 *   (not wanted): as mvn_softargmax3d.
 *   The logits are f32, except when a bf16 out_vol is wanted: the soft-argmax writes a bf16
 *   volume from bf16 logits only, so the logits are then bf16.  Bit-identical to mvn_v2v_head
 *   with those logits followed by the soft-argmax call, both on the whole batch.
 *   workspace >= mvn_v2v_head_softargmax_workspace_bytes(group_frames, J, Vx, Vy, Vz) bytes
 *   = G * J * Vx*Vy*Vz * 4 rounded up to 16, + mvn_softargmax3d_workspace_bytes(G, J, Vx, Vy, Vz),
 *   G the group size; 16-byte aligned, contents need no initialisation.
 * Errors as mvn_v2v_head, and MVN_ERR_ARG for both or neither of coords / cuboids or a flag
 * other than 0 / 1, MVN_ERR_SHAPE for a non-cubic volume with cuboids, MVN_ERR_WORKSPACE for a
 * missing or too small workspace.
 */
size_t mvn_v2v_head_softargmax_workspace_bytes(int group_frames, int J, int Vx, int Vy, int Vz);
int mvn_v2v_head_softargmax(const void* x, int x_dtype, int x_layout, const void* weight_packed,
                            const float* scale_shift, const float* bias3,
                            const float* coords, const float* cuboids, int transfer_cmu,
                            float multiplier, int softmax, float* out_xyz, void* out_vol, int out_dtype,
                            void* workspace, size_t workspace_bytes, int group_frames,
                            int B, int J, int Vx, int Vy, int Vz, void* stream);

/*
 * Full-resolution Res3DBlock convolution, eval mode (v2v.py:20-42): Conv3d(cin -> 32, k = 3,
 * stride 1, zero padding 1) + BatchNorm3d, an optional residual, ReLU, on bf16 MFMA with f32
 * accumulation, channels-last bf16 in and out.  Per output voxel and output channel co:
 *   acc = sum over the 27 taps and cin input channels of x * w   (bf16 operands, f32
 *         accumulation, summation order free; a tap outside the volume is zero and never
 *         reads the neighbouring frame)
 *   pre = fmaf(acc, scale[co], shift[co])
 *   r   = pre                                               skip_mode MVN_SKIP_NONE
 *       = pre + float(skip[voxel][co])                      MVN_SKIP_IDENTITY
 *       = pre + fmaf(acc_s, skip_scale[co], skip_shift[co]) MVN_SKIP_POINTWISE, acc_s the
 *         1x1x1 conv of skip[voxel][0..15] with skip_weight_packed (bf16 operands, f32)
 *   y   = bf16(r <= 0 ? +0 : r), nearest-even; a NaN r stays NaN (F.relu)
 * each fmaf and the add one f32 rounding.
 *   x              (B, V, V, V, cin) bf16, cin 16 | 32;  V % 16 == 0, 16 <= V <= 256
 *   weight_packed  mvn_v2v_conv3_packed_weight_bytes(cin) = 27 * 2 * 64 * 8 * 2 bytes (either
 *                  cin): bf16 weights as
 *                  [tap = (dx*3 + dy)*3 + dz][m 0..1][lane 0..63][j 0..7]
 *                    = W[16 m + (lane & 15)][8 (lane >> 4) + j][dx][dy][dz]
 *                  (W the Conv3d weight (32, cin, 3, 3, 3); tap (dx, dy, dz) multiplies input
 *                  voxel (x + dx - 1, y + dy - 1, z + dz - 1)); for cin = 16 the elements with
 *                  8 (lane >> 4) + j >= 16 are zero (K is zero-padded)
 *   scale, shift   (32) f32: BN and the conv bias folded
 *   skip           NONE: NULL.  IDENTITY: (B, V, V, V, 32) bf16, skip_cin 32.  POINTWISE:
 *                  (B, V, V, V, 16) bf16, skip_cin 16.  Must not overlap out.
 *   skip_weight_packed  POINTWISE only (NULL otherwise), mvn_v2v_conv3_skip_packed_weight_bytes(16)
 *                  = 2 * 64 * 8 * 2 bytes: [m 0..1][lane 0..63][j 0..7]
 *                    = Ws[16 m + (lane & 15)][8 (lane >> 4) + j], zero where 8 (lane >> 4) + j >= 16
 *   skip_scale, skip_shift  POINTWISE only (NULL otherwise): (32) f32
 *   out            (B, V, V, V, 32) bf16
 * A NaN or infinite input voxel reaches exactly its clipped 3^3 neighbourhood in all 32
 * channels, a non-finite skip voxel exactly its own voxel, as the stock modules' F.relu gives.
 * Checked before any HIP call: MVN_ERR_ARG for a null required pointer, an unknown skip_mode or
 * a skip / skip_weight_packed / skip_scale / skip_shift pointer that contradicts the mode
 * (given where the mode takes none, missing where it needs one); MVN_ERR_SHAPE for B < 1, a V
 * outside the multiples of 16 in [16, 256], a cin other than 16 / 32, a skip_cin other than 32
 * with IDENTITY or other than 16 with POINTWISE (ignored with NONE).  The size functions return
 * 0 for a cin they do not take.  Stream-ordered, allocates nothing, reentrant.
 */
#define MVN_SKIP_NONE      0
#define MVN_SKIP_IDENTITY  1
#define MVN_SKIP_POINTWISE 2
size_t mvn_v2v_conv3_packed_weight_bytes(int cin);
size_t mvn_v2v_conv3_skip_packed_weight_bytes(int cin);
int mvn_v2v_conv3(const void* x, int cin, const void* weight_packed, const float* scale, const float* shift,
                  int skip_mode, const void* skip, int skip_cin, const void* skip_weight_packed,
                  const float* skip_scale, const float* skip_shift, void* out, int B, int V, void* stream);

/*
 * A whole Res3DBlock in one call: mvn_v2v_conv3 (cin -> 32, skip NONE) into the hidden volume
 * held in `workspace`, then mvn_v2v_conv3 (32 -> 32) on it with the block's input x as the
 * skip, over groups of `group_frames` frames (<= 0: the default, one group's hidden volume
 * within half of the 256 MiB MALL, at most 64: 8 frames at V = 64).
 *   skip_mode      MVN_SKIP_IDENTITY (cin 32, the block's empty skip_con) or MVN_SKIP_POINTWISE
 *                  (cin 16, skip_con = Conv3d 1x1x1 + BatchNorm3d) with skip_weight_packed,
 *                  skip_scale, skip_shift as mvn_v2v_conv3's
 *   weight1_packed, scale1, shift1   the first conv (cin -> 32);  weight2_packed, scale2, shift2
 *                  the second (32 -> 32), packed as mvn_v2v_conv3's
 *   out            (B, V, V, V, 32) bf16; must not overlap x
 *   workspace      >= mvn_v2v_res3d_workspace_bytes(group_frames, V) = G * V^3 * 32 * 2 bytes, G the
 *                  group size (0 for a V the block does not take); 16-byte aligned, contents
 *                  need no initialisation
 * Bit-identical to the two launches on the whole batch.  Errors as mvn_v2v_conv3 (MVN_ERR_ARG
 * also for MVN_SKIP_NONE; MVN_ERR_SHAPE for IDENTITY with cin 16 or POINTWISE with cin 32), and
 * MVN_ERR_WORKSPACE for a missing or too small workspace.
 */
size_t mvn_v2v_res3d_workspace_bytes(int group_frames, int V);
int mvn_v2v_res3d(const void* x, int cin, const void* weight1_packed, const float* scale1, const float* shift1,
                  const void* weight2_packed, const float* scale2, const float* shift2, int skip_mode,
                  const void* skip_weight_packed, const float* skip_scale, const float* skip_shift, void* out,
                  void* workspace, size_t workspace_bytes, int group_frames, int B, int V, void* stream);

/*
 * F.max_pool3d(x, 2, 2) on a channels-last bf16 volume (Pool3DBlock(2), v2v.py:45-51), bit for
 * bit as torch computes it: per output voxel and channel the 8 window values are scanned in the
 * order x, y, z (z fastest) with m = -inf and the update `v > m || isnan(v)`: a NaN in the window
 * gives a NaN (the last one's bits), an all-negative window its largest value (never 0), a window
 * of -inf gives -inf, and among equal maxima (+0 and -0 included) the first in scan order wins.
 *   x    (B, V, V, V, C) bf16;  V even, 2 <= V <= 256;  C % 8 == 0, 8 <= C <= 128
 *   out  (B, V/2, V/2, V/2, C) bf16; must not overlap x
 * MVN_ERR_ARG for a null pointer; MVN_ERR_SHAPE for B < 1 or a V or C outside these sets.
 * Stream-ordered, allocates nothing, reentrant.
 */
int mvn_v2v_maxpool2(const void* x, void* out, int B, int V, int C, void* stream);

/*
 * mvn_v2v_conv3 with 64 output channels, for the Res3DBlocks of the first pooled level
 * (Res3DBlock(32, 64) and Res3DBlock(64, 64), v2v.py:20-42): Conv3d(cin -> 64, k = 3, stride 1,
 * zero padding 1) + BatchNorm3d, an optional residual, ReLU.  The arithmetic per output voxel and
 * channel is mvn_v2v_conv3's (acc, pre, r, y above), with
 *   x              (B, V, V, V, cin) bf16, cin 32 | 64;  V % 16 == 0, 16 <= V <= 128
 *   weight_packed  mvn_v2v_conv3_wide_packed_weight_bytes(cin) = 27 * (cin / 32) * 4 * 64 * 8 * 2
 *                  bytes: bf16 weights as
 *                  [tap = (dx*3 + dy)*3 + dz][kp 0..cin/32-1][m 0..3][lane 0..63][j 0..7]
 *                    = W[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]
 *                  (W the Conv3d weight (64, cin, 3, 3, 3); tap (dx, dy, dz) multiplies input
 *                  voxel (x + dx - 1, y + dy - 1, z + dz - 1))
 *   scale, shift   (64) f32: BN and the conv bias folded
 *   skip           NONE: NULL.  IDENTITY: (B, V, V, V, 64) bf16, skip_cin 64.  POINTWISE:
 *                  (B, V, V, V, 32) bf16, skip_cin 32.  Must not overlap out.
 *   skip_weight_packed  POINTWISE only (NULL otherwise),
 *                  mvn_v2v_conv3_wide_skip_packed_weight_bytes(32) = 4 * 64 * 8 * 2 bytes:
 *                  [m 0..3][lane 0..63][j 0..7] = Ws[16 m + (lane & 15)][8 (lane >> 4) + j]
 *                  (Ws the 1x1x1 Conv3d weight (64, 32))
 *   skip_scale, skip_shift  POINTWISE only (NULL otherwise): (64) f32
 *   out            (B, V, V, V, 64) bf16
 * A NaN or infinite input voxel reaches exactly its clipped 3^3 neighbourhood in all 64
 * channels, a non-finite skip voxel exactly its own voxel.  Errors as mvn_v2v_conv3:
 * MVN_ERR_ARG for a null required pointer, an unknown skip_mode or skip pointers that contradict
 * the mode; MVN_ERR_SHAPE for B < 1, a V outside the multiples of 16 in [16, 128], a cin other
 * than 32 / 64, a skip_cin other than 64 with IDENTITY or other than 32 with POINTWISE.  The size
 * functions return 0 for a cin they do not take.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_v2v_conv3_wide_packed_weight_bytes(int cin);
size_t mvn_v2v_conv3_wide_skip_packed_weight_bytes(int cin);
int mvn_v2v_conv3_wide(const void* x, int cin, const void* weight_packed, const float* scale, const float* shift,
                       int skip_mode, const void* skip, int skip_cin, const void* skip_weight_packed,
                       const float* skip_scale, const float* skip_shift, void* out, int B, int V, void* stream);

/*
 * Upsample3DBlock(64, 32, 2, 2), eval mode (v2v.py:53-65: ConvTranspose3d(64, 32, k = 2, stride 2)
 * + BatchNorm3d + ReLU), fused with the encoder-decoder's last `+ skip_x1` (v2v.py:133).  Per
 * input voxel (x, y, z), offset (dx, dy, dz) in {0, 1}^3 and output channel co:
 *   acc = sum over ci of in[x, y, z][ci] * W[ci][co][dx][dy][dz]   (bf16 operands, f32
 *         accumulation on MFMA, summation order free)
 *   pre = fmaf(acc, scale[co], shift[co])
 *   u   = pre <= 0 ? +0 : pre                                      (a NaN stays NaN)
 *   out[2x + dx, 2y + dy, 2z + dz][co] = bf16(u + float(skip[...][co])), nearest-even
 * (the ReLU before the add, none after it; without skip, bf16(u)).
 *   x              (B, V, V, V, 64) bf16;  V % 16 == 0, 16 <= V <= 128
 *   weight_packed  mvn_v2v_upsample2_packed_weight_bytes() = 2 * 16 * 64 * 8 * 2 bytes: bf16 as
 *                  [kp 0..1][m 0..15][lane 0..63][j 0..7]
 *                    = W[32 kp + 8 (lane >> 4) + j][16 (m & 1) + (lane & 15)][dx][dy][dz],
 *                  (dx*2 + dy)*2 + dz = m >> 1  (W the ConvTranspose3d weight (64, 32, 2, 2, 2))
 *   scale, shift   (32) f32: BN and the ConvTranspose bias folded
 *   skip           (B, 2V, 2V, 2V, 32) bf16, or NULL for no add; must not overlap out
 *   out            (B, 2V, 2V, 2V, 32) bf16
 * A non-finite input voxel reaches exactly its own 2x2x2 outputs (all channels), a non-finite
 * skip voxel exactly itself.  MVN_ERR_ARG for a null required pointer; MVN_ERR_SHAPE for B < 1 or
 * a V outside the multiples of 16 in [16, 128].  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_v2v_upsample2_packed_weight_bytes(void);
int mvn_v2v_upsample2(const void* x, const void* weight_packed, const float* scale, const float* shift,
                      const void* skip, void* out, int B, int V, void* stream);

/*
 * mvn_v2v_conv3 with 128 output channels, for the Res3DBlocks of the levels below the first pooled
 * one (Res3DBlock(64, 128) and Res3DBlock(128, 128), v2v.py:20-42): Conv3d(cin -> 128, k = 3,
 * stride 1, zero padding 1) + BatchNorm3d, an optional residual, ReLU.  The arithmetic per output
 * voxel and channel is mvn_v2v_conv3's (acc, pre, r, y above; the pointwise skip's acc_s is two
 * K = 32 MFMA passes over its 64 channels), with
 *   x              (B, D, D, D, cin) bf16, cin 64 | 128;  D any integer in [1, 64]
 *   weight_packed  mvn_v2v_conv3_deep_packed_weight_bytes(cin) = 27 * (cin / 32) * 8 * 64 * 8 * 2
 *                  bytes (442,368 | 884,736): bf16 weights as
 *                  [tap = (dx*3 + dy)*3 + dz][kp 0..cin/32-1][m 0..7][lane 0..63][j 0..7]
 *                    = W[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][dx][dy][dz]
 *                  (W the Conv3d weight (128, cin, 3, 3, 3); tap (dx, dy, dz) multiplies input
 *                  voxel (x + dx - 1, y + dy - 1, z + dz - 1); a tap outside the volume contributes
 *                  zero and never reads the neighbouring frame)
 *   scale, shift   (128) f32: BN and the conv bias folded
 *   skip           NONE: NULL.  IDENTITY: (B, D, D, D, 128) bf16, skip_cin 128.  POINTWISE:
 *                  (B, D, D, D, 64) bf16, skip_cin 64.  Must not overlap out.
 *   skip_weight_packed  POINTWISE only (NULL otherwise),
 *                  mvn_v2v_conv3_deep_skip_packed_weight_bytes(64) = 2 * 8 * 64 * 8 * 2 bytes:
 *                  [kp 0..1][m 0..7][lane 0..63][j 0..7] = Ws[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]
 *                  (Ws the 1x1x1 Conv3d weight (128, 64))
 *   skip_scale, skip_shift  POINTWISE only (NULL otherwise): (128) f32
 *   out            (B, D, D, D, 128) bf16
 * Volumes and packed weights are 16-byte aligned.  Deterministic: every output is one wave's sum
 * in a fixed order (no atomics), so two calls on the same data return the same bits.  A NaN or
 * infinite input voxel reaches exactly its 3^3 neighbourhood clipped to its own frame, in all 128
 * channels; a non-finite skip voxel exactly its own voxel.  Checked before any HIP call, argument
 * errors first: MVN_ERR_ARG for a null required pointer, an unknown skip_mode or skip pointers that
 * contradict the mode; MVN_ERR_SHAPE for B < 1, D outside [1, 64], a cin other than 64 / 128, a
 * skip_cin other than 128 with IDENTITY or other than 64 with POINTWISE, or B * D^3 above
 * INT_MAX / 8.  The size functions return 0 for a cin they do not take.  Stream-ordered, allocates
 * nothing, reentrant.
 */
size_t mvn_v2v_conv3_deep_packed_weight_bytes(int cin);
size_t mvn_v2v_conv3_deep_skip_packed_weight_bytes(int cin);
int mvn_v2v_conv3_deep(const void* x, int cin, const void* weight_packed, const float* scale, const float* shift,
                       int skip_mode, const void* skip, int skip_cin, const void* skip_weight_packed,
                       const float* skip_scale, const float* skip_shift, void* out, int B, int D, void* stream);

/*
 * Upsample3DBlock(128, cout, 2, 2), eval mode (v2v.py:53-65), fused with the `+ skip` behind it
 * (v2v.py:126-132): mvn_v2v_upsample2's arithmetic (acc over the 128 input channels in four K = 32
 * MFMA passes, pre, u, one rounding after the add) with
 *   x              (B, D, D, D, 128) bf16;  D any integer in [1, 64]
 *   cout           64 | 128
 *   weight_packed  mvn_v2v_upsample2_deep_packed_weight_bytes(cout) = 4 * 8 * (cout / 16) * 64 * 8 * 2
 *                  bytes: bf16 as [kp 0..3][m 0..8 cout/16 - 1][lane 0..63][j 0..7]
 *                    = W[32 kp + 8 (lane >> 4) + j][16 (m % (cout / 16)) + (lane & 15)][dx][dy][dz],
 *                  (dx*2 + dy)*2 + dz = m / (cout / 16)  (W the ConvTranspose3d weight
 *                  (128, cout, 2, 2, 2))
 *   scale, shift   (cout) f32: BN and the ConvTranspose bias folded
 *   skip           (B, 2D, 2D, 2D, cout) bf16, or NULL for no add; must not overlap out
 *   out            (B, 2D, 2D, 2D, cout) bf16
 * A non-finite input voxel reaches exactly its own 2x2x2 outputs (all channels), a non-finite skip
 * voxel exactly itself.  Deterministic.  MVN_ERR_ARG for a null required pointer; MVN_ERR_SHAPE
 * for B < 1, D outside [1, 64], another cout, or B * D^3 above INT_MAX / 8.  The size function
 * returns 0 for another cout.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_v2v_upsample2_deep_packed_weight_bytes(int cout);
int mvn_v2v_upsample2_deep(const void* x, int cout, const void* weight_packed, const float* scale,
                           const float* shift, const void* skip, void* out, int B, int D, void* stream);

/*
 * process_features of the volumetric model (triangulation.py:238-240, :345): Conv2d(cin, 32, 1) over
 * NCHW maps, on the f32-input MFMA (v_mfma_f32_32x32x2_f32).  No pack step:
 *   x       (n_images, cin, H, W)  x_dtype (f32 | bf16), contiguous
 *   weight  (32, cin)              f32 row-major, the convolution's own weight
 *   bias    (32)                   f32, or NULL for zeros
 *   out     (n_images, 32, H, W)   out_dtype (f32 | bf16), contiguous; all four dtype pairs
 * One arithmetic, defined bit for bit, for every dtype pair and both load paths:
 *   acc = bias[co];  for ci = 0 .. cin-1 in ascending order:  acc = fmaf(weight[co][ci], x[n][ci][p], acc)
 * An f32 out is acc, a bf16 out acc rounded to nearest-even; a bf16 x is widened to f32 (exact).
 * Non-finite values follow the chain: a NaN or infinite x[n][ci][p] reaches the 32 outputs of pixel
 * p of image n and no other.
 *   cout      must be 32
 *   cin       a multiple of 32 in [32, 512]
 *   H, W      any values >= 1; n_images * H * W == 0 returns MVN_OK without a launch
 *   4 GB      one image's maps, cin * H * W * sizeof(x element), must not exceed 2^31 - 1 bytes
 *             (in-image byte offsets are 32-bit, and every load goes through a range-checked buffer
 *             resource of one image); the whole batch may: the image base is 64-bit
 * Alignment: x and out need only the alignment of their element type, at any H * W.  The kernel
 * chooses per call from the actual pointers and H * W: where H * W % 4 == 0, x is aligned to four
 * of its elements (16 bytes f32, 8 bytes bf16) and out to four of its, it loads 16 (8) bytes and
 * stores 16 (8) bytes per lane; everywhere else it loads and stores single elements.  Both paths
 * return the same bits.  No load touches a byte outside x's n_images * cin * H * W elements and no
 * store a byte outside out's.
 * Checked before any HIP call: MVN_ERR_ARG for a NULL x, weight or out or an unknown dtype code;
 * MVN_ERR_SHAPE for another cout or cin, a negative extent, an image above the 2^31 - 1 bytes, or
 * n_images * ceil(H * W / 128) above INT_MAX / 2.  Stream-ordered, allocates nothing, reentrant.
 */
int mvn_feature_conv(const void* x, int x_dtype, const float* weight, const float* bias, void* out,
                     int out_dtype, int64_t n_images, int cin, int cout, int H, int W, void* stream);

/*
 * One layer of the 2-D backbone's deconv head (mvn/models/pose_resnet.py:266-291), eval mode:
 * ConvTranspose2d(cin, 256, k = 4, stride 2, padding 1, output_padding 0, bias folded) +
 * BatchNorm2d + ReLU on v_mfma_f32_16x16x32_bf16.  Per image n, output pixel
 * (oy, ox) of the 2H x 2W map and output channel co:
 *   acc = sum of x[n, iy, ix, ci] * W[ci][co][ky][kx] over ci and the (ky, kx) with
 *         oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx, 0 <= iy < H, 0 <= ix < W
 *         (products of bf16 operands, accumulated in f32 on the MFMA, summation order free)
 *   r   = fmaf(acc, scale[co], shift[co])
 *   y   = r <= 0 ? +0 : r                                          (a NaN stays NaN)
 *   out = y rounded once to out_dtype (bf16: nearest-even)
 * An even oy takes ky in {1, 3} (iy = oy / 2, oy / 2 - 1), an odd oy takes ky in {0, 2}
 * (iy = (oy + 1) / 2, (oy - 1) / 2), and the same along x: 2 x 2 taps in the interior, fewer on the
 * border, where a tap outside the image contributes zero and never reads the neighbouring image.
 *   x              (n_images, H, W, cin) bf16, channels-last
 *   cin            a multiple of 32 in [32, 2048]
 *   weight_packed  mvn_deconv4s2_packed_weight_bytes(cin) = 16 * (cin / 32) * 16 * 64 * 8 * 2 bytes:
 *                  bf16 as [tap = ky*4 + kx][kp 0..cin/32-1][m 0..15][lane 0..63][j 0..7]
 *                    = W[32 kp + 8 (lane >> 4) + j][16 m + (lane & 15)][ky][kx]
 *                  (W the ConvTranspose2d weight (cin, 256, 4, 4), rounded to bf16)
 *   scale, shift   (256) f32: BN and the deconv bias (if any) folded
 *   out_layout     MVN_LAYOUT_NHWC: out (n_images, 2H, 2W, 256), bf16 only (feeds the next layer);
 *                  MVN_LAYOUT_NCHW: out (n_images, 256, 2H, 2W), bf16 or f32
 *   H, W           >= 1, with H * W <= (2^31 - 1) / (2 cin) and <= (2^31 - 1) / 4096: one image of x
 *                  and one image of out (256 * 2H * 2W elements of up to 4 bytes) each stay below
 *                  2^31 bytes, the range of one buffer resource; the batch may be larger
 * x, weight_packed, scale, shift and out are 16-byte aligned.  The three outputs agree: the
 * channels-last result equals the NCHW bf16 result after a permute, and the NCHW f32 result
 * rounded to bf16 equals the NCHW bf16 result, bit for bit (the same MFMA sums in the same order,
 * one rounding).  Where W % 4 == 0 an NCHW lane stores 8 consecutive outputs of a row as 16-byte
 * words, elsewhere single elements, with the same bits.  Deterministic (no atomics).  A NaN or
 * infinite input pixel (iy, ix) reaches exactly the output rows 2 iy - 1 .. 2 iy + 2 and columns
 * 2 ix - 1 .. 2 ix + 2 of its own image, clipped, in all 256 channels.  No load touches a byte
 * outside x (range-checked buffer resource per image) and no store a byte outside out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer, an unknown layout or dtype (f32
 * with NHWC included), a cin outside the set, n_images < 0, H < 1 or W < 1, an image over the
 * limits above, more than INT_MAX blocks (n_images * ceil(H / 4) * ceil(W / 16) * 2), a pointer off
 * its alignment.  n_images == 0 returns MVN_OK without a launch.  The size function returns 0 for
 * a cin outside the set.  Stream-ordered, allocates nothing, reentrant.
 */
#define MVN_LAYOUT_NCHW 0      /* (M, C, H, W)                                      */
#define MVN_LAYOUT_NHWC 1      /* (M, H, W, C): channels-last                       */
size_t mvn_deconv4s2_packed_weight_bytes(int cin);
int mvn_deconv4s2(const void* x, const void* weight_packed, const float* scale, const float* shift, void* out,
                  int out_layout, int out_dtype, int64_t n_images, int cin, int H, int W, void* stream);

/*
 * The head's last layer with the volumetric model's process_features (or any Conv2d(256, 32, 1))
 * behind it in the same launch: mvn_deconv4s2 followed by a 256 -> 32 product
 * per output pixel, the 256-channel activation never stored to global memory.  x, weight_packed,
 * scale, shift, cin, H, W as for mvn_deconv4s2.  Per image n and output pixel (oy, ox):
 *   a[c]   = bf16(relu_keep_nan(fmaf(acc[c], scale[c], shift[c])))     c = 0 .. 255
 *            acc the same MFMA sums in the same order as mvn_deconv4s2's, so a is bit for bit what
 *            mvn_deconv4s2 writes with MVN_LAYOUT_NCHW / MVN_DTYPE_BF16
 *   out[p] = bias[p] + sum_c a[c] * hi[p][c] + sum_c a[c] * lo[p][c]   p = 0 .. 31
 *            hi = bf16(w), lo = bf16(w - hi) for the f32 projection weight w (32, 256), split once
 *            by the packer: hi + lo is within 2^-17 relative of w.  Products of bf16 operands
 *            (exact), accumulated in f32 on v_mfma_f32_16x16x32_bf16 in one fixed order: the
 *            accumulator starts at bias[p] and takes, for the 32-channel groups k = 0 .. 7 in
 *            ascending order, the MFMA of group k with hi and then the MFMA of group k with lo.
 *            No atomics: the same inputs give the same bits on every run and for every n_images.
 *   out    = that f32 value, or it rounded once to bf16 (nearest-even)
 *   proj_packed  mvn_deconv4s2_project_weight_bytes() = 2 * 8 * 2 * 64 * 8 * 2 = 32,768 bytes: bf16 as
 *                [part 0 = hi | 1 = lo][k 0..7][nt 0..1][lane 0..63][j 0..7]
 *                  = part(w[16 nt + (lane & 15)][32 k + 16 (j >> 2) + 4 (lane >> 4) + (j & 3)])
 *                (the K-slots of a group in the order in which a lane of the deconv's MFMA holds the
 *                channels of a pixel).  A projection with fewer than 32 rows is zero-padded.
 *   bias         (32) f32
 *   out          (n_images, 32, 2H, 2W) NCHW, out_dtype f32 or bf16
 * Where any a[c] of a pixel is NaN or infinite, that pixel's 32 outputs may each be NaN or
 * infinite, which one unspecified (inf * lo with lo = 0 is NaN); no other pixel is affected.  An
 * input pixel reaches the same clipped 4 x 4 box of outputs as in mvn_deconv4s2.  No load touches
 * a byte outside x and no store a byte outside out; where W % 4 == 0 a lane stores 8 consecutive
 * outputs of a row as 16-byte words, elsewhere single elements, with the same bits.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer (bias included), an unknown dtype,
 * a cin outside the set, n_images < 0, H < 1 or W < 1, an image over mvn_deconv4s2's limits, more
 * than INT_MAX / 2 blocks (n_images * ceil(H / 4) * ceil(W / 16)), a pointer off 16-byte alignment.
 * n_images == 0 returns MVN_OK without a launch.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_deconv4s2_project_weight_bytes(void);
int mvn_deconv4s2_project(const void* x, const void* weight_packed, const float* scale, const float* shift,
                          const void* proj_packed, const float* bias, void* out, int out_dtype, int64_t n_images,
                          int cin, int H, int W, void* stream);

/*
 * The 1x1 convolutions of the backbone's ResNet trunk (mvn/models/pose_resnet.py:57-95, Bottleneck:
 * conv1 + bn1 + relu, and conv3 + bn3 + the residual + relu), eval mode, on v_mfma_f32_16x16x32_bf16
 * (DESIGN.md §4.18).  Per image n, pixel (oy, ox) of the H x W map and output channel co:
 *   acc = sum over ci of x[n, oy, ox, ci] * w[co][ci]
 *         (products of bf16 operands, accumulated in f32 on the MFMA, summation order free)
 *   pre = fmaf(acc, scale[co], shift[co])
 *   r   = pre                                                    skip_mode MVN_SKIP_NONE
 *       = pre + float(skip[n, oy, ox, co])                       MVN_SKIP_IDENTITY
 *       = pre + fmaf(acc_s, skip_scale[co], skip_shift[co])      MVN_SKIP_POINTWISE, with
 *         acc_s = sum over cs of skip[n, s oy, s ox, cs] * w_s[co][cs], s = skip_stride: the block's
 *         downsample (Conv2d 1x1 with stride s + BatchNorm2d), fused
 *   y   = r <= 0 ? +0 : r                                        (a NaN stays NaN)
 *   out = y rounded once to bf16 (nearest-even)
 *   x              (n_images, H, W, cin) bf16, channels-last
 *   cin, cout, skip_cin   multiples of 64 in [64, 2048]
 *   weight_packed  mvn_conv1x1_packed_weight_bytes(cin, cout) = (cin / 32) * (cout / 16) * 64 * 8 * 2 bytes:
 *                  bf16 as [kp 0..cin/32-1][m 0..cout/16-1][lane 0..63][j 0..7]
 *                    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]
 *                  (w the Conv2d weight (cout, cin, 1, 1), rounded to bf16)
 *   scale, shift   (cout) f32: the BatchNorm folded
 *   skip           NULL (NONE); (n_images, H, W, cout) bf16 (IDENTITY); (n_images, skip_H, skip_W,
 *                  skip_cin) bf16 (POINTWISE), where H = (skip_H - 1) / skip_stride + 1 in integer
 *                  division and the same for W, skip_stride 1 or 2
 *   skip_weight_packed, skip_scale, skip_shift   POINTWISE only (NULL otherwise): w_s packed as
 *                  weight_packed with skip_cin for cin, and the downsample's folded BatchNorm (cout)
 *   skip_cin, skip_H, skip_W, skip_stride   read with POINTWISE only
 *   out            (n_images, H, W, cout) bf16, channels-last
 * Every tensor stays below 2^31 bytes (one buffer resource each) and every pointer is 16-byte
 * aligned.  The order of the sums is the same for the same launch: deterministic, no atomics.  A
 * NaN or infinite x[n, oy, ox, .] reaches out[n, oy, ox, .] only, a non-finite skip pixel the one
 * output pixel that reads it.  No load touches a byte outside an operand (range-checked buffer
 * resources for x and the pointwise skip) and no store a byte outside out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null required pointer, an unknown skip_mode, skip
 * arguments that contradict the mode, a channel count outside the set, n_images < 0, H < 1 or W < 1,
 * a tensor of 2^31 bytes or more, with POINTWISE a stride other than 1 or 2 or a skip extent that
 * does not give H x W, a pointer off its alignment.  n_images == 0 returns MVN_OK without a launch.
 * The size function returns 0 for a channel count outside the set.  Stream-ordered, allocates
 * nothing, reentrant.
 */
size_t mvn_conv1x1_packed_weight_bytes(int cin, int cout);
int mvn_conv1x1(const void* x, const void* weight_packed, const float* scale, const float* shift, int skip_mode,
                const void* skip, const void* skip_weight_packed, const float* skip_scale, const float* skip_shift,
                int skip_cin, int skip_H, int skip_W, int skip_stride, void* out, int64_t n_images, int H, int W,
                int cin, int cout, void* stream);

/*
 * The 3x3 convolution of the trunk's Bottleneck (conv2 + bn2 + relu; padding 1, stride 1 or 2, as
 * many outputs as inputs), eval mode, on v_mfma_f32_16x16x32_bf16.  The output is
 * (n_images, Ho, Wo, channels) with Ho = (H - 1) / stride + 1 and Wo = (W - 1) / stride + 1 in integer
 * division.  Per image n, output pixel (oy, ox) and output channel co:
 *   acc = sum over ci and the taps (ky, kx) in 0..2 with iy = stride oy - 1 + ky in [0, H) and
 *         ix = stride ox - 1 + kx in [0, W) of x[n, iy, ix, ci] * w[co][ci][ky][kx]
 *         (a tap outside the image contributes zero and never reads the neighbouring image;
 *         products of bf16 operands, accumulated in f32 on the MFMA, summation order free)
 *   y   = relu_keep_nan(fmaf(acc, scale[co], shift[co])), rounded once to bf16
 *   x              (n_images, H, W, channels) bf16, channels-last
 *   channels       a multiple of 64 in [64, 512]
 *   weight_packed  mvn_conv3x3_packed_weight_bytes(channels) = 9 * (channels / 32) * (channels / 16) * 64 * 8 * 2
 *                  bytes: bf16 as [tap = ky*3 + kx][kp 0..channels/32-1][m 0..channels/16-1][lane 0..63][j 0..7]
 *                    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]
 *                  (w the Conv2d weight (channels, channels, 3, 3), rounded to bf16)
 *   scale, shift   (channels) f32: the BatchNorm folded
 * x and out stay below 2^31 bytes and every pointer is 16-byte aligned.  Deterministic.  A NaN or
 * infinite input pixel (iy, ix) reaches exactly the output pixels (oy, ox) with |stride oy - iy| <= 1
 * and |stride ox - ix| <= 1 of its own image, in all channels.  No load touches a byte outside x and
 * no store a byte outside out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer, channels outside the set, a stride
 * other than 1 or 2, n_images < 0, H < 1 or W < 1, a tensor of 2^31 bytes or more, a pointer off its
 * alignment.  n_images == 0 returns MVN_OK without a launch.  The size function returns 0 for
 * channels outside the set.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_conv3x3_packed_weight_bytes(int channels);
int mvn_conv3x3(const void* x, const void* weight_packed, const float* scale, const float* shift, void* out,
                int64_t n_images, int H, int W, int channels, int stride, void* stream);

/*
 * The stem of the backbone's ResNet (mvn/models/pose_resnet.py:205-209, 294-297): Conv2d(3, 64, 7,
 * stride 2, padding 3) + BatchNorm2d + ReLU + MaxPool2d(3, stride 2, padding 1), eval mode, in one
 * launch on v_mfma_f32_16x16x32_bf16.  With Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1
 * in integer division and the same for W, per image n and channel co:
 *   c[n, co, cy, cx] = sum over ci in 0..2 and the taps (ky, kx) in 0..6 with iy = 2 cy - 3 + ky in [0, H)
 *         and ix = 2 cx - 3 + kx in [0, W) of bf16(images[n, ci, iy, ix]) * w[co][ci][ky][kx]
 *         (a tap outside the image contributes zero and never reads the neighbouring plane or image;
 *         products of bf16 operands, accumulated in f32 on the MFMA, summation order free)
 *   a   = relu_keep_nan(fmaf(c, scale[co], shift[co]))           f32; r <= 0 ? +0 : r, a NaN stays NaN
 *   p[n, py, px, co] = the maximum of a over cy in {2 py - 1, 2 py, 2 py + 1} within [0, Hc) and cx likewise
 *         within [0, Wc), with torch's update `v > m || isnan(v)`: a NaN in the window gives a NaN
 *   out = p rounded once to bf16 (nearest-even).  The kernel rounds a BEFORE the maximum (its map of a
 *         is held as bf16); rounding is monotone, so these are the bits of rounding behind the maximum.
 *   images         (n_images, 3, H, W) in_dtype (MVN_DTYPE_F32 | MVN_DTYPE_BF16), contiguous NCHW; an
 *                  f32 image is rounded once to bf16 in the kernel (nearest-even, NaN and +-inf kept)
 *   weight_packed  mvn_stem_packed_weight_bytes() = 6 * 4 * 64 * 8 * 2 = 24576 bytes: bf16 as
 *                  [kp 0..5][m 0..3][lane 0..63][j 0..7] = A[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j]
 *                  with A (64, 192): A[co][24 ky + 3 kx + ci] = w[co][ci][ky][kx] for ky, kx in 0..6 and
 *                  ci in 0..2 (w the Conv2d weight (64, 3, 7, 7), rounded to bf16), and zero in every
 *                  other slot: 24 ky + 21 .. 24 ky + 23 of each tap row and 168 .. 191.  The kernel
 *                  clears the pixel operand of those slots as well: they carry nothing, whatever the
 *                  weights there and the pixels beside the footprint hold.
 *   scale, shift   (64) f32: the BatchNorm (and a convolution bias) folded
 *   out            (n_images, Hp, Wp, 64) bf16, channels-last
 * images and out stay below 2^31 bytes.  weight_packed, scale, shift and out are 16-byte aligned; images
 * needs the alignment of its element only.  Deterministic: the order of the sums is fixed, no atomics.
 * A NaN or infinite input pixel (iy, ix) reaches exactly the outputs (py, px) with a cy in {2 py - 1 ..
 * 2 py + 1} within [0, Hc) with |2 cy - iy| <= 3, and likewise in x, of its own image, in all channels
 * (an infinity against a zero weight is a NaN, as in torch); a -inf or any value the ReLU removes does
 * not survive the pool.  No load touches a byte outside an operand (one range-checked buffer
 * resource over images) and no store a byte outside out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer, an unknown in_dtype, n_images < 0, H < 1
 * or W < 1, a tensor of 2^31 bytes or more, a pointer off its alignment.  n_images == 0 returns MVN_OK
 * without a launch.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_stem_packed_weight_bytes(void);
int mvn_stem(const void* images, int in_dtype, const void* weight_packed, const float* scale, const float* shift,
             void* out, int64_t n_images, int H, int W, void* stream);

/*
 * One convolution stage of the backbone's confidence heads (mvn/models/pose_resnet.py:144-153,
 * GlobalAveragePoolingHead.features): Conv2d(cin, cout, 3, padding 1) with bias + BatchNorm2d +
 * MaxPool2d(2) + ReLU, eval mode, in one launch on v_mfma_f32_16x16x32_bf16.  With
 * Hp = H / 2 and Wp = W / 2 in integer division (the pool floors: an odd trailing row or column of conv
 * pixels belongs to no window and is not computed, though the windows beside it read it as a tap), per
 * image n, window (py, px) and output channel co:
 *   acc_q = for each of the four conv pixels q = (2 py + dy, 2 px + dx), dy, dx in 0..1: the sum over ci
 *         and the taps (ky, kx) in 0..2 with iy = 2 py + dy - 1 + ky in [0, H) and ix = 2 px + dx - 1 + kx
 *         in [0, W) of x[n, iy, ix, ci] * w[co][ci][ky][kx]
 *         (a tap outside the image contributes zero and never reads the neighbouring image; products
 *         of bf16 operands, accumulated in f32 on the MFMA)
 *   r_q = fmaf(acc_q, scale[co], shift[co])      (scale may be negative: the fold comes before the maximum)
 *   m   = the maximum of the four r_q with torch's update `r > m || isnan(r)`: a NaN among them gives NaN
 *   y   = m <= 0 ? +0 : m                        (a NaN stays NaN)
 *   out = y, rounded once to bf16 (nearest-even) for a bf16 output
 *   x              (n_images, H, W, cin) bf16, channels-last; H, W >= 2
 *   cin            a multiple of 64 in [64, 2048];  cout a multiple of 64 in [64, 512]
 *   weight_packed  mvn_conv3x3_pool_packed_weight_bytes(cin, cout) = 9 * (cin / 32) * (cout / 16) * 64 * 8 * 2
 *                  bytes: bf16 as [tap = ky*3 + kx][kp 0..cin/32-1][m 0..cout/16-1][lane 0..63][j 0..7]
 *                    = w[16 m + (lane & 15)][32 kp + 8 (lane >> 4) + j][ky][kx]
 *                  (w the Conv2d weight (cout, cin, 3, 3), rounded to bf16)
 *   scale, shift   (cout) f32: the convolution's bias and the BatchNorm folded
 *   out            (n_images, Hp, Wp, cout) channels-last, out_dtype MVN_DTYPE_BF16 | MVN_DTYPE_F32; the two
 *                  agree bit for bit after rounding the f32 one
 * Order of the sum: the K-steps it = 0 .. 9 cin / 32 - 1 (tap-major: it = tap * cin / 32 + kp, each step the
 * MFMA's 32 channels) go to four accumulators a_s, a_s taking the steps [s per, (s + 1) per) within the range,
 * per = ceil(9 cin / 32 / 4) rounded up to even, each in ascending order; acc = ((a_0 + a_1) + a_2) + a_3 in
 * f32.  One fixed order for every launch: deterministic, no atomics.
 * x and out stay below 2^31 bytes and every pointer is 16-byte aligned.  A NaN or infinite input pixel
 * (iy, ix) reaches exactly the windows (py, px) with 2 py - 1 <= iy <= 2 py + 2 and 2 px - 1 <= ix <= 2 px + 2
 * of its own image, in all channels (an infinity against a zero weight is a NaN, as in torch; a -inf
 * or any value the ReLU removes does not survive it).  No load touches a byte outside an operand
 * (a range-checked buffer resource over x) and no store a byte outside out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer, a channel count outside its set, an
 * unknown out_dtype, n_images < 0, H < 2 or W < 2, a tensor of 2^31 bytes or more, a pointer
 * off its alignment.  n_images == 0 returns MVN_OK without a launch.  The size function returns 0 for
 * channels outside the sets.  Stream-ordered, allocates nothing, reentrant.
 */
size_t mvn_conv3x3_pool_packed_weight_bytes(int cin, int cout);
int mvn_conv3x3_pool(const void* x, const void* weight_packed, const float* scale, const float* shift, void* out,
                     int out_dtype, int64_t n_images, int H, int W, int cin, int cout, void* stream);

/*
 * The rest of a confidence head (pose_resnet.py:156-174): the mean over the pixels, Linear(c0, c1) +
 * ReLU + Linear(c1, c2) + ReLU + Linear(c2, n) and the Sigmoid, in one launch, all in f32 on the vector
 * ALU, one block per image.  Per image m:
 *   s[c]    = +0, then s[c] = s[c] + pooled[m, p, c] for the pixels p = 0 .. hw - 1 ascending
 *   x0[c]   = s[c] / float(hw)                                  (IEEE division)
 *   x1[o]   = relu_keep_nan(chain(W1, b1, x0)[o]),  x2[o] = relu_keep_nan(chain(W2, b2, x1)[o]),
 *   z[o]    = chain(W3, b3, x2)[o]
 *     with chain(W, b, v)[o]: acc = b[o], then acc = fmaf(W[o][i], v[i], acc) for i ascending
 *   out[m, o] = z[o]                           activation MVN_ACT_NONE (the logits)
 *             = 1.0f / (1.0f + expf(-z[o]))    MVN_ACT_SIGMOID: expf of the HIP device library (OCML's
 *               exp_f32, documented in the HIP math API reference with a maximum error of 1 ulp), one
 *               f32 add and one IEEE f32 division beside it
 *   pooled         (n_images, hw, c0) f32: the second mvn_conv3x3_pool's f32 output with its h x w pixels flat
 *   c0, c1, c2     multiples of 64 in [64, 512];  1 <= n <= 32;  hw >= 1
 *   params         mvn_confidence_tail_packed_bytes(c0, c1, c2, n) bytes of f32, each weight transposed
 *                  (in, out) so that the threads of consecutive outputs load consecutive words:
 *                    params[i * c1 + o]            = W1[o][i]      i < c0, o < c1
 *                    params[O1 + o]                = b1[o]         O1 = c0 c1
 *                    params[O2 + i * c2 + o]       = W2[o][i]      O2 = O1 + c1;  i < c1, o < c2
 *                    params[O3 + o]                = b2[o]         O3 = O2 + c1 c2
 *                    params[O4 + i * n + o]        = W3[o][i]      O4 = O3 + c2;  i < c2, o < n
 *                    params[O5 + o]                = b3[o]         O5 = O4 + c2 n
 *   out            (n_images, n) f32
 * pooled stays below 2^31 bytes.  Deterministic; an image's NaN or infinity stays in its own row of out.
 * Checked before any HIP call, all MVN_ERR_ARG: a null pointer, a width or n outside its set, an unknown
 * activation, n_images < 0, hw < 1, pooled of 2^31 bytes or more, a pointer off its 4-byte alignment.
 * n_images == 0 returns MVN_OK without a launch.  The size function returns 0 for widths outside the
 * sets.  Stream-ordered, allocates nothing, reentrant.
 */
#define MVN_ACT_NONE     0
#define MVN_ACT_SIGMOID  1
size_t mvn_confidence_tail_packed_bytes(int c0, int c1, int c2, int n);
int mvn_confidence_tail(const float* pooled, const float* params, float* out, int64_t n_images, int hw, int c0,
                        int c1, int c2, int n, int activation, void* stream);

/*
 * 2D soft-argmax of heatmaps.  Replaces mvn/utils/op.py:11-47 (integrate_tensor_2d) with
 * the caller's `heatmaps * heatmap_multiplier` (triangulation.py:164) fused.
 *   heatmaps  (B, J, H, W)  dtype (f32 | bf16), contiguous
 *   out_xy    (B, J, 2)     f32: (x, y) = sum p * (w, h) / sum p  (op.py:31-42)
 *   out_maps  (B, J, H, W)  out_dtype: softmax-normalised (softmax = 1) or relu'd maps
 *                           (softmax = 0, not normalised, op.py:27); NULL = not wanted
 * NaN follows torch in both modes: a map holding a NaN pixel has NaN (x, y); softmax makes the
 * whole returned map NaN, relu keeps the NaN at its pixel (F.relu(NaN) = NaN, not 0).  The same
 * holds for the maps and 2D points of mvn_algebraic_triangulate.
 */
int mvn_softargmax2d(const void* heatmaps, int dtype, float multiplier, int softmax, float* out_xy,
                     void* out_maps, int out_dtype, int B, int J, int H, int W, void* stream);

/*
 * Coordinate volumes (B, V, V, V, 3) f32 of the volumetric model, replacing the per-frame
 * loop of triangulation.py:280-341 (cuboid grid, rotation about the base point,
 * volumetric.py:87-114, optional CMU -> Human3.6M re-axing).  The caller forms per frame,
 * in float64 and rounded to f32 as torch does: position (B,3) = base - side/2,
 * centre (B,3) = base point, step (B,3) = side / (V-1), rot (B,3,3) the rotation matrix.
 */
int mvn_coord_volumes(const float* position, const float* centre, const float* step, const float* rot,
                      float* out, int B, int V, int transfer_cmu, void* stream);

/*
 * Unprojection and 3D soft-argmax with the coordinate volume formed in-kernel instead of
 * read: the caller of op.py:99 / op.py:84 in triangulation.py:280-353
 * builds coord_volumes from a per-frame cuboid and passes it straight to both ops; these
 * entry points take the cuboid itself and never materialise the (B, V, V, V, 3) volume
 * (12 B per voxel not read by either op).  Coordinates are bit-identical to
 * mvn_coord_volumes on the same cuboid, so results are bit-identical to mvn_unproject_ex /
 * mvn_softargmax3d fed that volume.
 *   cuboids  (B, MVN_CUBOID_FLOATS) f32 per frame: position[3], centre[3], step[3], rot[9]
 *            (the arguments of mvn_coord_volumes, interleaved per frame)
 *   transfer_cmu  0 | 1 as in mvn_coord_volumes;  grid V x V x V
 * mvn_unproject_cuboid needs N <= 8 (the tiled kernel); otherwise the arguments of
 * mvn_unproject_ex / mvn_softargmax3d.
 */
#define MVN_CUBOID_FLOATS 18
int mvn_unproject_cuboid(const void* feat, int feat_dtype,
                         const float* proj, const float* cuboids, int transfer_cmu, const float* conf,
                         void* out, int out_dtype, int out_layout,
                         int B, int N, int C, int H, int W, int V,
                         int agg, int align_corners, void* stream);
int mvn_softargmax3d_cuboid(const void* vol, int vol_dtype,
                            int64_t vol_bstride, int64_t vol_jstride,
                            const float* cuboids, int transfer_cmu, float multiplier, int softmax,
                            float* out_xyz, void* out_vol, int out_dtype,
                            void* workspace, size_t workspace_bytes,
                            int B, int J, int V, void* stream);

/*
 * Nearest voxel per (frame, joint): argmin over the V^3 voxels of the f32 distance
 * sqrt(((c - k)^2).sum(-1)) between coords[b] (B, Vx, Vy, Vz, 3) and keypoints (B, J, 3),
 * IEEE square root, first index on ties (torch.argmin).
 *   out_index (B, J) int32, flat row-major voxel index (VolumetricCELoss, loss.py:63-67).
 */
int mvn_nearest_voxel(const float* coords, const float* keypoints, int* out_index, int B, int J,
                      int Vx, int Vy, int Vz, void* stream);

/* ---- backward (autograd) ------------------------------------------------------------
 * Gradients of the three ops, replacing the ATen autograd the reference relies on
 * (grid_sampler_2d / softmax / einsum / svd backward).  Same buffer conventions as above.
 */

/*
 * d/d(feat) (and d/d(conf) for MVN_AGG_CONF) of mvn_unproject.
 *   grad_out   (B, C, Vx, Vy, Vz)  grad_out_dtype (f32 | bf16)
 *   grad_feat  (B, N, C, H, W) f32, ZERO-INITIALISED by the caller (accumulated with atomics)
 *   grad_conf  (B, N, C) f32 zero-initialised, or NULL (only read for MVN_AGG_CONF)
 * No gradient w.r.t. proj / coords (the reference builds both from numpy constants,
 * triangulation.py:272-341).  N <= 8.  Float atomics: last-bit order nondeterminism.
 */
int mvn_unproject_backward(const void* feat, int feat_dtype, const float* proj, const float* coords,
                           const float* conf, const void* grad_out, int grad_out_dtype,
                           float* grad_feat, float* grad_conf,
                           int B, int N, int C, int H, int W, int Vx, int Vy, int Vz,
                           int agg, int align_corners, void* stream);

/*
 * Deterministic variant of mvn_unproject_backward (the reference trains under
 * autograd.detect_anomaly, train.py:178) and mvn_rocm's default backward: every finite
 * contribution is scaled by a power of two 2^e and accumulated as a 64-bit integer (integer
 * adds are associative), then converted to f32 — two runs are bit-identical.  e is chosen per
 * (frame, channel) plane on the device from that plane's finite maxima of |grad_out| (and
 * |feat| for softmax, |conf| and |feat| for conf*) so that no sum of the plane can overflow.
 * Each contribution is rounded to a whole unit u = 2^-62 of the plane's bound
 * nvox * max|g| * factor before it is added, so an element fed by n contributions comes out
 * as the f32 rounding of an integer sum within n/2 units of its exact sum: absolute error
 * <= n/2 * u + half an f32 ulp (relative <= n * 2^-25 + 2^-24 once the element is above
 * 2^-38 of the bound, i.e. 2^24 units).  Non-finite contributions follow the reference's autograd element by element: a
 * NaN / inf grad_out, feature or confidence reaches exactly the gradient elements it reaches
 * in ATen's grid_sampler / softmax / mul backward (NaN if a NaN or both infinities meet there,
 * else the infinity); every other element stays finite.
 *   workspace  >= mvn_unproject_backward_workspace_bytes(B, N, C, H, W) bytes, any content
 *   grad_feat / grad_conf are fully written (no zero-initialisation needed).
 */
size_t mvn_unproject_backward_workspace_bytes(int B, int N, int C, int H, int W);
int mvn_unproject_backward_deterministic(const void* feat, int feat_dtype, const float* proj,
                                         const float* coords, const float* conf, const void* grad_out,
                                         int grad_out_dtype, float* grad_feat, float* grad_conf,
                                         void* workspace, size_t workspace_bytes,
                                         int B, int N, int C, int H, int W, int Vx, int Vy, int Vz,
                                         int agg, int align_corners, void* stream);

/*
 * d/d(vol) of mvn_softargmax3d (vol as passed to the forward, i.e. before `multiplier`).
 *   grad_xyz  (B, J, 3) f32 or NULL;  grad_vol (B, J, Vx, Vy, Vz) contiguous or NULL
 *   grad_in   (B, J, Vx, Vy, Vz) contiguous, dtype == vol_dtype, fully written
 *   workspace >= mvn_softargmax3d_backward_workspace_bytes(...) when softmax == 1
 */
size_t mvn_softargmax3d_backward_workspace_bytes(int B, int J, int Vx, int Vy, int Vz);

int mvn_softargmax3d_backward(const void* vol, int vol_dtype, int64_t vol_bstride, int64_t vol_jstride,
                              const float* coords, float multiplier, int softmax,
                              const float* grad_xyz, const void* grad_vol, int grad_vol_dtype,
                              void* grad_in, int grad_in_dtype,
                              void* workspace, size_t workspace_bytes,
                              int B, int J, int Vx, int Vy, int Vz, void* stream);

/*
 * d/d(pts) and d/d(conf) of mvn_dlt (eigenvector perturbation of A^T A, f64).
 *   grad_out (B, J, 3) f32;  grad_pts (B, N, J, 2) f32 written;  grad_conf (B, N, J) f32
 *   written, or NULL (must be NULL when conf is NULL).
 */
int mvn_dlt_backward(const float* proj, const float* pts, const float* conf, const float* grad_out,
                     float* grad_pts, float* grad_conf, int B, int N, int J, void* stream);

/*
 * Batched reprojection error.  Replaces mvn/utils/multiview.py:177-184
 * (calc_reprojection_error_matrix): HALF the Euclidean pixel distance between each 2D point
 * and the projection of its 3D point, f64 arithmetic.
 *
 *   points3d (B, J, 3)    f32
 *   pts      (B, N, J, 2) f32     2D points, pixels
 *   proj     (B, N, 3, 4) f32
 *   out      (B, J, N)    f32
 *
 * MVN_ERR_ARG for a null pointer, MVN_ERR_SHAPE for a non-positive or too large extent.
 */
int mvn_reprojection_error(const float* points3d, const float* pts, const float* proj,
                           float* out, int B, int N, int J, void* stream);

/*
 * RANSAC triangulation of a batch of points with Huber refinement.  Replaces the host loop
 * of mvn/models/triangulation.py:54-128 (RANSACTriangulationNet.triangulate_ransac over
 * B x J).  For each (b, j): every entry i < n_iters of the caller's list of view pairs is a
 * hypothesis -- the unweighted two-view DLT point (f64, multiview.py:119-127), whose inliers
 * are the pair itself and every view with reprojection error < epsilon (strict; a NaN error
 * is no inlier).  A pair with an index outside [0, N) or two equal indices is skipped and
 * never read through.  The hypothesis with the most inliers wins, the lowest i on a tie
 * (triangulation.py:96-97); with no valid pair all views are used (:100-101).  The result
 * is the unweighted DLT over the inlier views and, with direct_optimization = 1, the
 * minimiser of the reference's cost 1/2 sum rho(r_v^2) over them (r_v the half pixel
 * distance, rho scipy's Huber with f_scale 1) by a damped Gauss-Newton iteration in f64
 * that starts at the DLT point and accepts no step that raises the cost.
 *
 *   proj   (B, N, 3, 4) f32,  pts (B, N, J, 2) f32,  2 <= N <= 32
 *   pairs  int32: pairs_per_point = 0: (n_iters, 2), one list for every point;
 *                 pairs_per_point = 1: (B, J, n_iters, 2);  1 <= n_iters <= 4096
 *   out_xyz        (B, J, 3) f32
 *   out_inliers    (B, J)    u32   bit v set: view v was used
 *   out_error_mean (B, J)    f32   mean reprojection error over the inlier views at the
 *                                  returned point (triangulation.py:125-126); may be NULL
 *
 * Stream-ordered, allocates nothing, keeps no state.  MVN_ERR_ARG for a null pointer or a
 * flag other than 0 / 1; MVN_ERR_SHAPE for N < 2, N > 32, n_iters < 1, n_iters > 4096 or a
 * non-positive or too large extent.  Checked before any HIP call.
 */
int mvn_triangulate_ransac(const float* proj, const float* pts, const int32_t* pairs,
                           int pairs_per_point, int n_iters, float epsilon, int direct_optimization,
                           float* out_xyz, uint32_t* out_inliers, float* out_error_mean,
                           int B, int N, int J, void* stream);

/*
 * The algebraic model's forward after the backbone in one launch.  Replaces the chain of
 * mvn/models/triangulation.py:164-191: 2D soft-argmax of heatmaps * multiplier per view
 * (mvn_softargmax2d's arithmetic: the same bits), confidence normalisation
 * c / sum_v c + 1e-5 (f32, the sum sequential in view order; :173-174), upscale to image
 * pixels (:182-183) and the confidence-weighted DLT (mvn_dlt's arithmetic: the same bits as
 * mvn_dlt on out_kp2d and out_conf).
 *
 *   heatmaps  (B, N, J, H, W)  dtype (f32 | bf16), contiguous
 *   proj      (B, N, 3, 4) f32  image-resolution projection matrices
 *   conf      (B, N, J)    f32  raw per-view confidences; NULL = all ones (:161)
 *   scale_x, scale_y            image width / W, image height / H
 *   out_xyz   (B, J, 3)    f32
 *   out_kp2d  (B, N, J, 2) f32  2D points in image pixels: out_xy * (scale_x, scale_y)
 *   out_xy    (B, N, J, 2) f32  2D points in heatmap pixels (what a backward needs)
 *   out_conf  (B, N, J)    f32  normalised confidences
 *   out_maps  (B, N, J, H, W) maps_dtype: the maps mvn_softargmax2d returns; NULL = not wanted
 *
 * One block per (b, j): meant for small batches (latency), 1 <= N <= 32.  Stream-ordered,
 * reentrant, no workspace.  MVN_ERR_ARG for a null required pointer or softmax not 0 / 1;
 * MVN_ERR_SHAPE for N > 32 or a non-positive or too large extent; MVN_ERR_DTYPE for a
 * (dtype, maps_dtype) other than f32/f32, bf16/bf16, bf16/f32.  Checked before any HIP call.
 */
int mvn_algebraic_triangulate(const void* heatmaps, int dtype, float multiplier, int softmax,
                              const float* proj, const float* conf, float scale_x, float scale_y,
                              float* out_xyz, float* out_kp2d, float* out_xy, float* out_conf,
                              void* out_maps, int maps_dtype,
                              int B, int N, int J, int H, int W, void* stream);

/*
 * Test hook (tests only; process-wide, thread-safe): force unprojection code paths.
 *   lds_slots  > 0: LDS slot budget per staging pass of the tiled kernel (small budgets
 *              force the multi-pass and global-gather paths); 0 = the kernel's own budget
 *   kernel     0 = default dispatch, 1 = the simple register-geometry kernel,
 *              2 = the generic tiled kernel (skip the four-view kernel),
 *              3 = the four-view kernel with 16-byte LDS slots (its f32 channels-last shape)
 *                  where the default dispatch takes the 8-byte slots (4 views, f32, NCDHW, exact)
 * Returns MVN_OK, or MVN_ERR_ARG for a negative budget or an unknown kernel.
 */
int mvn_debug_set_unproject(int lds_slots, int kernel);

/*
 * Debug build only (make -C learnable-triangulation-pytorch_amd debug -> libmvn_hip_debug.so,
 * -DMVN_DEVICE_ASSERTS): device-side index / layout assertions count their failures instead of
 * trapping.  Reads and clears the counters of every kernel file: *enabled = 1 in the debug
 * build (0 in the release build, whose kernels carry no checks), *count = failures since the
 * last call, *first_line = source line of the first (0 when none).  Synchronise the device
 * first.  Returns MVN_OK, MVN_ERR_ARG for a null pointer, MVN_ERR_LAUNCH if a copy fails.
 */
int mvn_debug_device_asserts(int* enabled, unsigned* count, unsigned* first_line);

/*
 * Self-test of the device-side assertions: one 64-lane launch whose lanes >= n fail a check
 * (64 - n failures in the debug build, none in the release build).  0 <= n <= 64.
 */
int mvn_debug_dassert_selftest(int n, void* stream);

/*
 * Diagnostics: workgroups of the four-view unprojection kernel resident per CU (its LDS and
 * register budget; the persistent grid is this x the CU count), for f32 (bf16_maps = 0) or
 * bf16 (1) feature maps.  Needs a device; returns a count >= 1.
 */
int mvn_debug_unproject_occupancy(int bf16_maps);

/*
 * Diagnostics: the same count for the f32 softmax kernel of one tile shape of the four-view
 * kernel (csrc/unproject_x4.hip): shape 0 = 16-byte LDS slots, 5 = 8-byte slots.
 * *private_bytes receives the kernel's private-segment (scratch) size per work-item and
 * *registers its register count, both from hipFuncGetAttributes.  Needs a device.  Returns the
 * count, MVN_ERR_ARG for another shape or a null pointer, MVN_ERR_LAUNCH if a query fails.
 */
int mvn_debug_x4_shape_occupancy(int shape, int* private_bytes, int* registers);

/*
 * Diagnostics, host only (no device needed): the block -> tile order of the four-view
 * unprojection kernel (csrc/x4_order.hpp).  tiles[i] receives the tile that block i of a launch
 * over `frames` frames of nTx x nTy x nTz tiles works on (frame-major, then x, y, z tiles, z
 * fastest).  order: 0..3 = an X4Order of x4_order.hpp, -1 = the one the kernel is built with.
 * Returns MVN_OK, or MVN_ERR_ARG (null pointer, a count < 1, more than INT_MAX blocks, unknown
 * order).
 */
int mvn_debug_x4_block_tiles(int order, int frames, int nTx, int nTy, int nTz, int* tiles);

/*
 * Diagnostics, host only: image slots (pixels) one LDS pass of the four-view kernel holds, for
 * its f32 (shape 0), bf16 (1) or 8-view (2) tile shape; a tile whose footprints sum to more is
 * staged in several passes.  Returns the count, or MVN_ERR_ARG for an unknown shape.
 */
int mvn_debug_x4_image_slots(int shape);

/*
 * Diagnostics (tests): mvn_dlt with a trace of its null-vector solver (csrc/dlt_solver.hpp).
 * The same per-point code, so out_xyz (B, J, 3) holds mvn_dlt's bits; per point (B, J, int32)
 *   path   0 = an exactly zero column of R, 1 = inverse iteration, 2 = the Jacobi SVD
 *   steps  the inverse-iteration steps run (path 1), the Jacobi sweeps run, the last,
 *          rotation-free one included (path 2), 0 (path 0).
 * conf may be null (all ones).  Returns MVN_OK, MVN_ERR_ARG for a null pointer, MVN_ERR_SHAPE
 * as mvn_dlt, MVN_ERR_LAUNCH.
 */
int mvn_debug_dlt_trace(const float* proj, const float* pts, const float* conf, float* out_xyz,
                        int* path, int* steps, int B, int N, int J, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVN_HIP_H */
