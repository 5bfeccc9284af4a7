/*
 * transhuman_hip.h -- C ABI of libtranshuman_hip.so (gfx950 / MI355X only).
 *
 * The reference (pansanity666/TransHuman) is 100 % Python; its "native" hot
 * path is a sequence of torch / pytorch3d kernels launched from
 *   lib/networks/renderer/if_clight_renderer.py  (Renderer.render_fast/_render/batchify_rays)
 *   lib/networks/cross_transformer.py            (Network.forward and helpers)
 *   lib/networks/vision_transformer.py           (VisionTransformer.forward)
 *   lib/networks/renderer/nerf_net_utils.py      (raw2outputs)
 *   lib/networks/renderer/if_mesh_renderer.py    (Renderer.render)
 * Each entry point below names the reference lines it replaces.  The Python
 * classes in transhuman_amd/networks/ keep the reference's operator API and
 * bind these symbols with ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - all floating point data is fp32 unless stated (blend matrices: f64);
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *  - functions return 0 on success, <0 on error; th_last_error() gives the text;
 *  - no function allocates device memory: scratch comes from the caller via
 *    (workspace, workspace_bytes), sized with the matching *_workspace_bytes();
 *  - a th_ctx is bound to one device and must be used from one thread at a time.
 */
#ifndef TRANSHUMAN_HIP_H
#define TRANSHUMAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TH_ABI_VERSION 12

typedef struct th_ctx th_ctx;
typedef void* th_stream;

/* ---- library / context ------------------------------------------------ */
int         th_abi_version(void);
const char* th_last_error(void);
int         th_ctx_create(int device, th_ctx** out);
void        th_ctx_destroy(th_ctx* ctx);
/* sizeof() of a struct of this header as the LIBRARY was compiled with it: "th_points", "th_frame", "th_map_source",
 * "th_linear", "th_mlp_weights", "th_vit_block", "th_smpl_model", "th_adam_tensor"; 0 for an unknown name.  A binding written in another language
 * (INTEGRATION.md's ctypes stub) checks its own struct definitions against it -- a struct that is short by one field
 * makes the library read garbage pointers (ABI 10 grew th_points by two). */
size_t      th_sizeof(const char* type_name);

/* ---- stage timing (HIP events on the launch stream) --------------------- */
/* When enabled, the frame-level entry points bracket their stages with
 * hipEventRecord on `stream`; th_profile_read drains the accumulated
 * per-phase milliseconds / launch counts (arrays of TH_PROF_PHASES). */
enum { TH_PROF_HULL = 0, TH_PROF_DPARF = 1, TH_PROF_GATHER = 2, TH_PROF_MLP = 3, TH_PROF_COMPOSITE = 4,
       TH_PROF_VIT = 5, TH_PROF_FOLD = 6 /* th_map_fold: the f-consuming layers applied to the map's texels */, TH_PROF_PHASES = 8 };
int th_profile_enable(th_ctx* ctx, int on);
int th_profile_read(th_ctx* ctx, double* ms_out, int64_t* count_out);
/* Host milliseconds the calling thread spent inside the BLOCKING waits of the entry points (sample counts of
 * th_render_rays / th_render_pregather / th_eval_sigma_grid, th_range_read) since the last call; reads and clears.
 * bench.py subtracts it from the wall time of its queueing loop: what is left is the host's own cost per frame
 * (Python + ctypes + launch calls), the figure that decides whether a short multi-GPU frame is host-bound. */
int th_host_wait_read(th_ctx* ctx, double* ms_out);
/* Shader-clock probe: one wave, ~15 us, queued on `stream`; out_dev[0] = shader-clock ticks, out_dev[1] = the same
 * interval in 10 ns units of the constant 100 MHz counter (GHz = ticks / (10 * units)).  bench.py queues one behind
 * the dominant kernel of every timed step and reports the median: the frequency the chip sustains under the load
 * the roofline is priced at. */
int th_clock_probe(th_ctx* ctx, int64_t* out_dev /* [3] */, th_stream stream);
/* Cycle accounting of the fused MLP kernel (K6) from INSIDE its launches: `counters_dev` = 64 zeroed int64 words of device
 * memory (NULL switches it off).  While set, thread 0 of every 16th tile adds: [0] sampled tiles, [1..61] shader cycles
 * between consecutive workgroup barriers (the tile's phases, in order), [62] shader cycles and [63] ticks of the constant
 * 100 MHz counter over the whole tile -- [62] / (10 [63]) is the shader clock in GHz the chip ran at UNDER this kernel (the
 * probe above runs on whatever CU has room: beside the kernel, not inside it).  Costs ~0.5 % of the launch; bench.py uses it
 * for a short post-run measurement. */
int th_fused_cycles(th_ctx* ctx, int64_t* counters_dev);

/* ---- weights ----------------------------------------------------------- */
/* One dense layer: weight row-major [out_f][in_f] (a Conv1d(k=1)/Linear
 * weight with the trailing 1 squeezed), bias [out_f] or NULL. */
typedef struct {
    const float* w;
    const float* b;
    int out_f;
    int in_f;
} th_linear;

/* Per-point MLP of Network (cross_transformer.py:96-126). */
typedef struct {
    th_linear fc_0, alpha_res_0;
    th_linear key0, val0;          /* spatial_key_value_0 (pixel branch)  */
    th_linear key1, val1;          /* spatial_key_value_1 (token branch)  */
    th_linear fc_1, fc_2, fc_3, alpha_fc;
    th_linear feature_fc, rgb_res_0, view_fc, rgb_res_1, fc_4, rgb_fc;
    /* optional (w == NULL: absent): encoder.upsample_color, the 1x1 conv 3->128 that produces the last 128
     * channels of pixel_feat_map (encoder.py:95,:139).  When given, the three layers that read the 384-channel
     * pixel feature (alpha_res_0, rgb_res_0, rgb_res_1) are ALSO kept in a colour-folded form
     *   W' = [W[:, :256] | W[:, 256:] Wc | 0]  (in_f 260),  b' = b + W[:, 256:] bc
     * which is what the per-sample stage uses with a compact map (th_frame.map_channels = 260): bilinear
     * sampling is linear with weights summing to 1, so sampling r,g,b and lifting afterwards equals
     * sampling the lifted map. */
    th_linear upsample_color;
} th_mlp_weights;

/* One transformer block (vision_transformer.py:285-307). */
typedef struct {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    th_linear qkv, proj, fc1, fc2;
} th_vit_block;

/* Copies + re-packs the weights into the MFMA operand layout owned by ctx.
 * `dparf_alpha`/`n_freq`/`knn` = cfg.KNN_DIST_ALPHA / KNN_FREQ / KNN. */
int th_set_mlp_weights(th_ctx* ctx, const th_mlp_weights* w, th_stream stream);
/* K6 implementation switch: 1 (default) = one fused kernel per 32-sample tile, dense layers on
 * v_mfma_f32_32x32x16_f16 with fp16 hi/lo operand splitting (3 products, fp32 accumulate: fp32-class
 * accuracy); 0 = one fp32-MFMA GEMM launch per layer (exact fp32 products; also the path for V = 4). */
int th_set_mlp_mode(th_ctx* ctx, int mode);
/* Form of the fused kernel (mode 1) on the frame-level path (texel lists + neighbour records): 8 (default) = 512-thread
 * workgroups, two waves per SIMD, every wave owning half the output columns of a layer, dense layers on
 * v_mfma_f32_16x16x32_f16 (k_mlp_fused8_kernel.h, round 6); 4 = the 256-thread form of rounds 2-5 (one wave per SIMD,
 * v_mfma_f32_32x32x16_f16), which also serves every other hand-over (row operands, V = 1..3).  Same tile, same
 * arithmetic (three fp16 products per fp32 MAC); results differ by fp32 summation order only.  New contexts read
 * TH_FUSED_WAVES. */
int th_set_fused_waves(th_ctx* ctx, int waves);
/* K4 -> K6 hand-over of the token branch on the fused path (Network.get_human_representation, cross_transformer.py:151-205,
 * feeding fc_0, :291-295): 1 (default) = K4 writes, per sample, its 7 nearest token centres (as slots of the per-tile
 * union) and their softmax weights, and the fused kernel blends the rows of the per-frame table tokens fc_0[:, :192]^T on
 * the matrix pipe (0.34 KB per sample through HBM); 0 = K4 blends the rows in fp32 and hands them over (3.3 KB per
 * sample; a ray shard then equals the whole frame bit for bit instead of to fp32 rounding).  Env TH_TOK_GATHER=0 makes
 * 0 the default of new contexts. */
int th_set_tok_gather(th_ctx* ctx, int on);
/* K5 -> K6 hand-over of the pixel-aligned features on the fused path (get_pixel_aligned_feature,
 * if_clight_renderer.py:210-269, feeding alpha_res_0 / rgb_res_0 / rgb_res_1, cross_transformer.py:300-346), for frames
 * whose map is TH_MAP_SPLIT: 1 (default) = per 32-sample tile the list of DISTINCT corner texels of its V x 32 rows
 * (~79 of 384 on the headline frame) and per row four row numbers + bilinear weights + the blended colour (160 B per
 * sample); the fused kernel copies those texels -- of the FOLDED maps, th_map_fold / th_frame.map_fold: the layers that read
 * the features are applied to the map's texels once per frame -- into LDS and blends them itself with K5's weights; nothing of
 * the rows travels through HBM and two of the kernel's GEMMs are gone; 0 (or a frame without map_fold) = K5 writes the rows
 * (3.3 KB per sample, read back twice).  Env TH_ROWS_TEX=0 makes 0 the default of new contexts.  Ask th_shade_pool_bytes again
 * after a change. */
int th_set_tex_rows(th_ctx* ctx, int on);

/* Range guard of the fp16 hi/lo split arithmetic (fused MLP kernel, its producer K5, the ResNet-stem convolutions).
 * The reference computes this path in fp32 (cross_transformer.py:291-353 has no autocast); the fused kernel is
 * fp32-class only while every split value satisfies |x| < 65504 (fp16 range) and the tensor it belongs to is not
 * uniformly tiny (below 2^-14 the halves are subnormal: absolute resolution 2^-25).  The kernels keep launch-wide
 * maxima of |x| per split tensor in a device table; th_range_snapshot queues a copy of the table (and clears it)
 * behind the work issued so far on `stream` and returns a snapshot id (>= 0, monotonic; 8 pinned buffers rotate),
 * th_range_read waits for that copy and returns the TH_RANGE_SLOTS words (return value 2: the id is older than the 8
 * most recent snapshots and its buffer has been reused -- the caller must treat the frame as unchecked and render it
 * again): slots 0..5 = fp16 bit pattern of max |hi half| of
 * {f rows (K5), s, p, n, inter, fc_4 operand}; slot 6 = fp32 bit pattern of max |input| of the stem convolutions;
 * inf / NaN show up as values >= 0x7C00 (fp16 slots) / 0x7F800000 (fp32 slot).  th_render_rays,
 * th_eval_sigma_grid and th_network_forward take a snapshot at their end (th_range_last_slot).  A caller that finds
 * a slot >= TH_RANGE_FP16_LIMIT, or a non-zero slot below TH_RANGE_FP16_FLOOR, re-renders with th_set_mlp_mode(ctx, 0)
 * (per-layer fp32 MFMA): transhuman_amd/hip.py does exactly that. */
#define TH_RANGE_SLOTS 8
#define TH_RANGE_FP16_LIMIT 0x7B53u     /* 6.0e4 */
#define TH_RANGE_FP16_FLOOR 0x2400u     /* 2^-6  */
/* slot 7: fp16 bit pattern of max |a| of the operands of TransHE's dense layers (th_gemm_h3).  Slots 6 and 7 are
 * written by the stream that computes a frame's constants and are sticky (not cleared by a snapshot; slot 7 is cleared by
 * th_set_vit_weights, slot 6 by th_set_mlp_weights).  th_set_vit_mode(ctx, 0) moves TransHE's dense layers back to the fp32 MFMA GEMMs;
 * 1 (default): fp16-split arithmetic.  (ABI 5 had a mode 2, the whole forward as one persistent launch: correct, but slower
 * than the 63 launches and resident-workgroup-count dependent -- removed in ABI 6) */
int th_set_vit_mode(th_ctx* ctx, int mode);
int th_range_snapshot(th_ctx* ctx, th_stream stream);
int th_range_read(th_ctx* ctx, int slot, uint32_t* out /* [TH_RANGE_SLOTS] */);
int th_range_last_slot(th_ctx* ctx);
/* Samples shaded per pass of the per-sample stage (process-wide; default 524288, the reference's
 * batchify_rays chunk is 32768, if_clight_renderer.py:575).  Results do not depend on it; workspace
 * sizes do, so call it before the *_workspace_bytes() queries. */
int th_set_chunk_samples(int n);
int th_set_vit_weights(th_ctx* ctx, int depth, int dim, int heads, const th_vit_block* blocks,
                       const float* norm_w, const float* norm_b, th_stream stream);

/* ---- generic dense layer on the fp32 MFMA pipe (building block) -------- */
/* C[M, out_f] = act(A[M, in_f] * W^T + b);  act: 0 none, 1 relu, 2 gelu(erf).
 * lda/ldc in floats.  Packs W on the fly into `workspace`. */
size_t th_linear_workspace_bytes(int out_f, int in_f);
int th_linear_forward(th_ctx* ctx, const float* A, int lda, int M, const th_linear* lin, int act,
                      float* C, int ldc, void* workspace, size_t workspace_bytes, th_stream stream);

/* ---- K1: sample placement + SMPL-hull mask ------------------------------ */
/* if_clight_renderer.py:271-287 (get_sampling_points) + :440-444
 * (knn_points K=1, sqrt, < 0.1, per-ray any) and if_mesh_renderer.py:53-56.
 * Points come either from rays (pts==NULL: p = o + d*(near*(1-t)+far*t),
 * t_vals/one_minus_t are the S linspace values) or explicitly (pts[P,3]).
 * mask_out: uint8[P] (P = R*S or P); ray_hit_out: int32[R] or NULL. */
typedef struct {
    const float* pts;          /* explicit points [P,3] or NULL            */
    const float* ray_o;        /* [R,3]                                    */
    const float* ray_d;        /* [R,3]                                    */
    const float* near;         /* [R]                                      */
    const float* far;          /* [R]                                      */
    const float* t_vals;       /* [S] torch.linspace(0,1,S)                */
    const float* one_minus_t;  /* [S] 1 - t_vals                           */
    int R, S;                  /* rays, samples per ray (S=1 with pts)     */
    /* ABI 10 -- the reference's two sampling randomisations (NULL = off, what run.py:22,68,123 renders with):          */
    const float* z_vals;       /* [R,S] explicit sample depths: the stratified jitter of get_sampling_points            */
                               /* (if_clight_renderer.py:276-283, cfg.perturb > 0 in train() mode) replaces            */
                               /* near*(1-t)+far*t in every stage (hull test, neighbour records, texel lists, deltas)  */
    const float* sigma_noise;  /* [R,S] added to sigma in front of the relu of raw2alpha (nerf_net_utils.py:39-44,      */
                               /* cfg.raw_noise_std > 0: randn * std) on the rays that are composited (hit rays)       */
} th_points;

size_t th_hull_workspace_bytes(int n_verts);
int th_hull_mask(th_ctx* ctx, const th_points* p, const float* verts_world, int n_verts, float thresh,
                 uint8_t* mask_out, int32_t* ray_hit_out, void* workspace, size_t workspace_bytes,
                 th_stream stream);

/* ---- K2: paint SMPL vertices + cluster mean pooling --------------------- */
/* paint_neural_human :95-184 (project, bilinear grid_sample(align_corners,
 * border) of the NCHW holder map, zero invisible vertices) followed by
 * voxelization/can_body_grouping :356-371,:415-427 (CSR segmented mean).
 * cams: per view R[9], T[3], K[9] row-major = 21 floats.  scale_xy: the two
 * floats of sample_from_feature_map :193.  tokens_out [V,N_c,C]. */
int th_paint_group(th_ctx* ctx, const float* holder_map_nchw, int V, int C, int H, int W,
                   const float* verts_world, int n_verts, const float* cams, const float* scale_xy,
                   const uint8_t* vizmap, const int32_t* csr_offsets, const int32_t* csr_members,
                   int n_clusters, float* painted_out /* [V,n_verts,C] or NULL */, float* tokens_out,
                   th_stream stream);
/* voxelization of per-vertex rows: fp32 [n_verts,width] -> [N_c,width] */
int th_segment_mean_f32(th_ctx* ctx, const float* src, int width, const int32_t* csr_offsets,
                        const int32_t* csr_members, int n_clusters, float* out, th_stream stream);
/* blend matrices: f64 [n_verts,16] -> mean in f64 -> top-left 3x3 as fp32
 * [N_c,9] (cross_transformer.py:185) */
int th_segment_mean_rot_f64(th_ctx* ctx, const double* blend, const int32_t* csr_offsets,
                            const int32_t* csr_members, int n_clusters, float* rot_out,
                            th_stream stream);

/* channel counts of the channels-last pixel map */
#define TH_MAP_FULL    384   /* pixel_feat_map as the reference builds it: 256 latent + 128 lifted colour  */
#define TH_MAP_COMPACT 260   /* 256 latent | r g b | 0 : the colour lift is folded into the consumers        */
#define TH_MAP_SPLIT   256   /* the compact map as two planes: [V,H,W,256] latents (1 KiB rows: one aligned wave load per
                                corner texel) immediately followed by [V,H,W,4] (r, g, b, 0); same consumers / folds as 260 */

/* ---- K8: encoder tail written channels-last + painting from that map ------ */
/* encoder.py:133-146: bilinear-upsample (align_corners=True) the three ResNet latents
 * lat0 [V,64,h0,w0], lat1 [V,64,h1,w1], lat2 [V,128,h2,w2] to HxW, append upsample_color(img)
 * (1x1 conv 3->128, color_w [128,3], color_b [128]) and write pixel_feat_map DIRECTLY channels-last
 * [V,H,W,384] (the layout K5 gathers from).  dims_host = {h0,w0,h1,w1,h2,w2} (host ints).
 * color_w == NULL: write the COMPACT map [V,H,W,260] = 256 upsampled latent channels | r g b | 0 instead
 * (a third less HBM written per frame and read per sample; consumers use colour-folded weights). */
int th_upsample_concat_nhwc(th_ctx* ctx, const float* img, const float* lat0, const float* lat1,
                            const float* lat2, const int32_t* dims_host, int V, int H, int W,
                            const float* color_w, const float* color_b, float* out_nhwc, th_stream stream);
/* the compact map in the TH_MAP_SPLIT layout: out = [V,H,W,256] latents followed by [V,H,W,4] (r, g, b, 0) */
int th_upsample_concat_split(th_ctx* ctx, const float* img, const float* lat0, const float* lat1, const float* lat2,
                             const int32_t* dims_host, int V, int H, int W, float* out, th_stream stream);
/* Cropped map.  The reference builds pixel_feat_map over the whole image (encoder.py:133-146) and then samples it only
 * at points within hull_thresh of a target vertex (if_clight_renderer.py:440-444 -> :210-269) and at the projected input
 * vertices (:168-172).  th_map_box computes, per view, the texel box [x0,y0,x1,y1] (inclusive, box_out: device int32
 * [V][4]) that contains every texel such a gather can read: the projections of the eight corners of the axis-aligned cube
 * of half-width `reach` around every vertex of verts_a [na,3] and verts_b [nb,3] (world space; u, v are linear-fractional,
 * so their extrema over a cube in front of the camera sit at corners), in the texel coordinates of grid_sample
 * (align_corners=True, scale_xy as in th_pixel_gather), widened by two texels and clamped to the image (border padding
 * clamps monotonically); the whole image for a view with a cube corner at or behind its camera plane.
 * Behind the V boxes box_out also receives, per view and image row, the SPAN [x0, x1] (inclusive; x1 < x0: empty row) of
 * the vertices' own projected boxes that touch the row -- the body's outline inside the box, about half of it: box_out holds
 * V * 4 + V * H * 2 + V int32 (H <= 4096; the last V words are scratch of the kernels).  th_upsample_concat_split_box writes only the 64-texel runs of `out` that meet their
 * row's span (box == NULL: everything), th_map_fold only the texels inside it; the rest of `out` stays as it was.  No host
 * synchronisation: boxes and spans live on the device. */
int th_map_box(th_ctx* ctx, const float* verts_a, int na, const float* verts_b, int nb, const float* cams, int V,
               const float* scale_xy, int H, int W, float reach, int32_t* box_out, th_stream stream);
int th_upsample_concat_split_box(th_ctx* ctx, const float* img, const float* lat0, const float* lat1, const float* lat2,
                                 const int32_t* dims_host, int V, int H, int W, float* out, const int32_t* box,
                                 th_stream stream);
/* Demand-driven map (round 5).  Behind a th_render_prepass the texels a frame reads are known exactly: the four bilinear
 * corners, in every view, of the prepass's valid samples (get_pixel_aligned_feature, if_clight_renderer.py:210-269 behind the
 * hull mask :440-444) and of the painted input vertices (:168-172).  th_render_predemand (below, with the frame-level entry
 * points) marks them in a demand buffer of th_map_demand_bytes(V, H, W) bytes -- on the device, no host synchronisation --;
 * th_upsample_concat_split_demand writes only those texels of `out` (inside `box`, which may be NULL) and th_map_fold_demand
 * evaluates the folded layers only at the samples' texels (a compacted list: full tiles wherever the texels lie).  A rank of an
 * N-rank job reads about 1 / N of what the whole frame reads, so the map write and the fold shrink with the ray shard.  W must
 * be a multiple of 64.  Frames built this way carry the buffer in th_map_source.demand: a frame-level call whose sample list is
 * not the one the buffer was made from writes the rest of the map first (like the other premises of a cropped map). */
size_t th_map_demand_bytes(int V, int H, int W);
int th_upsample_concat_split_demand(th_ctx* ctx, const float* img, const float* lat0, const float* lat1, const float* lat2,
                                    const int32_t* dims_host, int V, int H, int W, float* out, const int32_t* box,
                                    const void* demand, th_stream stream);
/* paint_neural_human + can_body_grouping without materialising holder_feat_map: reduction_layer
 * (1x1 conv C->out_f, encoder.py:85,146) commutes with the bilinear sampling at :168-172, so the C-channel
 * channels-last map is sampled at the projected vertices and the layer is applied to those V*n_verts
 * rows; then the vizmap zeroing (:181-182) and the cluster mean (:356-371).  tokens_out [V,N_c,out_f].
 * C = 384 (full map) or 260 (compact map: `color_lift` = upsample_color is then required and is folded into
 * the 384-input reduction layer on the fly); color_lift may be NULL for C = 384. */
size_t th_paint_group_nhwc_workspace_bytes(int V, int n_verts, int C, int out_f);
int th_paint_group_nhwc(th_ctx* ctx, const float* map_nhwc, int V, int H, int W, int C,
                        const float* verts_world, int n_verts, const float* cams, const float* scale_xy,
                        const uint8_t* vizmap, const th_linear* reduction, const th_linear* color_lift,
                        const int32_t* csr_offsets,
                        const int32_t* csr_members, int n_clusters, float* tokens_out, void* workspace,
                        size_t workspace_bytes, th_stream stream);

/* K11 -- train-mode BatchNorm2d (+ residual) (+ ReLU), NCHW fp32: the elementwise tail of every ResNet stage of
 * SpatialEncoder.forward (encoder.py:114-126; torchvision BasicBlock: bn -> relu, bn -> += identity -> relu) with
 * the network in train() as run.py:29 leaves it: batch statistics (biased variance), running statistics updated with
 * `momentum` (unbiased variance), exactly F.batch_norm(training=True).  res may be NULL; running_* may be NULL (no
 * update); gamma/beta may be NULL (1 / 0).  y may alias x.  workspace: th_bn_workspace_bytes(N, C, H*W). */
/* K12 -- the bias-free convolutions of the ResNet18 stem (encoder.py:114-126: 7x7/2 3->64, 3x3 64->64, 3x3/2 64->128,
 * 3x3 128->128, 1x1/2 64->128; padding KS/2), NCHW fp32 in and out, as implicit GEMMs on v_mfma_f32_32x32x16_f16 with fp16 hi/lo split
 * operands (fp32-class accuracy).  th_conv_pack turns a [COUT,CIN,KS,KS] weight into the per-lane fragment image
 * (th_conv_pack_bytes bytes, device) and returns the power-of-two output scale to pass to th_conv2d; re-pack when the
 * weight changes.  th_conv2d_supported tells whether a shape is built. */
size_t th_conv_pack_bytes(int cout, int cin, int ks);
int th_conv_pack(th_ctx* ctx, const float* w, int cout, int cin, int ks, void* packed, size_t packed_bytes,
                 float* inv_scale_out, th_stream stream);
int th_conv2d_supported(int cin, int cout, int ks, int stride);
int th_conv2d(th_ctx* ctx, const float* x, int N, int cin, int H, int W, const void* packed, float inv_scale, int cout,
              int ks, int stride, float* y, th_stream stream);

/* nn.MaxPool2d(3, 2, 1) of the stem on [planes, H, W] fp32 -> [planes, (H-1)/2+1, (W-1)/2+1] */
int th_maxpool3x3s2(th_ctx* ctx, const float* x, int planes, int H, int W, float* y, th_stream stream);

size_t th_bn_workspace_bytes(int N, int C, int HW);
int th_bn_act(th_ctx* ctx, const float* x, const float* residual, int N, int C, int HW, const float* gamma,
              const float* beta, float eps, float momentum, float* running_mean, float* running_var, int relu,
              float* y, void* workspace, size_t workspace_bytes, th_stream stream);
/* The same sites with the module in eval() mode (the reference's Trainer.val, lib/train/trainers/trainer.py:131-150, runs
 * network.eval()): y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta [+ residual] [relu]; ONE launch, no
 * statistics pass, nothing updated. */
int th_bn_act_eval(th_ctx* ctx, const float* x, const float* residual, int N, int C, int HW, const float* gamma,
                   const float* beta, float eps, const float* running_mean, const float* running_var, int relu,
                   float* y, th_stream stream);
/* ABI 12 -- a convolution followed by a train-mode BatchNorm (every conv -> bn site of encoder.py:114-126) in TWO launches
 * instead of three: th_conv2d_stats is th_conv2d whose epilogue also leaves, per output channel, the sum and the sum of
 * squares of the values it stored as th_conv2d_stats_partials(...) float2 partials (`stats`: [cout][partials] float2, device,
 * 8-byte aligned); th_bn_act_stats is th_bn_act reading those instead of running its own statistics pass over y (the
 * partials of a channel are added in float64 in a fixed order: deterministic).  Same results as th_conv2d + th_bn_act up
 * to the rounding of the statistics (fp32 partial sums over <= 128 pixels). */
int th_conv2d_stats_partials(int N, int cin, int H, int W, int cout, int ks, int stride);
int th_conv2d_stats(th_ctx* ctx, const float* x, int N, int cin, int H, int W, const void* packed, float inv_scale,
                    int cout, int ks, int stride, float* y, void* stats, size_t stats_bytes, th_stream stream);
int th_bn_act_stats(th_ctx* ctx, const float* x, const float* residual, int N, int C, int HW, const void* stats,
                    int n_partials, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, int relu, float* y, th_stream stream);

/* ---- K3: TransHE (ViT-tiny) ---------------------------------------------- */
/* VisionTransformer.forward, vision_transformer.py:371-383.  x [V,N,dim]
 * tokens, pe [V,N,dim] sin-cos table (host-built, see vision_transformer.py),
 * out [V,N,dim]. */
size_t th_vit_workspace_bytes(int V, int N, int dim, int heads);
int th_vit_forward(th_ctx* ctx, const float* x, const float* pe, int V, int N, float* out,
                   void* workspace, size_t workspace_bytes, th_stream stream);

/* The attention of one TransHE layer on its own (addition, ABI 12; for tests: it feeds the two attention kernels chosen
 * q, k, v).  qkv fp32 [V, N, 3 dim] with column = which dim + head 64 + d (the rows the qkv layer writes), dim = heads 64;
 * out fp32 [V, N, dim] = softmax(q k^T 0.125) v per (view, head).  Runs the K / V^T operand split and then one attention
 * kernel, through the launch code th_vit_forward runs: form 0 = the forward's own choice (N > 700: attn3_kernel, else
 * attn2_kernel), 2 / 3 = attn2_kernel / attn3_kernel at any N; anything else is an argument error.  The result does not
 * depend on what the workspace held.  Operand range: |q|, |k|, |v| < 65504; fp32-class (hi + lo to 2^-22) from 2^-3 up,
 * an absolute 2^-25 per operand below.  Limits: 1 <= V <= 65535, 1 <= N <= 2^24, 1 <= heads <= 1024; qkv, out and the
 * workspace 16-byte aligned.  th_attention_workspace_bytes is 0 for a shape outside them. */
size_t th_attention_workspace_bytes(int V, int N, int heads);
int th_attention(th_ctx* ctx, const float* qkv, int V, int N, int heads, int form, float* out, void* workspace,
                 size_t workspace_bytes, th_stream stream);

/* The training form of that attention (addition, ABI 12).  th_attention_train is th_attention -- the same kernels, the same
 * `form`, bit for bit the same `out` -- which also writes lse fp32 [V][heads][N]: each row's log-sum-exp, natural log, of the
 * scaled logits q.k / 8.  th_attention_bwd takes qkv, that out and lse, and g_out fp32 [V, N, dim] (the gradient of the loss
 * with respect to out) and writes g_qkv fp32 [V, N, 3 dim] in qkv's column layout (it feeds the qkv layer's backward as it
 * is).  The probabilities are recomputed tile by tile from lse on fp32-input MFMA (no operand range); nothing N x N is
 * stored; there are no atomics: two runs agree bit for bit.  lse only centres the exponent: the rows are renormalised by
 * their own recomputed sums, and D = rowsum(g_out * out) is formed from the recomputed probabilities as well (out is
 * required and checked like the others but not read).  At N = 1 the q and k blocks of g_qkv are exactly 0 and the v
 * block is g_out.  Limits and refusals as th_attention: every pointer non-null and 16-byte aligned; the workspace queries
 * are 0 for a shape outside the limits.  Neither result depends on what the workspace held. */
size_t th_attention_train_workspace_bytes(int V, int N, int heads);
int th_attention_train(th_ctx* ctx, const float* qkv, int V, int N, int heads, int form, float* out, float* lse,
                       void* workspace, size_t workspace_bytes, th_stream stream);
size_t th_attention_bwd_workspace_bytes(int V, int N, int heads);
int th_attention_bwd(th_ctx* ctx, const float* qkv, const float* out, const float* lse, const float* g_out, int V, int N,
                     int heads, float* g_qkv, void* workspace, size_t workspace_bytes, th_stream stream);

/* The training form of TransHE's dense layers, LayerNorm and GELU (addition, ABI 12; k_vit_dense_bwd.hip).  Plain fp32 on the
 * MFMA pipe (v_mfma_f32_16x16x4_f32: an fp32 fmaf chain), no fp16 split and so no operand range.  A layer is
 * C[M, out_f] = op(A) W^T + b with W fp32 [out_f, in_f] row-major (th_linear; b may be NULL) and the operand form
 *     form 0: op(A) = A                      A [M, in_f]
 *     form 1: op(A) = LayerNorm(A; ln_w, ln_b, ln_eps) over the row (ln_w, ln_b fp32 [in_f]; in_f <= 256, M <= 8192)
 *     form 2: op(A) = gelu(A), exact erf     (ln_w, ln_b ignored in forms 0 and 2)
 * op(A) is never stored: the backward recomputes it from A on the operand's way into the matrix unit, for form 1 with the
 * row statistics of the forward bit for bit.  Shapes: M >= 1, in_f and out_f multiples of 16, leading dimensions in floats,
 * >= the row and multiples of 4, every pointer 16-byte aligned; anything else is refused with a message (th_last_error)
 * and nothing is launched; the workspace queries return 0 for a refused shape.
 *
 * th_linear_train_forward writes C.  th_linear_bwd takes g_C [M, out_f] = dL/dC and writes
 *     g_W [out_f, in_f] = sum_m g_C[m, :]^T op(A)[m, :]  and  g_b [out_f] = sum_m g_C[m, :]   (g_b may be NULL),
 *     g_A [M, in_f] = dL/dA, THROUGH the operand form (form 1: the LayerNorm backward, form 2: * gelu'(A)); NULL skips it,
 *     form 1 with g_A: g_ln_w [in_f] = sum_m g_op xhat and g_ln_b [in_f] = sum_m g_op, where g_op = g_C W.
 * The sums over m are taken in th_wgrad_chunk_rows() (LayerNorm parameters: th_layernorm_bwd_chunk_rows()) row chunks whose
 * partial results go to the workspace and are added in chunk order: no atomics, two runs agree bit for bit, and the result
 * does not depend on what the workspace held.  g_A must not overlap A or g_C.
 *
 * th_layernorm_forward / th_layernorm_bwd are LayerNorm on its own (dim a multiple of 16 up to 256; the statistics rule of
 * form 1): out = (x - mean) rstd w + b;  g_x = rstd (g w - mean(g w) - xhat mean(g w xhat)), g_w = sum_m g xhat,
 * g_b = sum_m g.  g_x may be g itself (in place). */
int    th_wgrad_chunk_rows(void);
int    th_layernorm_bwd_chunk_rows(void);
size_t th_linear_train_workspace_bytes(int M, int out_f, int in_f, int form);
int th_linear_train_forward(th_ctx* ctx, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b,
                            float ln_eps, const th_linear* lin, float* C, int ldc, void* workspace, size_t workspace_bytes,
                            th_stream stream);
size_t th_linear_bwd_workspace_bytes(int M, int out_f, int in_f, int form);
int th_linear_bwd(th_ctx* ctx, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b, float ln_eps,
                  const th_linear* lin, const float* g_C, int ldg, float* g_A, int ldga, float* g_W, float* g_b,
                  float* g_ln_w, float* g_ln_b, void* workspace, size_t workspace_bytes, th_stream stream);
int th_layernorm_forward(th_ctx* ctx, const float* x, int ldx, int M, int dim, const float* w, const float* b, float eps,
                         float* out, int ldo, th_stream stream);
size_t th_layernorm_bwd_workspace_bytes(int M, int dim);
int th_layernorm_bwd(th_ctx* ctx, const float* x, int ldx, int M, int dim, const float* w, float eps, const float* g, int ldg,
                     float* g_x, int ldgx, float* g_w, float* g_b, void* workspace, size_t workspace_bytes, th_stream stream);

/* The training form of the per-point network's layers (addition, ABI 12; k_pointnet_bwd.hip).  Same arithmetic,
 * conventions and refusals as th_linear_train_forward / th_linear_bwd form 0 above.
 *
 * th_linear_relu_forward: Y [M, out_f] = relu(A W^T + b), the ReLU in the GEMM's epilogue (no extra pass).
 * th_linear_relu_bwd takes A, Y and g_Y = dL/dY and writes what th_linear_bwd form 0 writes for g_C = g_Y * [Y > 0] (the gradient
 * at Y == 0 is 0): g_W, g_b (may be NULL) and g_A (NULL skips it).  The gate is applied on g_Y's way into the weight-gradient
 * kernel; the input gradient costs one elementwise pass over g_Y into the workspace.  g_Y is not modified.  The same
 * th_wgrad_chunk_rows() chunks added in chunk order: no atomics, two runs agree bit for bit, nothing depends on what the
 * workspace held.  g_A must not overlap A, Y or g_Y.
 *
 * th_xview_attention: the cross-view attention of the network (cross_transformer.py:128-149) on its own.  kvp, kvs [P, V, 384]
 * hold the rows [key(128) | value(256)] of the pixel and of the token branch; A[j][i] = kp_j . ks_i / sqrt(128), softmax over j,
 * n_i = vs_i + sum_j A[j][i] vp_j -> n [P, V, 256].  P >= 1, V in 1..4, pointers 16-byte aligned.
 * th_xview_attention_bwd: from g_n [P, V, 256] the gradients g_kvp, g_kvs [P, V, 384] in the layout of the inputs:
 *     g_vs_i = g_n_i,  g_vp_j = sum_i A[j][i] g_n_i,  dA[j][i] = vp_j . g_n_i,  dS[j][i] = A[j][i] (dA[j][i] - sum_j' A[j'][i] dA[j'][i]),
 *     g_kp_j = sum_i dS[j][i] ks_i / sqrt(128),  g_ks_i = sum_j dS[j][i] kp_j / sqrt(128).
 * The probabilities are recomputed from the keys with the forward's statements (bit for bit the forward's); nothing P x V x V
 * is stored; no atomics: two runs agree bit for bit.  At V = 1 both key blocks are exactly 0 and both value blocks are g_n. */
size_t th_linear_relu_workspace_bytes(int M, int out_f, int in_f);
int th_linear_relu_forward(th_ctx* ctx, const float* A, int lda, int M, const th_linear* lin, float* Y, int ldy, void* workspace,
                           size_t workspace_bytes, th_stream stream);
size_t th_linear_relu_bwd_workspace_bytes(int M, int out_f, int in_f);
int th_linear_relu_bwd(th_ctx* ctx, const float* A, int lda, const float* Y, int ldy, int M, const th_linear* lin,
                       const float* g_Y, int ldg, float* g_A, int ldga, float* g_W, float* g_b, void* workspace,
                       size_t workspace_bytes, th_stream stream);
int th_xview_attention(th_ctx* ctx, const float* kvp, const float* kvs, int P, int V, float* n, th_stream stream);
int th_xview_attention_bwd(th_ctx* ctx, const float* kvp, const float* kvs, const float* g_n, int P, int V, float* g_kvp,
                           float* g_kvs, th_stream stream);

/* ---- K4: DPaRF encoding --------------------------------------------------- */
/* Network.get_human_representation, cross_transformer.py:158-205.
 * pts_smpl [P,3]; centres [N_c,3]; rot [N_c,9]; tokens [V,N_c,192];
 * sel: int32[P] indices into pts or NULL (identity).
 * out: [P, V, 256] row-major (255 features + one zero pad column). */
int th_dparf_encode(th_ctx* ctx, const float* pts_smpl, const int32_t* sel, int P, const float* centres,
                    const float* rot, const float* tokens, int V, int n_clusters, float* out,
                    th_stream stream);

/* ---- K5: pixel-aligned feature gather -------------------------------------- */
/* get_pixel_aligned_feature :210-269 on a channels-last map
 * pixel_map_nhwc [V,H,W,C]; pts_world [P,3]; out [P,V,ldo] (ldo >= C floats per row, a multiple of 4;
 * columns C..ldo-1 are written as zeros). */
int th_nchw_to_nhwc(th_ctx* ctx, const float* src, int V, int C, int H, int W, float* dst, th_stream stream);
int th_pixel_gather(th_ctx* ctx, const float* pixel_map_nhwc, int V, int C, int H, int W,
                    const float* pts_world, const int32_t* sel, int P, const float* cams,
                    const float* scale_xy, float* out, int ldo, th_stream stream);
/* The form of the same gather that the frame-level entry points run (ABI 6): the split compact map (th_upsample_concat_split:
 * [V,H,W,256] latents followed by a [V,H,W,4] r g b 0 plane) in, TH_ROWS_SPLIT rows out -- per (sample, view) 272 / 8 groups
 * of [8 fp16 hi halves | 8 fp16 lo halves], x = hi + lo, the layout the fused MLP kernel stages by LDS-DMA; out_rows holds
 * P * V * ldo * 4 bytes.  (Exposed so that the split-row kernel can be tested on its own against th_pixel_gather.) */
int th_pixel_gather_split(th_ctx* ctx, const float* map_split, int V, int H, int W, const float* pts_world,
                          const int32_t* sel, int P, const float* cams, const float* scale_xy, void* out_rows,
                          int ldo, th_stream stream);

/* The layers that read the pixel-aligned features -- alpha_res_0, rgb_res_0 (under the folded view_fc) and rgb_res_1,
 * cross_transformer.py:316, :334, :346 -- applied to the TEXELS of a TH_MAP_SPLIT map instead of to every (sample, view) row:
 * they are linear and act directly on grid_sample's bilinear blends (if_clight_renderer.py:255-265), so they commute with the
 * sampling.  fold [2][V,H,W,256] fp32: plane 0 = alpha_res_0' texel, plane 1 = [Wa rgb_res_0' (128) | rgb_res_1' (128)] texel
 * (no biases; the colour lift is inside, th_mlp_weights.upsample_color).  box: th_map_box's output (boxes + row spans) -> only
 * texels inside each row's span are computed, or NULL: the whole map.  Once per frame, after th_set_mlp_weights; th_frame.map_fold. */
int th_map_fold(th_ctx* ctx, const float* map_split, int V, int H, int W, const int32_t* box, float* fold, th_stream stream);
int th_map_fold_demand(th_ctx* ctx, const float* map_split, int V, int H, int W, const void* demand, float* fold, th_stream stream);

/* K5t, the producer of the texel hand-over (th_set_tex_rows; k_pixtex.hip), on its own -- exposed for tests.  Samples are taken
 * in tiles of 32 consecutive entries (of `sel`, or of the points when sel is NULL); out (th_pixel_texlist_bytes(V, P) bytes,
 * T = ceil(P / 32) tiles) receives
 *   lists   [T][4 passes][128] uint32: word 0 = U | npass << 16 (U <= 103 texel rows of this pass; npass = 1, 2 or 4: sample s of
 *           the tile belongs to pass s / (32 / npass)), words 8 .. 8 + U - 1 = view * H * W + y * W + x of the pass's distinct
 *           corner texels;
 *   records [T][V][32][8]: {w00, w01, w10, w11} (float bits, grid_sample's bilinear weights, if_clight_renderer.py:210-269) and
 *           {o00, o01, o10, o11} = 1040 * (number of the corner's texel in its pass's list).
 * (map_split is not read: the lists depend on the cameras only.) */
size_t th_pixel_texlist_bytes(int V, int P);
int th_pixel_texlist(th_ctx* ctx, const float* map_split, int V, int H, int W, const float* pts_world, const int32_t* sel,
                     int P, const float* cams, const float* scale_xy, void* out, size_t out_bytes, th_stream stream);

/* ---- K6: per-point multi-view MLP ------------------------------------------ */
/* Network.forward, cross_transformer.py:207-353, on already-gathered inputs.
 * pixel_feat [V,384,P] (the reference's channel-major layout); viewdir [P,27];
 * pts_smpl [P,3]; mask uint8[P] or NULL.  raw_out [P,4] (rgb logits, sigma).
 * With a mask: progressive RGB (sigma>0 only) and zero rows where masked out;
 * without: RGB everywhere (MLP_forward_ori :280-289). */
size_t th_network_workspace_bytes(int V, int P);
int th_network_forward(th_ctx* ctx, const float* pixel_feat, const float* viewdir, const float* pts_smpl,
                       const uint8_t* mask, int P, const float* centres, const float* rot,
                       const float* tokens, int V, int n_clusters, float* raw_out, void* workspace,
                       size_t workspace_bytes, th_stream stream);

/* ---- K7: alpha compositing --------------------------------------------------- */
/* raw2outputs, nerf_net_utils.py:14-59.  raw [R,S,4]; z [R,S] or NULL (then
 * recomputed from near/far/t_vals); ray_d [R,3].  Outputs rgb [R,3], acc [R],
 * depth [R]; weights_out [R,S] or NULL. */
int th_composite(th_ctx* ctx, const float* raw, const float* z, const th_points* rays, int white_bkgd,
                 float* rgb, float* acc, float* depth, float* weights_out, th_stream stream);

/* ---- K17: training -- the adjoints of K4, K5 and K7 (additions, ABI 12) ----------------- */
/* Backward of th_dparf_encode with respect to the tokens: grad_out [P,V,256] (columns 192..255 -- positional encoding and
 * pad -- do not depend on the tokens and are ignored) -> grad_tokens [V,N_c,192],
 *   grad_tokens[v,c,:] = sum over (p,k) with idx_k(p) = c of w_k(p) grad_out[p,v,:192],
 * with the 7 neighbours and weights of th_dparf_encode on the same pts_smpl / centres (the forward's own selection code).
 * Every element is written (zeros for a centre nobody selected; P = 0 writes zeros); no float atomics: bit-identical from
 * run to run.  Points, centres and rotations get no gradient.  workspace: th_dparf_encode_bwd_workspace_bytes(P, V, N_c). */
size_t th_dparf_encode_bwd_workspace_bytes(int P, int V, int n_clusters);
int th_dparf_encode_bwd(th_ctx* ctx, const float* pts_smpl, int P, const float* centres, const float* rot, int V,
                        int n_clusters, const float* grad_out, float* grad_tokens, void* workspace, size_t workspace_bytes,
                        th_stream stream);
/* Backward of th_pixel_gather (sel = NULL) with respect to the map: grad_out [P,V,ldo] (columns C.. ignored) ->
 * grad_map_nhwc [V,H,W,C], every element written (the call clears the map, then adds with float atomics: results can differ
 * in the last bits from run to run).  C a multiple of 4. */
int th_pixel_gather_bwd(th_ctx* ctx, int V, int C, int H, int W, const float* pts_world, int P, const float* cams,
                        const float* scale_xy, const float* grad_out, int ldo, float* grad_map_nhwc, th_stream stream);
/* Backward of th_composite with respect to raw: g_rgb [R,3], g_acc [R], g_depth [R] -> g_raw [R,S,4], S <= 256.  z, rays,
 * near and far get no gradient.  Bit-identical from run to run. */
int th_composite_bwd(th_ctx* ctx, const float* raw, const float* z, const th_points* rays, int white_bkgd,
                     const float* g_rgb, const float* g_acc, const float* g_depth, float* g_raw, th_stream stream);

/* ---- K19: training -- the pixel-aligned gather read from the encoder's latents (additions, ABI 12) ---- */
/* What th_upsample_concat_nhwc -> th_pixel_gather (sel = NULL, C = 384) compute, without the [V,H,W,384] map: a bilinear
 * sample (grid_sample, align_corners, border; cams / scale_xy as in th_pixel_gather) of bilinearly upsampled latents
 * (upsample_bilinear2d, align_corners) is a linear combination of at most 3 x 3 texels per latent level.
 * lat0 [V,h0,w0,64], lat1 [V,h1,w1,64], lat2 [V,h2,w2,128]: CHANNELS-LAST fp32; dims = {h0,w0,h1,w1,h2,w2} (host), every
 * level 1 <= h <= H, 1 <= w <= W; img [V,3,H,W]; lift_w [128][3], lift_b [128] (upsample_color); H * W < 2^31.
 * out [P,V,ldo], ldo >= 384 and a multiple of 4: columns 0..63 lat0, 64..127 lat1, 128..255 lat2, 256..383 the lifted colour
 * (columns 384.. are not written); rgb_s [P,V,4]: the blended raw colours (r, g, b, 0).  P = 0: nothing is written. */
int th_latent_gather(th_ctx* ctx, const float* lat0, const float* lat1, const float* lat2, const int32_t* dims,
                     const float* img, const float* lift_w, const float* lift_b, int V, int H, int W, const float* pts_world,
                     int P, const float* cams, const float* scale_xy, float* out, int ldo, float* rgb_s, th_stream stream);
/* Its adjoint with respect to the three latents: grad_out [P,V,ldo] (columns 0..255 are read) -> g_lat0 / g_lat1 / g_lat2 in
 * the latents' channels-last layouts, every element written (the call clears them, then adds with float atomics: results
 * can differ in the last bits from run to run; P = 0 writes zeros).  Points, cameras and the image get no gradient; the
 * lift's own gradient is a reduction over grad_out[..., 256:384] and rgb_s (train_ops.LatentGatherFn). */
int th_latent_gather_bwd(th_ctx* ctx, const int32_t* dims, int V, int H, int W, const float* pts_world, int P,
                         const float* cams, const float* scale_xy, const float* grad_out, int ldo, float* g_lat0,
                         float* g_lat1, float* g_lat2, th_stream stream);
/* The same adjoint with no float atomic (the ordered form): the (sample, view) pairs are sorted by the map pixel of their
 * north-west corner (a stable radix sort: equal pixels keep ascending sample order), and every latent texel sums the pairs that
 * reach it in ascending (map row, map column, sample, slot) order on one fp32 accumulator per channel, with the coefficients
 * of th_latent_gather itself.  Every element of g_lat0 / g_lat1 / g_lat2 is stored exactly once (zeros where nothing
 * arrives; P = 0 writes zeros): nothing is cleared, and neither the outputs' nor the workspace's earlier contents matter.
 * Bit-identical from run to run.  g_lift_w [128,3] and g_lift_b [128] (both or both NULL): the lift's gradient, sums over
 * the P V rows of grad_out[..., 256:384] rgb_s[..., j] and of grad_out[..., 256:384] as fixed-order partial sums; they need
 * rgb_s [P,V,4] of the forward.  V H W < 2^31 - 1.  workspace: th_latent_gather_bwd_ordered_ws(V, H, W, P) bytes (a host
 * computation: no device is touched; 0 for arguments out of range). */
size_t th_latent_gather_bwd_ordered_ws(int V, int H, int W, int P);
int th_latent_gather_bwd_ordered(th_ctx* ctx, const int32_t* dims, int V, int H, int W, const float* pts_world, int P,
                                 const float* cams, const float* scale_xy, const float* grad_out, int ldo,
                                 const float* rgb_s, float* g_lat0, float* g_lat1, float* g_lat2, float* g_lift_w,
                                 float* g_lift_b, void* workspace, size_t workspace_bytes, th_stream stream);

/* ---- K9: ray generation for a target camera --------------------------- */
/* lib/utils/if_nerf/if_nerf_data_utils.py:11-30 (get_rays) + :65-97 (get_near_far) as the test split of
 * sample_ray_h36m uses them (:271-283): one ray per pixel of an H x W camera (K [3,3], R [3,3], T [3] float32,
 * HOST pointers -- 84 bytes of parameters), intersected with the box `bounds_host` = {min xyz, max xyz} of the
 * posed body (padded by 0.01, float64 arithmetic like the reference).  Dense outputs over the H*W pixels in
 * row-major order: ray_o/ray_d [H*W,3] (ray_d carries the reference's |d| < 1e-5 -> 1e-5 clamp), near/far [H*W]
 * (0 where the ray misses), mask_at_box uint8[H*W] (1: exactly two faces hit).  Compact with the mask to get the
 * reference's ray list. */
int th_gen_rays(th_ctx* ctx, const float* K_host, const float* R_host, const float* T_host,
                const float* bounds_host, int H, int W, float* ray_o, float* ray_d, float* near_out,
                float* far_out, uint8_t* mask_at_box, th_stream stream);

/* lib/utils/if_nerf/if_nerf_data_utils.py:49-62 (get_bound_2d_mask): the projected body box as an H x W uint8 mask
 * (used by sample_ray_h36m :211-213 to restrict the foreground mask).  corners_xy_host = the eight box corners
 * (get_bound_corners order, :33-46) projected with base_utils.project and rounded with np.round(..).astype(int)
 * on the HOST (8 points; transhuman_amd/hip.py::bound_2d_mask keeps the reference's numpy expressions); the kernel
 * rasterises the six faces with cv2.fillPoly's scan conversion (even-odd spans + 8-connected edges), vertex lists
 * as in :55-60.  OpenCV is third-party and absent: parity unpinned against cv2 itself, bit-exact against the
 * restatement in oracle/th_oracle.py. */
int th_bound_mask(th_ctx* ctx, const int32_t* corners_xy_host /* [8][2] */, int H, int W, uint8_t* mask,
                  th_stream stream);

/* ---- K13: marching cubes over the sigma cube ------------------------------ */
/* lib/networks/renderer/if_mesh_renderer.py:99-109: `mcubes.marching_cubes(np.pad(cube, 10), cfg.mesh_th)` and the
 * index -> world transform `vertices * voxel_size + (can_bounds[0] - 10 voxel_size)`.  PyMCubes is third-party and
 * absent (parity unpinned against mcubes itself): the published table-driven algorithm is restated in PyMCubes'
 * conventions (corner / edge numbering of the Bourke table, corner "inside" <=> value <= iso, one shared vertex per
 * cut edge at the float64 linear interpolation, table order of triangles) -- see csrc/k_mcubes.hip.
 * cube: [X][Y][Z] fp32 on the device (already padded by the caller).  Usage:
 *   th_marching_cubes_count  passes 1-2 (classification + prefix sums into `workspace`), waits for the stream and
 *                            returns {n_vertices, n_triangles} in counts_host;
 *   th_marching_cubes_emit   writes vertices (float64 [n_vertices,3] = index * scale + origin) and triangles
 *                            (int32 [n_triangles,3], indices into the vertex array) for the grid slab
 *                            x0 <= x < x1 of points / cells (0, X for everything); slabs of one count pass write
 *                            disjoint contiguous ranges of the same arrays (multi-GPU: one slab per rank);
 *   th_marching_cubes_range  {vertex, triangle} prefix at the first point of plane x (x = X: the totals): the
 *                            range a slab [x0, x1) fills is [range(x0), range(x1)).
 * Vertex order: owning grid point row-major, +x / +y / +z edge; triangle order: cell row-major, table order. */
size_t th_marching_cubes_workspace_bytes(int X, int Y, int Z);
int th_marching_cubes_count(th_ctx* ctx, const float* cube, int X, int Y, int Z, float iso, void* workspace,
                            size_t workspace_bytes, int64_t* counts_host /* [2] */, th_stream stream);
int th_marching_cubes_range(th_ctx* ctx, const void* workspace, int X, int Y, int Z, int x,
                            int64_t* prefix_host /* [2] */, th_stream stream);
int th_marching_cubes_emit(th_ctx* ctx, const float* cube, int X, int Y, int Z, float iso, const void* workspace,
                           int x0, int x1, const double* scale_host /* [3] */, const double* origin_host /* [3] */,
                           double* verts, int32_t* tris, th_stream stream);

/* ---- K24: connected components and the component filter of a triangle mesh (additions, ABI 12) ---- */
/* What a user of a marching-cubes mesh does next by hand with trimesh (`max(mesh.split(), key=lambda m: len(m.faces))`), defined
 * here (trimesh is absent): two faces are connected when they share a vertex INDEX (trimesh.split: an edge -- the rules differ only
 * where parts touch in one vertex); the label of a vertex is the smallest vertex index of its component; a vertex no face
 * references keeps its own index and belongs to no component with faces; a component's size is its number of faces.
 * faces: int32 [n_faces][3] on the device, positions double [n_verts][3] (as K13 writes them); either count may be 0.
 *   th_mesh_components    labels int32 [n_verts].  A multi-launch fixpoint of integer atomicMin hooks and pointer jumps (see
 *                         csrc/k_meshcc.hip: no workgroup waits for another); waits for the stream once per batch of sweeps.
 *                         info_host: {components with faces, sweeps, host reads of the sweep flags, label of the largest
 *                         component (most faces, a tie to the smallest label) or -1, its face count}.  More than
 *                         n_verts + 2 sweeps -- no valid mesh -- is an error.
 *   th_mesh_filter_count  keep flags + prefix sums into `workspace` from the labels; min_faces = 0 keeps the largest component,
 *                         n >= 1 every component with at least n faces; vertices without a face are always dropped.  Waits;
 *                         counts_host: {kept vertices, kept faces, components with faces, label of the largest or -1}.
 *   th_mesh_filter_emit   behind it, same workspace and arrays: kept vertices and faces in their original order, indices
 *                         renumbered densely; vert_map int32 [n_verts] = new index or -1.  verts / verts_out may be null.
 * A face index outside [0, n_verts) (th_mesh_filter_count: a label too) is found by a first pass, before anything is indexed by
 * it, and makes the call fail.  Integer atomics only: results are bit-identical from run to run whatever `workspace` held. */
size_t th_mesh_components_workspace_bytes(int n_verts, int n_faces);
int th_mesh_components(th_ctx* ctx, const int32_t* faces, int n_faces, int n_verts, int32_t* labels, void* workspace,
                       size_t workspace_bytes, int64_t* info_host /* [5] */, th_stream stream);
int th_mesh_filter_count(th_ctx* ctx, const int32_t* faces, int n_faces, int n_verts, const int32_t* labels, int min_faces,
                         void* workspace, size_t workspace_bytes, int64_t* counts_host /* [4] */, th_stream stream);
int th_mesh_filter_emit(th_ctx* ctx, const double* verts, const int32_t* faces, int n_faces, int n_verts, const void* workspace,
                        size_t workspace_bytes, double* verts_out, int32_t* faces_out, int32_t* vert_map, th_stream stream);

/* ---- evaluator metrics: SSIM ------------------------------------------------ */
/* lib/evaluators/if_nerf.py:108: skimage's structural_similarity(img_pred, img_gt, multichannel=True) of the evaluator's
 * cropped H x W x 3 float64 images, read as skimage 0.19 computes it for a float64 image without data_range: per channel a
 * 7 x 7 uniform window with sample covariance (49 / 48), data_range 2 (C1 = 4e-4, C2 = 3.6e-3), the mean of the SSIM map over
 * the pixels whose window lies inside the image (rows / columns 3 .. n - 4), then the mean over the channels.  (Pinned by the
 * formula, not by a run of skimage, which is third-party and absent.)
 * a, b: fp32 images [h][w][c] channel-last, rows `pitch` floats apart (>= w * c; a crop of a larger frame is a pointer offset
 * into it); all arithmetic in fp64.  out: ONE double on the device, bit-identical from run to run (fixed-order reduction, no
 * atomics).  Two launches on `stream`.  h < 7 or w < 7: error (skimage raises ValueError); the workspace query then gives 0. */
size_t th_ssim_workspace_bytes(int h, int w, int c);
int th_ssim(th_ctx* ctx, const float* a, const float* b, int h, int w, int c, int pitch, double* out, void* workspace,
            size_t workspace_bytes, th_stream stream);

/* ---- evaluator metrics: LPIPS (VGG16) ---------------------------------------- */
/* lib/evaluators/if_nerf.py:110-117: lpips.LPIPS(net="vgg") (version 0.1, lpips=True, spatial=False, eval mode;
 * third_parties/lpips/lpips.py:81-124) of the evaluator's crops mapped to [-1, 1]: ScalingLayer, VGG16 features[0:30]
 * (13 conv3x3 + ReLU, 4 max pools 2x2 floor), the taps relu1_2 .. relu5_3, per tap normalize_tensor (x / (sqrt(sum_c x^2 +
 * 1e-10) + 1e-10)) of both images, (f0 - f1)^2, the 1x1 lin_k dot (no bias), the spatial mean, then the sum of the taps.
 * Convolutions on the fp32-input MFMA (an fp32 fmaf chain, no reduced precision), the head and the means in fp64.
 * th_lpips_pack: conv_w[l] / conv_b[l] are DEVICE pointers to torchvision's features.{0,2,5,...,28}.weight [COUT][CIN][3][3]
 * / .bias [COUT], fp32; lin_w[k] to lin{k}.model.1.weight [1][C][1][1].  The packed image (th_lpips_pack_bytes() bytes,
 * caller-owned device memory) is written on `stream`.
 * th_lpips: in0, in1: NCHW [n][3][h][w] fp32 in [-1, 1] (device).  out: doubles [n][6] on the device: the five tap values
 * and their sum.  Both images go through the same launches (lpips(a, a) == 0 exactly); fixed-order reductions, no atomics:
 * bit-identical from run to run.  h < 16 or w < 16 (the fifth tap would be empty): error before any device work, and the
 * workspace query gives 0. */
size_t th_lpips_pack_bytes(void);
int th_lpips_pack(th_ctx* ctx, const float* const* conv_w /* [13] */, const float* const* conv_b /* [13] */,
                  const float* const* lin_w /* [5] */, void* packed, size_t bytes, th_stream stream);
size_t th_lpips_workspace_bytes(int n, int h, int w);
int th_lpips(th_ctx* ctx, const float* in0, const float* in1, int n, int h, int w, const void* packed, double* out,
             void* workspace, size_t workspace_bytes, th_stream stream);

/* ---- K21: LPIPS (VGG16) as the training loss -- its gradient with respect to in0 (additions, ABI 12) ------------ */
/* lib/train/trainers/if_nerf_clight.py:68-72 back-propagates through the metric above into the rendered patches; in1 is the
 * target and the VGG16 / lin weights are frozen, so only d total / d in0 exists.
 * th_lpips_pack_bwd: a second packed image (th_lpips_bwd_pack_bytes() bytes) from the same conv_w as th_lpips_pack: the taps
 * rotated by 180 degrees with the channel roles swapped, so that the input gradient of every 3x3 convolution runs through the
 * forward's MFMA tile (per 8-channel chunk a fresh fp32 chain, the chunks summed in fp32).
 * th_lpips_train: th_lpips -- the same launches, `out` bit-identical -- writing into `state` (th_lpips_train_state_bytes,
 * caller-owned) instead of a workspace.  Kept for th_lpips_bwd: the post-ReLU output of all 13 layers of the in0 images and
 * the five taps of the in1 images (NHWC); behind them scratch of the forward alone (in1's other layers, the pooled maps, the
 * head's partials).  Every byte th_lpips_bwd reads is written here.
 * th_lpips_bwd: g_out: doubles [n], the gradient of each image's total (out[i][5]); g_in0: fp32 NCHW [n][3][h][w], every
 * element written.  From the deepest level to the first: the head's derivative in fp64 at the stored fp32 features, rounded
 * to fp32 and added to the gradient from the deeper level; ReLU gates [y > 0] from the stored outputs; the max pools route to
 * the first element of a window (row-major) that equals its maximum, as torch does, cropped rows / columns get 0; layer 0
 * applies 1 / scale[c] of the ScalingLayer.  `in0` is the batch `state` was made from (not read: the state holds every
 * activation).  No atomics: bit-identical from run to run.  No host wait.  h, w >= 16 as for th_lpips (size queries give 0).
 * The stages on their own -- th_lpips_dgrad, th_lpips_pool_bwd, th_lpips_head_bwd: entries for the per-stage tests against
 * float64, NOT part of the stable surface: their signatures may change or go without an ABI version step; callers use
 * th_lpips_bwd.  Any H, W >= 1:
 * th_lpips_dgrad: g fp32 NHWC [Z][H][W][COUT_layer] -> out NHWC [Z][H][W][CIN_layer], 0 where gate_or_null (same layout as
 * out) is <= 0; layer 0: out NCHW [Z][3][H][W] times 1 / scale[c], no gate.
 * th_lpips_pool_bwd: g [Z][H/2][W/2][C], y [Z][H][W][C] (the map that was pooled) -> out [Z][H][W][C]; C a multiple of 4.
 * th_lpips_head_bwd: f0, f1 fp32 [N][hw][C], lin fp32 [C], g_out doubles [N] -> g [N][hw][C] = (accumulate ? g : 0) +
 * fp32(g_out[n] / hw * d head / d f0), then 0 where gate != 0 and f0 <= 0; C a multiple of 32. */
size_t th_lpips_bwd_pack_bytes(void);
int th_lpips_pack_bwd(th_ctx* ctx, const float* const* conv_w /* [13] */, void* packed_bwd, size_t bytes, th_stream stream);
size_t th_lpips_train_state_bytes(int n, int h, int w);
int th_lpips_train(th_ctx* ctx, const float* in0, const float* in1, int n, int h, int w, const void* packed, double* out,
                   void* state, size_t state_bytes, th_stream stream);
size_t th_lpips_bwd_workspace_bytes(int n, int h, int w);
int th_lpips_bwd(th_ctx* ctx, const double* g_out, const float* in0, int n, int h, int w, const void* packed,
                 const void* packed_bwd, const void* state, size_t state_bytes, float* g_in0, void* workspace,
                 size_t workspace_bytes, th_stream stream);
/* (test entries, may change:) */
int th_lpips_dgrad(th_ctx* ctx, int layer, const float* g, const float* gate_or_null, int Z, int H, int W,
                   const void* packed_bwd, float* out, th_stream stream);
int th_lpips_pool_bwd(th_ctx* ctx, const float* g, const float* y, int Z, int H, int W, int C, float* out, th_stream stream);
int th_lpips_head_bwd(th_ctx* ctx, const float* f0, const float* f1, int N, int hw, int C, const float* lin,
                      const double* g_out, int accumulate, int gate, float* g, th_stream stream);

/* ---- K14: mesh rasteriser, vertex visibility maps and SMPL depth maps -------------------------- */
/* batch['input_vizmaps'] ([1, V, 6890], the mask paint_neural_human applies at if_clight_renderer.py:176-182) and
 * batch['input_depthmaps'] are LOADED by the reference from the .npy files of rasterize_root/<human>/{visibility,depth} (can_smpl.py:439-475);
 * no program of the reference writes those files, so the rasteriser below is defined by this project (DESIGN.md 4 K14,
 * restated in numpy by transhuman_amd.visibility.rasterize_oracle):
 *   float64 projection of :123-126 without contraction; pixel centre (col, row) at (u, v) = (col, row); vertices snapped to 1/256
 *   pixel round-half-even; int64 edge functions with the top-left rule (y down), either winding, no back-face culling; a triangle
 *   is skipped for a view when a vertex has z <= 1e-3 or |u| or |v| >= 2^20, or when its snapped area is 0 -- there is NO
 *   clipping; depth = 1 / sum(w_i / z_i) in float64 rounded once to fp32; z-buffer of uint64 keys (depth bits << 32 | face)
 *   under a 64-bit atomicMin: nearest fragment, then lowest face index -- deterministic, independent of launch shape.
 * th_rasterize_mesh: verts_world fp32 [nv][3], faces int32 [nf][3] (either winding), cams [V][21] (R[9] T[3] K[9] row-major, as
 * everywhere here) -> depth fp32 [V][H][W] (`background` where nothing landed) and pix_to_face int32 [V][H][W] (-1 there).  Five
 * operations on `stream`, then ONE host wait on it: a face index outside [0, nv) is never dereferenced, its triangle is skipped
 * and the call returns an error.  1 <= H, W <= 16384; V H W, V nf, V nv < 2^31 (the workspace query gives 0 otherwise).
 * th_vertex_visibility: vis uint8 [V][nv] (the format th_paint_group* takes) = 1 iff the vertex is a corner of a face that owns
 * at least one pixel of pix_to_face[v]; entries of pix_to_face / faces outside the mesh are ignored.  No host wait.
 * th_depth_visibility: get_relative_depth, if_clight_renderer.py:75-93 as :129-133 calls it, in fp32: depthmaps fp32 [V][H][W]
 * sampled at uv / H * 2 - 1 (both coordinates over H, :85) by F.grid_sample's defaults (bilinear, zeros, align_corners=False)
 * -> surface_depth [V][nv]; vis_mask uint8 [V][nv] = depth <= surface + det; relative_depth [V][nv] = depth - (surface + det),
 * depth = the fp32 p_2 of :123-125.  No host wait. */
size_t th_rasterize_workspace_bytes(int V, int n_verts, int n_faces, int H, int W);
int th_rasterize_mesh(th_ctx* ctx, const float* verts_world, int n_verts, const int32_t* faces, int n_faces, const float* cams,
                      int V, int H, int W, float background, float* depth, int32_t* pix_to_face, void* workspace,
                      size_t workspace_bytes, th_stream stream);
int th_vertex_visibility(th_ctx* ctx, const int32_t* pix_to_face, const int32_t* faces, int n_faces, int n_verts, int V, int H,
                         int W, uint8_t* vis, th_stream stream);
int th_depth_visibility(th_ctx* ctx, const float* verts_world, int n_verts, const float* cams, int V, const float* depthmaps,
                        int H, int W, float det, float* surface_depth, uint8_t* vis_mask, float* relative_depth,
                        th_stream stream);

/* ---- K15: vertex normals and normal-coloured Phong frames of a mesh ---------------------------- */
/* render_mesh_dynamic.py:182-276 of the reference renders each extracted mesh with pytorch3d (MeshRasterizer, faces_per_pixel 1,
 * blur_radius 0; SoftPhongShader, PointLights at (0, 3, 0), default Materials; verts_rgb = 0.7 n + 0.7 with n the normals of the
 * mesh in the camera frame with y and z flipped).  pytorch3d is third-party and absent: parity with it is UNPINNED; the image
 * below is defined by this project after those settings and restated in float64 / int64 numpy by
 * transhuman_amd.mesh_render.vertex_normals_oracle / render_mesh_oracle.  Float64 on the exactly promoted fp32 inputs, no
 * contraction, every output rounded once to fp32.
 * th_vertex_normals: verts fp32 [nv][3], faces int32 [nf][3] -> normals fp32 [nv][3], pytorch3d's area-weighted rule: every corner
 * of a face receives c = (v1 - v0) x (v2 - v0), as the int64 q = rint(c 2^40) summed with 64-bit vector atomics (exact: the
 * result does not depend on the order of the faces or the launch shape, bit for bit), n = s / max(|s|, 1e-6), (0, 0, 0) for a
 * vertex without faces or with cancelling ones; flip != 0 negates.  Faces the rasteriser would skip count.  Two memsets and two
 * kernels on `stream`, NO host wait -- so what only the device can see is reported in `status`, ONE int32 on the device, valid
 * once the stream has passed the call: bit 0: a face index outside [0, nv) (never dereferenced, the face adds nothing); bit 1: a
 * face with |c_k| 2^40 > 2^62 / nf or not finite (outside the range in which no sum can leave int64; it adds nothing -- nothing
 * ever wraps).  0: the normals are valid.  transhuman_amd.mesh_render reads the word and raises.  The workspace holds the int64
 * sums [nv][3] at its start when the call has run.
 * th_shade_mesh: pix_to_face int32 [V][H][W] as th_rasterize_mesh wrote it for the same verts, faces and cams; vertex_normals as
 * above -> image fp32 [V][H][W][3], unclamped.  At a covered pixel the perspective-correct weights b_i = (w_i / z_i) / sum(w_j / z_j)
 * from the same snapped int64 edge functions as the rasteriser, p = sum b_i v_i, nh = unit(sum b_i n_i), texel t = sum b_i (0.7 F R n_i
 * + 0.7) with F = diag(1, -1, -1), lh = unit(light - p), vh = unit(-R^T T - p), d = nh . lh,
 * colour = (ambient + diffuse max(d, 0)) t + specular [d > 0] max(vh . (2 d nh - lh), 0)^shininess (unit(x) = x / max(|x|, 1e-6);
 * shininess a power of two, taken by squaring; the reference's settings: 0.5, 0.3, 0.2, 64).  Elsewhere, and where pix_to_face
 * names no face of the mesh: `background`, exactly.  light_host / background_host: 3 floats each on the HOST.  One kernel, no
 * host wait, no workspace.  V <= 65535; the rasteriser's limits on H, W otherwise. */
size_t th_vertex_normals_workspace_bytes(int n_verts, int n_faces);
int th_vertex_normals(th_ctx* ctx, const float* verts, int n_verts, const int32_t* faces, int n_faces, int flip, float* normals,
                      int32_t* status, void* workspace, size_t workspace_bytes, th_stream stream);
int th_shade_mesh(th_ctx* ctx, const float* verts_world, const float* vertex_normals, int n_verts, const int32_t* faces,
                  int n_faces, const float* cams, int V, int H, int W, const int32_t* pix_to_face, const float* light_host /* [3] */,
                  const float* background_host /* [3] */, float ambient, float diffuse, float specular, int shininess, float* image,
                  th_stream stream);

/* ---- K16: the input views from the raw camera pictures (undistort, resize, mask) ---------------- */
/* The reference's dataset prepares every input view on the host with OpenCV (lib/datasets/light_stage/can_smpl.py:118-200 get_mask /
 * get_input_mask, :629-660 process_loaded: / 255, cv2.undistort, cv2.resize INTER_AREA / INTER_NEAREST, black-out under the mask,
 * 5 x 5 erode / dilate border marked 100).  OpenCV is absent: parity with cv2 is UNPINNED (its SIMD paths may fuse the four-tap
 * sum; its 15-bit weight table has a saturation fix-up that is not reproduced); the image below is defined by this project after
 * OpenCV's documented algorithm and restated in numpy by transhuman_amd.preprocess.prepare_views_oracle /
 * combine_masks_oracle, which the device equals bit for bit: every step is one correctly rounded IEEE operation in a fixed order.
 * th_prep_views: img uint8 [V][H0][W0][3], msk uint8 [V][H0][W0], K fp32 [V][9] row-major, D fp32 [V][5] = (k1, k2, p1, p2, k3), lut
 * fp32 [256] = float(i) / 255.0f -- all DEVICE pointers -- n = 1 / ratio in {1, 2, 4} dividing H0 and W0, H = H0 / n, W = W0 / n
 * -> out_img fp32 [V][3][H][W], out_msk uint8 [V][H][W].  For source pixel (col j, row i), in float64 on the promoted K, D:
 * x = (j - cx) / fx, y = (i - cy) / fy, r2 = x x + y y, t = (2 x) y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2,
 * xd = (x kr + p1 t) + p2 (r2 + 2 x x), yd = (y kr + p1 (r2 + 2 y y)) + p2 t, u = fx xd + cx, v = fy yd + cy, iu = rint(32 u),
 * iv = rint(32 v) (|32 u| >= 2^30 or not finite: every tap outside), X = iu >> 5, a = iu & 31 (Y, b alike); taps (X,Y) (X+1,Y) (X,Y+1)
 * (X+1,Y+1) with integer weights (32-b)(32-a), (32-b) a, b (32-a), b a, a tap outside the image being 0; picture in fp32
 * o = ((s00 w00 + s01 w01) + s10 w10) + s11 w11 with s = lut[u8], w = W / 1024; mask (W00 m00 + ... + 512) >> 10 in integers.  Resize:
 * the n x n block of o summed in row-major order from 0, times 1 / (n n); mask at [n y][n x].  mask_bkgd != 0: where the resized
 * mask is 0 the picture is 0 (1 with white_bkgd != 0).  One kernel, no host wait, no workspace.
 * th_prep_mask: a, b_or_null uint8 [V][H0][W0] -> out uint8 [V][H0][W0] (not in place): m = (a != 0) | (b != 0); border = 0: that;
 * border odd <= 15: 100 where the maximum and minimum of m over the border x border window (the pixels of it inside the image)
 * differ.  One kernel, no host wait.  1 <= H0, W0 <= 16384, V <= 65535 for both. */
int th_prep_views(th_ctx* ctx, const uint8_t* img_u8, const uint8_t* msk_u8, int V, int H0, int W0, const float* K /* [V][9] */,
                  const float* D /* [V][5] */, int n, int mask_bkgd, int white_bkgd, const float* lut /* [256] */, float* out_img,
                  uint8_t* out_msk, th_stream stream);
int th_prep_mask(th_ctx* ctx, const uint8_t* a, const uint8_t* b_or_null, int V, int H0, int W0, int border, uint8_t* out,
                 th_stream stream);

/* ---- K25: colour jitter of the raw camera frames, in front of K16 (additions, ABI 12) ---------------- */
/* The reference's dataset puts the raw uint8 frame of the target view and of every input view through torchvision's ColorJitter
 * before it undistorts them (lib/datasets/light_stage/can_smpl.py:629-637; training only).  torchvision is absent: the order of
 * operations follows its documented ColorJitter and parity with it is UNPINNED; the arithmetic is Pillow's (ImageEnhance.Brightness /
 * Contrast / Color, convert("HSV") / convert("RGB")), restated in numpy by transhuman_amd.preprocess.color_jitter_oracle, which the
 * device equals bit for bit.  img uint8 [V][H][W][3] -> out uint8 [V][H][W][3], DEVICE pointers; out may be img
 * itself (otherwise the two must not overlap).  Step k = 0..3 runs operation (order >> 2 k) & 3 -- 0 brightness, 1 contrast,
 * 2 saturation, 3 hue; order must hold each once -- if bit `operation` of `enabled` is set.  Per pixel:
 * L = (19595 R + 38470 G + 7471 B + 32768) >> 16; blend(d, x, f) = d + f (x - d) in fp32 (x - d in integers, product and sum rounded
 * one by one), truncated for 0 <= f <= 1, otherwise 0 where <= 0, 255 where >= 255, else truncated; brightness blend(0, x, f);
 * saturation blend(L, x, f); contrast blend(m, x, f) with m = (2 sum L + H W) / (2 H W) in integers over THAT image as it stands at
 * that step; hue: Pillow's RGB -> HSV, H <- (H + hue_shift) & 255 (hue_shift = trunc(255 h) mod 256, 0..255), Pillow's HSV -> RGB,
 * every product, quotient, sum and difference rounded on its own (no fused multiply-add); hue_shift = 0 still makes the lossy
 * round trip.  Without contrast: one launch, no workspace read (it may be null).  With contrast: two launches; the first STORES one
 * 64-bit partial sum of L per workgroup into the workspace, the second adds them per image -- no atomics, nothing to clear, correct
 * whatever the workspace held, bit-identical from run to run.  No host wait.  1 <= H, W <= 16384, V <= 65535; enabled factors
 * finite and >= 0; the workspace 8-byte aligned and at least th_color_jitter_workspace_bytes(V, H, W) (0 for sizes out of range). */
size_t th_color_jitter_workspace_bytes(int V, int H, int W);
int th_color_jitter(th_ctx* ctx, const uint8_t* img_u8, int V, int H, int W, uint32_t order, float brightness, float contrast,
                    float saturation, int hue_shift, uint32_t enabled, uint8_t* out_u8, void* workspace, size_t workspace_bytes,
                    th_stream stream);

/* ---- K18: the training targets of a step -- patch ray sampling (additions, ABI 12) ---------------- */
/* The train split of sample_ray_patch (lib/utils/if_nerf/if_nerf_data_utils.py:445-499 with :287-443), which the reference runs per
 * step in numpy inside its dataset, on the dense per-pixel arrays of th_gen_rays.  All pointers are DEVICE pointers.
 * Inputs: ray_o, ray_d fp32 [H W][3], near, far fp32 [H W], ray_mask uint8 [H W] as th_gen_rays writes them; msk uint8 [H][W] (any
 * values, 100 = silhouette border); bound_mask uint8 [H][W] (th_bound_mask); img fp32, channel c of pixel p at
 * img[p pix_stride + c chan_stride] (HWC: 3, 1; CHW: 1, H W); draws fp64 [N][2] in [0, 1); subject_ratio; N patches of P x P.
 * m = msk * bound_mask in uint8, human = m > 0, background = ray_mask & ~human.  Patch i: candidate set = human if
 * draws[i][0] < subject_ratio else background, n its pixel count, centre = its k-th pixel in row-major order,
 * k = min(floor(draws[i][1] n), n - 1) with the product in fp64; x_min = clip(cx - P / 2, 0, W - P), y_min alike.
 * Outputs: patch_masks / patch_masks_sub uint8 [N][P][P] = ray_mask / human on the window; target_patches fp32 [N][P][P][3];
 * xy_min int32 [N][2] = (x_min, y_min); counts int32 [2][N] = n, then the window's ray count; and the ray list, patch after patch,
 * each window's ray_mask pixels in row-major order (rows allocated at the bound N P P, the first sum(counts[1]) are written):
 * out_rgb, out_ray_o, out_ray_d fp32 [.][3], out_near, out_far fp32 [.], out_sub_mask uint8 [.] (human), out_select_inds int64 [.]
 * (cumsum(ray_mask) - 1 at the pixel).  A patch whose candidate set is empty writes nothing but counts[0][i] = counts[1][i] = 0
 * (the reference raises there).  No atomics: bit-identical from run to run.  No host wait.
 * Limits (argument errors otherwise): 1 <= H, W <= 4096, 1 <= P <= 64, P <= min(H, W), 1 <= N <= 64. */
size_t th_patch_workspace_bytes(int H, int W);
int th_patch_rays(th_ctx* ctx, const float* ray_o, const float* ray_d, const float* near, const float* far, const uint8_t* ray_mask,
                  const uint8_t* msk, const uint8_t* bound_mask, const float* img, long long pix_stride, long long chan_stride, int H,
                  int W, const double* draws, double subject_ratio, int N, int P, uint8_t* patch_masks, uint8_t* patch_masks_sub,
                  float* target_patches, int32_t* xy_min, int32_t* counts, float* out_rgb, float* out_ray_o, float* out_ray_d,
                  float* out_near, float* out_far, uint8_t* out_sub_mask, int64_t* out_select_inds, void* workspace,
                  size_t workspace_bytes, th_stream stream);

/* ---- K10: SMPL linear blend skinning ------------------------------------ */
/* SMPL._call, lib/utils/SMPL.py:114-186, float64 like the reference.  Model arrays (DEVICE pointers, the fields
 * the reference reads from the SMPL pickle, :83-89): v_template [nv,3], shapedirs [nv,3,10], posedirs [nv,3,207],
 * J_regressor [24,nv] dense, weights [nv,24], parent int32[24] (parent[0] = -1).
 * Pose: either pose_aa = 72 float32 axis-angle values (cv2.Rodrigues form, :135-139) or rot = [24,3,3] float32
 * rotation matrices (:131-132); exactly one of the two is non-NULL.  beta: 10 float64 (device).
 * Outputs (device, float64): verts [nv,3] (SMPL-space posed vertices, :186), joints [24,3] (:163),
 * T [nv,4,4] (= the path's blend_mtx, :176). */
typedef struct {
    const double* v_template;
    const double* shapedirs;
    const double* posedirs;
    const double* J_regressor;
    const double* weights;
    const int32_t* parent;
    int n_verts;
} th_smpl_model;
size_t th_smpl_workspace_bytes(int n_verts);
int th_smpl_lbs(th_ctx* ctx, const th_smpl_model* model, const float* pose_aa, const float* rot, const double* beta,
                double* verts, double* joints, double* T, void* workspace, size_t workspace_bytes,
                th_stream stream);

/* view-direction embedding, if_clight_renderer.py:525-526 + embedder.py:9-35:
 * ray_d [R,3] -> [R, 3 + 6*view_res] */
int th_view_embed(th_ctx* ctx, const float* ray_d, int R, int view_res, float* out, th_stream stream);

/* ---- frame-level entry points -------------------------------------------------- */
/* What a cropped TH_MAP_SPLIT map was made from (host struct, device pointers; everything must stay alive as long as the
 * frame is used).  The frame-level entry points write the rest of the map themselves -- on their stream, in front of the
 * gather -- when a call leaves the crop's premise: the un-masked branch (R' <= small_frame_rays shades EVERY sample of
 * the hit rays), hull_thresh < 0 (no hull test) or hull_thresh > reach. */
typedef struct {
    const int32_t* box;            /* device [V][4] + [V][H][2], th_map_box    */
    float          reach;          /* the reach the box was computed with      */
    const float*   img;            /* arguments of th_upsample_concat_split    */
    const float*   lat0;
    const float*   lat1;
    const float*   lat2;
    int32_t        dims[6];
    const void*    demand;         /* NULL, or the th_render_predemand buffer the map (and its fold) was written for: only the
                                      texels the valid samples of THAT th_render_prepass (and the painted vertices) read exist */
} th_map_source;

/* Per-frame constants produced by th_paint_group / th_vit_forward / the
 * segment means, consumed by the per-sample stage. */
typedef struct {
    const float* verts_world;      /* [n_verts,3] tar_smpl_vertice            */
    int          n_verts;
    const float* Rh;               /* [9]                                     */
    const float* Th;               /* [3]                                     */
    const float* cams;             /* [V,21]                                  */
    const float* scale_xy;         /* [2]                                     */
    const float* pixel_map_nhwc;   /* [V,H,W,map_channels]                    */
    int          V, H, W;
    int          map_channels;     /* TH_MAP_FULL (384), TH_MAP_COMPACT (260) or TH_MAP_SPLIT (256 + 4; the last two need
                                      upsample_color weights) */
    const float* tokens;           /* [V,N_c,192] ViT output                  */
    const float* centres;          /* [N_c,3]                                 */
    const float* rot;              /* [N_c,9]                                 */
    int          n_clusters;
    float        hull_thresh;      /* 0.1                                     */
    int          small_frame_rays; /* 2400: R' <= this -> un-masked branch    */
    const th_map_source* map_source; /* NULL: pixel_map_nhwc is complete; else it is cropped to map_source->box */
    const float* map_fold;         /* NULL, or th_map_fold's output for pixel_map_nhwc (TH_MAP_SPLIT, same crop): [2][V,H,W,256];
                                      with it (and th_set_tex_rows 1) the per-sample stage takes the texel hand-over */
} th_frame;

/* Renderer.render_fast :429-484 incl. _render/batchify_rays/raw2outputs for a
 * range of rays (the unit that is sharded across GPUs).  Outputs are dense
 * over the R rays (zeros for rays that miss the hull).
 * stats_host (optional, int64[4]): hit rays, valid samples, range-guard snapshot slot (th_range_read), mode.
 *
 * Two caller-supplied buffers (ABI 6; one 25 GB worst-case workspace per frame in flight before):
 *  - `workspace` (th_render_workspace_bytes: ~25 B per SAMPLE of the ray list -- hull mask, sample list, dense raw, counts,
 *    view embeddings, the per-frame token table): one per frame in flight, it is what th_render_prepass writes;
 *  - `shade_pool` (th_shade_pool_bytes: ~0.5 KB per VALID sample on the fused path with the texel hand-over -- K5t's texel
 *    lists and row records (get_pixel_aligned_feature :210-269), the neighbour records and positional encodings of K4;
 *    ~3.6 KB with th_set_tex_rows(ctx, 0), when K5 writes the pixel-feature rows and K6 reads them back): ONE per context, shared by every workspace (the per-sample stage of a context runs
 *    on one stream at a time).  It is sized from the frame's valid-sample count, which th_render_prepass_wait puts on
 *    the host before the stage is queued; without a prepass size it for n_valid = R * S (then only the chunk buffers of
 *    th_set_chunk_samples samples are needed: the count bounds the chunk, not the pool). */
size_t th_render_workspace_bytes(const th_frame* f, int R, int S);
/* `f` needs V, H, W and map_channels; the result depends on the context's MLP / token-gather / texel hand-over modes (ask
 * again after th_set_mlp_mode / th_set_tok_gather / th_set_tex_rows).  with_pregather = 1: large enough for th_render_pregather + th_render_rays. */
size_t th_shade_pool_bytes(th_ctx* ctx, const th_frame* f, long long n_valid, int with_pregather);
int th_render_rays(th_ctx* ctx, const th_frame* f, const th_points* rays, float* rgb, float* acc,
                   float* depth, int white_bkgd, void* workspace, size_t workspace_bytes,
                   void* shade_pool, size_t shade_pool_bytes, int64_t* stats_host, th_stream stream);

/* Optional: run the ray-only front of th_render_rays (sample placement + hull mask :440-444, the R' <= 2400
 * rule :551, compaction, view-direction embedding) ahead of time.  It needs only the rays and, of `f`, the
 * fields verts_world / n_verts / V / hull_thresh / small_frame_rays -- so it can be queued BEFORE the per-frame
 * constants (encoder, tokens) are produced; its sample count then reaches the host while that work runs and the
 * following th_render_rays (same ctx, same workspace, same ray arrays) neither repeats the stage nor stalls the
 * queue on the read-back.  `stream` may differ from the stream of th_render_rays (which waits on an event): on a
 * side stream the hull pass fills the chip while the latency-bound encoder / TransHE launches run.  The caller
 * orders the prepass after the previous use of the workspace.  Up to 4 prepasses may be pending at once, each in
 * its own workspace (a frame pipeline keeps the ray-only stage of the next frames in flight); th_render_rays
 * consumes the one queued for ITS workspace.  Results are identical with or without it. */
int th_render_prepass(th_ctx* ctx, const th_frame* f, const th_points* rays, void* workspace,
                      size_t workspace_bytes, th_stream stream);
/* Optional second ahead-of-time stage, behind a th_render_prepass of the same workspace / ray arrays: the pixel-aligned
 * feature rows (get_pixel_aligned_feature, :210-269) and the 7-neighbour records of the human representation
 * (cross_transformer.py:151-205) of the first chunks of valid samples.  Neither needs the TransHE tokens on the
 * th_set_tok_gather(ctx, 1) path: `f` must be complete EXCEPT f->tokens, so a caller can run TransHE on another stream
 * beside this (texture-path-bound) stage instead of in front of it; the following th_render_rays (same workspace, same
 * map / token centres, complete frame) then only runs the fused MLP for those chunks.  Waits for the prepass's sample
 * count on the host.  A no-op (return 0) without a matching prepass or off the fused neighbour-record path; results are
 * identical with or without it. */
int th_render_pregather(th_ctx* ctx, const th_frame* f, const th_points* rays, void* workspace,
                        size_t workspace_bytes, void* shade_pool, size_t shade_pool_bytes, th_stream stream);
/* ABI 8.  Optional, behind a th_render_prepass of the same workspace / ray arrays and before its th_render_pregather: builds
 * the candidate grid of the 7-neighbour search (cross_transformer.py:151-160; exact pruning) for f->centres
 * into the workspace on `stream` -- a frame pipeline calls it on the stream that produced the centres (th_paint_group),
 * long before the pre-gather stage, which then starts with the neighbour search itself.  The caller orders `stream` before
 * the pre-gather stage (as for the prepass).  A no-op without a matching prepass; results are identical. */
int th_render_pregrid(th_ctx* ctx, const th_frame* f, const th_points* rays, void* workspace, size_t workspace_bytes,
                      th_stream stream);
/* ABI 9.  Optional, behind a th_render_prepass of the same workspace / ray arrays: marks, on `stream` (which is first ordered
 * behind the prepass), the map texels the prepass's valid samples read in the V views of f (f->cams, f->scale_xy, f->V, f->H,
 * f->W; the other fields as for th_render_prepass) and those the n_paint vertices of verts_paint read (NULL / 0: none -- e.g. a
 * rank that receives this frame's tokens) into `demand` (th_map_demand_bytes).  See th_upsample_concat_split_demand.  A frame
 * whose th_map_source.demand is this buffer is complete for exactly this prepass; returns 1 (and leaves `demand` untouched) without
 * a matching prepass. */
int th_render_predemand(th_ctx* ctx, const th_frame* f, const th_points* rays, void* workspace, size_t workspace_bytes,
                        const float* verts_paint, int n_paint, void* demand, size_t demand_bytes, th_stream stream);
/* ABI 8.  th_render_pregather for a frame pipeline that queues frame i+1's pre-gather stage right behind frame i's
 * th_render_rays on the same stream and shading pool: the neighbour-record producer (on the context's second stream) is
 * ordered behind the PER-SAMPLE stage of that th_render_rays -- the last user of the pool regions it writes -- instead of
 * behind everything queued on `stream` since, so frame i's compositing and whatever the caller queued after it (image
 * assembly, an all-gather) run beside the producer instead of in front of it.  The caller promises that everything the
 * stage reads -- the prepass of this workspace, `f` except f->tokens, the ray arrays -- was complete on `stream` BEFORE
 * that th_render_rays was queued (e.g. the stream waited on the event of the front that produced them); a non-NULL
 * f->tokens is taken as complete on `stream` now, and the per-frame token table is then queued here as well.  Without a
 * th_render_rays on the same stream and pool since the last pre-gather it behaves exactly as th_render_pregather;
 * `stream` has waited for the whole stage when the call returns, as there.  Results are identical. */
int th_render_pregather_early(th_ctx* ctx, const th_frame* f, const th_points* rays, void* workspace,
                              size_t workspace_bytes, void* shade_pool, size_t shade_pool_bytes, th_stream stream);
/* Waits (host) for the counts of the prepass pending in `workspace`: counts_host[0] = hit rays, [1] = 1 when the
 * R' <= small_frame_rays rule fired (un-masked branch), [2] = valid samples -- what th_shade_pool_bytes wants.
 * Returns 1 (and leaves counts_host alone) when no prepass is pending for that workspace. */
int th_render_prepass_wait(th_ctx* ctx, const void* workspace, int64_t* counts_host /* [3] */);
/* Drops a pending prepass (a caller that abandons the frame it was queued for must not let a later
 * th_render_rays that happens to reuse the same buffers pick it up). */
int th_render_prepass_cancel(th_ctx* ctx);                          /* all pending prepasses */
int th_render_prepass_drop(th_ctx* ctx, const void* workspace);     /* the one queued for this workspace */

/* if_mesh_renderer.Renderer.render :46-100 up to `cube`: sigma_raw per grid
 * point (0 outside the hull).  pts [P,3] world space. */
size_t th_sigma_grid_workspace_bytes(const th_frame* f, int P);
int th_eval_sigma_grid(th_ctx* ctx, const th_frame* f, const float* pts, int P, float* sigma_out,
                       void* workspace, size_t workspace_bytes, void* shade_pool, size_t shade_pool_bytes,
                       int64_t* stats_host, th_stream stream);
/* The radiance field at arbitrary points (additions, ABI 12): pts [P,3] world space, dirs [P,3] viewing directions (normalised
 * here; NULL: the zero embedding rows of if_mesh_renderer.py:62) -> raw_out [P,4] = {rgb logits, sigma_raw}.  Rows outside the
 * hull are exactly 0; inside, sigma everywhere and the RGB logits where sigma > 0 (0 elsewhere): what MLP_forward_ori's
 * progressive branch returns under the hull mask.  Workspace (th_sigma_grid_workspace_bytes), pool, statistics and range
 * snapshot as th_eval_sigma_grid. */
int th_eval_points(th_ctx* ctx, const th_frame* f, const float* pts, const float* dirs, int P, float* raw_out,
                   void* workspace, size_t workspace_bytes, void* shade_pool, size_t shade_pool_bytes,
                   int64_t* stats_host, th_stream stream);

/* ---- K22: the optimiser step -- value clipping + Adam / AdamW for every parameter tensor in one launch (additions, ABI 12) ---- */
/* What the reference's loop does per step with clip_grad_value_(., 40) and torch.optim.Adam over one parameter group per tensor
 * (lib/train/trainers/trainer.py:85-86, lib/train/optimizer.py:16-19), as ONE copy of a per-tensor table and ONE kernel.
 * All fp32, every operation rounded once, in this order (no FMA contraction; division and square root correctly rounded;
 * subnormals kept), per element of a tensor whose table entry is t:
 *     g  = clamp(g, -clip, clip)              with TH_ADAM_CLIP; a NaN stays NaN
 *     p  = p * t.decay_mul                    with TH_ADAM_T_DECOUPLED in t.flags (AdamW: decay_mul = fp32(1 - lr wd)), else
 *     g  = g + t.weight_decay * p             when t.weight_decay != 0
 *     m' = m + t.one_minus_beta1 * (g - m)
 *     v' = t.beta2 * v + (t.one_minus_beta2 * g) * g
 *     p' = p - t.step_size * (m' / (sqrt(v') / t.bc2_sqrt + t.eps))
 * with step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) computed by the caller in double precision and
 * rounded to fp32 once.  p, m, v are updated in place; TH_ADAM_ZERO_GRAD also writes 0 over g after reading it.  An entry whose
 * p is NULL is skipped (a parameter without a gradient this step).  Elementwise, no float atomics: two runs agree bit for bit.
 * TH_ADAM_COUNT_NONFINITE adds the number of NaN / +-inf gradient elements (before clipping) to a device word of the plan with
 * an integer atomic; it is read -- behind a stream synchronisation -- only by a call that passes nonfinite_out (the running
 * total since th_adam_plan), and such a call may pass n_tensors = 0 to read without stepping.
 *
 * th_adam_plan cuts the tensors (counts[i] fp32 elements each, contiguous) into chunks of th_adam_chunk_elems() elements, one
 * workgroup each, and uploads that chunk table into `table` (th_adam_table_bytes(n_tensors, sum of counts) bytes of device
 * memory, 16-byte aligned, owned by the caller and alive as long as the plan); `params` (optional) are checked to be device
 * pointers.  The call drains `stream`.  th_adam_step copies `scalars` (host memory, n_tensors entries, free for reuse on return)
 * through a ring of 16 pinned staging buffers of the plan into `table` and launches the kernel: two queue operations per step,
 * plus one event record every 8th step that tells the ring when a staging buffer may be rewritten.  128-bit accesses are used
 * for a tensor whose four pointers are 16-byte aligned, 32-bit ones otherwise.  TH_ADAM_CHECK_POINTERS asks the runtime about
 * every pointer of the step (a host pointer is refused with an error, not dereferenced); it costs ~1 us per pointer, so a
 * caller sets it when the pointers are new.  Data types and contiguity cannot be seen through a pointer: the Python binding
 * (transhuman_amd.hip.adam_step) refuses tensors that are not contiguous fp32 device tensors. */
#define TH_ADAM_CHUNK 4096
enum { TH_ADAM_CLIP = 1, TH_ADAM_ZERO_GRAD = 2, TH_ADAM_COUNT_NONFINITE = 4, TH_ADAM_CHECK_POINTERS = 8 };
enum { TH_ADAM_T_DECOUPLED = 1 };
typedef struct th_adam_tensor {
    void* p;               /* parameter, NULL: skip this tensor */
    void* g;               /* gradient */
    void* m;               /* exp_avg */
    void* v;               /* exp_avg_sq */
    float lr;              /* (informative: the kernel reads step_size and decay_mul) */
    float step_size;       /* lr / (1 - beta1^step) */
    float bc2_sqrt;        /* sqrt(1 - beta2^step) */
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
    float eps;
    float weight_decay;    /* coupled form; ignored with TH_ADAM_T_DECOUPLED */
    float decay_mul;       /* decoupled form: 1 - lr weight_decay */
    uint32_t flags;        /* TH_ADAM_T_* */
} th_adam_tensor;
typedef struct th_adam_plan_t th_adam_plan_t;
int    th_adam_chunk_elems(void);
size_t th_adam_table_bytes(int n_tensors, long long total_elems);      /* pure host call; 0 for sizes out of range */
int th_adam_plan(th_ctx* ctx, int n_tensors, const long long* counts, const void* const* params /* or NULL */, void* table,
                 size_t table_bytes, th_adam_plan_t** out, th_stream stream);
void th_adam_plan_destroy(th_adam_plan_t* plan);                         /* drains the device; `table` stays the caller's */
int th_adam_step(th_ctx* ctx, th_adam_plan_t* plan, const th_adam_tensor* scalars, int n_tensors, float clip, int flags,
                 unsigned long long* nonfinite_out /* or NULL */, th_stream stream);

/* ---- the gradient exchange of data-parallel training: every planned tensor into / out of ONE flat buffer (additions, ABI 12) ---- */
/* What DistributedDataParallel does with buckets and a copy per tensor, as one launch over the chunk table of a th_adam_plan_t
 * (one workgroup per chunk, 128-bit accesses where the flat buffer and the tensor are 16-byte aligned, 32-bit ones for tails and
 * unaligned tensors; no atomics, no LDS; two calls write identical bytes).  transhuman_amd/train_dist.py, DESIGN.md 4.
 *
 * The layout rule (th_adam_flat_layout, a pure host call): slots follow plan order and exist only for tensors whose byte in `live`
 * is non-zero (live NULL: every tensor); each slot starts at a multiple of 4 elements; the return value, flat_elems, is the end of
 * the last slot rounded up to 4 (0: no slot).  offsets_out[i] (optional) is the slot's first element, -1 without a slot.
 * -1 for a bad argument (n_tensors < 1, a count < 1).
 *
 * th_adam_pack: flat[offsets[i] + e] = grads[i][e] / (float)world for every tensor with a slot -- one correctly rounded fp32
 * division (subnormals kept, NaN and +-inf pass through); world == 1 copies the bits.  grads[i] NULL writes zeros (this rank has no
 * gradient for a tensor another rank has).  The padding behind a slot is written as zeros as well, so EVERY element of
 * flat[0 : flat_elems) is written by every call.  A tensor without a slot (offsets[i] < 0) is not touched.  grads[i] may BE
 * flat + offsets[i] (a gradient that already lives in its slot); any other overlap of a gradient with the flat buffer is undefined.
 * th_adam_unpack: dst[i][e] = flat[offsets[i] + e], bit for bit, for every tensor with a slot.
 *
 * `offsets` / `flat_elems` must be what th_adam_flat_layout gives for the plan's counts (checked on the host, so no slot can reach
 * past flat_elems), and flat[0 : flat_elems) must lie inside one device allocation (asked of the runtime
 * whenever a call names another buffer or length than the plan's last call; a repeated call costs no query).  The per-call pointers
 * and offsets travel through the plan's ring of pinned staging buffers like th_adam_step's table: one copy and one launch on
 * `stream`, no allocation, no synchronisation beyond the ring's own. */
long long th_adam_flat_layout(int n_tensors, const long long* counts, const uint8_t* live /* or NULL */, long long* offsets_out /* or NULL */);
int th_adam_pack(th_ctx* ctx, th_adam_plan_t* plan, const void* const* grads, const long long* offsets, int n_tensors, int world,
                 float* flat, long long flat_elems, th_stream stream);
int th_adam_unpack(th_ctx* ctx, th_adam_plan_t* plan, void* const* dst, const long long* offsets, int n_tensors, const float* flat,
                   long long flat_elems, th_stream stream);
/* K28, th_rank_sum: the sum of a reduce-scatter whose order this library owns (GradExchange(reduce="rank_ordered")).  parts
 * [world][slice_elems] is slice r of every rank's flat buffer as all_to_all_single delivers it to rank r;
 *   out[e] = ((parts[0][e] + parts[1][e]) + parts[2][e]) + ...     fp32, one rounding per addition, in rank order
 * (subnormals kept; NaN, +-inf and -0.0 as IEEE says; world == 1 copies the bits).  128-bit accesses when parts and out are 16-byte
 * aligned and slice_elems is a multiple of 4, 32-bit ones otherwise; no atomics, no LDS; two calls write identical bytes.  `out` may
 * be parts + r * slice_elems for any r (an element is read from every part and then written by one lane); any other overlap is
 * undefined.  Refused: world outside 1 .. 64, slice_elems < 1, null or misaligned (4-byte) pointers. */
int th_rank_sum(th_ctx* ctx, const float* parts, int world, long long slice_elems, float* out, th_stream stream);

/* ---- K23: the backward of the encoder trunk in training (additions, ABI 12) ---- */
/* The sites of SpatialEncoder.trunk (encoder.py:114-126: conv1 / bn1 / relu, the 3x3 / 2 max pool, layer1, layer2), backward only: the
 * forward stays the stock torch modules.  All tensors NCHW fp32, contiguous; H and W are the INPUT size of the convolution or the
 * pool, its output is Ho = (H + 2 (ks / 2) - ks) / stride + 1 rows.  No atomics, every sum in a fixed order: two runs agree bit
 * for bit.  Matrix work runs on the fp32-input MFMA, no reduced-precision operand and no range guard.  DESIGN.md 4, K23.
 *
 * th_conv2d_bwd_supported: 0, or bit 0 (1): th_conv2d_wgrad is built for this convolution, bit 1 (2): th_conv2d_dgrad as well.
 * Built: 3x3/1 64->64, 3x3/1 128->128, 3x3/2 64->128, 1x1/2 64->128 (both), 7x7/2 3->64 (weight gradient only).
 *
 * th_bn_act_bwd: train-mode BatchNorm (batch statistics, biased variance) followed by an optional residual add and an optional
 * ReLU.  y: the BatchNorm's input; out: the site's output, read for the gate [out > 0] (NULL: no ReLU); g: the gradient of the
 * site's output; gamma NULL: 1.  g_y: the gradient of y; g_res (optional): the gated gradient, which is the residual's; g_gamma /
 * g_beta [C] (optional).  Statistics and sums are fp64 (th_bn_act_bwd_slice_elems: the least slice of a channel one workgroup sums).
 * The statistics are those of the call's own batch: a SyncBatchNorm site, whose statistics are those of all ranks, takes the split
 * pair th_bn_act_bwd_sums / th_bn_act_bwd_apply declared below, which is this function bit for bit with one rank.
 *
 * th_conv2d_dgrad: g_y [N, cout, Ho, Wo] -> g_x [N, cin, H, W], every element written, from an image of the weights that
 * th_conv2d_dgrad_pack writes into caller-owned memory (th_conv2d_dgrad_pack_bytes, 16-byte aligned; pack again when the weights
 * change).  A workgroup owns th_conv2d_dgrad_tile_rows x th_conv2d_dgrad_tile_cols input pixels of one parity class.
 *
 * th_conv2d_wgrad: x [N, cin, H, W], g_y -> g_w [cout, cin, ks, ks].  The output pixels are cut into chunks of
 * th_conv2d_wgrad_chunk_pixels; each chunk's partial is a fresh MFMA chain, the chunks are added in chunk order (fp64, one rounding).
 *
 * th_maxpool3x3s2_bwd: x [planes, H, W] (the pool's input), g [planes, Ho, Wo] -> g_x; a window's gradient goes to the element
 * torch's forward records (the last one, kh outer / kw inner, with val > max || isnan(val)); the padding never wins. */
int    th_conv2d_bwd_supported(int cin, int cout, int ks, int stride);
int    th_conv2d_wgrad_chunk_pixels(void);
int    th_conv2d_dgrad_tile_rows(void);
int    th_conv2d_dgrad_tile_cols(void);
int    th_bn_act_bwd_slice_elems(void);
size_t th_bn_act_bwd_workspace_bytes(int N, int C, int HW);                                    /* pure host call; 0: unsupported */
int th_bn_act_bwd(th_ctx* ctx, const float* y, const float* out_or_null, const float* g, int N, int C, int HW,
                  const float* gamma_or_null, double eps, float* g_y, float* g_res_or_null, float* g_gamma_or_null,
                  float* g_beta_or_null, void* workspace, size_t workspace_bytes, th_stream stream);
/* The same backward for a SyncBatchNorm site (statistics of all ranks), split around the caller's collective (additions, ABI 12):
 * th_bn_act_bwd_sums: pass A over this rank's N images and the fixed-order sum of its slices -> record [C][6] fp64 on the device:
 * a0 a1 a2 a3 against the rank's own pivot p = y[0, c, 0, 0], then p and L = N HW.  The workspace is th_bn_act_bwd_workspace_bytes.
 * The caller gathers the ranks' records in rank order (one all_gather of C * 48 bytes).
 * th_bn_act_bwd_apply: records [world][C][6] -> the global sums, added over the ranks in rank order with d_r = p_r - p_0:
 *   A0 = sum (a0_r + L_r d_r), A1 = sum ((a1_r + (2 d_r) a0_r) + (L_r d_r) d_r), A2 = sum a2_r, A3 = sum (a3_r + d_r a2_r), L = sum L_r
 * then m, var, invstd, mg, mx, k as th_bn_act_bwd from A0..A3 and L, xhat = ((y - p_r) - (m - d_r)) invstd per element, and g_y, g_res
 * as th_bn_act_bwd.  g_beta = fp32(a2_r) and g_gamma = fp32((a3_r - (m - d_r) a2_r) invstd) are this rank's LOCAL sums (torch's
 * SyncBatchNorm returns the same; the gradient exchange averages them).  y, out, g, N are this rank's; world = 1, rank = 0 is
 * th_bn_act_bwd bit for bit.  No atomics, no wait on the host: DESIGN.md 4, K23. */
int th_bn_act_bwd_sums(th_ctx* ctx, const float* y, const float* out_or_null, const float* g, int N, int C, int HW,
                       double* record /* [C][6]: a0 a1 a2 a3 p L */, void* workspace, size_t workspace_bytes, th_stream stream);
int th_bn_act_bwd_apply(th_ctx* ctx, const float* y, const float* out_or_null, const float* g, int N, int C, int HW,
                        const float* gamma_or_null, double eps, const double* records /* [world][C][6] */, int world, int rank,
                        float* g_y, float* g_res_or_null, float* g_gamma_or_null, float* g_beta_or_null, th_stream stream);
int th_maxpool3x3s2_bwd(th_ctx* ctx, const float* x, const float* g, int planes, int H, int W, float* g_x, th_stream stream);
size_t th_conv2d_dgrad_pack_bytes(int cin, int cout, int ks, int stride);                     /* pure host call; 0: unsupported */
int th_conv2d_dgrad_pack(th_ctx* ctx, const float* w, int cin, int cout, int ks, int stride, void* packed, size_t packed_bytes,
                         th_stream stream);
int th_conv2d_dgrad(th_ctx* ctx, const float* g_y, int N, int cin, int cout, int ks, int stride, int H, int W, const void* packed,
                    size_t packed_bytes, float* g_x, th_stream stream);
size_t th_conv2d_wgrad_workspace_bytes(int N, int cin, int cout, int ks, int stride, int H, int W);   /* pure host call */
int th_conv2d_wgrad(th_ctx* ctx, const float* x, const float* g_y, int N, int cin, int cout, int ks, int stride, int H, int W,
                    float* g_w, void* workspace, size_t workspace_bytes, th_stream stream);

/* ---- K29: the forward convolutions of the encoder trunk in training (additions, ABI 12) ---- */
/* nn.Conv2d(cin, cout, ks, stride, ks / 2, bias=False), x [N, cin, H, W] -> y [N, cout, Ho, Wo], NCHW fp32 contiguous, Ho = (H + 2 (ks / 2)
 * - ks) / stride + 1, for the trunk's five shapes: 7x7/2 3->64, 3x3/1 64->64, 3x3/2 64->128, 1x1/2 64->128, 3x3/1 128->128
 * (th_conv2d_fwd32_supported: 1 for these, 0 otherwise).  An implicit GEMM on the fp32-input MFMA: no reduced-precision operand, no
 * range guard (th_conv2d, the inference stem's fp16-split convolution, is another function and stays what it is).  w is torch's layout
 * [cout][cin][ks][ks], read directly: nothing is packed or cached, there is no workspace.  A workgroup owns th_conv2d_fwd32_tile_rows x
 * th_conv2d_fwd32_tile_cols output pixels x 64 output channels of one image.  The reduction is cut into chunks of
 * th_conv2d_fwd32_chunk_channels input channels; a chunk is a fresh MFMA chain (taps kh outer, kw inner, channel pairs ascending; 7x7:
 * one chain per kernel row, channels outer, tap pairs inner, the eighth tap a zero on both operands), the chains are added in order in
 * fp64 and rounded to fp32 once.  No atomics; every output element is stored once and y is never read: two calls write identical
 * bytes.  Refused with a negative status and th_last_error: another shape, a null pointer, N outside 1 .. 16383, H or W < 1, 2^31 or
 * more elements in x or y.  DESIGN.md 4, K29. */
int th_conv2d_fwd32_supported(int cin, int cout, int ks, int stride);                          /* pure host call */
int th_conv2d_fwd32_tile_rows(void);
int th_conv2d_fwd32_tile_cols(void);
int th_conv2d_fwd32_chunk_channels(void);
int th_conv2d_fwd32(th_ctx* ctx, const float* x, int N, int cin, int H, int W, const float* w, int cout, int ks, int stride,
                    float* y, th_stream stream);

/* ---- K26: the dataset's other targets -- sample_ray_h36m, both splits, and get_acc (additions, ABI 12) ---------------- */
/* sample_ray_h36m (lib/utils/if_nerf/if_nerf_data_utils.py:516-614) and get_acc (:635-641), which the reference's dataset runs in
 * numpy for every test / evaluation batch and for the training batch without patch sampling (can_smpl.py:518-535), on the dense
 * per-pixel arrays of th_gen_rays.  All pointers are DEVICE pointers; ray_o, ray_d, near, far, ray_mask, msk, bound_mask and img
 * with its two strides are th_patch_rays' inputs.
 * m = msk * bound_mask in uint8; body = (m == 1), face = (m == 13), rand_set = (bound_mask == 1) & (m != 100).
 * th_ray_sample_train: draws fp64 [4][3][nrays] in [0, 1).  n = 0; while n < nrays: rem = nrays - n, n_body = (int)(rem body_ratio),
 * n_face = (int)(rem face_ratio) (fp64 products), n_rand = rem - n_body - n_face; the candidates of iteration i are, in this
 * order, n_body body pixels (an empty body class: the ONE pixel (1,1)), n_face face pixels (an empty face class: none), n_rand
 * rand_set pixels (an empty rand_set: the ONE pixel (0,0)); pick j of class c (0 body, 1 face, 2 rand) is the class's k-th pixel
 * in row-major order, k = min(floor(draws[i][c][j] n_c), n_c - 1); the candidates whose ray_mask holds are appended in order and
 * n grows by their number, so the final count can be nrays + 1.  Rows (allocated at nrays + 4): out_rgb, out_ray_o, out_ray_d
 * fp32 [.][3], out_near, out_far fp32 [.], out_coord int64 [.][2] = (row, col).  info int32 [4] = the ray count, the iterations
 * used, status bits (1: an iteration added nothing, 2: unfinished after 4 iterations, 4: a negative class count) and the last
 * iteration's candidate count; the rows below info[0] are written, nothing else is.  One workgroup runs the whole loop: no host
 * read between iterations.
 * th_ray_sample_test: the rows of the five dense arrays and the image where ray_mask holds, in row-major order (rows allocated at
 * H W); info[0] = their count, info[1..3] = 0.
 * th_ray_acc: coord int64 [n][2] = (row, col); acc uint8 [n] = 1 where any pixel of msk [H][W] is nonzero in the 25 x 25 window
 * centred on the coordinate and clipped to the image (cv2.dilate with a 25 x 25 kernel of ones, read at the coordinate).
 * No atomics: bit-identical from run to run.  No host wait; nothing is allocated.  Limits (argument errors before any launch):
 * 1 <= H, W <= 4096 (train: 2 <= H, W), 1 <= nrays <= 65536, 0 <= body_ratio, face_ratio, body_ratio + face_ratio <= 1; the
 * workspace at least th_ray_sample_workspace_bytes(H, W, nrays) (nrays is not read by the test split: pass 0; 0 bytes for sizes out
 * of range). */
size_t th_ray_sample_workspace_bytes(int H, int W, int nrays);
int th_ray_sample_train(th_ctx* ctx, const float* ray_o, const float* ray_d, const float* near, const float* far,
                        const uint8_t* ray_mask, const uint8_t* msk, const uint8_t* bound_mask, const float* img,
                        long long pix_stride, long long chan_stride, int H, int W, const double* draws, int nrays, double body_ratio,
                        double face_ratio, float* out_rgb, float* out_ray_o, float* out_ray_d, float* out_near, float* out_far,
                        int64_t* out_coord, int32_t* info, void* workspace, size_t workspace_bytes, th_stream stream);
int th_ray_sample_test(th_ctx* ctx, const float* ray_o, const float* ray_d, const float* near, const float* far,
                       const uint8_t* ray_mask, const float* img, long long pix_stride, long long chan_stride, int H, int W,
                       float* out_rgb, float* out_ray_o, float* out_ray_d, float* out_near, float* out_far, int32_t* info,
                       void* workspace, size_t workspace_bytes, th_stream stream);
int th_ray_acc(th_ctx* ctx, const int64_t* coord, int n, const uint8_t* msk, int H, int W, uint8_t* acc, th_stream stream);

/* ---- K27: cfg.use_truncation -- skip the samples far from every token centre (additions, ABI 12) ---------------------- */
/* Network.get_human_representation's mask_preserve = knn_dist.min(-1) < cfg.KNN_SIGMA (cross_transformer.py:175-180) and what
 * Network.forward does with it (:247-264): the per-point network runs on the preserved samples, raw = 0 for the others.
 * A sample is kept when sqrtf(d2min) < (float)sigma, d2min = the squared distance to its nearest centre by K4's own
 * expression -- bit for bit the distance of K4's first neighbour -- over K4's candidate grid where the grid builder takes
 * these centres (7 <= nc <= 4096, TH_DPARF_NOGRID unset), else over all of them: the same result.  A NaN distance drops.
 * All pointers are DEVICE pointers.
 * th_truncate_select: pts_smpl [P,3], centres [nc,3] (nc >= 1) -> mask uint8 [P] (1 = kept), sel int32 (allocated at P): the
 * kept indices, ascending, in sel[0 .. count), and count int32 [1].  No host wait: the caller reads count.  An ordered
 * compaction in three launches (+ two for the grid): no atomics, no workgroup waits for another, every output element is stored
 * once, nothing is cleared and nothing in the outputs or the workspace is read before it is written -- bit-identical from
 * run to run whatever the buffers held.  P = 0 writes count = 0.
 * th_truncate_scatter: rows_kept [n_kept,C] -> rows [P,C]: rows[sel[j]] = rows_kept[j], exact zeros in the rows with mask 0,
 * every element stored once; mask and sel[0 .. n_kept) as th_truncate_select left them.  th_truncate_scatter_bwd, its adjoint:
 * g_rows_kept[j] = g_rows[sel[j]].  C must be 4.
 * th_set_truncation: sigma > 0 switches the same rule on for th_render_rays, th_eval_sigma_grid and th_eval_points: behind the
 * shading and in front of compositing / extraction one more launch zeroes the dense raw rows of the hull-valid samples
 * whose nearest centre is sigma or farther away -- the reference's raw = 0.  The hull mask, the ray compaction and the
 * R' <= small_frame_rays rule are untouched.  sigma <= 0 (the default of a new context): off, no launch and no byte differs. */
int th_set_truncation(th_ctx* ctx, double sigma);
size_t th_truncate_select_workspace_bytes(int P, int nc);                                       /* pure host call */
int th_truncate_select(th_ctx* ctx, const float* pts_smpl, int P, const float* centres, int nc, double sigma, uint8_t* mask,
                       int32_t* sel, int32_t* count, void* workspace, size_t workspace_bytes, th_stream stream);
int th_truncate_scatter(th_ctx* ctx, const float* rows_kept, const uint8_t* mask, const int32_t* sel, int n_kept, int P, int C,
                        float* rows, th_stream stream);
int th_truncate_scatter_bwd(th_ctx* ctx, const float* g_rows, const int32_t* sel, int n_kept, int P, int C, float* g_rows_kept,
                            th_stream stream);

/* ---- DPaRF's hyper-parameters: cfg.KNN, cfg.KNN_FREQ, cfg.KNN_DIST_ALPHA (addition, ABI 12) ---------------------------- */
/* th_set_dparf: the number of neighbouring tokens (cross_transformer.py:170), the octave count of the local positional
 * encoding (:106) and the softmax temperature of the distances (:154) of EVERY entry of this context that runs K4 or its
 * backward: th_dparf_encode, th_dparf_encode_bwd, th_network_forward, th_render_rays, th_render_pregather, th_eval_sigma_grid,
 * th_eval_points.  A new context has (7, 10, 0.5).  knn 1..7 (a neighbour record holds seven (index, weight) pairs), n_freq
 * 1..10 (3 + 6 n_freq <= 63 PE channels inside fc_0's 256 padded columns; 0 octaves are not supported), alpha finite
 * and > 0, rounded to fp32 once; anything else is an error that names the values.  Fewer than knn token centres is an error of
 * the entry that runs K4.  w = softmax((-sqrt(d2)) / alpha), a true fp32 division.  Columns 195 + 6 n_freq .. 255 of an fp32
 * row are exact zero.  th_set_mlp_weights takes fc_0 of 256 x (195 + 6 n_freq) of the n_freq in force; changing n_freq
 * invalidates the uploaded MLP weights (upload again).  Workspace sizes do not depend on these values. */
int th_set_dparf(th_ctx* ctx, int knn, int n_freq, double alpha);

#ifdef __cplusplus
}
#endif
#endif /* TRANSHUMAN_HIP_H */
