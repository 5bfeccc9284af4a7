// LPIPS (VGG16, version 0.1, lpips=True, spatial=False, eval mode) of the evaluator (lib/evaluators/if_nerf.py:110-117,
// third_parties/lpips/lpips.py:81-124):
//   ScalingLayer (x - shift) / scale, VGG16 features[0:30] (13 conv3x3 s1 p1 + bias + ReLU, 4 max pools 2x2 s2 floor),
//   taps relu1_2 / relu2_2 / relu3_3 / relu4_3 / relu5_3, per tap and pixel normalize_tensor (x / (sqrt(sum_c x^2 + 1e-10)
//   + 1e-10)) of both images, (f0 - f1)^2, the 1x1 lin_k dot to one channel, the spatial mean; the result is the sum of
//   the five tap values.
//
// Numerics: the convolutions run on the fp32-input MFMA (v_mfma_f32_32x32x2_f32), bit for bit a k-ordered fp32 fmaf chain,
// so there is no reduced-precision operand anywhere and no range guard.  The head (normalisation, difference, lin dot,
// spatial mean, tap sum) is fp64 on the fp32 features.  Both images of a call go through the same launches (the batch is
// grid.z: images 0..N-1 are in0, N..2N-1 are in1), so lpips(a, a) is exactly 0.  No atomics: the per-workgroup partials are
// added in a fixed order by one workgroup, so the result is bit-identical from run to run.
//
// Activations between the launches are NHWC fp32 in the caller's workspace (two ping-pong buffers of 2N x 64 x H x W).
//
// lp_conv_kernel: implicit GEMM, M = pixels of an 8 x 16 output tile, N = 64 output channels, K = 9 x CIN taken in chunks
// of 8 input channels.  Per chunk the tile's 10 x 18 halo of 8 channels is staged in LDS as [c][row][col] and the chunk's
// packed weights as [k = tap * 8 + c][64]; wave w owns output rows 2w, 2w + 1 (32 pixels) x 64 channels: two 32 x 32
// accumulators, 36 k-steps of two MFMAs per chunk.  Each chunk's 72 products are a fresh MFMA chain added to a running fp32
// sum: one 4608-long fma chain (CIN 512) was 5-10x less accurate at the deep taps than torch's fp32 CPU convolution.
// The first layer (CIN 3) is one zero-padded chunk read from the NCHW input with the ScalingLayer applied in the staging.
//
// Training form (K21): th_lpips_train makes the same launches into a caller-owned state buffer that keeps what the backward reads:
// the post-ReLU output of all 13 layers of the in0 images and the five taps of the in1 images (a tap is one [2N] array, in0's
// images first).  The batch stays one grid.z: the convolutions' SPLIT form sends in1's other layers through two scratch
// buffers behind the kept part, where the pooled maps and the head's partials pass through as well.  th_lpips_bwd walks from the deepest level to the first and gives d total / d in0:
//   per level   lp_head_bwd_kernel   fp64 derivative of the tap's head at the stored fp32 features, rounded to fp32, added to
//                                    the gradient arriving from the deeper level, gated by [y > 0] of the tap
//   per layer   lp_conv_kernel<false, LP_EPI_DGRAD / LP_EPI_IMAGE>   the input gradient of a 3x3 / s1 / p1 convolution is the
//                                    same convolution with the taps rotated by 180 degrees and the channel roles swapped: the
//                                    forward's tile on a second packed image (lp_pack_bwd_kernel), the same per-chunk fresh MFMA
//                                    chains summed in fp32; no bias, no ReLU, the gate [y > 0] of the layer below in the
//                                    epilogue; layer 0: 3 channels, 1 / scale[c] of the ScalingLayer, NCHW
//   per pool    lp_pool_bwd_kernel   the gradient goes to the first element of the window (row-major) that equals its maximum,
//                                    torch's rule; rows / columns the floor cropped get 0
// Gradients are NHWC fp32 in two ping-pong buffers of N x 64 x H x W.  No atomics: bit-identical from run to run.
#include "th_internal.h"

#include <math.h>

namespace {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_TW = 16, LP_TH = 8;             // output tile: 16 columns x 8 rows = 128 pixels
constexpr int LP_HW = LP_TW + 2, LP_HH = LP_TH + 2;
constexpr int LP_CK = 8;                         // input channels per staged chunk
constexpr int LP_KC = 9 * LP_CK;                 // k per chunk
constexpr int LP_NB = 64;                        // output channels per workgroup
constexpr int LP_THREADS = 256;
constexpr int LP_HEAD_THREADS = 256;
constexpr int LP_HEAD_LANES = 8;                 // lanes per pixel in the head
constexpr int LP_HEAD_PIX = LP_HEAD_THREADS / LP_HEAD_LANES;
constexpr int LP_FIN_THREADS = 256;
constexpr int LP_NL = 13;
constexpr int LP_CMAX = 512;

constexpr int LP_CIN[LP_NL] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_NL] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_LEVEL_LAST[5] = {1, 3, 6, 9, 12};   // the layer whose ReLU output is the tap of each level
constexpr int LP_TAP_C[5] = {64, 128, 256, 512, 512};

// ScalingLayer buffers (lpips.py:126-133), fp32 like the module's
__constant__ float lp_shift[3] = {-.030f, -.088f, -.188f};
__constant__ float lp_scale[3] = {.458f, .448f, .450f};

__host__ __device__ constexpr int lp_cin_pad(int l) { return (LP_CIN[l] + LP_CK - 1) / LP_CK * LP_CK; }
size_t lp_wfloats(int l) { return (size_t)LP_COUT[l] * lp_cin_pad(l) * 9; }

// packed image: the 13 weight blocks, then bias [13][512], then lin [5][512] (floats)
size_t lp_woff(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += lp_wfloats(i);
    return o;
}
size_t lp_bias_off() { return lp_woff(LP_NL); }
size_t lp_lin_off() { return lp_bias_off() + (size_t)LP_NL * LP_CMAX; }
size_t lp_pack_floats() { return lp_lin_off() + (size_t)5 * LP_CMAX; }

// packed weights of one layer: [COUT / 64][CIN_pad / 8][k = tap * 8 + c][64], value W[co][ci][tap / 3][tap % 3], zero for
// ci >= CIN.  w: torch layout [COUT][CIN][3][3].
__global__ void lp_pack_kernel(const float* __restrict__ w, int CIN, int COUT, int nch, float* __restrict__ out) {
    const long long total = (long long)COUT * nch * LP_KC;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % LP_NB);
    const int k = (int)((idx / LP_NB) % LP_KC);
    const int ch = (int)((idx / (LP_NB * LP_KC)) % nch);
    const int cob = (int)(idx / ((long long)LP_NB * LP_KC * nch));
    const int tap = k / LP_CK, ci = ch * LP_CK + k % LP_CK, co = cob * LP_NB + j;
    out[idx] = ci < CIN ? w[((long long)co * CIN + ci) * 9 + tap] : 0.f;
}

// 3x3 / stride 1 / pad 1 convolution + bias + ReLU.  FIRST: the input is NCHW with 3 channels, images z < nsplit from `a`,
// the others from `b` (image z - nsplit), with the ScalingLayer applied; otherwise the input is NHWC [z][H][W][CIN] at `a`.
// Output NHWC [z][H][W][COUT].  grid: (tiles, COUT / 64, 2N).
// EPI (the input-gradient forms, on the image of lp_pack_bwd_kernel; CIN / COUT are then the forward layer's COUT / CIN):
//   LP_EPI_DGRAD  no bias, no ReLU; `bias` is the gate source: the stored output y of the layer below, NHWC like `out`, the
//                 result is 0 where y <= 0 (null: no gate, the layer below is a pool)
//   LP_EPI_IMAGE  layer 0: channels 0..2 of the block times 1 / scale[c], written NCHW [z][3][H][W]
// SPLIT (the training form of the forward, which keeps in0's layers and lets in1's pass through scratch): the images z >= nsplit
//   live in arrays of their own, indexed from z - nsplit: the input at `b` (as the first layer's always does), the output at `out2`
enum { LP_EPI_FORWARD = 0, LP_EPI_DGRAD = 1, LP_EPI_IMAGE = 2 };
template <bool FIRST, int EPI = LP_EPI_FORWARD, bool SPLIT = false>
__global__ __launch_bounds__(LP_THREADS) void lp_conv_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             int nsplit, int H, int W, int CIN, int COUT,
                                                             const float* __restrict__ wpk, const float* __restrict__ bias,
                                                             float* __restrict__ out, int tiles_x, float* __restrict__ out2) {
    __shared__ float sIn[LP_CK][LP_HH][LP_HW];
    __shared__ __attribute__((aligned(16))) float sW[LP_KC][LP_NB];

    const int tid = threadIdx.x, lane = tid % TH_WAVE, wave = tid / TH_WAVE;
    const int cob = blockIdx.y, z = blockIdx.z;
    if (SPLIT && z >= nsplit) {                              // rebase, so that a + z * ... and out + z * ... below address them
        if (!FIRST) a = b - (size_t)nsplit * H * W * CIN;
        out = out2 - (size_t)nsplit * H * W * COUT;
    }
    const int y0 = (blockIdx.x / tiles_x) * LP_TH, x0 = (blockIdx.x % tiles_x) * LP_TW;
    const int nch = FIRST ? 1 : CIN / LP_CK;
    const int i_pix = lane & 31, hk = lane >> 5;            // A row (pixel) and k half of this lane
    const int py = 2 * wave + (i_pix >> 4), px = i_pix & 15;

    lp_f32x16 tot0, tot1;                                    // sums of the chunks' products
    for (int r = 0; r < 16; ++r) tot0[r] = tot1[r] = 0.f;

    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();                             // previous chunk fully consumed
        // weights: 72 x 64 contiguous floats
        const float4* wsrc = (const float4*)(wpk + ((size_t)cob * nch + ch) * (LP_KC * LP_NB));
        for (int i = tid; i < LP_KC * LP_NB / 4; i += LP_THREADS) ((float4*)&sW[0][0])[i] = wsrc[i];
        // input halo
        if (FIRST) {
            const float* src = z < nsplit ? a + (size_t)z * 3 * H * W : b + (size_t)(z - nsplit) * 3 * H * W;
            for (int i = tid; i < LP_CK * LP_HH * LP_HW; i += LP_THREADS) {
                const int c = i / (LP_HH * LP_HW), r = (i / LP_HW) % LP_HH, col = i % LP_HW;
                const int gy = y0 - 1 + r, gx = x0 - 1 + col;
                float v = 0.f;
                if (c < 3 && gy >= 0 && gy < H && gx >= 0 && gx < W)
                    v = (src[((size_t)c * H + gy) * W + gx] - lp_shift[c]) / lp_scale[c];
                sIn[c][r][col] = v;
            }
        } else {
            const float* src = a + (size_t)z * H * W * CIN + ch * LP_CK;
            for (int i = tid; i < LP_HH * LP_HW * 2; i += LP_THREADS) {
                const int p = i >> 1, hf = i & 1;
                const int r = p / LP_HW, col = p % LP_HW;
                const int gy = y0 - 1 + r, gx = x0 - 1 + col;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                    v = *(const float4*)(src + ((size_t)gy * W + gx) * CIN + 4 * hf);
                sIn[4 * hf + 0][r][col] = v.x;
                sIn[4 * hf + 1][r][col] = v.y;
                sIn[4 * hf + 2][r][col] = v.z;
                sIn[4 * hf + 3][r][col] = v.w;
            }
        }
        __syncthreads();
        lp_f32x16 acc0, acc1;                                // this chunk's 72 products (a fresh fma chain)
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
        for (int s = 0; s < LP_KC / 2; ++s) {
            const int tap = (2 * s) / LP_CK, c = (2 * s) % LP_CK + hk;
            const float av = sIn[c][py + tap / 3][px + tap % 3];
            const float b0 = sW[2 * s + hk][i_pix], b1 = sW[2 * s + hk][32 + i_pix];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
        }
        tot0 += acc0;
        tot1 += acc1;
    }

    // epilogue: lane holds output channels co0 = cob * 64 + (lane & 31) and co0 + 32 for 16 pixels
    // (C/D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    const int co0 = cob * LP_NB + i_pix;
    if (EPI == LP_EPI_DGRAD) {
        float* dst = out + (size_t)z * H * W * COUT;
        const float* gate = bias ? bias + (size_t)z * H * W * COUT : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hk;
            const int gy = y0 + 2 * wave + (i >> 4), gx = x0 + (i & 15);
            if (gy < H && gx < W) {
                const size_t o = ((size_t)gy * W + gx) * COUT + co0;
                const bool on0 = gate ? gate[o] > 0.f : true, on1 = gate ? gate[o + 32] > 0.f : true;
                dst[o] = on0 ? tot0[r] : 0.f;
                dst[o + 32] = on1 ? tot1[r] : 0.f;
            }
        }
        return;
    }
    if (EPI == LP_EPI_IMAGE) {
        if (co0 < 3) {                                       // (cob == 0: the three image channels of the zero-padded block)
            float* dst = out + ((size_t)z * 3 + co0) * H * W;
            const float sc = lp_scale[co0];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * hk;
                const int gy = y0 + 2 * wave + (i >> 4), gx = x0 + (i & 15);
                if (gy < H && gx < W) dst[(size_t)gy * W + gx] = tot0[r] / sc;
            }
        }
        return;
    }
    const float bb0 = bias[co0], bb1 = bias[co0 + 32];
    float* dst = out + (size_t)z * H * W * COUT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hk;
        const int gy = y0 + 2 * wave + (i >> 4), gx = x0 + (i & 15);
        if (gy < H && gx < W) {
            float* o = dst + ((size_t)gy * W + gx) * COUT + co0;
            o[0] = fmaxf(tot0[r] + bb0, 0.f);
            o[32] = fmaxf(tot1[r] + bb1, 0.f);
        }
    }
}

// 2 x 2 / stride 2 max pool (floor), NHWC, 4 channels per thread
__global__ void lp_pool_kernel(const float* __restrict__ in, int Z, int H, int W, int C, float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const long long total = (long long)Z * Ho * Wo * C4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const long long p = idx / C4;
    const int xo = (int)(p % Wo), yo = (int)((p / Wo) % Ho), z = (int)(p / ((long long)Wo * Ho));
    const float4* s = (const float4*)(in + (size_t)z * H * W * C) + c4;
    const float4 v0 = s[((size_t)(2 * yo) * W + 2 * xo) * C4], v1 = s[((size_t)(2 * yo) * W + 2 * xo + 1) * C4];
    const float4 v2 = s[((size_t)(2 * yo + 1) * W + 2 * xo) * C4], v3 = s[((size_t)(2 * yo + 1) * W + 2 * xo + 1) * C4];
    float4 m;
    m.x = fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x));
    m.y = fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y));
    m.z = fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z));
    m.w = fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w));
    ((float4*)out)[idx] = m;
}

// fixed-order workgroup sum of one double per thread (every thread gets the result)
template <int NT>
__device__ double lp_block_sum(double v, double* red) {
    for (int o = TH_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, TH_WAVE);
    const int lane = threadIdx.x % TH_WAVE, wave = threadIdx.x / TH_WAVE;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NT / TH_WAVE; ++w) s += red[w];
    __syncthreads();
    return s;
}

__device__ double lp_group_sum(double v) {       // sum over the LP_HEAD_LANES lanes of a pixel, the same in each of them
    for (int o = 1; o < LP_HEAD_LANES; o <<= 1) v += __shfl_xor(v, o, TH_WAVE);
    return v;
}

// one tap: per pixel of image n, d = sum_c lin[c] (f0[c] / n0 - f1[c] / n1)^2 with nk = sqrt(sum_c fk[c]^2 + 1e-10) + 1e-10,
// in fp64.  f: NHWC [2N][hw][C] (image n and N + n).  8 lanes per pixel, each reading 4 channels of every 32.
// partial[n * gridDim.x + block] = the workgroup's sum of d.  grid: (cdiv(hw, 32), N).
__global__ __launch_bounds__(LP_HEAD_THREADS) void lp_head_kernel(const float* __restrict__ f, int N, int hw, int C,
                                                                  const float* __restrict__ lin,
                                                                  double* __restrict__ partial) {
    __shared__ double red[LP_HEAD_THREADS / TH_WAVE];
    const int n = blockIdx.y, sub = threadIdx.x % LP_HEAD_LANES;
    const int p = blockIdx.x * LP_HEAD_PIX + threadIdx.x / LP_HEAD_LANES;
    double d = 0.0;
    if (p < hw) {
        const float* f0 = f + ((size_t)n * hw + p) * C;
        const float* f1 = f + ((size_t)(N + n) * hw + p) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = 4 * sub; c < C; c += 4 * LP_HEAD_LANES) {
            const float4 u = *(const float4*)(f0 + c), v = *(const float4*)(f1 + c);
            s0 += (double)u.x * u.x + (double)u.y * u.y + (double)u.z * u.z + (double)u.w * u.w;
            s1 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
        s0 = lp_group_sum(s0);
        s1 = lp_group_sum(s1);
        const double n0 = sqrt(s0 + 1e-10) + 1e-10, n1 = sqrt(s1 + 1e-10) + 1e-10;
        for (int c = 4 * sub; c < C; c += 4 * LP_HEAD_LANES) {
            const float4 u = *(const float4*)(f0 + c), v = *(const float4*)(f1 + c);
            const float4 w = *(const float4*)(lin + c);
            double q;
            q = (double)u.x / n0 - (double)v.x / n1; d += (double)w.x * (q * q);
            q = (double)u.y / n0 - (double)v.y / n1; d += (double)w.y * (q * q);
            q = (double)u.z / n0 - (double)v.z / n1; d += (double)w.z * (q * q);
            q = (double)u.w / n0 - (double)v.w / n1; d += (double)w.w * (q * q);
        }
        d = lp_group_sum(d);
        if (sub) d = 0.0;                                    // count each pixel once
    }
    const double s = lp_block_sum<LP_HEAD_THREADS>(d, red);
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = s;
}

struct LpTaps {
    long long off[5];    // partial offsets (doubles) of each tap
    int nblk[5];         // workgroups per image of each tap
    double count[5];     // h_k * w_k
};

// out[n][k] = (sum of tap k's partials of image n) / (h_k w_k), out[n][5] = the sum of the five in tap order
__global__ __launch_bounds__(LP_FIN_THREADS) void lp_finish_kernel(const double* __restrict__ partial, LpTaps t, int N,
                                                                   double* __restrict__ out) {
    __shared__ double red[LP_FIN_THREADS / TH_WAVE];
    for (int n = 0; n < N; ++n) {
        double total = 0.0;
        for (int k = 0; k < 5; ++k) {
            const double* p = partial + t.off[k] + (size_t)n * t.nblk[k];
            double v = 0.0;
            for (int i = threadIdx.x; i < t.nblk[k]; i += LP_FIN_THREADS) v += p[i];
            const double m = lp_block_sum<LP_FIN_THREADS>(v, red) / t.count[k];
            total += m;
            if (threadIdx.x == 0) out[n * 6 + k] = m;
        }
        if (threadIdx.x == 0) out[n * 6 + 5] = total;
    }
}

// ---- training form: the adjoint --------------------------------------------------------------------------------------
// packed input-gradient weights of one layer: [CIN_pad64 / 64][COUT / 8][k = tap * 8 + c][64] with the value
// W[co = chunk * 8 + c][ci = block * 64 + j][2 - tap / 3][2 - tap % 3] (the taps rotated by 180 degrees), zero for ci >= CIN
// (layer 0: 3 of 64).  w: torch layout [COUT][CIN][3][3].
__global__ void lp_pack_bwd_kernel(const float* __restrict__ w, int CIN, int COUT, int nblk, float* __restrict__ out) {
    const int nch = COUT / LP_CK;
    const long long total = (long long)nblk * nch * LP_KC * LP_NB;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % LP_NB);
    const int k = (int)((idx / LP_NB) % LP_KC);
    const int ch = (int)((idx / (LP_NB * LP_KC)) % nch);
    const int blk = (int)(idx / ((long long)LP_NB * LP_KC * nch));
    const int tap = k / LP_CK, co = ch * LP_CK + k % LP_CK, ci = blk * LP_NB + j;
    out[idx] = ci < CIN ? w[((long long)co * CIN + ci) * 9 + (8 - tap)] : 0.f;
}

// backward of the 2 x 2 / stride 2 max pool (floor), NHWC, 4 channels per thread, one thread per element of the UNPOOLED map:
// g [Z][H / 2][W / 2][C] (gradient of the pooled map), y [Z][H][W][C] (the map that was pooled) -> out [Z][H][W][C], every
// element written: g where the element is the first of its window, in row-major window order, that equals the window's
// maximum (torch's rule), 0 elsewhere and in the rows / columns the floor cropped.
__global__ void lp_pool_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y, int Z, int H, int W, int C,
                                   float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const long long total = (long long)Z * H * W * C4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const long long p = idx / C4;
    const int x = (int)(p % W), yy = (int)((p / W) % H), z = (int)(p / ((long long)W * H));
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    const int yo = yy / 2, xo = x / 2;
    if (yo < Ho && xo < Wo) {
        const float4* s = (const float4*)(y + (size_t)z * H * W * C) + c4;
        const float4 v0 = s[((size_t)(2 * yo) * W + 2 * xo) * C4], v1 = s[((size_t)(2 * yo) * W + 2 * xo + 1) * C4];
        const float4 v2 = s[((size_t)(2 * yo + 1) * W + 2 * xo) * C4], v3 = s[((size_t)(2 * yo + 1) * W + 2 * xo + 1) * C4];
        const float4 gv = ((const float4*)(g + (size_t)z * Ho * Wo * C))[((size_t)yo * Wo + xo) * C4 + c4];
        const int me = (yy & 1) * 2 + (x & 1);               // this element's place in the window
        auto first = [](float a, float b, float c, float d) {
            const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
            return a == m ? 0 : b == m ? 1 : c == m ? 2 : 3;
        };
        r.x = first(v0.x, v1.x, v2.x, v3.x) == me ? gv.x : 0.f;
        r.y = first(v0.y, v1.y, v2.y, v3.y) == me ? gv.y : 0.f;
        r.z = first(v0.z, v1.z, v2.z, v3.z) == me ? gv.z : 0.f;
        r.w = first(v0.w, v1.w, v2.w, v3.w) == me ? gv.w : 0.f;
    }
    ((float4*)out)[idx] = r;
}

// backward of one tap's head (lp_head_kernel) with respect to f0, in fp64 on the fp32 features.  With nk = sqrt(sk + 1e-10) +
// 1e-10, rk = sqrt(sk + 1e-10), q[c] = f0[c] / n0 - f1[c] / n1 and T = sum_c 2 lin[c] q[c] f0[c]:
//   d d / d f0[j] = (2 lin[j] q[j] - f0[j] T / (n0 r0)) / n0
// times g_out[n] / hw (the spatial mean and the gradient of image n's total), rounded to fp32, added to g[n][p][j] when
// `accumulate` (the gradient arriving from the deeper level) and, when `gate`, zeroed where f0[j] <= 0 (the ReLU that
// produced the tap).
// f0, f1: [N][hw][C].  8 lanes per pixel as in lp_head_kernel.  grid: (cdiv(hw, 32), N).
__global__ __launch_bounds__(LP_HEAD_THREADS) void lp_head_bwd_kernel(const float* __restrict__ f0a,
                                                                      const float* __restrict__ f1a, int hw, int C,
                                                                      const float* __restrict__ lin,
                                                                      const double* __restrict__ g_out, int accumulate,
                                                                      int gate, float* __restrict__ g) {
    const int n = blockIdx.y, sub = threadIdx.x % LP_HEAD_LANES;
    const int p = blockIdx.x * LP_HEAD_PIX + threadIdx.x / LP_HEAD_LANES;
    const bool live = p < hw;                                // (dead pixels still take part in the shuffles)
    const size_t row = ((size_t)n * hw + (live ? p : 0)) * C;
    const float* f0 = f0a + row;
    const float* f1 = f1a + row;
    double s0 = 0.0, s1 = 0.0;
    if (live)
        for (int c = 4 * sub; c < C; c += 4 * LP_HEAD_LANES) {
            const float4 u = *(const float4*)(f0 + c), v = *(const float4*)(f1 + c);
            s0 += (double)u.x * u.x + (double)u.y * u.y + (double)u.z * u.z + (double)u.w * u.w;
            s1 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    s0 = lp_group_sum(s0);
    s1 = lp_group_sum(s1);
    const double r0 = sqrt(s0 + 1e-10), n0 = r0 + 1e-10, n1 = sqrt(s1 + 1e-10) + 1e-10;
    double t = 0.0;
    if (live)
        for (int c = 4 * sub; c < C; c += 4 * LP_HEAD_LANES) {
            const float4 u = *(const float4*)(f0 + c), v = *(const float4*)(f1 + c);
            const float4 w = *(const float4*)(lin + c);
            t += 2.0 * (double)w.x * ((double)u.x / n0 - (double)v.x / n1) * (double)u.x;
            t += 2.0 * (double)w.y * ((double)u.y / n0 - (double)v.y / n1) * (double)u.y;
            t += 2.0 * (double)w.z * ((double)u.z / n0 - (double)v.z / n1) * (double)u.z;
            t += 2.0 * (double)w.w * ((double)u.w / n0 - (double)v.w / n1) * (double)u.w;
        }
    t = lp_group_sum(t);
    if (!live) return;
    const double tn = t / (n0 * r0), k = g_out[n] / (double)hw;
    float* gr = g + row;
    for (int c = 4 * sub; c < C; c += 4 * LP_HEAD_LANES) {
        const float4 u = *(const float4*)(f0 + c), v = *(const float4*)(f1 + c);
        const float4 w = *(const float4*)(lin + c);
        float4 a = accumulate ? *(const float4*)(gr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        a.x += (float)((2.0 * (double)w.x * ((double)u.x / n0 - (double)v.x / n1) - (double)u.x * tn) / n0 * k);
        a.y += (float)((2.0 * (double)w.y * ((double)u.y / n0 - (double)v.y / n1) - (double)u.y * tn) / n0 * k);
        a.z += (float)((2.0 * (double)w.z * ((double)u.z / n0 - (double)v.z / n1) - (double)u.z * tn) / n0 * k);
        a.w += (float)((2.0 * (double)w.w * ((double)u.w / n0 - (double)v.w / n1) - (double)u.w * tn) / n0 * k);
        if (gate) {
            a.x = u.x > 0.f ? a.x : 0.f;
            a.y = u.y > 0.f ? a.y : 0.f;
            a.z = u.z > 0.f ? a.z : 0.f;
            a.w = u.w > 0.f ? a.w : 0.f;
        }
        *(float4*)(gr + c) = a;
    }
}

// spatial size of each level: H >> l with floor at every pool
void lp_levels(int h, int w, int* hl, int* wl) {
    hl[0] = h;
    wl[0] = w;
    for (int l = 1; l < 5; ++l) {
        hl[l] = hl[l - 1] / 2;
        wl[l] = wl[l - 1] / 2;
    }
}

size_t lp_act_floats(int n, int h, int w) { return (size_t)2 * n * 64 * h * w; }

LpTaps lp_taps(int n, int h, int w) {
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    LpTaps t;
    long long off = 0;
    for (int k = 0; k < 5; ++k) {
        t.off[k] = off;
        t.nblk[k] = th_cdiv((long long)hl[k] * wl[k], LP_HEAD_PIX);
        t.count[k] = (double)hl[k] * (double)wl[k];
        off += (long long)n * t.nblk[k];
    }
    return t;
}

size_t lp_partial_doubles(int n, int h, int w) {
    const LpTaps t = lp_taps(n, h, w);
    return (size_t)(t.off[4] + (long long)n * t.nblk[4]);
}

// packed input-gradient image: the 13 blocks of lp_pack_bwd_kernel (floats)
int lp_bwd_blocks(int l) { return (LP_CIN[l] + LP_NB - 1) / LP_NB; }
size_t lp_bwd_wfloats(int l) { return (size_t)lp_bwd_blocks(l) * LP_NB * LP_COUT[l] * 9; }
size_t lp_bwd_woff(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += lp_bwd_wfloats(i);
    return o;
}

int lp_level_of(int l) {
    for (int k = 0; k < 5; ++k)
        if (l <= LP_LEVEL_LAST[k]) return k;
    return 4;
}

// where the forward writes: the output of each layer -- images 0..n-1 at layer[l], images n..2n-1 at layer1[l] (null: behind
// the others in layer[l]; a tap is always one array, the pool and the head read it as such) --, the pooled map in front of
// levels 1..4, the head's partials
struct LpDest {
    float* layer[LP_NL];
    float* layer1[LP_NL];
    float* pool[5];
    double* partial;
};

bool lp_is_tap(int l) { return l == LP_LEVEL_LAST[lp_level_of(l)]; }

// floats of ONE image's output of layer l
size_t lp_layer_floats(int h, int w, int l) {
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    const int k = lp_level_of(l);
    return (size_t)hl[k] * wl[k] * LP_COUT[l];
}

// The training state.  Kept for the backward: in0's 13 layers and in1's five taps (a tap is [2N][H][W][C], in0's images first;
// every other layer [N][H][W][C]).  Scratch of the forward alone, dead when it returns: in1's other layers pass through two
// buffers (the first layer of a level writes sa, a middle layer sb), every pooled map through one, and the head's partials.
struct LpStatePlan {
    size_t layer[LP_NL], sa, sb, pool, partial;              // floats (partial: doubles)
};
LpStatePlan lp_state_plan(int n, int h, int w) {
    LpStatePlan p{};
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    for (int l = 0; l < LP_NL; ++l) {
        const size_t one = (size_t)n * lp_layer_floats(h, w, l);
        p.layer[l] = lp_is_tap(l) ? 2 * one : one;
        if (!lp_is_tap(l)) {
            const bool first = l == 0 || lp_is_tap(l - 1);
            size_t& sc = first ? p.sa : p.sb;
            if (one > sc) sc = one;
        }
    }
    for (int lev = 1; lev < 5; ++lev) {
        const size_t pf = (size_t)2 * n * hl[lev] * wl[lev] * LP_TAP_C[lev - 1];
        if (pf > p.pool) p.pool = pf;
    }
    p.partial = lp_partial_doubles(n, h, w);
    return p;
}
LpDest lp_state_layout(ThArena& arena, int n, int h, int w) {
    LpDest d;
    const LpStatePlan p = lp_state_plan(n, h, w);
    for (int l = 0; l < LP_NL; ++l) d.layer[l] = arena.take<float>(p.layer[l]);
    float* sa = arena.take<float>(p.sa);
    float* sb = arena.take<float>(p.sb);
    float* pool = arena.take<float>(p.pool);
    d.partial = arena.take<double>(p.partial);
    for (int l = 0; l < LP_NL; ++l) d.layer1[l] = lp_is_tap(l) ? nullptr : (l == 0 || lp_is_tap(l - 1)) ? sa : sb;
    d.pool[0] = nullptr;
    for (int lev = 1; lev < 5; ++lev) d.pool[lev] = pool;
    return d;
}

// the launches of the forward: 13 convolutions, 4 pools, 5 heads, the finish.  split: the destinations keep the two halves of
// the batch in separate arrays (the training state); otherwise every layer1[] is null and the launches are th_lpips's own.
int lp_forward(const float* in0, const float* in1, int n, int h, int w, const float* pk, double* out, const LpDest& d,
               bool split, hipStream_t s) {
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    const LpTaps taps = lp_taps(n, h, w);
    const int Z = 2 * n;
    int l = 0;
    for (int lev = 0; lev < 5; ++lev) {
        const int H = hl[lev], W = wl[lev];
        const float *cur = nullptr, *cur1 = nullptr;         // the current activation: images 0..n-1, n..2n-1 (null: the input)
        if (lev) {                                           // pool the previous tap
            const int C = LP_COUT[l - 1];
            const long long total = (long long)Z * (H) * (W) * (C / 4);
            hipLaunchKernelGGL(lp_pool_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, d.layer[l - 1], Z,
                               hl[lev - 1], wl[lev - 1], C, d.pool[lev]);
            TH_LAUNCH_CHECK();
            cur = d.pool[lev];
            cur1 = cur + (size_t)n * H * W * C;
        }
        const int tiles_x = th_cdiv(W, LP_TW), tiles = tiles_x * th_cdiv(H, LP_TH);
        for (; l <= LP_LEVEL_LAST[lev]; ++l) {
            const dim3 grid((unsigned)tiles, (unsigned)(LP_COUT[l] / LP_NB), (unsigned)Z);
            const float* wl_pk = pk + lp_woff(l);
            const float* bl = pk + lp_bias_off() + (size_t)l * LP_CMAX;
            float* o1 = d.layer1[l] ? d.layer1[l] : d.layer[l] + (size_t)n * H * W * LP_COUT[l];
            if (split) {
                if (l == 0)
                    hipLaunchKernelGGL((lp_conv_kernel<true, LP_EPI_FORWARD, true>), grid, dim3(LP_THREADS), 0, s, in0, in1, n,
                                       H, W, LP_CIN[l], LP_COUT[l], wl_pk, bl, d.layer[l], tiles_x, o1);
                else
                    hipLaunchKernelGGL((lp_conv_kernel<false, LP_EPI_FORWARD, true>), grid, dim3(LP_THREADS), 0, s, cur, cur1, n,
                                       H, W, LP_CIN[l], LP_COUT[l], wl_pk, bl, d.layer[l], tiles_x, o1);
            } else if (l == 0) {
                hipLaunchKernelGGL(lp_conv_kernel<true>, grid, dim3(LP_THREADS), 0, s, in0, in1, n, H, W, LP_CIN[l],
                                   LP_COUT[l], wl_pk, bl, d.layer[l], tiles_x, (float*)nullptr);
            } else {
                hipLaunchKernelGGL(lp_conv_kernel<false>, grid, dim3(LP_THREADS), 0, s, cur, cur, Z, H, W, LP_CIN[l],
                                   LP_COUT[l], wl_pk, bl, d.layer[l], tiles_x, (float*)nullptr);
            }
            TH_LAUNCH_CHECK();
            cur = d.layer[l];
            cur1 = o1;
        }
        hipLaunchKernelGGL(lp_head_kernel, dim3((unsigned)taps.nblk[lev], (unsigned)n), dim3(LP_HEAD_THREADS), 0, s, cur, n,
                           H * W, LP_TAP_C[lev], pk + lp_lin_off() + (size_t)lev * LP_CMAX, d.partial + taps.off[lev]);
        TH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(LP_FIN_THREADS), 0, s, d.partial, taps, n, out);
    TH_LAUNCH_CHECK();
    return 0;
}

int lp_dgrad_launch(int l, const float* g, const float* gate, int Z, int H, int W, const float* pkb, float* out,
                    hipStream_t s) {
    const int tiles_x = th_cdiv(W, LP_TW), tiles = tiles_x * th_cdiv(H, LP_TH);
    const dim3 grid((unsigned)tiles, (unsigned)lp_bwd_blocks(l), (unsigned)Z);
    // (the convolution's CIN / COUT are the forward layer's COUT / CIN; layer 0 writes 3 of its 64-channel block)
    if (l == 0)
        hipLaunchKernelGGL((lp_conv_kernel<false, LP_EPI_IMAGE>), grid, dim3(LP_THREADS), 0, s, g, g, Z, H, W, LP_COUT[l], 3,
                           pkb + lp_bwd_woff(l), (const float*)nullptr, out, tiles_x, (float*)nullptr);
    else
        hipLaunchKernelGGL((lp_conv_kernel<false, LP_EPI_DGRAD>), grid, dim3(LP_THREADS), 0, s, g, g, Z, H, W, LP_COUT[l],
                           LP_CIN[l], pkb + lp_bwd_woff(l), gate, out, tiles_x, (float*)nullptr);
    TH_LAUNCH_CHECK();
    return 0;
}

int lp_pool_bwd_launch(const float* g, const float* y, int Z, int H, int W, int C, float* out, hipStream_t s) {
    const long long total = (long long)Z * H * W * (C / 4);
    hipLaunchKernelGGL(lp_pool_bwd_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, g, y, Z, H, W, C, out);
    TH_LAUNCH_CHECK();
    return 0;
}

int lp_head_bwd_launch(const float* f0, const float* f1, int N, int hw, int C, const float* lin, const double* g_out,
                       int accumulate, int gate, float* g, hipStream_t s) {
    hipLaunchKernelGGL(lp_head_bwd_kernel, dim3((unsigned)th_cdiv(hw, LP_HEAD_PIX), (unsigned)N), dim3(LP_HEAD_THREADS), 0, s,
                       f0, f1, hw, C, lin, g_out, accumulate, gate, g);
    TH_LAUNCH_CHECK();
    return 0;
}

// th_lpips's workspace: two ping-pong activation buffers and the head's partials
struct LpWs { float* buf[2]; double* partial; };
LpWs lp_ws_layout(ThArena& arena, int n, int h, int w) {
    const size_t act = lp_act_floats(n, h, w);
    return {{arena.take<float>(act), arena.take<float>(act)}, arena.take<double>(lp_partial_doubles(n, h, w))};
}
// th_lpips_bwd's workspace: two ping-pong gradient buffers of the largest layer output of one image set
struct LpGrads { float* gb[2]; };
LpGrads lp_bwd_layout(ThArena& arena, int n, int h, int w) {
    const size_t g = (size_t)n * 64 * h * w;
    return {{arena.take<float>(g), arena.take<float>(g)}};
}
bool lp_image_ok(int n, int h, int w) { return n >= 1 && h >= 16 && w >= 16; }

}  // namespace

size_t th_lpips_pack_bytes_internal() { return lp_pack_floats() * sizeof(float); }

size_t th_lpips_ws(int n, int h, int w) { return lp_image_ok(n, h, w) ? th_measure(lp_ws_layout, n, h, w) : 0; }

int th_lpips_pack_launch(const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* packed,
                         size_t bytes, hipStream_t s) {
    TH_REQUIRE(bytes >= th_lpips_pack_bytes_internal(), "packed buffer too small");
    float* pk = (float*)packed;
    for (int l = 0; l < LP_NL; ++l) {
        TH_REQUIRE(conv_w[l] && conv_b[l], "null conv weight or bias of layer " + std::to_string(l));
        const int nch = lp_cin_pad(l) / LP_CK;
        const long long total = (long long)LP_COUT[l] * nch * LP_KC;
        hipLaunchKernelGGL(lp_pack_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, conv_w[l], LP_CIN[l],
                           LP_COUT[l], nch, pk + lp_woff(l));
        TH_LAUNCH_CHECK();
        TH_HIP(hipMemcpyAsync(pk + lp_bias_off() + (size_t)l * LP_CMAX, conv_b[l], LP_COUT[l] * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    }
    for (int k = 0; k < 5; ++k) {
        TH_REQUIRE(lin_w[k], "null lin weight of tap " + std::to_string(k));
        TH_HIP(hipMemcpyAsync(pk + lp_lin_off() + (size_t)k * LP_CMAX, lin_w[k], LP_TAP_C[k] * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int th_lpips_launch(const float* in0, const float* in1, int n, int h, int w, const void* packed, double* out, void* ws,
                    size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(h >= 16 && w >= 16, "image smaller than 16 x 16");
    TH_REQUIRE(n >= 1 && 2 * n <= 65535, "bad batch size");
    ThArena arena(ws, ws_bytes);
    const LpWs lw = lp_ws_layout(arena, n, h, w);
    TH_REQUIRE(arena.ok(), "workspace too small");
    float* const* buf = lw.buf;
    // two ping-pong buffers: every convolution and every pool writes the buffer its input is not in
    LpDest d;
    d.partial = lw.partial;
    int k = 0;
    for (int l = 0, lev = 0; l < LP_NL; ++l) {
        if (l > LP_LEVEL_LAST[lev]) d.pool[++lev] = buf[k++ & 1];
        d.layer[l] = buf[k++ & 1];
        d.layer1[l] = nullptr;
    }
    return lp_forward(in0, in1, n, h, w, (const float*)packed, out, d, false, s);
}

// ---- training form ----------------------------------------------------------------------------------------------------
size_t th_lpips_bwd_pack_bytes_internal() { return lp_bwd_woff(LP_NL) * sizeof(float); }

size_t th_lpips_state_bytes(int n, int h, int w) { return lp_image_ok(n, h, w) ? th_measure(lp_state_layout, n, h, w) : 0; }

size_t th_lpips_bwd_ws(int n, int h, int w) { return lp_image_ok(n, h, w) ? th_measure(lp_bwd_layout, n, h, w) : 0; }

int th_lpips_pack_bwd_launch(const float* const* conv_w, void* packed_bwd, size_t bytes, hipStream_t s) {
    TH_REQUIRE(bytes >= th_lpips_bwd_pack_bytes_internal(), "packed buffer too small");
    float* pk = (float*)packed_bwd;
    for (int l = 0; l < LP_NL; ++l) {
        TH_REQUIRE(conv_w[l], "null conv weight of layer " + std::to_string(l));
        const long long total = (long long)lp_bwd_wfloats(l);
        hipLaunchKernelGGL(lp_pack_bwd_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, conv_w[l], LP_CIN[l],
                           LP_COUT[l], lp_bwd_blocks(l), pk + lp_bwd_woff(l));
        TH_LAUNCH_CHECK();
    }
    return 0;
}

int th_lpips_train_launch(const float* in0, const float* in1, int n, int h, int w, const void* packed, double* out,
                          void* state, size_t state_bytes, hipStream_t s) {
    TH_REQUIRE(h >= 16 && w >= 16, "image smaller than 16 x 16");
    TH_REQUIRE(n >= 1 && 2 * n <= 65535, "bad batch size");
    ThArena st(state, state_bytes);
    const LpDest d = lp_state_layout(st, n, h, w);
    TH_REQUIRE(st.ok(), "state buffer too small");
    return lp_forward(in0, in1, n, h, w, (const float*)packed, out, d, true, s);
}

int th_lpips_bwd_launch(const double* g_out, int n, int h, int w, const void* packed, const void* packed_bwd,
                        const void* state, size_t state_bytes, float* g_in0, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(h >= 16 && w >= 16, "image smaller than 16 x 16");
    TH_REQUIRE(n >= 1 && 2 * n <= 65535, "bad batch size");
    ThArena st(const_cast<void*>(state), state_bytes);
    const LpDest d = lp_state_layout(st, n, h, w);
    TH_REQUIRE(st.ok(), "state buffer too small");
    ThArena arena(ws, ws_bytes);
    const LpGrads lg = lp_bwd_layout(arena, n, h, w);
    float* const* gb = lg.gb;
    TH_REQUIRE(arena.ok(), "workspace too small");
    const float* pk = (const float*)packed;
    const float* pkb = (const float*)packed_bwd;
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    int cur = 0;                                             // gb[cur]: the gradient of the current layer's output
    for (int lev = 4; lev >= 0; --lev) {
        const int H = hl[lev], W = wl[lev], L = LP_LEVEL_LAST[lev], first = lev ? LP_LEVEL_LAST[lev - 1] + 1 : 0;
        const int C = LP_TAP_C[lev];
        // the tap: images 0..n-1 of its layer are in0's features, n..2n-1 in1's
        TH_TRY(lp_head_bwd_launch(d.layer[L], d.layer[L] + (size_t)n * H * W * C, n, H * W, C,
                                  pk + lp_lin_off() + (size_t)lev * LP_CMAX, g_out, lev < 4, 1, gb[cur], s));
        for (int l = L; l >= first; --l) {
            if (l == 0) {
                TH_TRY(lp_dgrad_launch(0, gb[cur], nullptr, n, H, W, pkb, g_in0, s));
            } else {
                TH_TRY(lp_dgrad_launch(l, gb[cur], l > first ? d.layer[l - 1] : nullptr, n, H, W, pkb, gb[cur ^ 1], s));
                cur ^= 1;
            }
        }
        if (lev) {                                           // through the pool into the previous level's tap
            TH_TRY(lp_pool_bwd_launch(gb[cur], d.layer[first - 1], n, hl[lev - 1], wl[lev - 1], LP_TAP_C[lev - 1],
                                      gb[cur ^ 1], s));
            cur ^= 1;
        }
    }
    return 0;
}

// the stages of th_lpips_bwd on their own (for the tests of each against float64)
int th_lpips_dgrad_launch(int layer, const float* g, const float* gate, int Z, int H, int W, const void* packed_bwd, float* out,
                          hipStream_t s) {
    TH_REQUIRE(layer >= 0 && layer < LP_NL, "layer must be in 0..12");
    TH_REQUIRE(Z >= 1 && Z <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 24), "bad shape");
    TH_REQUIRE(layer > 0 || gate == nullptr, "layer 0 has no gate");
    return lp_dgrad_launch(layer, g, gate, Z, H, W, (const float*)packed_bwd, out, s);
}

int th_lpips_pool_bwd_launch(const float* g, const float* y, int Z, int H, int W, int C, float* out, hipStream_t s) {
    TH_REQUIRE(Z >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "bad shape (C must be a multiple of 4)");
    return lp_pool_bwd_launch(g, y, Z, H, W, C, out, s);
}

int th_lpips_head_bwd_launch(const float* f0, const float* f1, int N, int hw, int C, const float* lin, const double* g_out,
                             int accumulate, int gate, float* g, hipStream_t s) {
    TH_REQUIRE(N >= 1 && N <= 65535 && hw >= 1 && C >= 32 && C % 32 == 0, "bad shape (C must be a multiple of 32)");
    return lp_head_bwd_launch(f0, f1, N, hw, C, lin, g_out, accumulate, gate, g, s);
}
