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
template <bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void lp_conv_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             int nsplit, int H, int W, int CIN, int COUT,
                                                             const float* __restrict__ wpk, const float* __restrict__ bias,
                                                             float* __restrict__ out, int tiles_x) {
    __shared__ float sIn[LP_CK][LP_HH][LP_HW];
    __shared__ __attribute__((aligned(16))) float sW[LP_KC][LP_NB];

    const int tid = threadIdx.x, lane = tid % TH_WAVE, wave = tid / TH_WAVE;
    const int cob = blockIdx.y, z = blockIdx.z;
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

}  // namespace

size_t th_lpips_pack_bytes_internal() { return lp_pack_floats() * sizeof(float); }

size_t th_lpips_ws(int n, int h, int w) {
    if (n < 1 || h < 16 || w < 16) return 0;
    return 2 * th_align(lp_act_floats(n, h, w) * sizeof(float)) + th_align(lp_partial_doubles(n, h, w) * sizeof(double));
}

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
    TH_REQUIRE(ws_bytes >= th_lpips_ws(n, h, w), "workspace too small");
    const float* pk = (const float*)packed;
    ThArena arena(ws, ws_bytes);
    float* buf[2] = {arena.take<float>(lp_act_floats(n, h, w)), arena.take<float>(lp_act_floats(n, h, w))};
    double* partial = arena.take<double>(lp_partial_doubles(n, h, w));
    TH_REQUIRE(buf[0] && buf[1] && partial, "workspace too small");
    int hl[5], wl[5];
    lp_levels(h, w, hl, wl);
    const LpTaps taps = lp_taps(n, h, w);
    const int Z = 2 * n;

    int cur = -1;                                            // buffer holding the current activation (-1: the input)
    int l = 0;
    for (int lev = 0; lev < 5; ++lev) {
        const int H = hl[lev], W = wl[lev];
        if (lev) {                                           // pool the previous tap into the other buffer
            const int C = LP_COUT[l - 1];
            const long long total = (long long)Z * (H) * (W) * (C / 4);
            hipLaunchKernelGGL(lp_pool_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, buf[cur], Z,
                               hl[lev - 1], wl[lev - 1], C, buf[cur ^ 1]);
            TH_LAUNCH_CHECK();
            cur ^= 1;
        }
        const int tiles_x = th_cdiv(W, LP_TW), tiles = tiles_x * th_cdiv(H, LP_TH);
        for (; l <= LP_LEVEL_LAST[lev]; ++l) {
            const dim3 grid((unsigned)tiles, (unsigned)(LP_COUT[l] / LP_NB), (unsigned)Z);
            const float* wl_pk = pk + lp_woff(l);
            const float* bl = pk + lp_bias_off() + (size_t)l * LP_CMAX;
            if (l == 0) {
                hipLaunchKernelGGL(lp_conv_kernel<true>, grid, dim3(LP_THREADS), 0, s, in0, in1, n, H, W, LP_CIN[l],
                                   LP_COUT[l], wl_pk, bl, buf[0], tiles_x);
                cur = 0;
            } else {
                hipLaunchKernelGGL(lp_conv_kernel<false>, grid, dim3(LP_THREADS), 0, s, buf[cur], buf[cur], Z, H, W,
                                   LP_CIN[l], LP_COUT[l], wl_pk, bl, buf[cur ^ 1], tiles_x);
                cur ^= 1;
            }
            TH_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(lp_head_kernel, dim3((unsigned)taps.nblk[lev], (unsigned)n), dim3(LP_HEAD_THREADS), 0, s,
                           buf[cur], n, H * W, LP_TAP_C[lev], pk + lp_lin_off() + (size_t)lev * LP_CMAX,
                           partial + taps.off[lev]);
        TH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(LP_FIN_THREADS), 0, s, partial, taps, n, out);
    TH_LAUNCH_CHECK();
    return 0;
}
