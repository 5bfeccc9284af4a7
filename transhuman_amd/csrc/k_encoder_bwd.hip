// K23: the backward of the encoder trunk in training (SpatialEncoder.trunk: conv1 / bn1 / relu, the max pool, layer1, layer2 of
// ResNet18, encoder.py:114-126).  The forward stays the stock torch modules; nothing in this file is launched by inference or by
// bench.py.  All tensors are NCHW fp32, contiguous.  No kernel here uses an atomic and every sum has a fixed order: two runs on
// the same inputs agree bit for bit.
//
// eb_bn_sums_kernel / eb_bn_apply_kernel   train-mode BatchNorm (+ residual) (+ ReLU), backward.  With y the BatchNorm's input
//     (the convolution's output), out the site's output, g the arriving gradient, L = N * H * W elements per channel and the
//     pivot p = y[0, c, 0, 0] (a shift that keeps the second moment small next to the mean; the constant channel gives exactly 0):
//       g'  = g * [out > 0]                      with a ReLU (torch's rule: 0 at out == 0), else g' = g
//     pass A, per channel, all in fp64 (a product of two fp32 values is exact in fp64):
//       a0 = sum (y - p),  a1 = sum (y - p)^2,  a2 = sum g',  a3 = sum g' (y - p)
//     each thread adds its elements in index order (stride 256 inside a slice of at least EB_BN_SLICE elements), the workgroup adds its
//     threads by a shuffle tree and the waves in wave order, pass B adds the slices in slice order.
//     pass B, per channel, fp64, one rounding per operation, in this order:
//       m = a0 / L,  var = max(a1 / L - m * m, 0),  invstd = 1 / sqrt(var + eps),  s = a3 - m * a2   (= sum g' (y - mean))
//       g_beta = fp32(a2),  g_gamma = fp32(s * invstd),  mg = a2 / L,  mx = s * invstd / L,  k = gamma * invstd  (gamma NULL: 1)
//     per element, fp64, rounded to fp32 once at the end:
//       xhat = ((y - p) - m) * invstd,   g_y = fp32(k * ((g' - mg) - xhat * mx)),   g_res = g' (when asked for)
//     eb_bn_record_kernel / eb_bn_apply_sync_kernel: the same backward for a SyncBatchNorm site, split around the caller's
//     all_gather of one record per rank (th_bn_act_bwd_sums / th_bn_act_bwd_apply; the definition stands beside the kernels).
//
// eb_dgrad_kernel   the input gradient of a 3x3 / pad 1 or 1x1 / pad 0 convolution of stride 1 or 2 as an implicit GEMM on the
//     fp32-input MFMA (v_mfma_f32_32x32x2_f32): no reduced-precision operand, no range guard.  Input pixel (iy, ix) receives
//     g_y[(iy + p - kh) / s, (ix + p - kw) / s] W[co][ci][kh][kw] from the taps for which both divisions are exact.  Stride 1: one
//     class, nine taps -- the forward convolution with the taps rotated by 180 degrees and the channel roles swapped, as K21.
//     Stride 2: the input pixels fall into four parity classes (iy & 1, ix & 1); a class is a small stride-1 convolution over
//     g_y with 1, 2, 2 or 4 of the nine taps (1x1: one tap for class (0, 0), none for the others, which are written as zeros).
//     The parity form was chosen over a gather with all nine taps because the gather multiplies 9 taps per pixel of which on
//     average 2.25 are not structurally zero: four times the MFMA work and four times the staged weights.  A workgroup owns an
//     8 x 16 tile of one class (class coordinates ty = iy >> 1, tx = ix >> 1 at stride 2) x 64 input channels of one image.
//     Per chunk of 8 output channels the 10 x 18 halo of g_y and the chunk's packed weights [tap * 8 + c][64] are staged in LDS;
//     a chunk's taps * 8 products are a fresh MFMA chain (taps in kh-outer, kw-inner order, channels ascending) added to a running
//     fp64 sum in chunk order, which is rounded to fp32 once at the store.  The weights are the MFMA's A operand and the pixels
//     its B operand, so a lane holds one pixel and the stores of a register are 32 consecutive pixels of one channel plane.  Rows / columns of g_y outside [0, Ho) x [0, Wo)
//     count as zero: with odd or even H the last input row may receive nothing from some taps.
//
// eb_wgrad_kernel / eb_wgrad_reduce_kernel   g_W[co][j] = sum over output pixels m = (n, oy, ox) of g_y[n, co, oy, ox] *
//     x[n, ci, oy s + kh - p, ox s + kw - p] with j = (ci * ks + kh) * ks + kw (torch's weight layout).  A GEMM whose reduction
//     index is the output pixel, cut like K20's wgrad_kernel: chunks of EB_WG_CHUNK = 256 consecutive pixels per partial 64 x 64 tile
//     of (co, j).  Inside a chunk every EB_WG_CHAIN = 8 pixels are a fresh MFMA chain (pixels ascending) and the chains are added in
//     pixel order in fp64 registers -- one 256-long fp32 chain measured 4x the error of MIOpen's fp32 weight gradient against
//     float64 --; the chunk's tile is rounded to fp32 once and written to the workspace; the second kernel adds the chunks in chunk
//     order in fp64 and rounds once.  The im2col column of x is formed while staging (32 pixels at a time).
//
// eb_pool_bwd_kernel   max pool 3x3 / stride 2 / pad 1, gather form: one thread per input element; for each of the at most four
//     windows that cover it, the window is scanned as torch's forward scans it (kh outer, kw inner, the padding skipped; the
//     recorded element is the last one for which val > max || isnan(val), starting from -inf at the first valid element) and the
//     window's gradient is taken when that is this element; windows are added in (oy, ox) order.
#include "th_internal.h"

#include <math.h>

namespace {

typedef float eb_f32x16 __attribute__((ext_vector_type(16)));

constexpr int EB_THREADS = 256;
constexpr int EB_BN_SLICE = 8192;        // least number of elements of one channel per pass-A workgroup
constexpr int EB_BN_MAX_SLICES = 64;
constexpr int EB_TW = 16, EB_TH = 8;     // dgrad tile (class coordinates)
constexpr int EB_HW = EB_TW + 2, EB_HH = EB_TH + 2;
constexpr int EB_CK = 8;                 // output channels per staged chunk of dgrad
constexpr int EB_NB = 64;                // input channels per dgrad workgroup
constexpr int EB_WG_CHUNK = 256;         // output pixels per partial tile of wgrad (th_conv2d_wgrad_chunk_pixels)
constexpr int EB_WG_SUB = 32;            // pixels per LDS fill
constexpr int EB_WG_CHAIN = 8;           // pixels per MFMA chain
constexpr int EB_WG_TILE = 64;
constexpr int EB_WG_LD = EB_WG_TILE + 1;

// ---- BatchNorm -------------------------------------------------------------------------------------------------------------
struct EbBnPlan { long long L, slice; int S; };
EbBnPlan eb_bn_plan(int N, int HW) {
    EbBnPlan p;
    p.L = (long long)N * HW;
    long long per = (p.L + EB_BN_MAX_SLICES - 1) / EB_BN_MAX_SLICES;
    per = (per + EB_THREADS - 1) / EB_THREADS * EB_THREADS;
    p.slice = per > EB_BN_SLICE ? per : EB_BN_SLICE;
    p.S = (int)((p.L + p.slice - 1) / p.slice);
    return p;
}

// fixed-order workgroup sum of four doubles per thread; thread 0 holds the result
__device__ void eb_block_sum4(double v[4], double (*red)[4]) {
    for (int k = 0; k < 4; ++k)
        for (int o = TH_WAVE / 2; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, TH_WAVE);
    const int lane = threadIdx.x % TH_WAVE, wave = threadIdx.x / TH_WAVE;
    if (lane == 0)
        for (int k = 0; k < 4; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) {
            double s = red[0][k];
            for (int w = 1; w < EB_THREADS / TH_WAVE; ++w) s += red[w][k];
            v[k] = s;
        }
}

// grid (S, C): partial[(c * S + s) * 4 + k]
__global__ __launch_bounds__(EB_THREADS) void eb_bn_sums_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                                const float* __restrict__ g, int C, int HW, long long L,
                                                                long long slice, double* __restrict__ partial) {
    __shared__ double red[EB_THREADS / TH_WAVE][4];
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const double p = (double)y[(size_t)c * HW];
    const long long lo = (long long)s * slice, hi = lo + slice < L ? lo + slice : L;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    long long i = lo + threadIdx.x;
    int n = (int)(i / HW), r = (int)(i - (long long)n * HW);      // (one division per thread: the loop steps (n, r) along)
    for (; i < hi; i += EB_THREADS) {
        const size_t o = ((size_t)n * C + c) * HW + (size_t)r;
        float gv = g[o];
        if (out != nullptr) gv = out[o] > 0.f ? gv : 0.f;
        const double d = (double)y[o] - p, gd = (double)gv;
        a[0] += d;
        a[1] += d * d;
        a[2] += gd;
        a[3] += gd * d;
        r += EB_THREADS;
        if (r >= HW) {
            const int q = r / HW;
            n += q;
            r -= q * HW;
        }
    }
    eb_block_sum4(a, red);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) partial[((size_t)c * S + s) * 4 + k] = a[k];
}

// the per-element part of pass B over slice s of channel c: xhat = ((y - p) - m) * invstd with this rank's pivot and the mean
// relative to it
__device__ __forceinline__ void eb_bn_apply_slice(const float* __restrict__ y, const float* __restrict__ out,
                                                  const float* __restrict__ g, int C, int HW, long long L, long long slice, int c,
                                                  int s, double p, double m, double invstd, double k, double mg, double mx,
                                                  float* __restrict__ g_y, float* __restrict__ g_res) {
    const long long lo = (long long)s * slice, hi = lo + slice < L ? lo + slice : L;
    long long i = lo + threadIdx.x;
    int n = (int)(i / HW), r = (int)(i - (long long)n * HW);      // (one division per thread: the loop steps (n, r) along)
    for (; i < hi; i += EB_THREADS) {
        const size_t o = ((size_t)n * C + c) * HW + (size_t)r;
        float gv = g[o];
        if (out != nullptr) gv = out[o] > 0.f ? gv : 0.f;
        const double xhat = (((double)y[o] - p) - m) * invstd;
        g_y[o] = (float)(k * (((double)gv - mg) - xhat * mx));
        if (g_res != nullptr) g_res[o] = gv;
        r += EB_THREADS;
        if (r >= HW) {
            const int q = r / HW;
            n += q;
            r -= q * HW;
        }
    }
}

// grid (S, C), the same slices
__global__ __launch_bounds__(EB_THREADS) void eb_bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                                 const float* __restrict__ g, int C, int HW, long long L,
                                                                 long long slice, const double* __restrict__ partial,
                                                                 const float* __restrict__ gamma, double eps,
                                                                 float* __restrict__ g_y, float* __restrict__ g_res,
                                                                 float* __restrict__ g_gamma, float* __restrict__ g_beta) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < S; ++t)
        for (int k = 0; k < 4; ++k) a[k] += partial[((size_t)c * S + t) * 4 + k];
    const double p = (double)y[(size_t)c * HW];
    const double Ld = (double)L;
    const double m = a[0] / Ld;
    double var = a[1] / Ld - m * m;
    var = var > 0.0 ? var : 0.0;
    const double invstd = 1.0 / sqrt(var + eps);
    const double sgy = a[3] - m * a[2];
    const double mg = a[2] / Ld, mx = sgy * invstd / Ld;
    const double k = (gamma != nullptr ? (double)gamma[c] : 1.0) * invstd;
    if (s == 0 && threadIdx.x == 0) {
        if (g_beta != nullptr) g_beta[c] = (float)a[2];
        if (g_gamma != nullptr) g_gamma[c] = (float)(sgy * invstd);
    }
    eb_bn_apply_slice(y, out, g, C, HW, L, slice, c, s, p, m, invstd, k, mg, mx, g_y, g_res);
}

// ---- the split form for SyncBatchNorm sites: pass A ends in a record per channel, the ranks' records are gathered by the caller,
// pass B combines them in rank order.  record [C][6] = a0 a1 a2 a3 p L, every sum against the rank's OWN pivot p_r.  With
// d_r = p_r - p_0 (fp64) the sums against rank 0's pivot are, added over r in rank order (rank 0's terms taken as they are: d_0 = 0),
//   A0 = sum (a0_r + L_r d_r)     A1 = sum ((a1_r + (2 d_r) a0_r) + (L_r d_r) d_r)     A2 = sum a2_r     A3 = sum (a3_r + d_r a2_r)
// and L = sum L_r; m, var, invstd, mg, mx, k follow from them as in pass B above.  Per element xhat = ((y - p_r) - (m - d_r)) invstd;
// g_beta = fp32(a2_r) and g_gamma = fp32((a3_r - (m - d_r) a2_r) invstd) are the rank's LOCAL sums (the exchange averages them, as
// with torch's SyncBatchNorm).  One rank: every correction is absent and the launch pair IS th_bn_act_bwd, bit for bit.
constexpr int EB_BN_REC = 6;

// one thread per (channel, sum): the slices of pass A added in slice order, as eb_bn_apply_kernel adds them
__global__ __launch_bounds__(EB_THREADS) void eb_bn_record_kernel(const float* __restrict__ y, int C, int HW, long long L, int S,
                                                                  const double* __restrict__ partial, double* __restrict__ record) {
    const int i = blockIdx.x * EB_THREADS + threadIdx.x, c = i >> 2, k = i & 3;
    if (c >= C) return;
    double a = 0.0;
    for (int t = 0; t < S; ++t) a += partial[((size_t)c * S + t) * 4 + k];
    double* rec = record + (size_t)c * EB_BN_REC;
    rec[k] = a;
    if (k == 0) rec[4] = (double)y[(size_t)c * HW];
    if (k == 1) rec[5] = (double)L;
}

// grid (S, C), the slices of pass A
__global__ __launch_bounds__(EB_THREADS) void eb_bn_apply_sync_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                                      const float* __restrict__ g, int C, int HW, long long L,
                                                                      long long slice, const double* __restrict__ records, int world,
                                                                      int rank, const float* __restrict__ gamma, double eps,
                                                                      float* __restrict__ g_y, float* __restrict__ g_res,
                                                                      float* __restrict__ g_gamma, float* __restrict__ g_beta) {
    const int c = blockIdx.y, s = blockIdx.x;
    const double* r0 = records + (size_t)c * EB_BN_REC;
    const double p0 = r0[4];
    double A0 = r0[0], A1 = r0[1], A2 = r0[2], A3 = r0[3], Ld = r0[5];
    for (int r = 1; r < world; ++r) {
        const double* q = records + ((size_t)r * C + c) * EB_BN_REC;
        const double d = q[4] - p0, Lr = q[5];
        A0 += q[0] + Lr * d;
        A1 += (q[1] + (2.0 * d) * q[0]) + (Lr * d) * d;
        A2 += q[2];
        A3 += q[3] + d * q[2];
        Ld += Lr;
    }
    const double m = A0 / Ld;
    double var = A1 / Ld - m * m;
    var = var > 0.0 ? var : 0.0;
    const double invstd = 1.0 / sqrt(var + eps);
    const double sgy = A3 - m * A2;
    const double mg = A2 / Ld, mx = sgy * invstd / Ld;
    const double k = (gamma != nullptr ? (double)gamma[c] : 1.0) * invstd;
    const double* own = records + ((size_t)rank * C + c) * EB_BN_REC;
    const double p = own[4];
    const double ml = m - (p - p0);                              // the mean relative to this rank's pivot (rank 0: m - 0)
    if (s == 0 && threadIdx.x == 0) {
        if (g_beta != nullptr) g_beta[c] = (float)own[2];
        if (g_gamma != nullptr) g_gamma[c] = (float)((own[3] - ml * own[2]) * invstd);
    }
    eb_bn_apply_slice(y, out, g, C, HW, L, slice, c, s, p, ml, invstd, k, mg, mx, g_y, g_res);
}

// ---- max pool 3x3 / 2 / 1 -----------------------------------------------------------------------------------------------------
__global__ void eb_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, long long total, int H, int W, int Ho,
                                   int Wo, float* __restrict__ gx) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx % W), h = (int)((idx / W) % H);
    const long long plane = idx / ((long long)W * H);
    const float* xp = x + (size_t)plane * H * W;
    const float* gp = g + (size_t)plane * Ho * Wo;
    const int me = h * W + w;
    const int oy_hi = (h + 1) / 2 < Ho - 1 ? (h + 1) / 2 : Ho - 1;
    const int ox_hi = (w + 1) / 2 < Wo - 1 ? (w + 1) / 2 : Wo - 1;
    float acc = 0.f;
    for (int oy = h / 2; oy <= oy_hi; ++oy)
        for (int ox = w / 2; ox <= ox_hi; ++ox) {
            const int h0 = 2 * oy - 1 > 0 ? 2 * oy - 1 : 0, h1 = 2 * oy + 2 < H ? 2 * oy + 2 : H;
            const int w0 = 2 * ox - 1 > 0 ? 2 * ox - 1 : 0, w1 = 2 * ox + 2 < W ? 2 * ox + 2 : W;
            float mv = -INFINITY;
            int mi = h0 * W + w0;
            for (int ih = h0; ih < h1; ++ih)
                for (int iw = w0; iw < w1; ++iw) {
                    const float v = xp[ih * W + iw];
                    if (v > mv || isnan(v)) {
                        mv = v;
                        mi = ih * W + iw;
                    }
                }
            if (mi == me) acc = acc + gp[oy * Wo + ox];
        }
    gx[idx] = acc;
}

// ---- convolution shapes --------------------------------------------------------------------------------------------------------
// bit 0: weight gradient, bit 1: input gradient
int eb_supported(int cin, int cout, int ks, int stride) {
    if (cin == 3 && cout == 64 && ks == 7 && stride == 2) return 1;
    if (cin == 64 && cout == 64 && ks == 3 && stride == 1) return 3;
    if (cin == 128 && cout == 128 && ks == 3 && stride == 1) return 3;
    if (cin == 64 && cout == 128 && ks == 3 && stride == 2) return 3;
    if (cin == 64 && cout == 128 && ks == 1 && stride == 2) return 3;
    return 0;
}
int eb_out(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }

// ---- dgrad ---------------------------------------------------------------------------------------------------------------------
struct EbClass {
    int ntaps, py, px;
    int kh[9], kw[9], dy[9], dx[9];      // g_y row of class row ty: ty + dy
    long long woff;                      // floats into the packed image
};
struct EbClasses {
    int n;
    EbClass c[4];
    long long floats;
};
EbClasses eb_classes(int cin, int cout, int ks, int stride) {
    EbClasses t{};
    const int p = ks / 2;
    t.n = stride * stride;
    long long off = 0;
    for (int py = 0; py < stride; ++py)
        for (int px = 0; px < stride; ++px) {
            EbClass& k = t.c[py * stride + px];
            k.py = py;
            k.px = px;
            k.ntaps = 0;
            for (int kh = 0; kh < ks; ++kh) {
                if ((py + p - kh) % stride != 0) continue;
                for (int kw = 0; kw < ks; ++kw) {
                    if ((px + p - kw) % stride != 0) continue;
                    k.kh[k.ntaps] = kh;
                    k.kw[k.ntaps] = kw;
                    k.dy[k.ntaps] = (py + p - kh) / stride;
                    k.dx[k.ntaps] = (px + p - kw) / stride;
                    ++k.ntaps;
                }
            }
            k.woff = off;
            off += (long long)k.ntaps * cin * cout;
        }
    t.floats = off;
    return t;
}

// one class: out[((blk * nch + ch) * ntaps * 8 + t * 8 + c) * 64 + j] = W[co = ch * 8 + c][ci = blk * 64 + j][kh_t][kw_t]
__global__ void eb_dgrad_pack_kernel(const float* __restrict__ w, int CIN, int COUT, int ks, EbClass k, float* __restrict__ out) {
    const long long total = (long long)k.ntaps * CIN * COUT;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int nch = COUT / EB_CK, kc = k.ntaps * EB_CK;
    const int j = (int)(idx % EB_NB);
    const int kk = (int)((idx / EB_NB) % kc);
    const int ch = (int)((idx / ((long long)EB_NB * kc)) % nch);
    const int blk = (int)(idx / ((long long)EB_NB * kc * nch));
    const int t = kk / EB_CK, co = ch * EB_CK + kk % EB_CK, ci = blk * EB_NB + j;
    out[k.woff + idx] = w[(((size_t)co * CIN + ci) * ks + k.kh[t]) * ks + k.kw[t]];
}

// grid (tiles, CIN / 64, N * classes)
__global__ __launch_bounds__(EB_THREADS) void eb_dgrad_kernel(const float* __restrict__ gy, int COUT, int Ho, int Wo,
                                                              const float* __restrict__ wpk, EbClasses tab, int stride, int CIN,
                                                              int H, int W, float* __restrict__ gx, int tiles_x) {
    __shared__ float sIn[EB_CK][EB_HH][EB_HW];
    __shared__ __attribute__((aligned(16))) float sW[9 * EB_CK][EB_NB];

    const int tid = threadIdx.x, lane = tid % TH_WAVE, wave = tid / TH_WAVE;
    const int blk = blockIdx.y, cls = blockIdx.z % tab.n, n = blockIdx.z / tab.n;
    const EbClass& k = tab.c[cls];
    const int ty0 = (blockIdx.x / tiles_x) * EB_TH, tx0 = (blockIdx.x % tiles_x) * EB_TW;
    const int nch = k.ntaps ? COUT / EB_CK : 0;
    const int i_pix = lane & 31, hk = lane >> 5;
    const int py = 2 * wave + (i_pix >> 4), px = i_pix & 15;
    const int kc = k.ntaps * EB_CK;

    double tot0[16], tot1[16];                               // the chunks' chains, added in chunk order
    for (int r = 0; r < 16; ++r) tot0[r] = tot1[r] = 0.0;

    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();
        const float4* wsrc = (const float4*)(wpk + k.woff + ((size_t)blk * nch + ch) * ((size_t)kc * EB_NB));
        for (int i = tid; i < kc * EB_NB / 4; i += EB_THREADS) ((float4*)&sW[0][0])[i] = wsrc[i];
        const float* src = gy + ((size_t)n * COUT + (size_t)ch * EB_CK) * Ho * Wo;
        for (int i = tid; i < EB_CK * EB_HH * EB_HW; i += EB_THREADS) {
            const int c = i / (EB_HH * EB_HW), r = (i / EB_HW) % EB_HH, col = i % EB_HW;
            const int oy = ty0 - 1 + r, ox = tx0 - 1 + col;
            float v = 0.f;
            if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) v = src[((size_t)c * Ho + oy) * Wo + ox];
            sIn[c][r][col] = v;
        }
        __syncthreads();
        eb_f32x16 acc0, acc1;
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
        for (int t = 0; t < k.ntaps; ++t) {
            const int rr = py + 1 + k.dy[t], cc = px + 1 + k.dx[t];
#pragma unroll
            for (int q = 0; q < EB_CK / 2; ++q) {
                const int c = 2 * q + hk;
                const float pv = sIn[c][rr][cc];
                const float w0 = sW[t * EB_CK + c][i_pix], w1 = sW[t * EB_CK + c][32 + i_pix];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, pv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, pv, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tot0[r] += (double)acc0[r];
            tot1[r] += (double)acc1[r];
        }
    }

    // C/D map of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int iy = (ty0 + py) * stride + k.py, ix = (tx0 + px) * stride + k.px;
    if (iy < H && ix < W) {
        float* dst = gx + ((size_t)n * CIN + (size_t)blk * EB_NB) * H * W + (size_t)iy * W + ix;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hk;
            dst[(size_t)row * H * W] = (float)tot0[r];
            dst[(size_t)(row + 32) * H * W] = (float)tot1[r];
        }
    }
}

// ---- wgrad ---------------------------------------------------------------------------------------------------------------------
// grid (chunks, cdiv(J, 64), COUT / 64); part[(chunk * COUT + co) * J + j]
__global__ __launch_bounds__(EB_THREADS) void eb_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy, int CIN,
                                                              int H, int W, int COUT, int Ho, int Wo, int ks, int stride, int pad,
                                                              int Mtot, float* __restrict__ part) {
    __shared__ float sG[EB_WG_SUB][EB_WG_LD];
    __shared__ float sB[EB_WG_SUB][EB_WG_LD];
    const int tid = threadIdx.x, lane = tid % TH_WAVE, wave = tid / TH_WAVE;
    const int chunk = blockIdx.x, j0 = blockIdx.y * EB_WG_TILE, co0 = blockIdx.z * EB_WG_TILE;
    const int J = CIN * ks * ks, HoWo = Ho * Wo;
    const int pk = tid & 31, q = tid >> 5;
    // this thread's eight columns j0 + q + 8 e: the plane of x and the tap
    int jci[8], jkh[8], jkw[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = j0 + q + 8 * e;
        if (j < J) {
            jci[e] = j / (ks * ks);
            const int t = j - jci[e] * ks * ks;
            jkh[e] = t / ks - pad;
            jkw[e] = t % ks - pad;
        } else {
            jci[e] = -1;
            jkh[e] = jkw[e] = 0;
        }
    }
    const int i32 = lane & 31, hk = lane >> 5, cot = wave & 1, jt = wave >> 1;
    double tot[16];                                          // the chunk's chains, added in pixel order
    for (int r = 0; r < 16; ++r) tot[r] = 0.0;
#pragma unroll 1
    for (int sub = 0; sub < EB_WG_CHUNK / EB_WG_SUB; ++sub) {
        const int m = chunk * EB_WG_CHUNK + sub * EB_WG_SUB + pk;
        const bool live = m < Mtot;
        const int n = live ? m / HoWo : 0;
        const int rem = live ? m - n * HoWo : 0;
        const int oy = rem / Wo, ox = rem - oy * Wo;
        if (sub) __syncthreads();
        const float* gsrc = gy + ((size_t)n * COUT + co0 + q) * HoWo + rem;
#pragma unroll
        for (int e = 0; e < 8; ++e) sG[pk][q + 8 * e] = live ? gsrc[(size_t)8 * e * HoWo] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int iy = oy * stride + jkh[e], ix = ox * stride + jkw[e];
            float v = 0.f;
            if (live && jci[e] >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W)
                v = x[(((size_t)n * CIN + jci[e]) * H + iy) * W + ix];
            sB[pk][q + 8 * e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int c0 = 0; c0 < EB_WG_SUB; c0 += EB_WG_CHAIN) {
            eb_f32x16 acc;
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int st = 0; st < EB_WG_CHAIN / 2; ++st) {
                const int kk = c0 + 2 * st + hk;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sG[kk][cot * 32 + i32], sB[kk][jt * 32 + i32], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[r] += (double)acc[r];
        }
    }
    const int j = j0 + jt * 32 + i32;
    if (j < J) {
        float* dst = part + ((size_t)chunk * COUT + co0 + cot * 32) * J + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hk;
            dst[(size_t)row * J] = (float)tot[r];
        }
    }
}

__global__ void eb_wgrad_reduce_kernel(const float* __restrict__ part, int chunks, long long elems, float* __restrict__ gw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= elems) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += (double)part[(size_t)c * elems + i];
    gw[i] = (float)s;
}

bool eb_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
bool eb_dims_ok(int N, int cin, int cout, int ks, int stride, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || N > 16383) return false;
    const long long in = (long long)N * cin * H * W, out = (long long)N * cout * eb_out(H, ks, stride) * eb_out(W, ks, stride);
    return in < (1LL << 31) && out < (1LL << 31);
}

}  // namespace

int th_conv2d_bwd_supported_internal(int cin, int cout, int ks, int stride) { return eb_supported(cin, cout, ks, stride); }
int th_conv2d_wgrad_chunk_internal() { return EB_WG_CHUNK; }
void th_conv2d_dgrad_tile_internal(int* rows, int* cols) { *rows = EB_TH; *cols = EB_TW; }
int th_bn_act_bwd_slice_internal() { return EB_BN_SLICE; }

// four partial sums per (slice, channel)
static double* eb_bn_layout(ThArena& ar, int N, int C, int HW) { return ar.take<double>((size_t)C * eb_bn_plan(N, HW).S * 4); }
size_t th_bn_act_bwd_ws(int N, int C, int HW) {
    if (N < 1 || C < 1 || HW < 1 || (long long)N * C * HW >= (1LL << 31) || C > 65535) return 0;
    return th_measure(eb_bn_layout, N, C, HW);
}

int th_bn_act_bwd_launch(const float* y, const float* out, const float* g, int N, int C, int HW, const float* gamma, double eps,
                         float* g_y, float* g_res, float* g_gamma, float* g_beta, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(N >= 1 && C >= 1 && C <= 65535 && HW >= 1 && (long long)N * C * HW < (1LL << 31),
               "unsupported shape: N, C, HW >= 1, C <= 65535, fewer than 2^31 elements");
    TH_REQUIRE(eps > 0.0, "eps must be positive");
    ThArena ar(ws, ws_bytes);
    double* sums = eb_bn_layout(ar, N, C, HW);
    TH_REQUIRE(ar.ok(), "workspace too small");
    TH_REQUIRE((((uintptr_t)ws) & 7) == 0, "the workspace must be 8-byte aligned");
    const EbBnPlan p = eb_bn_plan(N, HW);
    const dim3 grid((unsigned)p.S, (unsigned)C);
    hipLaunchKernelGGL(eb_bn_sums_kernel, grid, dim3(EB_THREADS), 0, s, y, out, g, C, HW, p.L, p.slice, sums);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(eb_bn_apply_kernel, grid, dim3(EB_THREADS), 0, s, y, out, g, C, HW, p.L, p.slice, (const double*)sums, gamma,
                       eps, g_y, g_res, g_gamma, g_beta);
    TH_LAUNCH_CHECK();
    return 0;
}

// pass A of th_bn_act_bwd (the same slices, the same workspace) and the record of this rank
int th_bn_act_bwd_sums_launch(const float* y, const float* out, const float* g, int N, int C, int HW, double* record, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(N >= 1 && C >= 1 && C <= 65535 && HW >= 1 && (long long)N * C * HW < (1LL << 31),
               "unsupported shape: N, C, HW >= 1, C <= 65535, fewer than 2^31 elements");
    ThArena ar(ws, ws_bytes);
    double* sums = eb_bn_layout(ar, N, C, HW);
    TH_REQUIRE(ar.ok(), "workspace too small");
    TH_REQUIRE((((uintptr_t)ws) & 7) == 0 && (((uintptr_t)record) & 7) == 0, "the workspace and the record must be 8-byte aligned");
    const EbBnPlan p = eb_bn_plan(N, HW);
    hipLaunchKernelGGL(eb_bn_sums_kernel, dim3((unsigned)p.S, (unsigned)C), dim3(EB_THREADS), 0, s, y, out, g, C, HW, p.L, p.slice,
                       sums);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(eb_bn_record_kernel, dim3((unsigned)th_cdiv(4LL * C, EB_THREADS)), dim3(EB_THREADS), 0, s, y, C, HW, p.L, p.S,
                       (const double*)sums, record);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_bn_act_bwd_apply_launch(const float* y, const float* out, const float* g, int N, int C, int HW, const float* gamma, double eps,
                               const double* records, int world, int rank, float* g_y, float* g_res, float* g_gamma, float* g_beta,
                               hipStream_t s) {
    TH_REQUIRE(N >= 1 && C >= 1 && C <= 65535 && HW >= 1 && (long long)N * C * HW < (1LL << 31),
               "unsupported shape: N, C, HW >= 1, C <= 65535, fewer than 2^31 elements");
    TH_REQUIRE(eps > 0.0, "eps must be positive");
    TH_REQUIRE(world >= 1 && world <= 4096 && rank >= 0 && rank < world,
               "rank " + std::to_string(rank) + " of " + std::to_string(world) + ": world in 1 .. 4096, rank in 0 .. world - 1");
    TH_REQUIRE((((uintptr_t)records) & 7) == 0, "the records must be 8-byte aligned");
    const EbBnPlan p = eb_bn_plan(N, HW);
    hipLaunchKernelGGL(eb_bn_apply_sync_kernel, dim3((unsigned)p.S, (unsigned)C), dim3(EB_THREADS), 0, s, y, out, g, C, HW, p.L,
                       p.slice, records, world, rank, gamma, eps, g_y, g_res, g_gamma, g_beta);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_maxpool3x3s2_bwd_launch(const float* x, const float* g, int planes, int H, int W, float* gx, hipStream_t s) {
    TH_REQUIRE(planes >= 1 && H >= 1 && W >= 1 && (long long)planes * H * W < (1LL << 31),
               "unsupported shape: planes, H, W >= 1, fewer than 2^31 elements");
    const long long total = (long long)planes * H * W;
    hipLaunchKernelGGL(eb_pool_bwd_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, x, g, total, H, W, eb_out(H, 3, 2),
                       eb_out(W, 3, 2), gx);
    TH_LAUNCH_CHECK();
    return 0;
}

size_t th_conv2d_dgrad_pack_size(int cin, int cout, int ks, int stride) {
    if (!(eb_supported(cin, cout, ks, stride) & 2)) return 0;
    return th_align((size_t)eb_classes(cin, cout, ks, stride).floats * sizeof(float));
}

int th_conv2d_dgrad_pack_launch(const float* w, int cin, int cout, int ks, int stride, void* packed, size_t bytes, hipStream_t s) {
    TH_REQUIRE(eb_supported(cin, cout, ks, stride) & 2, "unsupported shape: no input gradient is built for this convolution");
    TH_REQUIRE(bytes >= th_conv2d_dgrad_pack_size(cin, cout, ks, stride), "packed buffer too small");
    TH_REQUIRE(eb_al16(packed), "the packed buffer must be 16-byte aligned");
    const EbClasses t = eb_classes(cin, cout, ks, stride);
    for (int c = 0; c < t.n; ++c) {
        const long long total = (long long)t.c[c].ntaps * cin * cout;
        if (total == 0) continue;
        hipLaunchKernelGGL(eb_dgrad_pack_kernel, dim3((unsigned)th_cdiv(total, 256)), dim3(256), 0, s, w, cin, cout, ks, t.c[c],
                           (float*)packed);
        TH_LAUNCH_CHECK();
    }
    return 0;
}

int th_conv2d_dgrad_launch(const float* gy, int N, int cin, int cout, int ks, int stride, int H, int W, const void* packed,
                           size_t packed_bytes, float* gx, hipStream_t s) {
    TH_REQUIRE(eb_supported(cin, cout, ks, stride) & 2, "unsupported shape: no input gradient is built for this convolution");
    TH_REQUIRE(eb_dims_ok(N, cin, cout, ks, stride, H, W), "unsupported shape: N in 1..16383, H, W >= 1, fewer than 2^31 elements");
    TH_REQUIRE(packed_bytes >= th_conv2d_dgrad_pack_size(cin, cout, ks, stride), "packed buffer too small");
    TH_REQUIRE(eb_al16(packed), "the packed buffer must be 16-byte aligned");
    const EbClasses t = eb_classes(cin, cout, ks, stride);
    const int Hc = th_cdiv(H, stride), Wc = th_cdiv(W, stride);
    const int tiles_x = th_cdiv(Wc, EB_TW), tiles = tiles_x * th_cdiv(Hc, EB_TH);
    const dim3 grid((unsigned)tiles, (unsigned)(cin / EB_NB), (unsigned)(N * t.n));
    hipLaunchKernelGGL(eb_dgrad_kernel, grid, dim3(EB_THREADS), 0, s, gy, cout, eb_out(H, ks, stride), eb_out(W, ks, stride),
                       (const float*)packed, t, stride, cin, H, W, gx, tiles_x);
    TH_LAUNCH_CHECK();
    return 0;
}

// one partial weight gradient [cout][cin ks ks] per chunk of output positions
static float* eb_wgrad_layout(ThArena& ar, int N, int cin, int cout, int ks, int stride, int H, int W) {
    const long long M = (long long)N * eb_out(H, ks, stride) * eb_out(W, ks, stride);
    return ar.take<float>((size_t)th_cdiv(M, EB_WG_CHUNK) * cout * cin * ks * ks);
}
size_t th_conv2d_wgrad_ws(int N, int cin, int cout, int ks, int stride, int H, int W) {
    if (!(eb_supported(cin, cout, ks, stride) & 1) || !eb_dims_ok(N, cin, cout, ks, stride, H, W)) return 0;
    return th_measure(eb_wgrad_layout, N, cin, cout, ks, stride, H, W);
}

int th_conv2d_wgrad_launch(const float* x, const float* gy, int N, int cin, int cout, int ks, int stride, int H, int W, float* gw,
                           void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(eb_supported(cin, cout, ks, stride) & 1, "unsupported shape: no weight gradient is built for this convolution");
    TH_REQUIRE(eb_dims_ok(N, cin, cout, ks, stride, H, W), "unsupported shape: N in 1..16383, H, W >= 1, fewer than 2^31 elements");
    ThArena ar(ws, ws_bytes);
    float* part = eb_wgrad_layout(ar, N, cin, cout, ks, stride, H, W);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int Ho = eb_out(H, ks, stride), Wo = eb_out(W, ks, stride), J = cin * ks * ks;
    const int Mtot = N * Ho * Wo, chunks = th_cdiv(Mtot, EB_WG_CHUNK);
    const dim3 grid((unsigned)chunks, (unsigned)th_cdiv(J, EB_WG_TILE), (unsigned)(cout / EB_WG_TILE));
    hipLaunchKernelGGL(eb_wgrad_kernel, grid, dim3(EB_THREADS), 0, s, x, gy, cin, H, W, cout, Ho, Wo, ks, stride, ks / 2, Mtot,
                       part);
    TH_LAUNCH_CHECK();
    const long long elems = (long long)cout * J;
    hipLaunchKernelGGL(eb_wgrad_reduce_kernel, dim3((unsigned)th_cdiv(elems, 256)), dim3(256), 0, s, (const float*)part, chunks, elems,
                       gw);
    TH_LAUNCH_CHECK();
    return 0;
}
