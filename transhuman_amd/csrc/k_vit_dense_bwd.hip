// K3 training form, dense half: the backward of TransHE's Linear / LayerNorm / GELU layers (and the thin forward entries
// that th_linear_forward does not serve), and the same layer with a ReLU on its OUTPUT, which the per-point network's training
// form is made of (K20, th_linear_relu_*).  Nothing in this file is launched by inference or by bench.py.
//
// For y = Linear(op(A)) with W [out, in] row-major and g_C = dL/dy [M, out]:
//
//   dgrad  g_op[M, in]  = g_C W             th_gemm on a weight image packed from W^T (pack_linear_t_kernel), then the
//                                           operand's own adjoint: nothing (op = identity), * gelu'(u) in place
//                                           (gelu_bwd_kernel), or the LayerNorm backward in place (ln_bwd_kernel)
//   wgrad  g_W[out, in] = sum_m g_C[m, out] op(A)[m, in],  g_b[out] = sum_m g_C[m, out]     wgrad_kernel (below)
//
// op(A) is never stored: LN(x) and gelu(u) are recomputed on the operand's way into LDS (the row statistics of LN come from
// ln_stats_kernel, which restates the 16-lanes-per-row two-pass rule of th_gemm_ln's prologue expression for expression, so
// the recomputed operand is bit for bit the one the forward GEMM multiplied).
//
// wgrad_kernel: both operands are activations stored [M, .] row-major and the reduction runs over the ROW index, so
// neither is in fragment order.  One workgroup (4 waves) owns a 64 (out) x 64 (in) tile of g_W for one chunk of
// WG_CHUNK = 256 rows: it stages 64 rows x 64 columns of g_C and of op(A) through LDS with coalesced 16-byte loads and reads
// the v_mfma_f32_16x16x4_f32 fragments transposed from there (ds_read_b32, lane = (row & 3, column): the row stride of 80
// floats puts the two rows of a 32-lane group 16 banks apart -- conflict-free).  Wave w accumulates out rows 16 w .. 16 w + 15
// against the four 16-column tiles of `in`.  M is 900 .. 4500 for TransHE: 4 .. 18 chunks x 9 .. 36 tiles cover the chip;
// the chunk count depends on M alone.  Every chunk writes its partial tile (and, from the in-tile-0 workgroups, its partial
// bias sums) to the workspace and reduce_kernel adds the partials IN CHUNK ORDER: no atomics, the result does not depend on
// scheduling.  LayerNorm's parameter gradients take the same two stages (ln_bwd_kernel's per-block column sums).
//
// A ReLU on the output: Y = relu(A W^T + b) is th_gemm's TH_ACT_RELU epilogue; the backward is form 0 with g_C = g_Y * [Y > 0]
// (torch's rule: 0 at Y == 0), gated on g_Y's way into LDS in wgrad_kernel<OP_PLAIN, true> and by one elementwise pass into the
// workspace (relu_gate_kernel) for the input gradient.
#include <algorithm>

#include "th_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WG_CHUNK 256       // rows per partial tile (th_wgrad_chunk_rows)
#define WG_ROWS 64         // rows staged per LDS fill
#define WG_TILE 64
#define WG_STRIDE 80       // floats per LDS row: 80 mod 32 = 16
#define LN_ROWS 64         // rows per block of ln_bwd_kernel (th_layernorm_bwd_chunk_rows)

enum { OP_PLAIN = 0, OP_LN = 1, OP_GELU = 2 };

__device__ __forceinline__ float vd_gelu_erf(float x) {      // th_gelu_erf of k_gemm.hip
    return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
}

// d/du gelu(u) = Phi(u) + u phi(u), exact erf
__device__ __forceinline__ float vd_gelu_grad(float u) {
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * u * u) * 0.39894228040143267794f;
    return cdf + u * pdf;
}

// pack_linear_kernel on W^T: the layer n' = input column, k' = output row, no bias
__global__ void pack_linear_t_kernel(const float* __restrict__ W, int out_f, int in_f, int NB, int KB,
                                     float* __restrict__ wp, float* __restrict__ bp) {
    long long total = (long long)NB * KB * 256;
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < total;
         o += (long long)gridDim.x * blockDim.x) {
        int e = (int)(o & 3);
        int lane = (int)((o >> 2) & 63);
        long long blk = o >> 8;
        int kb = (int)(blk % KB);
        int nb = (int)(blk / KB);
        int n = nb * 16 + (lane & 15);
        int k = kb * 16 + 4 * (lane >> 4) + e;
        wp[o] = (n < in_f && k < out_f) ? W[(long long)k * in_f + n] : 0.0f;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < NB * 16; i += gridDim.x * blockDim.x) bp[i] = 0.0f;
}

// The row statistics of th_gemm_ln's prologue (k_gemm.hip): 16 lanes per row, lane `sub` holds columns 4 (sub + 16 q) + e,
// two passes.  x == nullptr stands for a row past the end (all zeros).  Every lane of the 16 gets mean and rstd.
__device__ __forceinline__ void vd_row_stats(const float* __restrict__ x, int sub, int K, float eps, float (&v)[16],
                                             float& mean, float& rstd) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = 4 * (sub + 16 * q);
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x != nullptr && k < K) t = *reinterpret_cast<const float4*>(x + k);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        sum += (t.x + t.y) + (t.z + t.w);
    }
    sum = th_row16_sum(sum);
    mean = sum / (float)K;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = 4 * (sub + 16 * q);
        if (k < K) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { float d = v[4 * q + e] - mean; ss += d * d; }
        }
    }
    ss = th_row16_sum(ss);
    rstd = 1.0f / __fsqrt_rn(ss / (float)K + eps);
}

__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ X, int ldx, int M, int K, float eps,
                                                       float* __restrict__ stats) {
    const int gm = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    float v[16], mean, rstd;
    vd_row_stats(gm < M ? X + (long long)gm * ldx : nullptr, sub, K, eps, v, mean, rstd);
    if (sub == 0 && gm < M) { stats[2 * gm] = mean; stats[2 * gm + 1] = rstd; }
}

// o = LN(x): the operand th_gemm_ln multiplies, written out (the final norm of the ViT)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ X, int ldx, int M, int K,
                                                     const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                     float* __restrict__ O, int ldo) {
    const int gm = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    float v[16], mean, rstd;
    vd_row_stats(gm < M ? X + (long long)gm * ldx : nullptr, sub, K, eps, v, mean, rstd);
    if (gm >= M) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = 4 * (sub + 16 * q);
        if (k < K) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + k), b4 = *reinterpret_cast<const float4*>(b + k);
            float4 o;
            o.x = (v[4 * q] - mean) * rstd * w4.x + b4.x;
            o.y = (v[4 * q + 1] - mean) * rstd * w4.y + b4.y;
            o.z = (v[4 * q + 2] - mean) * rstd * w4.z + b4.z;
            o.w = (v[4 * q + 3] - mean) * rstd * w4.w + b4.w;
            *reinterpret_cast<float4*>(O + (long long)gm * ldo + k) = o;
        }
    }
}

// LayerNorm backward, 16 lanes per row, LN_ROWS rows per block (4 passes of 16):
//   xh = (x - mean) rstd,  gw = g w,  g_x = rstd (gw - mean(gw) - xh mean(gw xh))
// G and GX may be the same buffer (every lane reads its own elements of a row before it writes them).
// part[block][0][K] = sum over the block's rows of g xh, part[block][1][K] = sum of g: rows in ascending order (a lane adds its
// passes in order, then one thread per column adds the 16 row groups in order).
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ X, int ldx, int M, int K,
                                                     const float* __restrict__ w, float eps, const float* G, int ldg,
                                                     float* GX, int ldgx, float* __restrict__ part) {
    __shared__ float red[2][16][256];
    const int tid = threadIdx.x, rg = tid >> 4, sub = tid & 15;
    float wv[16], aw[16], ab[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = 4 * (sub + 16 * q);
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < K) t = *reinterpret_cast<const float4*>(w + k);
        wv[4 * q] = t.x; wv[4 * q + 1] = t.y; wv[4 * q + 2] = t.z; wv[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) { aw[j] = 0.f; ab[j] = 0.f; }
    // pass p holds rows 16 p + rg of the block: row groups hold interleaved rows, summed below as (p, rg) pairs in a fixed order
    for (int p = 0; p < LN_ROWS / 16; ++p) {
        const int gm = blockIdx.x * LN_ROWS + 16 * p + rg;
        const bool live = gm < M;
        float v[16], g[16], mean, rstd;
        vd_row_stats(live ? X + (long long)gm * ldx : nullptr, sub, K, eps, v, mean, rstd);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * (sub + 16 * q);
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && k < K) t = *reinterpret_cast<const float4*>(G + (long long)gm * ldg + k);
            g[4 * q] = t.x; g[4 * q + 1] = t.y; g[4 * q + 2] = t.z; g[4 * q + 3] = t.w;
        }
        float xh[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = live && 4 * (sub + 16 * (j >> 2)) < K;       // (a row past the end adds exact zeros)
            xh[j] = in ? (v[j] - mean) * rstd : 0.f;
            const float gw = g[j] * wv[j];
            s1 += gw;
            s2 += gw * xh[j];
            aw[j] += g[j] * xh[j];
            ab[j] += g[j];
        }
        s1 = th_row16_sum(s1);
        s2 = th_row16_sum(s2);
        const float m1 = s1 / (float)K, m2 = s2 / (float)K;
        if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * (sub + 16 * q);
                if (k < K) {
                    float4 o;
                    o.x = rstd * (g[4 * q] * wv[4 * q] - m1 - xh[4 * q] * m2);
                    o.y = rstd * (g[4 * q + 1] * wv[4 * q + 1] - m1 - xh[4 * q + 1] * m2);
                    o.z = rstd * (g[4 * q + 2] * wv[4 * q + 2] - m1 - xh[4 * q + 2] * m2);
                    o.w = rstd * (g[4 * q + 3] * wv[4 * q + 3] - m1 - xh[4 * q + 3] * m2);
                    *reinterpret_cast<float4*>(GX + (long long)gm * ldgx + k) = o;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = 4 * (sub + 16 * (j >> 2)) + (j & 3);
        red[0][rg][k] = aw[j];
        red[1][rg][k] = ab[j];
    }
    __syncthreads();
    if (tid < K) {
        float a = red[0][0][tid], b = red[1][0][tid];
        for (int r = 1; r < 16; ++r) { a += red[0][r][tid]; b += red[1][r][tid]; }
        part[(long long)blockIdx.x * 2 * K + tid] = a;
        part[(long long)blockIdx.x * 2 * K + K + tid] = b;
    }
}

// g[m, :] *= gelu'(u[m, :]) in place (rows of n floats, n % 4 == 0)
__global__ void gelu_bwd_kernel(const float* __restrict__ U, int ldu, float* __restrict__ G, int ldg, int M, int n) {
    const int n4 = n >> 2;
    const long long total = (long long)M * n4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / n4;
        const int c = 4 * (int)(i - m * n4);
        const float4 u = *reinterpret_cast<const float4*>(U + m * ldu + c);
        float4 g = *reinterpret_cast<float4*>(G + m * ldg + c);
        g.x *= vd_gelu_grad(u.x); g.y *= vd_gelu_grad(u.y); g.z *= vd_gelu_grad(u.z); g.w *= vd_gelu_grad(u.w);
        *reinterpret_cast<float4*>(G + m * ldg + c) = g;
    }
}

// G'[m, :] = G[m, :] * [Y[m, :] > 0] (dense G', n % 4 == 0)
__global__ void relu_gate_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ Y, int ldy, int M, int n,
                                 float* __restrict__ O) {
    const int n4 = n >> 2;
    const long long total = (long long)M * n4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / n4;
        const int c = 4 * (int)(i - m * n4);
        const float4 y = *reinterpret_cast<const float4*>(Y + m * ldy + c);
        float4 g = *reinterpret_cast<const float4*>(G + m * ldg + c);
        g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f;
        g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
        *reinterpret_cast<float4*>(O + m * n + c) = g;
    }
}

// o[m, :] = gelu(u[m, :]) (dense o, n % 4 == 0): fc2's input in the forward
__global__ void gelu_fwd_kernel(const float* __restrict__ U, int ldu, float* __restrict__ O, int M, int n) {
    const int n4 = n >> 2;
    const long long total = (long long)M * n4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / n4;
        const int c = 4 * (int)(i - m * n4);
        const float4 u = *reinterpret_cast<const float4*>(U + m * ldu + c);
        float4 o;
        o.x = vd_gelu_erf(u.x); o.y = vd_gelu_erf(u.y); o.z = vd_gelu_erf(u.z); o.w = vd_gelu_erf(u.w);
        *reinterpret_cast<float4*>(O + m * n + c) = o;
    }
}

// grid (ceil(out / 64), ceil(in / 64), chunks); part[chunk][out in + out]
// GATE (the layers with a ReLU on their output): g_C = G * [Y > 0], applied on G's way into LDS
template <int FORM, bool GATE = false>
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ A,
                                                    int lda, int M, int out_f, int in_f, const float* __restrict__ stats,
                                                    const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                    float* __restrict__ part, const float* __restrict__ Y, int ldy) {
    __shared__ __attribute__((aligned(16))) float Gs[WG_ROWS * WG_STRIDE];
    __shared__ __attribute__((aligned(16))) float As[WG_ROWS * WG_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * WG_TILE, i0 = blockIdx.y * WG_TILE;
    const int m_lo = blockIdx.z * WG_CHUNK;
    const int m_hi = min(M, m_lo + WG_CHUNK);
    const bool bias_wg = blockIdx.y == 0;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int mb = m_lo; mb < m_hi; mb += WG_ROWS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 4, c = 4 * (idx & 15), gm = mb + row;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f), a = g;
            if (gm < m_hi) {
                if (o0 + c < out_f) g = *reinterpret_cast<const float4*>(G + (long long)gm * ldg + o0 + c);
                if (GATE && o0 + c < out_f) {
                    const float4 y = *reinterpret_cast<const float4*>(Y + (long long)gm * ldy + o0 + c);
                    g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f;
                    g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
                }
                if (i0 + c < in_f) {
                    a = *reinterpret_cast<const float4*>(A + (long long)gm * lda + i0 + c);
                    if (FORM == OP_LN) {
                        const float mu = stats[2 * gm], rs = stats[2 * gm + 1];
                        const float4 w4 = *reinterpret_cast<const float4*>(ln_w + i0 + c);
                        const float4 b4 = *reinterpret_cast<const float4*>(ln_b + i0 + c);
                        a.x = (a.x - mu) * rs * w4.x + b4.x;
                        a.y = (a.y - mu) * rs * w4.y + b4.y;
                        a.z = (a.z - mu) * rs * w4.z + b4.z;
                        a.w = (a.w - mu) * rs * w4.w + b4.w;
                    } else if (FORM == OP_GELU) {
                        a.x = vd_gelu_erf(a.x); a.y = vd_gelu_erf(a.y); a.z = vd_gelu_erf(a.z); a.w = vd_gelu_erf(a.w);
                    }
                }
            }
            *reinterpret_cast<float4*>(&Gs[row * WG_STRIDE + c]) = g;
            *reinterpret_cast<float4*>(&As[row * WG_STRIDE + c]) = a;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < WG_ROWS / 4; ++kk) {
            const int r = 4 * kk + (lane >> 4);
            const float ga = Gs[r * WG_STRIDE + 16 * wave + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, As[r * WG_STRIDE + 16 * j + (lane & 15)], acc[j], 0, 0, 0);
        }
        if (bias_wg && tid < WG_TILE) {
            // blocked, not one chain over the chunk: four sums of 16 rows, paired, then onto the chunk's sum (a column of g_C has
            // no products to average its rounding out: one 256-term chain sat at the bar of the tests)
            float q[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                q[h] = 0.f;
                for (int r = 0; r < WG_ROWS / 4; ++r) q[h] += Gs[(16 * h + r) * WG_STRIDE + tid];
            }
            bsum += (q[0] + q[1]) + (q[2] + q[3]);
        }
        __syncthreads();
    }
    float* dst = part + (long long)blockIdx.z * ((long long)out_f * in_f + out_f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = i0 + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = o0 + 16 * wave + 4 * (lane >> 4) + r;
            if (row < out_f && col < in_f) dst[(long long)row * in_f + col] = acc[j][r];
        }
    }
    if (bias_wg && tid < WG_TILE && o0 + tid < out_f) dst[(long long)out_f * in_f + o0 + tid] = bsum;
}

// d[i] = part[0][i] + part[1][i] + ... in chunk order; element i < n1 goes to d1, the rest to d2 (either may be null)
__global__ void reduce_kernel(const float* __restrict__ part, int chunks, long long stride, long long n1, long long n,
                              float* __restrict__ d1, float* __restrict__ d2) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int c = 1; c < chunks; ++c) s += part[c * stride + i];
    if (i < n1) { if (d1) d1[i] = s; }
    else if (d2) d2[i - n1] = s;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static bool vd_shape_ok(int M, int out_f, int in_f, int form) {
    if (M < 1 || M > (1 << 24) || out_f < 16 || in_f < 16 || (out_f & 15) || (in_f & 15) || out_f > 65536 || in_f > 65536)
        return false;
    if (form == OP_LN) return in_f <= 256 && M <= 8192;        // (th_gemm_ln's range)
    return form == OP_PLAIN || form == OP_GELU;
}
static bool vd_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static int vd_chunks(int M) { return th_cdiv(M, WG_CHUNK); }
static int vd_ln_blocks(int M) { return th_cdiv(M, LN_ROWS); }
static unsigned vd_grid4(int M, int n) { return (unsigned)std::min<long long>(((long long)M * (n >> 2) + 255) / 256, 8192); }

#define VD_SHAPE_MSG "unsupported shape: M >= 1, in_f and out_f multiples of 16; form 1 (LayerNorm) also in_f <= 256, M <= 8192"
#define VD_FORM_MSG "form must be 0 (A), 1 (LayerNorm(A)) or 2 (gelu(A))"

// the backward's workspace: the image of W^T, then -- each only where the layer has it -- the gated g_Y (a ReLU on the output),
// the row statistics (LayerNorm), wgrad_kernel's partial tiles, ln_bwd_kernel's partial column sums (LayerNorm)
struct VdBwdWs { size_t pack, gate, stats, part, lnpart, total; };
static VdBwdWs vd_bwd_layout(int M, int out_f, int in_f, int form, int act) {
    VdBwdWs w{};
    w.pack = 0;
    size_t off = ThPacked::bytes(in_f, out_f);
    w.gate = off;
    if (act == TH_ACT_RELU) off += th_align((size_t)M * out_f * sizeof(float));
    w.stats = off;
    if (form == OP_LN) off += th_align((size_t)M * 2 * sizeof(float));
    w.part = off;
    off += th_align((size_t)vd_chunks(M) * ((size_t)out_f * in_f + out_f) * sizeof(float));
    w.lnpart = off;
    if (form == OP_LN) off += th_align((size_t)vd_ln_blocks(M) * 2 * in_f * sizeof(float));
    w.total = off;
    return w;
}

// the image of W^T for the input gradient (storage: ThPacked::bytes(in_f, out_f))
static int vd_pack_linear_t(const float* W, int out_f, int in_f, void* storage, ThPacked* P, hipStream_t s) {
    P->N = in_f; P->K = out_f; P->NB = in_f / 16; P->KB = out_f / 16;
    P->w = (float*)storage;
    P->b = (float*)((char*)storage + th_align((size_t)P->NB * P->KB * 256 * sizeof(float)));
    const long long total = (long long)P->NB * P->KB * 256;
    hipLaunchKernelGGL(pack_linear_t_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0, s, W,
                       out_f, in_f, P->NB, P->KB, P->w, P->b);
    TH_LAUNCH_CHECK();
    return 0;
}

static int vd_ln_bwd_launch(const float* x, int ldx, int M, int dim, const float* w, float eps, const float* g, int ldg,
                            float* gx, int ldgx, float* g_w, float* g_b, float* part, hipStream_t s) {
    const int blocks = vd_ln_blocks(M);
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, M, dim, w, eps, g, ldg, gx, ldgx, part);
    hipLaunchKernelGGL(reduce_kernel, dim3(th_cdiv(2 * dim, 256)), dim3(256), 0, s, part, blocks, (long long)2 * dim,
                       (long long)dim, (long long)2 * dim, g_w, g_b);
    TH_LAUNCH_CHECK();
    return 0;
}

// the forward's workspace: the packed layer, and for form 2 the GELU of the input rows [M, in_f]
struct VdFwdWs { void* pack; float* gelu; };
static VdFwdWs vd_fwd_layout(ThArena& ar, int M, int out_f, int in_f, int form) {
    return {ar.take<char>(ThPacked::bytes(out_f, in_f)), form == OP_GELU ? ar.take<float>((size_t)M * in_f) : nullptr};
}
// the partial column sums of th_layernorm_bwd: [blocks][2][dim]
static float* vd_ln_bwd_layout(ThArena& ar, int M, int dim) { return ar.take<float>((size_t)vd_ln_blocks(M) * 2 * dim); }

// C = act(op(A) W^T + b): the one forward behind th_linear_train_forward (act = TH_ACT_NONE) and th_linear_relu_forward
// (form 0, act = TH_ACT_RELU in the GEMM's epilogue)
static int vd_forward(th_ctx* c, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b, float ln_eps,
                      const th_linear* lin, int act, float* C, int ldc, void* ws, size_t ws_bytes, th_stream stream) {
    TH_REQUIRE(c && A && lin && C && ws, "null argument");
    TH_REQUIRE(lin->w != nullptr, "null argument (the layer's weight)");
    TH_REQUIRE(form >= OP_PLAIN && form <= OP_GELU && (act == TH_ACT_NONE || form == OP_PLAIN), VD_FORM_MSG);
    TH_REQUIRE(form != OP_LN || (ln_w && ln_b), "null argument (LayerNorm parameters of form 1)");
    TH_REQUIRE(vd_shape_ok(M, lin->out_f, lin->in_f, form), VD_SHAPE_MSG);
    TH_REQUIRE(lda >= lin->in_f && ldc >= lin->out_f && (lda & 3) == 0 && (ldc & 3) == 0,
               "lda / ldc (ldy): >= the row, multiples of 4");
    TH_REQUIRE(vd_al16(A) && vd_al16(C) && vd_al16(ws) && vd_al16(lin->w) && (form != OP_LN || (vd_al16(ln_w) && vd_al16(ln_b))),
               "pointers must be 16-byte aligned");
    ThArena ar(ws, ws_bytes);
    VdFwdWs w = vd_fwd_layout(ar, M, lin->out_f, lin->in_f, form);
    TH_REQUIRE(ar.ok(), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ThPacked P;
    TH_TRY(th_pack_linear(*lin, w.pack, &P, s));
    if (form == OP_LN) return th_gemm_ln(A, lda, M, P, ln_w, ln_b, ln_eps, TH_ACT_NONE, C, ldc, s);
    if (form == OP_GELU) {
        float* t = w.gelu;
        hipLaunchKernelGGL(gelu_fwd_kernel, dim3(vd_grid4(M, lin->in_f)), dim3(256), 0, s, A, lda, t, M, lin->in_f);
        TH_LAUNCH_CHECK();
        return th_gemm(t, lin->in_f, M, P, TH_ACT_NONE, C, ldc, s);
    }
    return th_gemm(A, lda, M, P, act, C, ldc, s);
}

// the one backward behind th_linear_bwd (act = TH_ACT_NONE, Y unused) and th_linear_relu_bwd (form 0, act = TH_ACT_RELU, Y the
// forward's output: g_C = g_Y * [Y > 0]).  Launches: [row statistics] -> ([gate] -> pack W^T -> th_gemm -> [gelu' | LN bwd]) ->
// wgrad_kernel -> reduce_kernel
static int vd_backward(th_ctx* c, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b, float ln_eps,
                       const th_linear* lin, int act, const float* Y, int ldy, const float* g_C, int ldg, float* g_A, int ldga,
                       float* g_W, float* g_b, float* g_ln_w, float* g_ln_b, void* ws, size_t ws_bytes, th_stream stream) {
    const bool gate = act == TH_ACT_RELU;
    TH_REQUIRE(c && A && lin && g_C && g_W && ws && (!gate || Y), "null argument");
    TH_REQUIRE(lin->w != nullptr, "null argument (the layer's weight)");
    TH_REQUIRE(form >= OP_PLAIN && form <= OP_GELU && (!gate || form == OP_PLAIN), VD_FORM_MSG);
    TH_REQUIRE(form != OP_LN || (ln_w && ln_b), "null argument (LayerNorm parameters of form 1)");
    TH_REQUIRE(form != OP_LN || g_A == nullptr || (g_ln_w && g_ln_b), "null argument (g_ln_w / g_ln_b go with g_A in form 1)");
    const int out_f = lin->out_f, in_f = lin->in_f;
    TH_REQUIRE(vd_shape_ok(M, out_f, in_f, form), VD_SHAPE_MSG);
    TH_REQUIRE(lda >= in_f && ldg >= out_f && (lda & 3) == 0 && (ldg & 3) == 0 && (!gate || (ldy >= out_f && (ldy & 3) == 0)) &&
                   (g_A == nullptr || (ldga >= in_f && (ldga & 3) == 0)),
               "lda / ldy / ldg / ldga: >= the row, multiples of 4");
    TH_REQUIRE(vd_al16(A) && (!gate || vd_al16(Y)) && vd_al16(g_C) && vd_al16(g_A) && vd_al16(g_W) && vd_al16(ws) &&
                   vd_al16(lin->w) && (form != OP_LN || (vd_al16(ln_w) && vd_al16(ln_b))),
               "pointers must be 16-byte aligned");
    const VdBwdWs L = vd_bwd_layout(M, out_f, in_f, form, act);
    TH_REQUIRE(ws_bytes >= L.total, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float* stats = (float*)(base + L.stats);
    float* part = (float*)(base + L.part);
    if (form == OP_LN) {
        hipLaunchKernelGGL(ln_stats_kernel, dim3(th_cdiv(M, 16)), dim3(256), 0, s, A, lda, M, in_f, ln_eps, stats);
        TH_LAUNCH_CHECK();
    }
    if (g_A != nullptr) {
        const float* g = g_C;
        int ld = ldg;
        if (gate) {
            float* gated = (float*)(base + L.gate);
            hipLaunchKernelGGL(relu_gate_kernel, dim3(vd_grid4(M, out_f)), dim3(256), 0, s, g_C, ldg, Y, ldy, M, out_f, gated);
            TH_LAUNCH_CHECK();
            g = gated;
            ld = out_f;
        }
        ThPacked P;
        TH_TRY(vd_pack_linear_t(lin->w, out_f, in_f, base + L.pack, &P, s));
        TH_TRY(th_gemm(g, ld, M, P, TH_ACT_NONE, g_A, ldga, s));
        if (form == OP_GELU) {
            hipLaunchKernelGGL(gelu_bwd_kernel, dim3(vd_grid4(M, in_f)), dim3(256), 0, s, A, lda, g_A, ldga, M, in_f);
            TH_LAUNCH_CHECK();
        } else if (form == OP_LN) {
            TH_TRY(vd_ln_bwd_launch(A, lda, M, in_f, ln_w, ln_eps, g_A, ldga, g_A, ldga, g_ln_w, g_ln_b,
                                    (float*)(base + L.lnpart), s));
        }
    }
    const int chunks = vd_chunks(M);
    dim3 grid(th_cdiv(out_f, WG_TILE), th_cdiv(in_f, WG_TILE), chunks);
    if (form == OP_LN)
        hipLaunchKernelGGL(wgrad_kernel<OP_LN>, grid, dim3(256), 0, s, g_C, ldg, A, lda, M, out_f, in_f, stats, ln_w, ln_b, part,
                           nullptr, 0);
    else if (form == OP_GELU)
        hipLaunchKernelGGL(wgrad_kernel<OP_GELU>, grid, dim3(256), 0, s, g_C, ldg, A, lda, M, out_f, in_f, nullptr, nullptr,
                           nullptr, part, nullptr, 0);
    else if (gate)
        hipLaunchKernelGGL((wgrad_kernel<OP_PLAIN, true>), grid, dim3(256), 0, s, g_C, ldg, A, lda, M, out_f, in_f, nullptr, nullptr,
                           nullptr, part, Y, ldy);
    else
        hipLaunchKernelGGL(wgrad_kernel<OP_PLAIN>, grid, dim3(256), 0, s, g_C, ldg, A, lda, M, out_f, in_f, nullptr, nullptr,
                           nullptr, part, nullptr, 0);
    const long long n1 = (long long)out_f * in_f, n = n1 + out_f;
    hipLaunchKernelGGL(reduce_kernel, dim3(th_cdiv(n, 256)), dim3(256), 0, s, part, chunks, n, n1, n, g_W, g_b);
    TH_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int th_wgrad_chunk_rows(void) { return WG_CHUNK; }
int th_layernorm_bwd_chunk_rows(void) { return LN_ROWS; }

size_t th_linear_train_workspace_bytes(int M, int out_f, int in_f, int form) {
    return vd_shape_ok(M, out_f, in_f, form) ? th_measure(vd_fwd_layout, M, out_f, in_f, form) : 0;
}

int th_linear_train_forward(th_ctx* c, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b,
                            float ln_eps, const th_linear* lin, float* C, int ldc, void* ws, size_t ws_bytes,
                            th_stream stream) {
    return vd_forward(c, A, lda, M, form, ln_w, ln_b, ln_eps, lin, TH_ACT_NONE, C, ldc, ws, ws_bytes, stream);
}

size_t th_linear_bwd_workspace_bytes(int M, int out_f, int in_f, int form) {
    if (!vd_shape_ok(M, out_f, in_f, form)) return 0;
    return vd_bwd_layout(M, out_f, in_f, form, TH_ACT_NONE).total;
}

int th_linear_bwd(th_ctx* c, const float* A, int lda, int M, int form, const float* ln_w, const float* ln_b, float ln_eps,
                  const th_linear* lin, const float* g_C, int ldg, float* g_A, int ldga, float* g_W, float* g_b,
                  float* g_ln_w, float* g_ln_b, void* ws, size_t ws_bytes, th_stream stream) {
    return vd_backward(c, A, lda, M, form, ln_w, ln_b, ln_eps, lin, TH_ACT_NONE, nullptr, 0, g_C, ldg, g_A, ldga, g_W, g_b,
                       g_ln_w, g_ln_b, ws, ws_bytes, stream);
}

// the same layer with a ReLU on its output (K20): form 0 of the bodies above
size_t th_linear_relu_workspace_bytes(int M, int out_f, int in_f) {
    return th_linear_train_workspace_bytes(M, out_f, in_f, OP_PLAIN);
}

int th_linear_relu_forward(th_ctx* c, const float* A, int lda, int M, const th_linear* lin, float* Y, int ldy, void* ws,
                           size_t ws_bytes, th_stream stream) {
    return vd_forward(c, A, lda, M, OP_PLAIN, nullptr, nullptr, 0.f, lin, TH_ACT_RELU, Y, ldy, ws, ws_bytes, stream);
}

size_t th_linear_relu_bwd_workspace_bytes(int M, int out_f, int in_f) {
    if (!vd_shape_ok(M, out_f, in_f, OP_PLAIN)) return 0;
    return vd_bwd_layout(M, out_f, in_f, OP_PLAIN, TH_ACT_RELU).total;
}

int th_linear_relu_bwd(th_ctx* c, const float* A, int lda, const float* Y, int ldy, int M, const th_linear* lin, const float* g_Y,
                       int ldg, float* g_A, int ldga, float* g_W, float* g_b, void* ws, size_t ws_bytes, th_stream stream) {
    return vd_backward(c, A, lda, M, OP_PLAIN, nullptr, nullptr, 0.f, lin, TH_ACT_RELU, Y, ldy, g_Y, ldg, g_A, ldga, g_W, g_b,
                       nullptr, nullptr, ws, ws_bytes, stream);
}

int th_layernorm_forward(th_ctx* c, const float* x, int ldx, int M, int dim, const float* w, const float* b, float eps,
                         float* out, int ldo, th_stream stream) {
    TH_REQUIRE(c && x && w && b && out, "null argument");
    TH_REQUIRE(M >= 1 && M <= (1 << 24) && dim >= 16 && dim <= 256 && (dim & 15) == 0,
               "unsupported shape: M >= 1, dim a multiple of 16 up to 256");
    TH_REQUIRE(ldx >= dim && ldo >= dim && (ldx & 3) == 0 && (ldo & 3) == 0, "ldx / ldo: >= dim, multiples of 4");
    TH_REQUIRE(vd_al16(x) && vd_al16(w) && vd_al16(b) && vd_al16(out), "pointers must be 16-byte aligned");
    hipLaunchKernelGGL(ln_fwd_kernel, dim3(th_cdiv(M, 16)), dim3(256), 0, (hipStream_t)stream, x, ldx, M, dim, w, b, eps, out, ldo);
    TH_LAUNCH_CHECK();
    return 0;
}

size_t th_layernorm_bwd_workspace_bytes(int M, int dim) {
    return (M < 1 || M > (1 << 24) || dim < 16 || dim > 256 || (dim & 15)) ? 0 : th_measure(vd_ln_bwd_layout, M, dim);
}

int th_layernorm_bwd(th_ctx* c, const float* x, int ldx, int M, int dim, const float* w, float eps, const float* g, int ldg,
                     float* g_x, int ldgx, float* g_w, float* g_b, void* ws, size_t ws_bytes, th_stream stream) {
    TH_REQUIRE(c && x && w && g && g_x && g_w && g_b && ws, "null argument");
    TH_REQUIRE(M >= 1 && M <= (1 << 24) && dim >= 16 && dim <= 256 && (dim & 15) == 0,
               "unsupported shape: M >= 1, dim a multiple of 16 up to 256");
    TH_REQUIRE(ldx >= dim && ldg >= dim && ldgx >= dim && (ldx & 3) == 0 && (ldg & 3) == 0 && (ldgx & 3) == 0,
               "ldx / ldg / ldgx: >= dim, multiples of 4");
    TH_REQUIRE(vd_al16(x) && vd_al16(w) && vd_al16(g) && vd_al16(g_x) && vd_al16(ws), "pointers must be 16-byte aligned");
    ThArena ar(ws, ws_bytes);
    float* part = vd_ln_bwd_layout(ar, M, dim);
    TH_REQUIRE(ar.ok(), "workspace too small");
    return vd_ln_bwd_launch(x, ldx, M, dim, w, eps, g, ldg, g_x, ldgx, g_w, g_b, part, (hipStream_t)stream);
}

}  // extern "C"
