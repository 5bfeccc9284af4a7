// K3, training form: the backward of one TransHE layer's attention, softmax(q k^T / 8) v per (view, head).
//
// Flash-style like the forward: the [V, heads, N, N] probabilities are never stored.  The forward (k_vit.hip, the LSE = true
// instantiations of attn2_kernel / attn3_kernel) leaves each row's log-sum-exp; here every tile of P is recomputed from it:
//
//     P_ij  = exp(s q_i.k_j - lse_i),  s = 1/8
//     D_i   = sum_d g_out[i,d] out[i,d] = sum_j P_ij dP_ij     (the second form, from the kernels' own P: see attn_bwd_dq_kernel)
//     dV_j  = sum_i P_ij g_out_i
//     dP_ij = g_out_i . v_j
//     dS_ij = P_ij (dP_ij - D_i)
//     dQ_i  = s sum_j dS_ij k_j                        (attn_bwd_dq_kernel:  one query tile, loop over key tiles)
//     dK_j  = s sum_i dS_ij q_i                        (attn_bwd_dkv_kernel: one key tile, loop over query tiles)
//
// No atomics: every output element is summed by one wave in one fixed order, so two runs agree bit for bit.  Each of the two
// kernels recomputes S and dP of its own tiles (9 products of N^2 x 64 in all, two of them for the row constants).
//
// All products run on v_mfma_f32_16x16x4_f32: fp32 operands, an exact fp32 fma chain, no operand range to guard (g_out may be
// anything fp32 holds).  Lane l = 16 g + c supplies A[row c][k g] and B[k g][column c]; the result sits at column c, rows
// 4 g + r.  Two things follow:
//  * the 64-long sums over d run as 4 blocks of 4 steps with step (blk, kk) summing d = 16 blk + 4 g + kk on lane group g --
//    a permutation of the summation index, the same on both operands -- so a lane fetches its 4 steps of a block as ONE float4;
//  * S and dP are formed with the index that the NEXT product sums over on the result's rows (keys for dQ: S^T = K Q^T;
//    queries for dK / dV: S = Q K^T): register r of lane (c, g) is then exactly the A operand of step r of that product
//    (k index g <-> row 4 g + r), with no LDS round trip and no cross-lane traffic.
// One workgroup = 4 waves = 64 rows of the kernel's own side; 64-row tiles of the other side are staged through LDS as fp32
// (rows padded to 68 floats: the float4 row reads and the scalar column reads are both conflict-free) and shared by the waves.
// Rows at index >= N are staged as zeros and P is masked by index, so they add exactly nothing.
//
// N = 1 is the degenerate softmax: P = 1 whatever the logit and dS = 0 identically, so dQ = dK = 0 and dV = g_out EXACTLY.
// The general path would get there only up to the rounding of exp(s q.k - lse); attn_bwd_single_kernel writes the exact result.

#include "th_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define AB_T 64                 // rows of a tile
#define AB_LD 68                // floats per LDS row (64 + 4: 272 B, keeps float4 alignment)

__device__ __forceinline__ float4 ab_load4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// one 64-row tile of two [.., 64] fp32 operands into LDS; rows >= N as zeros
__device__ __forceinline__ void ab_stage(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                         int r0, int N, float* As, float* Bs, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 4, c4 = idx & 15, gr = r0 + row;
        const bool ok = gr < N;
        const long long rr = ok ? gr : 0;
        *reinterpret_cast<float4*>(As + row * AB_LD + 4 * c4) = ab_load4(a + rr * lda + 4 * c4, ok);
        *reinterpret_cast<float4*>(Bs + row * AB_LD + 4 * c4) = ab_load4(b + rr * ldb + 4 * c4, ok);
    }
}

// this lane's operand fragments of row `row` of a [.., 64] fp32 matrix: f[blk] = d 16 blk + 4 g .. + 3
__device__ __forceinline__ void ab_row_frags(const float* __restrict__ p, bool ok, int g, float4 f[4]) {
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) f[blk] = ab_load4(p + 16 * blk + 4 * g, ok);
}

__device__ __forceinline__ float ab_e(const float4& v, int kk) { return kk == 0 ? v.x : kk == 1 ? v.y : kk == 2 ? v.z : v.w; }

// dQ: workgroup = 64 queries (wave w: 16 of them, one per lane column c), two sweeps over the 64-key tiles of K and V in LDS.
// Sweep 0 is the prologue that makes the row constants from THIS kernel's probabilities p_ij = exp(s q_i.k_j - lse_i):
//     l_i = sum_j p_ij          (1 up to the few 2^-22 by which the forward's logits differ from the fp32 ones here)
//     D_i = sum_j p_ij dP_ij / l_i
// written to the workspace as 1 / l_i and D_i for attn_bwd_dkv_kernel.  Sweep 1 forms dS_ij = (p_ij / l_i)(dP_ij - D_i) and
// dQ.  With these constants sum_j dS_ij = 0 holds to the rounding of the sums themselves, as in an fp32 evaluation of the
// softmax backward; with D_i = g_out_i . out_i and the forward's lse taken as exact it holds only to the forward's operand
// precision, and dQ_i = s sum_j dS_ij k_j multiplies what is left by |k| (measured: 50 x the fp32 error where all keys are
// long and parallel).  `lse` thereby only centres the exponent; `out` is not read.
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ g_out,
                                                          const float* __restrict__ lse, int N, int dim, float scale,
                                                          float* __restrict__ inv_l, float* __restrict__ D,
                                                          float* __restrict__ g_qkv) {
    __shared__ __attribute__((aligned(16))) float Ks[AB_T * AB_LD];
    __shared__ __attribute__((aligned(16))) float Vs[AB_T * AB_LD];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = blockIdx.y, view = blockIdx.z, heads = gridDim.y;
    const int ld = 3 * dim;
    const float* base = qkv + (long long)view * N * ld + head * 64;
    const int qb = blockIdx.x * AB_T + wave * 16, qi = qb + c;
    const bool qok = qi < N;

    float4 qf[4], dof[4];       // B operands of S^T = K Q^T and dP^T = V dO^T: column = query c
    ab_row_frags(base + (long long)(qok ? qi : 0) * ld, qok, g, qf);
    ab_row_frags(g_out + ((long long)view * N + (qok ? qi : 0)) * dim + head * 64, qok, g, dof);
    const long long so = ((long long)view * heads + head) * N + (qok ? qi : 0);
    const float lse_c = qok ? lse[so] : 0.f;
    float lsum = 0.f, dsum = 0.f, inv_c = 0.f, D_c = 0.f;

    f32x4 dq[4];                // dQ tiles: row = query qb + 4 g + r, column = d 16 jd + c
#pragma unroll
    for (int j = 0; j < 4; ++j) dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int k0 = 0; k0 < N; k0 += AB_T) {
            __syncthreads();        // everybody is done with the previous tile
            ab_stage(base + dim, ld, base + 2 * dim, ld, k0, N, Ks, Vs, tid);
            __syncthreads();
            if (qb >= N) continue;  // (wave-uniform; the wave still stages its share)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                f32x4 sacc = (f32x4){0.f, 0.f, 0.f, 0.f}, pacc = sacc;     // rows = keys k0 + 16 kt + 4 g + r, column = query c
                const float* kr = Ks + (kt * 16 + c) * AB_LD + 4 * g;
                const float* vr = Vs + (kt * 16 + c) * AB_LD + 4 * g;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) {
                    const float4 kf = *reinterpret_cast<const float4*>(kr + 16 * blk);
                    const float4 vf = *reinterpret_cast<const float4*>(vr + 16 * blk);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ab_e(kf, kk), ab_e(qf[blk], kk), sacc, 0, 0, 0);
                        pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ab_e(vf, kk), ab_e(dof[blk], kk), pacc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kl = kt * 16 + 4 * g + r;
                    const float p = (qok && k0 + kl < N) ? expf(sacc[r] * scale - lse_c) : 0.f;
                    if (sweep == 0) {
                        lsum += p;
                        dsum += p * pacc[r];
                    } else {
                        const float ds = (p * inv_c) * (pacc[r] - D_c);        // A[row = query c][k = g <-> key 4 g + r]
                        const float* kc = Ks + kl * AB_LD + c;                 // B[k = g][column = d 16 jd + c]
#pragma unroll
                        for (int j = 0; j < 4; ++j) dq[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, kc[16 * j], dq[j], 0, 0, 0);
                    }
                }
            }
        }
        if (sweep == 0) {           // the four lanes g of a query hold a quarter of its keys each: a fixed xor tree
            lsum += __shfl_xor(lsum, 16);
            lsum += __shfl_xor(lsum, 32);
            dsum += __shfl_xor(dsum, 16);
            dsum += __shfl_xor(dsum, 32);
            if (qok) {
                inv_c = 1.0f / lsum;
                D_c = dsum * inv_c;
                if (g == 0) {
                    inv_l[so] = inv_c;
                    D[so] = D_c;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = qb + 4 * g + r;
        if (row < N) {
            float* dst = g_qkv + ((long long)view * N + row) * ld + head * 64 + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[16 * j] = dq[j][r] * scale;
        }
    }
}

// dK, dV: workgroup = 64 keys (wave w: 16 of them, one per lane column c), loop over 64-query tiles of Q and dO in LDS
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ g_out,
                                                           const float* __restrict__ lse, const float* __restrict__ inv_l,
                                                           const float* __restrict__ D, int N, int dim, float scale,
                                                           float* __restrict__ g_qkv) {
    __shared__ __attribute__((aligned(16))) float Qs[AB_T * AB_LD];
    __shared__ __attribute__((aligned(16))) float Os[AB_T * AB_LD];
    __shared__ float lse_s[AB_T], inv_s[AB_T], D_s[AB_T];      // the rows' constants (attn_bwd_dq_kernel's prologue)
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = blockIdx.y, view = blockIdx.z, heads = gridDim.y;
    const int ld = 3 * dim;
    const float* base = qkv + (long long)view * N * ld + head * 64;
    const float* gbase = g_out + (long long)view * N * dim + head * 64;
    const long long sbase = ((long long)view * heads + head) * N;
    const int kb = blockIdx.x * AB_T + wave * 16, kj = kb + c;
    const bool kok = kj < N;

    float4 kf[4], vf[4];        // B operands of S = Q K^T and dP = dO V^T: column = key c
    ab_row_frags(base + dim + (long long)(kok ? kj : 0) * ld, kok, g, kf);
    ab_row_frags(base + 2 * dim + (long long)(kok ? kj : 0) * ld, kok, g, vf);

    f32x4 dk[4], dv[4];         // tiles: row = key kb + 4 g + r, column = d 16 jd + c
#pragma unroll
    for (int j = 0; j < 4; ++j) dk[j] = dv[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < N; q0 += AB_T) {
        __syncthreads();
        ab_stage(base, ld, gbase, dim, q0, N, Qs, Os, tid);
        if (tid < AB_T) {
            const bool ok = q0 + tid < N;
            lse_s[tid] = ok ? lse[sbase + q0 + tid] : 0.f;
            inv_s[tid] = ok ? inv_l[sbase + q0 + tid] : 0.f;
            D_s[tid] = ok ? D[sbase + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (kb >= N) continue;
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 sacc = (f32x4){0.f, 0.f, 0.f, 0.f}, pacc = sacc;     // rows = queries q0 + 16 qt + 4 g + r, column = key c
            const float* qr = Qs + (qt * 16 + c) * AB_LD + 4 * g;
            const float* orow = Os + (qt * 16 + c) * AB_LD + 4 * g;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                const float4 qf = *reinterpret_cast<const float4*>(qr + 16 * blk);
                const float4 of = *reinterpret_cast<const float4*>(orow + 16 * blk);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ab_e(qf, kk), ab_e(kf[blk], kk), sacc, 0, 0, 0);
                    pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ab_e(of, kk), ab_e(vf[blk], kk), pacc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = qt * 16 + 4 * g + r;
                const float p = (kok && q0 + ql < N) ? expf(sacc[r] * scale - lse_s[ql]) * inv_s[ql] : 0.f;
                const float ds = p * (pacc[r] - D_s[ql]);              // A[row = key c][k = g <-> query 4 g + r]
                const float* oc = Os + ql * AB_LD + c;                 // B[k = g][column = d 16 jd + c]
                const float* qc = Qs + ql * AB_LD + c;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, oc[16 * j], dv[j], 0, 0, 0);
                    dk[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, qc[16 * j], dk[j], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = kb + 4 * g + r;
        if (row < N) {
            float* dst = g_qkv + ((long long)view * N + row) * ld + dim + head * 64 + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dst[16 * j] = dk[j][r] * scale;
                dst[dim + 16 * j] = dv[j][r];
            }
        }
    }
}

// N = 1: g_qkv row = [0 .. 0 | 0 .. 0 | g_out row]
__global__ __launch_bounds__(256) void attn_bwd_single_kernel(const float* __restrict__ g_out, int V, int dim,
                                                              float* __restrict__ g_qkv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n = (long long)V * 3 * dim;
    if (i >= n) return;
    const long long view = i / (3 * dim);
    const int col = (int)(i - view * 3 * dim);
    g_qkv[i] = col >= 2 * dim ? g_out[view * dim + col - 2 * dim] : 0.f;
}

static bool attn_bwd_shape_ok(int V, int N, int heads) {
    return V > 0 && V <= 65535 && N > 0 && N <= (1 << 24) && heads > 0 && heads <= 1024;
}

// the rows' constants 1 / l and D, [V][heads][N] each; size 0 for a shape th_attention_bwd refuses
struct AttnBwdWs { float *inv_l, *D; };
static AttnBwdWs attn_bwd_layout(ThArena& ar, int V, int N, int heads) {
    return {ar.take<float>((size_t)V * heads * N), ar.take<float>((size_t)V * heads * N)};
}
size_t th_attn_bwd_ws(int V, int N, int heads) {
    return attn_bwd_shape_ok(V, N, heads) ? th_measure(attn_bwd_layout, V, N, heads) : 0;
}

int th_attention_bwd_launch(const float* qkv, const float* out, const float* lse, const float* g_out, int V, int N, int heads,
                            float* g_qkv, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(attn_bwd_shape_ok(V, N, heads), "th_attention_bwd: need 1 <= V <= 65535, 1 <= N <= 2^24, 1 <= heads <= 1024");
    TH_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)lse) & 15) == 0 &&
                   (((uintptr_t)g_out) & 15) == 0 && (((uintptr_t)g_qkv) & 15) == 0,
               "qkv, out, lse, g_out and g_qkv must be 16-byte aligned");
    TH_REQUIRE((((uintptr_t)ws) & 15) == 0, "workspace must be 16-byte aligned");
    ThArena ar(ws, ws_bytes);
    AttnBwdWs w = attn_bwd_layout(ar, V, N, heads);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int dim = heads * 64;
    const float scale = 0.125f;   // head_dim ** -0.5
    if (N == 1) {
        hipLaunchKernelGGL(attn_bwd_single_kernel, dim3(th_cdiv((long long)V * 3 * dim, 256)), dim3(256), 0, s, g_out, V, dim, g_qkv);
        TH_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(th_cdiv(N, AB_T), heads, V);
    // (every row's constants are written by the first launch before the second, on the same stream, reads them)
    hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), 0, s, qkv, g_out, lse, N, dim, scale, w.inv_l, w.D, g_qkv);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), 0, s, qkv, g_out, lse, w.inv_l, w.D, N, dim, scale, g_qkv);
    TH_LAUNCH_CHECK();
    return 0;
}
