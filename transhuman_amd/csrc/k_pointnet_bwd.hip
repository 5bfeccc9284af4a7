// K20: the training form of the per-point network (MLP_forward_ori, cross_transformer.py:273-353), layer by layer like
// th_mlp_forward (k_mlp.hip).  Nothing in this file is launched by inference or by bench.py.
//
// The dense layers, with and without a ReLU on their output, are the entries of k_vit_dense_bwd.hip (th_linear_relu_* /
// th_linear_train_forward / th_linear_bwd).  What is left here is the V x V cross-view attention (cross_transformer.py:128-149):
// forward: xattn_kernel of k_mlp.hip as it is; backward: xattn_bwd_kernel below, one wave per sample, the probabilities recomputed
// from the keys
#include "th_internal.h"

// ---- cross-view attention, backward ---------------------------------------------------------------------------------------------
// Rows as xattn_kernel: [key(128) | value(256)].  With A[j][i] = softmax_j(kp_j . ks_i / sqrt(128)) and n_i = vs_i + sum_j A[j][i] vp_j:
//   g_vs_i = g_n_i,   g_vp_j = sum_i A[j][i] g_n_i,   dA[j][i] = vp_j . g_n_i,
//   dS[j][i] = A[j][i] (dA[j][i] - sum_j' A[j'][i] dA[j'][i]),
//   g_kp_j = sum_i dS[j][i] ks_i / sqrt(128),   g_ks_i = sum_j dS[j][i] kp_j / sqrt(128).
// One wave per sample, four samples per workgroup.  A lane holds key columns lane, 64 + lane and value columns 4 lane .. 4 lane + 3 of
// every row; the logits and the softmax are xattn_kernel's statements, so A is the forward's bit for bit.  The V x V dots are
// 4 (values) or 2 (keys) terms per lane and a butterfly over the wave: every lane ends with the same sum.  Nothing P x V x V is
// stored, no LDS, no atomics.
template <int V>
__global__ __launch_bounds__(256) void xattn_bwd_kernel(const float* __restrict__ kvp, const float* __restrict__ kvs,
                                                        const float* __restrict__ g_n, int P, float* __restrict__ g_kvp,
                                                        float* __restrict__ g_kvs) {
    const int lane = threadIdx.x & 63;
    int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const float* bp = kvp + (long long)p * V * 384;
    const float* bs = kvs + (long long)p * V * 384;
    float* gp = g_kvp + (long long)p * V * 384;
    float* gs = g_kvs + (long long)p * V * 384;
    float kp[V][2], ks[V][2];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        kp[v][0] = bp[v * 384 + lane]; kp[v][1] = bp[v * 384 + 64 + lane];
        ks[v][0] = bs[v * 384 + lane]; ks[v][1] = bs[v * 384 + 64 + lane];
    }
    float A[V][V];
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float t = kp[j][0] * ks[i][0] + kp[j][1] * ks[i][1];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            A[j][i] = t / 11.313708498984761f;
        }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float m = A[0][i];
#pragma unroll
        for (int j = 1; j < V; ++j) m = fmaxf(m, A[j][i]);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) { A[j][i] = expf(A[j][i] - m); s = s + A[j][i]; }
#pragma unroll
        for (int j = 0; j < V; ++j) A[j][i] = A[j][i] / s;
    }
    float4 vp[V], gn[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        vp[v] = *reinterpret_cast<const float4*>(bp + v * 384 + 128 + 4 * lane);
        gn[v] = *reinterpret_cast<const float4*>(g_n + ((long long)p * V + v) * 256 + 4 * lane);
    }
    // value blocks
#pragma unroll
    for (int i = 0; i < V; ++i) *reinterpret_cast<float4*>(gs + i * 384 + 128 + 4 * lane) = gn[i];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float4 t;
        t.x = A[j][0] * gn[0].x; t.y = A[j][0] * gn[0].y; t.z = A[j][0] * gn[0].z; t.w = A[j][0] * gn[0].w;
#pragma unroll
        for (int i = 1; i < V; ++i) {
            t.x = t.x + A[j][i] * gn[i].x; t.y = t.y + A[j][i] * gn[i].y;
            t.z = t.z + A[j][i] * gn[i].z; t.w = t.w + A[j][i] * gn[i].w;
        }
        *reinterpret_cast<float4*>(gp + j * 384 + 128 + 4 * lane) = t;
    }
    // dS (overwrites dA)
    float dS[V][V];
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float t = (vp[j].x * gn[i].x + vp[j].y * gn[i].y) + (vp[j].z * gn[i].z + vp[j].w * gn[i].w);
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            dS[j][i] = t;
        }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float d = A[0][i] * dS[0][i];
#pragma unroll
        for (int j = 1; j < V; ++j) d = d + A[j][i] * dS[j][i];
#pragma unroll
        for (int j = 0; j < V; ++j) dS[j][i] = A[j][i] * (dS[j][i] - d);
    }
    // key blocks
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float a = dS[j][0] * ks[0][0], b = dS[j][0] * ks[0][1];
#pragma unroll
        for (int i = 1; i < V; ++i) { a = a + dS[j][i] * ks[i][0]; b = b + dS[j][i] * ks[i][1]; }
        gp[j * 384 + lane] = a / 11.313708498984761f;
        gp[j * 384 + 64 + lane] = b / 11.313708498984761f;
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float a = dS[0][i] * kp[0][0], b = dS[0][i] * kp[0][1];
#pragma unroll
        for (int j = 1; j < V; ++j) { a = a + dS[j][i] * kp[j][0]; b = b + dS[j][i] * kp[j][1]; }
        gs[i * 384 + lane] = a / 11.313708498984761f;
        gs[i * 384 + 64 + lane] = b / 11.313708498984761f;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static bool pn_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" {

int th_xview_attention(th_ctx* c, const float* kvp, const float* kvs, int P, int V, float* n, th_stream stream) {
    TH_REQUIRE(c && kvp && kvs && n, "null argument");
    TH_REQUIRE(V >= 1 && V <= 4 && P >= 1 && P <= (1 << 24), "unsupported shape: P >= 1, V in 1..4");
    TH_REQUIRE(pn_al16(kvp) && pn_al16(kvs) && pn_al16(n), "pointers must be 16-byte aligned");
    return th_xattn_launch(kvp, kvs, P, V, n, (hipStream_t)stream);
}

int th_xview_attention_bwd(th_ctx* c, const float* kvp, const float* kvs, const float* g_n, int P, int V, float* g_kvp,
                           float* g_kvs, th_stream stream) {
    TH_REQUIRE(c && kvp && kvs && g_n && g_kvp && g_kvs, "null argument");
    TH_REQUIRE(V >= 1 && V <= 4 && P >= 1 && P <= (1 << 24), "unsupported shape: P >= 1, V in 1..4");
    TH_REQUIRE(pn_al16(kvp) && pn_al16(kvs) && pn_al16(g_n) && pn_al16(g_kvp) && pn_al16(g_kvs), "pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    dim3 g4(th_cdiv(P, 4));
    switch (V) {
        case 1: hipLaunchKernelGGL(xattn_bwd_kernel<1>, g4, dim3(256), 0, s, kvp, kvs, g_n, P, g_kvp, g_kvs); break;
        case 2: hipLaunchKernelGGL(xattn_bwd_kernel<2>, g4, dim3(256), 0, s, kvp, kvs, g_n, P, g_kvp, g_kvs); break;
        case 3: hipLaunchKernelGGL(xattn_bwd_kernel<3>, g4, dim3(256), 0, s, kvp, kvs, g_n, P, g_kvp, g_kvs); break;
        default: hipLaunchKernelGGL(xattn_bwd_kernel<4>, g4, dim3(256), 0, s, kvp, kvs, g_n, P, g_kvp, g_kvs); break;
    }
    TH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
