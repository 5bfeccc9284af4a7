// K20: the training form of the per-point network (MLP_forward_ori, cross_transformer.py:273-353), layer by layer like
// th_mlp_forward (k_mlp.hip).  Nothing in this file is launched by inference or by bench.py.
//
// The dense layers are th_gemm launches on the fp32 MFMA pipe and the backward machinery of k_vit_dense_bwd.hip (the image of
// W^T for the input gradient, wgrad_kernel's 256-row chunks added in chunk order).  New arithmetic is two small pieces:
//
//   a ReLU on a layer's OUTPUT   Y = relu(A W^T + b) is th_gemm's TH_ACT_RELU epilogue; the backward is th_linear_bwd form 0
//                                with g_C = g_Y * [Y > 0] (torch's rule: 0 at Y == 0): gated on g_Y's way into LDS in
//                                wgrad_kernel<OP_PLAIN, true>, and by one elementwise pass into the workspace for the input gradient
//   the V x V cross-view attention (cross_transformer.py:128-149)   forward: xattn_kernel of k_mlp.hip as it is; backward:
//                                xattn_bwd_kernel below, one wave per sample, the probabilities recomputed from the keys
#include "th_internal.h"

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
static bool pn_shape_ok(int M, int out_f, int in_f) {
    return M >= 1 && M <= (1 << 24) && out_f >= 16 && in_f >= 16 && (out_f & 15) == 0 && (in_f & 15) == 0 && out_f <= 65536 &&
           in_f <= 65536;
}
static bool pn_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

struct PnBwdWs { size_t pack, gate, part, total; };
static PnBwdWs pn_bwd_layout(int M, int out_f, int in_f) {
    PnBwdWs w{};
    w.pack = 0;
    size_t off = ThPacked::bytes(in_f, out_f);
    w.gate = off;
    off += th_align((size_t)M * out_f * sizeof(float));
    w.part = off;
    off += th_align((size_t)th_wgrad_chunks(M) * ((size_t)out_f * in_f + out_f) * sizeof(float));
    w.total = off;
    return w;
}

#define PN_SHAPE_MSG "unsupported shape: M >= 1, in_f and out_f multiples of 16"

extern "C" {

size_t th_linear_relu_workspace_bytes(int M, int out_f, int in_f) {
    if (!pn_shape_ok(M, out_f, in_f)) return 0;
    return ThPacked::bytes(out_f, in_f);
}

int th_linear_relu_forward(th_ctx* c, const float* A, int lda, int M, const th_linear* lin, float* Y, int ldy, void* ws,
                           size_t ws_bytes, th_stream stream) {
    TH_REQUIRE(c && A && lin && Y && ws, "null argument");
    TH_REQUIRE(lin->w != nullptr, "null argument (the layer's weight)");
    TH_REQUIRE(pn_shape_ok(M, lin->out_f, lin->in_f), PN_SHAPE_MSG);
    TH_REQUIRE(lda >= lin->in_f && ldy >= lin->out_f && (lda & 3) == 0 && (ldy & 3) == 0, "lda / ldy: >= the row, multiples of 4");
    TH_REQUIRE(pn_al16(A) && pn_al16(Y) && pn_al16(ws) && pn_al16(lin->w), "pointers must be 16-byte aligned");
    TH_REQUIRE(ws_bytes >= th_linear_relu_workspace_bytes(M, lin->out_f, lin->in_f), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    ThPacked P;
    TH_TRY(th_pack_linear(*lin, ws, &P, s));
    return th_gemm(A, lda, M, P, TH_ACT_RELU, Y, ldy, s);
}

size_t th_linear_relu_bwd_workspace_bytes(int M, int out_f, int in_f) {
    if (!pn_shape_ok(M, out_f, in_f)) return 0;
    return pn_bwd_layout(M, out_f, in_f).total;
}

int th_linear_relu_bwd(th_ctx* c, const float* A, int lda, const float* Y, int ldy, int M, const th_linear* lin, const float* g_Y,
                       int ldg, float* g_A, int ldga, float* g_W, float* g_b, void* ws, size_t ws_bytes, th_stream stream) {
    TH_REQUIRE(c && A && Y && lin && g_Y && g_W && ws, "null argument");
    TH_REQUIRE(lin->w != nullptr, "null argument (the layer's weight)");
    const int out_f = lin->out_f, in_f = lin->in_f;
    TH_REQUIRE(pn_shape_ok(M, out_f, in_f), PN_SHAPE_MSG);
    TH_REQUIRE(lda >= in_f && ldy >= out_f && ldg >= out_f && (lda & 3) == 0 && (ldy & 3) == 0 && (ldg & 3) == 0 &&
                   (g_A == nullptr || (ldga >= in_f && (ldga & 3) == 0)),
               "lda / ldy / ldg / ldga: >= the row, multiples of 4");
    TH_REQUIRE(pn_al16(A) && pn_al16(Y) && pn_al16(g_Y) && pn_al16(g_A) && pn_al16(g_W) && pn_al16(ws) && pn_al16(lin->w),
               "pointers must be 16-byte aligned");
    const PnBwdWs L = pn_bwd_layout(M, out_f, in_f);
    TH_REQUIRE(ws_bytes >= L.total, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    if (g_A != nullptr) {
        float* gated = (float*)(base + L.gate);
        const long long n4 = (long long)M * (out_f >> 2);
        hipLaunchKernelGGL(relu_gate_kernel, dim3((unsigned)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192)), dim3(256), 0, s,
                           g_Y, ldg, Y, ldy, M, out_f, gated);
        TH_LAUNCH_CHECK();
        ThPacked P;
        TH_TRY(th_pack_linear_t(lin->w, out_f, in_f, base + L.pack, &P, s));
        TH_TRY(th_gemm(gated, out_f, M, P, TH_ACT_NONE, g_A, ldga, s));
    }
    return th_wgrad_relu_launch(g_Y, ldg, Y, ldy, A, lda, M, out_f, in_f, (float*)(base + L.part), g_W, g_b, s);
}

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
