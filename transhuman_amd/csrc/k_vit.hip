// K3: TransHE -- ViT-tiny over the N_c canonical-body tokens.
//
// VisionTransformer.forward (lib/networks/vision_transformer.py:371-383):
// x += PE; depth x [ pre-LN (eps 1e-6) -> fused qkv Linear -> 3-head
// softmax(q k^T * 0.125) v -> proj -> residual ; pre-LN -> FC 192->768 ->
// GELU(erf) -> FC 768->192 -> residual ] ; final LN   (:257-307).
// Dense layers: th_gemm_h3 (fp16-split MFMA; th_gemm_ln / th_gemm outside its range).
// Attention: flash-style on fp16-split MFMA operands, online softmax in registers;
// attn2_kernel (one wave = 16 queries, K / V^T fragments from L2) up to N = 700,
// attn3_kernel (64 queries share K / V^T tiles staged in LDS) above.  The
// [V,3,N,N] probability tensor the reference materialises (81 MB at N_c = 1500)
// never exists.
// Per-frame cost 12/23/110 GFLOP at N_c = 300/500/1500 (fp32 MFMA bound).

#include "th_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                           float* __restrict__ o) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] + b[i];
}

// wave per row, dim <= 256*... (dim=192 -> 3 values per lane)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int rows, int dim,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        float eps, float* __restrict__ o) {
    const int lane = threadIdx.x & 63;
    int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + (long long)r * dim;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int c = lane + 64 * i;
        v[i] = (c < dim) ? xr[c] : 0.f;
        s += v[i];
    }
    for (int q = 32; q > 0; q >>= 1) s += __shfl_xor(s, q);
    float mean = s / (float)dim;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float d = (lane + 64 * i < dim) ? v[i] - mean : 0.f;
        ss += d * d;
    }
    for (int q = 32; q > 0; q >>= 1) ss += __shfl_xor(ss, q);
    float rstd = 1.0f / __fsqrt_rn(ss / (float)dim + eps);
    float* orow = o + (long long)r * dim;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int c = lane + 64 * i;
        if (c < dim) orow[c] = (v[i] - mean) * rstd * w[c] + b[c];
    }
}

// ---- attention -------------------------------------------------------------------
// qkv rows: [T, 3*dim] with col = which*dim + head*64 + d  (:271).  head_dim = 64.
// softmax(q k^T * 0.125) v per (view, head), flash-style: 64-key tiles, online softmax in registers, the
// [V,3,N,N] probability tensor never exists.  Both products run on v_mfma_f32_16x16x32_f16 with the operands
// split into fp16 hi + lo (x = hi + lo to 2^-22; three products hi*hi + hi*lo + lo*hi, fp32 accumulate -- the
// same fp32-class scheme as the fused MLP): 48 MFMAs of 16 cycles per tile and wave instead of the
// 128 fp32 MFMAs of 32 cycles the 16x16x4 form needs.
#define AT_K 64

typedef _Float16 at_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 at_h4 __attribute__((ext_vector_type(4)));

// Supported operand range.  hi + lo reproduces x to 2^-22 relative while lo is a NORMAL fp16 number, i.e. for
// 2^-3 <= |x| < 65504 (above: hi overflows to inf).  Below 2^-3 lo is subnormal and the error of the pair is absolute, at most
// 2^-25 per operand -- harmless for the probabilities (in [0, 1], summed against an fp32 row sum) and for q, k, v of the
// magnitude of the product's own rows (max |q| ~ 6).  tests/test_gpu_vit.py holds both kernels to 4 x the error of an fp32
// evaluation for v scaled by 2^-10 .. 2^10 and q 2^-4 with k 2^4; a CPU emulation of the scheme leaves that class at v 2^-14
// (16 x the fp32 error) and at q 2^-8: operands that small are outside the supported range (scale them up first).
__device__ __forceinline__ void at_split(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// ---- attention, second form: operands split ONCE per layer, no LDS staging ------------------------------------
// The first form (round 2, since retired) converted every K / V tile fp32 -> fp16 hi/lo inside every workgroup (the V
// tile transposed with 2-byte LDS stores) between two block barriers: 8 q-blocks repeated the conversion of the same
// (view, head) and the 8-tile loop was a 31 us dependent chain.  Here kv_split_kernel writes, once per layer,
//   Kp [V][heads][2 planes][Npad][64]   K rows as fp16 hi | lo          (rows >= N zero)
//   Vp [V][heads][2 planes][64][Npad]   V^T rows (one d; keys in the fragment order of attn2_kernel) as fp16 hi | lo
// -- exactly the 16-byte B-operand fragments of the two products -- and attn2_kernel (ONE wave = 16 queries per
// workgroup, 288 workgroups at N = 500) loads them straight from L2 into registers: no block barrier, no conversion
// in the loop, V fragments of a tile requested before its S product, K fragments of the next tile before its P V.
// (Splitting the keys of a query block over 4 waves with a final merge, and feeding the LDS tiling from the pre-split
// planes, were both measured: no gain / slower -- this form is bound by its L2 traffic, the LDS form by its barriers.)
__global__ __launch_bounds__(256) void kv_split_kernel(const float* __restrict__ qkv, int N, int Npad, int dim,
                                                       _Float16* __restrict__ Kp, _Float16* __restrict__ Vp) {
    __shared__ float vt[64][65];
    const int tid = threadIdx.x, head = blockIdx.y, view = blockIdx.z, heads = gridDim.y;
    const int k0 = blockIdx.x * 64;
    const int ld = 3 * dim;
    const float* base = qkv + (long long)view * N * ld;
    const long long plane = (long long)Npad * 64;
    _Float16* kp = Kp + ((long long)view * heads + head) * 2 * plane;
    _Float16* vp = Vp + ((long long)view * heads + head) * 2 * plane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 4, c4 = idx & 15, key = k0 + row;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (key < N) {
            kv = *reinterpret_cast<const float4*>(base + (long long)key * ld + dim + head * 64 + 4 * c4);
            vv = *reinterpret_cast<const float4*>(base + (long long)key * ld + 2 * dim + head * 64 + 4 * c4);
        }
        const float kk[4] = {kv.x, kv.y, kv.z, kv.w};
        at_h4 kh, kl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            _Float16 x, y;
            at_split(kk[e], x, y);
            kh[e] = x; kl[e] = y;
        }
        *reinterpret_cast<at_h4*>(kp + (long long)key * 64 + 4 * c4) = kh;
        *reinterpret_cast<at_h4*>(kp + plane + (long long)key * 64 + 4 * c4) = kl;
        vt[row][4 * c4 + 0] = vv.x; vt[row][4 * c4 + 1] = vv.y; vt[row][4 * c4 + 2] = vv.z; vt[row][4 * c4 + 3] = vv.w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, d = idx >> 4, c4 = idx & 15;     // d row, 4 consecutive keys
        at_h4 vh, vl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            _Float16 x, y;
            at_split(vt[4 * c4 + e][d], x, y);
            vh[e] = x; vl[e] = y;
        }
        // keys 4 c4 .. 4 c4 + 3 of the 64-key block; within a 32-key block key offset 16 n + 4 g + j sits at position
        // 8 g + 4 n + j (the B-operand order of attn2_kernel's P^T fragments)
        const int ko = (4 * c4) & 31, pos = ((4 * c4) & 32) + 8 * ((ko & 15) >> 2) + 4 * (ko >> 4);
        *reinterpret_cast<at_h4*>(vp + (long long)d * Npad + k0 + pos) = vh;
        *reinterpret_cast<at_h4*>(vp + plane + (long long)d * Npad + k0 + pos) = vl;
    }
}

// The products are formed TRANSPOSED: S^T = K Q^T and O^T = V^T P^T.  An MFMA result tile holds, per lane, 4 consecutive
// rows of ONE column; with queries as columns a lane owns one query (lane & 15) and its 16 scores of a 64-key tile sit
// in its own registers: the row maximum / sum are in-register reductions plus two cross-row steps, the probabilities are
// already laid out as the B operand of the second product (k index = 8 (lane >> 4) + j  <->  key 16 (j >> 2) + 4 (lane >> 4)
// + (j & 3) of a 32-key block: kv_split_kernel stores V^T in that key order), and the softmax statistics of a query live
// in the lane that holds its output column -- no LDS, no barrier, no cross-lane traffic for the rescaling.  (The
// row-major form wrote P through LDS with 32 two-byte stores per tile and reduced 4 rows x 4 steps across lanes:
// 21.4 us per layer at N = 500; this form 16.6 us.  Splitting the keys of a query block over 4 waves with an LDS merge
// of the partial (m, l, O^T) triples was measured again on this form: 17.7 us -- the launch is not bound by the length of
// the per-wave chain.)
template <bool LSE>
__global__ __launch_bounds__(64) void attn2_kernel(const float* __restrict__ qkv, const _Float16* __restrict__ Kp,
                                                   const _Float16* __restrict__ Vp, int N, int Npad, int dim,
                                                   float scale, float* __restrict__ out, float* __restrict__ lse) {
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int kbeg = 0, kend = N;
    const int head = blockIdx.y, view = blockIdx.z, heads = gridDim.y;
    const int q0 = blockIdx.x * 16;
    const int ld = 3 * dim;
    const float* base = qkv + (long long)view * N * ld;
    const long long plane = (long long)Npad * 64;
    const _Float16* kp = Kp + ((long long)view * heads + head) * 2 * plane;
    const _Float16* vp = Vp + ((long long)view * heads + head) * 2 * plane;

    // Q^T fragments (B operand: column = query c, k = d = 32 s2 + 8 g + j)
    at_h8 qh[2], ql[2];
    {
        const int qi = q0 + c;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v8[e] = 0.f;
            if (qi < N) {
                const float* src = base + (long long)qi * ld + head * 64 + 32 * s2 + 8 * g;
                float4 a = *reinterpret_cast<const float4*>(src), b4 = *reinterpret_cast<const float4*>(src + 4);
                v8[0] = a.x; v8[1] = a.y; v8[2] = a.z; v8[3] = a.w; v8[4] = b4.x; v8[5] = b4.y; v8[6] = b4.z; v8[7] = b4.w;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 x, y;
                at_split(v8[e], x, y);
                qh[s2][e] = x; ql[s2][e] = y;
            }
        }
    }
    f32x4 oacc[4];              // O^T tiles: d = 16 jd + 4 g + r, column = query c
#pragma unroll
    for (int j = 0; j < 4; ++j) oacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mrun = -3.0e38f, lrun = 0.f;

    // fragments of one 64-key tile: K [nt][s2] (A operand: row = key k0 + 16 nt + c, k = d = 32 s2 + 8 g ..+7),
    //                               V^T [jd][s2] (A operand: row = d = 16 jd + c, k = position 8 g ..+7 of 32-key block s2)
    at_h8 kh[4][2], kl[4][2], vh[4][2], vl[4][2];
    auto load_k = [&](int k0) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const long long o = (long long)(k0 + nt * 16 + c) * 64 + 32 * s2 + 8 * g;
                kh[nt][s2] = *reinterpret_cast<const at_h8*>(kp + o);
                kl[nt][s2] = *reinterpret_cast<const at_h8*>(kp + plane + o);
            }
    };
    auto load_v = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const long long o = (long long)(j * 16 + c) * Npad + k0 + 32 * s2 + 8 * g;
                vh[j][s2] = *reinterpret_cast<const at_h8*>(vp + o);
                vl[j][s2] = *reinterpret_cast<const at_h8*>(vp + plane + o);
            }
    };
    if (kbeg < kend) load_k(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += AT_K) {
        load_v(k0);
        f32x4 sacc[4];          // S^T tiles: key = k0 + 16 nt + 4 g + r, column = query c
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            sacc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[nt][s2], ql[s2], sacc[nt], 0, 0, 0);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[nt][s2], qh[s2], sacc[nt], 0, 0, 0);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[nt][s2], qh[s2], sacc[nt], 0, 0, 0);
            }
        }
        if (k0 + AT_K < kend) load_k(k0 + AT_K);
        float m = -3.0e38f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + nt * 16 + 4 * g + r;
                const float sv = (key < N) ? sacc[nt][r] * scale : -3.0e38f;
                sacc[nt][r] = sv;
                m = fmaxf(m, sv);
            }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float mnew = fmaxf(mrun, m);
        const float corr = expf(mrun - mnew);
        mrun = mnew;
        float ls = 0.f;
        at_h8 ph[2], pl[2];     // P^T fragments (B operand) of the two 32-key blocks
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + nt * 16 + 4 * g + r;
                const float pv = (key < N) ? expf(sacc[nt][r] - mnew) : 0.f;
                ls += pv;
                _Float16 x, y;
                at_split(pv, x, y);
                ph[nt >> 1][4 * (nt & 1) + r] = x;
                pl[nt >> 1][4 * (nt & 1) + r] = y;
            }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        lrun = lrun * corr + ls;
#pragma unroll
        for (int j = 0; j < 4; ++j) oacc[j] *= corr;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[j][s2], pl[s2], oacc[j], 0, 0, 0);
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl[j][s2], ph[s2], oacc[j], 0, 0, 0);
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[j][s2], ph[s2], oacc[j], 0, 0, 0);
            }
    }
    // out[t][head*64 + d] = O / l      (x = (attn @ v).transpose(1,2).reshape(B,N,C), :278): 4 consecutive d per lane
    const int qi = q0 + c;
    if (qi < N) {
        const float inv = 1.0f / lrun;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<float4*>(out + ((long long)view * N + qi) * dim + head * 64 + j * 16 + 4 * g) =
                make_float4(oacc[j][0] * inv, oacc[j][1] * inv, oacc[j][2] * inv, oacc[j][3] * inv);
        // training form: the row's log-sum-exp of the scaled logits (the four lanes g of a query hold the same value)
        if constexpr (LSE) {
            if (g == 0) lse[((long long)view * heads + head) * N + qi] = mrun + logf(lrun);
        }
    }
}

// ---- attention, third form (round 6): attn2's arithmetic, K / V^T tiles shared by four waves through LDS ---------------------------
// attn2_kernel (one wave = 16 queries per workgroup) streams the whole K / V^T planes of its (view, head) from L2 per wave: at
// N = 1500 that is 650 MB per layer and the launch takes 172 us (3.8 TB/s: the L2's rate for this pattern); the retired round-2
// form converted and transposed every tile inside every workgroup (134 us).  Here one workgroup = 4 waves = 64 queries; a
// 64-key tile of the PRE-SPLIT planes (the qkv GEMM's epilogue writes them in fragment order) is copied into LDS by LDS-DMA, one
// plane per wave (K hi, K lo, V^T hi, V^T lo: 8 KB = 8 wave instructions each), double-buffered, ONE barrier per tile; every wave
// reads its fragments with ds_read_b128 and runs attn2's transposed products / online softmax in registers.  A quarter of the L2
// traffic, no conversion, no 2-byte LDS stores.  LDS rows are 128 B (8 slots of 16 B); slot s of row r sits at s ^ (r & 7): the
// 16 lanes a ds_read_b128 services per cycle (16 rows, two slot columns) then hit 16 different positions of the bank row
// (LDS-DMA writes lane-linear, so the swizzle is applied to the SOURCE address a lane fetches).
#define AT3_PLANE (64 * 128)           // bytes of one tile plane
template <bool LSE>
__global__ __launch_bounds__(256) void attn3_kernel(const float* __restrict__ qkv, const _Float16* __restrict__ Kp,
                                                    const _Float16* __restrict__ Vp, int N, int Npad, int dim,
                                                    float scale, float* __restrict__ out, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) char tiles[2][4 * AT3_PLANE];      // [buffer][K hi | K lo | V^T hi | V^T lo]
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = blockIdx.y, view = blockIdx.z, heads = gridDim.y;
    const int q0 = blockIdx.x * 64 + wave * 16;
    const int ld = 3 * dim;
    const float* base = qkv + (long long)view * N * ld;
    const long long plane = (long long)Npad * 64;
    const _Float16* kp = Kp + ((long long)view * heads + head) * 2 * plane;
    const _Float16* vp = Vp + ((long long)view * heads + head) * 2 * plane;

    // this wave's share of a tile copy: plane `wave` (0: K hi, 1: K lo, 2: V^T hi, 3: V^T lo), 8 x 1 KiB
    typedef __attribute__((address_space(1))) const void* at_gptr;
    typedef __attribute__((address_space(3))) void* at_lptr;
    auto stage = [&](int k0, int buf) {
        char* dst = tiles[buf] + wave * AT3_PLANE;
        const _Float16* src = (wave < 2 ? kp : vp) + (long long)(wave & 1) * plane;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int L = i * 64 + lane, r = L >> 3, sl = (L & 7) ^ (r & 7);          // LDS slot L holds logical slot sl of row r
            const _Float16* gsrc = wave < 2 ? src + (long long)(k0 + r) * 64 + 8 * sl               // K row = key k0 + r
                                            : src + (long long)r * Npad + k0 + 8 * sl;              // V^T row = d
            __builtin_amdgcn_global_load_lds((at_gptr)gsrc, (at_lptr)(dst + i * 1024), 16, 0, 0);
        }
    };

    // Q^T fragments (B operand: column = query c, k = d = 32 s2 + 8 g + j)
    at_h8 qh[2], ql[2];
    {
        const int qi = q0 + c;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v8[e] = 0.f;
            if (qi < N) {
                const float* src = base + (long long)qi * ld + head * 64 + 32 * s2 + 8 * g;
                float4 a = *reinterpret_cast<const float4*>(src), b4 = *reinterpret_cast<const float4*>(src + 4);
                v8[0] = a.x; v8[1] = a.y; v8[2] = a.z; v8[3] = a.w; v8[4] = b4.x; v8[5] = b4.y; v8[6] = b4.z; v8[7] = b4.w;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 x, y;
                at_split(v8[e], x, y);
                qh[s2][e] = x; ql[s2][e] = y;
            }
        }
    }
    f32x4 oacc[4];              // O^T tiles: d = 16 jd + 4 g + r, column = query c
#pragma unroll
    for (int j = 0; j < 4; ++j) oacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mrun = -3.0e38f, lrun = 0.f;
    const int foff = c * 128;                         // this lane's row inside a 16-row block of a tile plane
    const int sw = c & 7;

    stage(0, 0);
    int buf = 0;
    for (int k0 = 0; k0 < N; k0 += AT_K, buf ^= 1) {
        __builtin_amdgcn_s_waitcnt(0x0070);           // vmcnt(0): this wave's plane of the tile has landed
        __syncthreads();                              // ... and everybody's; everybody is done with the other buffer
        if (k0 + AT_K < N) stage(k0 + AT_K, buf ^ 1);
        const char* T = tiles[buf];
        f32x4 sacc[4];          // S^T tiles: key = k0 + 16 nt + 4 g + r, column = query c
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            sacc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int o = nt * 16 * 128 + foff + (((4 * s2 + g) ^ sw) << 4);
                const at_h8 kh = *reinterpret_cast<const at_h8*>(T + o);
                const at_h8 kl = *reinterpret_cast<const at_h8*>(T + AT3_PLANE + o);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[s2], sacc[nt], 0, 0, 0);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[s2], sacc[nt], 0, 0, 0);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[s2], sacc[nt], 0, 0, 0);
            }
        }
        float m = -3.0e38f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + nt * 16 + 4 * g + r;
                const float sv = (key < N) ? sacc[nt][r] * scale : -3.0e38f;
                sacc[nt][r] = sv;
                m = fmaxf(m, sv);
            }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float mnew = fmaxf(mrun, m);
        const float corr = expf(mrun - mnew);
        mrun = mnew;
        float ls = 0.f;
        at_h8 ph[2], pl[2];     // P^T fragments (B operand) of the two 32-key blocks (attn2_kernel's key order)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + nt * 16 + 4 * g + r;
                const float pv = (key < N) ? expf(sacc[nt][r] - mnew) : 0.f;
                ls += pv;
                _Float16 x, y;
                at_split(pv, x, y);
                ph[nt >> 1][4 * (nt & 1) + r] = x;
                pl[nt >> 1][4 * (nt & 1) + r] = y;
            }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        lrun = lrun * corr + ls;
#pragma unroll
        for (int j = 0; j < 4; ++j) oacc[j] *= corr;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = j * 16 * 128 + foff + (((4 * s2 + g) ^ sw) << 4);
                const at_h8 vh = *reinterpret_cast<const at_h8*>(T + 2 * AT3_PLANE + o);
                const at_h8 vl = *reinterpret_cast<const at_h8*>(T + 3 * AT3_PLANE + o);
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl[s2], oacc[j], 0, 0, 0);
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph[s2], oacc[j], 0, 0, 0);
                oacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph[s2], oacc[j], 0, 0, 0);
            }
    }
    const int qi = q0 + c;
    if (qi < N) {
        const float inv = 1.0f / lrun;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<float4*>(out + ((long long)view * N + qi) * dim + head * 64 + j * 16 + 4 * g) =
                make_float4(oacc[j][0] * inv, oacc[j][1] * inv, oacc[j][2] * inv, oacc[j][3] * inv);
        // training form: the row's log-sum-exp of the scaled logits (the four lanes g of a query hold the same value)
        if constexpr (LSE) {
            if (g == 0) lse[((long long)view * heads + head) * N + qi] = mrun + logf(lrun);
        }
    }
}

static int vit_npad(int N) { return (N + 63) / 64 * 64; }

// zero fill of the K / V^T planes as a KERNEL, not hipMemsetAsync: this forward is also replayed as a hipGraph (hip.vit_forward(
// graph=True)), and with the clear as a memset node the replayed graph produced non-finite tokens in a third of the runs of
// tests/test_gpu_parity.py::test_render_sequence_equals_per_frame_render on ROCm 7.2 (0 of 15 with
// DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, 0 of 40 with this kernel; the stem's graph -- kernel nodes only -- never failed; a stand-alone
// memset -> kernel graph does not fail either: tools/ubench/graph_memset_node.py).  profiles/r05_l_vit_graph_memset_node.txt
__global__ __launch_bounds__(256) void zero16_kernel(uint4* __restrict__ p, long long n16) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// few tokens: the register-fed form (more, shorter workgroups); many: the LDS-staged form (64 queries share every K / V
// tile: a quarter of the L2 traffic, which is what bounds the register-fed form from N ~ 1000 on).
// Measured ViT forward, N_c = 300 / 500 / 1500: 0.80 / 0.99 / 2.15 ms register-fed, 0.86 / 1.07 / 2.06 ms LDS-staged.
// (transposed register-fed form, late round 2: 0.77 / 0.95 / 1.19 / 2.06 ms at N_c = 500 / 800 / 1000 / 1500 against 0.93 / 1.16 /
// 1.27 / 1.76 ms LDS-staged)
// (round 6: from N ~ 700 on the third form -- attn2's arithmetic on K / V^T tiles shared through LDS, attn3_kernel)
static bool vit_attn_tile(int N) { return N > 700; }

// "split + attention" of one layer, shared by th_vit_launch, th_attention_launch and th_attention_train_launch:
// qkv [V, N, 3 dim] -> Y [V, N, dim].
// split: write the K / V^T operand planes from qkv here (false when the qkv GEMM's epilogue already did); tile: attn3_kernel.
// lse: nullptr (inference: the kernels as they always were) or [V][heads][N], each row's m + log(l) -- the LSE = true
// instantiations differ from the others by that one store.
static void vit_split_attention(const float* qkv, int V, int N, int Npad, int dim, int heads, bool split, bool tile,
                                _Float16* Kp, _Float16* Vp, float* Y, hipStream_t s, float* lse = nullptr) {
    const float scale = 0.125f;   // head_dim ** -0.5
    if (split) hipLaunchKernelGGL(kv_split_kernel, dim3(Npad / 64, heads, V), dim3(256), 0, s, qkv, N, Npad, dim, Kp, Vp);
    const dim3 g3(th_cdiv(N, 64), heads, V), g2(th_cdiv(N, 16), heads, V);
    float* none = nullptr;
    if (tile && lse) hipLaunchKernelGGL(attn3_kernel<true>, g3, dim3(256), 0, s, qkv, Kp, Vp, N, Npad, dim, scale, Y, lse);
    else if (tile) hipLaunchKernelGGL(attn3_kernel<false>, g3, dim3(256), 0, s, qkv, Kp, Vp, N, Npad, dim, scale, Y, none);
    else if (lse) hipLaunchKernelGGL(attn2_kernel<true>, g2, dim3(64), 0, s, qkv, Kp, Vp, N, Npad, dim, scale, Y, lse);
    else hipLaunchKernelGGL(attn2_kernel<false>, g2, dim3(64), 0, s, qkv, Kp, Vp, N, Npad, dim, scale, Y, none);
}

static bool attn_shape_ok(int V, int N, int heads) {
    return V > 0 && V <= 65535 && N > 0 && N <= (1 << 24) && heads > 0 && heads <= 1024;
}

// the split K / V^T planes of one layer (2 x [V][heads][2][Npad][64] halves); size 0 for a shape th_attention refuses
struct AttnPlanes { _Float16 *Kp, *Vp; };
static AttnPlanes attn_layout(ThArena& ar, int V, int N, int heads) {
    const size_t halves = (size_t)V * heads * 2 * vit_npad(N) * 64;
    return {ar.take<_Float16>(halves), ar.take<_Float16>(halves)};
}
size_t th_attn_ws(int V, int N, int heads) { return attn_shape_ok(V, N, heads) ? th_measure(attn_layout, V, N, heads) : 0; }

// The attention of one layer on its own (tests): kv_split_kernel, then the kernel th_vit_launch would pick (form 0) or a forced
// one (2: attn2_kernel, 3: attn3_kernel).  Every plane element the attention kernels read is written by kv_split_kernel first.
// lse: nullptr, or (the training form) [V][heads][N], from which k_vit_bwd.hip recomputes the probabilities.
int th_attention_train_launch(const float* qkv, int V, int N, int heads, int form, float* out, float* lse, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(attn_shape_ok(V, N, heads), "th_attention: need 1 <= V <= 65535, 1 <= N <= 2^24, 1 <= heads <= 1024");
    TH_REQUIRE(form == 0 || form == 2 || form == 3,
               "th_attention: form must be 0 (the forward's own choice), 2 (attn2_kernel) or 3 (attn3_kernel)");
    TH_REQUIRE((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)lse) & 15) == 0,
               "qkv, out and lse must be 16-byte aligned");
    TH_REQUIRE((((uintptr_t)ws) & 15) == 0, "workspace must be 16-byte aligned");
    ThArena ar(ws, ws_bytes);
    const AttnPlanes p = attn_layout(ar, V, N, heads);
    TH_REQUIRE(ar.ok(), "workspace too small");
    vit_split_attention(qkv, V, N, vit_npad(N), heads * 64, heads, true, form == 0 ? vit_attn_tile(N) : form == 3, p.Kp, p.Vp, out, s,
                        lse);
    TH_LAUNCH_CHECK();
    return 0;
}
int th_attention_launch(const float* qkv, int V, int N, int heads, int form, float* out, void* ws, size_t ws_bytes,
                        hipStream_t s) {
    return th_attention_train_launch(qkv, V, N, heads, form, out, nullptr, ws, ws_bytes, s);
}

// X, Y, qkv (3 dim) / mlp hidden (4 dim), and the attention planes of one layer
struct VitWs { float *X, *Y, *Q; AttnPlanes kv; };
static VitWs vit_layout(ThArena& ar, int V, int N, int dim, int heads) {
    const size_t T = (size_t)V * N;
    return {ar.take<float>(T * dim), ar.take<float>(T * dim), ar.take<float>(T * 4 * dim), attn_layout(ar, V, N, heads)};
}
size_t th_vit_ws(int V, int N, int dim, int heads) { return th_measure(vit_layout, V, N, dim, heads); }

int th_vit_launch(const ThVitPacked& W, const float* x, const float* pe, int V, int N, float* out, void* ws,
                  size_t ws_bytes, hipStream_t s, unsigned int* range, bool allow_h3) {
    TH_REQUIRE(W.ready, "ViT weights not set (th_set_vit_weights)");
    const int dim = W.dim, heads = W.heads;
    TH_REQUIRE(dim == heads * 64, "attention kernel is built for head_dim 64 (ViT-tiny: 192 = 3 x 64)");
    TH_REQUIRE(dim <= 512, "dim too large for the layernorm kernel");
    ThArena ar(ws, ws_bytes);
    VitWs w = vit_layout(ar, V, N, dim, heads);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int T = V * N, Npad = vit_npad(N);
    _Float16 *Kp = w.kv.Kp, *Vp = w.kv.Vp;
    const bool attn_tile = vit_attn_tile(N);
    long long n = (long long)T * dim;
    hipLaunchKernelGGL(add_kernel, dim3(th_cdiv(n, 256)), dim3(256), 0, s, x, pe, n, w.X);
    // the two pre-LayerNorms of a block run inside the GEMM that consumes them
    const bool fuse_ln = th_gemm_ln_ok(T, W.blocks[0].qkv) && th_gemm_ln_ok(T, W.blocks[0].fc1);
    // dense layers on the fp16-split MFMA path (th_gemm_h3)
    const bool h3 = allow_h3 && th_gemm_h3_ok(T, W.blocks[0].qkv, true) && th_gemm_h3_ok(T, W.blocks[0].fc1, true) &&
                    th_gemm_h3_ok(T, W.blocks[0].proj, false) && th_gemm_h3_ok(T, W.blocks[0].fc2, false);
    // the K / V^T operand planes of the register-fed attention are written by the qkv GEMM's epilogue (no kv_split launch);
    // the padding keys (N .. Npad) of the planes must read as zero: cleared once per forward
    const bool fuse_split = h3;
    const ThQkvSplit qs{Kp, Vp, N, Npad, heads, dim};
    if (fuse_split && Npad != N)
    {
        const long long n16 = (long long)((((char*)Vp - (char*)Kp) + (size_t)V * heads * 2 * Npad * 64 * sizeof(_Float16)) / 16);   // Kp .. end of Vp
        hipLaunchKernelGGL(zero16_kernel, dim3((unsigned)(th_cdiv(n16, 256) < 1024 ? th_cdiv(n16, 256) : 1024)), dim3(256), 0, s,
                           reinterpret_cast<uint4*>(Kp), n16);
    }
    for (int b = 0; b < W.depth; ++b) {
        const ThVitBlockPacked& B = W.blocks[b];
        if (h3) {
            TH_TRY(th_gemm_h3(w.X, dim, T, B.qkv, B.ln1_w, B.ln1_b, 1e-6f, TH_ACT_NONE, w.Q, 3 * dim, range, s, fuse_split ? &qs : nullptr));
        } else if (fuse_ln) {
            TH_TRY(th_gemm_ln(w.X, dim, T, B.qkv, B.ln1_w, B.ln1_b, 1e-6f, TH_ACT_NONE, w.Q, 3 * dim, s));
        } else {
            hipLaunchKernelGGL(layernorm_kernel, dim3(th_cdiv(T, 4)), dim3(256), 0, s, w.X, T, dim, B.ln1_w, B.ln1_b, 1e-6f, w.Y);
            TH_TRY(th_gemm(w.Y, dim, T, B.qkv, TH_ACT_NONE, w.Q, 3 * dim, s));
        }
        vit_split_attention(w.Q, V, N, Npad, dim, heads, !fuse_split, attn_tile, Kp, Vp, w.Y, s);
        if (h3) {
            TH_TRY(th_gemm_h3(w.Y, dim, T, B.proj, nullptr, nullptr, 0.f, TH_ACT_NONE | TH_GEMM_ACCUM, w.X, dim, range, s));
            TH_TRY(th_gemm_h3(w.X, dim, T, B.fc1, B.ln2_w, B.ln2_b, 1e-6f, TH_ACT_GELU, w.Q, 4 * dim, range, s));
            TH_TRY(th_gemm_h3(w.Q, 4 * dim, T, B.fc2, nullptr, nullptr, 0.f, TH_ACT_NONE | TH_GEMM_ACCUM, w.X, dim, range, s));
            continue;
        }
        TH_TRY(th_gemm(w.Y, dim, T, B.proj, TH_ACT_NONE | TH_GEMM_ACCUM, w.X, dim, s));
        if (fuse_ln) {
            TH_TRY(th_gemm_ln(w.X, dim, T, B.fc1, B.ln2_w, B.ln2_b, 1e-6f, TH_ACT_GELU, w.Q, 4 * dim, s));
        } else {
            hipLaunchKernelGGL(layernorm_kernel, dim3(th_cdiv(T, 4)), dim3(256), 0, s, w.X, T, dim, B.ln2_w, B.ln2_b, 1e-6f, w.Y);
            TH_TRY(th_gemm(w.Y, dim, T, B.fc1, TH_ACT_GELU, w.Q, 4 * dim, s));
        }
        TH_TRY(th_gemm(w.Q, 4 * dim, T, B.fc2, TH_ACT_NONE | TH_GEMM_ACCUM, w.X, dim, s));
    }
    hipLaunchKernelGGL(layernorm_kernel, dim3(th_cdiv(T, 4)), dim3(256), 0, s, w.X, T, dim, W.norm_w, W.norm_b, 1e-6f, out);
    TH_LAUNCH_CHECK();
    return 0;
}
