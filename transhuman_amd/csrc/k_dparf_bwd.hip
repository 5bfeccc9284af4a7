// K4 backward: the adjoint of the token blend of k_dparf.hip with respect to the tokens.
//
// Forward (per sample p, view v):  out[p,v,:192] = sum_k w_k(p) tokens[v, idx_k(p), :].  Its adjoint is
//   grad_tokens[v,c,:] = sum over the records (p,k) with idx_k(p) = c of  w_k(p) * grad_out[p,v,:192]
// -- 7 P contribution rows onto N_c destination rows (2.5 GB onto 500 rows at the training shape).  A float-atomic scatter
// onto so few rows runs an order of magnitude under the atomic rate and its sums depend on arrival order, so the sum is done
// per DESTINATION through an inverted index, without any float atomic:
//   1. records  the forward's own selection (dparf_kernel<false, -2, K>, TH_ROWS_REC): idx[7], w[7] per sample -- the same
//               statements as the forward that produced the loss, so no neighbour can differ between the two.  With
//               cfg.KNN = K < 7 the record's pairs K..6 are idx = -1, w = 0: the rank pass drops them (`c >= 0`) while the
//               workspace stays sized for 7 P entries;
//   2. count    one wave per unit of 256 consecutive samples: how many records of the unit name each centre -> cnt[c][unit];
//   3. scan     exclusive prefix over (centre major, unit minor): the start of every (centre, unit) segment; the start of a
//               centre's list is the start of its first segment;
//   4. fill     the count pass again, now writing (sample, weight) entries: inside a segment the order is (64-sample pass,
//               k, lane) -- a function of the input alone (ranks come from wave ballots, not from atomics);
//   5. partial  lists are cut into chunks of DPB_CHUNK entries; one wave per (chunk, view) adds its entries in list order
//               (48 lanes x float4 = the 192 token channels; 768 contiguous bytes of grad_out per entry);
//   6. reduce   one wave per (centre, view) adds the centre's partial rows in chunk order and writes the row -- zeros for a
//               centre nobody selected, so the output needs no clearing.
// Every step is a fixed function of the inputs: the result is bit-identical from run to run.
// Bound: reading 7 P V rows of 768 B back (L2 / HBM), ~1 ms at P = 153 600, V = 3.
#include "th_internal.h"

#define DPB_K 7
#define DPB_UNIT 256          // samples per counting unit (one wave, four passes of 64)
#define DPB_CHUNK 256         // list entries per partial sum
#define DPB_SCAN_T 1024

struct DpbPlan {
    size_t rec, off, nch, ent, part, total;
    int units, maxchunks;
};
static DpbPlan dpb_plan(int P, int V, int nc) {
    DpbPlan p;
    p.units = th_cdiv(P, DPB_UNIT);
    p.maxchunks = th_cdiv((long long)DPB_K * P, DPB_CHUNK) + nc;
    size_t o = 0;
    p.rec = o;  o += th_align((size_t)P * 16 * 4);
    p.off = o;  o += th_align(((size_t)nc * p.units + 1) * 4);
    p.nch = o;  o += th_align(((size_t)nc + 1) * 4);
    p.ent = o;  o += th_align((size_t)DPB_K * P * 8);
    p.part = o; o += th_align((size_t)p.maxchunks * V * 192 * 4);
    p.total = o;
    return p;
}
size_t th_dparf_bwd_ws(int P, int V, int nc) {
    if (P <= 0 || V <= 0 || nc <= 0) return 256;
    return dpb_plan(P, V, nc).total;
}

// One wave per unit.  FILL = false: cnt[c * units + u] = number of the unit's records that name centre c.
// FILL = true: `cnt` holds the scanned segment starts; entry (sample, weight) goes to start + rank.
template <bool FILL>
__global__ __launch_bounds__(64) void dpb_rank_kernel(const unsigned* __restrict__ rec, int P, int nc, int units,
                                                      int* __restrict__ cnt, int2* __restrict__ ent) {
    extern __shared__ int lcnt[];                       // [nc]
    const int lane = threadIdx.x, u = blockIdx.x;
    for (int c = lane; c < nc; c += 64) lcnt[c] = FILL ? cnt[(long long)c * units + u] : 0;
    __syncthreads();
    for (int pass = 0; pass < DPB_UNIT / 64; ++pass) {
        const int p = u * DPB_UNIT + pass * 64 + lane;
        for (int k = 0; k < DPB_K; ++k) {
            int c = -1;
            unsigned wbits = 0u;
            if (p < P) {
                c = (int)rec[(long long)p * 16 + k];
                wbits = rec[(long long)p * 16 + 8 + k];
            }
            const bool act = c >= 0 && c < nc;          // (a record outside the table is dropped, never followed)
            // rank of this lane among the lanes that name the same centre, and the size of that group
            bool done = !act;
            int rank = 0, total = 0;
            bool leader = false;
            for (;;) {
                const unsigned long long todo = __ballot(!done);
                if (todo == 0ull) break;
                const int first = __ffsll((long long)todo) - 1;
                const int cc = __shfl(c, first);
                const bool mine = !done && c == cc;
                const unsigned long long m = __ballot(mine);
                if (mine) {
                    rank = __popcll(m & ((1ull << lane) - 1ull));
                    total = __popcll(m);
                    leader = lane == first;
                    done = true;
                }
            }
            int base = 0;
            if (act) base = lcnt[c];
            __syncthreads();                             // (one wave: every read of this round precedes its writes)
            if (FILL && act) ent[base + rank] = make_int2(p, (int)wbits);
            if (leader) lcnt[c] = base + total;
            __syncthreads();
        }
    }
    if (!FILL)
        for (int c = lane; c < nc; c += 64) cnt[(long long)c * units + u] = lcnt[c];
}

// in-place exclusive prefix sum of data[0 .. n), the total goes to data[n]; one workgroup
__global__ __launch_bounds__(DPB_SCAN_T) void dpb_scan_kernel(int* __restrict__ data, long long n) {
    __shared__ int part[DPB_SCAN_T];
    const int t = threadIdx.x;
    const long long span = (n + DPB_SCAN_T - 1) / DPB_SCAN_T;
    const long long a = min(n, t * span), b = min(n, a + span);
    int s = 0;
    for (long long i = a; i < b; ++i) s += data[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < DPB_SCAN_T; o <<= 1) {
        const int x = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int run = part[t] - s;                               // exclusive prefix of this thread's span
    for (long long i = a; i < b; ++i) {
        const int x = data[i];
        data[i] = run;
        run += x;
    }
    if (t == DPB_SCAN_T - 1) data[n] = part[t];
}

// nch[c] = number of chunks of centre c's list
__global__ void dpb_nchunk_kernel(const int* __restrict__ off, int nc, int units, int* __restrict__ nch) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int len = off[(long long)(c + 1) * units] - off[(long long)c * units];
    nch[c] = (len + DPB_CHUNK - 1) / DPB_CHUNK;
}

// one wave per (chunk, view): part[chunk][v][192] = sum of the chunk's entries, in list order
__global__ __launch_bounds__(64) void dpb_partial_kernel(const int* __restrict__ off, const int* __restrict__ cbase, int nc,
                                                         int units, const int2* __restrict__ ent,
                                                         const float* __restrict__ gout, int V, float* __restrict__ part) {
    const int j = blockIdx.x, v = blockIdx.y, lane = threadIdx.x;
    if (j >= cbase[nc]) return;
    // the centre whose chunk range holds j: cbase[c] <= j < cbase[c + 1]
    int lo = 0, hi = nc;                                 // invariant: cbase[lo] <= j < cbase[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cbase[mid] <= j) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int e0 = off[(long long)c * units] + (j - cbase[c]) * DPB_CHUNK;
    const int e1 = min(e0 + DPB_CHUNK, off[(long long)(c + 1) * units]);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 48) {
        const float* g = gout + (long long)v * 256 + 4 * lane;
        for (int e = e0; e < e1; e += 8) {
            float4 r[8];
            float w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {                // eight row loads in flight (ragged tail: duplicate loads)
                const int2 en = ent[min(e + i, e1 - 1)];
                w[i] = __builtin_bit_cast(float, en.y);
                r[i] = *reinterpret_cast<const float4*>(g + (long long)en.x * V * 256);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (e + i < e1) {
                    acc.x = fmaf(w[i], r[i].x, acc.x); acc.y = fmaf(w[i], r[i].y, acc.y);
                    acc.z = fmaf(w[i], r[i].z, acc.z); acc.w = fmaf(w[i], r[i].w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4*>(part + ((long long)j * V + v) * 192 + 4 * lane) = acc;
    }
}

// one wave per (centre, view): the centre's partial rows added in chunk order
__global__ __launch_bounds__(64) void dpb_reduce_kernel(const int* __restrict__ cbase, int nc, int V,
                                                        const float* __restrict__ part, float* __restrict__ gtok) {
    const int c = blockIdx.x, v = blockIdx.y, lane = threadIdx.x;
    if (lane >= 48) return;
    const int j0 = cbase[c], j1 = cbase[c + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = j0; j < j1; ++j) {
        const float4 r = *reinterpret_cast<const float4*>(part + ((long long)j * V + v) * 192 + 4 * lane);
        if (j == j0) acc = r;
        else { acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += r.w; }
    }
    *reinterpret_cast<float4*>(gtok + ((long long)v * nc + c) * 192 + 4 * lane) = acc;
}

int th_dparf_bwd_launch(const float* pts_smpl, int P, const float* centres, const float* rot, int V, int nc, const ThDparfParams& dp,
                        const float* grad_out, float* grad_tokens, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(dp.knn >= 1 && dp.knn <= DPB_K, "KNN 1..7");
    if (!(P >= 0 && V >= 1 && nc >= dp.knn)) TH_FAIL("need P >= 0, V >= 1 and at least " + std::to_string(dp.knn) + " token centres");
    TH_REQUIRE(P <= (1 << 27) && V <= 65535, "too many samples or views");
    TH_REQUIRE((size_t)nc * 4 <= 64 * 1024, "too many token centres for the counting pass (16384)");
    if (P == 0) {
        TH_HIP(hipMemsetAsync(grad_tokens, 0, (size_t)V * nc * 192 * sizeof(float), s));
        return 0;
    }
    const DpbPlan pl = dpb_plan(P, V, nc);
    TH_REQUIRE(ws != nullptr && ws_bytes >= pl.total, "workspace too small (th_dparf_encode_bwd_workspace_bytes)");
    TH_REQUIRE((long long)nc * pl.units < (1ll << 30), "too many (centre, unit) segments");
    char* b = (char*)ws;
    unsigned* rec = (unsigned*)(b + pl.rec);
    int* off = (int*)(b + pl.off);
    int* nch = (int*)(b + pl.nch);
    int2* ent = (int2*)(b + pl.ent);
    float* part = (float*)(b + pl.part);
    TH_TRY(th_dparf_launch(pts_smpl, nullptr, nullptr, nullptr, nullptr, P, centres, rot, nullptr, V, nc, dp, (float*)rec,
                           nullptr, TH_ROWS_REC, nullptr, s));
    hipLaunchKernelGGL(dpb_rank_kernel<false>, dim3(pl.units), dim3(64), (size_t)nc * 4, s, rec, P, nc, pl.units, off, ent);
    hipLaunchKernelGGL(dpb_scan_kernel, dim3(1), dim3(DPB_SCAN_T), 0, s, off, (long long)nc * pl.units);
    hipLaunchKernelGGL(dpb_rank_kernel<true>, dim3(pl.units), dim3(64), (size_t)nc * 4, s, rec, P, nc, pl.units, off, ent);
    hipLaunchKernelGGL(dpb_nchunk_kernel, dim3(th_cdiv(nc, 256)), dim3(256), 0, s, off, nc, pl.units, nch);
    hipLaunchKernelGGL(dpb_scan_kernel, dim3(1), dim3(DPB_SCAN_T), 0, s, nch, (long long)nc);
    hipLaunchKernelGGL(dpb_partial_kernel, dim3(pl.maxchunks, V), dim3(64), 0, s, off, nch, nc, pl.units, ent, grad_out, V,
                       part);
    hipLaunchKernelGGL(dpb_reduce_kernel, dim3(nc, V), dim3(64), 0, s, nch, nc, V, part, grad_tokens);
    TH_LAUNCH_CHECK();
    return 0;
}
