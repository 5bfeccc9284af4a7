// K27: cfg.use_truncation -- drop the samples whose nearest token centre is KNN_SIGMA or farther away.
//
// Network.get_human_representation (cross_transformer.py:175-180): mask_preserve = knn_dist.min(-1) < cfg.KNN_SIGMA, the
// comparison in fp32; Network.forward's _forward (:247-264) runs the per-point network on the preserved samples only and
// leaves raw = 0 for the others.  Here: the mask and the ascending list of preserved samples (th_truncate_select), the
// scatter of the preserved rows back to all samples and its adjoint (th_truncate_scatter / _bwd), and the frame paths' form
// of the same thing: zero the dense raw rows of the dropped samples behind the shading (th_truncate_zero_launch).
//
// The distance is K4's: dp_nearest_d2 (k_dparf_near.h) scans with K4's own expression, over K4's candidate grid where there
// is one, so sqrtf(d2min) is bit for bit the distance of K4's first neighbour.
//
// th_truncate_select is an ordered compaction in three launches, without atomics and without one workgroup waiting for
// another:
//   tr_mask_kernel   one lane per sample: the test, mask[p], and the workgroup's count of kept samples (wave ballots, summed
//                    through LDS) -> blk[b]
//   tr_scan_kernel   ONE workgroup: exclusive prefix of blk[] -> off[], the total -> count
//   tr_emit_kernel   one lane per sample again: rank inside the wave by ballot, inside the workgroup through LDS, + off[b]
// mask, sel[0 .. count), count, blk and off are each stored exactly once and nothing is read before it is written, so the
// result neither depends on what the buffers held nor differs between runs.
// th_truncate_scatter needs the inverse of sel: a workgroup finds the slot of its first sample by one binary search in the
// (ascending) list, the lanes behind it by ballot ranks -- every row of the output is stored once, kept or zero.
// Bounds: all of them are launch-latency bound at the sizes of a training step (P = 153 600: 600 workgroups); tr_mask_kernel
// is VALU bound beyond that (N_c, or ~55 with the grid, distance evaluations per sample against 13 bytes of traffic), the
// others move 5 .. 36 bytes per sample.
#include "th_internal.h"
#include "k_dparf_near.h"

#define TR_THREADS 256
#define TR_WAVES (TR_THREADS / 64)
#define TR_SCAN_THREADS 1024

__device__ __forceinline__ bool tr_keep(float d2min, float sigma) { return __fsqrt_rn(d2min) < sigma; }

// exclusive rank of this lane's flag inside the workgroup and the workgroup's total; every thread of the workgroup calls it
__device__ __forceinline__ int tr_block_rank(bool flag, int* wsum /* [TR_WAVES] LDS */, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w) {
        const int c = wsum[w];
        base += (w < wave) ? c : 0;
        sum += c;
    }
    total = sum;
    return base + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(TR_THREADS) void tr_mask_kernel(const float* __restrict__ pts, int P, const float* __restrict__ centres,
                                                             int nc, float sigma, const DpGrid* __restrict__ gi,
                                                             const int* __restrict__ cell_count, const int* __restrict__ cand,
                                                             uint8_t* __restrict__ mask, int32_t* __restrict__ blk) {
    __shared__ int wsum[TR_WAVES];
    const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    bool keep = false;
    if (p < P) {
        keep = tr_keep(dp_nearest_d2(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], centres, nc, gi, cell_count, cand), sigma);
        mask[p] = keep ? 1 : 0;
    }
    int total;
    (void)tr_block_rank(keep, wsum, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: off[b] = blk[0] + .. + blk[b - 1], count[0] = the sum of all nb
__global__ __launch_bounds__(TR_SCAN_THREADS) void tr_scan_kernel(const int32_t* __restrict__ blk, int nb, int32_t* __restrict__ off,
                                                                  int32_t* __restrict__ count) {
    __shared__ int wsum[TR_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nb; base += TR_SCAN_THREADS) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? blk[i] : 0;
        int incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int wbase = 0, all = 0;
        for (int w = 0; w < TR_SCAN_THREADS / 64; ++w) {
            const int c = wsum[w];
            wbase += (w < wave) ? c : 0;
            all += c;
        }
        if (i < nb) off[i] = carry + wbase + incl - v;
        carry += all;
        __syncthreads();                                   // (wsum is rewritten by the next round)
    }
    if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(TR_THREADS) void tr_emit_kernel(const uint8_t* __restrict__ mask, int P, const int32_t* __restrict__ off,
                                                             int32_t* __restrict__ sel) {
    __shared__ int wsum[TR_WAVES];
    const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    const bool keep = p < P && mask[p] != 0;
    int total;
    const int r = tr_block_rank(keep, wsum, total);
    if (keep) sel[off[blockIdx.x] + r] = (int32_t)p;      // (off[b] + rank < count <= P: inside sel)
}

// rows [P][4]: rows[sel[j]] = rows_c[j], every other row 0
__global__ __launch_bounds__(TR_THREADS) void tr_scatter_kernel(const float4* __restrict__ rows_c, const uint8_t* __restrict__ mask,
                                                                const int32_t* __restrict__ sel, int n, int P,
                                                                float4* __restrict__ rows) {
    __shared__ int wsum[TR_WAVES];
    __shared__ int first;
    if (threadIdx.x == 0) {
        // the number of list entries below this workgroup's first sample = the slot of its first kept sample
        const long long p0 = (long long)blockIdx.x * TR_THREADS;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (sel[mid] < p0) lo = mid + 1; else hi = mid;
        }
        first = lo;
    }
    const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    const bool keep = p < P && mask[p] != 0;
    int total;
    const int r = tr_block_rank(keep, wsum, total);       // (its barrier also publishes `first`)
    if (p < P) {
        const int j = first + r;
        // (a mask and a list that disagree must not read outside rows_c: such a row is zero)
        rows[p] = (keep && j < n) ? rows_c[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the adjoint: g_c[j] = g[sel[j]]
__global__ __launch_bounds__(TR_THREADS) void tr_gather_kernel(const float4* __restrict__ g, const int32_t* __restrict__ sel, int n,
                                                               int P, float4* __restrict__ g_c) {
    const int j = blockIdx.x * TR_THREADS + threadIdx.x;
    if (j >= n) return;
    const int q = sel[j];
    g_c[j] = (q >= 0 && q < P) ? g[q] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// frame paths: raw[q] = 0 for the listed samples q = idx[i] whose nearest centre is sigma or farther away
__global__ __launch_bounds__(TR_THREADS) void tr_zero_kernel(ThPointSrc ps, const float* __restrict__ Rh, const float* __restrict__ Th,
                                                             const int32_t* __restrict__ idx, int n, const float* __restrict__ centres,
                                                             int nc, float sigma, const DpGrid* __restrict__ gi,
                                                             const int* __restrict__ cell_count, const int* __restrict__ cand,
                                                             float4* __restrict__ raw) {
    const int i = blockIdx.x * TR_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long q = idx[i];
    float wx, wy, wz, x, y, z;
    th_get_point(ps, q, wx, wy, wz);
    dp_world2smpl(wx, wy, wz, Rh, Th, x, y, z);
    if (!tr_keep(dp_nearest_d2(x, y, z, centres, nc, gi, cell_count, cand), sigma)) raw[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

static size_t tr_blocks(long long P) { return (size_t)((P + TR_THREADS - 1) / TR_THREADS); }

// per block of samples the kept count and its scanned offset, and K4's candidate grid of the centres
struct TrWs { int32_t *blk, *off; size_t gws_b; void* gws; };
static TrWs tr_layout(ThArena& ar, int P, int nc) {
    const size_t nb = tr_blocks(P > 0 ? P : 0), gws_b = th_dparf_grid_ws(nc > 0 ? nc : 1);
    return {ar.take<int32_t>(nb > 0 ? nb : 1), ar.take<int32_t>(nb > 0 ? nb : 1), gws_b, ar.take<char>(gws_b)};
}
size_t th_truncate_select_ws(int P, int nc) { return th_measure(tr_layout, P, nc); }

int th_truncate_select_launch(const float* pts_smpl, int P, const float* centres, int nc, float sigma, uint8_t* mask, int32_t* sel,
                              int32_t* count, void* ws, size_t ws_bytes, bool use_grid, hipStream_t s) {
    TH_REQUIRE(P >= 0 && nc >= 1, "th_truncate_select: P >= 0 and at least one token centre");
    const int nb = (int)tr_blocks(P);
    ThArena ar(ws, ws_bytes);
    TrWs w = tr_layout(ar, P, nc);
    TH_REQUIRE(ar.ok(), "th_truncate_select: workspace too small");
    DpGridView gv{nullptr, nullptr, nullptr};
    if (use_grid && P > 0 && th_dparf_grid_ok(nc)) {
        TH_TRY(th_dparf_grid_build(centres, nc, w.gws, w.gws_b, s));
        gv = dp_grid_view(w.gws, nc);
    }
    if (nb > 0) {
        hipLaunchKernelGGL(tr_mask_kernel, dim3(nb), dim3(TR_THREADS), 0, s, pts_smpl, P, centres, nc, sigma, gv.gi, gv.cell_count,
                           gv.cand, mask, w.blk);
    }
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), dim3(TR_SCAN_THREADS), 0, s, w.blk, nb, w.off, count);
    if (nb > 0) hipLaunchKernelGGL(tr_emit_kernel, dim3(nb), dim3(TR_THREADS), 0, s, mask, P, w.off, sel);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_truncate_scatter_launch(const float* rows_c, const uint8_t* mask, const int32_t* sel, int n, int P, float* rows, hipStream_t s) {
    TH_REQUIRE(P >= 0 && n >= 0 && n <= P, "th_truncate_scatter: 0 <= n <= P");
    if (P == 0) return 0;
    hipLaunchKernelGGL(tr_scatter_kernel, dim3((unsigned)tr_blocks(P)), dim3(TR_THREADS), 0, s, (const float4*)rows_c, mask, sel, n, P,
                       (float4*)rows);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_truncate_gather_launch(const float* g, const int32_t* sel, int n, int P, float* g_c, hipStream_t s) {
    TH_REQUIRE(P >= 0 && n >= 0 && n <= P, "th_truncate_scatter_bwd: 0 <= n <= P");
    if (n == 0) return 0;
    hipLaunchKernelGGL(tr_gather_kernel, dim3((unsigned)tr_blocks(n)), dim3(TR_THREADS), 0, s, (const float4*)g, sel, n, P, (float4*)g_c);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_truncate_zero_launch(const ThPointSrc& ps, const float* Rh, const float* Th, const int32_t* idx, int n, const float* centres,
                            int nc, float sigma, const void* grid_ws, float* raw, hipStream_t s) {
    if (n <= 0) return 0;
    TH_REQUIRE(nc >= 1, "th_set_truncation: at least one token centre");
    const DpGridView gv = dp_grid_view(grid_ws, nc);
    hipLaunchKernelGGL(tr_zero_kernel, dim3((unsigned)tr_blocks(n)), dim3(TR_THREADS), 0, s, ps, Rh, Th, idx, n, centres, nc, sigma, gv.gi,
                       gv.cell_count, gv.cand, (float4*)raw);
    TH_LAUNCH_CHECK();
    return 0;
}
