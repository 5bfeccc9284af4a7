// K19, ordered form: the adjoint of the latent gather (k_latgather.hip) with no float atomic, bit-identical from run to run.
//
// The atomic form scatters: every (sample, view) pair adds coef * g onto at most 27 latent texels.  This form gathers: every
// latent texel sums the pairs that reach it, one wave per texel (lane = channel), in an order that is a function of the inputs
// alone.  No float atomic and no integer atomic in global memory; nothing is cleared beforehand and every output element is
// stored exactly once, so neither the outputs' nor the workspace's earlier contents can show.
//
// The index.  All three levels' slot origins (a_l, b_l) are ups_coord's first tap of the sample's map corner (y0, x0)
// (lg_level), and floor(fl(s y)) is monotone in y: the pairs whose origin lies in [r - 2, r] x [c - 2, c] -- the only ones
// whose 3 x 3 slots can contain texel (r, c), also at the clamped last row / column, where a <= h - 1 keeps a in that range --
// are the pairs of a contiguous range of map rows, and in each of those rows of a contiguous range of map columns.  So ONE
// sort serves all three levels:
//   lgo_keys     key[e] = (v H + y0) W + x0 of pair e = p V + v (th_project + th_bilinear_setup through lg_setup), val[e] = e
//   lgo_hist / lgo_scan / lgo_scatter   a stable least-significant-digit radix sort of (key, val) by 8-bit digits, as many passes
//                as V H W - 1 has bytes: tiles of LGO_TILE pairs per workgroup, per-(digit, tile) counts, one exclusive scan, and a
//                scatter that ranks equal digits by (round, wave, lane) with ballots -- positions are computed, not drawn from
//                a ticket, so equal keys keep ascending e (= ascending sample index p: the key holds v)
//   lgo_csr      start[k] = the first sorted position whose key is >= k (a binary search per map pixel), start[V H W] = N
// The sum.  lgo_sum<NC, NW>: texel (v, r, c) of a level finds its map-row range [ylo, yhi) and column range [xlo, xhi) by
// binary search on ups_coord itself (no closed form to get wrong), walks the rows in ascending y0 and in each the one CSR
// segment start[(v H + y) W + xlo] .. start[(v H + y) W + xhi] in sorted order: the texel's list, in ascending (y0, x0, p).
// The list is cut into batches of LGO_B = 64 pairs: lane i re-derives pair i's coefficients with lg_setup + lg_level (the
// forward's own, bit for bit) and marks the slots k with cf[k] != 0 and lg_slot_index(a, b, k) == this texel; the wave then
// goes through the 64 in order (four rows of g requested at a time) and, per pair, through the marked slots in ascending k,
// doing acc = acc + coef * g[e, c0 + lane] (product rounded, then the sum: the operation of the atomic form) on one fp32
// accumulator per channel.  The coarser levels have the longer lists (about 9 / scale^2 map pixels reach a texel), so NW = 1,
// 2 or 4 waves share a texel (lgo_waves: by the map pixels per texel, a function of the dimensions alone): wave j takes
// batches j, j + NW, ... and the NW partial rows are added through LDS in wave order.  A texel nobody reaches stores 0.
//   order of one texel's sum: partial_j = the pairs of batches j, j + NW, ... in ascending (y0, x0, p), per pair the slots in
//   ascending k, one running fp32 sum; result = (..(partial_0 + partial_1) + ..) + partial_{NW-1}.
// The lift.  g_w[ch, j] = sum over rows of g[row, 256 + ch] rgb_s[row, j], g_b[ch] = sum of g[row, 256 + ch]:
//   lgo_lift_part   chunks of LGO_LIFT_ROWS consecutive rows, thread = channel, four running sums in row order -> part[chunk]
//   lgo_lift_sum    per output 64 lanes: lane i adds partials i, i + 64, ... in ascending order, then a fixed xor butterfly
#include "th_internal.h"
#include "k_latgather.h"

#define LGO_B 64            // pairs per batch of the sum kernel (one per lane)
#define LGO_ROUND 256       // pairs per round of a sort tile (one per thread)
#define LGO_TILE 2048       // pairs per sort tile = per workgroup of lgo_hist / lgo_scatter
#define LGO_LIFT_ROWS 256   // rows per partial of the lift's gradient

__global__ __launch_bounds__(256) void lgo_keys_kernel(int V, int H, int W, const float* __restrict__ pts_world, int N,
                                                       const float* __restrict__ cams, const float* __restrict__ scale,
                                                       unsigned* __restrict__ key, unsigned* __restrict__ val) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const int v = e % V;
    const Bilin bl = lg_setup(pts_world, e / V, cams + 21 * v, scale, H, W);
    key[e] = (unsigned)((v * H + bl.y0) * W + bl.x0);
    val[e] = (unsigned)e;
}

// cnt[d * ntile + tile] = the number of pairs of the tile whose digit is d
__global__ __launch_bounds__(256) void lgo_hist_kernel(const unsigned* __restrict__ key, int N, int shift, int ntile,
                                                       int* __restrict__ cnt) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * LGO_TILE;
    for (int r = 0; r < LGO_TILE / LGO_ROUND; ++r) {
        const int i = base + r * LGO_ROUND + threadIdx.x;
        if (i < N) atomicAdd(&h[(key[i] >> shift) & 255], 1);      // (LDS integer count: the total does not depend on order)
    }
    __syncthreads();
    cnt[threadIdx.x * ntile + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of cnt[0 .. n) in place, one workgroup: 1024 consecutive elements per step (a wave scan, then the 16 wave
// totals), the loads of eight steps requested together
__global__ __launch_bounds__(1024) void lgo_scan_kernel(int* __restrict__ cnt, int n) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 8 * 1024) {
        int x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = base + j * 1024 + t;
            x[j] = i < n ? cnt[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int s = x[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(s, d, 64);
                if (lane >= d) s += y;
            }
            if (lane == 63) wsum[wv] = s;
            __syncthreads();
            int off = 0, tot = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int z = wsum[q];
                off += q < wv ? z : 0;
                tot += z;
            }
            __syncthreads();
            const int i = base + j * 1024 + t;
            if (i < n) cnt[i] = carry + off + s - x[j];
            carry += tot;
        }
    }
}

// the stable scatter of one pass: the pairs of a tile go out in (round, wave, lane) order within each digit
__global__ __launch_bounds__(256) void lgo_scatter_kernel(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                          int N, int shift, int ntile, const int* __restrict__ off,
                                                          unsigned* __restrict__ key_out, unsigned* __restrict__ val_out) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    base[t] = off[t * ntile + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
    __syncthreads();
    const int tile0 = blockIdx.x * LGO_TILE;
    for (int r = 0; r < LGO_TILE / LGO_ROUND; ++r) {
        const int i = tile0 + r * LGO_ROUND + t;
        const bool ok = i < N;
        const unsigned k = ok ? key[i] : 0u, x = ok ? val[i] : 0u;
        const int d = (int)((k >> shift) & 255u);
        unsigned long long same = __ballot(ok);                       // the lanes of this wave with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bb = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? bb : ~bb;
        }
        const int below = __popcll(same & ((1ull << lane) - 1ull));
        if (ok && below == 0) wcnt[wv][d] = __popcll(same);            // (one writer per (wave, digit): the lowest lane)
        __syncthreads();
        if (ok) {
            int pos = base[d] + below;
            for (int w = 0; w < wv; ++w) pos += wcnt[w][d];
            key_out[pos] = k;                                          // (pos < N: the counts of a pass add up to N)
            val_out[pos] = x;
        }
        __syncthreads();
        base[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
#pragma unroll
        for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
        __syncthreads();
    }
}

// start[k] = the first position of the sorted keys that holds a key >= k, k = 0 .. nb (start[nb] = N)
__global__ __launch_bounds__(256) void lgo_csr_kernel(const unsigned* __restrict__ key, int N, int nb, int* __restrict__ start) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > nb) return;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if ((long long)key[mid] >= k) hi = mid; else lo = mid + 1;
    }
    start[k] = lo;
}

// the first map row / column in [0, out) whose first upsample tap is >= target (out if there is none); ups_coord's i0 is
// monotone in dst
__device__ __forceinline__ int lgo_first_ge(int target, int in, int out) {
    int lo = 0, hi = out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int i0, i1;
        float l0, l1;
        ups_coord(mid, in, out, i0, i1, l0, l1);
        if (i0 >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <int NC, int NW>   // NC = channels / 64 of the level, NW = waves per texel (1, 2 or 4)
__global__ __launch_bounds__(256) void lgo_sum_kernel(int h, int w, int V, int H, int W, const float* __restrict__ pts_world,
                                                      int N, const float* __restrict__ cams, const float* __restrict__ scale,
                                                      const float* __restrict__ gout, int ldo, int col0,
                                                      const unsigned* __restrict__ val, const int* __restrict__ start,
                                                      float* __restrict__ glat) {
    __shared__ float part[4][64 * NC];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = wv % NW;                                           // this wave takes the batches sub, sub + NW, ...
    const long long tex = (long long)blockIdx.x * (4 / NW) + wv / NW;
    const long long ntex = (long long)V * h * w;
    const bool live = tex < ntex;
    const int v = live ? (int)(tex / ((long long)h * w)) : 0;
    const int rc = live ? (int)(tex - (long long)v * h * w) : 0;
    const int r = rc / w, c = rc - r * w;
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    const float* cam = cams + 21 * v;

    int my_e = 0, fill = 0, batch = 0;
    // the batch held in lanes 0 .. n - 1: set-up per lane, then the pairs in lane order, the rows of four requested together
    auto flush = [&](int n) {
        const Bilin bl = lg_setup(pts_world, my_e / V, cam, scale, H, W);
        int a, b;
        float cf[9];
        lg_level(bl, h, w, H, W, a, b, cf);
        int m = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) m |= (cf[k] != 0.f && lg_slot_index(a, b, k, h, w) == rc) ? (1 << k) : 0;
        if (lane >= n) m = 0;
        unsigned long long todo = __ballot(m != 0);
        while (todo) {
            int ii[4], mm[4];
            float g[4][NC];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                              // (past the last pair: the first one again, no slot marked)
                const bool has = todo != 0;
                ii[u] = has ? __builtin_ctzll(todo) : ii[0];
                todo = has ? (todo & (todo - 1)) : 0;
                mm[u] = has ? __builtin_amdgcn_readlane(m, ii[u]) : 0;
                const float* grow = gout + (long long)__builtin_amdgcn_readlane(my_e, ii[u]) * ldo + col0;
#pragma unroll
                for (int j = 0; j < NC; ++j) g[u][j] = grow[64 * j + lane];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float cc = lg_lane_f(cf[k], ii[u]);
                    if ((mm[u] >> k) & 1) {
#pragma unroll
                        for (int j = 0; j < NC; ++j) acc[j] = acc[j] + cc * g[u][j];
                    }
                }
        }
    };

    if (live && N > 0) {
        const int ylo = lgo_first_ge(r - 2, h, H), yhi = lgo_first_ge(r + 1, h, H);
        const int xlo = lgo_first_ge(c - 2, w, W), xhi = lgo_first_ge(c + 1, w, W);
        for (int y = ylo; y < yhi; y += 64) {                          // the segment ends of 64 rows at a time, one row per lane
            const int nr = min(64, yhi - y);
            int seg_s = 0, seg_e = 0;
            if (lane < nr) {
                const long long row = ((long long)v * H + y + lane) * W;
                seg_s = start[row + xlo];
                seg_e = start[row + xhi];
            }
            for (int j = 0; j < nr; ++j) {
                int s = __builtin_amdgcn_readlane(seg_s, j);
                const int e = __builtin_amdgcn_readlane(seg_e, j);
                while (s < e) {
                    const int n = min(LGO_B - fill, e - s);
                    const bool mine = batch % NW == sub;
                    if (mine && lane >= fill && lane < fill + n) my_e = (int)val[s + (lane - fill)];
                    fill += n;
                    s += n;
                    if (fill == LGO_B) {
                        if (mine) flush(LGO_B);
                        fill = 0;
                        ++batch;
                    }
                }
            }
        }
        if (fill > 0 && batch % NW == sub) flush(fill);
    }
    if (NW == 1) {
        if (live) {
#pragma unroll
            for (int j = 0; j < NC; ++j) glat[tex * (64 * NC) + 64 * j + lane] = acc[j];
        }
    } else {
        // the texel's NW partial rows, added in wave order
#pragma unroll
        for (int j = 0; j < NC; ++j) part[wv][64 * j + lane] = acc[j];
        __syncthreads();
        if (live && sub == 0) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                float t = part[wv][64 * j + lane];
#pragma unroll
                for (int u = 1; u < NW; ++u) t = t + part[wv + u][64 * j + lane];
                glat[tex * (64 * NC) + 64 * j + lane] = t;
            }
        }
    }
}

// part[chunk][j][ch]: j = 0, 1, 2 the weight columns, j = 3 the bias; the rows of a chunk in ascending order
__global__ __launch_bounds__(128) void lgo_lift_part_kernel(const float* __restrict__ gout, int ldo,
                                                            const float* __restrict__ rgb_s, int rows,
                                                            float* __restrict__ part) {
    const int ch = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * LGO_LIFT_ROWS;
    const int n = (int)min((long long)LGO_LIFT_ROWS, rows - r0);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int i = 0; i < n; ++i) {
        const float g = gout[(r0 + i) * ldo + 256 + ch];
        const float4 c = *reinterpret_cast<const float4*>(rgb_s + (r0 + i) * 4);
        s0 = s0 + g * c.x;
        s1 = s1 + g * c.y;
        s2 = s2 + g * c.z;
        s3 = s3 + g;
    }
    float* p = part + (long long)blockIdx.x * 512;
    p[ch] = s0;
    p[128 + ch] = s1;
    p[256 + ch] = s2;
    p[384 + ch] = s3;
}

// one wave per output q = j * 128 + ch: lane i adds partials i, i + 64, ... in ascending order, then the xor butterfly
__global__ __launch_bounds__(256) void lgo_lift_sum_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ g_w,
                                                           float* __restrict__ g_b) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);      // 0 .. 511
    float s = 0.f;
    for (int k = lane; k < nchunk; k += 64) s = s + part[(long long)k * 512 + q];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d, 64);
    if (lane == 0) {
        const int j = q >> 7, ch = q & 127;
        if (j < 3) g_w[ch * 3 + j] = s; else g_b[ch] = s;
    }
}

static int lgo_check(const int* dims, int V, int H, int W, int P, int ldo) {
    TH_REQUIRE(V >= 1 && H >= 1 && W >= 1 && P >= 0, "need V, H, W >= 1 and P >= 0");
    TH_REQUIRE((ldo & 3) == 0 && ldo >= 384, "row stride must be a multiple of 4, ldo >= 384");
    TH_REQUIRE((long long)H * W < (1ll << 31), "image too large");
    TH_REQUIRE((long long)V * H * W < (1ll << 31) - 1, "V * H * W must stay below 2^31 - 1 (the sort key)");
    TH_REQUIRE((long long)P * V < (1ll << 31) - LGO_TILE, "P * V too large");
    for (int l = 0; l < 3; ++l)
        TH_REQUIRE(dims[2 * l] >= 1 && dims[2 * l + 1] >= 1 && dims[2 * l] <= H && dims[2 * l + 1] <= W,
                   "latent dimensions must be within 1 .. the image's");
    return 0;
}

// waves per texel: a texel's list grows with the map pixels per texel (3 / scale rows by 3 / scale columns of them reach it),
// so the coarser levels split theirs.  A function of the dimensions alone: it is part of the order of summation
static int lgo_waves(int h, int w, int H, int W) {
    const long long area = (long long)H * W, tex = (long long)h * w;
    return area >= 32 * tex ? 4 : area >= 8 * tex ? 2 : 1;
}

template <int NC, int NW>
static int lgo_sum_launch_t(int h, int w, int V, int H, int W, const float* pts_world, int N, const float* cams,
                            const float* scale, const float* grad_out, int ldo, int col0, const unsigned* val, const int* start,
                            float* glat, hipStream_t s) {
    const int blocks = th_cdiv((long long)V * h * w, 4 / NW);
    hipLaunchKernelGGL((lgo_sum_kernel<NC, NW>), dim3(blocks), dim3(256), 0, s, h, w, V, H, W, pts_world, N, cams, scale, grad_out,
                       ldo, col0, val, start, glat);
    TH_LAUNCH_CHECK();
    return 0;
}

#define LGO_SUM_ARGS h, w, V, H, W, pts_world, N, cams, scale, grad_out, ldo, col0, val, start, glat, s
static int lgo_sum_launch(int nc, int nw, int h, int w, int V, int H, int W, const float* pts_world, int N, const float* cams,
                          const float* scale, const float* grad_out, int ldo, int col0, const unsigned* val, const int* start,
                          float* glat, hipStream_t s) {
    if (nc == 1) return nw == 4 ? lgo_sum_launch_t<1, 4>(LGO_SUM_ARGS) : nw == 2 ? lgo_sum_launch_t<1, 2>(LGO_SUM_ARGS)
                                                                                 : lgo_sum_launch_t<1, 1>(LGO_SUM_ARGS);
    return nw == 4 ? lgo_sum_launch_t<2, 4>(LGO_SUM_ARGS) : nw == 2 ? lgo_sum_launch_t<2, 2>(LGO_SUM_ARGS)
                                                                    : lgo_sum_launch_t<2, 1>(LGO_SUM_ARGS);
}
#undef LGO_SUM_ARGS

// the sort's two key / value buffers over the n (sample, view) pairs, its digit counts, the segment starts, the lift's partial sums
struct LgoWs { size_t n, ntile, nchunk, nb; unsigned *key[2], *val[2]; int *cnt, *start; float* part; };
static LgoWs lgo_layout(ThArena& ar, int V, int H, int W, int P) {
    const size_t n = (size_t)P * V, ntile = (n + LGO_TILE - 1) / LGO_TILE, nchunk = (n + LGO_LIFT_ROWS - 1) / LGO_LIFT_ROWS;
    const size_t nb = (size_t)V * H * W;
    return {n, ntile, nchunk, nb, {ar.take<unsigned>(n), ar.take<unsigned>(n)}, {ar.take<unsigned>(n), ar.take<unsigned>(n)},
            ar.take<int>(256 * ntile), ar.take<int>(nb + 1), ar.take<float>(nchunk * 512)};
}

size_t th_latgather_bwd_ord_ws(int V, int H, int W, int P) {
    return (V < 1 || H < 1 || W < 1 || P < 0) ? 0 : th_measure(lgo_layout, V, H, W, P);
}

int th_latgather_bwd_ord_launch(const int* dims, int V, int H, int W, const float* pts_world, int P, const float* cams,
                                const float* scale, const float* grad_out, int ldo, const float* rgb_s, float* g0, float* g1,
                                float* g2, float* g_w, float* g_b, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_TRY(lgo_check(dims, V, H, W, P, ldo));
    ThArena ar(ws, ws_bytes);
    const LgoWs pl = lgo_layout(ar, V, H, W, P);
    TH_REQUIRE(ar.ok(), "workspace too small (th_latent_gather_bwd_ordered_ws)");
    unsigned *const *key = pl.key, *const *val = pl.val;
    const int N = (int)pl.n, ntile = (int)pl.ntile, nb = (int)pl.nb;
    int cur = 0;
    if (N > 0) {
        hipLaunchKernelGGL(lgo_keys_kernel, dim3(th_cdiv(N, 256)), dim3(256), 0, s, V, H, W, pts_world, N, cams, scale, key[0],
                           val[0]);
        TH_LAUNCH_CHECK();
        int bits = 1;
        while (bits < 31 && ((long long)nb - 1) >> bits) ++bits;
        for (int shift = 0; shift < bits; shift += 8) {
            hipLaunchKernelGGL(lgo_hist_kernel, dim3(ntile), dim3(256), 0, s, key[cur], N, shift, ntile, pl.cnt);
            TH_LAUNCH_CHECK();
            hipLaunchKernelGGL(lgo_scan_kernel, dim3(1), dim3(1024), 0, s, pl.cnt, 256 * ntile);
            TH_LAUNCH_CHECK();
            hipLaunchKernelGGL(lgo_scatter_kernel, dim3(ntile), dim3(256), 0, s, key[cur], val[cur], N, shift, ntile, pl.cnt,
                               key[cur ^ 1], val[cur ^ 1]);
            TH_LAUNCH_CHECK();
            cur ^= 1;
        }
        hipLaunchKernelGGL(lgo_csr_kernel, dim3(th_cdiv((long long)nb + 1, 256)), dim3(256), 0, s, key[cur], N, nb, pl.start);
        TH_LAUNCH_CHECK();
    }
    float* gl[3] = {g0, g1, g2};
    for (int l = 0; l < 3; ++l) {
        const int h = dims[2 * l], w = dims[2 * l + 1];
        TH_TRY(lgo_sum_launch(l == 2 ? 2 : 1, lgo_waves(h, w, H, W), h, w, V, H, W, pts_world, N, cams, scale, grad_out, ldo,
                              l == 2 ? 128 : 64 * l, val[cur], pl.start, gl[l], s));
    }
    if (g_w) {
        if (N > 0) {
            hipLaunchKernelGGL(lgo_lift_part_kernel, dim3((int)pl.nchunk), dim3(128), 0, s, grad_out, ldo, rgb_s, N, pl.part);
            TH_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(lgo_lift_sum_kernel, dim3(128), dim3(256), 0, s, pl.part, (int)pl.nchunk, g_w, g_b);
        TH_LAUNCH_CHECK();
    }
    return 0;
}
