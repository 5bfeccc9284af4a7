// K26: the targets the reference's dataset makes through sample_ray_h36m + get_acc -- both splits, on device.
//
// sample_ray_h36m (if_nerf_data_utils.py:516-614, called at can_smpl.py:518-535) restated for the dense per-pixel arrays that
// th_gen_rays (K9) writes; get_near_far is elementwise per ray, so a gathered subset of its dense result is what the reference
// computes on the subset.
//   m = msk * bound_mask in uint8 (:527); rand_set = (bound_mask == 1) & (m != 100) (:530); body = (m == 1), face = (m == 13)
//   test split (:600-612): the dense rows where the 3-D box test holds, in row-major order
//   train split (:532-598): while n < nrays: rem = nrays - n, n_body = int(rem body_ratio), n_face = int(rem face_ratio) (fp64
//     products, truncated), n_rand = rem - n_body - n_face; each class picks that many of its pixels (np.argwhere order) with
//     replacement; an empty body class gives the one coordinate (1,1), an empty rand_set the one coordinate (0,0), an empty face
//     class nothing; body, face, rand in that order; the coordinates whose ray hits the box are appended, n grows by their number
//     (so the final count can be nrays + 1).  Pick j of class c in iteration i is member min(floor(draws[i][c][j] n_c), n_c - 1).
//   get_acc (:635-641): 1 where any pixel of msk is nonzero in the 25 x 25 window centred on the coordinate, clipped to the image
//
// Nothing here computes: the stage selects and copies, so it equals its numpy restatement
// (transhuman_amd.train_targets.sample_rays_h36m_oracle) bit for bit; no atomic decides an order, and every element that is
// reported valid is stored (nothing relies on cleared memory).
//   rs_class_count_kernel  one lane per pixel: per-256-pixel-block counts of body / face / rand_set, and their wave64 ballots
//   rs_mask_count_kernel   the same for the box test alone (test split)
//   rs_scan_kernel         exclusive scan of the count rows (one workgroup per row), the totals behind them
//   rs_train_loop_kernel   ONE workgroup runs the whole loop: a lane per candidate finds its class member (binary search of the block
//                          prefixes, popcounts of the block's ballots, the r-th set bit of one word), tests K9's box mask and is
//                          appended in order through a workgroup prefix scan; the running count lives in LDS between iterations
//   rs_compact_kernel      test split: each pixel block writes its in-box rows behind the blocks before it (ballot rank)
//   rs_acc_kernel          one wave per coordinate: the window test
#include "th_internal.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / TH_WAVE)
#define RS_LOOP_THREADS 1024
#define RS_LOOP_WAVES (RS_LOOP_THREADS / TH_WAVE)
#define RS_MAX_DIM 4096
#define RS_MAX_RAYS 65536
#define RS_MAX_ITERS 4
#define RS_ACC_BORDER 25
// info[2] status bits
#define RS_ADDED_NOTHING 1
#define RS_UNFINISHED 2
#define RS_NEGATIVE_COUNT 4

__device__ __forceinline__ unsigned long long rs_below(int lane) { return (1ull << lane) - 1ull; }

// the per-block count of each of `rows` predicates (one wave ballot each) -> cnt[row][block]; bits[row][block][wave] if given
template <int ROWS>
__device__ __forceinline__ void rs_block_counts(const bool (&member)[ROWS], int nb, int32_t* __restrict__ cnt,
                                                unsigned long long* __restrict__ bits) {
    __shared__ int s[ROWS][RS_WAVES];
    const int lane = threadIdx.x & (TH_WAVE - 1), wave = threadIdx.x / TH_WAVE;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const unsigned long long b = __ballot(member[r]);
        if (lane == 0) {
            s[r][wave] = __popcll(b);
            if (bits) bits[((size_t)r * nb + blockIdx.x) * RS_WAVES + wave] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < ROWS) {
        int v = 0;
        for (int w = 0; w < RS_WAVES; ++w) v += s[threadIdx.x][w];
        cnt[(size_t)threadIdx.x * (nb + 1) + blockIdx.x] = v;
    }
}

// cnt: int32 [3][nb + 1], rows body / face / rand_set; bits: uint64 [3][nb][RS_WAVES]
__global__ __launch_bounds__(RS_THREADS) void rs_class_count_kernel(const uint8_t* __restrict__ msk, const uint8_t* __restrict__ bound,
                                                                    int npix, int nb, int32_t* __restrict__ cnt,
                                                                    unsigned long long* __restrict__ bits) {
    const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
    bool member[3] = {false, false, false};
    if (idx < npix) {
        const uint8_t b = bound[idx], m = (uint8_t)(msk[idx] * b);               // :527 (uint8 product)
        member[0] = m == 1;                                                      // :551
        member[1] = m == 13;                                                     // :560
        member[2] = b == 1 && m != 100;                                          // :530, :566
    }
    rs_block_counts<3>(member, nb, cnt, bits);
}

// cnt: int32 [nb + 1]
__global__ __launch_bounds__(RS_THREADS) void rs_mask_count_kernel(const uint8_t* __restrict__ ray_mask, int npix, int nb,
                                                                   int32_t* __restrict__ cnt) {
    const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
    const bool member[1] = {idx < npix && ray_mask[idx] != 0};
    rs_block_counts<1>(member, nb, cnt, nullptr);
}

// in place: row[b] becomes the number of set pixels in the blocks before b, row[nb] the total
__global__ __launch_bounds__(RS_THREADS) void rs_scan_kernel(int32_t* __restrict__ cnt, int nb) {
    __shared__ int s[RS_THREADS];
    int32_t* row = cnt + (size_t)blockIdx.x * (nb + 1);
    const int t = threadIdx.x, per = (nb + RS_THREADS - 1) / RS_THREADS;
    const int lo = min(t * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += row[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < RS_THREADS; off <<= 1) {
        const int v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int run = s[t] - sum;
    for (int i = lo; i < hi; ++i) {
        const int c = row[i];
        row[i] = run;
        run += c;
    }
    if (t == RS_THREADS - 1) row[nb] = s[t];
}

// the pixel index of member k (0 <= k < pre[nb]) of a class: its block is the last one with pre[b] <= k
__device__ __forceinline__ int rs_member_pixel(const int32_t* __restrict__ pre, const unsigned long long* __restrict__ bits, int nb,
                                               int k) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= k) lo = mid; else hi = mid - 1;
    }
    int r = k - pre[lo];
    const unsigned long long* words = bits + (size_t)lo * RS_WAVES;
    int w = 0;
    unsigned long long word = words[0];
    while (w < RS_WAVES - 1 && r >= __popcll(word)) {
        r -= __popcll(word);
        word = words[++w];
    }
    for (; r > 0; --r) word &= word - 1ull;                                      // drop the r lowest set bits
    return lo * RS_THREADS + w * TH_WAVE + (word ? __ffsll((long long)word) - 1 : 0);
}

__device__ __forceinline__ void rs_copy_ray(const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                            const float* __restrict__ near_in, const float* __restrict__ far_in,
                                            const float* __restrict__ img, long long pix_stride, long long chan_stride, long long pix,
                                            size_t dst, float* __restrict__ o_rgb, float* __restrict__ o_ray_o,
                                            float* __restrict__ o_ray_d, float* __restrict__ o_near, float* __restrict__ o_far) {
    const float* px = img + pix * pix_stride;
    o_rgb[3 * dst] = px[0];
    o_rgb[3 * dst + 1] = px[chan_stride];
    o_rgb[3 * dst + 2] = px[2 * chan_stride];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o_ray_o[3 * dst + a] = ray_o[3 * pix + a];
        o_ray_d[3 * dst + a] = ray_d[3 * pix + a];
    }
    o_near[dst] = near_in[pix];
    o_far[dst] = far_in[pix];
}

// info: int32 [4] = ray count, iterations used, status bits, the candidates of the last iteration
__global__ __launch_bounds__(RS_LOOP_THREADS) void rs_train_loop_kernel(
    const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float* __restrict__ near_in,
    const float* __restrict__ far_in, const uint8_t* __restrict__ ray_mask, const float* __restrict__ img, long long pix_stride,
    long long chan_stride, int W, const double* __restrict__ draws, int nrays, double body_ratio, double face_ratio, int nb,
    const int32_t* __restrict__ cnt, const unsigned long long* __restrict__ bits, int cap, float* __restrict__ o_rgb,
    float* __restrict__ o_ray_o, float* __restrict__ o_ray_d, float* __restrict__ o_near, float* __restrict__ o_far,
    int64_t* __restrict__ o_coord, int32_t* __restrict__ info) {
    __shared__ int s_cnt[RS_LOOP_WAVES];
    __shared__ int s_n;
    const int t = threadIdx.x, lane = t & (TH_WAVE - 1), wave = t / TH_WAVE;
    const int size[3] = {cnt[nb], cnt[(size_t)(nb + 1) + nb], cnt[2 * (size_t)(nb + 1) + nb]};
    if (t == 0) s_n = 0;
    __syncthreads();
    int iters = 0, status = 0, last = 0;
    while (true) {
        const int n = s_n;                                                       // (uniform: every lane reads the same LDS word)
        if (n >= nrays) break;                                                   // :545
        if (iters == RS_MAX_ITERS) { status |= RS_UNFINISHED; break; }
        const int rem = nrays - n;
        const int n_body = (int)((double)rem * body_ratio), n_face = (int)((double)rem * face_ratio);      // :546-547
        const int n_rand = rem - n_body - n_face;                                // :548
        if (n_body < 0 || n_face < 0 || n_rand < 0) { status |= RS_NEGATIVE_COUNT; break; }   // (np.random.randint raises)
        const int len0 = size[0] > 0 ? n_body : 1;                               // :553-557 (the fallback is ONE coordinate)
        const int len1 = size[1] > 0 ? n_face : 0;                               // :561-563, :572-575
        const int len2 = size[2] > 0 ? n_rand : 1;                               // :567-570
        const int total = len0 + len1 + len2;
        int run = n;
        for (int base = 0; base < total; base += RS_LOOP_THREADS) {
            const int j = base + t;
            int pix = 0;
            bool hit = false;
            if (j < total) {
                const int c = j < len0 ? 0 : (j < len0 + len1 ? 1 : 2);
                const int jj = j - (c == 0 ? 0 : (c == 1 ? len0 : len0 + len1));
                if (size[c] == 0) {
                    pix = c == 0 ? W + 1 : 0;                                    // (1,1) :557, (0,0) :570
                } else {
                    const double kf = floor(draws[((size_t)iters * 3 + c) * nrays + jj] * (double)size[c]);
                    const int k = kf >= 0.0 ? (kf < (double)size[c] ? (int)kf : size[c] - 1) : 0;   // (a NaN draw lands on 0)
                    pix = rs_member_pixel(cnt + (size_t)c * (nb + 1), bits + (size_t)c * nb * RS_WAVES, nb, k);
                }
                hit = ray_mask[pix] != 0;                                        // :581 (get_near_far's box test, K9's dense mask)
            }
            const unsigned long long bal = __ballot(hit);
            if (lane == 0) s_cnt[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, added = 0;
            for (int w = 0; w < RS_LOOP_WAVES; ++w) {
                if (w < wave) before += s_cnt[w];
                added += s_cnt[w];
            }
            const int dst = run + before + __popcll(bal & rs_below(lane));
            if (hit && dst < cap) {                                              // (dst <= nrays < cap by the loop's arithmetic)
                rs_copy_ray(ray_o, ray_d, near_in, far_in, img, pix_stride, chan_stride, pix, (size_t)dst, o_rgb, o_ray_o, o_ray_d,
                            o_near, o_far);
                o_coord[2 * (size_t)dst] = pix / W;                              // (row, col), :588
                o_coord[2 * (size_t)dst + 1] = pix % W;
            }
            run += added;
            __syncthreads();
        }
        ++iters;
        last = total;
        if (run == n) { status |= RS_ADDED_NOTHING; break; }                     // (the reference would never end)
        if (t == 0) s_n = run;
        __syncthreads();
    }
    if (t == 0) {
        info[0] = min(s_n, cap);
        info[1] = iters;
        info[2] = status;
        info[3] = last;
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_compact_kernel(
    const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float* __restrict__ near_in,
    const float* __restrict__ far_in, const uint8_t* __restrict__ ray_mask, const float* __restrict__ img, long long pix_stride,
    long long chan_stride, int npix, int nb, const int32_t* __restrict__ cnt, float* __restrict__ o_rgb, float* __restrict__ o_ray_o,
    float* __restrict__ o_ray_d, float* __restrict__ o_near, float* __restrict__ o_far, int32_t* __restrict__ info) {
    __shared__ int s_cnt[RS_WAVES];
    const int t = threadIdx.x, lane = t & (TH_WAVE - 1), wave = t / TH_WAVE;
    const int idx = blockIdx.x * RS_THREADS + t;
    const bool hit = idx < npix && ray_mask[idx] != 0;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    if (hit) {
        int before = __popcll(bal & rs_below(lane));
        for (int w = 0; w < wave; ++w) before += s_cnt[w];
        rs_copy_ray(ray_o, ray_d, near_in, far_in, img, pix_stride, chan_stride, idx, (size_t)cnt[blockIdx.x] + before, o_rgb,
                    o_ray_o, o_ray_d, o_near, o_far);
    }
    if (blockIdx.x == 0 && t == 0) {
        info[0] = cnt[nb];
        info[1] = 0;
        info[2] = 0;
        info[3] = 0;
    }
}

// one wave per coordinate (row, col): any nonzero pixel of msk in the window [row - 12, row + 12] x [col - 12, col + 12], clipped
__global__ __launch_bounds__(RS_THREADS) void rs_acc_kernel(const int64_t* __restrict__ coord, int n, const uint8_t* __restrict__ msk,
                                                            int H, int W, uint8_t* __restrict__ acc) {
    const int i = blockIdx.x * RS_WAVES + threadIdx.x / TH_WAVE, lane = threadIdx.x & (TH_WAVE - 1);
    if (i >= n) return;                                                          // (whole waves leave)
    const long long cy = coord[2 * (size_t)i], cx = coord[2 * (size_t)i + 1];
    const int half = RS_ACC_BORDER / 2;
    const long long y0 = max(cy - half, 0ll), y1 = min(cy + half, (long long)H - 1);
    const long long x0 = max(cx - half, 0ll), x1 = min(cx + half, (long long)W - 1);
    bool any = false;
    if (y0 <= y1 && x0 <= x1) {
        const int ww = (int)(x1 - x0 + 1), count = (int)(y1 - y0 + 1) * ww;
        for (int j = lane; j < count; j += TH_WAVE) any = any || msk[(y0 + j / ww) * W + x0 + j % ww] != 0;
    }
    const unsigned long long bal = __ballot(any);
    if (lane == 0) acc[i] = bal != 0ull ? 1 : 0;
}

static bool rs_sizes_ok(int H, int W) { return H >= 1 && W >= 1 && H <= RS_MAX_DIM && W <= RS_MAX_DIM; }

// three counters (and their scans) per block of pixels, and behind them the three classes' bit planes, one word per wave
struct RsWs { int32_t* cnt; unsigned long long* bits; };
static RsWs rs_layout(ThArena& ar, int H, int W) {
    const size_t nb = (size_t)th_cdiv((long long)H * W, RS_THREADS);
    return {ar.take<int32_t>(3 * (nb + 1)), ar.take<unsigned long long>(3 * nb * RS_WAVES)};
}
size_t th_ray_sample_ws(int H, int W, int nrays) {
    return (!rs_sizes_ok(H, W) || nrays < 0 || nrays > RS_MAX_RAYS) ? 0 : th_measure(rs_layout, H, W);
}

// the limits of the stage, checked before anything else
int th_ray_sample_check(int H, int W) {
    TH_REQUIRE(rs_sizes_ok(H, W), "image is " + std::to_string(H) + " x " + std::to_string(W) + ": 1 <= H, W <= 4096");
    return 0;
}

int th_ray_sample_train_check(int H, int W, int nrays, double body_ratio, double face_ratio) {
    TH_TRY(th_ray_sample_check(H, W));
    TH_REQUIRE(H >= 2 && W >= 2, "image is " + std::to_string(H) + " x " + std::to_string(W) +
                                     ": the train split needs H, W >= 2 (an empty body class samples pixel (1,1))");
    TH_REQUIRE(nrays >= 1 && nrays <= RS_MAX_RAYS, "nrays is " + std::to_string(nrays) + ": 1 <= nrays <= 65536");
    TH_REQUIRE(body_ratio >= 0.0 && face_ratio >= 0.0 && body_ratio + face_ratio <= 1.0,
               "body_ratio and face_ratio must be >= 0 and sum to at most 1");
    return 0;
}

int th_ray_sample_train_launch(const float* ray_o, const float* ray_d, const float* near_in, const float* far_in,
                               const uint8_t* ray_mask, const uint8_t* msk, const uint8_t* bound, const float* img,
                               long long pix_stride, long long chan_stride, int H, int W, const double* draws, int nrays,
                               double body_ratio, double face_ratio, float* o_rgb, float* o_ray_o, float* o_ray_d, float* o_near,
                               float* o_far, int64_t* o_coord, int32_t* info, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_TRY(th_ray_sample_train_check(H, W, nrays, body_ratio, face_ratio));
    TH_REQUIRE(pix_stride >= 1 && chan_stride >= 1, "image strides must be positive");
    ThArena ar(ws, ws_bytes);
    RsWs w = rs_layout(ar, H, W);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int npix = H * W, nb = th_cdiv(npix, RS_THREADS);
    hipLaunchKernelGGL(rs_class_count_kernel, dim3(nb), dim3(RS_THREADS), 0, s, msk, bound, npix, nb, w.cnt, w.bits);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_scan_kernel, dim3(3), dim3(RS_THREADS), 0, s, w.cnt, nb);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_train_loop_kernel, dim3(1), dim3(RS_LOOP_THREADS), 0, s, ray_o, ray_d, near_in, far_in, ray_mask, img,
                       pix_stride, chan_stride, W, draws, nrays, body_ratio, face_ratio, nb, w.cnt, w.bits, nrays + RS_MAX_ITERS, o_rgb,
                       o_ray_o, o_ray_d, o_near, o_far, o_coord, info);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_ray_sample_test_launch(const float* ray_o, const float* ray_d, const float* near_in, const float* far_in,
                              const uint8_t* ray_mask, const float* img, long long pix_stride, long long chan_stride, int H, int W,
                              float* o_rgb, float* o_ray_o, float* o_ray_d, float* o_near, float* o_far, int32_t* info, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    TH_TRY(th_ray_sample_check(H, W));
    TH_REQUIRE(pix_stride >= 1 && chan_stride >= 1, "image strides must be positive");
    ThArena ar(ws, ws_bytes);
    RsWs w = rs_layout(ar, H, W);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int npix = H * W, nb = th_cdiv(npix, RS_THREADS);
    hipLaunchKernelGGL(rs_mask_count_kernel, dim3(nb), dim3(RS_THREADS), 0, s, ray_mask, npix, nb, w.cnt);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(RS_THREADS), 0, s, w.cnt, nb);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_compact_kernel, dim3(nb), dim3(RS_THREADS), 0, s, ray_o, ray_d, near_in, far_in, ray_mask, img, pix_stride,
                       chan_stride, npix, nb, w.cnt, o_rgb, o_ray_o, o_ray_d, o_near, o_far, info);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_ray_acc_launch(const int64_t* coord, int n, const uint8_t* msk, int H, int W, uint8_t* acc, hipStream_t s) {
    TH_TRY(th_ray_sample_check(H, W));
    TH_REQUIRE(n >= 0 && n <= RS_MAX_DIM * RS_MAX_DIM, "n is " + std::to_string(n) + ": 0 <= n <= 4096 * 4096 coordinates");
    if (n == 0) return 0;
    hipLaunchKernelGGL(rs_acc_kernel, dim3(th_cdiv(n, RS_WAVES)), dim3(RS_THREADS), 0, s, coord, n, msk, H, W, acc);
    TH_LAUNCH_CHECK();
    return 0;
}
