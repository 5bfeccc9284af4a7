// K18: the training targets of one step -- patch ray sampling on device.
//
// The train split of sample_ray_patch (if_nerf_data_utils.py:445-499, called at can_smpl.py:507-516) with its helpers
// get_patch_ray_indices / _get_patch_ray_indices / sample_patch_rays (:287-443), restated for the dense per-pixel arrays that
// th_gen_rays (K9) writes.  The reference does this per step in numpy inside the DataLoader:
//   m = msk * bound_mask in uint8 (:455); human = m > 0 (:461, the border value 100 included); ray_mask = the 3-D box test of
//   get_near_far (:470); background = ray_mask & ~human (:368-371, bbox_mask is ray_mask reshaped, :482);
//   per patch: the candidate set is human if the first draw < sample_subject_ratio, else background (:383-386); the centre is
//   the k-th set pixel in np.where order (:299-304), k being np.random.choice's pick; the window is clipped into the image
//   (:307-315); its ray_mask pixels in row-major order are the patch's rays (:328-330), select_inds = cumsum(ray_mask) - 1 there
//   (:336-337); patch_masks = ray_mask, patch_masks_sub = human on the window (:329-344), target_patches = the image on the
//   window (:433-438); rgb / ray_o / ray_d / near / far / sub_mask are gathered at the rays (:347-353, :429-431), the patches
//   concatenated in order (:402), patch_div_indices the running total (:379-400).
// The two random numbers of a patch come in as draws[i] = (u0, u1) in [0, 1): set = u0 < subject_ratio, k = min(floor(u1 n), n-1)
// with the product in float64.
//
// Nothing here computes: the stage selects and copies, so it equals its numpy restatement
// (transhuman_amd.train_targets.sample_patch_rays_oracle) bit for bit, and no atomic decides an order.
//   patch_count_kernel    one lane per pixel: the per-256-pixel-block counts of ray_mask, human and background (wave64 ballots),
//                         and the ray_mask ballots themselves (one 64-bit word per wave) for select_inds
//   patch_scan_kernel     exclusive scan of the three count rows (one workgroup per row), the totals behind them
//   patch_window_kernel   one workgroup per patch: binary search of the block prefixes for the block of the k-th set pixel,
//                         ballot / popcount rank inside it; then the window's masks, target patch and ray count
//   patch_gather_kernel   one workgroup per patch: its offset is the sum of the earlier patches' counts; the window's rays are
//                         ranked by ballot / popcount and written to their final rows
// Bound: 3 B read per pixel in the first pass; everything after it touches N P^2 pixels.
#include "th_internal.h"

#define PT_THREADS 256
#define PT_WAVES (PT_THREADS / TH_WAVE)
#define PT_MAX_P 64
#define PT_MAX_N 64
#define PT_MAX_DIM 4096

__device__ __forceinline__ bool pt_human(const uint8_t* __restrict__ msk, const uint8_t* __restrict__ bound, long long p) {
    return (uint8_t)(msk[p] * bound[p]) > 0;                                  // :455 (uint8 product), :461
}

__device__ __forceinline__ unsigned long long pt_below(int lane) { return (1ull << lane) - 1ull; }

// cnt: int32 [3][nb + 1], rows ray_mask / human / background; bits: uint64 [nb][PT_WAVES]
__global__ __launch_bounds__(PT_THREADS) void patch_count_kernel(const uint8_t* __restrict__ ray_mask, const uint8_t* __restrict__ msk,
                                                                 const uint8_t* __restrict__ bound, int npix, int nb,
                                                                 int32_t* __restrict__ cnt, unsigned long long* __restrict__ bits) {
    __shared__ int s[3][PT_WAVES];
    const int idx = blockIdx.x * PT_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (TH_WAVE - 1), wave = threadIdx.x / TH_WAVE;
    const bool in = idx < npix;
    const bool rm = in && ray_mask[idx] != 0;
    const bool hu = in && pt_human(msk, bound, idx);
    const bool bg = rm && !hu;
    const unsigned long long b_rm = __ballot(rm), b_hu = __ballot(hu), b_bg = __ballot(bg);
    if (lane == 0) {
        bits[(size_t)blockIdx.x * PT_WAVES + wave] = b_rm;
        s[0][wave] = __popcll(b_rm);
        s[1][wave] = __popcll(b_hu);
        s[2][wave] = __popcll(b_bg);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int v = 0;
        for (int w = 0; w < PT_WAVES; ++w) v += s[threadIdx.x][w];
        cnt[(size_t)threadIdx.x * (nb + 1) + blockIdx.x] = v;
    }
}

// in place: row[b] becomes the number of set pixels in the blocks before b, row[nb] the total
__global__ __launch_bounds__(PT_THREADS) void patch_scan_kernel(int32_t* __restrict__ cnt, int nb) {
    __shared__ int s[PT_THREADS];
    int32_t* row = cnt + (size_t)blockIdx.x * (nb + 1);
    const int t = threadIdx.x, per = (nb + PT_THREADS - 1) / PT_THREADS;
    const int lo = min(t * per, nb), hi = min(lo + per, nb);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += row[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < PT_THREADS; off <<= 1) {
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
    if (t == PT_THREADS - 1) row[nb] = s[t];
}

// counts: int32 [2][N] = the candidate set's size n, the window's ray count; xy_min int32 [N][2]
__global__ __launch_bounds__(PT_THREADS) void patch_window_kernel(
    const uint8_t* __restrict__ ray_mask, const uint8_t* __restrict__ msk, const uint8_t* __restrict__ bound,
    const float* __restrict__ img, long long pix_stride, long long chan_stride, int H, int W, const double* __restrict__ draws,
    double subject_ratio, int N, int P, int nb, const int32_t* __restrict__ cnt, uint8_t* __restrict__ patch_masks,
    uint8_t* __restrict__ patch_masks_sub, float* __restrict__ target_patches, int32_t* __restrict__ xy_min,
    int32_t* __restrict__ counts) {
    __shared__ int s_cnt[PT_WAVES];
    __shared__ int s_centre;
    const int i = blockIdx.x, t = threadIdx.x, lane = t & (TH_WAVE - 1), wave = t / TH_WAVE;
    const int npix = H * W;
    const bool subject = draws[2 * i] < subject_ratio;                           // :383
    const int32_t* pre = cnt + (size_t)(subject ? 1 : 2) * (nb + 1);
    const int n = pre[nb];
    if (n == 0) {                                                                // (np.random.choice(0) raises, :302)
        if (t == 0) { counts[i] = 0; counts[N + i] = 0; }
        return;
    }
    const double kf = floor(draws[2 * i + 1] * (double)n);
    const int k = kf >= 0.0 ? (kf < (double)n ? (int)kf : n - 1) : 0;            // (a NaN draw lands on 0)
    // the block that holds the k-th set pixel: the last one with pre[b] <= k
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= k) lo = mid; else hi = mid - 1;
    }
    const int r = k - pre[lo];
    const int idx = lo * PT_THREADS + t;
    bool member = false;
    if (idx < npix) {
        const bool hu = pt_human(msk, bound, idx);
        member = subject ? hu : (ray_mask[idx] != 0 && !hu);
    }
    const unsigned long long bal = __ballot(member);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    if (t == 0) s_centre = 0;
    __syncthreads();
    int before = __popcll(bal & pt_below(lane));
    for (int w = 0; w < wave; ++w) before += s_cnt[w];
    if (member && before == r) s_centre = idx;                                   // np.where order is row-major (:299)
    __syncthreads();
    const int cx = s_centre % W, cy = s_centre / W;
    const int x_min = min(max(cx - P / 2, 0), W - P), y_min = min(max(cy - P / 2, 0), H - P);      // :307-315
    const int PP = P * P;
    int rays = 0;
    for (int base = 0; base < PP; base += PT_THREADS) {
        const int j = base + t;
        bool rm = false;
        if (j < PP) {
            const int wy = j / P, wx = j - wy * P;
            const long long pix = (long long)(y_min + wy) * W + (x_min + wx);
            rm = ray_mask[pix] != 0;
            const size_t o = (size_t)i * PP + j;
            patch_masks[o] = rm ? 1 : 0;                                         // :329, :343
            patch_masks_sub[o] = pt_human(msk, bound, pix) ? 1 : 0;              // :332, :344
            const float* px = img + pix * pix_stride;
            target_patches[3 * o] = px[0];                                       // :437
            target_patches[3 * o + 1] = px[chan_stride];
            target_patches[3 * o + 2] = px[2 * chan_stride];
        }
        rays += __popcll(__ballot(rm));
    }
    if (lane == 0) s_cnt[wave] = rays;
    __syncthreads();
    if (t == 0) {
        int total = 0;
        for (int w = 0; w < PT_WAVES; ++w) total += s_cnt[w];
        counts[i] = n;
        counts[N + i] = total;
        xy_min[2 * i] = x_min;
        xy_min[2 * i + 1] = y_min;
    }
}

__global__ __launch_bounds__(PT_THREADS) void patch_gather_kernel(
    const float* __restrict__ ray_o, const float* __restrict__ ray_d, const float* __restrict__ near_in,
    const float* __restrict__ far_in, const float* __restrict__ img, long long pix_stride, long long chan_stride, int W, int N,
    int P, int nb, const int32_t* __restrict__ cnt, const unsigned long long* __restrict__ bits,
    const uint8_t* __restrict__ patch_masks, const uint8_t* __restrict__ patch_masks_sub, const int32_t* __restrict__ xy_min,
    const int32_t* __restrict__ counts, float* __restrict__ o_rgb, float* __restrict__ o_ray_o, float* __restrict__ o_ray_d,
    float* __restrict__ o_near, float* __restrict__ o_far, uint8_t* __restrict__ o_sub, int64_t* __restrict__ o_inds) {
    __shared__ int s_cnt[PT_WAVES];
    const int i = blockIdx.x, t = threadIdx.x, lane = t & (TH_WAVE - 1), wave = t / TH_WAVE;
    if (counts[i] == 0 || counts[N + i] == 0) return;
    int run = 0;                                                                 // patch_div_indices[i] (:379-400)
    for (int j = 0; j < i; ++j) run += counts[N + j];
    const int x_min = xy_min[2 * i], y_min = xy_min[2 * i + 1], PP = P * P;
    for (int base = 0; base < PP; base += PT_THREADS) {
        const int j = base + t;
        const size_t o = (size_t)i * PP + j;
        const bool rm = j < PP && patch_masks[o] != 0;
        const unsigned long long bal = __ballot(rm);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < PT_WAVES; ++w) {
            if (w < wave) before += s_cnt[w];
            total += s_cnt[w];
        }
        if (rm) {
            const size_t dst = (size_t)run + before + __popcll(bal & pt_below(lane));
            const int wy = j / P, wx = j - wy * P;
            const long long pix = (long long)(y_min + wy) * W + (x_min + wx);
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
            o_sub[dst] = patch_masks_sub[o];                                     // :431, :468
            // cumsum(ray_mask) - 1 at a set pixel (:336-337): the set pixels in front of it
            const long long blk = pix / PT_THREADS;
            const int pw = (int)(pix % PT_THREADS) / TH_WAVE, pl = (int)(pix % TH_WAVE);
            long long ind = cnt[blk] + __popcll(bits[blk * PT_WAVES + pw] & pt_below(pl));
            for (int w = 0; w < pw; ++w) ind += __popcll(bits[blk * PT_WAVES + w]);
            o_inds[dst] = ind;
        }
        run += total;
        __syncthreads();
    }
}

static bool pt_sizes_ok(int H, int W) { return H >= 1 && W >= 1 && H <= PT_MAX_DIM && W <= PT_MAX_DIM; }

// three counters (and their scans) per block of pixels, and behind them the blocks' bit planes, one word per wave
struct PtWs { int32_t* cnt; unsigned long long* bits; };
static PtWs pt_layout(ThArena& ar, int H, int W) {
    const size_t nb = (size_t)th_cdiv((long long)H * W, PT_THREADS);
    return {ar.take<int32_t>(3 * (nb + 1)), ar.take<unsigned long long>(nb * PT_WAVES)};
}
size_t th_patch_ws(int H, int W) { return pt_sizes_ok(H, W) ? th_measure(pt_layout, H, W) : 0; }

// the limits of the stage, checked before anything else (th_patch_rays reports them ahead of a null pointer)
int th_patch_check(int H, int W, int N, int P) {
    TH_REQUIRE(pt_sizes_ok(H, W), "image is " + std::to_string(H) + " x " + std::to_string(W) + ": 1 <= H, W <= 4096");
    TH_REQUIRE(P >= 1 && P <= PT_MAX_P && P <= H && P <= W,
               "patch size is " + std::to_string(P) + ": 1 <= P <= 64 and P <= min(H, W)");
    TH_REQUIRE(N >= 1 && N <= PT_MAX_N, "N is " + std::to_string(N) + ": 1 <= N <= 64 patches");
    return 0;
}

int th_patch_rays_launch(const float* ray_o, const float* ray_d, const float* near_in, const float* far_in, const uint8_t* ray_mask,
                         const uint8_t* msk, const uint8_t* bound, const float* img, long long pix_stride, long long chan_stride,
                         int H, int W, const double* draws, double subject_ratio, int N, int P, uint8_t* patch_masks,
                         uint8_t* patch_masks_sub, float* target_patches, int32_t* xy_min, int32_t* counts, float* o_rgb,
                         float* o_ray_o, float* o_ray_d, float* o_near, float* o_far, uint8_t* o_sub, int64_t* o_inds, void* ws,
                         size_t ws_bytes, hipStream_t s) {
    TH_TRY(th_patch_check(H, W, N, P));
    TH_REQUIRE(pix_stride >= 1 && chan_stride >= 1, "image strides must be positive");
    ThArena ar(ws, ws_bytes);
    PtWs w = pt_layout(ar, H, W);
    TH_REQUIRE(ar.ok(), "workspace too small");
    const int npix = H * W, nb = th_cdiv(npix, PT_THREADS);
    hipLaunchKernelGGL(patch_count_kernel, dim3(nb), dim3(PT_THREADS), 0, s, ray_mask, msk, bound, npix, nb, w.cnt, w.bits);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(patch_scan_kernel, dim3(3), dim3(PT_THREADS), 0, s, w.cnt, nb);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(patch_window_kernel, dim3(N), dim3(PT_THREADS), 0, s, ray_mask, msk, bound, img, pix_stride, chan_stride, H,
                       W, draws, subject_ratio, N, P, nb, w.cnt, patch_masks, patch_masks_sub, target_patches, xy_min, counts);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(patch_gather_kernel, dim3(N), dim3(PT_THREADS), 0, s, ray_o, ray_d, near_in, far_in, img, pix_stride,
                       chan_stride, W, N, P, nb, w.cnt, w.bits, patch_masks, patch_masks_sub, xy_min, counts, o_rgb, o_ray_o, o_ray_d,
                       o_near, o_far, o_sub, o_inds);
    TH_LAUNCH_CHECK();
    return 0;
}
