// Image metrics of the evaluator (lib/evaluators/if_nerf.py:108, :121-144): SSIM as skimage 0.19's
// structural_similarity(img_pred, img_gt, multichannel=True) computes it on the evaluator's float64 crops:
//   per channel, a 7 x 7 uniform window (win_size 7, no Gaussian weights), sample covariance (cov_norm = 49 / 48),
//   data_range 2 (the float64 dtype range [-1, 1]): C1 = (0.01 * 2)^2, C2 = (0.03 * 2)^2,
//   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
//   channel value = mean of S over the pixels whose window lies inside the image (skimage's crop(S, 3): its
//   reflect padding never reaches the mean), result = mean over the channels.
// The inputs are fp32 (the reference's images are float32 values held in float64 arrays); every operation here is
// fp64 on them, so the kernel sees the reference's numbers.
//
// ssim_tile_kernel: one workgroup per (16 x 32 output tile, channel).  The tile's 22 x 38 input pixels of both images are
// staged in LDS as fp32; 7-wide row sums of the five products (a, b, a a, b b, a b) over the 22 rows go to LDS in fp64, then
// each thread takes the 7-tall column sums of two outputs, forms S and adds the valid ones.  The workgroup's sum of S is
// written to partial[channel][tile] -- no atomics.  ssim_finish_kernel (one workgroup) adds the partials of each channel in
// a fixed order: the result is bit-identical from run to run.
#include "th_internal.h"

namespace {

constexpr int SS_WIN = 7;
constexpr int SS_TW = 32;                        // output tile: columns
constexpr int SS_TH = 16;                        //              rows
constexpr int SS_IW = SS_TW + SS_WIN - 1;        // staged input: 38 columns
constexpr int SS_IH = SS_TH + SS_WIN - 1;        //               22 rows
constexpr int SS_THREADS = 256;
constexpr int SS_FIN_THREADS = 256;

// fixed-order workgroup sum of one double per thread (every thread gets the result)
template <int NT>
__device__ double block_sum(double v, double* red) {
    for (int o = TH_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, TH_WAVE);
    const int lane = threadIdx.x % TH_WAVE, wave = threadIdx.x / TH_WAVE;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NT / TH_WAVE; ++w) s += red[w];
    __syncthreads();                             // red[] may be reused by the caller
    return s;
}

__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               int H, int W, int C, long long pitch, int tiles_x,
                                                               double* __restrict__ partial) {
    __shared__ float sa[SS_IH][SS_IW], sb[SS_IH][SS_IW];
    __shared__ double rs[5][SS_IH][SS_TW];       // row sums of a, b, a a, b b, a b
    __shared__ double red[SS_THREADS / TH_WAVE];

    const int tile = blockIdx.x, ch = blockIdx.y;
    const int Ho = H - (SS_WIN - 1), Wo = W - (SS_WIN - 1);   // outputs whose window lies inside the image
    const int oy0 = (tile / tiles_x) * SS_TH, ox0 = (tile % tiles_x) * SS_TW;
    // output (oy, ox) of the valid region is image pixel (oy + 3, ox + 3); its window starts at image (oy, ox)
    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += SS_THREADS) {
        const int r = i / SS_IW, cx = i % SS_IW;
        const int y = oy0 + r, x = ox0 + cx;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            const long long off = (long long)y * pitch + (long long)x * C + ch;
            va = a[off];
            vb = b[off];
        }
        sa[r][cx] = va;
        sb[r][cx] = vb;
    }
    __syncthreads();

    for (int i = threadIdx.x; i < SS_IH * SS_TW; i += SS_THREADS) {
        const int r = i / SS_TW, cx = i % SS_TW;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int k = 0; k < SS_WIN; ++k) {
            const double x = (double)sa[r][cx + k], y = (double)sb[r][cx + k];
            s0 += x;
            s1 += y;
            s2 += x * x;
            s3 += y * y;
            s4 += x * y;
        }
        rs[0][r][cx] = s0;
        rs[1][r][cx] = s1;
        rs[2][r][cx] = s2;
        rs[3][r][cx] = s3;
        rs[4][r][cx] = s4;
    }
    __syncthreads();

    const double inv_np = 1.0 / (SS_WIN * SS_WIN);
    const double cov_norm = (double)(SS_WIN * SS_WIN) / (SS_WIN * SS_WIN - 1);
    const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
    double acc = 0.0;
    for (int i = threadIdx.x; i < SS_TH * SS_TW; i += SS_THREADS) {
        const int r = i / SS_TW, cx = i % SS_TW;
        if (oy0 + r >= Ho || ox0 + cx >= Wo) continue;
        double t[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SS_WIN; ++k) s += rs[q][r + k][cx];
            t[q] = s * inv_np;
        }
        const double ux = t[0], uy = t[1];
        const double vx = cov_norm * (t[2] - ux * ux);
        const double vy = cov_norm * (t[3] - uy * uy);
        const double vxy = cov_norm * (t[4] - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        acc += (A1 * A2) / (B1 * B2);
    }
    const double s = block_sum<SS_THREADS>(acc, red);
    if (threadIdx.x == 0) partial[(long long)ch * gridDim.x + tile] = s;
}

// out[0] = mean over the channels of (sum of the channel's partials) / (Ho * Wo)
__global__ __launch_bounds__(SS_FIN_THREADS) void ssim_finish_kernel(const double* __restrict__ partial, int n_tiles, int C,
                                                                     double count, double* __restrict__ out) {
    __shared__ double red[SS_FIN_THREADS / TH_WAVE];
    double total = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        double v = 0.0;
        for (int i = threadIdx.x; i < n_tiles; i += SS_FIN_THREADS) v += partial[(long long)ch * n_tiles + i];
        total += block_sum<SS_FIN_THREADS>(v, red) / count;
    }
    if (threadIdx.x == 0) out[0] = total / C;
}

int ssim_tiles(int h, int w) {
    const int tx = th_cdiv(w - (SS_WIN - 1), SS_TW), ty = th_cdiv(h - (SS_WIN - 1), SS_TH);
    return tx * ty;
}

}  // namespace

// every tile's partial sum per channel
static double* ssim_layout(ThArena& ar, int h, int w, int c) { return ar.take<double>((size_t)ssim_tiles(h, w) * c); }
size_t th_ssim_ws(int h, int w, int c) { return (h < SS_WIN || w < SS_WIN || c < 1) ? 0 : th_measure(ssim_layout, h, w, c); }

int th_ssim_launch(const float* a, const float* b, int h, int w, int c, long long pitch, double* out, void* ws,
                   size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(h >= SS_WIN && w >= SS_WIN, "image smaller than the 7 x 7 window");
    TH_REQUIRE(c >= 1 && pitch >= (long long)w * c, "bad channel count or row pitch");
    ThArena ar(ws, ws_bytes);
    double* partial = ssim_layout(ar, h, w, c);
    TH_REQUIRE(ar.ok(), "workspace too small");
    TH_REQUIRE(c <= 65535, "too many channels");
    const int tiles_x = th_cdiv(w - (SS_WIN - 1), SS_TW), n_tiles = ssim_tiles(h, w);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)n_tiles, (unsigned)c), dim3(SS_THREADS), 0, s, a, b, h, w, c, pitch,
                       tiles_x, partial);
    TH_LAUNCH_CHECK();
    const double count = (double)(h - (SS_WIN - 1)) * (double)(w - (SS_WIN - 1));
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(SS_FIN_THREADS), 0, s, partial, n_tiles, c, count, out);
    TH_LAUNCH_CHECK();
    return 0;
}
