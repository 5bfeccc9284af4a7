// K16: the input views of a frame, prepared from the raw camera pictures: lens undistortion, area resize, background masking, and
// the union / border marking of the raw masks (what the reference's dataset does on the host with OpenCV for every view of every
// frame, lib/datasets/light_stage/can_smpl.py:118-200 get_mask / get_input_mask and :629-660 process_loaded).  OpenCV is absent
// wherever this project builds or runs, so no picture of cv2's own exists to compare with: the image is DEFINED BY THIS PROJECT,
// written after OpenCV's documented algorithm (initUndistortRectifyMap + remap INTER_LINEAR with 5 fractional bits, resize
// INTER_AREA by an integer factor / INTER_NEAREST, erode / dilate with a square kernel), and bit parity with cv2 is UNPINNED: its
// SIMD paths may fuse the four-tap sum and its 15-bit integer weight table has a saturation fix-up that is not reproduced
// (DESIGN.md 4 K16).
//
// Definition (normative; transhuman_amd/preprocess.py::prepare_views_oracle / combine_masks_oracle restate it in numpy).  Every
// step is ONE correctly rounded IEEE operation in the order written, without contraction: the device equals the restatement bit
// for bit.
//   map         float64 on the exactly promoted fp32 K, D = (k1, k2, p1, p2, k3), for source pixel (col j, row i):
//               x = (j - cx) / fx, y = (i - cy) / fy, x2 = x x, y2 = y y, r2 = x2 + y2, t = (2 x) y,
//               kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = (x kr + p1 t) + p2 (r2 + 2 x2), yd = (y kr + p1 (r2 + 2 y2)) + p2 t,
//               u = fx xd + cx, v = fy yd + cy, iu = rint(32 u), iv = rint(32 v) (half to even); a coordinate with
//               |32 u| >= 2^30 or not finite is taken as iu = -2^20 (every tap outside).  X = iu >> 5, a = iu & 31 (likewise Y, b).
//   weights     of the taps (X, Y), (X+1, Y), (X, Y+1), (X+1, Y+1): W00 = (32-b)(32-a), W01 = (32-b) a, W10 = b (32-a), W11 = b a
//               (sum 1024); a tap outside the image is the constant 0.
//   picture     per channel in fp32: s = lut[u8] (= float(u8) / 255.0f, filled by the caller), w = float(W) / 1024 (exact),
//               o = ((s00 w00 + s01 w01) + s10 w10) + s11 w11.
//   mask        m' = (W00 m00 + W01 m01 + W10 m10 + W11 m11 + 512) >> 10 in integers (any uint8 value, 100 included).
//   resize      picture: the n x n block summed in fp32 in row-major order from 0, times float(1 / (n n)); mask: m'[n y, n x].
//   background  with mask_bkgd, a pixel whose resized mask is 0 becomes `background` on all three channels.
//   raw masks   m = (a != 0) | (b != 0); with border > 0 (odd, <= 15): ero / dil = min / max of m over the border x border window,
//               over the pixels of it that lie inside the image; m = 100 where dil - ero == 1.
//
// Kernels
//   prep_views_kernel<n>   one lane per OUTPUT pixel and view; a workgroup is a 32 x 8 output tile, so one wave covers 32 x 2
//                          outputs = a 32 n x 2 n patch of the source, whose 4 n^2 taps per lane land on the same 96 n-byte row
//                          segments of the uint8 picture as its neighbours' (for a mild distortion the taps of consecutive lanes
//                          are 3 n bytes apart: every byte of a fetched line is used by the wave that fetched it).  The float64
//                          map (~40 operations, two divisions) is evaluated once per source pixel for the three channels and the
//                          mask; the three NCHW planes and the mask are written directly, consecutive lanes on consecutive floats;
//                          no full-resolution float intermediate exists.  The 256-entry table sits in LDS.
//   prep_mask_kernel       one lane per pixel, same tile.  The union of the tile and its halo is staged once in LDS as 2-bit codes
//                          and the border x border window is taken separably (OR along the rows, then along the columns): per
//                          pixel ~2 bytes read from memory and ~3 border LDS reads instead of 2 border^2 reads through the cache
//                          (V = 3 at 1024 x 1024, border 5: 66 us that way).
#include "th_internal.h"

namespace {

constexpr int PV_TX = 32, PV_TY = 8, PV_THREADS = PV_TX * PV_TY;
constexpr int PV_MAX_DIM = 16384;
constexpr double PV_Q_MAX = 1073741824.0;      // 2^30
constexpr int PV_Q_OUT = -(1 << 20);

struct PvCam {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ int pv_quant(double u) {
#pragma clang fp contract(off)
    const double q = 32.0 * u;
    return fabs(q) < PV_Q_MAX ? (int)rint(q) : PV_Q_OUT;      // (NaN compares false)
}

// 32 x the source coordinates that source pixel (col j, row i) of the undistorted picture reads
__device__ __forceinline__ void pv_map(const PvCam& c, int j, int i, int& iu, int& iv) {
#pragma clang fp contract(off)
    const double x = ((double)j - c.cx) / c.fx, y = ((double)i - c.cy) / c.fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, t = (2.0 * x) * y;
    const double kr = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xd = (x * kr + c.p1 * t) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * t;
    iu = pv_quant(c.fx * xd + c.cx);
    iv = pv_quant(c.fy * yd + c.cy);
}

template <int N>
__global__ __launch_bounds__(PV_THREADS) void prep_views_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ msk,
                                                                int H0, int W0, const float* __restrict__ K,
                                                                const float* __restrict__ D, int mask_bkgd, float background,
                                                                const float* __restrict__ lut, float* __restrict__ out_img,
                                                                uint8_t* __restrict__ out_msk) {
#pragma clang fp contract(off)
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int H = H0 / N, W = W0 / N;
    const int ox = blockIdx.x * PV_TX + (threadIdx.x & (PV_TX - 1)), oy = blockIdx.y * PV_TY + threadIdx.x / PV_TX;
    if (ox >= W || oy >= H) return;
    const int view = blockIdx.z;
    const float* k = K + 9 * view;
    const float* d = D + 5 * view;
    const PvCam cam = {(double)k[0], (double)k[4], (double)k[2], (double)k[5], (double)d[0], (double)d[1], (double)d[2], (double)d[3],
                       (double)d[4]};
    const size_t plane0 = (size_t)view * H0 * W0;
    const uint8_t* pic = img + 3 * plane0;
    const uint8_t* mk = msk + plane0;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int m_out = 0;
    constexpr int UNROLL_ROWS = N <= 2 ? N : 1;                  // (n = 4 unrolled 16 times takes 250 registers)
#pragma unroll UNROLL_ROWS
    for (int dy = 0; dy < N; ++dy) {
#pragma unroll
        for (int dx = 0; dx < N; ++dx) {
            int iu, iv;
            pv_map(cam, ox * N + dx, oy * N + dy, iu, iv);
            const int X = iu >> 5, Y = iv >> 5, a = iu & 31, b = iv & 31;
            const int wi[4] = {(32 - b) * (32 - a), (32 - b) * a, b * (32 - a), b * a};
            const bool in_x[2] = {(unsigned)X < (unsigned)W0, (unsigned)(X + 1) < (unsigned)W0};
            const bool in_y[2] = {(unsigned)Y < (unsigned)H0, (unsigned)(Y + 1) < (unsigned)H0};
            float o[3] = {0.0f, 0.0f, 0.0f};
            int msum = 512;
#pragma unroll
            for (int tap = 0; tap < 4; ++tap) {
                const int ty = tap >> 1, tx = tap & 1;
                const bool inside = in_x[tx] && in_y[ty];
                const size_t at = inside ? (size_t)(Y + ty) * W0 + (size_t)(X + tx) : 0;       // (never dereferenced outside)
                const float w = (float)wi[tap] * 0.0009765625f;                                // / 1024, exact
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float s = inside ? s_lut[pic[3 * at + ch]] : 0.0f;
                    const float p = s * w;
                    o[ch] = tap == 0 ? p : o[ch] + p;
                }
                if (dy == 0 && dx == 0) msum += wi[tap] * (inside ? (int)mk[at] : 0);
            }
            if (dy == 0 && dx == 0) m_out = msum >> 10;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + o[ch];
        }
    }
    const float scale = 1.0f / (float)(N * N);                                                 // 1, 1/4, 1/16: exact
    const size_t hw = (size_t)H * W, px = (size_t)oy * W + ox;
    const bool blank = mask_bkgd && m_out == 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out_img[((size_t)view * 3 + ch) * hw + px] = blank ? background : acc[ch] * scale;
    out_msk[(size_t)view * hw + px] = (uint8_t)m_out;
}

// prep_mask_kernel's three phases for lane t of the workgroup whose tile starts at (x0, y0); r = border / 2.  A pixel's code is 1
// where the union is set, 2 where it is clear and 0 outside the image, so the OR over a window is 3 exactly where the window's
// pixels inside the image hold both: dil - ero == 1.
constexpr int PM_R = 7, PM_COLS = PV_TX + 2 * PM_R, PM_ROWS = PV_TY + 2 * PM_R;

// codes of the tile and its halo of r pixels
__device__ __forceinline__ void pm_load(int t, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H0, int W0, int x0,
                                        int y0, int r, uint8_t (*code)[PM_COLS]) {
    const int cols = PV_TX + 2 * r, rows = PV_TY + 2 * r;
    for (int k = t; k < rows * cols; k += PV_THREADS) {
        const int row = k / cols, col = k - row * cols;
        const int y = y0 - r + row, x = x0 - r + col;
        uint8_t c = 0;
        if ((unsigned)y < (unsigned)H0 && (unsigned)x < (unsigned)W0) {
            const size_t q = (size_t)y * W0 + x;
            c = (a[q] != 0) || (b && b[q] != 0) ? 1 : 2;
        }
        code[row][col] = c;
    }
}

// OR over the `border` columns around every column of the tile, for every row of tile and halo
__device__ __forceinline__ void pm_rows(int t, int r, const uint8_t (*code)[PM_COLS], uint8_t (*orow)[PV_TX]) {
    const int rows = PV_TY + 2 * r;
    for (int k = t; k < rows * PV_TX; k += PV_THREADS) {
        const int row = k / PV_TX, col = k & (PV_TX - 1);
        int c = 0;
        for (int d = 0; d <= 2 * r; ++d) c |= code[row][col + d];
        orow[row][col] = (uint8_t)c;
    }
}

// OR over the `border` rows, and the pixel
__device__ __forceinline__ void pm_out(int t, int H0, int W0, int x0, int y0, int r, const uint8_t (*code)[PM_COLS],
                                       const uint8_t (*orow)[PV_TX], uint8_t* __restrict__ out) {
    const int col = t & (PV_TX - 1), row = t / PV_TX;
    const int x = x0 + col, y = y0 + row;
    if (x >= W0 || y >= H0) return;
    int c = 0;
    for (int d = 0; d <= 2 * r; ++d) c |= orow[row + d][col];
    out[(size_t)y * W0 + x] = c == 3 ? 100 : (code[row + r][col + r] == 1 ? 1 : 0);
}

__global__ __launch_bounds__(PV_THREADS) void prep_mask_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H0,
                                                               int W0, int border, uint8_t* __restrict__ out) {
    __shared__ uint8_t s_code[PM_ROWS][PM_COLS];
    __shared__ uint8_t s_orow[PM_ROWS][PV_TX];
    const size_t plane = (size_t)blockIdx.z * H0 * W0;
    const int x0 = blockIdx.x * PV_TX, y0 = blockIdx.y * PV_TY, r = border >> 1, t = threadIdx.x;
    pm_load(t, a + plane, b ? b + plane : nullptr, H0, W0, x0, y0, r, s_code);
    __syncthreads();
    pm_rows(t, r, s_code, s_orow);
    __syncthreads();
    pm_out(t, H0, W0, x0, y0, r, s_code, s_orow, out + plane);
}

bool pv_size_ok(int V, int H0, int W0) { return V >= 1 && V <= 65535 && H0 >= 1 && W0 >= 1 && H0 <= PV_MAX_DIM && W0 <= PV_MAX_DIM; }

}  // namespace

int th_prep_views_launch(const uint8_t* img, const uint8_t* msk, int V, int H0, int W0, const float* K, const float* D, int n,
                         int mask_bkgd, int white_bkgd, const float* lut, float* out_img, uint8_t* out_msk, hipStream_t s) {
    TH_REQUIRE(pv_size_ok(V, H0, W0), "bad view count or image size (1 <= V <= 65535; 1 <= H0, W0 <= 16384)");
    TH_REQUIRE(n == 1 || n == 2 || n == 4, "n = 1 / ratio must be 1, 2 or 4");
    TH_REQUIRE(H0 % n == 0 && W0 % n == 0, "image size not divisible by n = 1 / ratio");
    const dim3 grid(th_cdiv(W0 / n, PV_TX), th_cdiv(H0 / n, PV_TY), V), block(PV_THREADS);
    const float bg = white_bkgd ? 1.0f : 0.0f;
    const int mb = mask_bkgd ? 1 : 0;
    if (n == 1) hipLaunchKernelGGL(prep_views_kernel<1>, grid, block, 0, s, img, msk, H0, W0, K, D, mb, bg, lut, out_img, out_msk);
    else if (n == 2) hipLaunchKernelGGL(prep_views_kernel<2>, grid, block, 0, s, img, msk, H0, W0, K, D, mb, bg, lut, out_img, out_msk);
    else hipLaunchKernelGGL(prep_views_kernel<4>, grid, block, 0, s, img, msk, H0, W0, K, D, mb, bg, lut, out_img, out_msk);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_prep_mask_launch(const uint8_t* a, const uint8_t* b, int V, int H0, int W0, int border, uint8_t* out, hipStream_t s) {
    TH_REQUIRE(pv_size_ok(V, H0, W0), "bad view count or image size (1 <= V <= 65535; 1 <= H0, W0 <= 16384)");
    TH_REQUIRE(border == 0 || (border > 0 && border <= 15 && (border & 1)), "border must be 0 or an odd value up to 15");
    hipLaunchKernelGGL(prep_mask_kernel, dim3(th_cdiv(W0, PV_TX), th_cdiv(H0, PV_TY), V), dim3(PV_THREADS), 0, s, a, b, H0, W0,
                       border, out);
    TH_LAUNCH_CHECK();
    return 0;
}
