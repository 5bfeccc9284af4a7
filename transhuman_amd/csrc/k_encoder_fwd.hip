// K29: the forward convolutions of the encoder trunk in training (SpatialEncoder.trunk: conv1, layer1, layer2 of ResNet18,
// encoder.py:114-126): nn.Conv2d(cin, cout, ks, stride, ks // 2, bias=False) for 7x7/2 3->64, 3x3/1 64->64, 3x3/2 64->128, 1x1/2 64->128
// and 3x3/1 128->128.  NCHW fp32, contiguous, in and out.  Nothing in this file is launched by inference or by bench.py (the inference
// stem keeps the fp16-split th_conv2d of k_conv.hip).  The BatchNorm and the max pool of the training forward are th_bn_act (K11) and
// th_maxpool3x3s2 as they are.
//
// ef_conv_kernel<KS, S>   an implicit GEMM on the fp32-input MFMA (v_mfma_f32_32x32x2_f32): no reduced-precision operand, no range
//     guard, no atomics.  A workgroup of four waves owns an 8 x 16 tile of output pixels x 64 output channels of one image; a wave
//     owns two tile rows (32 pixels) x 64 channels as two 32 x 32 accumulators.  The weights are the MFMA's A operand and the pixels
//     its B operand, so a lane holds one pixel and the stores of a register are 32 consecutive pixels (two rows of 16) of one channel
//     plane.  Every output element of the image is stored exactly once and the output is never read: two runs agree bit for bit
//     whatever the buffer held before.
//
//     The reduction over (ci, kh, kw) is cut into chunks of th_conv2d_fwd32_chunk_channels = 8 input channels (conv1: its 3 channels
//     are one chunk).  Per chunk the workgroup stages in LDS
//       the input halo of the chunk's channels: 10 x 18 at 3x3/1, 17 x 33 at 3x3/2, 21 x 37 at 7x7/2, the strided 8 x 16 at 1x1/2;
//           rows and columns outside the image are written as zeros (the padding);
//       the chunk's weights, read directly from torch's layout [cout][cin][ks][ks] -- for a chunk the ks * ks * 8 floats of one row
//           `co` are contiguous --, transposed to [k][co]: no packed weight image, no cache per weight version, no workspace.
//     3x3 and 1x1: a chunk's ks * ks * 8 products are ONE fresh MFMA chain (accumulator cleared), in this order: taps kh outer, kw
//     inner; inside a tap the channel pairs (c, c + 1), c = 0, 2, 4, 6 of the chunk, one MFMA each (the instruction's two k slots).
//     7x7: the chunk's 147 products are SEVEN chains, one per kernel row kh, in this order: channels c = 0, 1, 2; inside a channel
//     the tap pairs (kw, kw + 1), kw = 0, 2, 4, 6, one MFMA each; the slot kw = 7 pads the row's 7 taps to an even count and is a
//     structural zero on BOTH operands (a literal 0, not a read).  A 21-long chain keeps conv1's rounding next to that of the other
//     shapes' 8..72-long chains; one 147-long fp32 chain was not tried.
//     The chains are added in chunk order (7x7: kh order) to fp64 registers and the sum is rounded to fp32 once at the store.
//     The order inside one MFMA (two products and the accumulator) is the instruction's.
//
// Resources (hipcc -O3, gfx950; DESIGN.md K29 holds the table): scratch 0 for all four instantiations.
#include "th_internal.h"

namespace {

typedef float ef_f32x16 __attribute__((ext_vector_type(16)));

constexpr int EF_THREADS = 256;
constexpr int EF_TW = 16, EF_TH = 8;     // output pixels per workgroup
constexpr int EF_CK = 8;                 // input channels per chunk (th_conv2d_fwd32_chunk_channels)
constexpr int EF_NB = 64;                // output channels per workgroup
constexpr int EF_WLD = EF_NB + 1;        // row pitch of the staged weights

template <int KS, int S>
struct EfGeom {
    static constexpr int P = KS / 2;
    static constexpr int KK = KS * KS;
    static constexpr int STEP = KS == 1 ? S : 1;              // input pixels between two staged positions (1x1/2 stages the strided grid)
    static constexpr int SL = S / STEP;                       // staged positions between two output pixels
    static constexpr int HH = (EF_TH - 1) * SL + KS, HW = (EF_TW - 1) * SL + KS;
    static constexpr int CK = KS == 7 ? 3 : EF_CK;            // channels per chunk
    static constexpr int ROWS = KK * CK;                      // staged weight rows per chunk
};

int ef_supported(int cin, int cout, int ks, int stride) {
    if (cin == 3 && cout == 64 && ks == 7 && stride == 2) return 1;
    if (cin == 64 && cout == 64 && ks == 3 && stride == 1) return 1;
    if (cin == 64 && cout == 128 && ks == 3 && stride == 2) return 1;
    if (cin == 64 && cout == 128 && ks == 1 && stride == 2) return 1;
    if (cin == 128 && cout == 128 && ks == 3 && stride == 1) return 1;
    return 0;
}
int ef_out(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }

// grid (tiles, COUT / 64, N)
template <int KS, int S>
__global__ __launch_bounds__(EF_THREADS) void ef_conv_kernel(const float* __restrict__ x, int CIN, int H, int W,
                                                             const float* __restrict__ w, int COUT, int Ho, int Wo,
                                                             float* __restrict__ y, int tiles_x) {
    using G = EfGeom<KS, S>;
    constexpr int PLANE = G::HH * G::HW;
    // (+ 1 element / + 1 row: the pad slot of the 7x7 form forms an address one past its tap row before the value is replaced by 0)
    __shared__ float sIn[G::CK * PLANE + 1];
    __shared__ float sW[(G::ROWS + 1) * EF_WLD];

    const int tid = threadIdx.x, lane = tid % TH_WAVE, wave = tid / TH_WAVE;
    const int blk = blockIdx.y, n = blockIdx.z;
    const int oy0 = (blockIdx.x / tiles_x) * EF_TH, ox0 = (blockIdx.x % tiles_x) * EF_TW;
    const int i_pix = lane & 31, hk = lane >> 5;
    const int py = 2 * wave + (i_pix >> 4), px = i_pix & 15;
    const int pbase = py * G::SL * G::HW + px * G::SL;       // the staged position of this pixel's tap (0, 0)
    const int nch = CIN / G::CK;

    double tot0[16], tot1[16];                               // the chains, added in chunk order
#pragma unroll
    for (int r = 0; r < 16; ++r) tot0[r] = tot1[r] = 0.0;

#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();
        // weights: row co of the chunk is G::ROWS contiguous floats at k = c * KK + t
        const float* wsrc = w + ((size_t)blk * EF_NB * CIN + (size_t)ch * G::CK) * G::KK;
        for (int i = tid; i < EF_NB * G::ROWS; i += EF_THREADS) {
            const int co = i / G::ROWS, k = i - co * G::ROWS;
            const int c = k / G::KK, t = k - c * G::KK;
            const int row = KS == 7 ? k : t * G::CK + c;
            sW[row * EF_WLD + co] = wsrc[(size_t)co * CIN * G::KK + k];
        }
        const float* src = x + ((size_t)n * CIN + (size_t)ch * G::CK) * H * W;
        for (int i = tid; i < G::CK * PLANE; i += EF_THREADS) {
            const int c = i / PLANE, rem = i - c * PLANE, r = rem / G::HW, col = rem - r * G::HW;
            const int iy = oy0 * S - G::P + r * G::STEP, ix = ox0 * S - G::P + col * G::STEP;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = src[((size_t)c * H + iy) * W + ix];
            sIn[i] = v;
        }
        __syncthreads();

        if constexpr (KS == 7) {
#pragma unroll 1
            for (int kh = 0; kh < KS; ++kh) {
                ef_f32x16 acc0, acc1;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
                const float* pin = sIn + pbase + kh * G::HW + hk;
                const float* pw = sW + (kh * KS + hk) * EF_WLD + i_pix;
#pragma unroll
                for (int c = 0; c < G::CK; ++c)
#pragma unroll
                    for (int q = 0; q < (KS + 1) / 2; ++q) {
                        const bool pad = 2 * q + 1 == KS && hk;          // the slot kw = 7
                        const float pv = pad ? 0.f : pin[c * PLANE + 2 * q];
                        const float w0 = pad ? 0.f : pw[(c * G::KK + 2 * q) * EF_WLD];
                        const float w1 = pad ? 0.f : pw[(c * G::KK + 2 * q) * EF_WLD + 32];
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, pv, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, pv, acc1, 0, 0, 0);
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot0[r] += (double)acc0[r];
                    tot1[r] += (double)acc1[r];
                }
            }
        } else {
            ef_f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
            const float* pin = sIn + pbase + hk * PLANE;
            const float* pw = sW + hk * EF_WLD + i_pix;
#pragma unroll
            for (int kh = 0; kh < KS; ++kh)
#pragma unroll
                for (int kw = 0; kw < KS; ++kw)
#pragma unroll
                    for (int q = 0; q < G::CK / 2; ++q) {
                        const float pv = pin[2 * q * PLANE + kh * G::HW + kw];
                        const float w0 = pw[((kh * KS + kw) * G::CK + 2 * q) * EF_WLD];
                        const float w1 = pw[((kh * KS + kw) * G::CK + 2 * q) * EF_WLD + 32];
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, pv, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, pv, acc1, 0, 0, 0);
                    }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tot0[r] += (double)acc0[r];
                tot1[r] += (double)acc1[r];
            }
        }
    }

    // C/D map of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy < Ho && ox < Wo) {
        float* dst = y + (((size_t)n * COUT + (size_t)blk * EF_NB) * Ho + oy) * Wo + ox;
        const size_t plane = (size_t)Ho * Wo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hk;
            dst[(size_t)row * plane] = (float)tot0[r];
            dst[(size_t)(row + 32) * plane] = (float)tot1[r];
        }
    }
}

template <int KS, int S>
void ef_launch(const float* x, int N, int cin, int H, int W, const float* w, int cout, float* y, hipStream_t s) {
    const int Ho = ef_out(H, KS, S), Wo = ef_out(W, KS, S);
    const int tiles_x = th_cdiv(Wo, EF_TW), tiles = tiles_x * th_cdiv(Ho, EF_TH);
    const dim3 grid((unsigned)tiles, (unsigned)(cout / EF_NB), (unsigned)N);
    hipLaunchKernelGGL((ef_conv_kernel<KS, S>), grid, dim3(EF_THREADS), 0, s, x, cin, H, W, w, cout, Ho, Wo, y, tiles_x);
}

}  // namespace

int th_conv2d_fwd32_supported_internal(int cin, int cout, int ks, int stride) { return ef_supported(cin, cout, ks, stride); }
void th_conv2d_fwd32_tile_internal(int* rows, int* cols) { *rows = EF_TH; *cols = EF_TW; }
int th_conv2d_fwd32_chunk_internal() { return EF_CK; }

int th_conv2d_fwd32_launch(const float* x, int N, int cin, int H, int W, const float* w, int cout, int ks, int stride, float* y,
                           hipStream_t s) {
    TH_REQUIRE(ef_supported(cin, cout, ks, stride),
               "unsupported shape: built for 7x7/2 3->64, 3x3/1 64->64, 3x3/2 64->128, 1x1/2 64->128 and 3x3/1 128->128");
    TH_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 16383, "unsupported shape: N in 1..16383, H, W >= 1");
    const long long in = (long long)N * cin * H * W, out = (long long)N * cout * ef_out(H, ks, stride) * ef_out(W, ks, stride);
    TH_REQUIRE(in < (1LL << 31) && out < (1LL << 31), "unsupported shape: 2^31 elements or more");
    if (ks == 7)
        ef_launch<7, 2>(x, N, cin, H, W, w, cout, y, s);
    else if (ks == 1)
        ef_launch<1, 2>(x, N, cin, H, W, w, cout, y, s);
    else if (stride == 2)
        ef_launch<3, 2>(x, N, cin, H, W, w, cout, y, s);
    else
        ef_launch<3, 1>(x, N, cin, H, W, w, cout, y, s);
    TH_LAUNCH_CHECK();
    return 0;
}
