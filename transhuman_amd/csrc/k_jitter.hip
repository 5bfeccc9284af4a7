// K25: colour jitter of the raw uint8 camera frames, in front of K16 (what the reference's dataset does per item on the host through
// torchvision's ColorJitter on PIL images, lib/datasets/light_stage/can_smpl.py:629-637, for the target view and every input view
// before they are undistorted).  torchvision is absent wherever this project builds or runs: the order of operations follows its
// documented ColorJitter and parity with torchvision is UNPINNED; the image arithmetic is Pillow's (ImageEnhance.Brightness /
// Contrast / Color = ImageChops blend against black / the mean grey / the pixel's grey; convert("HSV") / convert("RGB")), which
// tests/test_jitter_host.py holds the numpy restatement (transhuman_amd/preprocess.py::color_jitter_oracle) to byte for byte and
// tests/test_gpu_jitter.py holds this file to, on the whole 2^24 colour cube for the hue.
//
// Definition (normative), per uint8 pixel:
//   grey        L = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   blend       blend(d, x, f) = d + f (x - d) in fp32: x - d in integers, the product and the sum rounded one by one; 0 <= f <= 1:
//               truncated; otherwise 0 where <= 0, 255 where >= 255, else truncated
//   brightness  blend(0, x, f) per channel;  saturation  blend(L, x, f) per channel with L of that pixel
//   contrast    blend(m, x, f), m = (2 sum L + n) / (2 n) in integers over the n pixels of THAT image as it stands at that step
//   hue         RGB -> HSV, H <- (H + d) & 255, HSV -> RGB (lossy for d = 0 too, which is part of the result).
//               RGB -> HSV: V = max; max == min: H = S = 0; else fp32 c = max - min, s = c / max, rc, gc, bc = (max - R) / c, ...;
//               h = bc - gc | 2.0 + rc - bc | 4.0 + gc - rc (R | G | B is the maximum, tested in that order) in double, rounded to
//               fp32; h <- fp32(fmod(double(h) / 6.0 + 1.0, 1.0)); H = clip(int(double(h) 255.0)), S = clip(int(double(s) 255.0)).
//               HSV -> RGB: S == 0: R = G = B = V; else in double x = H 6.0 / 255.0, i = floor(x), f = x - i, fs = S / 255.0,
//               p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f))), half away from zero, clipped;
//               (R, G, B) by i mod 6: (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q).
//   Every product, quotient, sum and difference is ONE correctly rounded IEEE operation: nothing here may be contracted into a
//   fused multiply-add (1 - fs f would change q on part of the cube).
//
// Kernels.  jitter_kernel<REDUCE>: grid (G, V), 256 lanes.  A view starts at byte 3 v H W: pixel-aligned, not 16-byte-aligned in
// general.  Its first `head` pixels (< 16: up to the first pixel that starts on a 16-byte boundary) and its last (n - head) % 16
// go one pixel per lane through byte loads and stores; between them one lane takes 16 pixels = 48 bytes as three 128-bit loads and
// three 128-bit stores, workgroups striding over the chunks.  The four pixels of 12 bytes are taken from the low words of the
// 12-word register window, which is then rotated by three words: every index is a constant (no scratch) and the chain is
// instantiated for four pixels, not sixteen.  If img and out differ in their alignment mod 16 every pixel takes the narrow path.
// With contrast enabled there are two launches: REDUCE = true applies the operations that precede contrast, sums L per lane
// (uint32: <= 64 chunks of 16 pixels), per wave (__shfl_xor), per workgroup (four LDS words) and STORES one uint64 into slot
// [v][workgroup] of the caller's workspace; REDUCE = false has every workgroup add the G slots of its view (G <= 1024: four loads
// per lane), derive m and run the whole chain.  No atomics, nothing cleared, every slot that is read was written by the launch
// before: correct whatever the workspace held, and integer sums do not depend on their order (bit-identical run to run).
#include "th_internal.h"

namespace {

constexpr int JT_THREADS = 256, JT_MAX_G = 1024, JT_MAX_DIM = 16384;

struct JtParams {
    float brightness, contrast, saturation;
    int hue_shift;        // d, 0..255
    unsigned int order;   // the operation of step k at bits 2 k, 2 k + 1
    int enabled;          // bit op
    int steps;            // how many steps of the chain to run
};

__device__ __forceinline__ int jt_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ int jt_blend(int d, int x, float f) {
#pragma clang fp contract(off)
    const float t = __fadd_rn((float)d, __fmul_rn(f, (float)(x - d)));
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int jt_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int jt_round8(double v) { return jt_clip8((int)round(v)); }

__device__ __forceinline__ void jt_hue(int& r, int& g, int& b, int shift) {
#pragma clang fp contract(off)
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float c = (float)(mx - mn);
        const float s = __fdiv_rn(c, (float)mx);
        const float rc = __fdiv_rn((float)(mx - r), c), gc = __fdiv_rn((float)(mx - g), c), bc = __fdiv_rn((float)(mx - b), c);
        const double hd = r == mx ? __dsub_rn((double)bc, (double)gc)
                                  : (g == mx ? __dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc)
                                             : __dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc));
        float h = (float)hd;
        const double x = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);             // in [5/6, 11/6]
        h = (float)(x >= 1.0 ? __dsub_rn(x, 1.0) : x);                         // fmod(x, 1.0), exact
        H = jt_clip8((int)__dmul_rn((double)h, 255.0));
        S = jt_clip8((int)__dmul_rn((double)s, 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double x = __ddiv_rn(__dmul_rn((double)H, 6.0), 255.0);
    const double fi = floor(x);
    const double f = __dsub_rn(x, fi), fs = __ddiv_rn((double)S, 255.0), v = (double)V;
    const int p = jt_round8(__dmul_rn(v, __dsub_rn(1.0, fs)));
    const int q = jt_round8(__dmul_rn(v, __dsub_rn(1.0, __dmul_rn(fs, f))));
    const int t = jt_round8(__dmul_rn(v, __dsub_rn(1.0, __dmul_rn(fs, __dsub_rn(1.0, f)))));
    switch ((int)fi % 6) {
        case 0: r = V, g = t, b = p; break;
        case 1: r = q, g = V, b = p; break;
        case 2: r = p, g = V, b = t; break;
        case 3: r = p, g = q, b = V; break;
        case 4: r = t, g = p, b = V; break;
        default: r = V, g = p, b = q; break;
    }
}

// the first P.steps steps of the chain on one pixel; `mean` is read by the contrast step only
__device__ __forceinline__ void jt_chain(const JtParams& P, int mean, int& r, int& g, int& b) {
    for (int k = 0; k < P.steps; ++k) {
        const int op = (int)((P.order >> (2 * k)) & 3u);
        if (!((P.enabled >> op) & 1)) continue;
        if (op == 3) {
            jt_hue(r, g, b, P.hue_shift);
        } else {
            const float f = op == 0 ? P.brightness : (op == 1 ? P.contrast : P.saturation);
            const int L = jt_grey(r, g, b);
            const int d = op == 0 ? 0 : (op == 1 ? mean : L);
            r = jt_blend(d, r, f), g = jt_blend(d, g, f), b = jt_blend(d, b, f);
        }
    }
}

// the sum of `x` over the workgroup, in every lane (one use per kernel: `part` is not reused)
__device__ __forceinline__ unsigned long long jt_block_sum(unsigned long long x, unsigned long long* part) {
#pragma unroll
    for (int o = TH_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, TH_WAVE);
    if ((threadIdx.x & (TH_WAVE - 1)) == 0) part[threadIdx.x / TH_WAVE] = x;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < JT_THREADS / TH_WAVE; ++w) s += part[w];
    return s;
}

template <bool REDUCE>
__global__ __launch_bounds__(JT_THREADS) void jitter_kernel(const uint8_t* img, uint8_t* out, long long n,
                                                            JtParams P, int wide, unsigned long long* __restrict__ ws) {
    __shared__ unsigned long long s_part[JT_THREADS / TH_WAVE];
    const int view = blockIdx.y, G = gridDim.x;
    const int t = threadIdx.x;
    int mean = 0;
    if (!REDUCE && ws) {                                                      // (uniform over the launch)
        unsigned long long s = 0;
        for (int k = t; k < G; k += JT_THREADS) s += ws[(size_t)view * G + k];
        s = jt_block_sum(s, s_part);
        mean = (int)((2 * s + (unsigned long long)n) / (2 * (unsigned long long)n));
    }
    const uint8_t* src = img + (size_t)view * (size_t)n * 3;
    uint8_t* dst = REDUCE ? nullptr : out + (size_t)view * (size_t)n * 3;
    // head: the pixels before the first one that starts on a 16-byte boundary (3 * 11 = 33 = 1 mod 16)
    const long long head = wide ? (long long)((((16 - (int)((uintptr_t)src & 15)) & 15) * 11) & 15) : n;
    const long long first = head < n ? head : n;
    const long long chunks = (n - first) >> 4, tail0 = first + (chunks << 4);
    const long long lane = (long long)blockIdx.x * JT_THREADS + t, stride = (long long)G * JT_THREADS;
    unsigned int sum = 0;

    // narrow path: [0, first) and [tail0, n), one pixel per lane
    for (long long k = lane; k < first + (n - tail0); k += stride) {
        const size_t px = (size_t)(k < first ? k : tail0 + (k - first));
        int r = src[3 * px], g = src[3 * px + 1], b = src[3 * px + 2];
        jt_chain(P, mean, r, g, b);
        if (REDUCE) {
            sum += (unsigned int)jt_grey(r, g, b);
        } else {
            dst[3 * px] = (uint8_t)r, dst[3 * px + 1] = (uint8_t)g, dst[3 * px + 2] = (uint8_t)b;
        }
    }
    // wide path: 16 pixels = three 128-bit words per lane
    for (long long c = lane; c < chunks; c += stride) {
        const size_t at = (size_t)first * 3 + (size_t)c * 48;                 // 16-byte aligned: (src + 3 head) is, and 48 = 3 * 16
        const uint4* in4 = reinterpret_cast<const uint4*>(src + at);
        const uint4 a0 = in4[0], a1 = in4[1], a2 = in4[2];
        unsigned int w[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll 1
        for (int grp = 0; grp < 4; ++grp) {
            unsigned int o[3] = {0u, 0u, 0u};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int ch[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) ch[k] = (int)((w[(3 * p + k) >> 2] >> (8 * ((3 * p + k) & 3))) & 255u);
                jt_chain(P, mean, ch[0], ch[1], ch[2]);
                if (REDUCE) sum += (unsigned int)jt_grey(ch[0], ch[1], ch[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) o[(3 * p + k) >> 2] |= (unsigned int)ch[k] << (8 * ((3 * p + k) & 3));
            }
            // rotate the window by three words: the next four pixels come to the front, the finished ones go to the back
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = w[k + 3];
            w[9] = o[0], w[10] = o[1], w[11] = o[2];
        }
        if (!REDUCE) {
            uint4* out4 = reinterpret_cast<uint4*>(dst + at);
            out4[0] = make_uint4(w[0], w[1], w[2], w[3]);
            out4[1] = make_uint4(w[4], w[5], w[6], w[7]);
            out4[2] = make_uint4(w[8], w[9], w[10], w[11]);
        }
    }
    if (REDUCE) {
        const unsigned long long s = jt_block_sum(sum, s_part);
        if (t == 0) ws[(size_t)view * G + blockIdx.x] = s;
    }
}

bool jt_size_ok(int V, int H, int W) { return V >= 1 && V <= 65535 && H >= 1 && W >= 1 && H <= JT_MAX_DIM && W <= JT_MAX_DIM; }

// workgroups per view: one chunk per lane up to JT_MAX_G workgroups, then the lanes stride (16384 x 16384: 64 chunks per lane)
int jt_groups(long long n) {
    const long long g = ((n >> 4) + JT_THREADS - 1) / JT_THREADS;
    return (int)(g < 1 ? 1 : (g > JT_MAX_G ? JT_MAX_G : g));
}

}  // namespace

// one slot per (image, pixel group): the group's grey sum for the contrast step
static unsigned long long* jt_layout(ThArena& ar, int V, int H, int W) {
    return ar.take<unsigned long long>((size_t)V * jt_groups((long long)H * W));
}
size_t th_color_jitter_ws(int V, int H, int W) { return jt_size_ok(V, H, W) ? th_measure(jt_layout, V, H, W) : 0; }

int th_color_jitter_launch(const uint8_t* img, int V, int H, int W, uint32_t order, float brightness, float contrast,
                           float saturation, int hue_shift, uint32_t enabled, uint8_t* out, void* ws, size_t ws_bytes,
                           hipStream_t s) {
    TH_REQUIRE(jt_size_ok(V, H, W), "bad image count or size (1 <= V <= 65535; 1 <= H, W <= 16384)");
    TH_REQUIRE(order < 256u && enabled < 16u, "order is four 2-bit operation numbers, enabled a 4-bit mask");
    JtParams P = {};
    int seen = 0, contrast_at = 4;
    for (int k = 0; k < 4; ++k) {
        const int op = (int)((order >> (2 * k)) & 3u);
        seen |= 1 << op;
        if (op == 1) contrast_at = k;
    }
    TH_REQUIRE(seen == 15, "order is not a permutation of the operations 0..3");
    TH_REQUIRE(hue_shift >= 0 && hue_shift <= 255, "hue_shift must be 0..255");
    const float f[3] = {brightness, contrast, saturation};
    for (int k = 0; k < 3; ++k) {
        TH_REQUIRE(!((enabled >> k) & 1u) || (f[k] >= 0.0f && f[k] <= 3.0e38f), "an enabled factor must be finite and >= 0");
    }
    P.brightness = brightness, P.contrast = contrast, P.saturation = saturation;
    P.order = order;
    P.hue_shift = hue_shift;
    P.enabled = (int)enabled;
    const long long n = (long long)H * W;
    const size_t total = (size_t)V * (size_t)n * 3;
    TH_REQUIRE(out == img || out + total <= img || img + total <= out, "out must be img itself or not overlap it");
    const int G = jt_groups(n);
    const int wide = (((uintptr_t)img ^ (uintptr_t)out) & 15) == 0 ? 1 : 0;
    const bool two = (enabled >> 1) & 1u;
    unsigned long long* slots = nullptr;
    if (two) {
        ThArena ar(ws, ws_bytes);
        slots = jt_layout(ar, V, H, W);
        TH_REQUIRE(ws && ar.ok(), "workspace missing or smaller than th_color_jitter_workspace_bytes");
        TH_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
        P.steps = contrast_at;
        hipLaunchKernelGGL(jitter_kernel<true>, dim3(G, V), dim3(JT_THREADS), 0, s, img, (uint8_t*)nullptr, n, P, wide, slots);
        TH_LAUNCH_CHECK();
    }
    P.steps = 4;
    hipLaunchKernelGGL(jitter_kernel<false>, dim3(G, V), dim3(JT_THREADS), 0, s, img, out, n, P, wide, slots);
    TH_LAUNCH_CHECK();
    return 0;
}
