// K19: the pixel-aligned gather of training read straight from the encoder's latents, and its adjoint.
//
// The dense pair K8 -> K5 upsamples the three ResNet latents to H x W (upsample_bilinear2d, align_corners=True), appends the
// colour lift and samples the 384-channel map bilinearly (grid_sample, align_corners=True, border).  Both steps are linear
// and per channel, so a sample of the map is a fixed linear combination of latent texels:
//   out[p,v, c0_l + c] = sum over the four map corners q = (Y, X) and the 2 x 2 upsample taps (ty, tx) of
//                        w_q(p,v) * ly_l(Y)[ty] * lx_l(X)[tx] * lat_l[v, ry_l(Y)[ty], rx_l(X)[tx], c]
// with (corners, w_q) from th_project + th_bilinear_setup and (ry, ly), (rx, lx) from ups_coord -- the rules of K5 and K8,
// restated nowhere.  Neither the [V,H,W,384] map nor its gradient exists.
// Tap bound: with h <= H the ups_coord scale is <= 1, so the source row of map row y0 + 1 is at most one above that of y0
// (fl(s (y0 + 1)) <= a + 2 for a = floor(fl(s y0)), with equality only when the product is the integer a + 2 itself, and then
// its second tap carries the weight l1 = 0): every tap with a non-zero weight lies in rows {a, a + 1, a + 2}, likewise for
// columns.  The 16 composite taps are merged into those 3 x 3 slots (lg_level below; a tap outside them has weight exactly 0
// and is dropped), in a fixed order, by the one device function both kernels call: the backward's coefficients are the
// forward's, bit for bit.  A 1 x 1 level has scale 0: all 16 taps fall into slot (0, 0).
// Columns 256..383 are the colour lift fmaf(b, w2, fmaf(g, w1, r w0)) + bias of each of the four image texels, blended with
// the grid weights in K5's statement order (pg_blend); rgb_s[p,v] = the blended raw (r, g, b, 0), which the lift's weight
// gradient needs.
//
// Grouping as pixgather_bwd_kernel: one wave per 16 consecutive samples of one view, lane i < 16 does sample i's set-up, the
// slot origin and the nine coefficients per level come back as wave-uniform scalars (v_readlane), lane = channel: every
// load, store and atomic of a wave is 256 contiguous bytes of one texel row / output row.
// Forward: all nine slot loads of a level are issued unconditionally (addresses clamped into the level, a zero coefficient
// multiplies a finite texel), so the 36 loads of a row are in flight together; the latents (69 MB at 512 x 512, V = 3)
// stay in L2 / MALL.
// Backward: clears the three latent gradients (hipMemsetAsync) and adds coef * g[p,v,c] with no-return global float atomics,
// skipping zero coefficients (scalar branch).  Float atomic sums depend on arrival order: the result is NOT bitwise
// reproducible from run to run (last-bit differences, like k_pixfeat_bwd.hip and torch's own grid_sample / upsample
// backwards); every element is within fp32 summation error of the exact adjoint.
#include "th_internal.h"
#include "k_latgather.h"

#define LG_G 16

template <int NC>   // NC = channels / 64 of the level
__device__ __forceinline__ void lg_fwd_level(const float* __restrict__ lat, int h, int w, int a, int b, const float (&cf)[9],
                                             int i, int lane, float* __restrict__ orow) {
    const int sa = __builtin_amdgcn_readlane(a, i), sb = __builtin_amdgcn_readlane(b, i);
    float x[9][NC];
    float c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        c[k] = lg_lane_f(cf[k], i);
        const float* t = lat + (long long)lg_slot_index(sa, sb, k, h, w) * (64 * NC);
#pragma unroll
        for (int j = 0; j < NC; ++j) x[k][j] = t[64 * j + lane];
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float acc = x[0][j] * c[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) acc = fmaf(x[k][j], c[k], acc);
        orow[64 * j + lane] = acc;
    }
}

__global__ __launch_bounds__(256) void latgather_kernel(const float* __restrict__ lat0, const float* __restrict__ lat1,
                                                        const float* __restrict__ lat2, LgLevels L,
                                                        const float* __restrict__ img, const float* __restrict__ wc,
                                                        const float* __restrict__ bc, int V, int H, int W,
                                                        const float* __restrict__ pts_world, int P,
                                                        const float* __restrict__ cams, const float* __restrict__ scale,
                                                        float* __restrict__ out, int ldo, float* __restrict__ rgb_s) {
    const int lane = threadIdx.x & 63;
    const long long grp = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long ngrp = (long long)((P + LG_G - 1) / LG_G) * V;
    if (grp >= ngrp) return;
    const int v = (int)(grp % V);
    const int p0 = (int)(grp / V) * LG_G;
    const int nrow = min(LG_G, P - p0);
    const Bilin bl = lg_setup(pts_world, p0 + min(lane, nrow - 1), cams + 21 * v, scale, H, W);
    int a0, b0, a1, b1, a2, b2;
    float cf0[9], cf1[9], cf2[9];
    lg_level(bl, L.h[0], L.w[0], H, W, a0, b0, cf0);
    lg_level(bl, L.h[1], L.w[1], H, W, a1, b1, cf1);
    lg_level(bl, L.h[2], L.w[2], H, W, a2, b2, cf2);
    // the four image texels of this lane's sample, and their blend
    const long long hw = (long long)H * W;
    const float* ip = img + (long long)v * 3 * hw;
    const int ci[4] = {bl.i00, bl.i01, bl.i10, bl.i11};
    float cr[4], cg[4], cb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { cr[q] = ip[ci[q]]; cg[q] = ip[hw + ci[q]]; cb[q] = ip[2 * hw + ci[q]]; }
    if (lane < nrow) {
        float4 s;
        s.x = fmaf(cr[3], bl.w11, fmaf(cr[2], bl.w10, fmaf(cr[1], bl.w01, cr[0] * bl.w00)));
        s.y = fmaf(cg[3], bl.w11, fmaf(cg[2], bl.w10, fmaf(cg[1], bl.w01, cg[0] * bl.w00)));
        s.z = fmaf(cb[3], bl.w11, fmaf(cb[2], bl.w10, fmaf(cb[1], bl.w01, cb[0] * bl.w00)));
        s.w = 0.f;
        *reinterpret_cast<float4*>(rgb_s + ((long long)(p0 + lane) * V + v) * 4) = s;
    }
    // this lane's two lift channels
    float lw[2][3], lb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ch = 64 * j + lane;
        lw[j][0] = wc[3 * ch]; lw[j][1] = wc[3 * ch + 1]; lw[j][2] = wc[3 * ch + 2];
        lb[j] = bc[ch];
    }
    const float* l0 = lat0 + (long long)v * L.h[0] * L.w[0] * 64;
    const float* l1 = lat1 + (long long)v * L.h[1] * L.w[1] * 64;
    const float* l2 = lat2 + (long long)v * L.h[2] * L.w[2] * 128;
    for (int i = 0; i < nrow; ++i) {
        float* orow = out + ((long long)(p0 + i) * V + v) * ldo;
        lg_fwd_level<1>(l0, L.h[0], L.w[0], a0, b0, cf0, i, lane, orow);
        lg_fwd_level<1>(l1, L.h[1], L.w[1], a1, b1, cf1, i, lane, orow + 64);
        lg_fwd_level<2>(l2, L.h[2], L.w[2], a2, b2, cf2, i, lane, orow + 128);
        const float w00 = lg_lane_f(bl.w00, i), w01 = lg_lane_f(bl.w01, i), w10 = lg_lane_f(bl.w10, i), w11 = lg_lane_f(bl.w11, i);
        float r[4], g[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { r[q] = lg_lane_f(cr[q], i); g[q] = lg_lane_f(cg[q], i); b[q] = lg_lane_f(cb[q], i); }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = fmaf(b[q], lw[j][2], fmaf(g[q], lw[j][1], r[q] * lw[j][0])) + lb[j];
            orow[256 + 64 * j + lane] = fmaf(t[3], w11, fmaf(t[2], w10, fmaf(t[1], w01, t[0] * w00)));
        }
    }
}

template <int NC>
__device__ __forceinline__ void lg_bwd_level(float* __restrict__ glat, int h, int w, int a, int b, const float (&cf)[9], int i,
                                             int lane, const float* __restrict__ grow) {
    const int sa = __builtin_amdgcn_readlane(a, i), sb = __builtin_amdgcn_readlane(b, i);
    float g[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) g[j] = grow[64 * j + lane];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float c = lg_lane_f(cf[k], i);
        if (c != 0.f) {
            float* t = glat + (long long)lg_slot_index(sa, sb, k, h, w) * (64 * NC);
#pragma unroll
            for (int j = 0; j < NC; ++j) atomicAdd(t + 64 * j + lane, c * g[j]);      // (result unused: no-return form)
        }
    }
}

__global__ __launch_bounds__(256) void latgather_bwd_kernel(LgLevels L, int V, int H, int W,
                                                            const float* __restrict__ pts_world, int P,
                                                            const float* __restrict__ cams, const float* __restrict__ scale,
                                                            const float* __restrict__ gout, int ldo, float* __restrict__ g0,
                                                            float* __restrict__ g1, float* __restrict__ g2) {
    const int lane = threadIdx.x & 63;
    const long long grp = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long ngrp = (long long)((P + LG_G - 1) / LG_G) * V;
    if (grp >= ngrp) return;
    const int v = (int)(grp % V);
    const int p0 = (int)(grp / V) * LG_G;
    const int nrow = min(LG_G, P - p0);
    const Bilin bl = lg_setup(pts_world, p0 + min(lane, nrow - 1), cams + 21 * v, scale, H, W);
    int a0, b0, a1, b1, a2, b2;
    float cf0[9], cf1[9], cf2[9];
    lg_level(bl, L.h[0], L.w[0], H, W, a0, b0, cf0);
    lg_level(bl, L.h[1], L.w[1], H, W, a1, b1, cf1);
    lg_level(bl, L.h[2], L.w[2], H, W, a2, b2, cf2);
    float* m0 = g0 + (long long)v * L.h[0] * L.w[0] * 64;
    float* m1 = g1 + (long long)v * L.h[1] * L.w[1] * 64;
    float* m2 = g2 + (long long)v * L.h[2] * L.w[2] * 128;
    for (int i = 0; i < nrow; ++i) {
        const float* grow = gout + ((long long)(p0 + i) * V + v) * ldo;
        lg_bwd_level<1>(m0, L.h[0], L.w[0], a0, b0, cf0, i, lane, grow);
        lg_bwd_level<1>(m1, L.h[1], L.w[1], a1, b1, cf1, i, lane, grow + 64);
        lg_bwd_level<2>(m2, L.h[2], L.w[2], a2, b2, cf2, i, lane, grow + 128);
    }
}

static int lg_check(const int* dims, int V, int H, int W, int P, int ldo) {
    TH_REQUIRE(V >= 1 && H >= 1 && W >= 1 && P >= 0, "need V, H, W >= 1 and P >= 0");
    TH_REQUIRE((ldo & 3) == 0 && ldo >= 384, "row stride must be a multiple of 4, ldo >= 384");
    TH_REQUIRE((long long)H * W < (1ll << 31), "image too large");
    for (int l = 0; l < 3; ++l)
        TH_REQUIRE(dims[2 * l] >= 1 && dims[2 * l + 1] >= 1 && dims[2 * l] <= H && dims[2 * l + 1] <= W,
                   "latent dimensions must be within 1 .. the image's");
    return 0;
}

int th_latgather_launch(const float* lat0, const float* lat1, const float* lat2, const int* dims, const float* img,
                        const float* wc, const float* bc, int V, int H, int W, const float* pts_world, int P, const float* cams,
                        const float* scale, float* out, int ldo, float* rgb_s, hipStream_t s) {
    TH_TRY(lg_check(dims, V, H, W, P, ldo));
    if (P == 0) return 0;
    LgLevels L{{dims[0], dims[2], dims[4]}, {dims[1], dims[3], dims[5]}};
    const long long groups = (long long)th_cdiv(P, LG_G) * V;
    hipLaunchKernelGGL(latgather_kernel, dim3(th_cdiv(groups, 4)), dim3(256), 0, s, lat0, lat1, lat2, L, img, wc, bc, V, H, W,
                       pts_world, P, cams, scale, out, ldo, rgb_s);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_latgather_bwd_launch(const int* dims, int V, int H, int W, const float* pts_world, int P, const float* cams,
                            const float* scale, const float* grad_out, int ldo, float* g0, float* g1, float* g2,
                            hipStream_t s) {
    TH_TRY(lg_check(dims, V, H, W, P, ldo));
    TH_HIP(hipMemsetAsync(g0, 0, (size_t)V * dims[0] * dims[1] * 64 * sizeof(float), s));
    TH_HIP(hipMemsetAsync(g1, 0, (size_t)V * dims[2] * dims[3] * 64 * sizeof(float), s));
    TH_HIP(hipMemsetAsync(g2, 0, (size_t)V * dims[4] * dims[5] * 128 * sizeof(float), s));
    if (P == 0) return 0;
    LgLevels L{{dims[0], dims[2], dims[4]}, {dims[1], dims[3], dims[5]}};
    const long long groups = (long long)th_cdiv(P, LG_G) * V;
    hipLaunchKernelGGL(latgather_bwd_kernel, dim3(th_cdiv(groups, 4)), dim3(256), 0, s, L, V, H, W, pts_world, P, cams, scale,
                       grad_out, ldo, g0, g1, g2);
    TH_LAUNCH_CHECK();
    return 0;
}
