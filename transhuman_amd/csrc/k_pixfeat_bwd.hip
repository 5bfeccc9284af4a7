// K5 backward: the adjoint of the pixel-aligned gather of k_pixfeat.hip with respect to the channels-last map.
//
// Forward (per sample p, view v):  out[p,v,:C] = sum over the four corners q of  w_q(p,v) * map[v, texel_q(p,v), :C]
// (th_project + th_bilinear_setup of th_internal.h: projection, border clamp, grid_sample's weights).  Its adjoint is
//   grad_map[v, t, :] = sum over (p, q) with texel_q(p,v) = t of  w_q(p,v) * grad_out[p,v,:C].
// The destinations are H W V rows of 4 C bytes (1 536 at C = 384) and the contributions spread over many of them, the case
// in which global float atomics run at their full chip-wide rate: the kernel clears the map and adds with no-return
// global_atomic_add_f32, each wave instruction 256 contiguous bytes of one texel row (lane = channel).  The same grouping
// and the same phase 1 as pixgather_f32_kernel: one wave per 16 consecutive samples of one view, lane i < 16 projects sample
// i with the forward's own device functions, the corner indices / weights come back as wave-uniform scalars.
// A corner whose weight is zero (the clamped side of a border sample) contributes nothing and is skipped.
// Float atomic sums depend on arrival order: the result is NOT bitwise reproducible from run to run (last-bit differences,
// like torch's grid_sample backward); every element is within fp32 summation error of the exact adjoint.
// Bound: the atomic rate, 16 C bytes added per (sample, view): 2.8 GB at P = 153 600, V = 3 -> ~2.2 ms.
#include "th_internal.h"

#define PGB_G 16

__global__ __launch_bounds__(256) void pixgather_bwd_kernel(int V, int C, int H, int W, const float* __restrict__ pts_world,
                                                            int P, const float* __restrict__ cams,
                                                            const float* __restrict__ scale, const float* __restrict__ gout,
                                                            int ldo, float* __restrict__ gmap) {
    const int lane = threadIdx.x & 63;
    const long long grp = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long ngrp = (long long)((P + PGB_G - 1) / PGB_G) * V;
    if (grp >= ngrp) return;
    const int v = (int)(grp % V);
    const int p0 = (int)(grp / V) * PGB_G;
    const int nrow = min(PGB_G, P - p0);
    float* m = gmap + (long long)v * H * W * C;
    Bilin b;
    {
        const int p = p0 + min(lane, nrow - 1);
        const float x = pts_world[3 * (long long)p], y = pts_world[3 * (long long)p + 1], z = pts_world[3 * (long long)p + 2];
        float uu, vv;
        th_project(cams + 21 * v, x, y, z, uu, vv);
        b = th_bilinear_setup(uu, vv, scale[0], scale[1], H, W);
    }
    for (int i = 0; i < nrow; ++i) {
        const int idx[4] = {__builtin_amdgcn_readlane(b.i00, i), __builtin_amdgcn_readlane(b.i01, i),
                            __builtin_amdgcn_readlane(b.i10, i), __builtin_amdgcn_readlane(b.i11, i)};
        const float w[4] = {__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b.w00), i)),
                            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b.w01), i)),
                            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b.w10), i)),
                            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b.w11), i))};
        const float* g = gout + ((long long)(p0 + i) * V + v) * ldo;
        for (int c = lane; c < C; c += 64) {
            const float gv = g[c];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (w[q] != 0.f) atomicAdd(m + (long long)idx[q] * C + c, w[q] * gv);      // (result unused: no-return form)
        }
    }
}

int th_pixgather_bwd_launch(int V, int C, int H, int W, const float* pts_world, int P, const float* cams, const float* scale,
                            const float* grad_out, int ldo, float* grad_map, hipStream_t s) {
    TH_REQUIRE(V >= 1 && H >= 1 && W >= 1 && P >= 0, "need V, H, W >= 1 and P >= 0");
    TH_REQUIRE(C >= 4 && (C & 3) == 0 && (ldo & 3) == 0 && ldo >= C, "channel count / row stride must be multiples of 4, ldo >= C");
    TH_REQUIRE((long long)H * W < (1ll << 31), "map too large");
    TH_HIP(hipMemsetAsync(grad_map, 0, (size_t)V * H * W * C * sizeof(float), s));
    if (P == 0) return 0;
    const long long groups = (long long)th_cdiv(P, PGB_G) * V;
    hipLaunchKernelGGL(pixgather_bwd_kernel, dim3(th_cdiv(groups, 4)), dim3(256), 0, s, V, C, H, W, pts_world, P, cams, scale,
                       grad_out, ldo, grad_map);
    TH_LAUNCH_CHECK();
    return 0;
}
