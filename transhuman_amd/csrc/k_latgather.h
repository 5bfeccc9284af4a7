// The per-sample set-up of K19 shared by its kernels (k_latgather.hip: forward and atomic adjoint; k_latgather_ord.hip: the
// ordered adjoint): one level's slot origin and 3 x 3 merged coefficients, and the clamped texel index of a slot.  Every
// kernel calls these same functions, so the coefficients of an adjoint are the forward's, bit for bit.
#pragma once
#include "th_internal.h"

struct LgLevels {
    int h[3], w[3];
};

// one level's 3 x 3 merged coefficients of one sample: slot (dr, dc) is latent texel (a + dr, b + dc)
__device__ __forceinline__ void lg_level(const Bilin& bl, int h, int w, int H, int W, int& a, int& b, float (&cf)[9]) {
    int ry[2][2], rx[2][2];
    float ly[2][2], lx[2][2];
    ups_coord(bl.y0, h, H, ry[0][0], ry[0][1], ly[0][0], ly[0][1]);
    ups_coord(bl.y1, h, H, ry[1][0], ry[1][1], ly[1][0], ly[1][1]);
    ups_coord(bl.x0, w, W, rx[0][0], rx[0][1], lx[0][0], lx[0][1]);
    ups_coord(bl.x1, w, W, rx[1][0], rx[1][1], lx[1][0], lx[1][1]);
    a = ry[0][0];
    b = rx[0][0];
    const float wq[2][2] = {{bl.w00, bl.w01}, {bl.w10, bl.w11}};
#pragma unroll
    for (int k = 0; k < 9; ++k) cf[k] = 0.f;
#pragma unroll
    for (int Y = 0; Y < 2; ++Y)
#pragma unroll
        for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    const int dr = ry[Y][ty] - a, dc = rx[X][tx] - b;
                    const int slot = (dr >= 0 && dr < 3 && dc >= 0 && dc < 3) ? dr * 3 + dc : -1;
                    const float t = wq[Y][X] * ly[Y][ty] * lx[X][tx];
#pragma unroll
                    for (int k = 0; k < 9; ++k) cf[k] += (slot == k) ? t : 0.f;      // (selects: no indexed registers)
                }
}

// lane i < nrow: the set-up of sample p0 + i (lanes beyond repeat the last sample)
__device__ __forceinline__ Bilin lg_setup(const float* __restrict__ pts_world, int p, const float* __restrict__ cam,
                                          const float* __restrict__ scale, int H, int W) {
    const float x = pts_world[3 * (long long)p], y = pts_world[3 * (long long)p + 1], z = pts_world[3 * (long long)p + 2];
    float uu, vv;
    th_project(cam, x, y, z, uu, vv);
    return th_bilinear_setup(uu, vv, scale[0], scale[1], H, W);
}

__device__ __forceinline__ float lg_lane_f(float v, int i) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}

// the clamped texel index of slot k of a level whose slot origin is (sa, sb)
__device__ __forceinline__ int lg_slot_index(int sa, int sb, int k, int h, int w) {
    return min(sa + k / 3, h - 1) * w + min(sb + k % 3, w - 1);
}
