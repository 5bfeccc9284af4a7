// What K4 (k_dparf.hip) and K27 (k_truncate.hip) share about "distance to a token centre": the squared-distance expression,
// the candidate grid's record, and -- for K27 -- the distance to the NEAREST centre by the same scan K4 runs for its seven.
// One copy, so the truncation test `sqrt(d2min) < sigma` sees bit for bit the distance of K4's first neighbour.
#pragma once
#include "th_internal.h"

#define DPG_MAXCELLS 32768
#define DPG_STRIDE 192
#define DPG_CELL 0.075f        // cell size asked for at N_c = 500; 0.1: lists of ~70 candidates, 0.075: ~55, K4 0.73 -> 0.71 ms; (dpgrid_setup_kernel grows it until the grid fits DPG_MAXCELLS)
struct DpGrid {
    float gmin[3];
    float g, inv_g;
    int dim[3];
    int ncell;          // 0: grid disabled (too many cells)
};

// th_dparf_grid_build's workspace: the grid's record, every cell's candidate count and list (only the builder casts the const away)
struct DpGridView { const DpGrid* gi; const int *cell_count, *cand; };
static inline DpGridView dp_grid_layout(ThArena& ar) {
    return {ar.take<DpGrid>(1), ar.take<int>(DPG_MAXCELLS), ar.take<int>((size_t)DPG_MAXCELLS * DPG_STRIDE)};
}
// the view of a built grid handed on without its size (nullptr: no grid, the scans run over all centres)
static inline DpGridView dp_grid_view(const void* grid_ws, int nc) {
    if (grid_ws == nullptr) return {nullptr, nullptr, nullptr};
    ThArena ar(const_cast<void*>(grid_ws), th_dparf_grid_ws(nc));
    return dp_grid_layout(ar);
}

#ifdef __HIPCC__
// |p - c|^2 as (dx dx + dy dy) + dz dz, every product and sum rounded on its own (the library is built without contraction);
// tests/dparf_cases.py pins this order
__device__ __forceinline__ float dp_dist2(float x, float y, float z, float cx, float cy, float cz) {
    float dx = x - cx, dy = y - cy, dz = z - cz;
    float d2 = dx * dx + dy * dy;
    d2 = d2 + dz * dz;
    return d2;
}

// world2smpl, if_clight_renderer.py:289-295: (p - Th) @ Rh, the three fused chains K4 forms
__device__ __forceinline__ void dp_world2smpl(float wx, float wy, float wz, const float* __restrict__ Rh,
                                              const float* __restrict__ Th, float& x, float& y, float& z) {
    float ax = wx - Th[0], ay = wy - Th[1], az = wz - Th[2];
    x = fmaf(az, Rh[6], fmaf(ay, Rh[3], ax * Rh[0]));
    y = fmaf(az, Rh[7], fmaf(ay, Rh[4], ax * Rh[1]));
    z = fmaf(az, Rh[8], fmaf(ay, Rh[5], ax * Rh[2]));
}

// min over the centres of dp_dist2 -- over the candidate list of the point's grid cell where there is one (an exact superset of
// its 7 nearest centres, so of its nearest), else over all nc centres: the value of K4's bd[0].  3e38 if no distance compares
// below it (a NaN coordinate).  `centres` is read from global memory: the full scan's addresses are wave-uniform.
__device__ __forceinline__ float dp_nearest_d2(float x, float y, float z, const float* __restrict__ centres, int nc,
                                               const DpGrid* __restrict__ gi, const int* __restrict__ cell_count,
                                               const int* __restrict__ cand) {
    const int* list = nullptr;
    int nlist = nc;
    if (gi != nullptr && gi->ncell > 0) {
        const int cx = (int)floorf((x - gi->gmin[0]) * gi->inv_g), cy = (int)floorf((y - gi->gmin[1]) * gi->inv_g),
                  cz = (int)floorf((z - gi->gmin[2]) * gi->inv_g);
        if (cx >= 0 && cx < gi->dim[0] && cy >= 0 && cy < gi->dim[1] && cz >= 0 && cz < gi->dim[2]) {
            const int cell = (cz * gi->dim[1] + cy) * gi->dim[0] + cx;
            const int cnt = cell_count[cell];
            if (cnt >= 0) {
                list = cand + (long long)cell * DPG_STRIDE;
                nlist = cnt;
            }
        }
    }
    float best = 3.0e38f;
    for (int j = 0; j < nlist; ++j) {
        const int c = list ? list[j] : j;
        const float d2 = dp_dist2(x, y, z, centres[3 * c], centres[3 * c + 1], centres[3 * c + 2]);
        if (d2 < best) best = d2;
    }
    return best;
}
#endif
