// K14: z-buffer rasteriser of a triangle mesh into V depth / face-index images, and the two vertex-visibility rules on top of it
// (batch['input_vizmaps'] and batch['input_depthmaps'] of the reference, can_smpl.py:439-475, which it only LOADS from an
// archive: no program of the reference writes them, so the rasteriser's definition is this project's own).
//
// Definition (normative; transhuman_amd/visibility.py::rasterize_oracle restates it in numpy and reproduces pix_to_face bit
// for bit):
//   projection   per vertex and view in float64 on the exactly promoted fp32 inputs, no contraction, in this order:
//                cam_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i,  p_i = (K_i0 cam_0 + K_i1 cam_1) + K_i2 cam_2,
//                u = p_0 / p_2, v = p_1 / p_2, z = cam_2           (if_clight_renderer.py:123-126 in float64)
//   pixel grid   the centre of pixel (col, row) is (u, v) = (col, row)   (the reference's align_corners=True sampling)
//   snapping     X = rint(256 u), Y = rint(256 v), round-half-even: 1/256 pixel
//   skipped      a triangle with a vertex at z <= 1e-3, or with |u| or |v| not below 2^20 (NaN included), or of zero snapped
//                area.  There is NO clipping: a triangle that crosses the near plane is dropped whole.
//   coverage     either winding; the triangle is oriented to positive area 2A = E(V0, V1, V2) by swapping V1 and V2, with
//                E(A, B, P) = (Bx - Ax)(Py - Ay) - (By - Ay)(Px - Ax) in int64; e_0 = E(V1, V2, P), e_1 = E(V2, V0, P),
//                e_2 = E(V0, V1, P) at the pixel centre P = (256 col, 256 row).  A pixel is covered where every e_i > 0, or
//                e_i = 0 on a top or left edge: with y pointing down and this orientation an edge A -> B is a top edge when
//                By = Ay and Bx > Ax, a left edge when By < Ay.  The neighbour across a shared edge walks it the other way
//                round, so a pixel centre on it belongs to exactly one of the two.  Only the pixels of the snapped bounding
//                box, clamped to the image, are visited.
//   depth        w_i = e_i / 2A, zf = 1 / ((w_0 / z_0 + w_1 / z_1) + w_2 / z_2) in float64 (oriented order), rounded once to
//                fp32
//   z-buffer     one uint64 per pixel, (fp32 bits of zf) << 32 | face index, initialised to all ones, reduced with the 64-bit
//                atomicMin: the nearest fragment wins, equal fp32 depths go to the lower face index -- the result does not
//                depend on the launch shape or the order of the faces' execution.
//
// Kernels
//   raster_project_kernel   the V nv projections, once, into the workspace (16 B per vertex and view)
//   raster_small_kernel     one triangle per lane while its clamped box has at most RS_SMALL_PIXELS pixels (a projected SMPL
//                           triangle at 512^2 covers about 6); larger ones go onto a compacted list
//   raster_big_kernel       that list, one 256-lane workgroup per (triangle, slice of RS_BIG_SPLIT), lanes striding over the box: an
//                           image-filling triangle is 128 pixels per lane at 512^2, not 262 144 in one
//   raster_resolve_kernel   keys -> depth (background where nothing landed) and pix_to_face (-1)
// Plain vector atomics only (global 64-bit atomicMin, one 32-bit atomicAdd per listed triangle).
#include "th_internal.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_SMALL_PIXELS = 64;    // clamped-box pixels one lane rasterises itself
constexpr int RS_BIG_SPLIT = 8;        // workgroups that share the box of one listed triangle
constexpr int RS_BIG_GRID = 1024;      // workgroups (x) striding over the list
constexpr double RS_NEAR = 1e-3;
constexpr double RS_UV_MAX = 1048576.0;   // 2^20

struct RsVert {          // one projected vertex of one view; z = 0 marks a vertex that skips its triangles
    int X, Y;            // snapped to 1/256 pixel (|u|, |v| < 2^20: 29 bits)
    double z;
};

struct RsTri {           // oriented to positive area
    long long X[3], Y[3];
    double z[3];
    long long area2;
    bool tl[3];          // e_i's edge is a top or left edge
    int x0, x1, y0, y1;  // clamped box, inclusive
};

__global__ __launch_bounds__(RS_THREADS) void raster_project_kernel(const float* __restrict__ verts, int nv,
                                                                    const float* __restrict__ cams, int V,
                                                                    RsVert* __restrict__ out, unsigned* __restrict__ counters) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i == 0) { counters[0] = 0u; counters[1] = 0u; }     // [0] listed triangles, [1] bad face index seen
    if (i >= V * nv) return;
    const int view = i / nv, k = i % nv;
    const float* c = cams + 21 * view;
    const double x = (double)verts[3 * k], y = (double)verts[3 * k + 1], z = (double)verts[3 * k + 2];
    double cam[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        cam[a] = (((double)c[3 * a] * x + (double)c[3 * a + 1] * y) + (double)c[3 * a + 2] * z) + (double)c[9 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = ((double)c[12 + 3 * a] * cam[0] + (double)c[12 + 3 * a + 1] * cam[1]) + (double)c[12 + 3 * a + 2] * cam[2];
    const double u = p[0] / p[2], v = p[1] / p[2];
    RsVert r;
    const bool ok = cam[2] > RS_NEAR && fabs(u) < RS_UV_MAX && fabs(v) < RS_UV_MAX;    // (false for NaN)
    r.X = ok ? (int)rint(u * 256.0) : 0;
    r.Y = ok ? (int)rint(v * 256.0) : 0;
    r.z = ok ? cam[2] : 0.0;
    out[i] = r;
}

__device__ __forceinline__ long long rs_edge(long long ax, long long ay, long long bx, long long by, long long px,
                                             long long py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ bool rs_top_left(long long ax, long long ay, long long bx, long long by) {
    return (by == ay && bx > ax) || by < ay;
}

// false: the triangle is skipped for this view (or has an index outside [0, nv): *bad is then set)
__device__ __forceinline__ bool rs_setup(const RsVert* __restrict__ pv, const int* __restrict__ faces, int face, int nv, int H,
                                         int W, RsTri& t, unsigned* __restrict__ bad) {
    const int i0 = faces[3 * face], i1 = faces[3 * face + 1], i2 = faces[3 * face + 2];
    if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) {
        *bad = 1u;
        return false;
    }
    RsVert a = pv[i0], b = pv[i1], c = pv[i2];
    if (a.z == 0.0 || b.z == 0.0 || c.z == 0.0) return false;
    long long area2 = rs_edge(a.X, a.Y, b.X, b.Y, c.X, c.Y);
    if (area2 == 0) return false;
    if (area2 < 0) { RsVert s = b; b = c; c = s; area2 = -area2; }
    t.X[0] = a.X; t.Y[0] = a.Y; t.z[0] = a.z;
    t.X[1] = b.X; t.Y[1] = b.Y; t.z[1] = b.z;
    t.X[2] = c.X; t.Y[2] = c.Y; t.z[2] = c.z;
    t.area2 = area2;
    t.tl[0] = rs_top_left(t.X[1], t.Y[1], t.X[2], t.Y[2]);
    t.tl[1] = rs_top_left(t.X[2], t.Y[2], t.X[0], t.Y[0]);
    t.tl[2] = rs_top_left(t.X[0], t.Y[0], t.X[1], t.Y[1]);
    const int xmin = min(a.X, min(b.X, c.X)), xmax = max(a.X, max(b.X, c.X));
    const int ymin = min(a.Y, min(b.Y, c.Y)), ymax = max(a.Y, max(b.Y, c.Y));
    // first / last pixel centre inside the snapped box (arithmetic shifts: floor for negative coordinates too)
    t.x0 = max((xmin + 255) >> 8, 0); t.x1 = min(xmax >> 8, W - 1);
    t.y0 = max((ymin + 255) >> 8, 0); t.y1 = min(ymax >> 8, H - 1);
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

__device__ __forceinline__ void rs_pixel(const RsTri& t, int col, int row, int W, unsigned face,
                                         unsigned long long* __restrict__ zbuf /* this view's */) {
#pragma clang fp contract(off)
    const long long px = (long long)col * 256, py = (long long)row * 256;
    const long long e0 = rs_edge(t.X[1], t.Y[1], t.X[2], t.Y[2], px, py);
    const long long e1 = rs_edge(t.X[2], t.Y[2], t.X[0], t.Y[0], px, py);
    const long long e2 = rs_edge(t.X[0], t.Y[0], t.X[1], t.Y[1], px, py);
    const bool in = (e0 > 0 || (e0 == 0 && t.tl[0])) && (e1 > 0 || (e1 == 0 && t.tl[1])) && (e2 > 0 || (e2 == 0 && t.tl[2]));
    if (!in) return;
    const double area = (double)t.area2;
    const double w0 = (double)e0 / area, w1 = (double)e1 / area, w2 = (double)e2 / area;
    const double zf = 1.0 / ((w0 / t.z[0] + w1 / t.z[1]) + w2 / t.z[2]);
    const float zr = (float)zf;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zr) << 32) | (unsigned long long)face;
    atomicMin(&zbuf[(long long)row * W + col], key);
}

__global__ __launch_bounds__(RS_THREADS) void raster_small_kernel(const RsVert* __restrict__ proj,
                                                                  const int* __restrict__ faces, int nf, int nv, int V, int H,
                                                                  int W, unsigned long long* __restrict__ zbuf,
                                                                  unsigned* __restrict__ big_list,
                                                                  unsigned* __restrict__ counters) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= V * nf) return;
    const int view = i / nf, face = i % nf;
    RsTri t;
    if (!rs_setup(proj + (long long)view * nv, faces, face, nv, H, W, t, counters + 1)) return;
    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    if ((long long)bw * bh > RS_SMALL_PIXELS) {
        big_list[atomicAdd(&counters[0], 1u)] = (unsigned)i;     // (at most V nf entries: the list's capacity)
        return;
    }
    unsigned long long* zb = zbuf + (long long)view * H * W;
    for (int row = t.y0; row <= t.y1; ++row)
        for (int col = t.x0; col <= t.x1; ++col) rs_pixel(t, col, row, W, (unsigned)face, zb);
}

__global__ __launch_bounds__(RS_THREADS) void raster_big_kernel(const RsVert* __restrict__ proj, const int* __restrict__ faces,
                                                                int nf, int nv, int H, int W,
                                                                unsigned long long* __restrict__ zbuf,
                                                                const unsigned* __restrict__ big_list,
                                                                unsigned* __restrict__ counters) {
    const unsigned n = counters[0];
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const unsigned i = big_list[e];
        const int view = (int)(i / (unsigned)nf), face = (int)(i % (unsigned)nf);
        RsTri t;
        if (!rs_setup(proj + (long long)view * nv, faces, face, nv, H, W, t, counters + 1)) continue;
        const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
        const long long np = (long long)bw * bh;
        unsigned long long* zb = zbuf + (long long)view * H * W;
        for (long long p = (long long)blockIdx.y * RS_THREADS + threadIdx.x; p < np; p += (long long)RS_BIG_SPLIT * RS_THREADS) {
            const int r = (int)(p / bw), c = (int)(p - (long long)r * bw);
            rs_pixel(t, t.x0 + c, t.y0 + r, W, (unsigned)face, zb);
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void raster_resolve_kernel(const unsigned long long* __restrict__ zbuf, long long n,
                                                                    float background, float* __restrict__ depth,
                                                                    int* __restrict__ pix_to_face) {
    const long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = zbuf[i];
    const bool hit = key != ~0ull;
    depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : background;
    pix_to_face[i] = hit ? (int)(unsigned)(key & 0xffffffffull) : -1;
}

// vertex n is visible in view v iff it is a corner of a face that owns a pixel of pix_to_face[v]: byte 1 at the three corners of
// every pixel's face (equal-value races).  Entries outside the mesh are ignored.
__global__ __launch_bounds__(RS_THREADS) void vertex_visibility_kernel(const int* __restrict__ pix_to_face,
                                                                       const int* __restrict__ faces, int nf, int nv,
                                                                       long long hw, long long n, uint8_t* __restrict__ vis) {
    const long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = pix_to_face[i];
    if ((unsigned)f >= (unsigned)nf) return;
    uint8_t* o = vis + (i / hw) * nv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int idx = faces[3 * f + k];
        if ((unsigned)idx < (unsigned)nv) o[idx] = 1;
    }
}

// get_relative_depth (if_clight_renderer.py:75-93) on the projection of :123-126, fp32, operation for operation:
//   uv_normed = uv / H * 2 - 1 (BOTH coordinates over shape[2] = H, :85), F.grid_sample at its defaults (bilinear, zeros padding,
//   align_corners=False: x = ((g + 1) W - 1) / 2), vis = depth <= surface + det, relative = depth - (surface + det),
//   depth = p_2 (:131).
__global__ __launch_bounds__(RS_THREADS) void depth_visibility_kernel(const float* __restrict__ verts, int nv,
                                                                      const float* __restrict__ cams, int V,
                                                                      const float* __restrict__ dmap, int H, int W, float det,
                                                                      float* __restrict__ surface, uint8_t* __restrict__ vis,
                                                                      float* __restrict__ relative) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= V * nv) return;
    const int view = i / nv, k = i % nv;
    const float* cam = cams + 21 * view;
    const float x = verts[3 * k], y = verts[3 * k + 1], z = verts[3 * k + 2];
    // (th_project's arithmetic, keeping p_2)
    const float cx = fmaf(cam[2], z, fmaf(cam[1], y, cam[0] * x)) + cam[9];
    const float cy = fmaf(cam[5], z, fmaf(cam[4], y, cam[3] * x)) + cam[10];
    const float cz = fmaf(cam[8], z, fmaf(cam[7], y, cam[6] * x)) + cam[11];
    const float* K = cam + 12;
    const float px = fmaf(K[2], cz, fmaf(K[1], cy, K[0] * cx));
    const float py = fmaf(K[5], cz, fmaf(K[4], cy, K[3] * cx));
    const float pz = fmaf(K[8], cz, fmaf(K[7], cy, K[6] * cx));
    const float u = px / pz, v = py / pz;
    const float gx = (u / (float)H) * 2.0f - 1.0f, gy = (v / (float)H) * 2.0f - 1.0f;
    const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    float s = 0.0f;
    // (a coordinate that is not finite or far outside samples nothing but padding, like grid_sample's out-of-range corners)
    if (ix > -2.0f && ix < (float)W + 1.0f && iy > -2.0f && iy < (float)H + 1.0f) {
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
        const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
        const float* m = dmap + (long long)view * H * W;
        const bool xin0 = x0 >= 0 && x0 < W, xin1 = x1 >= 0 && x1 < W, yin0 = y0 >= 0 && y0 < H, yin1 = y1 >= 0 && y1 < H;
        if (xin0 && yin0) s = s + m[(long long)y0 * W + x0] * (wx0 * wy0);
        if (xin1 && yin0) s = s + m[(long long)y0 * W + x1] * (wx1 * wy0);
        if (xin0 && yin1) s = s + m[(long long)y1 * W + x0] * (wx0 * wy1);
        if (xin1 && yin1) s = s + m[(long long)y1 * W + x1] * (wx1 * wy1);
    }
    const float lim = s + det;
    surface[i] = s;
    vis[i] = pz <= lim ? 1 : 0;
    relative[i] = pz - lim;
}

struct RsLayout { size_t proj, zbuf, list, counters, total; };

RsLayout rs_layout(int V, int nv, int nf, int H, int W) {
    RsLayout l;
    size_t off = 0;
    l.proj = off;     off += th_align((size_t)V * nv * sizeof(RsVert));
    l.zbuf = off;     off += th_align((size_t)V * H * W * sizeof(unsigned long long));
    l.list = off;     off += th_align((size_t)V * nf * sizeof(unsigned));
    l.counters = off; off += th_align(2 * sizeof(unsigned));
    l.total = off;
    return l;
}

bool rs_shape_ok(int V, int nv, int nf, int H, int W) {
    return V >= 1 && nv >= 1 && nf >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 &&
           (long long)V * H * W < (1LL << 31) && (long long)V * nf < (1LL << 31) && (long long)V * nv < (1LL << 31);
}

}  // namespace

size_t th_raster_ws(int V, int nv, int nf, int H, int W) {
    if (!rs_shape_ok(V, nv, nf, H, W)) return 0;
    return rs_layout(V, nv, nf, H, W).total;
}

int th_raster_launch(const float* verts, int nv, const int32_t* faces, int nf, const float* cams, int V, int H, int W,
                     float background, float* depth, int32_t* pix_to_face, void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(rs_shape_ok(V, nv, nf, H, W), "bad mesh, view count or image size (1 <= H, W <= 16384; V H W, V nf, V nv < 2^31)");
    const RsLayout l = rs_layout(V, nv, nf, H, W);
    TH_REQUIRE(ws_bytes >= l.total, "workspace too small (th_rasterize_workspace_bytes)");
    char* base = (char*)ws;
    RsVert* proj = (RsVert*)(base + l.proj);
    unsigned long long* zbuf = (unsigned long long*)(base + l.zbuf);
    unsigned* list = (unsigned*)(base + l.list);
    unsigned* counters = (unsigned*)(base + l.counters);
    const long long npix = (long long)V * H * W;
    TH_HIP(hipMemsetAsync(zbuf, 0xff, (size_t)npix * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(raster_project_kernel, dim3(th_cdiv((long long)V * nv, RS_THREADS)), dim3(RS_THREADS), 0, s, verts, nv,
                       cams, V, proj, counters);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_small_kernel, dim3(th_cdiv((long long)V * nf, RS_THREADS)), dim3(RS_THREADS), 0, s, proj, faces,
                       nf, nv, V, H, W, zbuf, list, counters);
    TH_LAUNCH_CHECK();
    const long long ntri = (long long)V * nf;
    hipLaunchKernelGGL(raster_big_kernel, dim3((unsigned)(ntri < RS_BIG_GRID ? ntri : RS_BIG_GRID), RS_BIG_SPLIT),
                       dim3(RS_THREADS), 0, s, proj, faces, nf, nv, H, W, zbuf, list, counters);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(th_cdiv(npix, RS_THREADS)), dim3(RS_THREADS), 0, s, zbuf, npix, background,
                       depth, pix_to_face);
    TH_LAUNCH_CHECK();
    // face indices outside [0, nv) were skipped on the device (never dereferenced) and flagged: report them
    unsigned flag = 0;
    TH_HIP(hipMemcpyAsync(&flag, counters + 1, sizeof(flag), hipMemcpyDeviceToHost, s));
    TH_HIP(hipStreamSynchronize(s));
    TH_REQUIRE(flag == 0, "a face index is outside [0, n_verts)");
    return 0;
}

int th_vertex_visibility_launch(const int32_t* pix_to_face, const int32_t* faces, int nf, int nv, int V, int H, int W,
                                uint8_t* vis, hipStream_t s) {
    TH_REQUIRE(rs_shape_ok(V, nv, nf, H, W), "bad mesh, view count or image size");
    const long long n = (long long)V * H * W;
    TH_HIP(hipMemsetAsync(vis, 0, (size_t)V * nv, s));
    hipLaunchKernelGGL(vertex_visibility_kernel, dim3(th_cdiv(n, RS_THREADS)), dim3(RS_THREADS), 0, s, pix_to_face, faces, nf, nv,
                       (long long)H * W, n, vis);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_depth_visibility_launch(const float* verts, int nv, const float* cams, int V, const float* depthmaps, int H, int W,
                               float det, float* surface, uint8_t* vis, float* relative, hipStream_t s) {
    TH_REQUIRE(rs_shape_ok(V, nv, 1, H, W), "bad vertex count, view count or image size");
    hipLaunchKernelGGL(depth_visibility_kernel, dim3(th_cdiv((long long)V * nv, RS_THREADS)), dim3(RS_THREADS), 0, s, verts, nv,
                       cams, V, depthmaps, H, W, det, surface, vis, relative);
    TH_LAUNCH_CHECK();
    return 0;
}
