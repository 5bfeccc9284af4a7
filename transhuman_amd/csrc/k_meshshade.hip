// K15: area-weighted vertex normals of a triangle mesh and the normal-coloured Phong image of it, on top of K14's depth /
// pix_to_face (the frames of the reference's render_mesh_dynamic.py:182-276, which renders them with pytorch3d's MeshRasterizer +
// SoftPhongShader.  pytorch3d is third-party and absent, so no frame of the reference's exists to compare with: the image is
// defined by this project, following the settings the script passes, and parity with pytorch3d itself is unpinned -- DESIGN.md 4
// K15).
//
// Definition (normative; transhuman_amd/mesh_render.py::vertex_normals_oracle / render_mesh_oracle restate it in float64 / int64
// numpy).  All arithmetic is float64 on the exactly promoted fp32 inputs, without contraction, in the order written; every
// output is rounded once to fp32.
//   vertex normals   face (i0, i1, i2): e1 = v1 - v0, e2 = v2 - v0, c = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z,
//                    e1_x e2_y - e1_y e2_x); q = rint(c 2^40) per component (round-half-even) as int64; every corner of the face
//                    receives q: an exact integer sum per vertex and component, whatever the order of the faces and the launch
//                    shape.  s = (double)sum 2^-40, n = s / max(sqrt((s_x^2 + s_y^2) + s_z^2), 1e-6) (a vertex without faces, or
//                    with cancelling ones: (0, 0, 0)); flip: n = 0 - n.  The normals belong to the mesh, not to a view: faces the
//                    rasteriser skips count.
//   range            a mesh is in range when every |c_k| 2^40 <= 2^62 / nf (evaluated in float64): no vertex is a corner of
//                    more than nf faces with c != 0, so no true sum leaves (-2^63, 2^63).  A face outside the range adds nothing
//                    and sets bit 1 of the status word; a face index outside [0, nv) is never dereferenced, its face adds
//                    nothing and sets bit 0.
//   fragments        at a pixel with pix_to_face = f >= 0: the three snapped projections of K14 (its expression order), the
//                    orientation to positive area by swapping the 2nd and 3rd corner, e_i and 2A in int64 at the pixel centre,
//                    w_i = e_i / 2A, b_i = (w_i / z_i) / ((w_0 / z_0 + w_1 / z_1) + w_2 / z_2): the perspective-correct weights, from
//                    the integers that decided the coverage.  Sums over the corners are ((b_0 x_0 + b_1 x_1) + b_2 x_2), oriented order.
//   shading          p = sum b_i v_i, n = sum b_i n_i, nh = n / max(|n|, 1e-6); texel t = sum b_i (0.7 (F R n_i) + 0.7) with R the
//                    view's rotation, (R n)_a = (R_a0 n_x + R_a1 n_y) + R_a2 n_z, F = diag(1, -1, -1); lh = (L - p) / max(|L - p|, 1e-6),
//                    vh = (C - p) / max(|C - p|, 1e-6), C_a = 0 - ((R_0a T_0 + R_1a T_1) + R_2a T_2); |x| = sqrt((x_0^2 + x_1^2) + x_2^2),
//                    dots in the same association; d = nh . lh, r = (2 d) nh - lh, s = max(vh . r, 0) squared log2(m) times;
//                    colour_c = (a + k_d max(d, 0)) t_c + k_s (d > 0 ? s : 0).  Unclamped.  Elsewhere: background, exactly.
//
// Kernels
//   normals_accumulate_kernel   one lane per face: 9 plain 64-bit vector atomicAdd (zeros are not sent).  A 256^3 marching-cubes
//                               mesh has ~4e5 faces: 3.6e6 adds of 8 bytes, two orders of magnitude under a millisecond's worth
//                               of the chip's atomic rate; valence-512 vertices serialise 512 adds, no more.
//   normals_finish_kernel       one lane per vertex
//   mesh_shade_kernel           one lane per pixel, consecutive lanes on consecutive pixels of a row-major image, views in grid z;
//                               the three projections are recomputed per covered pixel (63 float64 operations) rather than kept
//                               from the rasteriser's workspace, which belongs to another call.
#include "th_internal.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr double MS_SCALE = 1099511627776.0;            // 2^40
constexpr double MS_SUM_MAX = 4611686018427387904.0;    // 2^62
constexpr double MS_EPS = 1e-6;
constexpr double MS_NEAR = 1e-3;                         // (K14's skip rules)
constexpr double MS_UV_MAX = 1048576.0;

struct MsParams {
    double light[3];
    float background[3];
    double ambient, diffuse, specular;
    int squarings;       // log2(shininess)
};

__global__ __launch_bounds__(MS_THREADS) void normals_accumulate_kernel(const float* __restrict__ verts, int nv,
                                                                        const int* __restrict__ faces, int nf, double limit,
                                                                        unsigned long long* __restrict__ sums,
                                                                        unsigned* __restrict__ status) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= nf) return;
    const int idx[3] = {faces[3 * (long long)i], faces[3 * (long long)i + 1], faces[3 * (long long)i + 2]};
    if ((unsigned)idx[0] >= (unsigned)nv || (unsigned)idx[1] >= (unsigned)nv || (unsigned)idx[2] >= (unsigned)nv) {
        atomicOr(status, 1u);
        return;
    }
    double v[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[k][a] = (double)verts[3 * (long long)idx[k] + a];
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = v[1][a] - v[0][a]; e2[a] = v[2][a] - v[0][a]; }
    const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double t[3] = {c[0] * MS_SCALE, c[1] * MS_SCALE, c[2] * MS_SCALE};
    if (!(fabs(t[0]) <= limit && fabs(t[1]) <= limit && fabs(t[2]) <= limit)) {     // (NaN and infinity included)
        atomicOr(status, 2u);
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long q = (long long)rint(t[a]);
        if (q == 0) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(&sums[3 * (long long)idx[k] + a], (unsigned long long)q);     // (two's complement)
    }
}

__device__ __forceinline__ double ms_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// x / max(|x|, 1e-6)
__device__ __forceinline__ void ms_unit(const double* x, double* out) {
#pragma clang fp contract(off)
    const double len = fmax(sqrt(ms_dot(x, x)), MS_EPS);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = x[a] / len;
}

__global__ __launch_bounds__(MS_THREADS) void normals_finish_kernel(const unsigned long long* __restrict__ sums, int nv, int flip,
                                                                    float* __restrict__ normals) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= nv) return;
    double s[3], n[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = (double)(long long)sums[3 * (long long)i + a] / MS_SCALE;      // (a power of two: exact)
    ms_unit(s, n);
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * (long long)i + a] = (float)(flip ? 0.0 - n[a] : n[a]);
}

struct MsCorner {
    long long X, Y;      // snapped to 1/256 pixel
    double z;
    int idx;
};

// K14's projection (raster_project_kernel), false where its triangle is skipped
__device__ __forceinline__ bool ms_project(const float* __restrict__ c, const float* __restrict__ p, MsCorner& o) {
#pragma clang fp contract(off)
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    double cam[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        cam[a] = (((double)c[3 * a] * x + (double)c[3 * a + 1] * y) + (double)c[3 * a + 2] * z) + (double)c[9 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        q[a] = ((double)c[12 + 3 * a] * cam[0] + (double)c[12 + 3 * a + 1] * cam[1]) + (double)c[12 + 3 * a + 2] * cam[2];
    const double u = q[0] / q[2], w = q[1] / q[2];
    if (!(cam[2] > MS_NEAR && fabs(u) < MS_UV_MAX && fabs(w) < MS_UV_MAX)) return false;
    o.X = (long long)rint(u * 256.0);
    o.Y = (long long)rint(w * 256.0);
    o.z = cam[2];
    return true;
}

__device__ __forceinline__ long long ms_edge(const MsCorner& a, const MsCorner& b, long long px, long long py) {
    return (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X);
}

__global__ __launch_bounds__(MS_THREADS) void mesh_shade_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                int nv, const int* __restrict__ faces, int nf,
                                                                const float* __restrict__ cams, int H, int W,
                                                                const int* __restrict__ pix_to_face, MsParams prm,
                                                                float* __restrict__ image) {
#pragma clang fp contract(off)
    const long long hw = (long long)H * W;
    const long long pix = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (pix >= hw) return;
    const int view = blockIdx.z;
    const long long at = (long long)view * hw + pix;
    float* out = image + 3 * at;
    float rgb[3] = {prm.background[0], prm.background[1], prm.background[2]};
    const float* cm = cams + 21 * view;
    const int f = pix_to_face[at];
    MsCorner t[3];
    // (an entry that is no face of this mesh, or a face the rasteriser skips for this view, shades as background)
    bool hit = (unsigned)f < (unsigned)nf;
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[k].idx = faces[3 * (long long)f + k];
            hit = hit && (unsigned)t[k].idx < (unsigned)nv;
        }
    }
    if (hit) {
#pragma unroll
        for (int k = 0; k < 3; ++k) hit = ms_project(cm, verts + 3 * (long long)t[k].idx, t[k]) && hit;
    }
    long long area2 = 0;
    if (hit) {
        area2 = ms_edge(t[0], t[1], t[2].X, t[2].Y);
        if (area2 < 0) { const MsCorner s = t[1]; t[1] = t[2]; t[2] = s; area2 = -area2; }
        hit = area2 != 0;
    }
    if (hit) {
        const int row = (int)(pix / W), col = (int)(pix - (long long)row * W);
        const long long px = (long long)col * 256, py = (long long)row * 256;
        const double area = (double)area2;
        const double e[3] = {(double)ms_edge(t[1], t[2], px, py), (double)ms_edge(t[2], t[0], px, py),
                             (double)ms_edge(t[0], t[1], px, py)};
        const double wz[3] = {(e[0] / area) / t[0].z, (e[1] / area) / t[1].z, (e[2] / area) / t[2].z};
        const double den = (wz[0] + wz[1]) + wz[2];
        const double b[3] = {wz[0] / den, wz[1] / den, wz[2] / den};
        double v[3][3], n[3][3], tex[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[k][a] = (double)verts[3 * (long long)t[k].idx + a];
                n[k][a] = (double)normals[3 * (long long)t[k].idx + a];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double m = ((double)cm[3 * a] * n[k][0] + (double)cm[3 * a + 1] * n[k][1]) + (double)cm[3 * a + 2] * n[k][2];
                tex[k][a] = 0.7 * (a == 0 ? m : 0.0 - m) + 0.7;
            }
        }
        double p[3], nn[3], tx[3], eye[3], tl[3], tv[3], nh[3], lh[3], vh[3], r[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = (b[0] * v[0][a] + b[1] * v[1][a]) + b[2] * v[2][a];
            nn[a] = (b[0] * n[0][a] + b[1] * n[1][a]) + b[2] * n[2][a];
            tx[a] = (b[0] * tex[0][a] + b[1] * tex[1][a]) + b[2] * tex[2][a];
            eye[a] = 0.0 - (((double)cm[a] * (double)cm[9] + (double)cm[3 + a] * (double)cm[10]) + (double)cm[6 + a] * (double)cm[11]);
            tl[a] = prm.light[a] - p[a];
            tv[a] = eye[a] - p[a];
        }
        ms_unit(nn, nh);
        ms_unit(tl, lh);
        ms_unit(tv, vh);
        const double d = ms_dot(nh, lh);
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] = (2.0 * d) * nh[a] - lh[a];
        double s = fmax(ms_dot(vh, r), 0.0);
        for (int k = 0; k < prm.squarings; ++k) s = s * s;
        const double shade = prm.ambient + prm.diffuse * fmax(d, 0.0);
        const double spec = prm.specular * (d > 0.0 ? s : 0.0);
#pragma unroll
        for (int a = 0; a < 3; ++a) rgb[a] = (float)(shade * tx[a] + spec);
    }
    out[0] = rgb[0]; out[1] = rgb[1]; out[2] = rgb[2];
}

bool ms_mesh_ok(int nv, int nf) { return nv >= 1 && nf >= 1; }

}  // namespace

// the vertices' exact integer normal sums [nv][3]
static unsigned long long* normals_layout(ThArena& ar, int nv) { return ar.take<unsigned long long>((size_t)nv * 3); }
size_t th_vertex_normals_ws(int nv, int nf) { return ms_mesh_ok(nv, nf) ? th_measure(normals_layout, nv) : 0; }

int th_vertex_normals_launch(const float* verts, int nv, const int32_t* faces, int nf, int flip, float* normals, int32_t* status,
                             void* ws, size_t ws_bytes, hipStream_t s) {
    TH_REQUIRE(ms_mesh_ok(nv, nf), "bad mesh (n_verts, n_faces >= 1)");
    ThArena ar(ws, ws_bytes);
    unsigned long long* sums = normals_layout(ar, nv);
    TH_REQUIRE(ar.ok(), "workspace too small (th_vertex_normals_workspace_bytes)");
    TH_HIP(hipMemsetAsync(sums, 0, (size_t)nv * 3 * sizeof(unsigned long long), s));
    TH_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(normals_accumulate_kernel, dim3(th_cdiv(nf, MS_THREADS)), dim3(MS_THREADS), 0, s, verts, nv, faces, nf,
                       MS_SUM_MAX / (double)nf, sums, (unsigned*)status);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(normals_finish_kernel, dim3(th_cdiv(nv, MS_THREADS)), dim3(MS_THREADS), 0, s, sums, nv, flip ? 1 : 0,
                       normals);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_shade_mesh_launch(const float* verts, const float* normals, int nv, const int32_t* faces, int nf, const float* cams, int V,
                         int H, int W, const int32_t* pix_to_face, const float* light, const float* background, float ambient,
                         float diffuse, float specular, int shininess, float* image, hipStream_t s) {
    TH_REQUIRE(ms_mesh_ok(nv, nf) && V >= 1 && V <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 &&
                   (long long)V * H * W < (1LL << 31),
               "bad mesh, view count or image size (1 <= H, W <= 16384; V <= 65535; V H W < 2^31)");
    TH_REQUIRE(shininess >= 1 && (shininess & (shininess - 1)) == 0, "shininess must be a power of two (it is taken by squaring)");
    MsParams prm;
    for (int a = 0; a < 3; ++a) { prm.light[a] = (double)light[a]; prm.background[a] = background[a]; }
    prm.ambient = (double)ambient; prm.diffuse = (double)diffuse; prm.specular = (double)specular;
    prm.squarings = 0;
    while ((1 << prm.squarings) < shininess) ++prm.squarings;
    hipLaunchKernelGGL(mesh_shade_kernel, dim3(th_cdiv((long long)H * W, MS_THREADS), 1, V), dim3(MS_THREADS), 0, s, verts, normals,
                       nv, faces, nf, cams, H, W, pix_to_face, prm, image);
    TH_LAUNCH_CHECK();
    return 0;
}
