// K7: alpha-composited ray integration + view-direction embedding.
//
// raw2outputs (lib/networks/renderer/nerf_net_utils.py:14-59): delta_i =
// (z_{i+1}-z_i)*|d| with delta_last = 1e10*|d|, c = sigmoid(raw_rgb),
// alpha = 1 - exp(-relu(sigma)*delta), T_i = prod_{j<i}(1 - alpha_j + 1e-10),
// w = alpha*T, rgb = sum w c, depth = sum w z, acc = sum w.
// One wavefront per ray: with the reference's 64 samples/ray a ray is exactly
// one wave64; the exclusive transmittance product is a shuffle scan and the
// three sums are shuffle reductions (no LDS).  S != 64 runs in 64-sample
// passes carrying T across passes.
// Bound: HBM streaming, 16 B/sample in (raw) + 20 B/ray out.
#include "th_internal.h"

__global__ __launch_bounds__(256) void composite_kernel(const float4* __restrict__ raw, const float* __restrict__ zin,
                                                        ThPointSrc ps, int white, float* __restrict__ rgb,
                                                        float* __restrict__ acc, float* __restrict__ depth,
                                                        float* __restrict__ wout, const uint8_t* __restrict__ mask,
                                                        const int32_t* __restrict__ ray_hit) {
    const int lane = threadIdx.x & 63;
    int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= ps.R) return;
    const int S = ps.S;
    // A ray that misses the hull has no live sample (the hull stage raises ray_hit with every mask bit it sets): every weight is
    // 0 and the outputs are exact zeros (no white background either, see below) -- written without the 64 exponentials and the
    // scan.  4/5 of the headline frame's rays: 265 -> 90 us.
    if (ray_hit != nullptr && mask != nullptr && ray_hit[ray] == 0) {
        if (wout)
            for (int s = lane; s < S; s += 64) wout[(long long)ray * S + s] = 0.f;
        if (lane == 0) {
            rgb[3 * ray] = 0.f; rgb[3 * ray + 1] = 0.f; rgb[3 * ray + 2] = 0.f;
            acc[ray] = 0.f;
            depth[ray] = 0.f;
        }
        return;
    }
    float dx = ps.ray_d[3 * ray], dy = ps.ray_d[3 * ray + 1], dz = ps.ray_d[3 * ray + 2];
    float nd = dx * dx + dy * dy;
    nd = __fsqrt_rn(nd + dz * dz);                       // torch.norm(rays_d)
    float carryT = 1.0f;
    float sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f, sa = 0.f;
    // (render_fast composites the rays that hit the hull only, if_clight_renderer.py:467-476: a ray that misses stays zero)
    const bool noisy = ps.noise != nullptr && (ray_hit == nullptr || ray_hit[ray] != 0);
    for (int base = 0; base < S; base += 64) {
        int s = base + lane;
        bool ok = s < S;
        float z = 0.f, zn = 0.f;
        if (ok) {
            z = zin ? zin[(long long)ray * S + s] : th_sample_z(ps, ray, s);
            if (s + 1 < S) zn = zin ? zin[(long long)ray * S + s + 1] : th_sample_z(ps, ray, s + 1);
        }
        float delta = (s + 1 < S) ? (zn - z) : 1e10f;
        delta = delta * nd;
        // mask given: samples outside the hull carry raw = 0 (cross_transformer.py:231) without being stored or read
        const bool live = ok && (mask == nullptr || mask[(long long)ray * S + s] != 0);
        float4 r = live ? raw[(long long)ray * S + s] : make_float4(0.f, 0.f, 0.f, 0.f);
        // density noise (nerf_net_utils.py:39-44): on every sample of a composited ray, the zeros outside the hull included
        if (noisy && ok) r.w = r.w + ps.noise[(long long)ray * S + s];
        float alpha = ok ? 1.0f - expf(-fmaxf(r.w, 0.0f) * delta) : 0.0f;
        float t = (1.0f - alpha) + 1e-10f;                // factor contributed to later samples
        if (!ok) t = 1.0f;
        // inclusive product scan over the wave, then shift to exclusive
        float inc = t;
        for (int o = 1; o < 64; o <<= 1) {
            float u = __shfl_up(inc, o);
            if (lane >= o) inc = inc * u;
        }
        float excl = __shfl_up(inc, 1);
        if (lane == 0) excl = 1.0f;
        float T = carryT * excl;
        float w = alpha * T;
        carryT = carryT * __shfl(inc, 63);
        if (ok && wout) wout[(long long)ray * S + s] = w;
        float cr = 1.0f / (1.0f + expf(-r.x)), cg = 1.0f / (1.0f + expf(-r.y)), cb = 1.0f / (1.0f + expf(-r.z));
        sr += w * cr; sg += w * cg; sb += w * cb; sd += w * z; sa += w;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sr += __shfl_xor(sr, o); sg += __shfl_xor(sg, o); sb += __shfl_xor(sb, o);
        sd += __shfl_xor(sd, o); sa += __shfl_xor(sa, o);
    }
    if (lane == 0) {
        // white background: render_fast composites only the rays that hit the hull and scatters them into zeros
        // (if_clight_renderer.py:467-476), so a ray that misses stays black even with white_bkgd; Renderer.render
        // (:486-498) composites every ray (ray_hit == nullptr or all ones)
        if (white && (ray_hit == nullptr || ray_hit[ray] != 0)) { float bg = 1.0f - sa; sr += bg; sg += bg; sb += bg; }
        rgb[3 * ray] = sr; rgb[3 * ray + 1] = sg; rgb[3 * ray + 2] = sb;
        acc[ray] = sa;
        depth[ray] = sd;
    }
}

int th_composite_launch(const float* raw, const float* z, const ThPointSrc& ps, int white, float* rgb, float* acc,
                        float* depth, float* wout, const uint8_t* mask, hipStream_t s, const int32_t* ray_hit) {
    if (ps.R <= 0) return 0;
    hipLaunchKernelGGL(composite_kernel, dim3(th_cdiv(ps.R, 4)), dim3(256), 0, s, (const float4*)raw, z, ps, white, rgb,
                       acc, depth, wout, mask, ray_hit);
    TH_LAUNCH_CHECK();
    return 0;
}

// view embedding: v = d/|d| ; [v, sin(2^k v), cos(2^k v)] (embedder.py:9-35, view_res=4)
// `hit` (optional): rays whose flag is zero are skipped -- their rows are never read (a view direction is looked up per
// SHADED sample, and every shaded sample belongs to a ray that touches the hull): 4/5 of the frame's 24 sin / cos per ray
__global__ void view_embed_kernel(const float* __restrict__ d, int R, int res, float* __restrict__ out,
                                  const int32_t* __restrict__ hit) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (hit != nullptr && hit[r] == 0) return;
    float x = d[3 * r], y = d[3 * r + 1], z = d[3 * r + 2];
    float n = x * x + y * y;
    n = __fsqrt_rn(n + z * z);
    float v[3] = {x / n, y / n, z / n};
    float* o = out + (long long)r * (3 + 6 * res);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    for (int k = 0; k < res; ++k) {
        float f = (float)(1 << k);
        for (int a = 0; a < 3; ++a) {
            o[3 + 6 * k + a] = sinf(v[a] * f);
            o[3 + 6 * k + 3 + a] = cosf(v[a] * f);
        }
    }
}
int th_view_embed_launch(const float* d, int R, int res, float* out, hipStream_t s, const int32_t* hit) {
    if (R <= 0) return 0;
    hipLaunchKernelGGL(view_embed_kernel, dim3(th_cdiv(R, 256)), dim3(256), 0, s, d, R, res, out, hit);
    TH_LAUNCH_CHECK();
    return 0;
}

// ---- K7 backward ----------------------------------------------------------------------------------------------------------
// raw2outputs' adjoint with respect to raw [R,S,4], term by term as torch differentiates nerf_net_utils.py:14-59.  With
//   c = sigmoid(raw_rgb), s = relu(raw_sigma), e = exp(-s delta), a = 1 - e, t = 1 - a + 1e-10, T_i = prod_{j<i} t_j, w = a T:
//   G_i      = g_rgb . c_i + g_acc' + g_depth z_i          (dL/dw_i; white background: g_acc' = g_acc - sum(g_rgb), else g_acc)
//   d raw_rgb = w_i g_rgb c_i (1 - c_i)                     (sigmoid')
//   dL/da_i  = G_i T_i - (sum_{j>i} G_j w_j) / t_i          (cumprod's backward: the reversed cumulative sum over the input)
//   d raw_sigma = [raw_sigma > 0] dL/da_i delta_i e_i       (relu'(0) = 0; delta_last = 1e10 |d|)
// One wave per ray, like the forward: the transmittance is the forward's own product scan (same statements, same carry across
// 64-sample passes), then the passes run in reverse with a wave suffix-sum scan for sum_{j>i} G_j w_j and its carry.  Every
// step is a fixed function of the inputs: bit-identical from run to run.  z, ray_d, near and far get no gradient.
#define CB_MAXPASS 4          // S <= 256
__global__ __launch_bounds__(256) void composite_bwd_kernel(const float4* __restrict__ raw, const float* __restrict__ zin,
                                                            ThPointSrc ps, int white, const float* __restrict__ g_rgb,
                                                            const float* __restrict__ g_acc, const float* __restrict__ g_depth,
                                                            float4* __restrict__ g_raw) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= ps.R) return;
    const int S = ps.S;
    const float dx = ps.ray_d[3 * ray], dy = ps.ray_d[3 * ray + 1], dz = ps.ray_d[3 * ray + 2];
    float nd = dx * dx + dy * dy;
    nd = __fsqrt_rn(nd + dz * dz);
    const float gr = g_rgb[3 * ray], gg = g_rgb[3 * ray + 1], gb = g_rgb[3 * ray + 2], gd = g_depth[ray];
    float ga = g_acc[ray];
    if (white) ga = ga - ((gr + gg) + gb);
    const int npass = (S + 63) / 64;
    float carryT[CB_MAXPASS + 1];
    carryT[0] = 1.0f;
    float suffix = 0.f;                                  // sum of G_j w_j over the passes behind the current one
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        // dir 0: the forward's transmittance carried into every pass; dir 1: the passes in reverse
#pragma unroll
        for (int it = 0; it < CB_MAXPASS; ++it) {
            const int pass = dir == 0 ? it : CB_MAXPASS - 1 - it;
            if (pass >= npass) continue;
            const int s = pass * 64 + lane;
            const bool ok = s < S;
            float z = 0.f, zn = 0.f;
            if (ok) {
                z = zin ? zin[(long long)ray * S + s] : th_sample_z(ps, ray, s);
                if (s + 1 < S) zn = zin ? zin[(long long)ray * S + s + 1] : th_sample_z(ps, ray, s + 1);
            }
            float delta = (s + 1 < S) ? (zn - z) : 1e10f;
            delta = delta * nd;
            const float4 r = ok ? raw[(long long)ray * S + s] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float e = expf(-fmaxf(r.w, 0.0f) * delta);
            const float alpha = ok ? 1.0f - e : 0.0f;
            float t = (1.0f - alpha) + 1e-10f;
            if (!ok) t = 1.0f;
            float inc = t;
            for (int o = 1; o < 64; o <<= 1) {
                const float u = __shfl_up(inc, o);
                if (lane >= o) inc = inc * u;
            }
            if (dir == 0) {
                carryT[pass + 1] = carryT[pass] * __shfl(inc, 63);
                continue;
            }
            float excl = __shfl_up(inc, 1);
            if (lane == 0) excl = 1.0f;
            const float T = carryT[pass] * excl;
            const float w = alpha * T;
            const float cr = 1.0f / (1.0f + expf(-r.x)), cg = 1.0f / (1.0f + expf(-r.y)), cb = 1.0f / (1.0f + expf(-r.z));
            const float G = ((gr * cr + gg * cg) + gb * cb) + ga + gd * z;
            const float x = ok ? G * w : 0.f;
            float sfx = x;                               // inclusive suffix sum over the wave
            for (int o = 1; o < 64; o <<= 1) {
                const float u = __shfl_down(sfx, o);
                if (lane + o < 64) sfx = sfx + u;
            }
            float after = __shfl_down(sfx, 1);
            if (lane == 63) after = 0.f;
            after = after + suffix;
            suffix = suffix + __shfl(sfx, 0);
            const float g_a = G * T - after / t;
            float4 o4;
            o4.x = (w * gr) * ((1.0f - cr) * cr);
            o4.y = (w * gg) * ((1.0f - cg) * cg);
            o4.z = (w * gb) * ((1.0f - cb) * cb);
            o4.w = r.w > 0.0f ? (g_a * e) * delta : 0.0f;
            if (ok) g_raw[(long long)ray * S + s] = o4;
        }
    }
}

int th_composite_bwd_launch(const float* raw, const float* z, const ThPointSrc& ps, int white, const float* g_rgb,
                            const float* g_acc, const float* g_depth, float* g_raw, hipStream_t s) {
    TH_REQUIRE(ps.R >= 0 && ps.S >= 1 && ps.S <= 64 * CB_MAXPASS, "need 1 <= S <= 256 samples per ray");
    if (ps.R == 0) return 0;
    hipLaunchKernelGGL(composite_bwd_kernel, dim3(th_cdiv(ps.R, 4)), dim3(256), 0, s, (const float4*)raw, z, ps, white, g_rgb,
                       g_acc, g_depth, (float4*)g_raw);
    TH_LAUNCH_CHECK();
    return 0;
}
