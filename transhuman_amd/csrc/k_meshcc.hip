// K24: connected components of a welded triangle mesh and the order-preserving component filter, on device.
//
// Definition (this project's; transhuman_amd/mesh_clean.py restates it in numpy): two faces are connected when they share a
// vertex INDEX; the label of a vertex is the smallest vertex index of its component; a vertex no face references keeps its own
// index and belongs to no component with faces; a component's size is its number of faces (degenerate and duplicate faces
// count).  trimesh.split connects through shared EDGES: the two rules differ only where parts touch in a single vertex.
//
// Components: a multi-launch fixpoint.  No workgroup ever waits for another inside a kernel (no spin, no device-wide barrier,
// no persistent kernel); the only ordering is the kernel boundary.
//   init   label[v] = v
//   hook   one thread per face: m = min(label[a], label[b], label[c]) from plain loads, then an agent-scope integer atomicMin
//          of m onto the three labels and onto the three entries the labels point at (label[label[a]] ...: the roots, so that
//          whole trees merge and not only their rims); a launch raises its own flag word when any atomicMin lowered a value
//   jump   one thread per vertex: label[v] = label[label[v]], followed up to CC_HOPS entries deep; CC_JUMPS launches per sweep
// The host queues CC_BATCH sweeps (hook + jumps), reads the batch's flag words through a pinned buffer and stops at the first
// hook launch that lowered nothing.
//
// Why this ends with the right labels although a plain load inside a launch may return a stale (older, larger) label:
//   (1) labels only decrease: every write is an atomicMin, or a jump's store of a value read from label[label[v]] <= label[v];
//   (2) a label is always an index of the same component: m is the label of a vertex of the same face, a jump reads the label
//       of a vertex of the same component, and a stale value is an earlier label, to which the same applies;
//   (3) label[v] <= v throughout: true at init, and writes only lower;
//   (4) a hook launch that lowered nothing wrote nothing, so every load in it returned the launch-start values, which the
//       kernel boundary made visible.  No atomicMin lowering anything means la == lb == lc for every face at those values:
//       every face is uniform, so every component is constant.  By (2) and (3) the component's smallest vertex r has
//       label[r] <= r inside the component, i.e. label[r] == r, so the constant is r.  Unreferenced vertices are never touched
//       by a hook and a jump maps v -> label[v] = v.
// Bound on the sweeps: r never changes; a vertex at face-distance k from r has, at the start of hook k, a face-neighbour
// labelled r (launch-start value, nothing lower exists), so it is labelled r after hook k.  Every vertex is done after at most
// (n_verts - 1) hooks and the next one lowers nothing: no valid mesh reaches the cap of n_verts + 2 sweeps.  (In practice the
// root hooks and the jumps merge trees geometrically: a handful of sweeps.)
//
// Integer atomics only (min, add, or, a packed 64-bit max): every output is a function of the input alone, bit-identical from
// run to run whatever the workspace held before -- every workspace word that is read is written first by the same call.
//
// Filter: face counts per label (integer atomicAdd, pre-reduced per wave over runs of adjacent faces with one label), the
// largest component as ONE packed key (count << 32) | ~label under atomicMax (a tie goes to the smallest label), keep flags per
// vertex and face, exclusive prefix sums (the block-sum scan of k_mcubes.hip) and a scatter: kept vertices and faces stay in
// their original order, indices remapped, vert_map[v] = new index or -1.
#include <cstring>

#include "th_internal.h"

#define CC_HOPS 8        // entries a jump follows per launch
#define CC_JUMPS 2       // jump launches per sweep
#define CC_BATCH 4       // sweeps queued per host read of the flags
#define CC_SCAN_B 1024

// control block at the start of the workspace (int32 words)
#define CC_ERR 0         // bit 0: a face index outside [0, nv); bit 1: a label outside [0, nv)
#define CC_NCOMP 1       // components with at least one face
#define CC_BEST 4        // (words 4-5: the 64-bit arg-max key)
#define CC_FLAGS 8       // words 8..8+CC_BATCH-1: "this hook launch lowered a label"
#define CC_TOTALS 16     // words 16-19: kept vertices, kept faces (two int64)
#define CC_CTL_WORDS 32

__global__ __launch_bounds__(256) void cc_check_faces_kernel(const int32_t* __restrict__ faces, long long n3, int nv,
                                                             int* __restrict__ ctl) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const bool bad = i < n3 && (unsigned)faces[i] >= (unsigned)nv;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&ctl[CC_ERR], 1);
}
__global__ __launch_bounds__(256) void cc_check_labels_kernel(const int32_t* __restrict__ label, int nv, int* __restrict__ ctl) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const bool bad = v < nv && (unsigned)label[v] >= (unsigned)nv;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&ctl[CC_ERR], 2);
}

__global__ __launch_bounds__(256) void cc_init_kernel(int32_t* __restrict__ label, int nv) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v < nv) label[v] = (int32_t)v;
}

__device__ __forceinline__ bool cc_lower(int32_t* p, int m) {
    return __hip_atomic_fetch_min(p, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > m;
}

// `label` is read and written by other workgroups in the same launch: plain (vector) loads, never const / __restrict__
__global__ __launch_bounds__(256) void cc_hook_kernel(const int32_t* __restrict__ faces, int nf, int32_t* label, int* flag) {
    const long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool lowered = false;
    if (f < nf) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const int la = label[a], lb = label[b], lc = label[c];
        const int m = min(la, min(lb, lc));
        // (a label that already reads m cannot be lowered by m: its true value is <= what was read)
        if (la > m) { lowered |= cc_lower(&label[a], m); lowered |= cc_lower(&label[la], m); }
        if (lb > m) { lowered |= cc_lower(&label[b], m); lowered |= cc_lower(&label[lb], m); }
        if (lc > m) { lowered |= cc_lower(&label[c], m); lowered |= cc_lower(&label[lc], m); }
    }
    if (__any(lowered) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void cc_jump_kernel(int32_t* label, int nv) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int l0 = label[v];
    int l = l0;
#pragma unroll 1
    for (int h = 0; h < CC_HOPS; ++h) {
        const int n = label[l];
        if (n == l) break;
        l = n;
    }
    if (l != l0) label[v] = l;
}

// faces per label: cnt[label of the face] += 1, one atomicAdd per run of adjacent faces of a wave with the same label
__global__ __launch_bounds__(256) void cc_count_kernel(const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ label,
                                                       int* __restrict__ cnt) {
    const long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool act = f < nf;
    const int l = act ? label[faces[3 * f]] : -1;
    const int lp = __shfl_up(l, 1);
    const bool head = act && (lane == 0 || lp != l);
    const unsigned long long hm = __ballot(head), am = __ballot(act);      // (the active lanes are a prefix of the wave)
    if (head) {
        const unsigned long long above = lane == 63 ? 0ull : (hm >> (lane + 1)) << (lane + 1);
        const int end = above ? __ffsll((long long)above) - 1 : __popcll(am);
        atomicAdd(&cnt[l], end - lane);
    }
}

// components with faces, and the largest one: key = (count << 32) | ~label, wave maximum first
__global__ __launch_bounds__(256) void cc_best_kernel(const int* __restrict__ cnt, int nv, int* __restrict__ ctl) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int n = v < nv ? cnt[v] : 0;
    unsigned hi = n > 0 ? (unsigned)n : 0u, lo = n > 0 ? ~(unsigned)v : 0u;
    const unsigned long long some = __ballot(n > 0);
    if (some == 0) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ohi = __shfl_xor(hi, o), olo = __shfl_xor(lo, o);
        if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&ctl[CC_NCOMP], __popcll(some));
        atomicMax((unsigned long long*)(ctl + CC_BEST), ((unsigned long long)hi << 32) | lo);
    }
}

// keep flags.  min_faces == 0: the largest component only; else every component with >= min_faces faces.  A vertex no face
// references has cnt[label] == 0 and is always dropped.
__global__ __launch_bounds__(256) void cc_keep_verts_kernel(const int32_t* __restrict__ label, int nv, const int* __restrict__ cnt,
                                                            const int* __restrict__ ctl, int min_faces, int* __restrict__ vflag) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int l = label[v], n = cnt[l];
    bool keep;
    if (min_faces == 0) {
        const unsigned long long key = *(const unsigned long long*)(ctl + CC_BEST);
        keep = n > 0 && key != 0ull && l == (int)~(unsigned)(key & 0xffffffffull);
    } else {
        keep = n > 0 && n >= min_faces;
    }
    vflag[v] = keep ? 1 : 0;
}
__global__ __launch_bounds__(256) void cc_keep_faces_kernel(const int32_t* __restrict__ faces, int nf, const int* __restrict__ vflag,
                                                            int* __restrict__ fflag) {
    const long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (f < nf) fflag[f] = vflag[faces[3 * f]];
}

// exclusive prefix sums of 0/1 flags (the scan of k_mcubes.hip: 1024 elements per block, block sums, one block over the sums)
__global__ __launch_bounds__(256) void cc_scan_block_kernel(const int* __restrict__ in, int* __restrict__ out, long long n,
                                                            long long* __restrict__ sums) {
    __shared__ int ws[4];
    const long long base = (long long)blockIdx.x * CC_SCAN_B + 4 * threadIdx.x;
    int v[4];
    int t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < n ? in[base + k] : 0;
        t += v[k];
    }
    int inc = t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += ws[w];
    int run = woff + inc - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 255) sums[blockIdx.x] = (long long)run;
}
__global__ __launch_bounds__(1024) void cc_scan_sums_kernel(long long* __restrict__ sums, int nb, long long* __restrict__ total) {
    __shared__ long long part[1024];
    const int per = (nb + 1023) / 1024;
    const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    long long t = 0;
    for (int i = lo; i < hi; ++i) t += sums[i];
    part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < 1024; ++i) { const long long v = part[i]; part[i] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const long long v = sums[i]; sums[i] = run; run += v; }
}
__global__ __launch_bounds__(256) void cc_scan_add_kernel(int* __restrict__ a, long long n, const long long* __restrict__ sums) {
    const long long base = (long long)blockIdx.x * CC_SCAN_B + 4 * threadIdx.x;
    const int off = (int)sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < n) a[base + k] += off;
}

__global__ __launch_bounds__(256) void cc_emit_verts_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ vflag,
                                                            const int* __restrict__ vscan, double* __restrict__ verts_out,
                                                            int32_t* __restrict__ vert_map) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= nv) return;
    if (!vflag[v]) { vert_map[v] = -1; return; }
    const long long j = vscan[v];
    vert_map[v] = (int32_t)j;
    if (verts != nullptr) {
        verts_out[3 * j] = verts[3 * v];
        verts_out[3 * j + 1] = verts[3 * v + 1];
        verts_out[3 * j + 2] = verts[3 * v + 2];
    }
}
__global__ __launch_bounds__(256) void cc_emit_faces_kernel(const int32_t* __restrict__ faces, int nf, const int* __restrict__ fflag,
                                                            const int* __restrict__ fscan, const int* __restrict__ vscan,
                                                            int32_t* __restrict__ faces_out) {
    const long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (f >= nf || !fflag[f]) return;
    const long long j = fscan[f];
#pragma unroll
    for (int k = 0; k < 3; ++k) faces_out[3 * j + k] = vscan[faces[3 * f + k]];      // (a kept face has three kept corners)
}

// ---- workspace ----
static size_t cc_nb(long long n) { return (size_t)((n + CC_SCAN_B - 1) / CC_SCAN_B); }
// control words, the labels' face counts, keep flags and their prefix sums of vertices and faces, the scans' block sums
struct CcWs { int *ctl, *cnt, *vflag, *vscan, *fflag, *fscan; long long *vsums, *fsums; };
static CcWs cc_layout(ThArena& ar, int nv, int nf) {
    return {ar.take<int>(CC_CTL_WORDS), ar.take<int>((size_t)nv), ar.take<int>((size_t)nv), ar.take<int>((size_t)nv),
            ar.take<int>((size_t)nf), ar.take<int>((size_t)nf), ar.take<long long>(cc_nb(nv) + 2),
            ar.take<long long>(cc_nb(nf) + 2)};
}
size_t th_meshcc_ws(int nv, int nf) { return (nv < 0 || nf < 0) ? 0 : th_measure(cc_layout, nv, nf); }
static int cc_carve(const void* ws, size_t ws_bytes, int nv, int nf, CcWs& w) {
    ThArena ar(const_cast<void*>(ws), ws_bytes);
    w = cc_layout(ar, nv, nf);
    TH_REQUIRE(ar.ok(), "workspace too small");
    return 0;
}

// first pass: every face index (and, with `label`, every label) inside [0, nv); the error word comes to the host BEFORE
// anything is indexed by them.  `pinned`: 8 int32 words of pinned host memory.
static int cc_checked(const int32_t* faces, int nf, int nv, const int32_t* label, const CcWs& w, int32_t* pinned, hipStream_t s) {
    TH_HIP(hipMemsetAsync(w.ctl, 0, CC_CTL_WORDS * sizeof(int), s));
    if (nf > 0)
        hipLaunchKernelGGL(cc_check_faces_kernel, dim3(th_cdiv(3LL * nf, 256)), dim3(256), 0, s, faces, 3LL * nf, nv, w.ctl);
    if (label != nullptr && nv > 0)
        hipLaunchKernelGGL(cc_check_labels_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, label, nv, w.ctl);
    TH_LAUNCH_CHECK();
    TH_HIP(hipMemcpyAsync(pinned, w.ctl + CC_ERR, sizeof(int), hipMemcpyDeviceToHost, s));
    TH_HIP(hipStreamSynchronize(s));
    TH_REQUIRE((pinned[0] & 1) == 0, "a face index is outside [0, n_verts)");
    TH_REQUIRE((pinned[0] & 2) == 0, "a label is outside [0, n_verts)");
    return 0;
}

// face counts per label, the number of components with faces and the arg-max key (ctl is clear: cc_checked)
static int cc_stats(const int32_t* faces, int nf, int nv, const int32_t* label, const CcWs& w, hipStream_t s) {
    if (nv <= 0) return 0;
    TH_HIP(hipMemsetAsync(w.cnt, 0, (size_t)nv * sizeof(int), s));
    if (nf > 0) hipLaunchKernelGGL(cc_count_kernel, dim3(th_cdiv(nf, 256)), dim3(256), 0, s, faces, nf, label, w.cnt);
    hipLaunchKernelGGL(cc_best_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, w.cnt, nv, w.ctl);
    TH_LAUNCH_CHECK();
    return 0;
}

// info_host: {components with faces, sweeps, host reads of the flags, label of the largest component or -1, its faces}
int th_meshcc_components_launch(const int32_t* faces, int nf, int nv, int32_t* label, void* ws, size_t ws_bytes, int32_t* pinned,
                                int64_t* info_host, hipStream_t s) {
    TH_REQUIRE(nv >= 0 && nf >= 0, "negative size");
    CcWs w;
    TH_TRY(cc_carve(ws, ws_bytes, nv, nf, w));
    for (int k = 0; k < 5; ++k) info_host[k] = k == 3 ? -1 : 0;
    if (nv == 0 && nf == 0) return 0;
    TH_TRY(cc_checked(faces, nf, nv, nullptr, w, pinned, s));
    hipLaunchKernelGGL(cc_init_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, label, nv);
    TH_LAUNCH_CHECK();
    long long sweeps = 0, reads = 0;
    if (nf > 0) {
        const long long cap = (long long)nv + 2;          // (no valid mesh gets here: the header comment)
        bool done = false;
        while (!done) {
            TH_REQUIRE(sweeps < cap, "no fixpoint within n_verts + 2 sweeps");
            const int nb = (int)(cap - sweeps < CC_BATCH ? cap - sweeps : CC_BATCH);
            TH_HIP(hipMemsetAsync(w.ctl + CC_FLAGS, 0, CC_BATCH * sizeof(int), s));
            for (int k = 0; k < nb; ++k) {
                hipLaunchKernelGGL(cc_hook_kernel, dim3(th_cdiv(nf, 256)), dim3(256), 0, s, faces, nf, label, w.ctl + CC_FLAGS + k);
                for (int j = 0; j < CC_JUMPS; ++j)
                    hipLaunchKernelGGL(cc_jump_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, label, nv);
            }
            TH_LAUNCH_CHECK();
            TH_HIP(hipMemcpyAsync(pinned, w.ctl + CC_FLAGS, CC_BATCH * sizeof(int), hipMemcpyDeviceToHost, s));
            TH_HIP(hipStreamSynchronize(s));
            ++reads;
            int k = 0;
            while (k < nb && pinned[k] != 0) ++k;          // the first hook launch of the batch that lowered nothing
            done = k < nb;
            sweeps += done ? k + 1 : nb;
        }
    }
    TH_TRY(cc_stats(faces, nf, nv, label, w, s));
    TH_HIP(hipMemcpyAsync(pinned, w.ctl, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    TH_HIP(hipStreamSynchronize(s));
    unsigned long long key;
    memcpy(&key, pinned + CC_BEST, sizeof(key));
    info_host[0] = pinned[CC_NCOMP];
    info_host[1] = sweeps;
    info_host[2] = reads;
    info_host[3] = key ? (int64_t)(int32_t)~(uint32_t)(key & 0xffffffffull) : -1;
    info_host[4] = (int64_t)(key >> 32);
    return 0;
}

// keep flags and their prefix sums into the workspace; counts_host: {kept vertices, kept faces, components with faces,
// label of the largest component or -1}
int th_meshcc_filter_count_launch(const int32_t* faces, int nf, int nv, const int32_t* label, int min_faces, void* ws,
                                  size_t ws_bytes, int32_t* pinned, int64_t* counts_host, hipStream_t s) {
    TH_REQUIRE(nv >= 0 && nf >= 0 && min_faces >= 0, "negative size");
    CcWs w;
    TH_TRY(cc_carve(ws, ws_bytes, nv, nf, w));
    for (int k = 0; k < 4; ++k) counts_host[k] = k == 3 ? -1 : 0;
    if (nv == 0 && nf == 0) return 0;
    TH_TRY(cc_checked(faces, nf, nv, label, w, pinned, s));
    if (nv == 0) return 0;
    TH_TRY(cc_stats(faces, nf, nv, label, w, s));
    long long* totals = (long long*)(w.ctl + CC_TOTALS);
    hipLaunchKernelGGL(cc_keep_verts_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, label, nv, w.cnt, w.ctl, min_faces, w.vflag);
    const int nbv = (int)cc_nb(nv), nbf = (int)cc_nb(nf);
    hipLaunchKernelGGL(cc_scan_block_kernel, dim3(nbv), dim3(256), 0, s, w.vflag, w.vscan, (long long)nv, w.vsums);
    hipLaunchKernelGGL(cc_scan_sums_kernel, dim3(1), dim3(1024), 0, s, w.vsums, nbv, totals);
    hipLaunchKernelGGL(cc_scan_add_kernel, dim3(nbv), dim3(256), 0, s, w.vscan, (long long)nv, w.vsums);
    if (nf > 0) {
        hipLaunchKernelGGL(cc_keep_faces_kernel, dim3(th_cdiv(nf, 256)), dim3(256), 0, s, faces, nf, w.vflag, w.fflag);
        hipLaunchKernelGGL(cc_scan_block_kernel, dim3(nbf), dim3(256), 0, s, w.fflag, w.fscan, (long long)nf, w.fsums);
        hipLaunchKernelGGL(cc_scan_sums_kernel, dim3(1), dim3(1024), 0, s, w.fsums, nbf, totals + 1);
        hipLaunchKernelGGL(cc_scan_add_kernel, dim3(nbf), dim3(256), 0, s, w.fscan, (long long)nf, w.fsums);
    }
    TH_LAUNCH_CHECK();
    TH_HIP(hipMemcpyAsync(pinned, w.ctl, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    long long h[2];
    TH_HIP(hipMemcpyAsync(h, totals, sizeof(h), hipMemcpyDeviceToHost, s));
    TH_HIP(hipStreamSynchronize(s));
    unsigned long long key;
    memcpy(&key, pinned + CC_BEST, sizeof(key));
    counts_host[0] = h[0];
    counts_host[1] = nf > 0 ? h[1] : 0;
    counts_host[2] = pinned[CC_NCOMP];
    counts_host[3] = key ? (int64_t)(int32_t)~(uint32_t)(key & 0xffffffffull) : -1;
    return 0;
}

// the scatter behind th_meshcc_filter_count_launch on the same workspace and arrays.  verts may be null (map and faces only).
int th_meshcc_filter_emit_launch(const double* verts, const int32_t* faces, int nf, int nv, const void* ws, size_t ws_bytes,
                                 double* verts_out, int32_t* faces_out, int32_t* vert_map, hipStream_t s) {
    TH_REQUIRE(nv >= 0 && nf >= 0, "negative size");
    CcWs w;
    TH_TRY(cc_carve(ws, ws_bytes, nv, nf, w));
    if (nv <= 0) return 0;
    hipLaunchKernelGGL(cc_emit_verts_kernel, dim3(th_cdiv(nv, 256)), dim3(256), 0, s, verts, nv, w.vflag, w.vscan, verts_out, vert_map);
    if (nf > 0)
        hipLaunchKernelGGL(cc_emit_faces_kernel, dim3(th_cdiv(nf, 256)), dim3(256), 0, s, faces, nf, w.fflag, w.fscan, w.vscan, faces_out);
    TH_LAUNCH_CHECK();
    return 0;
}
