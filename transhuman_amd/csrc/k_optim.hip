// K22: the optimiser step -- value clipping and the Adam / AdamW update of EVERY parameter tensor in one launch.
//
// The reference trains with torch.optim.Adam over one parameter group per tensor (lib/train/optimizer.py:16-19, 293 groups)
// behind clip_grad_value_(., 40) (lib/train/trainers/trainer.py:85): a set of small launches per tensor and step.  Here a
// step is one table copy and one kernel, whatever the tensor count:
//   chunk table    built once per parameter set (th_adam_plan): (tensor, element offset, count) per workgroup, every chunk
//                  but a tensor's last holding TH_ADAM_CHUNK elements; it stays on the device
//   tensor table   th_adam_tensor per tensor: the four data pointers and the step's scalars, computed on the host and
//                  rounded to fp32 once.  It travels through a ring of pinned staging buffers (kRing slots; an event per
//                  half of the ring, recorded once every kRing / 2 steps, says when that half's copies have left the host)
//   adam_step_kernel   one workgroup per chunk; 128-bit accesses where all four base pointers are 16-byte aligned (chunk
//                  offsets are multiples of 4 elements), a scalar path for the tail and for unaligned tensors
// Arithmetic (fp32, each operation rounded once -- the library is built with -ffp-contract=off; division and square root are
// correctly rounded, subnormals kept), the definition transhuman_amd.train_optim.adam_step_oracle restates in numpy:
//   g  = clamp(g, -c, c)                  (TH_ADAM_CLIP; a NaN stays NaN, as in torch.clamp)
//   g  = g + wd p                         (coupled, wd != 0)      or      p = p decay_mul   (TH_ADAM_T_DECOUPLED)
//   m' = m + (1 - b1) (g - m)
//   v' = b2 v + ((1 - b2) g) g
//   p' = p - step_size (m' / (sqrt(v') / bc2_sqrt + eps))
// Purely elementwise: no float atomics, no LDS, no scratch, bit-identical from run to run.  The only atomic is the integer
// count of non-finite gradient elements (TH_ADAM_COUNT_NONFINITE), one per wave that saw any.
// Bound: 16 B read + 12 B written per element (+ 4 B with TH_ADAM_ZERO_GRAD).
//
// The gradient exchange of data-parallel training (transhuman_amd/train_dist.py) walks the same chunk table:
//   adam_pack_kernel     flat[off_i + e] = g_i[e] / world for every tensor with a slot (zeros for a NULL g_i and for the
//                        padding behind a slot), so that ONE all-reduce of `flat` averages every gradient
//   adam_unpack_kernel   dst_i[e] = flat[off_i + e]
// with a per-call table of (pointer, slot offset) per tensor that travels through the same ring of staging buffers into a
// region of its own behind the chunk table.  The slots follow ad_flat_layout, the one statement of the layout rule in C.
//   rank_sum_kernel      K28, at the end of the file: the rank-ordered sum of the slices a reduce-scatter delivered
#include "th_internal.h"

#include <string.h>
#include <vector>

#define AD_THREADS 256
#define AD_VEC (TH_ADAM_CHUNK / 4 / AD_THREADS)      // float4 groups per lane of a full chunk
static_assert(TH_ADAM_CHUNK % (4 * AD_THREADS) == 0, "a full chunk is a whole number of float4 rounds");
static_assert(sizeof(th_adam_tensor) == 72, "th_adam_tensor layout (INTEGRATION.md)");

struct AdChunk {
    int32_t tensor;
    int32_t count;
    int64_t offset;
};

// device image behind the caller's `table` pointer
struct AdHeader {
    unsigned long long nonfinite;
    unsigned long long pad[31];
};

// per-call entry of the pack / unpack kernels: the tensor's own memory and the offset of its slot (< 0: no slot)
struct AdSlot {
    void* ptr;
    long long off;
};
static_assert(sizeof(AdSlot) <= sizeof(th_adam_tensor), "a slot table fits a staging buffer of the ring");

static inline size_t ad_tensor_off() { return sizeof(AdHeader); }
static inline size_t ad_chunk_off(int n_tensors) { return ad_tensor_off() + th_align((size_t)n_tensors * sizeof(th_adam_tensor)); }
static inline long long ad_max_chunks(int n_tensors, long long total) { return total / TH_ADAM_CHUNK + n_tensors; }
static inline size_t ad_slot_off(int n_tensors, long long total) {
    return ad_chunk_off(n_tensors) + th_align((size_t)ad_max_chunks(n_tensors, total) * sizeof(AdChunk));
}

struct th_adam_plan_t {
    static constexpr int kRing = 16;
    th_ctx* ctx = nullptr;
    char* table = nullptr;            // device
    int n_tensors = 0, n_chunks = 0;
    char* pinned = nullptr;           // kRing staging images of the tensor table + one read-back word
    size_t slot_bytes = 0;
    hipEvent_t half_ev[2] = {nullptr, nullptr};
    bool half_pending[2] = {false, false};
    hipStream_t half_stream[2] = {nullptr, nullptr};
    unsigned long long gen = 0;
    std::vector<long long> counts;    // elements per tensor (the layout rule is checked against them)
    size_t slot_table_off = 0;        // the AdSlot table of pack / unpack inside `table`
    const void* checked_flat = nullptr;   // the flat buffer the runtime was last asked about (pack / unpack ask when it changes)
    long long checked_elems = -1;
    std::vector<AdSlot> slot_host;    // ... and where a call assembles it (sized once: a call allocates nothing)
};

struct AdScalars {
    float step_size, bc2_sqrt, omb1, beta2, omb2, eps, wd, decay_mul, clip;
    bool decoupled, do_clip;
};

__device__ __forceinline__ void ad_elem(float& p, float& g, float& m, float& v, const AdScalars& s) {
    if (s.do_clip) g = g < -s.clip ? -s.clip : (g > s.clip ? s.clip : g);        // (compares are false on NaN: it stays)
    if (s.decoupled) p = p * s.decay_mul;
    else if (s.wd != 0.f) g = g + s.wd * p;
    m = m + s.omb1 * (g - m);
    v = s.beta2 * v + (s.omb2 * g) * g;
    p = p - s.step_size * (m / (sqrtf(v) / s.bc2_sqrt + s.eps));
}

__device__ __forceinline__ int ad_bad(float g) { return !(fabsf(g) <= 3.402823466e38f); }

typedef float AdF4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float AdGlobalF;
typedef __attribute__((address_space(1))) AdF4 AdGlobalF4;

__device__ __forceinline__ void ad_elem4(AdF4& P, AdF4& G, AdF4& M, AdF4& V, const AdScalars& s, int& bad) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float p = P[e], g = G[e], m = M[e], v = V[e];
        bad += ad_bad(g);
        ad_elem(p, g, m, v, s);
        P[e] = p; M[e] = m; V[e] = v;
    }
}

__global__ __launch_bounds__(AD_THREADS) void adam_step_kernel(const th_adam_tensor* __restrict__ tensors,
                                                               const AdChunk* __restrict__ chunks, float clip, int flags,
                                                               unsigned long long* __restrict__ nonfinite) {
    const AdChunk ch = chunks[blockIdx.x];
    const th_adam_tensor t = tensors[ch.tensor];
    if (t.p == nullptr) return;                                                   // no gradient this step: untouched
    AdScalars s;
    s.step_size = t.step_size; s.bc2_sqrt = t.bc2_sqrt; s.omb1 = t.one_minus_beta1; s.beta2 = t.beta2;
    s.omb2 = t.one_minus_beta2; s.eps = t.eps; s.wd = t.weight_decay; s.decay_mul = t.decay_mul; s.clip = clip;
    s.decoupled = (t.flags & TH_ADAM_T_DECOUPLED) != 0;
    s.do_clip = (flags & TH_ADAM_CLIP) != 0;
    const bool zero = (flags & TH_ADAM_ZERO_GRAD) != 0;
    // (the pointers come out of a table, so the compiler takes them for generic addresses and emits flat_load / flat_store;
    // they are global memory: say so and get global_load_dwordx4)
    AdGlobalF* __restrict__ p = (AdGlobalF*)(uintptr_t)t.p + ch.offset;
    AdGlobalF* __restrict__ g = (AdGlobalF*)(uintptr_t)t.g + ch.offset;
    AdGlobalF* __restrict__ m = (AdGlobalF*)(uintptr_t)t.m + ch.offset;
    AdGlobalF* __restrict__ v = (AdGlobalF*)(uintptr_t)t.v + ch.offset;
    const int n = ch.count, tid = threadIdx.x;
    int bad = 0;
    const bool aligned = ((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v)) & 15) == 0;
    int done = 0;
    if (aligned) {
        AdGlobalF4* p4 = (AdGlobalF4*)p; AdGlobalF4* g4 = (AdGlobalF4*)g; AdGlobalF4* m4 = (AdGlobalF4*)m;
        AdGlobalF4* v4 = (AdGlobalF4*)v;
        const AdF4 z4 = {0.f, 0.f, 0.f, 0.f};
        if (n == TH_ADAM_CHUNK) {
            AdF4 P[AD_VEC], G[AD_VEC], M[AD_VEC], V[AD_VEC];
#pragma unroll
            for (int r = 0; r < AD_VEC; ++r) {                                   // every load of the chunk in flight at once
                const int i = r * AD_THREADS + tid;
                P[r] = p4[i]; G[r] = g4[i]; M[r] = m4[i]; V[r] = v4[i];
            }
#pragma unroll
            for (int r = 0; r < AD_VEC; ++r) {
                const int i = r * AD_THREADS + tid;
                ad_elem4(P[r], G[r], M[r], V[r], s, bad);
                p4[i] = P[r]; m4[i] = M[r]; v4[i] = V[r];
                if (zero) g4[i] = z4;
            }
            done = n;
        } else {
            const int n4 = n >> 2;
            for (int i = tid; i < n4; i += AD_THREADS) {
                AdF4 P = p4[i], G = g4[i], M = m4[i], V = v4[i];
                ad_elem4(P, G, M, V, s, bad);
                p4[i] = P; m4[i] = M; v4[i] = V;
                if (zero) g4[i] = z4;
            }
            done = n4 << 2;
        }
    }
    for (int i = done + tid; i < n; i += AD_THREADS) {                           // tail, or a tensor off the 16-byte grid
        float P = p[i], G = g[i], M = m[i], V = v[i];
        bad += ad_bad(G);
        ad_elem(P, G, M, V, s);
        p[i] = P; m[i] = M; v[i] = V;
        if (zero) g[i] = 0.f;
    }
    if ((flags & TH_ADAM_COUNT_NONFINITE) && __ballot(bad != 0) != 0ull) {       // (rare: most waves never get here)
#pragma unroll
        for (int off = TH_WAVE / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off, TH_WAVE);
        if ((tid & (TH_WAVE - 1)) == 0) atomicAdd(nonfinite, (unsigned long long)bad);
    }
}

int th_adam_chunk_elems(void) { return TH_ADAM_CHUNK; }

size_t th_adam_table_bytes(int n_tensors, long long total_elems) {
    if (n_tensors < 1 || total_elems < 1) return 0;
    const long long nc = ad_max_chunks(n_tensors, total_elems);
    if (nc > 0x7fffffffLL) return 0;
    return ad_slot_off(n_tensors, total_elems) + th_align((size_t)n_tensors * sizeof(AdSlot));
}

static int ad_device_pointer(th_ctx* c, const void* ptr, const char* what, int i) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, ptr);
    if (e != hipSuccess) (void)hipGetLastError();
    TH_REQUIRE(e == hipSuccess && a.type == hipMemoryTypeDevice,
               std::string(what) + " of tensor " + std::to_string(i) + " is not a device pointer");
    TH_REQUIRE(a.device == c->device, std::string(what) + " of tensor " + std::to_string(i) + " lives on another device");
    return 0;
}

void th_adam_plan_destroy(th_adam_plan_t* pl) {
    if (!pl) return;
    // (copies of the current half of the ring have no event yet: drain the device before the pinned memory goes)
    if (pl->ctx && hipSetDevice(pl->ctx->device) == hipSuccess) (void)hipDeviceSynchronize();
    for (int h = 0; h < 2; ++h) {
        if (pl->half_ev[h]) {
            if (pl->half_pending[h]) (void)hipEventSynchronize(pl->half_ev[h]);
            (void)hipEventDestroy(pl->half_ev[h]);
        }
    }
    if (pl->pinned) (void)hipHostFree(pl->pinned);
    delete pl;
}

int th_adam_plan(th_ctx* c, int n_tensors, const long long* counts, const void* const* params, void* table, size_t table_bytes,
                 th_adam_plan_t** out, th_stream stream) {
    TH_REQUIRE(c && counts && table && out, "null argument");
    TH_REQUIRE(n_tensors >= 1 && n_tensors <= (1 << 20), "n_tensors is " + std::to_string(n_tensors) + ": 1 .. 2^20");
    long long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        TH_REQUIRE(counts[i] >= 1 && counts[i] <= (1LL << 40), "tensor " + std::to_string(i) + " has no elements");
        total += counts[i];
    }
    const size_t need = th_adam_table_bytes(n_tensors, total);
    TH_REQUIRE(need != 0 && table_bytes >= need, "table too small");
    TH_REQUIRE(((uintptr_t)table & 15) == 0, "table must be 16-byte aligned");
    TH_HIP(hipSetDevice(c->device));
    TH_TRY(ad_device_pointer(c, table, "the table", -1));
    if (params)
        for (int i = 0; i < n_tensors; ++i) TH_TRY(ad_device_pointer(c, params[i], "the parameter", i));
    hipStream_t s = (hipStream_t)stream;
    th_adam_plan_t* pl = new th_adam_plan_t();
    pl->ctx = c;
    pl->table = (char*)table;
    pl->n_tensors = n_tensors;
    pl->slot_bytes = th_align((size_t)n_tensors * sizeof(th_adam_tensor));
    pl->counts.assign(counts, counts + n_tensors);
    pl->slot_table_off = ad_slot_off(n_tensors, total);
    pl->slot_host.resize((size_t)n_tensors);
    auto fail = [&](int rc) { th_adam_plan_destroy(pl); return rc; };
    long long nc = 0;
    for (int i = 0; i < n_tensors; ++i) nc += (counts[i] + TH_ADAM_CHUNK - 1) / TH_ADAM_CHUNK;
    pl->n_chunks = (int)nc;                                                      // <= ad_max_chunks <= 2^31 - 1 (table_bytes != 0)
    const size_t chunk_bytes = (size_t)nc * sizeof(AdChunk);
    // the chunk table is staged in the ring's memory (nothing else uses it yet) and the stream is drained before the first step
    const size_t ring_bytes = th_adam_plan_t::kRing * pl->slot_bytes + 256;
    const size_t pin_bytes = ring_bytes > chunk_bytes ? ring_bytes : chunk_bytes;
    if (hipHostMalloc((void**)&pl->pinned, pin_bytes, hipHostMallocDefault) != hipSuccess) {
        pl->pinned = nullptr;
        (void)hipGetLastError();
        th_set_error("th_adam_plan: pinned staging allocation failed");
        return fail(-2);
    }
    AdChunk* hc = (AdChunk*)pl->pinned;
    long long k = 0;
    for (int i = 0; i < n_tensors; ++i)
        for (long long o = 0; o < counts[i]; o += TH_ADAM_CHUNK) {
            const long long left = counts[i] - o;
            hc[k].tensor = i;
            hc[k].count = (int32_t)(left < TH_ADAM_CHUNK ? left : TH_ADAM_CHUNK);
            hc[k].offset = o;
            ++k;
        }
    hipError_t e = hipMemsetAsync(table, 0, sizeof(AdHeader), s);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->table + ad_chunk_off(n_tensors), hc, chunk_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (int h = 0; h < 2 && e == hipSuccess; ++h) e = hipEventCreateWithFlags(&pl->half_ev[h], hipEventDisableTiming);
    if (e != hipSuccess) {
        th_set_error(std::string("th_adam_plan: ") + hipGetErrorString(e));
        return fail(-2);
    }
    *out = pl;
    return 0;
}

// Copies `bytes` of a per-call table from host memory (free for reuse on return) to `dst` on the device through the next
// staging buffer of the ring.  That buffer's previous copy was queued kRing calls ago; the event of its half of the ring was
// recorded behind the LAST copy of that half, so one wait at the half's first buffer covers all of them.  *last_of_half is the
// half whose event the caller records behind its kernel (ad_stage_done), or -1.
static int ad_stage(th_ctx* c, th_adam_plan_t* pl, const void* src, size_t bytes, void* dst, hipStream_t s, int* last_of_half) {
    const int slot = (int)(pl->gen % th_adam_plan_t::kRing), half = slot / (th_adam_plan_t::kRing / 2);
    const bool first = slot % (th_adam_plan_t::kRing / 2) == 0, last = (slot + 1) % (th_adam_plan_t::kRing / 2) == 0;
    if (first && pl->half_pending[half]) {
        ThWaitClock wc(c);
        TH_HIP(hipEventSynchronize(pl->half_ev[half]));
        pl->half_pending[half] = false;
    }
    // (a caller that changes streams inside a half: the event below would only cover the new stream's copies)
    if (!first && pl->half_stream[half] != s) TH_HIP(hipStreamSynchronize(pl->half_stream[half]));
    pl->half_stream[half] = s;
    char* stage = pl->pinned + (size_t)slot * pl->slot_bytes;
    memcpy(stage, src, bytes);
    ++pl->gen;
    TH_HIP(hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, s));
    *last_of_half = last ? half : -1;
    return 0;
}

static int ad_stage_done(th_adam_plan_t* pl, int last_of_half, hipStream_t s) {
    if (last_of_half >= 0) {
        TH_HIP(hipEventRecord(pl->half_ev[last_of_half], s));
        pl->half_pending[last_of_half] = true;
    }
    return 0;
}

int th_adam_step(th_ctx* c, th_adam_plan_t* pl, const th_adam_tensor* scalars, int n_tensors, float clip, int flags,
                 unsigned long long* nonfinite_out, th_stream stream) {
    TH_REQUIRE(c && pl && pl->ctx == c, "the plan belongs to another context");
    TH_REQUIRE((flags & ~(TH_ADAM_CLIP | TH_ADAM_ZERO_GRAD | TH_ADAM_COUNT_NONFINITE | TH_ADAM_CHECK_POINTERS)) == 0, "unknown flag");
    hipStream_t s = (hipStream_t)stream;
    if (n_tensors != 0) {
        int last_of_half = -1;
        TH_REQUIRE(scalars && n_tensors == pl->n_tensors,
                   "the plan holds " + std::to_string(pl->n_tensors) + " tensors, the step names " + std::to_string(n_tensors));
        TH_REQUIRE(!(flags & TH_ADAM_CLIP) || clip >= 0.f, "the clip value must be >= 0 (and not NaN)");
        for (int i = 0; i < n_tensors; ++i) {
            const th_adam_tensor& t = scalars[i];
            if (!t.p) continue;
            TH_REQUIRE(t.g && t.m && t.v, "tensor " + std::to_string(i) + " lacks a gradient or moment pointer");
            TH_REQUIRE((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3) == 0,
                       "tensor " + std::to_string(i) + " is not 4-byte aligned");
            if (flags & TH_ADAM_CHECK_POINTERS) {
                TH_TRY(ad_device_pointer(c, t.p, "the parameter", i));
                TH_TRY(ad_device_pointer(c, t.g, "the gradient", i));
                TH_TRY(ad_device_pointer(c, t.m, "exp_avg", i));
                TH_TRY(ad_device_pointer(c, t.v, "exp_avg_sq", i));
            }
        }
        TH_TRY(ad_stage(c, pl, scalars, (size_t)n_tensors * sizeof(th_adam_tensor), pl->table + ad_tensor_off(), s, &last_of_half));
        hipLaunchKernelGGL(adam_step_kernel, dim3(pl->n_chunks), dim3(AD_THREADS), 0, s,
                           (const th_adam_tensor*)(pl->table + ad_tensor_off()),
                           (const AdChunk*)(pl->table + ad_chunk_off(pl->n_tensors)), clip, flags,
                           (unsigned long long*)pl->table);
        TH_LAUNCH_CHECK();
        TH_TRY(ad_stage_done(pl, last_of_half, s));
    }
    if (nonfinite_out) {
        unsigned long long* word = (unsigned long long*)(pl->pinned + th_adam_plan_t::kRing * pl->slot_bytes);
        TH_HIP(hipMemcpyAsync(word, pl->table, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        ThWaitClock wc(c);
        TH_HIP(hipStreamSynchronize(s));
        *nonfinite_out = *word;
    }
    return 0;
}

// ---- the gradient exchange: every planned tensor into / out of one flat buffer ----
// The layout rule (train_dist.flat_layout restates it): slots in plan order, only for tensors whose byte in `live` is set (NULL:
// all), each starting at a multiple of 4 elements; the buffer ends at the last slot's end rounded up to 4.
long long ad_flat_layout(int n_tensors, const long long* counts, const uint8_t* live, long long* offsets_out) {
    long long end = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const bool has = !live || live[i];
        if (offsets_out) offsets_out[i] = has ? end : -1;
        if (has) end = (end + counts[i] + 3) & ~3LL;
    }
    return end;
}

// One workgroup per chunk of the plan.  src may BE dst (a gradient that already lives in its slot): every element is read and
// then written by the same lane, nothing else is read.  The lanes behind a tensor's last element write the slot's padding; a
// chunk that is not its tensor's last ends on a multiple of TH_ADAM_CHUNK and has none.
__global__ __launch_bounds__(AD_THREADS) void adam_pack_kernel(const AdSlot* __restrict__ slots, const AdChunk* __restrict__ chunks,
                                                               float* flat_, float world, int copy) {
    const AdChunk ch = chunks[blockIdx.x];
    const AdSlot sl = slots[ch.tensor];
    if (sl.off < 0) return;                                                       // no slot: not touched
    AdGlobalF* dst = (AdGlobalF*)(uintptr_t)flat_ + sl.off + ch.offset;
    const AdGlobalF* src = sl.ptr ? (const AdGlobalF*)(uintptr_t)sl.ptr + ch.offset : nullptr;
    const int n = ch.count, tid = threadIdx.x;
    const bool aligned = ((((uintptr_t)flat_) | ((uintptr_t)sl.ptr)) & 15) == 0;  // (slot and chunk offsets are multiples of 4)
    int done = 0;
    if (aligned) {
        AdGlobalF4* d4 = (AdGlobalF4*)dst;
        const AdGlobalF4* s4 = (const AdGlobalF4*)src;
        const AdF4 z4 = {0.f, 0.f, 0.f, 0.f};
        if (n == TH_ADAM_CHUNK && src) {
            AdF4 G[AD_VEC];
#pragma unroll
            for (int r = 0; r < AD_VEC; ++r) G[r] = s4[r * AD_THREADS + tid];    // every load of the chunk in flight at once
#pragma unroll
            for (int r = 0; r < AD_VEC; ++r) {
                if (!copy) G[r] = G[r] / world;                                  // (correctly rounded, element by element)
                d4[r * AD_THREADS + tid] = G[r];
            }
            done = n;
        } else {
            const int n4 = n >> 2;
            for (int i = tid; i < n4; i += AD_THREADS) {
                AdF4 G = src ? s4[i] : z4;
                if (!copy) G = G / world;
                d4[i] = G;
            }
            done = n4 << 2;
        }
    }
    for (int i = done + tid; i < n; i += AD_THREADS) {                           // tail, or a tensor off the 16-byte grid
        float G = src ? src[i] : 0.f;
        if (!copy) G = G / world;
        dst[i] = G;
    }
    const int padded = (n + 3) & ~3;
    if (tid < padded - n) dst[n + tid] = 0.f;
}

__global__ __launch_bounds__(AD_THREADS) void adam_unpack_kernel(const AdSlot* __restrict__ slots, const AdChunk* __restrict__ chunks,
                                                                 const float* __restrict__ flat_) {
    const AdChunk ch = chunks[blockIdx.x];
    const AdSlot sl = slots[ch.tensor];
    if (sl.off < 0 || sl.ptr == nullptr) return;
    const AdGlobalF* __restrict__ src = (const AdGlobalF*)(uintptr_t)flat_ + sl.off + ch.offset;
    AdGlobalF* __restrict__ dst = (AdGlobalF*)(uintptr_t)sl.ptr + ch.offset;
    const int n = ch.count, tid = threadIdx.x;
    const bool aligned = ((((uintptr_t)flat_) | ((uintptr_t)sl.ptr)) & 15) == 0;
    int done = 0;
    if (aligned) {
        const AdGlobalF4* s4 = (const AdGlobalF4*)src;
        AdGlobalF4* d4 = (AdGlobalF4*)dst;
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += AD_THREADS) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += AD_THREADS) dst[i] = src[i];
}

// the checks and the launch shared by th_adam_pack / th_adam_unpack (th_api.hip); ptrs[i] NULL: zeros (pack only)
int th_adam_flat_launch(th_ctx* c, th_adam_plan_t* pl, int unpack, const void* const* ptrs, const long long* offsets, int n_tensors,
                        int world, float* flat, long long flat_elems, hipStream_t s) {
    TH_REQUIRE(c && pl && pl->ctx == c, "the plan belongs to another context");
    TH_REQUIRE(ptrs && offsets && flat, "null argument");
    TH_REQUIRE(n_tensors == pl->n_tensors,
               "the plan holds " + std::to_string(pl->n_tensors) + " tensors, the call names " + std::to_string(n_tensors));
    TH_REQUIRE(world >= 1 && world <= (1 << 20), "world is " + std::to_string(world) + ": 1 .. 2^20");
    TH_REQUIRE(((uintptr_t)flat & 3) == 0, "the flat buffer is not 4-byte aligned");
    // the offsets must BE the layout rule's: then every slot lies inside [0, flat_elems) and the slots with their padding tile it
    long long end = 0;
    std::vector<AdSlot>& slots = pl->slot_host;
    for (int i = 0; i < n_tensors; ++i) {
        if (offsets[i] >= 0) {
            TH_REQUIRE(offsets[i] == end, "the slot of tensor " + std::to_string(i) + " starts at " + std::to_string(offsets[i]) +
                                              ", the layout rule puts it at " + std::to_string(end));
            end = (end + pl->counts[i] + 3) & ~3LL;
            TH_REQUIRE(!unpack || ptrs[i], "tensor " + std::to_string(i) + " has a slot and no destination");
            TH_REQUIRE(((uintptr_t)ptrs[i] & 3) == 0, "tensor " + std::to_string(i) + " is not 4-byte aligned");
        }
        slots[i].ptr = offsets[i] >= 0 ? const_cast<void*>(ptrs[i]) : nullptr;
        slots[i].off = offsets[i] >= 0 ? offsets[i] : -1;
    }
    TH_REQUIRE(end == flat_elems, "flat_elems is " + std::to_string(flat_elems) + ", the layout ends at " + std::to_string(end));
    if (end == 0) return 0;
    TH_HIP(hipSetDevice(c->device));
    if (pl->checked_flat != (const void*)flat || pl->checked_elems != flat_elems) {   // asked of the runtime when the buffer is new
        TH_TRY(ad_device_pointer(c, flat, "the flat buffer", -1));
        hipDeviceptr_t base = nullptr;                                           // (the whole buffer, not just its first byte)
        size_t size = 0;
        const hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)flat);
        if (e != hipSuccess) (void)hipGetLastError();
        TH_REQUIRE(e == hipSuccess && (const char*)flat + (size_t)flat_elems * 4 <= (const char*)base + size,
                   "the flat buffer's allocation holds fewer than flat_elems elements");
        pl->checked_flat = flat;
        pl->checked_elems = flat_elems;
    }
    int last_of_half = -1;
    AdSlot* dev_slots = (AdSlot*)(pl->table + pl->slot_table_off);
    TH_TRY(ad_stage(c, pl, slots.data(), (size_t)n_tensors * sizeof(AdSlot), dev_slots, s, &last_of_half));
    const AdChunk* chunks = (const AdChunk*)(pl->table + ad_chunk_off(pl->n_tensors));
    if (unpack)
        hipLaunchKernelGGL(adam_unpack_kernel, dim3(pl->n_chunks), dim3(AD_THREADS), 0, s, (const AdSlot*)dev_slots, chunks,
                           (const float*)flat);
    else
        hipLaunchKernelGGL(adam_pack_kernel, dim3(pl->n_chunks), dim3(AD_THREADS), 0, s, (const AdSlot*)dev_slots, chunks, flat,
                           (float)world, world == 1 ? 1 : 0);
    TH_LAUNCH_CHECK();
    return ad_stage_done(pl, last_of_half, s);
}

// ---- K28: the rank-ordered sum of the exchange's reduce-scatter ----
// parts [world][slice_elems] holds slice r of every rank's flat buffer, as all_to_all_single delivers it to rank r:
//   out[e] = ((parts[0][e] + parts[1][e]) + parts[2][e]) + ...      fp32, one rounding per addition, in rank order
// which is grad_exchange_oracle's sum for any world, whatever order a collective would take.  One lane owns an element (a group
// of four on the 128-bit path): it reads the element of every part and then writes it, so `out` may BE any of the parts.  No
// atomics, no LDS; subnormals are kept (the library's default), NaN, +-inf and -0.0 are the adder's; world == 1 copies the bits.
// The 128-bit path needs parts and out on the 16-byte grid and slice_elems a multiple of 4 (every part then starts on the grid).
template <typename T, typename G>
__global__ __launch_bounds__(AD_THREADS) void rank_sum_kernel(const float* parts_, int world, long long stride, long long n,
                                                               float* out_) {
    const long long i = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (i >= n) return;
    const G* parts = (const G*)(uintptr_t)parts_ + i;                             // (stride and n count T's)
    T acc = parts[0];
    int r = 1;
    for (; r + 4 <= world; r += 4) {                                              // four loads in flight, added in rank order
        const T a = parts[(long long)r * stride], b = parts[(long long)(r + 1) * stride], c = parts[(long long)(r + 2) * stride],
                d = parts[(long long)(r + 3) * stride];
        acc = acc + a;
        acc = acc + b;
        acc = acc + c;
        acc = acc + d;
    }
    for (; r < world; ++r) acc = acc + parts[(long long)r * stride];
    ((G*)(uintptr_t)out_)[i] = acc;
}

int th_rank_sum_launch(const float* parts, int world, long long slice_elems, float* out, hipStream_t s) {
    TH_REQUIRE(parts && out, "null argument");
    TH_REQUIRE(world >= 1 && world <= 64, "world is " + std::to_string(world) + ": 1 .. 64");
    TH_REQUIRE(slice_elems >= 1 && slice_elems <= (1LL << 36), "slice_elems is " + std::to_string(slice_elems) + ": 1 .. 2^36");
    TH_REQUIRE(((((uintptr_t)parts) | ((uintptr_t)out)) & 3) == 0, "parts and out must be 4-byte aligned");
    const bool wide = ((((uintptr_t)parts) | ((uintptr_t)out)) & 15) == 0 && slice_elems % 4 == 0;
    if (wide) {
        const long long n4 = slice_elems / 4;
        hipLaunchKernelGGL((rank_sum_kernel<AdF4, AdGlobalF4>), dim3((unsigned)((n4 + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS),
                           0, s, parts, world, n4, n4, out);
    } else {
        hipLaunchKernelGGL((rank_sum_kernel<float, AdGlobalF>), dim3((unsigned)((slice_elems + AD_THREADS - 1) / AD_THREADS)),
                           dim3(AD_THREADS), 0, s, parts, world, slice_elems, slice_elems, out);
    }
    TH_LAUNCH_CHECK();
    return 0;
}
