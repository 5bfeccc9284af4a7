// Bump allocator over a caller-supplied workspace, and the same walk without a buffer to size one (plain C++, no HIP).
// A workspace has ONE statement of its layout: a function (ThArena&, shape...) that takes its pieces in order and returns the
// pointers.  The size function runs it on a measuring arena (th_measure), the launcher on a carving one and asks ok() once.
#pragma once
#include <stddef.h>

static inline size_t th_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct ThArena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool measuring = true, fits = true;
    ThArena() {}                                                                 // measure: no buffer, take() only adds up
    ThArena(void* p, size_t n) : base((char*)p), cap(n), measuring(false) {}     // carve n bytes at p
    // `count` elements, rounded up to 256 bytes.  Measuring: null.  Carving: null, and ok() false from then on, past the capacity.
    template <typename T>
    T* take(size_t count) {
        const size_t bytes = th_align(count * sizeof(T));
        if (!measuring && bytes > cap - off) fits = false;
        if (measuring || bytes > cap - off) {
            if (measuring) off += bytes;
            return nullptr;
        }
        off += bytes;
        return (T*)(base + off - bytes);
    }
    bool ok() const { return fits; }
    size_t used() const { return off; }
};

// bytes a layout takes: layout(ThArena&, shape...) run once on a measuring arena
template <typename F, typename... A>
static inline size_t th_measure(F layout, A... shape) {
    ThArena ar;
    layout(ar, shape...);
    return ar.used();
}
