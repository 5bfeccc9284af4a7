// Stand-alone check of transhuman_amd/csrc/th_arena.h (tests/test_workspace_sizes.py compiles and runs it; no HIP, no GPU).
// For every take sequence: measuring gives the bytes a carve consumes, a carve into exactly that many bytes fits and hands out
// in-bounds, 256-byte-spaced pieces, and a carve into one byte fewer does not fit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "th_arena.h"

struct Take { int elem; size_t count; };          // elem: sizeof of the element type (1, 2, 4, 8, 16)
struct Elem16 { uint64_t a, b; };

static char* take_one(ThArena& ar, const Take& t) {
    switch (t.elem) {
        case 1: return (char*)ar.take<uint8_t>(t.count);
        case 2: return (char*)ar.take<uint16_t>(t.count);
        case 4: return (char*)ar.take<float>(t.count);
        case 8: return (char*)ar.take<double>(t.count);
        default: return (char*)ar.take<Elem16>(t.count);
    }
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL sequence %d: ", seq_no); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_sequence(int seq_no, const std::vector<Take>& seq) {
    size_t want = 0;                                              // the rule, restated: every piece rounded up to 256 bytes
    for (const Take& t : seq) want += (t.count * t.elem + 255) / 256 * 256;
    const size_t n = th_measure([&](ThArena& ar) {
        for (const Take& t : seq) CHECK(take_one(ar, t) == nullptr, "a measuring take returned a pointer");
        CHECK(ar.ok(), "a measuring arena reported a misfit");
    });
    CHECK(n == want, "measured %zu bytes, the pieces add up to %zu", n, want);
    // exactly n bytes: fits; every piece lies inside, and is written end to end (a sanitizer build sees any overrun)
    char* buf = (char*)malloc(n ? n : 1);
    {
        ThArena ar(buf, n);
        size_t at = 0;
        for (const Take& t : seq) {
            char* p = take_one(ar, t);
            const size_t bytes = t.count * t.elem;
            CHECK(p == buf + at, "piece at offset %td, expected %zu", p - buf, at);
            if (p) memset(p, 0x5a, bytes);
            at += (bytes + 255) / 256 * 256;
        }
        CHECK(ar.ok(), "a carve into the measured %zu bytes did not fit", n);
        CHECK(ar.used() == n, "a carve used %zu of the measured %zu bytes", ar.used(), n);
    }
    free(buf);
    // one byte fewer: does not fit, the flag stays set, and no piece handed out passes the end
    if (n > 0) {
        char* small = (char*)malloc(n - 1 ? n - 1 : 1);
        ThArena ar(small, n - 1);
        for (const Take& t : seq) {
            char* p = take_one(ar, t);
            if (p) CHECK((size_t)(p - small) + (t.count * t.elem + 255) / 256 * 256 <= n - 1, "a piece passes the short buffer's end");
        }
        CHECK(!ar.ok(), "a carve into %zu bytes (one fewer than measured) fitted", n - 1);
        CHECK(ar.used() <= n - 1, "a short carve used %zu of %zu bytes", ar.used(), n - 1);
        free(small);
    }
}

int main() {
    std::vector<std::vector<Take>> seqs = {
        {{1, 1}},                                        // one byte -> 256
        {{1, 0}},                                        // nothing at all
        {{4, 0}, {8, 0}, {1, 0}},                        // zero-length takes only
        {{1, 256}},                                      // exact multiples need no padding
        {{1, 257}},                                      // one byte over
        {{4, 64}, {4, 65}, {4, 63}},
        {{8, 0}, {4, 33}, {1, 0}, {2, 50}, {16, 0}},     // zero-length takes between padded ones
        {{1, 17 * 19}, {4, 33 * 50}, {8, 207}, {2, 3 * 333 * 64}},
        {{16, 1}, {16, 16}, {16, 17}},
        {{1, 255}, {1, 1}, {1, 255}, {1, 1}},
        {{4, 6890 * 3}, {4, 4097}, {8, 24 * 16}, {4, 24 * 9}},
        {{1, 1 << 20}, {4, (1 << 18) + 1}, {1, 0}},
    };
    uint64_t r = 0x9E3779B97F4A7C15ull;                 // a fixed pseudo-random tail: lengths 1 .. 12, counts with and without padding
    auto next = [&]() { r = r * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(r >> 33); };
    const int elems[5] = {1, 2, 4, 8, 16};
    for (int i = 0; i < 36; ++i) {
        std::vector<Take> s;
        const int len = 1 + next() % 12;
        for (int k = 0; k < len; ++k) {
            const uint32_t pick = next() % 8;
            const size_t count = pick == 0 ? 0 : pick == 1 ? 64 * (1 + next() % 9) : next() % 5000;
            s.push_back({elems[next() % 5], count});
        }
        seqs.push_back(s);
    }
    int no = 0;
    for (const auto& s : seqs) check_sequence(no++, s);
    printf("%d take sequences, %d failures\n", no, g_fail);
    return g_fail ? 1 : 0;
}
