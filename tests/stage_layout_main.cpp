// Stand-alone host program (tests/test_stage_layout_host.py builds it with the address sanitizer): the HOST staging
// layout of csrc/tpc_mpc_stage.h for the tables the compact entries build, walked as stage_in / stage_out walk it over a
// heap buffer of exactly the bytes stage_layout asks for.  No HIP call: every row the copies would touch is written
// here with memset, so a slot too small or an overlap is the sanitizer's to find; the rest is checked by hand.
#include "../trajectory_controller_amd/csrc/tpc_mpc_stage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace tpc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static int64_t pad(int64_t b) { return (b + 255) / 256 * 256; }

// what stage_in and stage_out do to the buffer, and what must hold of the offsets
static void walk(std::vector<StagedArray> t, int64_t n) {
    static char there;
    for (auto& a : t)
        if (a.ptr) a.ptr = &there;
    const int64_t total = stage_layout(t.data(), (int)t.size(), n);
    CHECK(total % 256 == 0);
    char* buf = (char*)std::malloc(total ? (size_t)total : 1);
    int64_t end = 0;
    for (const auto& a : t) {
        if (!a.ptr) continue;
        CHECK(a.off % 256 == 0);
        CHECK(a.off >= end);   // in the table's order, no overlap
        CHECK(stage_elems(a, n) <= stage_pitch(a, n));
        for (int64_t r = 0; r < a.rows; ++r)
            std::memset(buf + a.off + r * stage_pitch(a, n) * a.width, 0xAB, (size_t)(stage_elems(a, n) * a.width));
        // a kernel may touch a per-instance row up to the wavefront's end
        std::memset(buf + a.off, 0xCD, (size_t)(a.rows * stage_pitch(a, n) * a.width));
        end = a.off + pad(a.rows * stage_pitch(a, n) * a.width);
    }
    CHECK(end == total);   // an absent array takes no bytes
    std::free(buf);
}

int main() {
    static char x;
    const int64_t ns[] = {1, 63, 64, 65, 130, 4097};
    for (int64_t n : ns) {
        CHECK(stage_ld(n) >= n && stage_ld(n) % 64 == 0 && stage_ld(n) - n < 64);
        // tpc_mpc_solve_batch_compact: fp64 and fp32, with and without iters; never below the hand-laid layout it
        // replaces, and at most one wavefront's padding per slot above it
        for (int es : {8, 4})
            for (int iters = 0; iters < 2; ++iters) {
                std::vector<StagedArray> t = {staged(&x, kStageIn, 1, n, es), staged(&x, kStageIn, 1, n, es),
                                              staged(&x, kStageIn, 1, n, es), staged(&x, kStageOut, 1, n, es),
                                              staged(&x, kStageOut, 1, n, es), staged(iters ? &x : nullptr, kStageOut, 1, n, 4)};
                const int64_t total = stage_layout(t.data(), 6, n), was = 5 * pad(n * es) + (iters ? pad(n * 4) : 0);
                CHECK(total >= was && total <= was + 6 * 256);
                walk(t, n);
            }
        // the exact solve (H = 7): every subset of params_rows, start and the five optional outputs
        for (int H : {4, 7})
            for (int m = 0; m < 128; ++m) {
                auto on = [&](int bit) -> const void* { return (m >> bit) & 1 ? &x : nullptr; };
                walk({staged(&x, kStageIn, 1, n), staged(&x, kStageIn, 1, n), staged(&x, kStageIn, 1, n),
                      staged(on(0), kStageIn, 10, n), staged(on(1), kStageIn, 2 * H, n), staged(&x, kStageOut, 1, n),
                      staged(&x, kStageOut, 1, n), staged(on(2), kStageOut, 2 * H, n), staged(on(3), kStageOut, 1, n),
                      staged(on(4), kStageOut, 1, n), staged(on(5), kStageOut, 1, n, 4), staged(on(6), kStageOut, 1, n, 4)},
                     n);
            }
        // the backward pass: dparams is one row of ten sums, whatever n is
        for (int m = 0; m < 64; ++m) {
            auto on = [&](int bit) -> const void* { return (m >> bit) & 1 ? &x : nullptr; };
            std::vector<StagedArray> t = {staged(on(0), kStageIn, 10, n), staged(&x, kStageIn, 14, n),
                                          staged(on(1), kStageIn, 1, n, 4), staged(on(2), kStageOut, 10, n),
                                          staged(on(3), kStageOut, 1, n), staged(on(4), kStageOut, 1, n, 8, 10)};
            walk(t, n);
            stage_layout(t.data(), 6, n);
            if (on(4)) CHECK(stage_elems(t[5], n) == 10 && stage_pitch(t[5], n) == 10);
        }
    }
    // a table with nothing in it
    StagedArray none = staged(nullptr, kStageIn, 5, 7);
    CHECK(stage_layout(&none, 1, 7) == 0 && none.dev == nullptr);
    if (failures) return 1;
    std::printf("stage layout ok\n");
    return 0;
}
