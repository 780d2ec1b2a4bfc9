// The table behind every HOST-memory call's staging (tpc_mpc_api.cpp: stage_in / stage_out): one StagedArray per array
// of the call, a slot for each array that is there.  Plain arithmetic on the table, no HIP: the layout is what a
// stand-alone host program can check (tests/stage_layout_main.cpp).
#pragma once

#include <cstdint>

namespace tpc {

enum StageRole : int { kStageIn = 1, kStageOut = 2, kStageInOut = kStageIn | kStageOut };

struct StagedArray {
    const void* ptr;   // the caller's array; null: not there -- no slot, no copy
    int64_t rows;      // component rows
    int64_t ld;        // the caller's leading dimension, in elements
    int width;         // bytes per element
    int role;          // StageRole: copied in, copied back, or both
    int64_t elems;     // elements per row where that is not the batch's n (0: n): a row that is not per instance
    int64_t off;       // stage_layout: the slot's offset
    void* dev;         // what the kernels take: the caller's array, or after stage_in the slot
};

inline StagedArray staged(const void* ptr, int role, int64_t rows, int64_t ld, int width = 8, int64_t elems = 0) {
    return StagedArray{ptr, rows, ld, width, role, elems, 0, const_cast<void*>(ptr)};
}

// leading dimension of the per-instance slots: n rounded up to a wavefront
inline int64_t stage_ld(int64_t n) { return (n + 63) / 64 * 64; }
// elements copied per row of a, and the distance between its rows in the slot
inline int64_t stage_elems(const StagedArray& a, int64_t n) { return a.elems ? a.elems : n; }
inline int64_t stage_pitch(const StagedArray& a, int64_t n) { return a.elems ? a.elems : stage_ld(n); }

// Gives every array of t[0..count) that is there a 256-byte padded slot, in the table's order: the bytes the buffer
// needs.  The one place that lays HOST staging out.
inline int64_t stage_layout(StagedArray* t, int count, int64_t n) {
    int64_t total = 0;
    for (int c = 0; c < count; ++c) {
        t[c].off = total;
        if (t[c].ptr) total += (t[c].rows * stage_pitch(t[c], n) * t[c].width + 255) / 256 * 256;
    }
    return total;
}

}  // namespace tpc
