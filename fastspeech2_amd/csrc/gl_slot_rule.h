// Slot -> tile rule of the device-driven Griffin-Lim planner (griffin_lim.h: gl_plan_scan / gl_plan_emit).
// The grids of a device-driven call are sized from host-known capacities: gl_slot_capacity slots, one workgroup each.  The planner
// gives slot s the s-th tile of the batch (utterances in batch order, each one's tiles f0 = 0, F, 2F, ..; utterances with L < 2 own
// no sample and get no tile) or, past the last tile, an empty record.  Plain C++ with no HIP dependency, like gl_tile_rule.h:
// tests/test_vocoder_async_host.py compiles it on the host and compares it with fastspeech2_amd/vocoder.py: slot_tiles.
#pragma once
#include <stdint.h>

#include "gl_tile_rule.h"

namespace fs2 {

// tiles of an utterance of L frames (the host plan's rule, griffin_lim_host.h: gl_plan)
GL_HD constexpr int gl_tile_count(int L, int F) { return L >= 2 ? (L + F - 1) / F : 0; }

// slots that hold the tiles of ANY batch of B utterances with sum L <= frame_capacity: ceil(L / F) <= L / F + (F - 1) / F, so
// sum ceil(L_b / F) <= (sum L_b + B (F - 1)) / F < frame_capacity / F + B
GL_HD constexpr int64_t gl_slot_capacity(int64_t frame_capacity, int F, int B) { return frame_capacity / F + B; }

struct GlSlot {
    int b;      // utterance, or -1: no tile (an empty record)
    int f0;     // first frame of the tile, utterance-local
};

// tile_end[b] = tiles of utterances 0 .. b (inclusive prefix sum of gl_tile_count, non-decreasing).  The slot's utterance is the
// first b with tile_end[b] > slot (binary search: utterances without tiles are skipped by the strict comparison).
GL_HD inline GlSlot gl_slot_tile(const int* tile_end, int B, int F, int slot) {
    int lo = 0, hi = B;                       // invariant: tile_end[i] <= slot for i < lo, tile_end[i] > slot for i >= hi
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (tile_end[mid] > slot) hi = mid; else lo = mid + 1;
    }
    GlSlot r;
    if (lo >= B) { r.b = -1; r.f0 = 0; return r; }
    r.b = lo;
    r.f0 = (slot - (lo ? tile_end[lo - 1] : 0)) * F;
    return r;
}

}  // namespace fs2
