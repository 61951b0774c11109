// One more construct for the host stand-in (hip_standin.h stays as it is): the shuffle of a whole record to the next lane in ONE
// exchange.  csrc/dtw.h moves a cell's record (seven fields) up one lane per step of its sweep; through hip_standin.h's __shfl_up that
// is fourteen waits at a wave's barrier per step, and the sweep of the edge batch has some 4,000 steps -- minutes of futex traffic on
// a small machine.  Here the record is written to one of two exchange buffers, the wave meets once, and the neighbour's copy is read:
// the buffers alternate from call to call, and a lane can only reach the call after the next by passing the next call's barrier, which
// every lane reaches after its read of this one.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <type_traits>
#include "hip_standin.h"
alignas(16) inline unsigned char g_record[2][4][64][64];
inline thread_local unsigned g_record_calls;
template <typename T> T standin_shfl_up_record(const T& v) {
    static_assert(sizeof(T) <= 64 && std::is_trivially_copyable_v<T>, "a record of at most 64 bytes");
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const unsigned half = g_record_calls++ & 1;
    std::memcpy(g_record[half][w][l], &v, sizeof(T));
    g_wave_bar[w]->arrive_and_wait();
    T r;
    std::memcpy(&r, g_record[half][w][l > 0 ? l - 1 : l], sizeof(T));
    return r;
}
#define FS2_STANDIN_SHFL_UP_RECORD(v) standin_shfl_up_record(v)
