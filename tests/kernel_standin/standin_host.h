// What the operator headers of fastspeech2_amd/csrc expect of their includer (fs2_runtime.hip) besides HIP itself, for the stand-in
// mains beside this file: include/fs2.h, fail() and align_up().  A refusal prints its format to stderr and returns its code; the
// mains report the codes.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include "hip_standin.h"
#include "fs2.h"
inline int fail(void*, int code, const char* fmt, ...) { fprintf(stderr, "fail: %s\n", fmt); return code; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
