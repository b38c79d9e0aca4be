// Per-stream slot state as csrc/realtime.hip, csrc/aec.hip, csrc/resample_stream.hip and csrc/highband.hip lay it out: a header, then
// one 256-byte-aligned record per slot, all in one caller-owned allocation.  Here, once: the alignment, the checks every entry point
// starts with, the reset (one kernel, csrc/slot_state.hip) and the geometry header that the canceller's and the converters' kernels
// compare against.
#pragma once
#include "common.h"

#define SLOT_MAX_STREAMS (1 << 20)
#define SLOT_GEOM_HDR_BYTES 256        // a geometry header: up to eight ints (what _init was given), zeros behind them

constexpr long long slot_al(long long x) { return (x + 255) / 256 * 256; }

// The checks of a state argument, in one order for every module: null, max_streams, the module's own parameters (params(): NELE_OK, or
// the status it set), the size against the module's *_state_bytes (need; bytes_fn and arg2 name that call in the message - arg2 < 0: it
// takes max_streams alone), the alignment.
template <class Params>
int slot_state_check(const char* name, const void* state, long long state_bytes, int S, Params params, long long need, const char* bytes_fn,
                     int arg2 = -1) {
    NELE_CHECK_ARG(state, "%s: null state", name);
    NELE_CHECK_ARG(S > 0 && S <= SLOT_MAX_STREAMS, "%s: max_streams=%d must be in 1 .. 1048576", name, S);
    if (int st = params()) return st;
    if (arg2 < 0)
        NELE_CHECK_ARG(state_bytes >= need, "%s: state of %lld bytes is smaller than %s(%d) = %lld", name, state_bytes, bytes_fn, S, need);
    else
        NELE_CHECK_ARG(state_bytes >= need, "%s: state of %lld bytes is smaller than %s(%d, %d) = %lld", name, state_bytes, bytes_fn, S, arg2, need);
    NELE_CHECK_ARG(((size_t)state % 256) == 0, "%s: state must be 256-byte aligned", name);
    return NELE_OK;
}

// csrc/slot_state.hip: zero the records (rec_bytes each, a multiple of 256, behind hdr_bytes) of the slots with slots[b] != 0 (null: all
// S); nhdr in 1 .. 8: also write the geometry header hdr[0 .. nhdr) at the start of the state, zeros up to SLOT_GEOM_HDR_BYTES.
// first: the value of a reset record's first int (the scheduled converter's lead; every other module's records start with a zero).
__attribute__((visibility("hidden"))) int slot_state_reset(const char* name, void* state, long long hdr_bytes, long long rec_bytes, int S,
                                                           const unsigned char* slots, int nhdr, const int* hdr, void* stream, int first = 0);

// is this the state _init laid out for these parameters?  (a kernel that finds it is not touches nothing)
__device__ __forceinline__ bool slot_hdr_matches(const unsigned char* state, int v0, int v1) {
    const int* hdr = reinterpret_cast<const int*>(state);
    return hdr[0] == v0 && hdr[1] == v1;
}
__device__ __forceinline__ bool slot_hdr_matches(const unsigned char* state, int v0, int v1, int v2, int v3) {
    const int* hdr = reinterpret_cast<const int*>(state);
    return hdr[0] == v0 && hdr[1] == v1 && hdr[2] == v2 && hdr[3] == v3;
}
__device__ __forceinline__ bool slot_hdr_matches(const unsigned char* state, int v0, int v1, int v2, int v3, int v4, int v5) {
    const int* hdr = reinterpret_cast<const int*>(state);
    return slot_hdr_matches(state, v0, v1, v2, v3) && hdr[4] == v4 && hdr[5] == v5;
}
__device__ __forceinline__ bool slot_hdr_matches(const unsigned char* state, int v0, int v1, int v2, int v3, int v4, int v5, int v6) {
    const int* hdr = reinterpret_cast<const int*>(state);
    return slot_hdr_matches(state, v0, v1, v2, v3) && hdr[4] == v4 && hdr[5] == v5 && hdr[6] == v6;
}
