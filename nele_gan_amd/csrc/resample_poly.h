// What the offline resampler (csrc/resample.hip) and the stream converter (csrc/resample_stream.hip) share, once: the limits, the
// filter's geometry and the inner product.  The stream converter promises the offline resampler's bits; it keeps
// that promise by running this code, not a copy of it.  Span staging stays with each kernel: the offline one stages zeros outside the
// row, the stream one the slot's history in front of the row.
#pragma once
#include "common.h"

#define RS_TILE 256                    // outputs per workgroup = threads per workgroup
#define RS_TAB_LDS_BYTES 16384         // tables up to this size are staged in LDS beside the input span (a stream converter takes no other)
#define RS_MAX_RATIO 16
#define RS_MAX_FACTOR 1024
#define RS_MAX_ZEROS 64

static inline int rs_half(int up, int down, int zeros) { return zeros * (up > down ? up : down); }
static inline int rs_K(int up, int half) { return (2 * half + 1 + up - 1) / up; }

// input samples a tile can touch: q_last - q_first <= floor((RS_TILE - 1) down / up) + 1, and K - 1 more in front of q_first.
// At the extreme allowed ratio (down = 16 up, zeros = 64: K = 2049) 255 * 16 + 2049 + 1 = 6130 doubles = 49040 bytes; with the largest
// LDS table 65424 bytes - inside the 64 KiB a launch gets without an attribute.
__host__ __device__ static inline int rs_span(int up, int down, int K) { return (int)(((long long)(RS_TILE - 1) * down) / up) + K + 1; }

// the zeros in 1 .. RS_MAX_ZEROS whose table width is K (0: none)
static inline int rs_zeros_of(int up, int down, int K) {
    for (int z = 1; z <= RS_MAX_ZEROS; ++z)
        if (rs_K(up, rs_half(up, down, z)) == K) return z;
    return 0;
}

static inline int rs_check_ratio(const char* name, int up, int down) {
    NELE_CHECK_ARG(up >= 1 && up <= RS_MAX_FACTOR && down >= 1 && down <= RS_MAX_FACTOR, "%s: up=%d or down=%d outside 1 .. %d", name, up, down,
                   RS_MAX_FACTOR);
    NELE_CHECK_ARG(down <= RS_MAX_RATIO * up && up <= RS_MAX_RATIO * down, "%s: up=%d / down=%d outside 1/%d .. %d", name, up, down, RS_MAX_RATIO,
                   RS_MAX_RATIO);
    return NELE_OK;
}

// sum_{k < K} hrow[k] xq[-k]: float64, k ascending, one fma per term - the order both kernels' bits are defined by
__device__ __forceinline__ double rs_dot(const double* __restrict__ hrow, const double* __restrict__ xq, int K) {
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) acc = fma(hrow[k], xq[-k], acc);
    return acc;
}
