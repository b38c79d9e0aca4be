// What csrc/estoi.hip (the batch ESTOI) and csrc/monitor.hip (the running one) both read, once: the frame geometry, the third-octave
// band edges, the frame window and the taps of the 16 -> 10 kHz resampling filter.
#pragma once
#include "common.h"

#define ES_NFRAME 256
#define ES_HOP 128
#define ES_NB 15
#define ES_NSEG 30
#define ES_HALF 290   // half length of the resampling filter
#define ES_EPS 2.220446049250313e-16

// pystoi thirdoct(10000, 512, 15, 150): bins [lo, hi) nearest to the band edges (checked against oracle/estoi.py)
static __constant__ int c_tob_lo[ES_NB] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
static __constant__ int c_tob_hi[ES_NB] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__device__ __forceinline__ double hann_sym256(int j) { return 0.5 - 0.5 * cospi(2.0 * (double)(j + 1) / 257.0); }

__device__ __forceinline__ double bessel_i0(double x) {
    // power series, converges quickly for the beta used here (5.65)
    double s = 1.0, t = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 60; ++k) {
        t *= q / ((double)k * (double)k);
        s += t;
        if (t < 1e-20 * s) break;
    }
    return s;
}

// filter taps: 5 * kaiser(581, beta) * sinc-lowpass, normalised to unit DC gain before the *5.  Every thread of a workgroup of 1024
// (>= 581) calls this with its own t = threadIdx.x; -> tap t (0 for t >= 581).  red: 16 doubles of LDS.
__device__ __forceinline__ double es_filter_tap(int t, double* red) {
    const int Lh = ES_HALF, n = 2 * Lh + 1;
    const double beta = 0.1102 * (60.0 - 8.7);
    const double fc = 1.0 / 16.0;
    double v = 0.0;
    if (t < n) {
        const double tt = (double)(t - Lh);
        const double arg = 2.0 * fc * tt;
        const double sinc = (t == Lh) ? 1.0 : sinpi(arg) / (M_PI * arg);
        const double ideal = 2.0 * 5.0 * fc * sinc;
        const double r = 2.0 * (double)t / (double)(n - 1) - 1.0;
        const double kais = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / bessel_i0(beta);
        v = kais * ideal;
    }
    const double tot = block_sum(v, red);
    return (t < n) ? 5.0 * v / tot : 0.0;
}
