// Band and spectrum arithmetic of the feature front end, defined once for features.hip (offline) and realtime.hip (hop by hop).
// Every float32 / float64 operation follows numpy's order (audio_util.py), so the including file is compiled with -ffp-contract=off
// (Makefile EXACT).  The band edge table is a per-translation-unit constant: no symbol crosses object files.
#pragma once
#include "common.h"

static __constant__ int c_gmt[NELE_NBANDS] = {0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
                                               24, 25, 26, 28, 30, 32, 34, 36, 38, 41, 43, 46, 49, 52, 55, 58, 62, 66, 70, 74,
                                               79, 83, 88, 93, 99, 105, 111, 117, 124, 131, 139, 147, 156, 165, 174, 184, 195,
                                               206, 218, 230, 243, 257};

// Band energy of band i from tmp[257] (= |X|^2, float32), in the accumulation order of
// compute_band_E (audio_util.py:40-48): first the "frac" shares of band i-1's bins, then the
// "1-frac" shares of band i's own bins; float32 products, float64 running sum.
__device__ __forceinline__ float band_energy(const float* tmp, int i) {
    double acc = 0.0;
    if (i >= 1) {
        const int g0 = c_gmt[i - 1], size = c_gmt[i] - g0;
        for (int j = 0; j < size; ++j) {
            const float fr = (float)((double)j / (double)size);
            acc += (double)(fr * tmp[g0 + j]);
        }
    }
    if (i <= NELE_NBANDS - 2) {
        const int g0 = c_gmt[i], size = c_gmt[i + 1] - g0;
        for (int j = 0; j < size; ++j) {
            const float fr = (float)(1.0 - (double)j / (double)size);
            acc += (double)(fr * tmp[g0 + j]);
        }
    }
    return (float)acc;
}

// The same sums with the per-bin weights from LDS tables: band_energy() pays a float64 division per term on the one wave that runs it
// (PMC: stft_band_wave_kernel and band_from_psd_kernel are bound by instruction issue, and the divisions are most of it).
// frw[k] = (float)(j / size), omw[k] = (float)(1 - j / size) for bin k = g0 + j of its band - the very expressions above, evaluated once
// per workgroup by one thread per BAND (<= 14 bins each; a per-bin fill that searches its band costs more than it saves: measured), so
// every product and the order of the float64 sum are unchanged: bit-identical.
__device__ __forceinline__ void band_weights_init(float* __restrict__ frw, float* __restrict__ omw) {
    const int i = threadIdx.x;
    if (i <= NELE_NBANDS - 2) {
        const int g0 = c_gmt[i], size = c_gmt[i + 1] - g0;
        for (int j = 0; j < size; ++j) {
            frw[g0 + j] = (float)((double)j / (double)size);
            omw[g0 + j] = (float)(1.0 - (double)j / (double)size);
        }
    }
}
__device__ __forceinline__ float band_energy_w(const float* tmp, const float* __restrict__ frw, const float* __restrict__ omw, int i) {
    double acc = 0.0;
    if (i >= 1) {
        const int g0 = c_gmt[i - 1], g1 = c_gmt[i];
        for (int k = g0; k < g1; ++k) acc += (double)(frw[k] * tmp[k]);
    }
    if (i <= NELE_NBANDS - 2) {
        const int g0 = c_gmt[i], g1 = c_gmt[i + 1];
        for (int k = g0; k < g1; ++k) acc += (double)(omw[k] * tmp[k]);
    }
    return (float)acc;
}

// np.abs(complex64) as numpy >= 1.25 computes it on FMA-capable x86 hosts (SIMD loop
// loops_unary_complex: larger * sqrt(fma(r, r, 1)), r = smaller / larger), so that |X|^2 is
// bit-identical to the oracle's and threshold decisions downstream (IMCRA, VAD) see the same values.
__device__ __forceinline__ float np_cabsf(float re, float im) {
    re = fabsf(re);
    im = fabsf(im);
    const float larger = fmaxf(re, im), smaller = fminf(im, re);
    if (larger == 0.f) return 0.f;
    const float ratio = smaller / larger;
    return sqrtf(__builtin_fmaf(ratio, ratio, 1.0f)) * larger;
}

__device__ __forceinline__ double hann512(int n) { return 0.5 - 0.5 * cospi((double)n / 256.0); }

// interp_band_gain (audio_util.py:93-110): bin k of band i (c_gmt[i] <= k < c_gmt[i + 1]) takes wlo of band i's gain and whi of band
// i + 1's.  band_gain_weights is the form that is given the band, band_gain the one that searches it (2 <= k <= 255: bins 0, 1 and
// 256 have fixed gains), band_gain_sqrt adds the fixed gains and np.sqrt (audio_util.py:85).
__device__ __forceinline__ void band_gain_weights(int k, int i, float& wlo, float& whi) {
    const int size = c_gmt[i + 1] - c_gmt[i], jj = k - c_gmt[i];
    const double frac = (double)jj / (double)size;
    wlo = (float)(1.0 - frac);
    whi = (float)frac;
}
__device__ __forceinline__ float band_gain(const float* __restrict__ a2, int k) {
    int i = 0;
    while (c_gmt[i + 1] <= k) ++i;
    float wlo, whi;
    band_gain_weights(k, i, wlo, whi);
    return wlo * a2[i] + whi * a2[i + 1];
}
__device__ __forceinline__ double band_gain_sqrt(const float* __restrict__ a2, int k) {
    if (k <= 1) return sqrt(1e-4);
    if (k == NELE_NBINS - 1) return sqrt(1e-2);
    return sqrt((double)band_gain(a2, k));
}

// One sample of the resynthesis (audio_util.py:60-65, librosa's overlap-add into a float32 buffer and window_sumsquare with the same
// float32 staging): x1 = the earlier frame's second half at n, x2 = the later frame's first half, wa = hann512(n + 256), wb = hann512(n).
__device__ __forceinline__ float istft_ola(double x1, double x2, double wa, double wb) {
    float y = (float)(wa * x1);
    y = (float)((double)y + wb * x2);
    float wss = (float)(wa * wa);
    wss = (float)((double)wss + wb * wb);
    return y / wss;
}
