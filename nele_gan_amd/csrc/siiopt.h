// SII-optimal band gains (Taal, Jensen & Leijon, IEEE SPL 2013): the one definition of a frame's arithmetic -
// steps 1 to 4 of the contract - for the offline kernel (siiopt.hip) and the real-time rule hop (realtime.hip).  One wave, lane = band.
// Both users are compiled with -ffp-contract=off (Makefile EXACT), so a frame's mask is the same bits in both.
#pragma once
#include "common.h"
#include "../../include/nele_hip_ext5.h"

// step 1: band feature (energy ** 1/6, float32) -> band power, float64
__device__ __forceinline__ double siiopt_power(float feat) {
    const double x = (double)feat, x2 = x * x;
    return x2 * x2 * x2;
}
__device__ __forceinline__ double siiopt_noise(float feat) {
    const double n = siiopt_power(feat);
    return (n > NELE_SIIOPT_NMIN) ? n : NELE_SIIOPT_NMIN;          // written so that a NaN feature gives the floor
}

// step 2: long-term speech power after frame t (prefix mean, then exponential)
__device__ __forceinline__ double siiopt_sbar_step(double Sbar, double P, int t, double lam) {
    const double k = fmax(1.0 / (double)(t + 1), 1.0 - lam);
    return Sbar + k * (P - Sbar);
}

// steps 3 and 4: water-filling at total power sum Sbar, then the gain.  Every lane of the wave must be here (wave_sum, ballot).
__device__ __forceinline__ float siiopt_solve(double Sbar, double N, double gamma, double strength) {
    const double r = wave_sum(Sbar);
    const double g = sqrt(gamma * N);
    bool act = gamma > 0.0 && Sbar > 0.0;
    double p = 0.0;
    for (int round = 0; round < 64 && __ballot(act) != 0ull; ++round) {      // wave-uniform: c only falls, a removed band stays removed
        const double c = (r + wave_sum(act ? N : 0.0)) / wave_sum(act ? g : 0.0);
        p = act ? c * g - N : 0.0;
        const bool out = act && !(p > 0.0);
        if (out) { act = false; p = 0.0; }
        if (__ballot(out) == 0ull) break;
    }
    if (!act) p = 0.0;
    double alpha = Sbar > 0.0 ? p / Sbar : 1.0;
    alpha = fmin(fmax(alpha, exp(-NELE_SIIOPT_LOGMAX)), exp(NELE_SIIOPT_LOGMAX));
    return strength == 1.0 ? (float)alpha : (float)exp(strength * log(alpha));
}

// one frame t of one row / slot: Sbar (this lane's band) is advanced in place; -> the frame's mask value of this band
__device__ __forceinline__ float siiopt_frame(double& Sbar, float cb, float nb, double gamma, int t, double lam, double strength) {
    Sbar = siiopt_sbar_step(Sbar, siiopt_power(cb), t, lam);
    return siiopt_solve(Sbar, siiopt_noise(nb), gamma, strength);
}
