// The per-bin steps of one IMCRA frame (noise_est/imcra.py), defined once for the kernels that run them: imcra_band_kernel,
// imcra_ind_kernel and imcra_track_kernel (features.hip), rt_front_kernel (realtime.hip) and ns_hop_kernel (ns.hip).  A step is the
// arithmetic of the lines it names, in numpy's order of operations and with numpy's float32 / float64 staging (the including file is
// compiled with -ffp-contract=off); the state goes in and out by reference to the caller's registers.  The loop over frames, the
// neighbour exchange, the storage of the minima and the state's layout stay with each kernel.
#pragma once
#include "common.h"

constexpr double IMCRA_ALPHA_S = 0.9, IMCRA_ALPHA_D = 0.85, IMCRA_BMIN = 3.2, IMCRA_GAMMA0 = 4.6, IMCRA_GAMMA1 = 3.0, IMCRA_ZETA0 = 1.67;
constexpr double IMCRA_BETA = 1.47, IMCRA_ALPHA_DD = 0.92, IMCRA_P_UP = 0.9;
constexpr double IMCRA_ONE_M_AS = 1.0 - IMCRA_ALPHA_S, IMCRA_ONE_M_AD = 1.0 - IMCRA_ALPHA_D, IMCRA_ONE_M_ADD = 1.0 - IMCRA_ALPHA_DD;
__device__ __forceinline__ double imcra_xi_min() { return pow(10.0, -25.0 / 20.0); }

// fsmooth's weights of bin k (imcra.py:270-280: sym_hanning(3), row-normalised: an edge bin has two taps)
__device__ __forceinline__ void imcra_smooth_weights(int k, double& w0, double& w1, double& w2) {
    double a = 0.25, b = 0.5, c = 0.25;
    if (k == 0) { a = 0.0; b = 1.0 / 1.5; c = 0.5 / 1.5; }
    if (k == NELE_NBINS - 1) { a = 0.5 / 1.5; b = 1.0 / 1.5; c = 0.0; }
    w0 = a; w1 = b; w2 = c;
}
// fsmooth over the left neighbour, the bin and the right neighbour (at an edge the absent one has weight 0: any finite value stands in)
__device__ __forceinline__ double imcra_smooth3(double w0, double w1, double w2, double vl, double vc, double vr) {
    return (w0 * vl + w1 * vc) + w2 * vr;
}

// imcra.py:543-557, decision-directed a-priori SNR of frame l: new Gamma and G, returns xi.  Lambda_D (hence Gamma, xi_ML) is a float32
// array for frames 1..15 (Lam32: what frames 0..14 wrote) and float64 from frame 16 on and in frame 0 (Lam64).
__device__ __forceinline__ double imcra_snr_step(int l, float Y2f, double Lam64, float Lam32, double& G, double& Gamma) {
    const double xi_G = (l == 0) ? 1.0 : (G * G) * Gamma;
    double term;
    if (l == 0 || l >= 16) {
        Gamma = (double)Y2f / Lam64;
        double xi_ML = Gamma - 1.0;
        if (xi_ML < 1e-6) xi_ML = 1e-6;
        term = IMCRA_ONE_M_ADD * xi_ML;
    } else {
        const float Gf = Y2f / Lam32;
        float xf = Gf - 1.0f;
        if (xf < (float)1e-6) xf = (float)1e-6;
        term = (double)((float)IMCRA_ONE_M_ADD * xf);
        Gamma = (double)Gf;
    }
    double xi = IMCRA_ALPHA_DD * xi_G + term;
    if (xi < imcra_xi_min()) xi = imcra_xi_min();
    G = xi / (1.0 + xi);
    return xi;
}

// imcra.py:386-387, 400-401: time smoothing of S (and of S~) by the frame's frequency-smoothed value
__device__ __forceinline__ double imcra_tsmooth(double S, double Sf) { return IMCRA_ALPHA_S * S + IMCRA_ONE_M_AS * Sf; }

// imcra.py:386-390, 400-404: S and its two running minima
__device__ __forceinline__ void imcra_s_step(double Sf, double& S, double& Smin, double& Smin_sw) {
    S = imcra_tsmooth(S, Sf);
    Smin = fmin(Smin, S);
    Smin_sw = fmin(Smin_sw, S);
}
// imcra.py:405-409: the rough speech indicator I of a frame l >= 15 (true: no strong speech in the bin)
__device__ __forceinline__ bool imcra_indicator(double Y2, double S, double Smin) {
    const double Gamma_min = Y2 / (IMCRA_BMIN * Smin);
    const double zeta = S / (IMCRA_BMIN * Smin);
    return Gamma_min < IMCRA_GAMMA0 && zeta < IMCRA_ZETA0;
}

// imcra.py:392: lambda_D of frames 0..14, a float32 array smoothed by float32 scalars
__device__ __forceinline__ float imcra_lambda32_step(float Lam32, float Y2f) {
    return (float)IMCRA_ALPHA_D * Lam32 + (float)IMCRA_ONE_M_AD * Y2f;
}

// imcra.py:415-429: S~ from tSf = fsmooth(I |Y|^2) and norm = fsmooth(I), its running minima, and the speech-absence prior q, returned as
// post_speech_prob's q / (1 - q) (imcra.py:34), or -1 where q = 1 (there p = 0)
__device__ __forceinline__ double imcra_prior_step(double Y2, double S, double tSf, double norm, double& tS, double& tSmin, double& tSmin_sw) {
    if (norm > 0.0) tSf = tSf / norm;
    tS = imcra_tsmooth(tS, tSf);
    tSmin = fmin(tSmin, tS);
    tSmin_sw = fmin(tSmin_sw, tS);
    const double tG = Y2 / (IMCRA_BMIN * tSmin);
    const double tz = S / (IMCRA_BMIN * tSmin);
    double q = 0.0;
    if (tG <= 1.0 && tz < IMCRA_ZETA0) q = 1.0;
    else if (1.0 < tG && tG < IMCRA_GAMMA1 && tz < IMCRA_ZETA0) q = (IMCRA_GAMMA1 - tG) / (IMCRA_GAMMA1 - 1.0);
    return (q < 1.0) ? q / (1.0 - q) : -1.0;
}

// imcra.py:22-36, 432-441: speech-presence probability from r = imcra_prior_step's result, then the recursive PSD update; returns the
// new (float64) lambda_D and hands back the p that drove it.  CAP: p is held to IMCRA_P_UP as the reference's tracker holds it; the
// noise suppressor (csrc/ns.hip) runs the uncapped form.
template <bool CAP>
__device__ __forceinline__ double imcra_psd_step_p(double Y2, double Gamma, double xi, double r, double& ovL, double& p) {
    const double nu = Gamma * xi / (1.0 + xi);
    p = 0.0;
    if (r >= 0.0) p = 1.0 / (1.0 + r * (1.0 + xi) * exp(-nu));
    if (CAP && p > IMCRA_P_UP) p = IMCRA_P_UP;
    const double tad = IMCRA_ALPHA_D + IMCRA_ONE_M_AD * p;
    ovL = tad * ovL + (1.0 - tad) * Y2;
    return IMCRA_BETA * ovL;
}
__device__ __forceinline__ double imcra_psd_step(double Y2, double Gamma, double xi, double r, double& ovL) {
    double p;
    return imcra_psd_step_p<true>(Y2, Gamma, xi, r, ovL, p);
}

// imcra.py:443-481, what every form of the minima store (LDS rows, eight registers, the stream record) decides alike: the store is
// written in every V = 15th frame (j counts the frames since frame 15 or since the last store), into slot u mod U (np.roll of the U = 8
// columns == a ring), and the minimum runs over the n slots filled so far.
__device__ __forceinline__ bool imcra_store_due(int j, int u, int& slot, int& n) {
    slot = u & 7;
    n = (u < 8) ? (u + 1) : 8;
    return j + 1 == 15;
}
__device__ __forceinline__ void imcra_advance(int& j, int& u) {
    if (++j == 15) { j = 0; ++u; }
}
