// SII-optimal band gains, offline (nele_siiopt_mask): band features of a padded batch in, the mask out, in the
// layouts of the generator's forward pass ([B][T][64] float32 each).  The frame arithmetic is siiopt.h's, shared with the real-time
// rule hop of realtime.hip; this file is built without FMA contraction (Makefile EXACT) as that one is, so both give the same bits.
// Only the long-term speech power Sbar is serial over the frames (one multiply-add per frame and band); the water-filling of a frame
// (three wave sums per round, 2 to 3 rounds, sqrt / log / exp) is some hundred times that and independent of every other frame.  So:
// one workgroup of 512 threads per row, frames in chunks of 64 - (1) wave 0 scans Sbar over the chunk into LDS (lane = band, 32 KB),
// (2) the eight waves solve the chunk's frames, frame j of the chunk by wave j % 8.  Everything stays inside the row in a fixed order:
// a row's mask does not depend on B or on the row's position.
#include "siiopt.h"

#define SO_CH 64
#define SO_THREADS 512

__global__ __launch_bounds__(SO_THREADS) void siiopt_mask_kernel(const float* __restrict__ cb, const float* __restrict__ nb,
                                                                 const double* __restrict__ gamma, int T, double lam, double strength,
                                                                 float* __restrict__ mask) {
    __shared__ double sbar[SO_CH][64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)b * T * 64;
    const double g = gamma[lane];
    double S = 0.0;                                                  // wave 0's running Sbar of band `lane`
    for (int c0 = 0; c0 < T; c0 += SO_CH) {
        const int nc = min(SO_CH, T - c0);
        __syncthreads();                                             // the previous chunk's solves have read sbar
        if (wv == 0) {
            for (int j = 0; j < nc; ++j) {
                S = siiopt_sbar_step(S, siiopt_power(cb[base + (size_t)(c0 + j) * 64 + lane]), c0 + j, lam);
                sbar[j][lane] = S;
            }
        }
        __syncthreads();
        for (int j = wv; j < nc; j += SO_THREADS / 64) {
            const size_t o = base + (size_t)(c0 + j) * 64 + lane;
            mask[o] = siiopt_solve(sbar[j][lane], siiopt_noise(nb[o]), g, strength);
        }
    }
}

// shared by the three entry points (realtime.hip declares it): the rule's host-side parameter checks
int siiopt_check(const char* name, const double* gamma, double lam, double strength) {
    NELE_CHECK_ARG(gamma, "%s: null gamma", name);
    NELE_CHECK_ARG(lam >= 0.0 && lam < 1.0, "%s: lam=%g must be in [0, 1)", name, lam);
    NELE_CHECK_ARG(strength > 0.0 && strength <= 1.0, "%s: strength=%g must be in (0, 1]", name, strength);
    return NELE_OK;
}

extern "C" int nele_siiopt_mask(const float* cb, const float* nb, const double* gamma, int B, int T, double lam, double strength, float* mask,
                                void* stream) {
    NELE_CHECK_ARG(cb && nb && mask, "nele_siiopt_mask: null cb / nb / mask");
    NELE_CHECK_ARG(B >= 1 && T >= 1 && (long long)B * T <= (1LL << 31), "nele_siiopt_mask: B=%d, T=%d must be >= 1 (B T <= 2^31)", B, T);
    if (int st = siiopt_check("nele_siiopt_mask", gamma, lam, strength)) return st;
    hipLaunchKernelGGL(siiopt_mask_kernel, dim3(B), dim3(SO_THREADS), 0, as_stream(stream), cb, nb, gamma, T, lam, strength, mask);
    NELE_CHECK_LAUNCH("nele_siiopt_mask");
    return NELE_OK;
}
