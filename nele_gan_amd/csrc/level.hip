// Active speech level (ITU-T P.56 method B, the reference's asl_P56.py:23-148 at fs = 16000, nbits = 16) and noise mixing at a target SNR
// (DESIGN.md "Noise mixing at an active-level SNR").
//
// nele_asl_p56_var - one workgroup of P56_NT threads per utterance, samples in chunks of P56_CH through LDS:
//   (1) all threads: u[i] = (1 - g) |x[i]| in float64 (off the recurrence's dependency chain) and the thread's share of sum x^2;
//   (2) ONE lane: the two one-pole recurrences of the envelope in sample order, y[k] = u[k] + z; z = g y[k] - the operation order of
//       scipy.signal.lfilter([1-g, 0], [1, -g], .) - q written over u.  This file is built without FMA contraction (Makefile EXACT): the
//       product (1 - g) p[k] and the sum with z stay two roundings, as in lfilter's C loop.  The SEQUENTIAL form was built, not a chunked
//       scan: a threshold comparison q[k] >= c[j] is a discontinuity, the activity counts must equal the reference's integers, and only
//       the reference's own operation order gives that by construction;
//   (3) all threads: thread (threshold j, segment s of the chunk) - threshold j counts sample k iff some k' in [k - 3200, k] has
//       q[k'] >= c[j] (the reference's hangover counters say exactly this: its `break` only skips thresholds that cannot count).  Pass A
//       finds each segment's last exceedance, pass B walks the segment with the last exceedance before it carried in.  Index maxima and
//       integer counts: exact in any order;
//   then one lane runs the reference's tail (asl_P56.py:60-94, bin_interp) in float64.
// Everything stays inside the utterance's own row in an order fixed by its length alone: a row's result is bit-identical at B = 1 and
// inside any padded batch.
//
// nele_mix_noise_var - one workgroup per utterance: mean square of the pool segment in float64 (thread-strided partial sums, fixed-order
// block sum), gain = sqrt(S / (10^(snr/10) Nms)) in float64, noise[k] = (float)(gain * v[k]), zeros behind the row's end.
#include "common.h"
#include "../../include/nele_hip.h"

#define P56_NT 256
#define P56_CH 2048
#define P56_NTHR 15
#define P56_NSEG (P56_NT / 16)
#define P56_SEG (P56_CH / P56_NSEG)
#define P56_HANG 3200                                     // ceil(fs H) = ceil(16000 * 0.2)
#define P56_MARGIN 15.9
#define P56_EPS 2.220446049250313e-16                     // np.finfo(float).eps
#define P56_G 0x1.feef37b358867p-1                        // np.exp(-1 / (fs T)) = exp(-1 / 480), the float64 the reference filters with (tests/test_p56_cpu.py)

// asl_P56.py:98-148.  The bounds upcount / lwcount never move (the reference halves towards the same two ends): kept as it is.
__device__ static void p56_bin_interp(double upcount, double lwcount, double upthr, double lwthr, double margin, double tol, double* asl_ms_log,
                                      double* cc) {
    if (fabs(upcount - upthr - margin) < tol) { *asl_ms_log = upcount; *cc = upthr; return; }
    if (fabs(lwcount - lwthr - margin) < tol) { *asl_ms_log = lwcount; *cc = lwthr; return; }
    double midcount = (upcount + lwcount) / 2.0, midthr = (upthr + lwthr) / 2.0;
    int iterno = 1;
    for (int guard = 0; guard < 4096; ++guard) {          // (the tolerance grows by 10 % per turn after 20: ends within a few hundred)
        const double diff = midcount - midthr - margin;
        if (fabs(diff) <= tol) break;
        iterno += 1;
        if (iterno > 20) tol = tol * 1.1;
        if (diff > tol) {
            midcount = (upcount + midcount) / 2.0;
            midthr = (upthr + midthr) / 2.0;
        } else if (diff < -tol) {
            midcount = (midcount + lwcount) / 2.0;
            midthr = (midthr + lwthr) / 2.0;
        }
    }
    *asl_ms_log = midcount;
    *cc = midthr;
}

__global__ __launch_bounds__(P56_NT) void asl_p56_kernel(const float* __restrict__ x, const int* __restrict__ lengths, int Lmax,
                                                         double* __restrict__ asl_msq, double* __restrict__ actfact, double* __restrict__ c0_out,
                                                         double* __restrict__ sq_out, long long* __restrict__ counts, int* __restrict__ status) {
    __shared__ double q[P56_CH];                          // u, then the envelope q, of the chunk
    __shared__ int seglast[P56_NSEG][16];
    __shared__ int carry[16];                             // last exceedance of threshold j before the chunk (-1: none yet)
    __shared__ long long segcnt[P56_NSEG][16];
    __shared__ double scratch[P56_NT / 64];
    __shared__ double zs[2];                              // the two filter states between chunks
    const int b = blockIdx.x, tid = threadIdx.x, j = tid & 15, s = tid >> 4;
    int len = lengths ? lengths[b] : Lmax;
    len = max(0, min(len, Lmax));
    const float* xr = x + (size_t)b * Lmax;
    const double g = P56_G, omg = 1.0 - g;
    const double cj = ldexp(1.0, min(j, P56_NTHR - 1) - 15);
    if (tid < 16) carry[tid] = -1;
    if (tid < 2) zs[tid] = 0.0;
    double sqacc = 0.0;
    long long cnt = 0;
    for (int k0 = 0; k0 < len; k0 += P56_CH) {
        const int n = min(P56_CH, len - k0);
        __syncthreads();
        for (int i = tid; i < n; i += P56_NT) {
            const double v = (double)xr[k0 + i];
            sqacc += v * v;
            q[i] = omg * fabs(v);
        }
        __syncthreads();
        if (tid == 0) {
            double zp = zs[0], zq = zs[1];
#pragma unroll 8
            for (int i = 0; i < n; ++i) {
                const double p = q[i] + zp;
                zp = g * p;
                const double e = omg * p + zq;
                zq = g * e;
                q[i] = e;
            }
            zs[0] = zp;
            zs[1] = zq;
        }
        __syncthreads();
        const int i0 = s * P56_SEG, i1 = min(n, i0 + P56_SEG);
        int last = -1;
        if (j < P56_NTHR)
            for (int i = i0; i < i1; ++i)
                if (q[i] >= cj) last = k0 + i;
        seglast[s][j] = last;
        __syncthreads();
        if (j < P56_NTHR) {
            last = carry[j];
            for (int t = 0; t < s; ++t) last = max(last, seglast[t][j]);
            for (int i = i0; i < i1; ++i) {
                const int k = k0 + i;
                if (q[i] >= cj) last = k;
                cnt += (last >= 0 && k - last <= P56_HANG) ? 1 : 0;
            }
        }
        __syncthreads();
        if (s == P56_NSEG - 1) {                          // (the chunk's last exceedance: this segment's walk saw all of them)
            int l2 = carry[j];
            for (int t = 0; t < P56_NSEG; ++t) l2 = max(l2, seglast[t][j]);
            carry[j] = l2;
        }
    }
    const double sq = block_sum(sqacc, scratch);
    segcnt[s][j] = cnt;
    __syncthreads();
    if (tid == 0) {
        long long a[P56_NTHR];
        for (int t = 0; t < P56_NTHR; ++t) {
            long long c = 0;
            for (int u = 0; u < P56_NSEG; ++u) c += segcnt[u][t];
            a[t] = c + 1;                                 // the reference starts at -1 and adds 2 (asl_P56.py:39, :65)
            counts[(size_t)b * P56_NTHR + t] = a[t];
        }
        double r_asl = 0.0, r_act = 0.0, r_c0 = 0.0;
        int st = 0;
        if (a[0] == 1) {
            st = NELE_P56_SILENT;                         // asl_P56.py:62-63 (the reference fails on the unset c0)
        } else {
            const double AdB1 = 10.0 * log10(sq / (double)a[0] + P56_EPS);
            const double CdB1 = 20.0 * log10(ldexp(1.0, -15) + P56_EPS);
            if (AdB1 - CdB1 < P56_MARGIN) {
                st = NELE_P56_BELOW_MARGIN;               // :69-70 (likewise)
            } else {
                st = NELE_P56_NO_CROSSING;                // :83-94 falls through with c0 unset
                double AdBp = AdB1, CdBp = CdB1;
                for (int t = 1; t < P56_NTHR; ++t) {
                    const double AdB = 10.0 * log10(sq / ((double)a[t] + P56_EPS) + P56_EPS);
                    const double CdB = 20.0 * log10(ldexp(1.0, t - 15) + P56_EPS);
                    if (AdB - CdB <= P56_MARGIN) {
                        double ml, cl0;
                        p56_bin_interp(AdB, AdBp, CdB, CdBp, P56_MARGIN, 0.5, &ml, &cl0);
                        r_asl = pow(10.0, ml / 10.0);
                        r_act = (sq / (double)len) / r_asl;
                        r_c0 = pow(10.0, cl0 / 20.0);
                        st = 0;
                        break;
                    }
                    AdBp = AdB;
                    CdBp = CdB;
                }
            }
        }
        asl_msq[b] = r_asl;
        actfact[b] = r_act;
        c0_out[b] = r_c0;
        sq_out[b] = sq;
        status[b] = st;
    }
}

extern "C" long long nele_asl_p56_workspace_bytes(int B, int Lmax) {
    (void)B;
    (void)Lmax;
    return 0;                                             // the envelope never leaves LDS
}

extern "C" int nele_asl_p56_var(const float* x, const int* lengths, int B, int Lmax, void* workspace, long long workspace_bytes, double* asl_msq,
                                double* actfact, double* c0, double* sq, long long* counts, int* status, void* stream) {
    NELE_CHECK_ARG(x && asl_msq && actfact && c0 && sq && counts && status && B > 0 && Lmax > 0, "nele_asl_p56_var: bad arguments");
    NELE_CHECK_ARG(workspace_bytes >= nele_asl_p56_workspace_bytes(B, Lmax), "nele_asl_p56_var: workspace too small");
    (void)workspace;
    hipLaunchKernelGGL(asl_p56_kernel, dim3(B), dim3(P56_NT), 0, as_stream(stream), x, lengths, Lmax, asl_msq, actfact, c0, sq, counts, status);
    NELE_CHECK_LAUNCH("nele_asl_p56_var");
    return NELE_OK;
}

#define MIX_NT 1024

__global__ __launch_bounds__(MIX_NT) void mix_noise_kernel(const float* __restrict__ pool, const int* __restrict__ pool_lengths, int N, int Ln,
                                                           const int* __restrict__ rows, const int* __restrict__ offsets,
                                                           const double* __restrict__ snr_db, const double* __restrict__ level,
                                                           const int* __restrict__ lengths, int Lmax, float* __restrict__ noise,
                                                           double* __restrict__ gain_out, int* __restrict__ status) {
    __shared__ double scratch[MIX_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int len = lengths ? lengths[b] : Lmax;
    len = max(0, min(len, Lmax));
    float* out = noise + (size_t)b * Lmax;
    const int row = rows[b];
    int st = 0, plen = 0;
    if (row < 0 || row >= N) {
        st = NELE_MIX_BAD_ROW;
    } else {
        plen = pool_lengths ? pool_lengths[row] : Ln;
        if (plen <= 0 || plen > Ln) st = NELE_MIX_BAD_ROW;
    }
    if (st) plen = 1;
    double gain = 0.0;
    const float* pr = pool;
    int first = 0, step = 0;                              // this thread's running index (start + k) mod plen: first < plen, step < plen
    if (!st) {                                            // (block-uniform)
        pr = pool + (size_t)row * Ln;
        const int start = (int)(((long long)offsets[b] % plen + plen) % plen);
        first = (int)(((long long)start + tid) % plen);
        step = MIX_NT % plen;
        double acc = 0.0;
        int idx = first;
        for (int k = tid; k < len; k += MIX_NT) {
            const double v = (double)pr[idx];
            acc += v * v;
            idx += step;
            if (idx >= plen) idx -= plen;
        }
        const double tot = block_sum(acc, scratch);
        const double nms = len > 0 ? tot / (double)len : 0.0;
        const double S = level[b];
        if (!(nms > 0.0)) st |= NELE_MIX_ZERO_NOISE;
        if (!(S > 0.0)) st |= NELE_MIX_ZERO_LEVEL;
        if (!st) gain = sqrt(S / (pow(10.0, snr_db[b] / 10.0) * nms));
    }
    int idx = first;
    for (int k = tid; k < Lmax; k += MIX_NT) {
        out[k] = (k < len && !st) ? (float)(gain * (double)pr[idx]) : 0.f;
        idx += step;
        if (idx >= plen) idx -= plen;
    }
    if (tid == 0) {
        gain_out[b] = gain;
        status[b] = st;
    }
}

extern "C" int nele_mix_noise_var(const float* pool, const int* pool_lengths, int N, int Ln, const int* rows, const int* offsets,
                                  const double* snr_db, const double* level, const int* lengths, int B, int Lmax, float* noise, double* gain,
                                  int* status, void* stream) {
    NELE_CHECK_ARG(pool && rows && offsets && snr_db && level && noise && gain && status && N > 0 && Ln > 0 && B > 0 && Lmax > 0,
                   "nele_mix_noise_var: bad arguments");
    hipLaunchKernelGGL(mix_noise_kernel, dim3(B), dim3(MIX_NT), 0, as_stream(stream), pool, pool_lengths, N, Ln, rows, offsets, snr_db, level,
                       lengths, Lmax, noise, gain, status);
    NELE_CHECK_LAUNCH("nele_mix_noise_var");
    return NELE_OK;
}
