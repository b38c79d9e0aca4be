// Noise suppression for the real-time uplink, many concurrent streams (nele_ns_*): the optimally-modified log-spectral amplitude gain
// (Cohen & Berdugo 2001) on the project's IMCRA noise tracker, applied to what the echo canceller leaves, on the real-time path's
// blocks - 256-sample hops, sqrt-Hann windowed 512-sample frames, float64 transforms (fft512.h).  The arithmetic is DESIGN.md section
// 21; tests/ns_ref.py restates it in numpy.
//   ns_hop_kernel : one wave per stream, four streams per workgroup, looping over the call's hops
// res_hop_kernel's shape (csrc/res.hip): a wave keeps its stream's whole per-bin state in registers across the call's hops.  Lane l
// holds bins 64 m + l, m < 5 - slot 4 is bin 256 and exists in lane 0 alone; the other lanes skip it - and samples 64 m + l (m < 4) of
// x_prev and the overlap-add tail.  Per hop: one forward transform of w [x_prev, x] (imaginary part zero: bins 0 .. 256 are E), one
// IMCRA frame in the steps of imcra.h and rt_front_kernel's order, the gain, one inverse transform of the Hermitian extension of G E.
// The three-tap frequency smoothing of Y2, I and I Y2 is the only coupling between bins: the wave's exchange buffer carries them, as
// double [259] each with the edge bins doubled.  The two minima rings are touched every 15th frame and stay in the stream's record.
// State is read and written with plain loads and stores by the stream's own wave; no atomics, nothing crosses waves: a slot's bits do
// not depend on the hop grouping, on B or on the other slots.
// In the Makefile's EXACT list (no FMA contraction): the IMCRA steps keep numpy's operation order, as in realtime.hip.
#include "common.h"
#include "fft512.h"
#include "imcra.h"
#include "slot_state.h"
#include "../../include/nele_hip_ext4.h"

namespace {

#define NS_BLK 256                                         // samples per hop
#define NS_WAVES 4                                         // streams per workgroup
#define NS_NB 264                                          // bins padded
constexpr long long NS_HDR_BYTES = SLOT_GEOM_HDR_BYTES;    // int [0] = max_streams, [1] = the record's bytes (what nele_ns_init laid out)
// per-stream record, byte offsets
constexpr long long NS_O_CTL = 0;                                       // int [3]: l (frames so far, stops at 16), j, u (the minima store's)
constexpr long long NS_O_XPREV = 64;                                    // float [256]: the previous hop of x (float32 in, kept exactly)
constexpr long long NS_O_OLA = NS_O_XPREV + 4 * NS_BLK;                 // double [256]: the overlap-add tail o[256:512]
constexpr long long NS_O_LAM32 = NS_O_OLA + 8 * NS_BLK;                 // float [NS_NB]: lambda_D of frames 0 .. 14
constexpr long long NS_O_IMD = NS_O_LAM32 + 4 * NS_NB;                  // double [NS_NIMD][NS_NB]: IMCRA's per-bin state, NS_F_*
enum { NS_F_G, NS_F_GAMMA, NS_F_LAM64, NS_F_S, NS_F_SMIN, NS_F_SMINSW, NS_F_TS, NS_F_TSMIN, NS_F_TSMINSW, NS_F_OVL, NS_NIMD };
constexpr long long NS_O_RING = NS_O_IMD + 8LL * NS_NIMD * NS_NB;       // double [2][8][NS_NB]: the minima stores of S and of S~
constexpr long long NS_REC_BYTES = slot_al(NS_O_RING + 8LL * 16 * NS_NB);
static_assert(NS_O_OLA % 8 == 0 && NS_O_IMD % 8 == 0 && NS_REC_BYTES == 59136, "the record of DESIGN.md section 21");
constexpr double NS_EULER = 0.5772156649015329;
// the exchange buffer as doubles: Y2, I Y2 and I with the edge bins doubled (bin k at [k + 1])
constexpr int NS_X_Y2 = 0, NS_X_IY = 264, NS_X_I = 528;
static_assert(NS_X_I + NELE_NBINS + 2 <= 2 * FFTW_SLOTS && NELE_NBINS == NS_BLK + 1, "three [259] rows fit the exchange buffer");

struct NsArgs {
    unsigned char* state;
    int S;
    const float* x;              // [S][ld]
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double gmin;
    float* out;                  // [S][ld]
    double *gains, *noise_psd, *presence;   // [S][nh][257] or null
};

// w[n] = sqrt(0.5 - 0.5 cos(2 pi n / 512))
__device__ __forceinline__ double ns_window(int n) { return sqrt(0.5 - 0.5 * cospi((double)n / 256.0)); }

// E1(x), x > 0 (section 21 step 4): below 1 the series -gamma - ln x - sum_k (-x)^k / (k k!); from 1 on the continued fraction
// e^-x / (x + 1 - 1 / (x + 3 - 4 / (x + 5 - ...))) by its forward recurrence A_n = b_n A_{n-1} + a_n A_{n-2}, B_n likewise - no
// division inside the loop (the Lentz form of tests/ns_ref.py has two, and 92 rounds at x = 1) - both pairs scaled by 2^-512, which
// is exact, when B passes 2^512; it stops where two convergents agree to 2^-50 of their value.  Held to scipy.special.exp1 at 2e-14
// relative over [1, 700] on a host restatement.  Beyond 700 E1 < 1e-306 and exp(E1 / 2) is 1 to the last bit: 0.  Each lane stops at
// its own convergence; the caps end the loops on a NaN.
__device__ __forceinline__ double ns_e1(double x) {
    if (x < 1.0) {
        double ans = -log(x) - NS_EULER, fact = 1.0;
        for (int i = 1; i <= 40; ++i) {
            fact = fact * (-x / i);
            const double d = -fact / i;
            ans += d;
            if (fabs(d) < fabs(ans) * 0x1p-52) break;
        }
        return ans;
    }
    if (x > 700.0) return 0.0;
    double Am = 0.0, A = 1.0, Bm = 1.0, B = x + 1.0;       // A_0 / B_0 = 0 / 1, A_1 / B_1 = 1 / (x + 1)
    for (int n = 2; n <= 200; ++n) {
        const double an = -(double)(n - 1) * (n - 1), bn = x + (2 * n - 1);
        const double An = bn * A + an * Am, Bn = bn * B + an * Bm;
        Am = A; Bm = B; A = An; B = Bn;
        const double cross = A * Bm;                       // A_n / B_n - A_{n-1} / B_{n-1} = (A_n B_{n-1} - A_{n-1} B_n) / (B_n B_{n-1})
        if (fabs(cross - Am * B) < fabs(cross) * 0x1p-50) break;
        if (fabs(B) > 0x1p512) { A *= 0x1p-512; Am *= 0x1p-512; B *= 0x1p-512; Bm *= 0x1p-512; }
    }
    return (A / B) * exp(-x);
}

__global__ __launch_bounds__(64 * NS_WAVES) void ns_hop_kernel(NsArgs a) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[NS_WAVES][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();                                       // the only workgroup barrier: from here on a wave is on its own
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * NS_WAVES + w;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, (int)NS_REC_BYTES)) return;   // not the state nele_ns_init laid out for S: touch nothing
    unsigned char* rec = a.state + NS_HDR_BYTES + (size_t)b * NS_REC_BYTES;
    int* ctl = reinterpret_cast<int*>(rec + NS_O_CTL);
    float* xprevp = reinterpret_cast<float*>(rec + NS_O_XPREV);
    double* olap = reinterpret_cast<double*>(rec + NS_O_OLA);
    float* lam32p = reinterpret_cast<float*>(rec + NS_O_LAM32);
    double* imd = reinterpret_cast<double*>(rec + NS_O_IMD);
    double* ring = reinterpret_cast<double*>(rec + NS_O_RING);         // S: [slot][bin]; S~: [8 + slot][bin]
    double2* xw = xws[w];
    double* xd = reinterpret_cast<double*>(xw);
    const bool lane0 = (lane == 0);
    const int nm = lane0 ? 5 : 4;                          // bin slots of this lane: 64 m + lane <= 256
    const double2 zero = make_double2(0.0, 0.0);
    const double ln_gmin = log(a.gmin);

    // the stream's state and its window values: element m of each array belongs to index 64 m + lane
    float xp[4];
    double ola[4], wlo[4], whi[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = 64 * m + lane;
        xp[m] = xprevp[j];
        ola[m] = olap[j];
        wlo[m] = ns_window(j);
        whi[m] = ns_window(NS_BLK + j);
    }
    double G[5], Gamma[5], Lam64[5], S[5], Smin[5], Smin_sw[5], tS[5], tSmin[5], tSmin_sw[5], ovL[5];
    float Lam32[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        G[m] = Gamma[m] = Lam64[m] = S[m] = Smin[m] = Smin_sw[m] = tS[m] = tSmin[m] = tSmin_sw[m] = ovL[m] = 0.0;
        Lam32[m] = 0.f;
        if (m < nm) {
            const int k = 64 * m + lane;
            G[m] = imd[NS_F_G * NS_NB + k];
            Gamma[m] = imd[NS_F_GAMMA * NS_NB + k];
            Lam64[m] = imd[NS_F_LAM64 * NS_NB + k];
            S[m] = imd[NS_F_S * NS_NB + k];
            Smin[m] = imd[NS_F_SMIN * NS_NB + k];
            Smin_sw[m] = imd[NS_F_SMINSW * NS_NB + k];
            tS[m] = imd[NS_F_TS * NS_NB + k];
            tSmin[m] = imd[NS_F_TSMIN * NS_NB + k];
            tSmin_sw[m] = imd[NS_F_TSMINSW * NS_NB + k];
            ovL[m] = imd[NS_F_OVL * NS_NB + k];
            Lam32[m] = lam32p[k];
        }
    }
    int l = ctl[0], j = ctl[1], u = ctl[2];
    const float* xb = a.x + (size_t)b * a.ld;
    float* outb = a.out + (size_t)b * a.ld;
    const size_t row0 = (size_t)b * a.nh * NELE_NBINS;

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * NS_BLK, row = row0 + (size_t)h * NELE_NBINS;
        // ---- 1. E = rfft512(w [x_prev, x]); x_prev <- x
        float xn[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) xn[m] = xb[col + 64 * m + lane];
        fftw_wave_sync();                                  // the previous hop's reads of xw precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = 64 * m + lane;
            xw[fftw_slot(n)] = make_double2(wlo[m] * (double)xp[m], 0.0);
            xw[fftw_slot(NS_BLK + n)] = make_double2(whi[m] * (double)xn[m], 0.0);
            xp[m] = xn[m];
        }
        fftw_wave_sync();
        double2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = xw[fftw_slot(fftw_n(lane, r))];
        fftw_wave_sync();
        fft512_wave<false>(v, xw, tw, lane);
        fft512_wave_store(v, xw, lane);
        // ---- 2. Y2f = float32(|E|^2 + eps)
        double2 E[5];
        float Y2f[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            E[m] = zero;
            Y2f[m] = 0.f;
            if (m < nm) {
                E[m] = xw[fftw_slot(64 * m + lane)];
                Y2f[m] = (float)((E[m].x * E[m].x + E[m].y * E[m].y) + NELE_NS_EPS);
            }
        }
        fftw_wave_sync();                                  // every lane's reads of the spectrum precede these writes
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            if (m < nm) {
                const int k = 64 * m + lane;
                xd[NS_X_Y2 + k + 1] = (double)Y2f[m];
                if (k == 0) xd[NS_X_Y2] = (double)Y2f[m];
                if (k == NELE_NBINS - 1) xd[NS_X_Y2 + NELE_NBINS + 1] = (double)Y2f[m];
            }
        }
        fftw_wave_sync();
        // ---- 3. one IMCRA frame (the steps of imcra.h in rt_front_kernel's order), p uncapped
        double xi[5], p[5], I[5], lam[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            xi[m] = p[m] = I[m] = lam[m] = 0.0;
            if (m < nm) {
                const int k = 64 * m + lane;
                double w0, w1, w2;
                imcra_smooth_weights(k, w0, w1, w2);
                const double Y2 = (double)Y2f[m];
                const double Sf = imcra_smooth3(w0, w1, w2, xd[NS_X_Y2 + k], xd[NS_X_Y2 + k + 1], xd[NS_X_Y2 + k + 2]);
                if (l == 0) Lam64[m] = 1e-6;               // the tracker's start; G and Gamma are not read in frame 0
                xi[m] = imcra_snr_step(l, Y2f[m], Lam64[m], Lam32[m], G[m], Gamma[m]);
                if (l == 0) {
                    S[m] = Sf; tS[m] = Sf; Smin[m] = Sf; tSmin[m] = Sf; Smin_sw[m] = Sf; tSmin_sw[m] = Sf;
                    ovL[m] = Y2;
                    Lam32[m] = Y2f[m];
                }
                imcra_s_step(Sf, S[m], Smin[m], Smin_sw[m]);
                if (l < 15) {
                    Lam32[m] = imcra_lambda32_step(Lam32[m], Y2f[m]);
                    lam[m] = (double)Lam32[m];
                } else {
                    I[m] = imcra_indicator(Y2, S[m], Smin[m]) ? 1.0 : 0.0;
                    const double IY = I[m] * Y2;
                    xd[NS_X_IY + k + 1] = IY;
                    xd[NS_X_I + k + 1] = I[m];
                    if (k == 0) { xd[NS_X_IY] = IY; xd[NS_X_I] = I[m]; }
                    if (k == NELE_NBINS - 1) { xd[NS_X_IY + NELE_NBINS + 1] = IY; xd[NS_X_I + NELE_NBINS + 1] = I[m]; }
                }
            }
        }
        if (l >= 15) {                                     // the indicator of every bin before the prior
            fftw_wave_sync();
            int slot, nst;
            const bool store = imcra_store_due(j, u, slot, nst);
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                if (m < nm) {
                    const int k = 64 * m + lane;
                    double w0, w1, w2;
                    imcra_smooth_weights(k, w0, w1, w2);
                    const double Y2 = (double)Y2f[m];
                    const double norm = imcra_smooth3(w0, w1, w2, xd[NS_X_I + k], xd[NS_X_I + k + 1], xd[NS_X_I + k + 2]);
                    const double tSf = imcra_smooth3(w0, w1, w2, xd[NS_X_IY + k], xd[NS_X_IY + k + 1], xd[NS_X_IY + k + 2]);
                    const double r = imcra_prior_step(Y2, S[m], tSf, norm, tS[m], tSmin[m], tSmin_sw[m]);
                    Lam64[m] = imcra_psd_step_p<false>(Y2, Gamma[m], xi[m], r, ovL[m], p[m]);
                    lam[m] = Lam64[m];
                    if (store) {                           // the minima store: the stream record
                        ring[slot * NS_NB + k] = Smin_sw[m];
                        ring[(8 + slot) * NS_NB + k] = tSmin_sw[m];
                        double mm = Smin_sw[m], tm = tSmin_sw[m];
                        for (int i = 0; i < nst; ++i) {
                            if (i == slot) continue;       // this frame's own store is in hand
                            mm = fmin(mm, ring[i * NS_NB + k]);
                            tm = fmin(tm, ring[(8 + i) * NS_NB + k]);
                        }
                        Smin[m] = mm; tSmin[m] = tm;
                        Smin_sw[m] = S[m]; tSmin_sw[m] = tS[m];
                    }
                }
            }
            imcra_advance(j, u);
            if (u >= 16) u -= 8;                           // only u mod 8 and min(u + 1, 8) are ever read
        }
        if (l < 16) ++l;                                   // only l == 0, l < 15 and l < 16 are ever read
        // ---- 4. the gain; ge = G E in the packed layout (slot 0 = (bin 0, bin 256), both real)
        double2 ge[4];
        double g_ny = 0.0;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            if (m < nm) {
                const int k = 64 * m + lane;
                const double nu = Gamma[m] * xi[m] / (1.0 + xi[m]);
                const double gh1 = fmin(G[m] * exp(0.5 * ns_e1(fmax(nu, NELE_NS_NU_MIN))), 1.0);   // G[m] = xi / (1 + xi)
                const double g = exp(p[m] * log(gh1) + (1.0 - p[m]) * ln_gmin);
                if (a.gains) a.gains[row + k] = g;
                if (a.noise_psd) a.noise_psd[row + k] = lam[m];
                if (a.presence) a.presence[row + k] = p[m];
                if (m < 4) ge[m] = make_double2(g * E[m].x, g * E[m].y);
                else g_ny = g * E[m].x;
            }
        }
        if (lane0) ge[0].y = g_ny;
        // ---- 5. o = w irfft512(G E); out = ola + o[0:256], ola <- o[256:512]
        fftw_wave_sync();                                  // every lane's reads of the smoothing rows precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) xw[64 * m + lane] = ge[m];
        fftw_wave_sync();
        const double2 g0 = xw[0];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = fftw_n(lane, r);
            const int k = ((n <= 256) ? n : 512 - n) & 255;
            v[r] = fft512_packed_join(xw[k], zero, g0, zero, n);
        }
        fftw_wave_sync();
        fft512_wave<true>(v, xw, tw, lane);                // v[m].x = 512 irfft(G E)[64 m + lane]
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            outb[col + 64 * m + lane] = (float)(ola[m] + wlo[m] * (v[m].x * (1.0 / 512.0)));
            ola[m] = whi[m] * (v[m + 4].x * (1.0 / 512.0));
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int n = 64 * m + lane;
        xprevp[n] = xp[m];
        olap[n] = ola[m];
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        if (m < nm) {
            const int k = 64 * m + lane;
            imd[NS_F_G * NS_NB + k] = G[m];
            imd[NS_F_GAMMA * NS_NB + k] = Gamma[m];
            imd[NS_F_LAM64 * NS_NB + k] = Lam64[m];
            imd[NS_F_S * NS_NB + k] = S[m];
            imd[NS_F_SMIN * NS_NB + k] = Smin[m];
            imd[NS_F_SMINSW * NS_NB + k] = Smin_sw[m];
            imd[NS_F_TS * NS_NB + k] = tS[m];
            imd[NS_F_TSMIN * NS_NB + k] = tSmin[m];
            imd[NS_F_TSMINSW * NS_NB + k] = tSmin_sw[m];
            imd[NS_F_OVL * NS_NB + k] = ovL[m];
            lam32p[k] = Lam32[m];
        }
    }
    if (lane0) { ctl[0] = l; ctl[1] = j; ctl[2] = u; }
}

int ns_check(const char* name, const void* state, long long state_bytes, int S) {
    return slot_state_check(name, state, state_bytes, S, []() -> int { return NELE_OK; }, nele_ns_state_bytes(S), "nele_ns_state_bytes");
}

// slots == null: every record; write_hdr: the header too
int ns_reset(const char* name, void* state, int S, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, (int)NS_REC_BYTES};
    return slot_state_reset(name, state, NS_HDR_BYTES, NS_REC_BYTES, S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_ns_state_bytes(int max_streams) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS) return -1;
    return NS_HDR_BYTES + (long long)max_streams * NS_REC_BYTES;
}

extern "C" long long nele_ns_stream_record_bytes(void) { return NS_REC_BYTES; }

extern "C" int nele_ns_init(void* state, long long state_bytes, int max_streams, void* stream) {
    int st = ns_check("nele_ns_init", state, state_bytes, max_streams);
    if (st) return st;
    return ns_reset("nele_ns_init", state, max_streams, nullptr, true, stream);
}

extern "C" int nele_ns_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream) {
    int st = ns_check("nele_ns_reset", state, state_bytes, max_streams);
    if (st) return st;
    return ns_reset("nele_ns_reset", state, max_streams, slots, false, stream);
}

extern "C" int nele_ns_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh, double gmin,
                           float* out, double* gains, double* noise_psd, double* presence, void* stream) {
    int st = ns_check("nele_ns_hop", state, state_bytes, max_streams);
    if (st) return st;
    NELE_CHECK_ARG(x && out, "nele_ns_hop: null x / out");
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "nele_ns_hop: nh=%d must be in 1 .. 1048576", nh);
    NELE_CHECK_ARG(gmin > 0.0 && gmin <= 1.0, "nele_ns_hop: gmin=%g must be in (0, 1]", gmin);
    NsArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.x = x;
    a.ld = (long long)nh * NS_BLK;
    a.active = active;
    a.nh = nh;
    a.gmin = gmin;
    a.out = out;
    a.gains = gains;
    a.noise_psd = noise_psd;
    a.presence = presence;
    hipLaunchKernelGGL(ns_hop_kernel, dim3((max_streams + NS_WAVES - 1) / NS_WAVES), dim3(64 * NS_WAVES), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH("nele_ns_hop");
    return NELE_OK;
}
