// Real-time, hop-by-hop enhancement of many concurrent streams (nele_rt_*): the causal form of the offline path
// (audio_util.py:53-65 STFT, :30-50 band energies, noise_est/imcra.py IMCRA, model.py:83-98 Generator_Conv1D_cLN, audio_util.py:76-110
// resynthesis), one 256-sample hop of every stream at a time.  Per hop, four kinds of launch ("Real-time enhancement"):
//   rt_front_kernel   one workgroup per stream: append the hop, FFT of the new clean + noise frame (one complex float64 transform),
//                     clean band ** 1/6, one IMCRA frame for all 257 bins, noise band ** 1/6 -> the generator's 128-wide input row
//   rt_layer_kernel   one launch per Conv1d layer: GEMM of (stream, frame) rows over the per-stream history ring; the layer's INPUT
//                     normalisation (cLN of the previous layer's raw output on the running float64 sums, LeakyReLU) is done by the consumer,
//                     so no cross-workgroup reduction is needed for the channel sums
//   rt_head_kernel    one workgroup per stream: cLN of the last layer, fc1 / fc2, exp(3.2 tanh), energy normalisation (prefix or fixed),
//                     then the resynthesis of one output hop (band-gain interpolation, iFFT, Hann window, overlap-add / window sum-square)
//   rt_rule_kernel    (nele_rt_rule_*) in place of the layer and head kernels: SII-optimal band gains (siiopt.h) on the front's row, then
//                     the head's course from the mask on - two launches per hop, no weights
// Every stream owns a fixed record of the state buffer; inactive or finished slots return at once.  A slot's arithmetic never depends on
// the other slots or on how its hops were grouped into calls: bit-reproducible per slot.
// This file is compiled with -ffp-contract=off (Makefile EXACT): the feature and IMCRA arithmetic mirrors numpy's operation order.
#include "common.h"
#include "fft512.h"
#include "featmath.h"
#include "imcra.h"
#include "slot_state.h"
#include "siiopt.h"
#include "../../include/nele_hip.h"

int siiopt_check(const char* name, const double* gamma, double lam, double strength);      // siiopt.hip

namespace {

// ---- generator geometry (model.py:43-82)
__host__ __device__ constexpr int rt_cin(int l) { return l == 0 ? 128 : 256; }
__host__ __device__ constexpr int rt_nout(int l) { return l == 5 ? 64 : 256; }
__host__ __device__ constexpr int rt_taps(int l) { return (l == 0 || l == 5) ? 5 : 7; }
__host__ __device__ constexpr long long rt_wsize(int l) { return (long long)rt_cin(l) * rt_nout(l) * rt_taps(l); }
// flat parameter offsets (floats) in nn.Module.parameters() order: per layer {weight [N][Cin][K], bias, gain0, bias0}, fc1.w, fc1.b, fc2.w, fc2.b
__host__ __device__ constexpr long long rt_poff(int l) {
    long long o = 0;
    for (int i = 0; i < l; ++i) o += rt_wsize(i) + 3LL * rt_nout(i);
    return o;
}
constexpr long long RT_FC1W = rt_poff(6), RT_FC1B = RT_FC1W + 4096, RT_FC2W = RT_FC1B + 64, RT_FC2B = RT_FC2W + 4096;
constexpr long long RT_NPARAMS = RT_FC2B + 64;
static_assert(RT_NPARAMS == 2093120, "generator parameter count");
// transposed convolution weights [K * Cin][N] (element (tap, c, n) at ((tap * Cin + c) * N + n)), float32 or bf16, one after the other
__host__ __device__ constexpr long long rt_woff(int l) {
    long long o = 0;
    for (int i = 0; i < l; ++i) o += rt_wsize(i);
    return o;
}
constexpr long long RT_NW = rt_woff(6);

// ---- state buffer: [weights area][stream record 0][stream record 1] ...
constexpr long long RT_W_BYTES = slot_al(4 * RT_NW);                  // conv weights (float32 size; bf16 uses the first half)
constexpr long long RT_P_BYTES = slot_al(4 * RT_NPARAMS);             // copy of the flat parameters (biases, cLN affine, fc)
constexpr long long RT_HDR_BYTES = RT_W_BYTES + RT_P_BYTES;

#define RT_RING 8                                                     // history frames kept per layer input (>= taps + 1)
#define RT_NB 260                                                     // bins padded
// per-stream record, byte offsets
struct RtHead {
    int hops;        // hops received
    int done;        // finish() ran: the slot ignores hops until reset
    int j, u;        // IMCRA minimum-tracking counters (imcra.py:452-481)
    int nf, f0;      // this launch sequence: new frames and the first of them
    int emit;        // this launch sequence emits an output hop
    int pad;
};
constexpr long long RT_O_HEAD = 0;
constexpr long long RT_O_CLN = 32;                                    // double [6][2][2]: running (sum, sum of squares) per layer, by frame parity
constexpr long long RT_O_NSUM = RT_O_CLN + 8 * 24;                    // double [2]: sum P, sum mask P (prefix normalisation)
constexpr long long RT_O_IMD = slot_al(RT_O_NSUM + 16);               // double [26][RT_NB]: IMCRA per-bin state
constexpr int RT_NIMD = 26;
constexpr long long RT_O_LAM32 = RT_O_IMD + 8LL * RT_NIMD * RT_NB;    // float [RT_NB]
constexpr long long RT_O_XR = slot_al(RT_O_LAM32 + 4 * RT_NB);        // float [2][3][256]: input ring (clean, noise) by hop % 3
constexpr long long RT_O_SPEC = RT_O_XR + 4 * 2 * 3 * 256;            // float2 [2][257]: clean spectrum by frame parity
constexpr long long RT_O_CB = slot_al(RT_O_SPEC + 8 * 2 * 257);       // float [2][64]: clean band ** 1/6 by frame parity
constexpr long long RT_O_A2 = RT_O_CB + 4 * 128;                      // float [2][64]: alpha^2 by frame parity
__host__ __device__ constexpr long long rt_act_off(int l) {            // float [RT_RING][Cin]: layer l's input rows by frame % RT_RING
    long long o = RT_O_A2 + 4 * 128;
    for (int i = 0; i < l; ++i) o += 4LL * RT_RING * rt_cin(i);
    return o;
}
__host__ __device__ constexpr long long rt_y_off(int l) {              // float [2][N]: layer l's raw output (conv + bias) by frame parity
    long long o = rt_act_off(6);
    for (int i = 0; i < l; ++i) o += 4LL * 2 * rt_nout(i);
    return o;
}
constexpr long long RT_REC_BYTES = slot_al(rt_y_off(6));

// IMCRA per-bin double fields
enum { IM_S = 0, IM_TS, IM_SMIN, IM_TSMIN, IM_SMINSW, IM_TSMINSW, IM_OVL, IM_LAM64, IM_G, IM_GAMMA, IM_ST = 10, IM_TST = 18 };

struct RtArgs {
    unsigned char* state;
    int S;                       // slots
    const float* clean;          // [S][ld] (hop at column offset 0) or null (finish: tails)
    const float* noise;
    long long ld;                // row stride of clean / noise / out
    const unsigned char* active; // [S] or null (all)
    const int* tail;             // finish: [S] samples of the last partial hop (< 0: not finishing); null in a hop launch
    const float* beta2;          // [S] fixed beta^2 or null (prefix normalisation)
    float* out;                  // [S][ld] (the hop's 256 columns at offset 0)
    float* dbg_band;             // [S][dbg_frames][64] each, or null
    float* dbg_noise;
    float* dbg_mask;
    float* dbg_alpha2;
    int dbg_frames;
};

__device__ __forceinline__ unsigned char* rt_rec(const RtArgs& a, int b) { return a.state + RT_HDR_BYTES + (size_t)b * RT_REC_BYTES; }
__device__ __forceinline__ RtHead* rt_head(unsigned char* r) { return reinterpret_cast<RtHead*>(r + RT_O_HEAD); }
__device__ __forceinline__ double* rt_cln(unsigned char* r, int l, int par) { return reinterpret_cast<double*>(r + RT_O_CLN) + (l * 2 + par) * 2; }
__device__ __forceinline__ float* rt_act(unsigned char* r, int l) { return reinterpret_cast<float*>(r + rt_act_off(l)); }
__device__ __forceinline__ float* rt_y(unsigned char* r, int l, int par) { return reinterpret_cast<float*>(r + rt_y_off(l)) + par * rt_nout(l); }

__device__ __forceinline__ float rt_bf16(float x) {       // round to nearest even bf16, as the MFMA operands of the bf16 mode
    return (float)(__bf16)x;
}

// ============================================================================================ front: features + IMCRA
#define RT_FRONT_THREADS 320
__global__ __launch_bounds__(RT_FRONT_THREADS) void rt_front_kernel(RtArgs a) {
    __shared__ Fft512Lds s;
    __shared__ float xc[NELE_NFFT], xn[NELE_NFFT];
    __shared__ double y2[NELE_NBINS + 2], sa[NELE_NBINS + 2], sb[NELE_NBINS + 2];
    __shared__ float pc[NELE_NBINS + 3], pn[NELE_NBINS + 3];
    __shared__ int ctl[4];
    const int b = blockIdx.x, k = threadIdx.x;
    if (b >= a.S) return;
    unsigned char* rec = rt_rec(a, b);
    RtHead* hd = rt_head(rec);
    const bool fin = a.tail != nullptr;
    float* xr = reinterpret_cast<float*>(rec + RT_O_XR);           // [2][3][256]
    // mode 0: nothing this launch (inactive, finished, or not finishing); 1: the stream's first hop (stored; its output columns are zeros);
    // 2: new frames.  A hop m >= 2 brings frame m; hop 1 brings frames 0 and 1 (frame 0's reflection needs x[256]); finish brings the
    // end-reflected frame n of a stream of n hops + r samples.  Every mode 2 launch emits output hop (newest frame - 1).
    if (k == 0) {
        int mode = 0, nf = 0, f0 = 0, L = -1;
        const int m = hd->hops;
        const bool act = !a.active || a.active[b];
        if (act && !hd->done) {
            if (fin) {
                const int r = a.tail[b];
                if (r >= 0 && r < NELE_HOP && m >= 2) { mode = 2; nf = 1; f0 = m; L = NELE_HOP * m + r; }
            } else if (m == 0) {
                mode = 1;
            } else {
                mode = 2; nf = (m == 1) ? 2 : 1; f0 = (m == 1) ? 0 : m;
            }
        }
        ctl[0] = mode; ctl[1] = nf; ctl[2] = f0; ctl[3] = L;
    }
    __syncthreads();
    const int mode = ctl[0], nf = ctl[1], f0 = ctl[2], L = ctl[3];
    const int emit = 1;
    if (mode == 0) {                                               // the later kernels of this launch sequence skip the slot
        if (k == 0) { hd->nf = 0; hd->emit = 0; }
        return;
    }
    if (mode == 1) {
        if (k < NELE_HOP) {
            xr[k] = a.clean[(size_t)b * a.ld + k];
            xr[768 + k] = a.noise[(size_t)b * a.ld + k];
            a.out[(size_t)b * a.ld + k] = 0.f;
        }
        if (k == 0) { hd->hops = 1; hd->nf = 0; hd->emit = 0; }
        return;
    }
    // ---- append the hop (or the zero-padded tail) to the input ring
    const int hslot = hd->hops % 3;
    if (k < NELE_HOP) {
        const bool in = !fin || k < a.tail[b];
        xr[hslot * 256 + k] = in ? a.clean[(size_t)b * a.ld + k] : 0.f;
        xr[768 + hslot * 256 + k] = in ? a.noise[(size_t)b * a.ld + k] : 0.f;
    }
    fft512_init_twiddles(s);
    // ---- IMCRA state of this bin (registers)
    const bool bin = k < NELE_NBINS;
    double* imd = reinterpret_cast<double*>(rec + RT_O_IMD);
    float* lam32p = reinterpret_cast<float*>(rec + RT_O_LAM32);
    auto IM = [&](int f) -> double& { return imd[f * RT_NB + (bin ? k : NELE_NBINS)]; };
    double S = 0, tS = 0, Smin = 0, tSmin = 0, Smin_sw = 0, tSmin_sw = 0, ovL = 0, Lam64 = 1e-6, G = 1.0, Gamma = 1.0;
    float Lam32 = 0.f;
    int j = 0, u = 0;
    if (f0 > 0) {
        S = IM(IM_S); tS = IM(IM_TS); Smin = IM(IM_SMIN); tSmin = IM(IM_TSMIN); Smin_sw = IM(IM_SMINSW); tSmin_sw = IM(IM_TSMINSW);
        ovL = IM(IM_OVL); Lam64 = IM(IM_LAM64); G = IM(IM_G); Gamma = IM(IM_GAMMA);
        Lam32 = lam32p[bin ? k : NELE_NBINS];
        j = hd->j; u = hd->u;
    }
    const bool edge_lo = (k == 0), edge_hi = (k == NELE_NBINS - 1);
    double w0, w1, w2;
    imcra_smooth_weights(k, w0, w1, w2);
    __syncthreads();                                               // ring written, twiddles ready

    float2* specr = reinterpret_cast<float2*>(rec + RT_O_SPEC);
    float* cbr = reinterpret_cast<float*>(rec + RT_O_CB);
    float* act0 = rt_act(rec, 0);
    for (int f = f0; f < f0 + nf; ++f) {
        // ---- frame f covers input samples [256 f - 256, 256 f + 256), reflected at 0 (and at the end L in finish)
        for (int n = k; n < NELE_NFFT; n += RT_FRONT_THREADS) {
            int o = NELE_HOP * f + n - NELE_HOP;
            if (o < 0) o = -o;
            if (L > 0 && o >= L) o = 2 * (L - 1) - o;
            const int hs = (o / NELE_HOP) % 3, idx = o % NELE_HOP;
            xc[n] = xr[hs * 256 + idx];
            xn[n] = xr[768 + hs * 256 + idx];
        }
        __syncthreads();
        for (int n = k; n < NELE_NFFT; n += RT_FRONT_THREADS) {
            const double w = hann512(n);
            s.x[fft512_brev(n)] = make_double2(w * (double)xc[n], w * (double)xn[n]);
        }
        __syncthreads();
        fft512_run<false>(s);
        float Y2f = 0.f;
        if (bin) {
            const double2 zk = s.x[k], zn = s.x[(NELE_NFFT - k) & (NELE_NFFT - 1)];
            double2 Ad, Bd;
            fft512_pair_split(zk, zn, Ad, Bd);
            const float2 A = make_float2((float)Ad.x, (float)Ad.y);
            const float2 Bv = make_float2((float)Bd.x, (float)Bd.y);
            specr[(f & 1) * NELE_NBINS + k] = A;
            const float m0 = np_cabsf(A.x, A.y), m1 = np_cabsf(Bv.x, Bv.y);
            pc[k] = m0 * m0;
            Y2f = m1 * m1;                                         // np.abs(complex64) ** 2 in float32
            y2[k + 1] = (double)Y2f;
            if (edge_lo) y2[0] = (double)Y2f;
            if (edge_hi) y2[NELE_NBINS + 1] = (double)Y2f;
        }
        __syncthreads();
        // ---- one IMCRA frame (the steps of imcra.h in imcra_band_kernel's order, state from the stream's record)
        const int l = f;
        float outv = 0.f;
        double xi = 0.0, I = 0.0;
        if (bin) {
            const double Y2 = (double)Y2f;
            const double Sf = imcra_smooth3(w0, w1, w2, y2[k], y2[k + 1], y2[k + 2]);
            xi = imcra_snr_step(l, Y2f, Lam64, Lam32, G, Gamma);
            if (l == 0) {
                S = Sf; tS = Sf; Smin = Sf; tSmin = Sf; Smin_sw = Sf; tSmin_sw = Sf;
                ovL = Y2;
                Lam32 = Y2f;
            }
            imcra_s_step(Sf, S, Smin, Smin_sw);
            if (l < 15) {
                Lam32 = imcra_lambda32_step(Lam32, Y2f);
                outv = Lam32;
            } else {
                I = imcra_indicator(Y2, S, Smin) ? 1.0 : 0.0;
            }
        }
        if (l >= 15) {                                             // the indicator of every bin before the prior: one barrier
            if (bin) {
                const double IY = I * (double)Y2f;
                sa[k + 1] = IY;
                sb[k + 1] = I;
                if (edge_lo) { sa[0] = IY; sb[0] = I; }
                if (edge_hi) { sa[NELE_NBINS + 1] = IY; sb[NELE_NBINS + 1] = I; }
            }
            __syncthreads();
            if (bin) {
                const double Y2 = (double)Y2f;
                const double norm = imcra_smooth3(w0, w1, w2, sb[k], sb[k + 1], sb[k + 2]);
                const double tSf = imcra_smooth3(w0, w1, w2, sa[k], sa[k + 1], sa[k + 2]);
                const double r = imcra_prior_step(Y2, S, tSf, norm, tS, tSmin, tSmin_sw);
                Lam64 = imcra_psd_step(Y2, Gamma, xi, r, ovL);
                outv = (float)Lam64;
                int slot, nst;
                if (imcra_store_due(j, u, slot, nst)) {            // the minima store: the stream record
                    IM(IM_ST + slot) = Smin_sw;
                    IM(IM_TST + slot) = tSmin_sw;
                    double mm = IM(IM_ST), tm = IM(IM_TST);
                    for (int i = 1; i < nst; ++i) { mm = fmin(mm, IM(IM_ST + i)); tm = fmin(tm, IM(IM_TST + i)); }
                    Smin = mm; tSmin = tm;
                    Smin_sw = S; tSmin_sw = tS;
                }
            }
            imcra_advance(j, u);
        }
        if (bin) {
            const float r = sqrtf(outv);                           // band feature of sqrt(PSD) (audio_util.py:446-451)
            pn[k] = r * r;
        }
        __syncthreads();
        if (k < 2 * NELE_NBANDS) {
            const int i = k & 63;
            const float e = (k < NELE_NBANDS) ? band_energy(pc, i) : band_energy(pn, i);
            const float v = nele_pow_f32(e, (float)(1.0 / 6.0));
            float* row = act0 + (f % RT_RING) * 128;
            row[k] = v;                                            // the bf16 mode rounds it where the layer stages it
            if (k < NELE_NBANDS) cbr[(f & 1) * 64 + i] = v;
            float* dbg = (k < NELE_NBANDS) ? a.dbg_band : a.dbg_noise;
            if (dbg && f < a.dbg_frames) dbg[((size_t)b * a.dbg_frames + f) * 64 + i] = v;
        }
        __syncthreads();                                           // xc / xn / s / y2 / pc / pn are rewritten by the next frame
    }
    // ---- state back
    if (bin) {
        IM(IM_S) = S; IM(IM_TS) = tS; IM(IM_SMIN) = Smin; IM(IM_TSMIN) = tSmin; IM(IM_SMINSW) = Smin_sw; IM(IM_TSMINSW) = tSmin_sw;
        IM(IM_OVL) = ovL; IM(IM_LAM64) = Lam64; IM(IM_G) = G; IM(IM_GAMMA) = Gamma;
        lam32p[k] = Lam32;
    }
    if (k == 0) {
        hd->j = j; hd->u = u;
        hd->nf = nf; hd->f0 = f0; hd->emit = emit;
        hd->hops = hd->hops + 1;
        if (fin) hd->done = 1;
    }
}

// ============================================================================================ generator layers
// grid (ceil(S / RT_SB), N / 64), block 256: 4 streams x up to 2 new frames = 8 rows; thread = (output channel, quarter of the reduction)
#define RT_SB 4
#define RT_ROWS 8
template <int LAYER, bool BF16>
__global__ __launch_bounds__(256) void rt_layer_kernel(RtArgs a, const void* __restrict__ wt, const float* __restrict__ params) {
    constexpr int CIN = rt_cin(LAYER), NOUT = rt_nout(LAYER), KT = rt_taps(LAYER), KTOT = KT * CIN;
    __shared__ float xs[RT_ROWS * KTOT];
    __shared__ int rs[RT_ROWS], rf[RT_ROWS], nrows_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s0 = blockIdx.x * RT_SB;
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < RT_SB; ++i) {
            const int b = s0 + i;
            if (b >= a.S) break;
            const RtHead* hd = rt_head(rt_rec(a, b));
            for (int d = 0; d < hd->nf; ++d) { rs[n] = i; rf[n] = hd->f0 + d; ++n; }
        }
        nrows_s = n;
    }
    __syncthreads();
    const int nrows = nrows_s;
    if (nrows == 0) return;
    // ---- the new frames' input rows (LAYER >= 1): cLN of the previous layer's raw output on the running float64 sums, LeakyReLU(0.3)
    if (LAYER >= 1) {
        const int b = s0 + wv;
        if (b < a.S) {
            unsigned char* rec = rt_rec(a, b);
            const RtHead* hd = rt_head(rec);
            const int nf = hd->nf, f0 = hd->f0;
            if (nf > 0) {
                double Ssum = 0.0, Qsum = 0.0;
                if (f0 > 0) { const double* c = rt_cln(rec, LAYER - 1, (f0 - 1) & 1); Ssum = c[0]; Qsum = c[1]; }
                const float* gain = params + rt_poff(LAYER - 1) + rt_wsize(LAYER - 1) + CIN;
                const float* bias = gain + CIN;
                float* ring = rt_act(rec, LAYER);
                for (int f = f0; f < f0 + nf; ++f) {
                    const float* y = rt_y(rec, LAYER - 1, f & 1);
                    float v[CIN / 64];
                    double sl = 0.0, ql = 0.0;
#pragma unroll
                    for (int i = 0; i < CIN / 64; ++i) {
                        v[i] = y[lane + 64 * i];
                        sl += (double)v[i];
                        ql += (double)v[i] * (double)v[i];
                    }
                    Ssum += wave_sum(sl);
                    Qsum += wave_sum(ql);
                    const double n = (double)CIN * (double)(f + 1);   // model.py:188-199
                    const double m = Ssum / n;
                    const double var = (Qsum - 2.0 * m * Ssum) / n + m * m;
                    const float mean = (float)m, rstd = (float)(1.0 / sqrt(var + 1e-8));
#pragma unroll
                    for (int i = 0; i < CIN / 64; ++i) {
                        const int c = lane + 64 * i;
                        float o = (v[i] - mean) * rstd * gain[c] + bias[c];
                        o = o > 0.f ? o : 0.3f * o;
                        if (BF16) o = rt_bf16(o);
                        for (int r = 0; r < nrows; ++r) {
                            const int tap = f - rf[r] + KT - 1;
                            if (rs[r] == wv && tap >= 0 && tap < KT) xs[r * KTOT + tap * CIN + c] = o;
                        }
                        if (blockIdx.y == 0) ring[(f % RT_RING) * CIN + c] = o;
                    }
                }
                if (blockIdx.y == 0 && lane == 0) { double* c = rt_cln(rec, LAYER - 1, (f0 + nf - 1) & 1); c[0] = Ssum; c[1] = Qsum; }
            }
        }
    }
    // ---- the older frames from the history ring (zeros before the first frame: Chomp1d's causal padding)
    for (int r = 0; r < nrows; ++r) {
        unsigned char* rec = rt_rec(a, s0 + rs[r]);
        const int f0 = rt_head(rec)->f0;
        const float* ring = rt_act(rec, LAYER);
        for (int e = tid; e < KTOT; e += 256) {
            const int tap = e / CIN, c = e - tap * CIN;
            const int src = rf[r] - (KT - 1) + tap;
            if (LAYER >= 1 && src >= f0) continue;                   // written above
            float v = 0.f;
            if (src >= 0) {
                v = ring[(src % RT_RING) * CIN + c];
                if (BF16 && LAYER == 0) v = rt_bf16(v);
            }
            xs[r * KTOT + e] = v;
        }
    }
    __syncthreads();
    // ---- GEMM: channel n, reduction quarter wv
    const int n = blockIdx.y * 64 + lane;
    constexpr int KQ = KTOT / 4;
    float acc[RT_ROWS];
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) acc[r] = 0.f;
    const int k0 = wv * KQ;
#pragma unroll 16
    for (int kk = 0; kk < KQ; ++kk) {                                // (unrolled: 16 weight loads in flight; the sums keep their order)
        const int kx = k0 + kk;
        float w;
        if (BF16) {
            const unsigned short h = reinterpret_cast<const unsigned short*>(wt)[(size_t)kx * NOUT + n];
            w = __uint_as_float((unsigned)h << 16);
        } else {
            w = reinterpret_cast<const float*>(wt)[(size_t)kx * NOUT + n];
        }
#pragma unroll
        for (int r = 0; r < RT_ROWS; ++r)
            if (r < nrows) acc[r] = __builtin_fmaf(w, xs[r * KTOT + kx], acc[r]);
    }
    __syncthreads();
    float* part = xs;                                                // [4][RT_ROWS][64]
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) part[(wv * RT_ROWS + r) * 64 + lane] = acc[r];
    __syncthreads();
    if (wv == 0) {
        const float bias = params[rt_poff(LAYER) + rt_wsize(LAYER) + n];
        for (int r = 0; r < nrows; ++r) {
            float y = part[(0 * RT_ROWS + r) * 64 + lane] + part[(1 * RT_ROWS + r) * 64 + lane];
            y = y + part[(2 * RT_ROWS + r) * 64 + lane];
            y = y + part[(3 * RT_ROWS + r) * 64 + lane];
            y = y + bias;
            rt_y(rt_rec(a, s0 + rs[r]), LAYER, rf[r] & 1)[n] = y;
        }
    }
}

// ============================================================================================ from the mask on (head and rule kernels)
// Frame f of slot b, wave 0, lane = band: the mask value mk -> alpha^2 by the prefix or the fixed normalisation, into the record's
// alpha^2 row of the frame's parity and the debug outputs.  SP / SMP: the slot's running float64 sums (prefix normalisation).
__device__ __forceinline__ void rt_mask_tail(const RtArgs& a, int b, int f, int lane, float mk, const float* cbr, float* a2r, double& SP,
                                             double& SMP) {
    float a2;
    if (a.beta2) {
        a2 = mk * a.beta2[b];
    } else {                                                 // prefix energy normalisation, float64 running sums
        const double p = (double)nele_powi_f32(cbr[(f & 1) * 64 + lane], 6.0f);
        SP += wave_sum(p);
        SMP += wave_sum((double)mk * p);
        const double ratio = SMP > 0.0 ? SP / SMP : 1.0;
        a2 = (float)((double)mk * ratio);
    }
    a2r[(f & 1) * 64 + lane] = a2;
    if (a.dbg_mask && f < a.dbg_frames) a.dbg_mask[((size_t)b * a.dbg_frames + f) * 64 + lane] = mk;
    if (a.dbg_alpha2 && f < a.dbg_frames) a.dbg_alpha2[((size_t)b * a.dbg_frames + f) * 64 + lane] = a2;
}

// Output hop fa = fb - 1 of slot b, fb the newest frame: second half of frame fa + first half of frame fb (features.hip
// gain_istft_kernel).  The whole workgroup of 256 threads, after a barrier behind the last rt_mask_tail.
__device__ __forceinline__ void rt_resynth(const RtArgs& a, int b, const unsigned char* rec, Fft512Lds& s, int tid, int fb) {
    const int fa = fb - 1;
    const float* a2r = reinterpret_cast<const float*>(rec + RT_O_A2);
    const float* a2a = a2r + (fa & 1) * 64;
    const float* a2b = a2r + (fb & 1) * 64;
    const float2* specr = reinterpret_cast<const float2*>(rec + RT_O_SPEC);
    const float2* Xa = specr + (fa & 1) * NELE_NBINS;
    const float2* Xb = specr + (fb & 1) * NELE_NBINS;
    fft512_init_twiddles(s);
    for (int kk = tid; kk < NELE_NBINS; kk += 256) {
        const double ga = band_gain_sqrt(a2a, kk), gb = band_gain_sqrt(a2b, kk);
        const float2 xa = Xa[kk], xb = Xb[kk];
        double ar = ga * (double)xa.x, ai = ga * (double)xa.y;
        double br = gb * (double)xb.x, bi = gb * (double)xb.y;
        if (kk == 0 || kk == NELE_NBINS - 1) { ai = 0.0; bi = 0.0; }
        s.x[fft512_brev(kk)] = make_double2(ar - bi, ai + br);
        if (kk >= 1 && kk <= 255) s.x[fft512_brev(NELE_NFFT - kk)] = make_double2(ar + bi, br - ai);
    }
    __syncthreads();
    fft512_run<true>(s);
    {
        const int n = tid;
        const double x1 = s.x[n + 256].x * (1.0 / 512.0);
        const double x2 = s.x[n].y * (1.0 / 512.0);
        a.out[(size_t)b * a.ld + n] = istft_ola(x1, x2, hann512(n + 256), hann512(n));
    }
}

// ============================================================================================ head + normalisation + resynthesis
template <bool BF16>
__global__ __launch_bounds__(256) void rt_head_kernel(RtArgs a, const float* __restrict__ params) {
    __shared__ Fft512Lds s;
    __shared__ float h1[64], h2[64], msk[64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (b >= a.S) return;
    unsigned char* rec = rt_rec(a, b);
    const RtHead* hd = rt_head(rec);
    const int nf = hd->nf, f0 = hd->f0, emit = hd->emit;
    if (nf == 0) return;
    float* cbr = reinterpret_cast<float*>(rec + RT_O_CB);
    float* a2r = reinterpret_cast<float*>(rec + RT_O_A2);
    double* nsum = reinterpret_cast<double*>(rec + RT_O_NSUM);
    double Ssum = 0.0, Qsum = 0.0, SP = 0.0, SMP = 0.0;
    if (f0 > 0) { const double* c = rt_cln(rec, 5, (f0 - 1) & 1); Ssum = c[0]; Qsum = c[1]; SP = nsum[0]; SMP = nsum[1]; }
    const float* gain = params + rt_poff(5) + rt_wsize(5) + 64;
    const float* bias = gain + 64;
    for (int f = f0; f < f0 + nf; ++f) {
        if (tid < 64) {                                              // cLN of the last layer, LeakyReLU (model.py:91)
            const float v = rt_y(rec, 5, f & 1)[lane];
            Ssum += wave_sum((double)v);
            Qsum += wave_sum((double)v * (double)v);
            const double n = 64.0 * (double)(f + 1);
            const double m = Ssum / n;
            const double var = (Qsum - 2.0 * m * Ssum) / n + m * m;
            const float mean = (float)m, rstd = (float)(1.0 / sqrt(var + 1e-8));
            float o = (v - mean) * rstd * gain[lane] + bias[lane];
            o = o > 0.f ? o : 0.3f * o;
            h1[lane] = BF16 ? rt_bf16(o) : o;
        }
        __syncthreads();
        if (tid < 64) {                                              // fc1, LeakyReLU (model.py:94-95)
            const float* w = params + RT_FC1W + lane * 64;
            float o = 0.f;
            for (int i = 0; i < 64; ++i) o = __builtin_fmaf(BF16 ? rt_bf16(w[i]) : w[i], h1[i], o);
            o = o + params[RT_FC1B + lane];
            o = o > 0.f ? o : 0.3f * o;
            h2[lane] = BF16 ? rt_bf16(o) : o;
        }
        __syncthreads();
        if (tid < 64) {                                              // fc2, exp(3.2 tanh) (model.py:96-98)
            const float* w = params + RT_FC2W + lane * 64;
            float o = 0.f;
            for (int i = 0; i < 64; ++i) o = __builtin_fmaf(BF16 ? rt_bf16(w[i]) : w[i], h2[i], o);
            o = o + params[RT_FC2B + lane];
            const float mk = expf(3.2f * tanhf(o));
            msk[lane] = mk;
            rt_mask_tail(a, b, f, lane, mk, cbr, a2r, SP, SMP);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* c = rt_cln(rec, 5, (f0 + nf - 1) & 1);
        c[0] = Ssum; c[1] = Qsum;
        nsum[0] = SP; nsum[1] = SMP;
    }
    if (!emit) return;
    rt_resynth(a, b, rec, s, tid, f0 + nf - 1);
}

// ============================================================================================ the rule in the generator's place
// SII-optimal band gains (siiopt.h) on the front's 128-wide row, then rt_head_kernel's course from the mask on.
// One workgroup per stream; wave 0 runs the frames (lane = band).  Sbar [64] float64 is the rule's only state: it lies where the
// generator's layer-1 history ring does, which nothing touches in this mode (nele_rt_reset zeroes it with the record).
constexpr long long RT_O_SBAR = rt_act_off(1);
static_assert(RT_O_SBAR % 8 == 0 && RT_O_SBAR + 8 * 64 <= rt_act_off(2), "Sbar inside the idle layer-1 ring");
__global__ __launch_bounds__(256) void rt_rule_kernel(RtArgs a, const double* __restrict__ gamma, double lam, double strength) {
    __shared__ Fft512Lds s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (b >= a.S) return;
    unsigned char* rec = rt_rec(a, b);
    const RtHead* hd = rt_head(rec);
    const int nf = hd->nf, f0 = hd->f0, emit = hd->emit;
    if (nf == 0) return;
    if (tid < 64) {
        const float* cbr = reinterpret_cast<const float*>(rec + RT_O_CB);
        float* a2r = reinterpret_cast<float*>(rec + RT_O_A2);
        double* nsum = reinterpret_cast<double*>(rec + RT_O_NSUM);
        double* sbar = reinterpret_cast<double*>(rec + RT_O_SBAR);
        const float* act0 = rt_act(rec, 0);
        const double g = gamma[lane];
        double SP = 0.0, SMP = 0.0, Sbar = 0.0;
        if (f0 > 0) { SP = nsum[0]; SMP = nsum[1]; Sbar = sbar[lane]; }
        for (int f = f0; f < f0 + nf; ++f) {
            const float* row = act0 + (f % RT_RING) * 128;
            const float mk = siiopt_frame(Sbar, row[lane], row[64 + lane], g, f, lam, strength);
            rt_mask_tail(a, b, f, lane, mk, cbr, a2r, SP, SMP);
        }
        sbar[lane] = Sbar;
        if (tid == 0) { nsum[0] = SP; nsum[1] = SMP; }
    }
    if (!emit) return;
    __syncthreads();
    rt_resynth(a, b, rec, s, tid, f0 + nf - 1);
}

// ============================================================================================ weights, reset
// conv weight [N][Cin][K] -> [K * Cin][N] (float32, or bf16 rounded to nearest even)
__global__ void rt_weights_kernel(const float* __restrict__ params, unsigned char* __restrict__ state, int bf16) {
    float* pcopy = reinterpret_cast<float*>(state + RT_W_BYTES);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < RT_NPARAMS; i += (long long)gridDim.x * blockDim.x) pcopy[i] = params[i];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < RT_NW; i += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        while (l < 5 && i >= rt_woff(l + 1)) ++l;
        const long long e = i - rt_woff(l);
        const int Cin = rt_cin(l), N = rt_nout(l), K = rt_taps(l);
        const int n = (int)(e % N), kc = (int)(e / N), tap = kc / Cin, c = kc - tap * Cin;
        const float w = params[rt_poff(l) + ((long long)n * Cin + c) * K + tap];
        if (bf16) {
            const __bf16 h = (__bf16)w;
            reinterpret_cast<unsigned short*>(state)[i] = *reinterpret_cast<const unsigned short*>(&h);
        } else {
            reinterpret_cast<float*>(state)[i] = w;
        }
    }
}

int rt_check(const char* name, void* state, long long state_bytes, int S, int prec) {
    if (int st = slot_state_check(name, state, state_bytes, S, [] { return NELE_OK; }, nele_rt_state_bytes(S), "nele_rt_state_bytes")) return st;
    NELE_CHECK_ARG(prec == NELE_PREC_F32 || prec == NELE_PREC_BF16, "%s: precision=%d (0: f32, 1: bf16)", name, prec);
    return NELE_OK;
}

template <bool BF16>
void rt_launch_chain(const RtArgs& a, hipStream_t st) {
    const unsigned char* w = a.state;
    const float* params = reinterpret_cast<const float*>(a.state + RT_W_BYTES);
    const size_t es = BF16 ? 2 : 4;
    const unsigned gx = (unsigned)((a.S + RT_SB - 1) / RT_SB);
    hipLaunchKernelGGL(rt_front_kernel, dim3(a.S), dim3(RT_FRONT_THREADS), 0, st, a);
    hipLaunchKernelGGL((rt_layer_kernel<0, BF16>), dim3(gx, rt_nout(0) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(0)), params);
    hipLaunchKernelGGL((rt_layer_kernel<1, BF16>), dim3(gx, rt_nout(1) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(1)), params);
    hipLaunchKernelGGL((rt_layer_kernel<2, BF16>), dim3(gx, rt_nout(2) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(2)), params);
    hipLaunchKernelGGL((rt_layer_kernel<3, BF16>), dim3(gx, rt_nout(3) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(3)), params);
    hipLaunchKernelGGL((rt_layer_kernel<4, BF16>), dim3(gx, rt_nout(4) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(4)), params);
    hipLaunchKernelGGL((rt_layer_kernel<5, BF16>), dim3(gx, rt_nout(5) / 64), dim3(256), 0, st, a, (const void*)(w + es * rt_woff(5)), params);
    hipLaunchKernelGGL((rt_head_kernel<BF16>), dim3(a.S), dim3(256), 0, st, a, params);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_rt_state_bytes(int max_streams) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS) return -1;
    return RT_HDR_BYTES + (long long)max_streams * RT_REC_BYTES;
}

extern "C" long long nele_rt_stream_record_bytes(void) { return RT_REC_BYTES; }

extern "C" int nele_rt_set_weights(void* state, long long state_bytes, int max_streams, const float* params_flat, int precision, void* stream) {
    int st = rt_check("nele_rt_set_weights", state, state_bytes, max_streams, precision);
    if (st) return st;
    NELE_CHECK_ARG(params_flat, "nele_rt_set_weights: null params_flat");
    hipLaunchKernelGGL(rt_weights_kernel, dim3(1024), dim3(256), 0, as_stream(stream), params_flat, (unsigned char*)state, precision == NELE_PREC_BF16 ? 1 : 0);
    NELE_CHECK_LAUNCH("nele_rt_set_weights");
    return NELE_OK;
}

extern "C" int nele_rt_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream) {
    int st = rt_check("nele_rt_reset", state, state_bytes, max_streams, NELE_PREC_F32);
    if (st) return st;
    // no header write: what precedes the records here is the weights area
    return slot_state_reset("nele_rt_reset", state, RT_HDR_BYTES, RT_REC_BYTES, max_streams, slots, 0, nullptr, stream);
}

extern "C" int nele_rt_init(void* state, long long state_bytes, int max_streams, const float* params_flat, int precision, void* stream) {
    int st = rt_check("nele_rt_init", state, state_bytes, max_streams, precision);
    if (st) return st;
    NELE_CHECK_ARG(params_flat, "nele_rt_init: null params_flat");
    st = nele_rt_set_weights(state, state_bytes, max_streams, params_flat, precision, stream);
    if (st) return st;
    return nele_rt_reset(state, state_bytes, max_streams, nullptr, stream);
}

extern "C" int nele_rt_hop(void* state, long long state_bytes, int max_streams, int precision, const float* clean, const float* noise,
                           const unsigned char* active, int nh, const float* beta2, float* out, float* dbg_band, float* dbg_noise, float* dbg_mask,
                           float* dbg_alpha2, int dbg_frames, void* stream) {
    int st = rt_check("nele_rt_hop", state, state_bytes, max_streams, precision);
    if (st) return st;
    NELE_CHECK_ARG(clean && noise && out, "nele_rt_hop: null clean / noise / out");
    NELE_CHECK_ARG(nh >= 1, "nele_rt_hop: nh=%d must be >= 1", nh);
    NELE_CHECK_ARG(dbg_frames >= 0 && (dbg_frames > 0 || !(dbg_band || dbg_noise || dbg_mask || dbg_alpha2)),
                   "nele_rt_hop: dbg_frames=%d with debug outputs", dbg_frames);
    RtArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.ld = (long long)nh * NELE_HOP;
    a.active = active;
    a.beta2 = beta2;
    a.dbg_band = dbg_band; a.dbg_noise = dbg_noise; a.dbg_mask = dbg_mask; a.dbg_alpha2 = dbg_alpha2; a.dbg_frames = dbg_frames;
    for (int h = 0; h < nh; ++h) {
        a.clean = clean + (size_t)h * NELE_HOP;
        a.noise = noise + (size_t)h * NELE_HOP;
        a.out = out + (size_t)h * NELE_HOP;
        if (precision == NELE_PREC_BF16) rt_launch_chain<true>(a, as_stream(stream));
        else rt_launch_chain<false>(a, as_stream(stream));
    }
    NELE_CHECK_LAUNCH("nele_rt_hop");
    return NELE_OK;
}

extern "C" int nele_rt_finish(void* state, long long state_bytes, int max_streams, int precision, const float* clean_tail, const float* noise_tail,
                              const int* tail_lengths, const float* beta2, float* out, float* dbg_band, float* dbg_noise, float* dbg_mask,
                              float* dbg_alpha2, int dbg_frames, void* stream) {
    int st = rt_check("nele_rt_finish", state, state_bytes, max_streams, precision);
    if (st) return st;
    NELE_CHECK_ARG(clean_tail && noise_tail && tail_lengths && out, "nele_rt_finish: null clean_tail / noise_tail / tail_lengths / out");
    NELE_CHECK_ARG(dbg_frames >= 0 && (dbg_frames > 0 || !(dbg_band || dbg_noise || dbg_mask || dbg_alpha2)),
                   "nele_rt_finish: dbg_frames=%d with debug outputs", dbg_frames);
    RtArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.ld = NELE_HOP;
    a.clean = clean_tail;
    a.noise = noise_tail;
    a.tail = tail_lengths;
    a.beta2 = beta2;
    a.out = out;
    a.dbg_band = dbg_band; a.dbg_noise = dbg_noise; a.dbg_mask = dbg_mask; a.dbg_alpha2 = dbg_alpha2; a.dbg_frames = dbg_frames;
    if (precision == NELE_PREC_BF16) rt_launch_chain<true>(a, as_stream(stream));
    else rt_launch_chain<false>(a, as_stream(stream));
    NELE_CHECK_LAUNCH("nele_rt_finish");
    return NELE_OK;
}

// ---- the rule in the generator's place (include/nele_hip_ext5.h): rt_front_kernel, then rt_rule_kernel - two launches per hop
extern "C" int nele_rt_rule_hop(void* state, long long state_bytes, int max_streams, const double* gamma, double lam, double strength,
                                const float* clean, const float* noise, const unsigned char* active, int nh, const float* beta2, float* out,
                                float* dbg_band, float* dbg_noise, float* dbg_mask, float* dbg_alpha2, int dbg_frames, void* stream) {
    int st = rt_check("nele_rt_rule_hop", state, state_bytes, max_streams, NELE_PREC_F32);
    if (st) return st;
    if ((st = siiopt_check("nele_rt_rule_hop", gamma, lam, strength))) return st;
    NELE_CHECK_ARG(clean && noise && out, "nele_rt_rule_hop: null clean / noise / out");
    NELE_CHECK_ARG(nh >= 1, "nele_rt_rule_hop: nh=%d must be >= 1", nh);
    NELE_CHECK_ARG(dbg_frames >= 0 && (dbg_frames > 0 || !(dbg_band || dbg_noise || dbg_mask || dbg_alpha2)),
                   "nele_rt_rule_hop: dbg_frames=%d with debug outputs", dbg_frames);
    RtArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.ld = (long long)nh * NELE_HOP;
    a.active = active;
    a.beta2 = beta2;
    a.dbg_band = dbg_band; a.dbg_noise = dbg_noise; a.dbg_mask = dbg_mask; a.dbg_alpha2 = dbg_alpha2; a.dbg_frames = dbg_frames;
    for (int h = 0; h < nh; ++h) {
        a.clean = clean + (size_t)h * NELE_HOP;
        a.noise = noise + (size_t)h * NELE_HOP;
        a.out = out + (size_t)h * NELE_HOP;
        hipLaunchKernelGGL(rt_front_kernel, dim3(a.S), dim3(RT_FRONT_THREADS), 0, as_stream(stream), a);
        hipLaunchKernelGGL(rt_rule_kernel, dim3(a.S), dim3(256), 0, as_stream(stream), a, gamma, lam, strength);
    }
    NELE_CHECK_LAUNCH("nele_rt_rule_hop");
    return NELE_OK;
}

extern "C" int nele_rt_rule_finish(void* state, long long state_bytes, int max_streams, const double* gamma, double lam, double strength,
                                   const float* clean_tail, const float* noise_tail, const int* tail_lengths, const float* beta2, float* out,
                                   float* dbg_band, float* dbg_noise, float* dbg_mask, float* dbg_alpha2, int dbg_frames, void* stream) {
    int st = rt_check("nele_rt_rule_finish", state, state_bytes, max_streams, NELE_PREC_F32);
    if (st) return st;
    if ((st = siiopt_check("nele_rt_rule_finish", gamma, lam, strength))) return st;
    NELE_CHECK_ARG(clean_tail && noise_tail && tail_lengths && out, "nele_rt_rule_finish: null clean_tail / noise_tail / tail_lengths / out");
    NELE_CHECK_ARG(dbg_frames >= 0 && (dbg_frames > 0 || !(dbg_band || dbg_noise || dbg_mask || dbg_alpha2)),
                   "nele_rt_rule_finish: dbg_frames=%d with debug outputs", dbg_frames);
    RtArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.ld = NELE_HOP;
    a.clean = clean_tail;
    a.noise = noise_tail;
    a.tail = tail_lengths;
    a.beta2 = beta2;
    a.out = out;
    a.dbg_band = dbg_band; a.dbg_noise = dbg_noise; a.dbg_mask = dbg_mask; a.dbg_alpha2 = dbg_alpha2; a.dbg_frames = dbg_frames;
    hipLaunchKernelGGL(rt_front_kernel, dim3(a.S), dim3(RT_FRONT_THREADS), 0, as_stream(stream), a);
    hipLaunchKernelGGL(rt_rule_kernel, dim3(a.S), dim3(256), 0, as_stream(stream), a, gamma, lam, strength);
    NELE_CHECK_LAUNCH("nele_rt_rule_finish");
    return NELE_OK;
}
