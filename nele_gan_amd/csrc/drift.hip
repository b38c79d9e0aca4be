// Clock drift between playback and capture, followed ahead of the echo canceller (nele_drift_*, include/nele_hip_ext2.h): per stream
// slot a fractional, moving delay line that stands where the bulk search's whole-hop delay line stands.  `played` is handed on late by
// tau(t) samples through a 65 x 64 table of Kaiser-windowed sincs (neighbouring rows blended linearly); tau and its rate follow a
// second-order loop on the phase slope between a fast and a slow average of the SCOT-weighted cross-spectrum of the microphone against
// the slot's own output.  256-sample hops, 512-point float64 transforms (fft512.h), the packed spectra of csrc/aec.hip (256 double2:
// slot k = bin k, slot 0 = (bin 0, bin 256), products component-wise in slot 0).  The arithmetic is DESIGN.md section 19;
// tests/drift_ref.py restates it in numpy.
//   drift_table_kernel    : nele_drift_init's table, 65 workgroups of 64 threads
//   drift_hop_kernel      : one workgroup of 256 threads per stream and call, looping over the call's hops
//   drift_set_rate_kernel : one thread per slot
//   drift_status_kernel   : one thread per slot
//   drift_taps_kernel     : the table, copied out
// Every operand is the stream's own, every sum has a fixed order: a slot's bits do not depend on the hop grouping, on B or on the other
// slots.  State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "../../include/nele_hip_ext.h"
#include "../../include/nele_hip_ext2.h"

namespace {

constexpr int DR_BLK = 256;                                // samples per hop = slots per spectrum
constexpr int DR_ROWS = NELE_DRIFT_PHASES + 1;
constexpr int DR_K = NELE_DRIFT_TAPS;
constexpr int DR_LEAD = DR_K / 2 - 1;                      // 31: the table's centre tap, and TAU_MIN
static_assert(NELE_DRIFT_PHASES == 64 && DR_K == 64, "q = (t - 31) 64 is split with a shift and a mask; the table fills 33 280 bytes of LDS");
constexpr long long DR_TABLE_BYTES = 8LL * DR_ROWS * DR_K;                       // 33 280
constexpr long long DR_O_TABLE = SLOT_GEOM_HDR_BYTES;                            // int [0] = max_streams, [1] = blocks ahead of it
constexpr long long DR_HDR_BYTES = slot_al(DR_O_TABLE + DR_TABLE_BYTES);
// per-stream record, byte offsets.  A cleared record is a fresh slot, so the base the slot last took is kept plus one (0 = none).
constexpr long long DR_O_META = 0;                         // int [16]: DR_M_*
constexpr long long DR_O_LOOP = 64;                        // double [3]: tau, rate, delta
constexpr long long DR_O_UPREV = 256;                      // float [256]: the previous output hop
constexpr long long DR_O_SD = DR_O_UPREV + 4 * DR_BLK;     // double [257 (+ 7)]: S_d
constexpr long long DR_O_SU = DR_O_SD + 8 * 264;           // double [257 (+ 7)]: S_u
constexpr long long DR_O_CF = DR_O_SU + 8 * 264;           // double2 [256]: C_f, packed
constexpr long long DR_O_CS = DR_O_CF + 16 * DR_BLK;       // double2 [256]: C_s, packed
constexpr long long DR_O_RING = slot_al(DR_O_CS + 16 * DR_BLK);                  // float [R][256]: hop of k hops ago at (rhead - k) mod R
__host__ __device__ constexpr int dr_ring_hops(int Q) { return Q + 4; }
__host__ __device__ constexpr long long dr_rec_bytes(int Q) { return slot_al(DR_O_RING + 4LL * DR_BLK * dr_ring_hops(Q)); }
enum { DR_M_RHEAD = 0, DR_M_BASE1 = 1, DR_M_N = 2, DR_M_SNAPS = 3 };

__host__ __device__ constexpr double dr_tau_max(int Q) { return (double)(DR_BLK * (dr_ring_hops(Q) - 1) - DR_K / 2 - 1); }

struct DriftArgs {
    unsigned char* state;
    int S, Q;
    const float* mic;            // [S][ld]
    const float* played;
    long long ld;
    const int* base_hops;        // [S]
    const unsigned char* active; // [S] or null (all)
    const unsigned char* adapt;  // [S] or null (all)
    int nh;
    double lam_fast, lam_slow, kp, ki;
    float* aligned;              // [S][ld]
    unsigned char* snapped;      // [S] or null
};

struct DriftLds {                                          // 52.5 KB of the 64 KB a plain launch may have
    double table[DR_ROWS * DR_K];
    double2 tw[256];
    double2 xw[FFTW_SLOTS];
    double span[384];                                      // the hop's stretch of the ring (at most 320 samples)
    float ubuf[2 * DR_BLK];                                // [u_prev, u]
    float dbuf[DR_BLK];
    double red[8];                                         // the waves' partial sums
    double loop[3];                                        // tau, rate, delta: thread 0's, for everyone
};

// lo for a NaN: whatever the slot was fed, every index below stays inside the ring, the span and the table
__device__ __forceinline__ double dr_clamp(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// t_j of section 19, step 3, for every thread the same operations (the span's ends are taken from it): the product rounded, then the sum
__device__ __forceinline__ double dr_tj(double tau, double rate, int j, double tau_max) {
#pragma clang fp contract(off)
    const double step = rate * (double)(j + 1);
    return dr_clamp(tau + step, (double)DR_LEAD, tau_max);
}

// I0(x), 0 <= x <= 8: the power series, 40 terms (the 40th is below 1e-30 of the sum)
__device__ __forceinline__ double dr_i0(double x) {
    const double h = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int m = 1; m <= 40; ++m) {
        term *= h / ((double)m * (double)m);
        sum += term;
    }
    return sum;
}

// grid 65, block 64: T[p][k] = sinc(t) I0(beta sqrt(max(0, 1 - (t / 32)^2))) / I0(beta), t = k - 31 - p / 64
__global__ __launch_bounds__(64) void drift_table_kernel(unsigned char* state) {
    const int p = blockIdx.x, k = threadIdx.x;
    const double t = (double)(k - DR_LEAD) - (double)p / (double)NELE_DRIFT_PHASES;
    const double s = (t == 0.0) ? 1.0 : sinpi(t) / (M_PI * t);
    const double r = t / (double)(DR_K / 2);
    const double w = dr_i0(NELE_DRIFT_BETA * sqrt(fmax(0.0, 1.0 - r * r))) / dr_i0(NELE_DRIFT_BETA);
    reinterpret_cast<double*>(state + DR_O_TABLE)[p * DR_K + k] = s * w;
}

__global__ __launch_bounds__(256) void drift_hop_kernel(DriftArgs a) {
    __shared__ DriftLds L;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) {                        // neither read nor written; no snap fell in this call
        if (t == 0 && a.snapped) a.snapped[b] = 0;
        return;
    }
    if (!slot_hdr_matches(a.state, a.S, a.Q)) return;      // not the state nele_drift_init laid out for (S, Q): touch nothing
    const int Q = a.Q, R = dr_ring_hops(Q), N = R * DR_BLK;
    const double tau_max = dr_tau_max(Q);
    unsigned char* rec = a.state + DR_HDR_BYTES + (size_t)b * dr_rec_bytes(Q);
    int* meta = reinterpret_cast<int*>(rec + DR_O_META);
    double* loopp = reinterpret_cast<double*>(rec + DR_O_LOOP);
    float* uprev = reinterpret_cast<float*>(rec + DR_O_UPREV);
    double* Sdp = reinterpret_cast<double*>(rec + DR_O_SD);
    double* Sup = reinterpret_cast<double*>(rec + DR_O_SU);
    double2* Cfp = reinterpret_cast<double2*>(rec + DR_O_CF);
    double2* Csp = reinterpret_cast<double2*>(rec + DR_O_CS);
    float* ring = reinterpret_cast<float*>(rec + DR_O_RING);
    const int w = t >> 6, lane = t & 63;
    const bool slot0 = (t == 0);
    const bool adapts = !a.adapt || a.adapt[b];
    const double one_m_smooth = 1.0 - NELE_DRIFT_SMOOTH;

    // the slot's scalars are workgroup-uniform: every thread keeps them
    int rhead = min(max(meta[DR_M_RHEAD], 0), R - 1);
    int base1 = min(max(meta[DR_M_BASE1], 0), Q);
    int n = meta[DR_M_N], snaps = meta[DR_M_SNAPS];
    double tau = loopp[0], rate = loopp[1], delta = loopp[2];
    const int base = a.base_hops[b];
    const bool snap = base >= 0 && base < Q && base + 1 != base1;
    const bool locked_in = base1 != 0;                     // a slot that comes in unlocked and stays so reads and writes the ring only
    bool est = false;                                      // the estimator's state is in registers and LDS (and goes back at the end)
    double sd = 0.0, su = 0.0, sd_ny = 0.0, su_ny = 0.0;
    double2 cf = make_double2(0.0, 0.0), cs = cf;
    if (snap) {                                            // tau <- the base; the estimator cleared; rate and the ring kept
        tau = fmax((double)(DR_BLK * base), (double)DR_LEAD);
        base1 = base + 1;
        n = 0;
        delta = 0.0;
        snaps = (snaps < 0x7fffffff) ? snaps + 1 : snaps;
        L.ubuf[t] = 0.0f;
        est = true;
    } else if (locked_in) {
        L.ubuf[t] = uprev[t];
        sd = Sdp[t];
        su = Sup[t];
        cf = Cfp[t];
        cs = Csp[t];
        if (slot0) {
            sd_ny = Sdp[DR_BLK];
            su_ny = Sup[DR_BLK];
        }
        est = true;
    }
    if (est) {
        fft512_fill_twiddles(L.tw);
        const double* tab = reinterpret_cast<const double*>(a.state + DR_O_TABLE);
        for (int i = t; i < DR_ROWS * DR_K; i += 256) L.table[i] = tab[i];
    }
    const float* micb = a.mic + (size_t)b * a.ld;
    const float* plb = a.played + (size_t)b * a.ld;
    float* outb = a.aligned + (size_t)b * a.ld;

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * DR_BLK;
        // ---- 1. push x onto the ring
        const float xv = plb[col + t];
        rhead = (rhead + 1 == R) ? 0 : rhead + 1;
        ring[(size_t)rhead * DR_BLK + t] = xv;
        // ---- 2. before the first snap: zeros, nothing else (workgroup-uniform)
        if (!est) {
            outb[col + t] = 0.0f;
            continue;
        }
        const float dv = micb[col + t];
        __syncthreads();                                   // the ring's newest hop (and, first hop, the table, the twiddles and u_prev)
        // ---- 3. the warp: thread j takes u_j.  The span of the ring that the hop reads, as float64 in LDS: D is monotone in j, so its
        // extremes are those of samples 0 and 255, and sample j, tap k sits at span[j - D + Dmax + 63 - k]
        const int D0 = (int)floor((dr_tj(tau, rate, 0, tau_max) - (double)DR_LEAD) * 64.0) >> 6;
        const int D1 = (int)floor((dr_tj(tau, rate, DR_BLK - 1, tau_max) - (double)DR_LEAD) * 64.0) >> 6;
        const int Dmin = min(D0, D1), Dmax = max(D0, D1);
        const int len = DR_BLK + DR_K - 1 + (Dmax - Dmin); // 319 or 320
        for (int i = t; i < len; i += 256) {
            int idx = rhead * DR_BLK + (i - Dmax - (DR_K - 1));                  // i - Dmax - 63 in -256 (R - 1) + 1 .. 255 - Dmin
            if (idx < 0) idx += N;
            L.span[i] = (double)ring[idx];
        }
        __syncthreads();
        float uf;
        {
            const double q = (dr_tj(tau, rate, t, tau_max) - (double)DR_LEAD) * 64.0;
            const double qf = floor(q);
            const double al = q - qf;
            const int qi = (int)qf;
            const int D = min(max(qi >> 6, Dmin), Dmax), p = qi & 63;            // (the clamp changes nothing: D0 and D1 bracket it)
            const double* T0 = L.table + p * DR_K;
            const double* T1 = T0 + DR_K;
            const double* sp = L.span + (t - D + Dmax + (DR_K - 1));
            double acc = 0.0;
#pragma unroll 8
            for (int k = 0; k < DR_K; ++k) {
                const double c0 = T0[k];
                acc += (c0 + al * (T1[k] - c0)) * sp[-k];
            }
            uf = (float)acc;
        }
        outb[col + t] = uf;
        L.ubuf[DR_BLK + t] = uf;
        L.dbuf[t] = dv;
        // ---- 4. tau moves on by the hop's drift (every thread: the same operations)
        tau = dr_clamp(tau + 256.0 * rate, (double)DR_LEAD, tau_max);
        __syncthreads();
        // ---- 5. the estimator, on the rounded output: U = rfft512([u_prev, u]) and Dm = rfft512([0 x 256, d]) from one complex
        // transform (wave 0)
        if (w == 0) {
            double2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int i = fftw_n(lane, r);
                v[r] = make_double2((double)L.ubuf[i], (i >= DR_BLK) ? (double)L.dbuf[i - DR_BLK] : 0.0);
            }
            fftw_wave_sync();
            fft512_wave<false>(v, L.xw, L.tw, lane);
            fft512_wave_store(v, L.xw, lane);
        }
        __syncthreads();
        L.ubuf[t] = uf;                                    // u_prev <- u (wave 0 has read ubuf; its upper half is next written behind two barriers)
        double num, den;
        {
            double2 U, Dm;
            fft512_packed_split(L.xw, t, U, Dm);
            double2 c;
            if (slot0) {                                   // bins 0 and 256: real, component-wise
                sd = NELE_DRIFT_SMOOTH * sd + one_m_smooth * (Dm.x * Dm.x);
                sd_ny = NELE_DRIFT_SMOOTH * sd_ny + one_m_smooth * (Dm.y * Dm.y);
                su = NELE_DRIFT_SMOOTH * su + one_m_smooth * (U.x * U.x);
                su_ny = NELE_DRIFT_SMOOTH * su_ny + one_m_smooth * (U.y * U.y);
                c = make_double2(Dm.x * U.x / sqrt(sd * su + NELE_DRIFT_EPS), Dm.y * U.y / sqrt(sd_ny * su_ny + NELE_DRIFT_EPS));
            } else {
                sd = NELE_DRIFT_SMOOTH * sd + one_m_smooth * (Dm.x * Dm.x + Dm.y * Dm.y);
                su = NELE_DRIFT_SMOOTH * su + one_m_smooth * (U.x * U.x + U.y * U.y);
                const double s = sqrt(sd * su + NELE_DRIFT_EPS);
                c = make_double2((Dm.x * U.x + Dm.y * U.y) / s, (Dm.y * U.x - Dm.x * U.y) / s);
            }
            cf = make_double2(a.lam_fast * cf.x + (1.0 - a.lam_fast) * c.x, a.lam_fast * cf.y + (1.0 - a.lam_fast) * c.y);
            cs = make_double2(a.lam_slow * cs.x + (1.0 - a.lam_slow) * c.x, a.lam_slow * cs.y + (1.0 - a.lam_slow) * c.y);
            if (slot0) {                                   // bin 0 weighs nothing; bin 256: z real, so only k^2 |z|
                num = 0.0;
                den = 65536.0 * fabs(cf.y * cs.y);
            } else {
                const double zx = cf.x * cs.x + cf.y * cs.y, zy = cf.y * cs.x - cf.x * cs.y;
                const double kk = (double)t;
                num = kk * zy;
                den = kk * kk * sqrt(zx * zx + zy * zy);
            }
        }
        n = (n < 0x7fffffff) ? n + 1 : n;
        num = wave_sum(num);
        den = wave_sum(den);
        if (lane == 0) {
            L.red[w] = num;
            L.red[4 + w] = den;
        }
        __syncthreads();
        // ---- 6. the loop (thread 0), and its tau, rate and delta to everyone
        if (slot0) {
            const double nsum = (L.red[0] + L.red[1]) + (L.red[2] + L.red[3]);
            const double dsum = (L.red[4] + L.red[5]) + (L.red[6] + L.red[7]);
            double dl = -(512.0 / (2.0 * M_PI)) * nsum / (dsum + NELE_DRIFT_TINY);
            double tn = tau, rn = rate;
            if (n > NELE_DRIFT_WARM && adapts) {
                rn = dr_clamp(rate + a.ki * dl / 256.0, -NELE_DRIFT_MAX_RATE, NELE_DRIFT_MAX_RATE);
                tn = dr_clamp(tau + a.kp * dl, (double)DR_LEAD, tau_max);
            }
            L.loop[0] = tn;
            L.loop[1] = rn;
            L.loop[2] = dl;
        }
        __syncthreads();
        tau = L.loop[0];
        rate = L.loop[1];
        delta = L.loop[2];
    }
    if (est) {
        uprev[t] = L.ubuf[t];
        Sdp[t] = sd;
        Sup[t] = su;
        Cfp[t] = cf;
        Csp[t] = cs;
    }
    if (slot0) {
        meta[DR_M_RHEAD] = rhead;
        if (est) {
            Sdp[DR_BLK] = sd_ny;
            Sup[DR_BLK] = su_ny;
            meta[DR_M_BASE1] = base1;
            meta[DR_M_N] = n;
            meta[DR_M_SNAPS] = snaps;
            loopp[0] = tau;
            loopp[1] = rate;
            loopp[2] = delta;
        }
        if (a.snapped) a.snapped[b] = snap ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void drift_set_rate_kernel(unsigned char* state, int S, int Q, const unsigned char* __restrict__ slots,
                                                              const double* __restrict__ rate) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    if (slots && !slots[b]) return;
    const double r = rate[b];
    if (!(fabs(r) <= NELE_DRIFT_MAX_RATE)) return;         // out of range or not a number: the slot stays as it is
    reinterpret_cast<double*>(state + DR_HDR_BYTES + (size_t)b * dr_rec_bytes(Q) + DR_O_LOOP)[1] = r;
}

__global__ __launch_bounds__(256) void drift_status_kernel(const unsigned char* __restrict__ state, int S, int Q, double* __restrict__ info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    const unsigned char* rec = state + DR_HDR_BYTES + (size_t)b * dr_rec_bytes(Q);
    const int* meta = reinterpret_cast<const int*>(rec + DR_O_META);
    const double* loopp = reinterpret_cast<const double*>(rec + DR_O_LOOP);
    double* o = info + (size_t)b * NELE_DRIFT_INFO;
    o[NELE_DRIFT_I_TAU] = loopp[0];
    o[NELE_DRIFT_I_RATE] = loopp[1];
    o[NELE_DRIFT_I_DELTA] = loopp[2];
    o[NELE_DRIFT_I_N] = (double)meta[DR_M_N];
    o[NELE_DRIFT_I_BASE] = (double)(min(max(meta[DR_M_BASE1], 0), Q) - 1);
    o[NELE_DRIFT_I_SNAPS] = (double)meta[DR_M_SNAPS];
}

__global__ __launch_bounds__(256) void drift_taps_kernel(const unsigned char* __restrict__ state, int S, int Q, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= DR_ROWS * DR_K || !slot_hdr_matches(state, S, Q)) return;
    out[i] = reinterpret_cast<const double*>(state + DR_O_TABLE)[i];
}

// ---- the host side
long long drift_state_bytes(int S, int Q) {
    if (S <= 0 || S > SLOT_MAX_STREAMS || Q < 2 || Q > NELE_BULK_MAX_BLOCKS) return -1;
    return DR_HDR_BYTES + (long long)S * dr_rec_bytes(Q);
}

int drift_check(const char* name, const void* state, long long state_bytes, int S, int Q) {
    auto params = [&]() -> int {
        NELE_CHECK_ARG(Q >= 2 && Q <= NELE_BULK_MAX_BLOCKS, "%s: blocks=%d must be in 2 .. %d", name, Q, NELE_BULK_MAX_BLOCKS);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, drift_state_bytes(S, Q), "nele_drift_state_bytes", Q);
}

int drift_reset(const char* name, void* state, long long state_bytes, int S, int Q, const unsigned char* slots, bool init, void* stream) {
    int st = drift_check(name, state, state_bytes, S, Q);
    if (st) return st;
    const int hdr[2] = {S, Q};
    st = slot_state_reset(name, state, DR_HDR_BYTES, dr_rec_bytes(Q), S, slots, init ? 2 : 0, hdr, stream);
    if (st || !init) return st;
    hipLaunchKernelGGL(drift_table_kernel, dim3(DR_ROWS), dim3(DR_K), 0, as_stream(stream), (unsigned char*)state);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_drift_state_bytes(int max_streams, int blocks) { return drift_state_bytes(max_streams, blocks); }
extern "C" long long nele_drift_stream_record_bytes(int blocks) {
    return (blocks < 2 || blocks > NELE_BULK_MAX_BLOCKS) ? -1 : dr_rec_bytes(blocks);
}

extern "C" int nele_drift_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream) {
    return drift_reset("nele_drift_init", state, state_bytes, max_streams, blocks, nullptr, true, stream);
}

extern "C" int nele_drift_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream) {
    return drift_reset("nele_drift_reset", state, state_bytes, max_streams, blocks, slots, false, stream);
}

extern "C" int nele_drift_set_rate(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                                   const double* rate_dev, void* stream) {
    const char* name = "nele_drift_set_rate";
    int st = drift_check(name, state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(rate_dev, "%s: null rate_dev", name);
    hipLaunchKernelGGL(drift_set_rate_kernel, dim3((max_streams + 255) / 256), dim3(256), 0, as_stream(stream), (unsigned char*)state, max_streams,
                       blocks, slots, rate_dev);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

extern "C" int nele_drift_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                              const int* base_hops, const unsigned char* active, const unsigned char* adapt, int nh, double lam_fast,
                              double lam_slow, double kp, double ki, float* aligned, unsigned char* snapped, void* stream) {
    const char* name = "nele_drift_hop";
    int st = drift_check(name, state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(mic, "%s: null mic", name);
    NELE_CHECK_ARG(played, "%s: null played", name);
    NELE_CHECK_ARG(base_hops, "%s: null base_hops", name);
    NELE_CHECK_ARG(aligned, "%s: null aligned", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(lam_fast > 0.0 && lam_fast < 1.0, "%s: lam_fast=%g must be in (0, 1)", name, lam_fast);
    NELE_CHECK_ARG(lam_slow > lam_fast && lam_slow < 1.0, "%s: lam_slow=%g must be in (lam_fast, 1)", name, lam_slow);
    NELE_CHECK_ARG(kp >= 0.0 && kp <= 1e300, "%s: kp=%g must be finite and >= 0", name, kp);
    NELE_CHECK_ARG(ki >= 0.0 && ki <= 1e300, "%s: ki=%g must be finite and >= 0", name, ki);
    DriftArgs a = {(unsigned char*)state, max_streams, blocks, mic,      played, (long long)nh * DR_BLK, base_hops, active, adapt,
                   nh,                    lam_fast,    lam_slow, kp,     ki,     aligned,                snapped};
    hipLaunchKernelGGL(drift_hop_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

extern "C" int nele_drift_status(const void* state, long long state_bytes, int max_streams, int blocks, double* info, void* stream) {
    const char* name = "nele_drift_status";
    int st = drift_check(name, state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(info, "%s: null info", name);
    hipLaunchKernelGGL(drift_status_kernel, dim3((max_streams + 255) / 256), dim3(256), 0, as_stream(stream), (const unsigned char*)state,
                       max_streams, blocks, info);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

extern "C" int nele_drift_taps(const void* state, long long state_bytes, int max_streams, int blocks, double* taps_out_dev, void* stream) {
    const char* name = "nele_drift_taps";
    int st = drift_check(name, state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(taps_out_dev, "%s: null taps_out_dev", name);
    hipLaunchKernelGGL(drift_taps_kernel, dim3((DR_ROWS * DR_K + 255) / 256), dim3(256), 0, as_stream(stream), (const unsigned char*)state,
                       max_streams, blocks, taps_out_dev);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
