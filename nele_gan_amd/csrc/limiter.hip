// Look-ahead true-peak limiter, the last stage of the real-time path, many concurrent streams (nele_lim_*): 256-sample hops, one hop of
// delay, up to 192 samples of look-ahead, a 4 x oversampled peak detector, a decaying maximum of the wanted reduction and a moving
// average over the look-ahead that ramps the gain into every peak.  The arithmetic is DESIGN.md section 26; tests/limiter_ref.py
// restates it in numpy and the two agree in every bit of out, gain and peak.
//   lim_hop_kernel : one wave per stream, one stream per workgroup, looping over the call's hops
// drc_hop_kernel's shape (csrc/drc.hip): the stream's state stays on chip across the call's hops - the last 262 samples in a ring of
// 1024 floats in LDS, the last LA values of q at the head of the hop's q array, d in a register.  Per emitted hop the 64 lanes compute
// the interpolated maxima (three 12-tap sums per sample), p and r, then the sliding minimum m by doubling, all through LDS; lane 0 runs the decaying
// maximum in sample order - one multiply and one max on the dependent path, 256 steps, 256 + LA on a slot's first emitted hop - and
// the 64 lanes take the (LA + 1)-term means in index order, hold them under r, apply the gain and clamp.  max and min here are fmax and fmin: a NaN
// operand is passed over, which is what section 26 (d) and numpy's fmax / fmin say.
// State is read and written with plain loads and stores by the stream's own wave; no atomics, no workgroup barrier, nothing crosses
// waves: a slot's bits do not depend on the hop grouping, on max_streams or on the other slots.
// In the Makefile's EXACT list (no FMA contraction): the sums keep the operation order of section 26.
#include "common.h"
#include "slot_state.h"
#include <cmath>
#include "../../include/nele_hip_ext9.h"

namespace {

#define LIM_BLK NELE_LIM_HOP                               // samples per hop
#define LIM_MAXLA NELE_LIM_MAX_LOOKAHEAD
#define LIM_REACH 6                                        // p[i] reads s[i - 6 .. i + 6]
#define LIM_HIST (LIM_BLK + LIM_REACH)                     // input samples a record keeps: 262
#define LIM_RING 1024                                      // floats: >= LIM_HIST + 256, a power of two
#define LIM_NR (LIM_BLK + 2 * LIM_MAXLA)                   // r values of a hop at most: n - LA (first emitted hop) .. n + 255 + LA
constexpr long long LIM_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = the record's bytes, [2] = LA, [3] = LIM_HIST
// per-stream record, byte offsets
constexpr long long LIM_O_CTL = 0;                         // int [1]: hops so far, stops at 2
constexpr long long LIM_O_D = 64;                          // double: d
constexpr long long LIM_O_HIST = 128;                      // float [262]: the samples before the next hop (float32 in, kept exactly)
constexpr long long LIM_O_Q = 1184;                        // double [LA]: the last LA values of q
constexpr long long lim_rec_bytes(int la) { return slot_al(LIM_O_Q + 8LL * la); }
static_assert(LIM_O_HIST + 4 * LIM_HIST <= LIM_O_Q && LIM_O_Q % 8 == 0 && lim_rec_bytes(80) == 2048 && lim_rec_bytes(LIM_MAXLA) == 2816,
              "the record of section 26");
static_assert(LIM_MAXLA + LIM_REACH < LIM_BLK && LIM_HIST + 2 * LIM_BLK <= LIM_RING, "the emitted hop reads into the newest hop only");

struct LimArgs {
    unsigned char* state;
    int S;
    const float* x;              // [S][ld]
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh, la, use_taps;
    double c, drive, rel;
    float cf;                    // the largest float32 <= c
    double f[NELE_LIM_TAPS];     // f_k[m] at [12 (k - 1) + m + 5]
    float* out;                  // [S][ld]
    double* gain;                // [S][ld] or null
    double* peak;                // [S][nh] or null
};

// orders the LDS accesses of ONE wave (fft512.h's fftw_wave_sync)
__device__ __forceinline__ void lim_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64) void lim_hop_kernel(LimArgs a) {
    __shared__ float ring[LIM_RING];                       // sample t of the call (t = -262 at the history's start) at [(t + 262) & 1023]
    __shared__ double um[LIM_NR + 1];                      // max_k |u_k[i]| at [i - (t0 - LA - 1)]; then, with rr, the minima of step 3
    __shared__ double rr[LIM_NR];                          // r[i] at [i - (t0 - LA)]
    __shared__ double qq[LIM_BLK + LIM_MAXLA];             // q[n] at [n - (t0 - LA)]
    const int lane = threadIdx.x, b = blockIdx.x, LA = a.la;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    const int rec_bytes = (int)lim_rec_bytes(LA);
    if (!slot_hdr_matches(a.state, a.S, rec_bytes, LA, LIM_HIST)) return;      // not the state nele_lim_init laid out for (S, LA): touch nothing
    unsigned char* rec = a.state + LIM_HDR_BYTES + (size_t)b * rec_bytes;
    int* ctl = reinterpret_cast<int*>(rec + LIM_O_CTL);
    double* dp = reinterpret_cast<double*>(rec + LIM_O_D);
    float* histp = reinterpret_cast<float*>(rec + LIM_O_HIST);
    double* qp = reinterpret_cast<double*>(rec + LIM_O_Q);

    int cnt = ctl[0];
    double d = dp[0];
    for (int i = lane; i < LIM_HIST; i += 64) ring[i] = histp[i];
    for (int i = lane; i < LA; i += 64) qq[i] = qp[i];
    const float* xb = a.x + (size_t)b * a.ld;
    float* outb = a.out + (size_t)b * a.ld;
    double* gainb = a.gain ? a.gain + (size_t)b * a.ld : nullptr;
    const double terms = (double)(LA + 1);

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * LIM_BLK;
        const int t0 = (h - 1) * LIM_BLK;                  // the emitted hop's first sample, in the call's time
        float xn[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) xn[m] = xb[col + 64 * m + lane];
        lim_wave_sync();                                   // the previous hop's reads of the ring precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) ring[(t0 + LIM_BLK + LIM_HIST + 64 * m + lane) & (LIM_RING - 1)] = xn[m];
        lim_wave_sync();
        if (cnt == 0) {                                    // the slot's first hop: nothing to emit yet
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                outb[col + 64 * m + lane] = 0.f;
                if (gainb) gainb[col + 64 * m + lane] = 0.0;
            }
            if (a.peak && lane == 0) a.peak[(size_t)b * a.nh + h] = 0.0;
            cnt = 1;
            continue;
        }
        const bool first = cnt == 1;                       // the emitted hop is the stream's hop 0: zeros before t0, LA more steps
        const int lo = first ? 0 : LA;                     // first index of r, m and q this hop computes; the last r is at 255 + 2 LA
        const int nr = LIM_BLK + 2 * LA;
        // s[t], zero before the stream's start
        auto sv = [&](int t) -> double { return (first && t < t0) ? 0.0 : a.drive * (double)ring[(t + LIM_HIST) & (LIM_RING - 1)]; };
        // ---- 1a. um = max_k |u_k[i]| for i = t0 - LA - 1 + j, j = lo .. nr
        if (a.use_taps) {
            for (int j = lo + lane; j <= nr; j += 64) {
                const int i = t0 - LA - 1 + j;
                double sw[12];
#pragma unroll
                for (int m = 0; m < 12; ++m) sw[m] = sv(i - 5 + m);
                double best = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double u = 0.0;
#pragma unroll
                    for (int m = 0; m < 12; ++m) u += a.f[12 * k + m] * sw[m];
                    best = fmax(best, fabs(u));
                }
                um[j] = best;
            }
            lim_wave_sync();
        }
        // ---- 1b, 2. p[i] and r[i] for i = t0 - LA + j, j = lo .. nr - 1; the emitted hop's largest p
        double pk = 0.0;
        for (int j = lo + lane; j < nr; j += 64) {
            double p = fabs(sv(t0 - LA + j));
            if (a.use_taps) p = fmax(fmax(p, um[j + 1]), um[j]);
            rr[j] = p > a.c ? a.c / p : 1.0;
            if (j >= LA && j < LA + LIM_BLK) pk = fmax(pk, p);
        }
        pk = wave_max(pk);
        if (a.peak && lane == 0) a.peak[(size_t)b * a.nh + h] = pk;
        lim_wave_sync();
        double rn[4];                                      // r of the emitted hop's samples: step 5 holds the gain under it
#pragma unroll
        for (int m = 0; m < 4; ++m) rn[m] = rr[LA + 64 * m + lane];
        // ---- 3. m[n] = min r[n .. n + LA], n = t0 - LA + j, j = lo .. LA + 255.  min is exact in any order: minima over 2, 4 .. P
        // consecutive values by doubling (P the largest power of two <= LA + 1), from one buffer into the other, then two
        // overlapping windows of P.  An index clamped to the last r only enters minima that no used window reads.
        double* src = rr;
        double* dst = um;
        int span = 1;
        for (; 2 * span <= LA + 1; span *= 2) {
            for (int j = lo + lane; j < nr; j += 64) dst[j] = fmin(src[j], src[min(j + span, nr - 1)]);
            lim_wave_sync();
            double* t = src;
            src = dst;
            dst = t;
        }
        for (int j = lo + lane; j < LA + LIM_BLK; j += 64) dst[j] = fmin(src[j], src[j + LA + 1 - span]);
        const double* mm = dst;
        lim_wave_sync();
        // ---- 4. the decaying maximum, in sample order, on lane 0
        if (lane == 0) {
            double dv = first ? 0.0 : d;
#pragma unroll 8
            for (int j = lo; j < LA + LIM_BLK; ++j) {
                dv = fmax(1.0 - mm[j], a.rel * dv);
                qq[j] = 1.0 - dv;
            }
            d = dv;
        }
        lim_wave_sync();
        // ---- 5, 6. the mean of q over the look-ahead in index order, the gain, the clamp
        double qn[3];                                      // q[t0 + 256 + i], i < LA, for the next hop
#pragma unroll
        for (int m = 0; m < 3; ++m) qn[m] = (64 * m + lane < LA) ? qq[LIM_BLK + 64 * m + lane] : 0.0;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};              // four sums side by side, each in index order
        for (int k = 0; k <= LA; ++k) {
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] += qq[64 * m + lane + k];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = 64 * m + lane;
            const double g = fmin(acc[m] / terms, rn[m]);
            const double y = g * sv(t0 + n);
            const float o = (float)y;
            outb[col + n] = o > a.cf ? a.cf : (o < -a.cf ? -a.cf : o);
            if (gainb) gainb[col + n] = g;
        }
        lim_wave_sync();                                   // the means are read: q moves on by a hop
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (64 * m + lane < LA) qq[64 * m + lane] = qn[m];
        cnt = 2;
    }
    // ---- the history moves on by the call's hops
    lim_wave_sync();
    const int base = a.nh * LIM_BLK;
    for (int i = lane; i < LIM_HIST; i += 64) histp[i] = ring[(base + i) & (LIM_RING - 1)];
    for (int i = lane; i < LA; i += 64) qp[i] = qq[i];
    if (lane == 0) {                                       // (lane 0 ran the recursion: d is its)
        ctl[0] = cnt;
        dp[0] = d;
    }
}

bool lim_la_ok(int la) { return la >= 1 && la <= LIM_MAXLA; }

int lim_check(const char* name, const void* state, long long state_bytes, int S, int la) {
    return slot_state_check(
        name, state, state_bytes, S,
        [&]() -> int {
            NELE_CHECK_ARG(lim_la_ok(la), "%s: lookahead=%d must be in 1 .. %d", name, la, LIM_MAXLA);
            return NELE_OK;
        },
        lim_la_ok(la) ? nele_lim_state_bytes(S, la) : 0, "nele_lim_state_bytes", la);
}

// slots == null: every record; write_hdr: the header too
int lim_reset(const char* name, void* state, int S, int la, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[4] = {S, (int)lim_rec_bytes(la), la, LIM_HIST};
    return slot_state_reset(name, state, LIM_HDR_BYTES, lim_rec_bytes(la), S, slots, write_hdr ? 4 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_lim_stream_record_bytes(int lookahead) { return lim_la_ok(lookahead) ? lim_rec_bytes(lookahead) : -1; }

extern "C" long long nele_lim_state_bytes(int max_streams, int lookahead) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || !lim_la_ok(lookahead)) return -1;
    return LIM_HDR_BYTES + (long long)max_streams * lim_rec_bytes(lookahead);
}

extern "C" int nele_lim_init(void* state, long long state_bytes, int max_streams, int lookahead, void* stream) {
    int st = lim_check("nele_lim_init", state, state_bytes, max_streams, lookahead);
    if (st) return st;
    return lim_reset("nele_lim_init", state, max_streams, lookahead, nullptr, true, stream);
}

extern "C" int nele_lim_reset(void* state, long long state_bytes, int max_streams, int lookahead, const unsigned char* slots, void* stream) {
    int st = lim_check("nele_lim_reset", state, state_bytes, max_streams, lookahead);
    if (st) return st;
    return lim_reset("nele_lim_reset", state, max_streams, lookahead, slots, false, stream);
}

extern "C" int nele_lim_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh,
                            double ceiling, double drive, int lookahead, double rel, const double* taps_host, float* out, double* gain,
                            double* peak, void* stream) {
    const char* name = "nele_lim_hop";
    int st = lim_check(name, state, state_bytes, max_streams, lookahead);
    if (st) return st;
    NELE_CHECK_ARG(x && out, "%s: null x / out", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(ceiling > 0.0 && std::isfinite(ceiling), "%s: ceiling=%g must be positive and finite", name, ceiling);
    NELE_CHECK_ARG(drive > 0.0 && std::isfinite(drive), "%s: drive=%g must be positive and finite", name, drive);
    NELE_CHECK_ARG(rel >= 0.0 && rel < 1.0, "%s: rel=%g must be in [0, 1)", name, rel);
    if (taps_host)
        for (int i = 0; i < NELE_LIM_TAPS; ++i) NELE_CHECK_ARG(std::isfinite(taps_host[i]), "%s: tap %d is not finite", name, i);
    float cf = (float)ceiling;                              // the largest float32 <= ceiling
    if ((double)cf > ceiling) cf = std::nextafterf(cf, 0.f);
    NELE_CHECK_ARG(cf > 0.f && std::isfinite(cf), "%s: ceiling=%g has no positive finite float32 at or below it", name, ceiling);
    LimArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.x = x;
    a.ld = (long long)nh * LIM_BLK;
    a.active = active;
    a.nh = nh;
    a.la = lookahead;
    a.use_taps = taps_host != nullptr;
    a.c = ceiling;
    a.drive = drive;
    a.rel = rel;
    a.cf = cf;
    for (int i = 0; i < NELE_LIM_TAPS; ++i) a.f[i] = taps_host ? taps_host[i] : 0.0;
    a.out = out;
    a.gain = gain;
    a.peak = peak;
    hipLaunchKernelGGL(lim_hop_kernel, dim3(max_streams), dim3(64), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
