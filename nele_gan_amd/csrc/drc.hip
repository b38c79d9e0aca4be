// Dynamic range compression behind the enhancer of the real-time path, many concurrent streams (nele_drc_*): stage 2 of SSDRC (csrc/ssdrc.hip,
// DESIGN.md section 11) in a causal form - 256-sample hops, one hop of delay, 144 samples of look-ahead, a decaying maximum for the
// reference level and a recursive energy equaliser.  The arithmetic is DESIGN.md section 23; tests/drc_ref.py restates it in numpy.
//   drc_hop_kernel : one wave per stream, one stream per workgroup, looping over the call's hops
// ns_hop_kernel's shape (csrc/ns.hip) without its sharing of a workgroup: the stream's state stays on chip across the call's hops -
// the last 656 samples in a ring of 1024 floats in LDS, the six scalars in registers.  Per emitted hop the 64 lanes compute the 416 magnitudes (32 antisymmetric tap pairs each)
// and the 256 centred means (161 terms each, in index order) through LDS; lane 0 then runs the 256 attack / release steps - a data-dependent
// recursion with no prefix form, the latency floor of the hop: both branches are computed and the comparison selects one, which leaves
// multiply, add, select on the dependent path - and the 64 lanes apply the curve, the gain and the equaliser's ramp.  The hop maximum
// and the two hop sums are lane partials in index order followed by the xor butterfly (wave_max / wave_sum): every lane holds the same bits.
// State is read and written with plain loads and stores by the stream's own wave; no atomics, no workgroup barrier, nothing crosses
// waves: a slot's bits do not depend on the hop grouping, on max_streams or on the other slots.
// In the Makefile's EXACT list (no FMA contraction): the sums keep the operation order of section 23.
#include "common.h"
#include "slot_state.h"
#include <cmath>
#include "../../include/nele_hip_ext6.h"

namespace {

#define DRC_BLK NELE_DRC_HOP                               // samples per hop
#define DRC_WAVES 1                                        // streams per workgroup: measured, 4 cost 0.047 ms a hop at B = 16 .. 256 where 1 costs 0.035
#define DRC_HIL 64                                         // Hilbert FIR half-length: odd taps 1, 3 .. 63
#define DRC_AVG 80                                         // half-width of the centred mean
#define DRC_NA (DRC_BLK + 2 * DRC_AVG)                     // magnitudes per hop: 416
#define DRC_RING 1024                                      // floats: >= NELE_DRC_HIST + DRC_BLK, a power of two
constexpr long long DRC_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = the record's bytes (what nele_drc_init laid out)
// per-stream record, byte offsets
constexpr long long DRC_O_CTL = 0;                         // int [1]: hops so far, stops at 2
constexpr long long DRC_O_DBL = 64;                        // double [5]: DRC_F_*
enum { DRC_F_EH, DRC_F_M, DRC_F_EIN, DRC_F_EOUT, DRC_F_GPREV, DRC_NDBL };
constexpr long long DRC_O_HIST = 128;                      // float [400]: the samples before the next hop (float32 in, kept exactly)
constexpr long long DRC_REC_BYTES = slot_al(DRC_O_HIST + 4 * NELE_DRC_HIST);
static_assert(NELE_DRC_HIST == DRC_BLK + DRC_AVG + DRC_HIL && NELE_DRC_LOOKAHEAD == DRC_AVG + DRC_HIL, "the window of DESIGN.md section 23");
static_assert(DRC_O_DBL + 8 * DRC_NDBL <= DRC_O_HIST && DRC_REC_BYTES == 1792 && NELE_DRC_HIST + DRC_BLK <= DRC_RING, "the record of section 23");

struct DrcArgs {
    unsigned char* state;
    int S;
    const float* x;              // [S][ld]
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh, equalise, n_knots;
    double attack, release, e0_ratio, rho, lam;
    double kx[NELE_SSDRC_MAX_KNOTS], ky[NELE_SSDRC_MAX_KNOTS];
    double hil[DRC_HIL / 2];     // h[2 k + 1]
    const double* ref_level;     // [S] or null
    float* out;                  // [S][ld]
    double* gain;                // [S][ld] or null
    double* level;               // [S][nh] or null
};

// orders the LDS accesses of ONE wave (fft512.h's fftw_wave_sync)
__device__ __forceinline__ void drc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// section 11's static curve: unity slope below the first knot, a limiter above the last one
__device__ __forceinline__ double drc_curve(const DrcArgs& a, double xin) {
    if (xin < a.kx[0]) return xin + (a.ky[0] - a.kx[0]);
    double out = a.ky[a.n_knots - 1];
    for (int j = 0; j + 1 < a.n_knots; ++j)
        if (xin >= a.kx[j] && xin < a.kx[j + 1]) out = (a.ky[j + 1] - a.ky[j]) / (a.kx[j + 1] - a.kx[j]) * (xin - a.kx[j]) + a.ky[j];
    return out;
}

__global__ __launch_bounds__(64 * DRC_WAVES) void drc_hop_kernel(DrcArgs a) {
    __shared__ float ring_s[DRC_WAVES][DRC_RING];          // sample t of the call (t = -400 at the history's start) at [(t + 400) & 1023]
    __shared__ double aa_s[DRC_WAVES][DRC_NA];             // a at 256 j - 80 + q
    __shared__ double ee_s[DRC_WAVES][DRC_BLK];            // e of the hop, then e-hat
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * DRC_WAVES + w;
    if (b >= a.S) return;                                  // (no workgroup barrier below: a wave is on its own)
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, (int)DRC_REC_BYTES)) return;   // not the state nele_drc_init laid out for S: touch nothing
    unsigned char* rec = a.state + DRC_HDR_BYTES + (size_t)b * DRC_REC_BYTES;
    int* ctl = reinterpret_cast<int*>(rec + DRC_O_CTL);
    double* dbl = reinterpret_cast<double*>(rec + DRC_O_DBL);
    float* histp = reinterpret_cast<float*>(rec + DRC_O_HIST);
    float* ring = ring_s[w];
    double* aa = aa_s[w];
    double* ee = ee_s[w];

    int cnt = ctl[0];
    double eh = dbl[DRC_F_EH], M = dbl[DRC_F_M], Ein = dbl[DRC_F_EIN], Eout = dbl[DRC_F_EOUT], gprev = dbl[DRC_F_GPREV];
    for (int i = lane; i < NELE_DRC_HIST; i += 64) ring[i] = histp[i];
    const double fixed = a.ref_level ? a.ref_level[b] : 0.0;
    const double om_att = 1.0 - a.attack, om_rel = 1.0 - a.release;
    const float* xb = a.x + (size_t)b * a.ld;
    float* outb = a.out + (size_t)b * a.ld;
    double* gainb = a.gain ? a.gain + (size_t)b * a.ld : nullptr;

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * DRC_BLK;
        const int pos = (h * DRC_BLK) & (DRC_RING - 1);    // ring index of the sample 400 before this hop
        float xn[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) xn[m] = xb[col + 64 * m + lane];
        drc_wave_sync();                                   // the previous hop's reads of the ring precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) ring[(pos + NELE_DRC_HIST + 64 * m + lane) & (DRC_RING - 1)] = xn[m];
        drc_wave_sync();
        if (cnt == 0) {                                    // the slot's first hop: nothing to emit yet
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                outb[col + 64 * m + lane] = 0.f;
                if (gainb) gainb[col + 64 * m + lane] = 0.0;
            }
            if (a.level && lane == 0) a.level[(size_t)b * a.nh + h] = 0.0;
            cnt = 1;
            continue;
        }
        // ---- 1. a[i] = sqrt(s^2 + sh^2) for i = 256 j - 80 + q; s[256 j - 144 + r] is ring[pos + r]
        for (int q = lane; q < DRC_NA; q += 64) {
            const int c = pos + DRC_HIL + q;
            double sh = 0.0;
#pragma unroll 8
            for (int k = 0; k < DRC_HIL / 2; ++k)
                sh += a.hil[k] * ((double)ring[(c - (2 * k + 1)) & (DRC_RING - 1)] - (double)ring[(c + (2 * k + 1)) & (DRC_RING - 1)]);
            const double s = (double)ring[c & (DRC_RING - 1)];
            aa[q] = (cnt == 1 && q < DRC_AVG) ? 0.0 : sqrt(s * s + sh * sh);     // before the stream's start the magnitude is zero
        }
        drc_wave_sync();
        // ---- 2. e[n] = (sum_{i = n - 80}^{n + 80} a[i]) / 161 in index order; the hop maximum
        double mx = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = 64 * m + lane;
            double acc = 0.0;
#pragma unroll 7
            for (int k = 0; k <= 2 * DRC_AVG; ++k) acc += aa[n + k];
            const double e = acc / (double)(2 * DRC_AVG + 1);
            ee[n] = e;
            mx = fmax(mx, e);
        }
        mx = wave_max(mx);
        drc_wave_sync();
        // ---- 3. the attack / release chain, in sample order, on lane 0
        if (lane == 0) {
            double p = eh;
#pragma unroll 8
            for (int n = 0; n < DRC_BLK; ++n) {
                const double ev = ee[n];
                const double up = a.attack * p + om_att * ev, down = a.release * p + om_rel * ev;
                p = ev >= p ? up : down;
                ee[n] = p;
            }
            eh = p;
        }
        drc_wave_sync();
        // ---- 4. the reference level
        M = fmax(mx, a.rho * M);
        const double e0 = a.ref_level ? fixed : a.e0_ratio * M;
        if (a.level && lane == 0) a.level[(size_t)b * a.nh + h] = e0;
        // ---- 5. the curve and the gain
        double s[4], g1[4], y[4], pin = 0.0, pout = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = 64 * m + lane;
            s[m] = (double)ring[(pos + NELE_DRC_LOOKAHEAD + n) & (DRC_RING - 1)];
            g1[m] = 1.0;
            if (e0 > 0.0) {
                const double xin = 20.0 * log10(fmax(ee[n], 1e-10 * e0) / e0);
                g1[m] = pow(10.0, (drc_curve(a, xin) - xin) / 20.0);
            }
            y[m] = g1[m] * s[m];
            pin += s[m] * s[m];
            pout += y[m] * y[m];
        }
        // ---- 6. the equaliser: its gain moves linearly from the last hop's to this hop's
        double g = 1.0;
        if (a.equalise) {
            Ein = a.lam * Ein + wave_sum(pin);
            Eout = a.lam * Eout + wave_sum(pout);
            g = Eout > 0.0 ? sqrt(Ein / Eout) : 1.0;
        }
        const double gp = cnt == 1 ? 1.0 : gprev;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int n = 64 * m + lane;
            const double r = gp + (g - gp) * (double)(n + 1) / (double)DRC_BLK;
            outb[col + n] = (float)(y[m] * r);
            if (gainb) gainb[col + n] = g1[m] * r;
        }
        gprev = g;
        cnt = 2;
    }
    // ---- 7. the history moves on by the call's hops
    drc_wave_sync();
    const int pos = (a.nh * DRC_BLK) & (DRC_RING - 1);
    for (int i = lane; i < NELE_DRC_HIST; i += 64) histp[i] = ring[(pos + i) & (DRC_RING - 1)];
    if (lane == 0) {                                       // (lane 0 ran the chain: e-hat is its)
        ctl[0] = cnt;
        dbl[DRC_F_EH] = eh;
        dbl[DRC_F_M] = M;
        dbl[DRC_F_EIN] = Ein;
        dbl[DRC_F_EOUT] = Eout;
        dbl[DRC_F_GPREV] = gprev;
    }
}

int drc_check(const char* name, const void* state, long long state_bytes, int S) {
    return slot_state_check(name, state, state_bytes, S, []() -> int { return NELE_OK; }, nele_drc_state_bytes(S), "nele_drc_state_bytes");
}

// slots == null: every record; write_hdr: the header too
int drc_reset(const char* name, void* state, int S, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, (int)DRC_REC_BYTES};
    return slot_state_reset(name, state, DRC_HDR_BYTES, DRC_REC_BYTES, S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_drc_state_bytes(int max_streams) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS) return -1;
    return DRC_HDR_BYTES + (long long)max_streams * DRC_REC_BYTES;
}

extern "C" long long nele_drc_stream_record_bytes(void) { return DRC_REC_BYTES; }

extern "C" int nele_drc_init(void* state, long long state_bytes, int max_streams, void* stream) {
    int st = drc_check("nele_drc_init", state, state_bytes, max_streams);
    if (st) return st;
    return drc_reset("nele_drc_init", state, max_streams, nullptr, true, stream);
}

extern "C" int nele_drc_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream) {
    int st = drc_check("nele_drc_reset", state, state_bytes, max_streams);
    if (st) return st;
    return drc_reset("nele_drc_reset", state, max_streams, slots, false, stream);
}

extern "C" int nele_drc_hop(void* state, long long state_bytes, int max_streams, const float* x, const unsigned char* active, int nh,
                            const nele_ssdrc_params* params, double rho, double lam, int equalise, const double* ref_level, float* out,
                            double* gain, double* level, void* stream) {
    const char* name = "nele_drc_hop";
    int st = drc_check(name, state, state_bytes, max_streams);
    if (st) return st;
    NELE_CHECK_ARG(x && out, "%s: null x / out", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(params, "%s: null params", name);
    const nele_ssdrc_params* p = params;
    NELE_CHECK_ARG(p->attack >= 0.0 && p->attack < 1.0 && p->release >= 0.0 && p->release < 1.0, "%s: attack / release outside [0, 1)", name);
    NELE_CHECK_ARG(p->e0_ratio > 0.0 && std::isfinite(p->e0_ratio), "%s: e0_ratio must be positive and finite", name);
    NELE_CHECK_ARG(p->n_knots >= 2 && p->n_knots <= NELE_SSDRC_MAX_KNOTS, "%s: n_knots=%d outside 2 .. %d", name, p->n_knots, NELE_SSDRC_MAX_KNOTS);
    for (int j = 0; j < p->n_knots; ++j)
        NELE_CHECK_ARG(std::isfinite(p->knot_in_db[j]) && std::isfinite(p->knot_out_db[j]), "%s: knot %d is not finite", name, j);
    for (int j = 0; j + 1 < p->n_knots; ++j) NELE_CHECK_ARG(p->knot_in_db[j] < p->knot_in_db[j + 1], "%s: knot_in_db must ascend", name);
    NELE_CHECK_ARG(rho >= 0.0 && rho < 1.0, "%s: rho=%g must be in [0, 1)", name, rho);
    NELE_CHECK_ARG(lam >= 0.0 && lam < 1.0, "%s: lam=%g must be in [0, 1)", name, lam);
    DrcArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.x = x;
    a.ld = (long long)nh * DRC_BLK;
    a.active = active;
    a.nh = nh;
    a.equalise = equalise != 0;
    a.n_knots = p->n_knots;
    a.attack = p->attack;
    a.release = p->release;
    a.e0_ratio = p->e0_ratio;
    a.rho = rho;
    a.lam = lam;
    for (int j = 0; j < NELE_SSDRC_MAX_KNOTS; ++j) {
        a.kx[j] = j < p->n_knots ? p->knot_in_db[j] : 0.0;
        a.ky[j] = j < p->n_knots ? p->knot_out_db[j] : 0.0;
    }
    for (int k = 0; k < DRC_HIL / 2; ++k) {                 // h[m] = 2 / (pi m) (0.54 + 0.46 cos(pi m / 64)), m = 2 k + 1
        const double m = (double)(2 * k + 1);
        a.hil[k] = 2.0 / (M_PI * m) * (0.54 + 0.46 * std::cos(M_PI * m / (double)DRC_HIL));
    }
    a.ref_level = ref_level;
    a.out = out;
    a.gain = gain;
    a.level = level;
    hipLaunchKernelGGL(drc_hop_kernel, dim3((max_streams + DRC_WAVES - 1) / DRC_WAVES), dim3(64 * DRC_WAVES), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
