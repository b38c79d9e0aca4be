// Residual-echo suppression behind the echo canceller for many concurrent streams (nele_res_*): a spectral post-filter on the
// canceller's residual, driven by the canceller's own echo estimate, on the real-time path's blocks - 256-sample hops, sqrt-Hann
// windowed 512-sample frames, float64 transforms (fft512.h).  The arithmetic is DESIGN.md section 17; tests/res_ref.py restates it
// in numpy.
//   res_hop_kernel : one wave per stream, four streams per workgroup, looping over the call's hops
// A wave keeps its stream's whole state in registers across the call's hops: lane l holds bins 64 m + l (m < 4) of the smoothed
// spectra - lane 0 bin 256 as well - and samples 64 m + l of e_prev, y_prev and the overlap-add tail.  Per hop: one forward complex
// transform of w e + i w y, split into E and Y (the packed half spectrum of fft512.h: slot 0 = (bin 0, bin 256), both real), the gain,
// one inverse transform of the Hermitian extension of G E.  The wave's exchange buffer is the only LDS a stream uses; the twiddle table
// is the workgroup's.  State is read and written with plain loads and stores by the stream's own wave; no atomics, nothing crosses
// waves, and a transform's operands are the stream's own: a slot's bits do not depend on the hop grouping, on B or on the other slots.
// Not in the Makefile's EXACT list: the reference's transform is numpy's pocketfft, whose operation order this one does not share, so
// there is no bit pattern that switching FMA contraction off would preserve; the bounds of section 17 hold with contraction on.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "../../include/nele_hip_ext.h"

namespace {

#define RES_BLK 256                                        // samples per hop = slots per packed spectrum
#define RES_WAVES 4                                        // streams per workgroup
constexpr long long RES_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = the record's bytes (what nele_res_init laid out)
// per-stream record, byte offsets
constexpr long long RES_O_EPREV = 0;                                    // float [256]: the previous hop of `residual` (float32 in, kept exactly)
constexpr long long RES_O_YPREV = RES_O_EPREV + 4 * RES_BLK;            // float [256]: the previous hop of `echo`
constexpr long long RES_O_OLA = RES_O_YPREV + 4 * RES_BLK;              // double [256]: the overlap-add tail o[256:512]
constexpr long long RES_O_SEE = RES_O_OLA + 8 * RES_BLK;                // double [257 (+ 7)]: S_ee
constexpr long long RES_O_SYY = RES_O_SEE + 8 * 264;                    // double [257 (+ 7)]: S_yy
constexpr long long RES_O_SEY = RES_O_SYY + 8 * 264;                    // double2 [257 (+ 7)]: S_ey (imaginary part zero in bins 0 and 256)
constexpr long long RES_REC_BYTES = slot_al(RES_O_SEY + 16 * 264);
static_assert(RES_O_SEY % 16 == 0 && RES_REC_BYTES == 12544, "the record of DESIGN.md section 17");

struct ResArgs {
    unsigned char* state;
    int S;
    const float* residual;       // [S][ld]
    const float* echo;
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double beta, gmin2;          // gmin2 = gmin^2
    float* out;                  // [S][ld]
    double* gains;               // [S][nh][257] or null
};

// w[n] = sqrt(0.5 - 0.5 cos(2 pi n / 512))
__device__ __forceinline__ double res_window(int n) { return sqrt(0.5 - 0.5 * cospi((double)n / 256.0)); }

// step 3: R = |S_ey|^2 / (S_yy + eps), G = sqrt(max(1 - beta R / (S_ee + eps), gmin^2)); sey2 = |S_ey|^2
__device__ __forceinline__ double res_gain(double see, double syy, double sey2, double beta, double gmin2) {
    const double R = sey2 / (syy + NELE_RES_EPS);
    return sqrt(fmax(1.0 - beta * R / (see + NELE_RES_EPS), gmin2));
}

__global__ __launch_bounds__(64 * RES_WAVES) void res_hop_kernel(ResArgs a) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[RES_WAVES][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();                                       // the only workgroup barrier: from here on a wave is on its own
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * RES_WAVES + w;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, (int)RES_REC_BYTES)) return;   // not the state nele_res_init laid out for S: touch nothing
    unsigned char* rec = a.state + RES_HDR_BYTES + (size_t)b * RES_REC_BYTES;
    float* eprevp = reinterpret_cast<float*>(rec + RES_O_EPREV);
    float* yprevp = reinterpret_cast<float*>(rec + RES_O_YPREV);
    double* olap = reinterpret_cast<double*>(rec + RES_O_OLA);
    double* Seep = reinterpret_cast<double*>(rec + RES_O_SEE);
    double* Syyp = reinterpret_cast<double*>(rec + RES_O_SYY);
    double2* Seyp = reinterpret_cast<double2*>(rec + RES_O_SEY);
    double2* xw = xws[w];
    const bool lane0 = (lane == 0);
    const double one_m_smooth = 1.0 - NELE_RES_SMOOTH;
    const double2 zero = make_double2(0.0, 0.0);

    // the stream's state and its window values: element m of each array belongs to index 64 m + lane
    float ep[4], yp[4];
    double ola[4], see[4], syy[4], wlo[4], whi[4];
    double2 sey[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = 64 * m + lane;
        ep[m] = eprevp[j];
        yp[m] = yprevp[j];
        ola[m] = olap[j];
        see[m] = Seep[j];
        syy[m] = Syyp[j];
        sey[m] = Seyp[j];
        wlo[m] = res_window(j);
        whi[m] = res_window(RES_BLK + j);
    }
    double see_ny = 0.0, syy_ny = 0.0, sey_ny = 0.0;       // bin 256 (lane 0)
    if (lane0) {
        see_ny = Seep[RES_BLK];
        syy_ny = Syyp[RES_BLK];
        sey_ny = Seyp[RES_BLK].x;
    }
    const float* resb = a.residual + (size_t)b * a.ld;
    const float* echob = a.echo + (size_t)b * a.ld;
    float* outb = a.out + (size_t)b * a.ld;
    double* gainb = a.gains ? a.gains + (size_t)b * a.nh * 257 : nullptr;

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * RES_BLK;
        // ---- 1. Z = fft512(w [e_prev, e] + i w [y_prev, y]), split into E and Y; e_prev <- e, y_prev <- y
        float en[4], yn[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            en[m] = resb[col + 64 * m + lane];
            yn[m] = echob[col + 64 * m + lane];
        }
        fftw_wave_sync();                                  // the previous hop's reads of xw precede these writes
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int j = 64 * m + lane;
            xw[fftw_slot(j)] = make_double2(wlo[m] * (double)ep[m], wlo[m] * (double)yp[m]);
            xw[fftw_slot(RES_BLK + j)] = make_double2(whi[m] * (double)en[m], whi[m] * (double)yn[m]);
            ep[m] = en[m];
            yp[m] = yn[m];
        }
        fftw_wave_sync();
        double2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = xw[fftw_slot(fftw_n(lane, r))];
        fftw_wave_sync();
        fft512_wave<false>(v, xw, tw, lane);
        fft512_wave_store(v, xw, lane);
        // ---- 2. the smoothed spectra, 3. the gain; ge = G E in the packed layout
        double2 ge[4];
        double g_ny = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = 64 * m + lane;
            double2 E, Y;
            fft512_packed_split(xw, k, E, Y);
            double G;
            if (k == 0) {                                  // bins 0 and 256: E and Y are real there
                see[0] = NELE_RES_SMOOTH * see[0] + one_m_smooth * (E.x * E.x);
                syy[0] = NELE_RES_SMOOTH * syy[0] + one_m_smooth * (Y.x * Y.x);
                sey[0] = make_double2(NELE_RES_SMOOTH * sey[0].x + one_m_smooth * (E.x * Y.x), 0.0);
                see_ny = NELE_RES_SMOOTH * see_ny + one_m_smooth * (E.y * E.y);
                syy_ny = NELE_RES_SMOOTH * syy_ny + one_m_smooth * (Y.y * Y.y);
                sey_ny = NELE_RES_SMOOTH * sey_ny + one_m_smooth * (E.y * Y.y);
                G = res_gain(see[0], syy[0], sey[0].x * sey[0].x, a.beta, a.gmin2);
                g_ny = res_gain(see_ny, syy_ny, sey_ny * sey_ny, a.beta, a.gmin2);
                ge[m] = make_double2(G * E.x, g_ny * E.y);
            } else {
                see[m] = NELE_RES_SMOOTH * see[m] + one_m_smooth * (E.x * E.x + E.y * E.y);
                syy[m] = NELE_RES_SMOOTH * syy[m] + one_m_smooth * (Y.x * Y.x + Y.y * Y.y);
                sey[m] = make_double2(NELE_RES_SMOOTH * sey[m].x + one_m_smooth * (E.x * Y.x + E.y * Y.y),
                                      NELE_RES_SMOOTH * sey[m].y + one_m_smooth * (E.y * Y.x - E.x * Y.y));   // E conj(Y)
                G = res_gain(see[m], syy[m], sey[m].x * sey[m].x + sey[m].y * sey[m].y, a.beta, a.gmin2);
                ge[m] = make_double2(G * E.x, G * E.y);
            }
            if (gainb) gainb[(size_t)h * 257 + k] = G;
        }
        if (gainb && lane0) gainb[(size_t)h * 257 + RES_BLK] = g_ny;
        // ---- 4. o = w irfft512(G E); out = ola + o[0:256], ola <- o[256:512]
        fftw_wave_sync();                                  // every lane's reads of Z precede these writes
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
        const int j = 64 * m + lane;
        eprevp[j] = ep[m];
        yprevp[j] = yp[m];
        olap[j] = ola[m];
        Seep[j] = see[m];
        Syyp[j] = syy[m];
        Seyp[j] = sey[m];
    }
    if (lane0) {
        Seep[RES_BLK] = see_ny;
        Syyp[RES_BLK] = syy_ny;
        Seyp[RES_BLK] = make_double2(sey_ny, 0.0);
    }
}

int res_check(const char* name, const void* state, long long state_bytes, int S) {
    return slot_state_check(name, state, state_bytes, S, []() -> int { return NELE_OK; }, nele_res_state_bytes(S), "nele_res_state_bytes");
}

// slots == null: every record; write_hdr: the header too
int res_reset(const char* name, void* state, int S, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, (int)RES_REC_BYTES};
    return slot_state_reset(name, state, RES_HDR_BYTES, RES_REC_BYTES, S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_res_state_bytes(int max_streams) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS) return -1;
    return RES_HDR_BYTES + (long long)max_streams * RES_REC_BYTES;
}

extern "C" long long nele_res_stream_record_bytes(void) { return RES_REC_BYTES; }

extern "C" int nele_res_init(void* state, long long state_bytes, int max_streams, void* stream) {
    int st = res_check("nele_res_init", state, state_bytes, max_streams);
    if (st) return st;
    return res_reset("nele_res_init", state, max_streams, nullptr, true, stream);
}

extern "C" int nele_res_reset(void* state, long long state_bytes, int max_streams, const unsigned char* slots, void* stream) {
    int st = res_check("nele_res_reset", state, state_bytes, max_streams);
    if (st) return st;
    return res_reset("nele_res_reset", state, max_streams, slots, false, stream);
}

extern "C" int nele_res_hop(void* state, long long state_bytes, int max_streams, const float* residual, const float* echo,
                            const unsigned char* active, int nh, double beta, double gmin, float* out, double* gains, void* stream) {
    int st = res_check("nele_res_hop", state, state_bytes, max_streams);
    if (st) return st;
    NELE_CHECK_ARG(residual && echo && out, "nele_res_hop: null residual / echo / out");
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "nele_res_hop: nh=%d must be in 1 .. 1048576", nh);
    NELE_CHECK_ARG(beta >= 0.0 && beta <= 1e300, "nele_res_hop: beta=%g must be finite and >= 0", beta);
    NELE_CHECK_ARG(gmin > 0.0 && gmin <= 1.0, "nele_res_hop: gmin=%g must be in (0, 1]", gmin);
    ResArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.residual = residual;
    a.echo = echo;
    a.ld = (long long)nh * RES_BLK;
    a.active = active;
    a.nh = nh;
    a.beta = beta;
    a.gmin2 = gmin * gmin;
    a.out = out;
    a.gains = gains;
    hipLaunchKernelGGL(res_hop_kernel, dim3((max_streams + RES_WAVES - 1) / RES_WAVES), dim3(64 * RES_WAVES), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH("nele_res_hop");
    return NELE_OK;
}
