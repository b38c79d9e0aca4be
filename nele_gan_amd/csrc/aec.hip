// Acoustic echo cancellation for many concurrent streams (nele_aec_*): a partitioned-block frequency-domain adaptive filter per stream,
// overlap-save and gradient-constrained (Soo & Pang 1990), on the real-time enhancer's blocks - 256-sample hops, 512-point float64
// transforms (fft512.h).  The arithmetic is DESIGN.md section 14; tests/aec_ref.py restates it in numpy.
//   aec_hop_kernel   : one workgroup per stream and call, looping over the call's hops
//   aec_path_kernel  : the impulse-response estimate, one wave per pair of partitions
// A spectrum of a real 512-sample signal is 256 double2: slot k = bin k for k = 1 .. 255, slot 0 = (bin 0, bin 256) - both real, so
// their imaginary parts are zero by construction and products are taken component-wise in slot 0 (as csrc/fftconv.hip).
// Two real transforms share one complex transform (z = a + i b); the two partitions of a pair share the constraint's inverse and
// forward transform, an odd P leaves the last partition with a zero partner.  Pairs are (0, 1), (2, 3), ... whatever the ring position,
// and a transform's operands are the stream's own: a slot's bits do not depend on the hop grouping, on B or on the other slots.
// State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "../../include/nele_hip.h"

namespace {

#define AEC_BLK 256                                        // samples per hop = slots per spectrum
#define AEC_MAXP NELE_AEC_MAX_PARTITIONS
constexpr long long AEC_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = partitions (what nele_aec_init was given)
// per-stream record, byte offsets
constexpr long long AEC_O_HEAD = 0;                        // int: ring position of the newest far-end spectrum X_0
constexpr long long AEC_O_XPREV = 256;                     // float [256]: the previous hop of `played` (float32 in, kept exactly)
constexpr long long AEC_O_SE = AEC_O_XPREV + 4 * AEC_BLK;  // double [257 (+ 7)]: S_e
constexpr long long AEC_O_X = slot_al(AEC_O_SE + 8 * 264);  // double2 [P][256]: ring of far-end spectra, X_p at (head + p) % P
__host__ __device__ constexpr long long aec_o_w(int P) { return AEC_O_X + 16LL * AEC_BLK * P; }       // double2 [P][256]: W_p
__host__ __device__ constexpr long long aec_rec_bytes(int P) { return slot_al(AEC_O_X + 2 * 16LL * AEC_BLK * P); }

struct AecArgs {
    unsigned char* state;
    int S, P;
    const float* mic;            // [S][ld]
    const float* played;
    long long ld;
    const unsigned char* active; // [S] or null (all)
    const unsigned char* adapt;  // [S] or null (all)
    int nh;
    double mu, gP, delta;        // gP = gamma * P
    float* residual;             // [S][ld]
    float* echo;                 // [S][ld] or null
};

// one wave: spectrum (256 slots, to `out` in LDS) of the real signal whose sample n is val(n)
template <class Val>
__device__ __forceinline__ void aec_forward_real(Val val, double2* __restrict__ xw, const double2* __restrict__ tw, int lane,
                                                 double2* __restrict__ out) {
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = make_double2(val(fftw_n(lane, r)), 0.0);
    fftw_wave_sync();                                      // the wave's earlier reads of xw precede the transform's writes
    fft512_wave<false>(v, xw, tw, lane);
    fft512_wave_store(v, xw, lane);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double2 xa, xb;
        fft512_packed_split(xw, 64 * m + lane, xa, xb);
        out[64 * m + lane] = xa;
    }
}

__global__ __launch_bounds__(256) void aec_hop_kernel(AecArgs a) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[4][FFTW_SLOTS];
    __shared__ double2 specA[AEC_BLK];                     // X_0, then E
    __shared__ double2 specB[AEC_BLK];                     // Y, then G
    __shared__ double ebuf[AEC_BLK];
    __shared__ float xbuf[2 * AEC_BLK];                    // [x_prev, x]
    const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, a.P)) return;      // not the state nele_aec_init laid out for (S, P): touch nothing
    const int P = a.P;
    unsigned char* rec = a.state + AEC_HDR_BYTES + (size_t)b * aec_rec_bytes(P);
    int* headp = reinterpret_cast<int*>(rec + AEC_O_HEAD);
    float* xprev = reinterpret_cast<float*>(rec + AEC_O_XPREV);
    double* Sep = reinterpret_cast<double*>(rec + AEC_O_SE);
    double2* ring = reinterpret_cast<double2*>(rec + AEC_O_X);
    double2* Wst = reinterpret_cast<double2*>(rec + aec_o_w(P));
    const bool adapt = !a.adapt || a.adapt[b];
    const bool slot0 = (t == 0);
    const double one_m_smooth = 1.0 - NELE_AEC_SMOOTH;
    double2* xw = xws[w];

    fft512_fill_twiddles(tw);
    xbuf[t] = xprev[t];
    int head = min(max(*headp, 0), P - 1);
    double se = Sep[t], se_ny = slot0 ? Sep[AEC_BLK] : 0.0;   // S_e of bin t (thread 0: bins 0 and 256)
    const float* micb = a.mic + (size_t)b * a.ld;
    const float* plb = a.played + (size_t)b * a.ld;
    float* resb = a.residual + (size_t)b * a.ld;
    float* echob = a.echo ? a.echo + (size_t)b * a.ld : nullptr;
    __syncthreads();

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * AEC_BLK;
        // ---- 1. X_0 = rfft512([x_prev, x]) (wave 0)
        if (w == 0) {
            float xs[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                xs[m] = plb[col + 64 * m + lane];
                xbuf[AEC_BLK + 64 * m + lane] = xs[m];
            }
            fftw_wave_sync();
            aec_forward_real([&](int n) { return (double)xbuf[n]; }, xw, tw, lane, specA);
#pragma unroll
            for (int m = 0; m < 4; ++m) xbuf[64 * m + lane] = xs[m];          // x_prev <- x (every read of xbuf above is behind a wave sync)
        }
        __syncthreads();
        // ---- 2. the ring moves up one place; Y = sum_p W_p X_p and sum_p |X_p|^2 in ascending p (thread t: slot t)
        head = (head == 0) ? P - 1 : head - 1;
        const double2 X0 = specA[t];
        ring[(size_t)head * AEC_BLK + t] = X0;
        double2 Y = make_double2(0.0, 0.0);
        double sa = 0.0, sb = 0.0;                         // sum |X_p|^2 (slot 0: bin 0 in sa, bin 256 in sb)
        for (int p = 0; p < P; ++p) {
            int rp = head + p;
            if (rp >= P) rp -= P;
            const double2 X = (p == 0) ? X0 : ring[(size_t)rp * AEC_BLK + t];
            const double2 W = Wst[(size_t)p * AEC_BLK + t];
            if (slot0) {
                Y.x = fma(W.x, X.x, Y.x);
                Y.y = fma(W.y, X.y, Y.y);
                sa = fma(X.x, X.x, sa);
                sb = fma(X.y, X.y, sb);
            } else {
                Y.x += W.x * X.x - W.y * X.y;
                Y.y += W.x * X.y + W.y * X.x;
                sa += X.x * X.x + X.y * X.y;
            }
        }
        specB[t] = Y;
        __syncthreads();
        // ---- 3. y = irfft512(Y)[256:], e = d - y, E = rfft512([0 x 256, e]) (wave 0)
        if (w == 0) {
            const double2 y0 = specB[0], zero = make_double2(0.0, 0.0);
            double2 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int n = fftw_n(lane, r);
                const int k = (n <= 256) ? n : 512 - n;
                v[r] = fft512_packed_join(specB[k & 255], zero, y0, zero, n);
            }
            fftw_wave_sync();
            fft512_wave<true>(v, xw, tw, lane);
#pragma unroll
            for (int m = 4; m < 8; ++m) {                  // v[m].x = 512 y[64 m + lane]
                const int j = 64 * (m - 4) + lane;
                const double y = v[m].x * (1.0 / 512.0);
                const double e = (double)micb[col + j] - y;
                resb[col + j] = (float)e;
                if (echob) echob[col + j] = (float)y;
                ebuf[j] = e;
            }
            fftw_wave_sync();
            aec_forward_real([&](int n) { return (n >= AEC_BLK) ? ebuf[n - AEC_BLK] : 0.0; }, xw, tw, lane, specA);
        }
        __syncthreads();
        // ---- 4. S_e (always), then G = mu E / D
        {
            const double2 E = specA[t];
            double2 G;
            if (slot0) {
                se = NELE_AEC_SMOOTH * se + one_m_smooth * (E.x * E.x);
                se_ny = NELE_AEC_SMOOTH * se_ny + one_m_smooth * (E.y * E.y);
                G = make_double2(a.mu * E.x / (sa + a.gP * se + a.delta), a.mu * E.y / (sb + a.gP * se_ny + a.delta));
            } else {
                se = NELE_AEC_SMOOTH * se + one_m_smooth * (E.x * E.x + E.y * E.y);
                const double D = sa + a.gP * se + a.delta;
                G = make_double2(a.mu * E.x / D, a.mu * E.y / D);
            }
            specB[t] = G;
        }
        __syncthreads();
        // ---- 5. W_p += rfft512(first half of irfft512(conj(X_p) G)), one wave per pair of partitions
        if (adapt) {
            for (int q = w; 2 * q < P; q += 4) {
                const int p0 = 2 * q, p1 = p0 + 1;
                const bool two = p1 < P;
                int r0 = head + p0, r1 = head + p1;
                if (r0 >= P) r0 -= P;
                if (r1 >= P) r1 -= P;
                const double2* Xa = ring + (size_t)r0 * AEC_BLK;
                const double2* Xb = ring + (size_t)(two ? r1 : r0) * AEC_BLK;
                fftw_wave_sync();                          // the previous pair's reads of xw precede these writes
#pragma unroll
                for (int m = 0; m < 4; ++m) {              // conj(X) G of both partitions: slots [0, 256) and [256, 512) of xw
                    const int k = 64 * m + lane;
                    const double2 G = specB[k], xa = Xa[k], xb = Xb[k];
                    double2 ga, gb;
                    if (k == 0) {
                        ga = make_double2(xa.x * G.x, xa.y * G.y);
                        gb = make_double2(xb.x * G.x, xb.y * G.y);
                    } else {
                        ga = make_double2(xa.x * G.x + xa.y * G.y, xa.x * G.y - xa.y * G.x);
                        gb = make_double2(xb.x * G.x + xb.y * G.y, xb.x * G.y - xb.y * G.x);
                    }
                    if (!two) gb = make_double2(0.0, 0.0);
                    xw[k] = ga;
                    xw[AEC_BLK + k] = gb;
                }
                fftw_wave_sync();
                const double2 a0 = xw[0], b0 = xw[AEC_BLK];
                double2 v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int n = fftw_n(lane, r);
                    const int k = ((n <= 256) ? n : 512 - n) & 255;
                    v[r] = fft512_packed_join(xw[k], xw[AEC_BLK + k], a0, b0, n);
                }
                fftw_wave_sync();
                fft512_wave<true>(v, xw, tw, lane);        // v[m] = 512 (g_a + i g_b)[64 m + lane]
#pragma unroll
                for (int m = 0; m < 4; ++m) v[m] = make_double2(v[m].x * (1.0 / 512.0), v[m].y * (1.0 / 512.0));
#pragma unroll
                for (int m = 4; m < 8; ++m) v[m] = make_double2(0.0, 0.0);     // the constraint: g[256:512] = 0
                fft512_wave_store(v, xw, lane);
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = xw[fftw_slot(fftw_n(lane, r))];
                fftw_wave_sync();
                fft512_wave<false>(v, xw, tw, lane);
                fft512_wave_store(v, xw, lane);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int k = 64 * m + lane;
                    double2 da, db;
                    fft512_packed_split(xw, k, da, db);
                    double2* Wa = Wst + (size_t)p0 * AEC_BLK + k;
                    const double2 wa = *Wa;
                    *Wa = make_double2(wa.x + da.x, wa.y + da.y);
                    if (two) {
                        double2* Wb = Wst + (size_t)p1 * AEC_BLK + k;
                        const double2 wb = *Wb;
                        *Wb = make_double2(wb.x + db.x, wb.y + db.y);
                    }
                }
            }
        }
        __syncthreads();                                   // W and the ring are the next hop's operands; specA / specB are free again
    }
    xprev[t] = xbuf[t];
    Sep[t] = se;
    if (slot0) {
        Sep[AEC_BLK] = se_ny;
        *headp = head;
    }
}

// h[b][256 p + n] = irfft512(W_p)[n], n < 256.  grid (S, ceil(ceil(P / 2) / 4)), block 256: one wave per pair of partitions.
__global__ __launch_bounds__(256) void aec_path_kernel(const unsigned char* __restrict__ state, int S, int P, double* __restrict__ hout) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[4][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (b >= S || !slot_hdr_matches(state, S, P)) return;
    const int p0 = 2 * (blockIdx.y * 4 + w), p1 = p0 + 1;
    if (p0 >= P) return;
    const bool two = p1 < P;
    const double2* Wst = reinterpret_cast<const double2*>(state + AEC_HDR_BYTES + (size_t)b * aec_rec_bytes(P) + aec_o_w(P));
    const double2* Wa = Wst + (size_t)p0 * AEC_BLK;
    const double2* Wb = Wst + (size_t)(two ? p1 : p0) * AEC_BLK;
    double2* xw = xws[w];
    const double2 zero = make_double2(0.0, 0.0);
    const double2 a0 = Wa[0], b0 = two ? Wb[0] : zero;
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = fftw_n(lane, r);
        const int k = ((n <= 256) ? n : 512 - n) & 255;
        v[r] = fft512_packed_join(Wa[k], two ? Wb[k] : zero, a0, b0, n);
    }
    fft512_wave<true>(v, xw, tw, lane);
    double* hb = hout + (size_t)b * P * AEC_BLK;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int n = 64 * m + lane;
        hb[(size_t)p0 * AEC_BLK + n] = v[m].x * (1.0 / 512.0);
        if (two) hb[(size_t)p1 * AEC_BLK + n] = v[m].y * (1.0 / 512.0);
    }
}

int aec_check(const char* name, const void* state, long long state_bytes, int S, int P) {
    auto params = [&]() -> int {
        NELE_CHECK_ARG(P >= 1 && P <= AEC_MAXP, "%s: partitions=%d must be in 1 .. %d", name, P, AEC_MAXP);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_aec_state_bytes(S, P), "nele_aec_state_bytes", P);
}

// slots == null: every record; write_hdr: the header too
int aec_reset(const char* name, void* state, int S, int P, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, P};
    return slot_state_reset(name, state, AEC_HDR_BYTES, aec_rec_bytes(P), S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_aec_state_bytes(int max_streams, int partitions) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || partitions < 1 || partitions > AEC_MAXP) return -1;
    return AEC_HDR_BYTES + (long long)max_streams * aec_rec_bytes(partitions);
}

extern "C" long long nele_aec_stream_record_bytes(int partitions) {
    if (partitions < 1 || partitions > AEC_MAXP) return -1;
    return aec_rec_bytes(partitions);
}

extern "C" int nele_aec_init(void* state, long long state_bytes, int max_streams, int partitions, void* stream) {
    int st = aec_check("nele_aec_init", state, state_bytes, max_streams, partitions);
    if (st) return st;
    return aec_reset("nele_aec_init", state, max_streams, partitions, nullptr, true, stream);
}

extern "C" int nele_aec_reset(void* state, long long state_bytes, int max_streams, int partitions, const unsigned char* slots, void* stream) {
    int st = aec_check("nele_aec_reset", state, state_bytes, max_streams, partitions);
    if (st) return st;
    return aec_reset("nele_aec_reset", state, max_streams, partitions, slots, false, stream);
}

extern "C" int nele_aec_hop(void* state, long long state_bytes, int max_streams, int partitions, const float* mic, const float* played,
                            const unsigned char* active, const unsigned char* adapt, int nh, double mu, double gamma, double delta,
                            float* residual, float* echo, void* stream) {
    int st = aec_check("nele_aec_hop", state, state_bytes, max_streams, partitions);
    if (st) return st;
    NELE_CHECK_ARG(mic && played && residual, "nele_aec_hop: null mic / played / residual");
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "nele_aec_hop: nh=%d must be in 1 .. 1048576", nh);
    NELE_CHECK_ARG(mu > 0.0 && mu < 2.0, "nele_aec_hop: mu=%g must be in (0, 2)", mu);
    NELE_CHECK_ARG(gamma >= 0.0 && gamma <= 1e300, "nele_aec_hop: gamma=%g must be finite and >= 0", gamma);
    NELE_CHECK_ARG(delta > 0.0 && delta <= 1e300, "nele_aec_hop: delta=%g must be finite and > 0", delta);
    AecArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.P = partitions;
    a.mic = mic;
    a.played = played;
    a.ld = (long long)nh * AEC_BLK;
    a.active = active;
    a.adapt = adapt;
    a.nh = nh;
    a.mu = mu;
    a.gP = gamma * (double)partitions;
    a.delta = delta;
    a.residual = residual;
    a.echo = echo;
    hipLaunchKernelGGL(aec_hop_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH("nele_aec_hop");
    return NELE_OK;
}

extern "C" int nele_aec_echo_path(const void* state, long long state_bytes, int max_streams, int partitions, double* h, void* stream) {
    int st = aec_check("nele_aec_echo_path", state, state_bytes, max_streams, partitions);
    if (st) return st;
    NELE_CHECK_ARG(h, "nele_aec_echo_path: null h");
    const int pairs = (partitions + 1) / 2;
    hipLaunchKernelGGL(aec_path_kernel, dim3(max_streams, (pairs + 3) / 4), dim3(256), 0, as_stream(stream), (const unsigned char*)state, max_streams,
                       partitions, h);
    NELE_CHECK_LAUNCH("nele_aec_echo_path");
    return NELE_OK;
}
