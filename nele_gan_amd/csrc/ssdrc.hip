// SSDRC: spectral shaping and dynamic range compression of clean speech (Zorila, Kandia and Stylianou, Interspeech 2012) - the
// pre-enhanced 'MultiEnh' examples of the training loop and the `ssdrc` baseline of the scoring path, made from the clean signal alone.
// The algorithm is the one DESIGN.md section 11 fixes (every choice the paper leaves open is made there); this file states it once more
// only where a kernel needs it.  x [B][Lmax] float32 with lengths [B]; everything between the input and the output is float64.
//   ssdrc_tables_kernel   : window, fixed shaping H_r, pre-emphasis ramp, Hilbert taps - depend on nothing, written once per call
//   ssdrc_voicing_kernel  : per frame rms / max(zero crossings, 1), divided by the row's maximum -> P_v [B][NF]     (one workgroup per row)
//   ssdrc_shape_kernel    : one wave per PAIR of frames, four complex 512-point transforms (fft512_wave) for the pair's eight real ones:
//                           a + i b -> X_a, X_b;  l_a + i l_b -> cepstra;  liftered cepstra -> ln(E/T);  Y_a + i Y_b -> windowed frames
//   ssdrc_ola_kernel      : s[n] = frame(n / 256)[256 + n % 256] + frame(n / 256 + 1)[n % 256]  (two summands: no order to fix)
//   ssdrc_envelope_kernel : Hilbert FIR, magnitude, 161-sample centred mean from an LDS tile with a halo of 64 + 80 samples each side
//   ssdrc_gain_kernel     : one wave per row: row maximum of e, then blocks of e through LDS - lane 0 runs the attack / release chain
//                           (a data-dependent recursion: no prefix form), all lanes apply the static curve and the gain
//   ssdrc_final_kernel    : sum x^2 and sum y^2 of the row in ONE summation order, y *= sqrt(sum x^2 / sum y^2), float32, zeros behind the end
// Every reduction stays inside its row in a fixed order and no kernel reads another row: a row's bits do not depend on B, on Lmax or on
// its position in the batch.  With both stages off sum y^2 is sum x^2 bit for bit, the scale is 1.0 and the output is the input.
#include "common.h"
#include "fft512.h"
#include "ws_arena.h"
#include <cmath>
#include "../../include/nele_hip.h"

#define SS_N 512
#define SS_HOP 256
#define SS_HIL 64                      // Hilbert FIR half-length: odd taps 1, 3 .. 63 (the even ones are zero)
#define SS_AVG 80                      // half-width of the centred mean (161 samples)
#define SS_TILE 1024                   // samples per workgroup of the envelope and overlap-add kernels
#define SS_BLK 2048                    // samples per block of the gain kernel
#define SS_TAB_WIN 0
#define SS_TAB_HR 512
#define SS_TAB_PRE 1024
#define SS_TAB_HIL 1536
#define SS_TAB_DOUBLES 1568

struct SsCurve {
    int n;
    double e0_ratio, attack, release;
    double kx[NELE_SSDRC_MAX_KNOTS], ky[NELE_SSDRC_MAX_KNOTS];
};

__device__ __forceinline__ int ss_row_length(const int* lengths, int b, int Lmax) {
    return lengths ? min(max(lengths[b], 0), Lmax) : Lmax;
}
__host__ __device__ static inline int ss_frames(int len) { return (len + SS_HOP - 1) / SS_HOP + 1; }     // t = 0 .. ceil(len / 256)

__global__ __launch_bounds__(512) void ssdrc_tables_kernel(double* __restrict__ tab) {
    const int k = threadIdx.x;
    tab[SS_TAB_WIN + k] = sqrt(0.5 - 0.5 * cospi((double)k / 256.0));
    const double f = 31.25 * (double)min(k, SS_N - k);
    double db;
    if (f < 500.0) db = -6.0 * log2(500.0 / fmax(f, 31.25));
    else if (f <= 1000.0) db = 0.0;
    else if (f <= 4000.0) db = 12.0 * log2(f / 1000.0);
    else db = 24.0;
    tab[SS_TAB_HR + k] = pow(10.0, db / 20.0);
    tab[SS_TAB_PRE + k] = fmax(f - 1000.0, 0.0) / 7000.0;
    if (k < SS_HIL / 2) {
        const double m = (double)(2 * k + 1);
        tab[SS_TAB_HIL + k] = 2.0 / (M_PI * m) * (0.54 + 0.46 * cospi(m / (double)SS_HIL));
    }
}

// grid B, block 1024: wave w takes frames w, w + 16, ..; a lane holds 8 consecutive samples of the frame and the one before them
__global__ __launch_bounds__(1024) void ssdrc_voicing_kernel(const float* __restrict__ x, const int* __restrict__ lengths, int Lmax, int NF,
                                                             double* __restrict__ pv) {
    __shared__ double red[16];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int len = ss_row_length(lengths, b, Lmax), nfr = ss_frames(len);
    const float* xb = x + (size_t)b * Lmax;
    double* pb = pv + (size_t)b * NF;
    double vmax = 0.0;
    for (int t = wv; t < nfr; t += 16) {
        const int g0 = SS_HOP * t - SS_HOP + 8 * lane;
        double ss = 0.0, z = 0.0;
        double prev = (lane > 0 && g0 - 1 >= 0 && g0 - 1 < len) ? (double)xb[g0 - 1] : 0.0;      // (sample 0 of the frame has no predecessor)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int g = g0 + i;
            const double s = (g >= 0 && g < len) ? (double)xb[g] : 0.0;
            ss += s * s;
            if ((lane > 0 || i > 0) && s * prev < 0.0) z += 1.0;
            prev = s;
        }
        ss = wave_sum(ss);
        z = wave_sum(z);
        const double v = sqrt(ss / (double)SS_N) / fmax(z, 1.0);
        if (lane == 0) pb[t] = v;
        vmax = fmax(vmax, v);
    }
    vmax = block_max(vmax, red);
    if (lane == 0)
        for (int t = wv; t < nfr; t += 16) pb[t] = vmax > 0.0 ? pb[t] / vmax : 0.0;               // (the thread reads what it wrote itself)
}

// the natural-order array the wave left in xw (fft512_wave_store) -> the transform's input order
__device__ __forceinline__ void ss_restage(double2 (&v)[8], double2* __restrict__ xw, int lane) {
    fft512_wave_store(v, xw, lane);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = xw[fftw_slot(fftw_n(lane, r))];
    fftw_wave_sync();                                        // the wave's reads precede the transform's writes to the same LDS
}

// grid (ceil(ceil(NF / 2) / 4), B), block 256: wave w of workgroup g shapes frames ta = 2 (4 g + w) and ta + 1 of row b into
// fr[b][t][512] (the windowed output frames, before overlap-add).  Frames behind the row's last one are not computed.
__global__ __launch_bounds__(256) void ssdrc_shape_kernel(const float* __restrict__ x, const int* __restrict__ lengths, int Lmax, int NF,
                                                          const double* __restrict__ tab, const double* __restrict__ pv, int Q, double beta,
                                                          double g, double* __restrict__ fr) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[4][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();
    const int b = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int len = ss_row_length(lengths, b, Lmax), nfr = ss_frames(len);
    const int ta = (blockIdx.x * 4 + w) * 2;
    if (ta >= nfr) return;                                   // (wave-uniform; no workgroup barrier below)
    const bool has_b = ta + 1 < nfr;
    double2* xw = xws[w];
    const float* xb = x + (size_t)b * Lmax;
    const double* win = tab + SS_TAB_WIN;
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = fftw_n(lane, r);
        const int ga = SS_HOP * ta - SS_HOP + n, gb = ga + SS_HOP;
        const double wn = win[n];
        const double sa = (ga >= 0 && ga < len) ? (double)xb[ga] : 0.0;
        const double sb = (has_b && gb >= 0 && gb < len) ? (double)xb[gb] : 0.0;
        v[r] = make_double2(sa * wn, sb * wn);
    }
    fft512_wave<false>(v, xw, tw, lane);                     // Z = FFT(a + i b): v[m] = Z[64 m + lane]
    fft512_wave_store(v, xw, lane);
    double2 Xa[8], Xb[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = 64 * m + lane;
        const double2 zk = v[m], zn = xw[fftw_slot((SS_N - k) & (SS_N - 1))];
        fft512_pair_split(zk, zn, Xa[m], Xb[m]);
        v[m] = make_double2(0.5 * log(fmax(Xa[m].x * Xa[m].x + Xa[m].y * Xa[m].y, 1e-20)),
                            0.5 * log(fmax(Xb[m].x * Xb[m].x + Xb[m].y * Xb[m].y, 1e-20)));
    }
    fftw_wave_sync();                                        // every lane has read its mirrored bins
    ss_restage(v, xw, lane);
    fft512_wave<true>(v, xw, tw, lane);                      // 512 (c_a + i c_b): both log spectra are real and even, so are their cepstra
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int q = 64 * m + lane;
        const bool keep = (q >= 2 && q <= Q) || (q >= SS_N - Q && q <= SS_N - 2);
        v[m] = keep ? make_double2(v[m].x * (1.0 / 512.0), v[m].y * (1.0 / 512.0)) : make_double2(0.0, 0.0);
    }
    fftw_wave_sync();
    ss_restage(v, xw, lane);
    fft512_wave<false>(v, xw, tw, lane);                     // ln(E/T)_a + i ln(E/T)_b at k = 64 m + lane
    const double pa = pv[(size_t)b * NF + ta], pb = has_b ? pv[(size_t)b * NF + ta + 1] : 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int k = 64 * m + lane;
        const double hr = tab[SS_TAB_HR + k], pre = tab[SS_TAB_PRE + k];
        const double ga = exp(beta * pa * v[m].x) * (1.0 + g * pa * pre) * hr;
        const double gb = exp(beta * pb * v[m].y) * (1.0 + g * pb * pre) * hr;
        const double2 ya = make_double2(Xa[m].x * ga, Xa[m].y * ga), yb = make_double2(Xb[m].x * gb, Xb[m].y * gb);
        v[m] = make_double2(ya.x - yb.y, ya.y + yb.x);       // Y_a + i Y_b
    }
    fftw_wave_sync();
    ss_restage(v, xw, lane);
    fft512_wave<true>(v, xw, tw, lane);                      // 512 (y_a + i y_b)[64 m + lane]
    double* fa = fr + ((size_t)b * NF + ta) * SS_N;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int n = 64 * m + lane;
        const double wn = win[n] * (1.0 / 512.0);
        fa[n] = v[m].x * wn;
        if (has_b) fa[SS_N + n] = v[m].y * wn;
    }
}

// grid (ceil(Lmax / SS_TILE), B), block 256.  fr == NULL (shaping off): s = (double)x.  Zeros behind the row's end.
__global__ __launch_bounds__(256) void ssdrc_ola_kernel(const float* __restrict__ x, const double* __restrict__ fr, const int* __restrict__ lengths,
                                                        int Lmax, int NF, double* __restrict__ s) {
    const int b = blockIdx.y;
    const int len = ss_row_length(lengths, b, Lmax);
    const int n1 = min(Lmax, (int)(blockIdx.x + 1) * SS_TILE);
    for (int n = blockIdx.x * SS_TILE + threadIdx.x; n < n1; n += 256) {
        double v = 0.0;
        if (n < len) {
            if (fr) {
                const int h = n / SS_HOP, r = n % SS_HOP;
                const double* f0 = fr + ((size_t)b * NF + h) * SS_N;          // frames h and h + 1 <= ceil(len / 256) exist for n < len
                v = f0[SS_HOP + r] + f0[SS_N + r];
            } else {
                v = (double)x[(size_t)b * Lmax + n];
            }
        }
        s[(size_t)b * Lmax + n] = v;
    }
}

// grid (ceil(Lmax / SS_TILE), B), block 256: e[n] for the tile's n < len (tiles behind the row's end do nothing)
__global__ __launch_bounds__(256) void ssdrc_envelope_kernel(const double* __restrict__ s, const int* __restrict__ lengths, int Lmax,
                                                             const double* __restrict__ tab, double* __restrict__ e) {
    __shared__ double ss[SS_TILE + 2 * (SS_HIL + SS_AVG)];   // s at tile0 - 144 + i
    __shared__ double aa[SS_TILE + 2 * SS_AVG];              // a at tile0 - 80 + i
    __shared__ double hil[SS_HIL / 2];
    const int b = blockIdx.y, tid = threadIdx.x, tile0 = blockIdx.x * SS_TILE;
    const int len = ss_row_length(lengths, b, Lmax);
    if (tile0 >= len) return;                                // (workgroup-uniform)
    const double* sb = s + (size_t)b * Lmax;
    if (tid < SS_HIL / 2) hil[tid] = tab[SS_TAB_HIL + tid];
    for (int i = tid; i < SS_TILE + 2 * (SS_HIL + SS_AVG); i += 256) {
        const int g = tile0 - (SS_HIL + SS_AVG) + i;
        ss[i] = (g >= 0 && g < len) ? sb[g] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < SS_TILE + 2 * SS_AVG; i += 256) {
        const int g = tile0 - SS_AVG + i, c = i + SS_HIL;
        double a = 0.0;
        if (g >= 0 && g < len) {
            double sh = 0.0;
#pragma unroll 8
            for (int j = 0; j < SS_HIL / 2; ++j) sh += hil[j] * (ss[c - (2 * j + 1)] - ss[c + (2 * j + 1)]);
            a = sqrt(ss[c] * ss[c] + sh * sh);
        }
        aa[i] = a;
    }
    __syncthreads();
    for (int i = tid; i < SS_TILE; i += 256) {
        const int g = tile0 + i;
        if (g < len) {
            double acc = 0.0;
#pragma unroll 7
            for (int j = 0; j <= 2 * SS_AVG; ++j) acc += aa[i + j];
            e[(size_t)b * Lmax + g] = acc / (double)(2 * SS_AVG + 1);
        }
    }
}

__device__ __forceinline__ double ss_curve(const SsCurve& c, double xin) {
    if (xin < c.kx[0]) return xin + (c.ky[0] - c.kx[0]);     // unity slope below the first knot
    double out = c.ky[c.n - 1];                              // a limiter above the last one
    for (int j = 0; j + 1 < c.n; ++j)
        if (xin >= c.kx[j] && xin < c.kx[j + 1]) out = c.ky[j] + (xin - c.kx[j]) * ((c.ky[j + 1] - c.ky[j]) / (c.kx[j + 1] - c.kx[j]));
    return out;
}

// grid B, block 64: y may alias s (an element is read and written by the same lane).  ehat may be NULL.
__global__ __launch_bounds__(64) void ssdrc_gain_kernel(const double* s, const double* __restrict__ e, const int* __restrict__ lengths, int Lmax,
                                                        SsCurve cv, double* y, double* __restrict__ ehat) {
    __shared__ double eb[SS_BLK];
    __shared__ double carry;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = ss_row_length(lengths, b, Lmax);
    const size_t base = (size_t)b * Lmax;
    double mx = 0.0;
    for (int i = lane; i < len; i += 64) mx = fmax(mx, e[base + i]);
    mx = wave_max(mx);
    const double e0 = cv.e0_ratio * mx;
    if (lane == 0) carry = 0.0;
    for (int c0 = 0; c0 < len; c0 += SS_BLK) {
        const int nc = min(SS_BLK, len - c0);
        __syncthreads();
        for (int i = lane; i < nc; i += 64) eb[i] = e[base + c0 + i];
        __syncthreads();
        if (lane == 0) {                                     // the chain, in sample order
            double p = carry;
            for (int i = 0; i < nc; ++i) {
                const double ev = eb[i];
                const double a = ev >= p ? cv.attack : cv.release;
                p = a * p + (1.0 - a) * ev;
                eb[i] = p;
            }
            carry = p;
        }
        __syncthreads();
        for (int i = lane; i < nc; i += 64) {
            const double eh = eb[i];
            double gain = 1.0;
            if (e0 > 0.0) {
                const double xin = 20.0 * log10(fmax(eh, 1e-10 * e0) / e0);
                gain = pow(10.0, (ss_curve(cv, xin) - xin) / 20.0);
            }
            y[base + c0 + i] = gain * s[base + c0 + i];
            if (ehat) ehat[base + c0 + i] = eh;
        }
    }
    for (int i = len + lane; i < Lmax; i += 64) {
        y[base + i] = 0.0;
        if (ehat) ehat[base + i] = 0.0;
    }
}

// grid B, block 1024: equal energy.  Both sums run thread-strided and through block_sum in the same order.
__global__ __launch_bounds__(1024) void ssdrc_final_kernel(const float* __restrict__ x, const double* __restrict__ yd, const int* __restrict__ lengths,
                                                           int Lmax, float* __restrict__ y) {
    __shared__ double red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = ss_row_length(lengths, b, Lmax);
    const size_t base = (size_t)b * Lmax;
    double sx = 0.0, sy = 0.0;
    for (int i = tid; i < len; i += 1024) {
        const double xv = (double)x[base + i], yv = yd[base + i];
        sx += xv * xv;
        sy += yv * yv;
    }
    sx = block_sum(sx, red);
    sy = block_sum(sy, red);
    const double scale = sy > 0.0 ? sqrt(sx / sy) : 0.0;
    for (int i = tid; i < Lmax; i += 1024) y[base + i] = i < len ? (float)(yd[base + i] * scale) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------- host
static inline long long ss_align256(long long v) { return (long long)ws_round256((size_t)v); }
static inline int ss_nf(int Lmax) { return ss_frames(Lmax); }

struct SsLayout {
    long long tab, pv, fr, s1, e, total;
};
static SsLayout ss_layout(int B, int Lmax) {
    SsLayout l;
    const long long NF = ss_nf(Lmax), BL = ss_align256((long long)B * Lmax * (long long)sizeof(double));
    l.tab = 0;
    l.pv = l.tab + ss_align256(SS_TAB_DOUBLES * (long long)sizeof(double));
    l.fr = l.pv + ss_align256((long long)B * NF * (long long)sizeof(double));
    l.s1 = l.fr + ss_align256((long long)B * NF * SS_N * (long long)sizeof(double));
    l.e = l.s1 + BL;
    l.total = l.e + BL;
    return l;
}

static int ss_check(const char* name, const void* in, const void* out, int B, int Lmax, const nele_ssdrc_params* p, const void* ws) {
    NELE_CHECK_ARG(in && out && p && ws, "%s: null input, output, params or workspace", name);
    NELE_CHECK_ARG(B > 0 && B <= 65535 && Lmax > 0 && Lmax <= NELE_SSDRC_MAX_SAMPLES, "%s: B=%d outside 1 .. 65535 or Lmax=%d outside 1 .. %d", name, B,
                   Lmax, NELE_SSDRC_MAX_SAMPLES);
    NELE_CHECK_ARG(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", name);
    NELE_CHECK_ARG(p->lifter_q >= 2 && p->lifter_q <= 255, "%s: lifter_q=%d outside 2 .. 255", name, p->lifter_q);
    NELE_CHECK_ARG(std::isfinite(p->beta) && std::isfinite(p->preemph), "%s: beta / preemph is not finite", name);
    NELE_CHECK_ARG(p->attack >= 0.0 && p->attack < 1.0 && p->release >= 0.0 && p->release < 1.0, "%s: attack / release outside [0, 1)", name);
    NELE_CHECK_ARG(p->e0_ratio > 0.0, "%s: e0_ratio must be positive", name);
    NELE_CHECK_ARG(p->n_knots >= 2 && p->n_knots <= NELE_SSDRC_MAX_KNOTS, "%s: n_knots=%d outside 2 .. %d", name, p->n_knots, NELE_SSDRC_MAX_KNOTS);
    for (int j = 0; j < p->n_knots; ++j)
        NELE_CHECK_ARG(std::isfinite(p->knot_in_db[j]) && std::isfinite(p->knot_out_db[j]), "%s: knot %d is not finite", name, j);
    for (int j = 0; j + 1 < p->n_knots; ++j)
        NELE_CHECK_ARG(p->knot_in_db[j] < p->knot_in_db[j + 1], "%s: knot_in_db must ascend", name);
    return NELE_OK;
}

static SsCurve ss_curve_of(const nele_ssdrc_params* p) {
    SsCurve c;
    c.n = p->n_knots;
    c.e0_ratio = p->e0_ratio;
    c.attack = p->attack;
    c.release = p->release;
    for (int j = 0; j < NELE_SSDRC_MAX_KNOTS; ++j) {
        c.kx[j] = j < p->n_knots ? p->knot_in_db[j] : 0.0;
        c.ky[j] = j < p->n_knots ? p->knot_out_db[j] : 0.0;
    }
    return c;
}

// stage 1 into s [B][Lmax] float64 (zeros behind each row's end)
static int ss_launch_shape(const char* name, const float* x, const int* lengths, int B, int Lmax, const nele_ssdrc_params* p, double* s, char* ws,
                           hipStream_t st) {
    const SsLayout l = ss_layout(B, Lmax);
    const int NF = ss_nf(Lmax);
    double* tab = (double*)(ws + l.tab);
    double* pv = (double*)(ws + l.pv);
    double* fr = (double*)(ws + l.fr);
    const dim3 tiles((Lmax + SS_TILE - 1) / SS_TILE, B);
    if (p->shape) {
        NELE_PROF("ssdrc_voicing", st, hipLaunchKernelGGL(ssdrc_tables_kernel, dim3(1), dim3(512), 0, st, tab);
                  hipLaunchKernelGGL(ssdrc_voicing_kernel, dim3(B), dim3(1024), 0, st, x, lengths, Lmax, NF, pv));
        NELE_PROF("ssdrc_shape", st, hipLaunchKernelGGL(ssdrc_shape_kernel, dim3(((NF + 1) / 2 + 3) / 4, B), dim3(256), 0, st, x, lengths, Lmax, NF,
                                                        (const double*)tab, (const double*)pv, p->lifter_q, p->beta, p->preemph, fr));
    }
    NELE_PROF("ssdrc_ola", st, hipLaunchKernelGGL(ssdrc_ola_kernel, tiles, dim3(256), 0, st, x, p->shape ? (const double*)fr : (const double*)nullptr,
                                                  lengths, Lmax, NF, s));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

// stage 2: s -> y (may alias s), ehat optional
static int ss_launch_compress(const char* name, const double* s, const int* lengths, int B, int Lmax, const nele_ssdrc_params* p, double* y,
                              double* ehat, char* ws, bool tables, hipStream_t st) {
    const SsLayout l = ss_layout(B, Lmax);
    double* tab = (double*)(ws + l.tab);
    double* e = (double*)(ws + l.e);
    const dim3 tiles((Lmax + SS_TILE - 1) / SS_TILE, B);
    if (tables) hipLaunchKernelGGL(ssdrc_tables_kernel, dim3(1), dim3(512), 0, st, tab);
    NELE_PROF("ssdrc_envelope", st, hipLaunchKernelGGL(ssdrc_envelope_kernel, tiles, dim3(256), 0, st, s, lengths, Lmax, (const double*)tab, e));
    NELE_PROF("ssdrc_gain", st, hipLaunchKernelGGL(ssdrc_gain_kernel, dim3(B), dim3(64), 0, st, s, (const double*)e, lengths, Lmax, ss_curve_of(p), y, ehat));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}

extern "C" long long nele_ssdrc_ws_bytes(int B, int Lmax) {
    if (B <= 0 || B > 65535 || Lmax <= 0 || Lmax > NELE_SSDRC_MAX_SAMPLES) {
        nele_set_error(NELE_ERR_INVALID_ARG, "nele_ssdrc_ws_bytes: B=%d outside 1 .. 65535 or Lmax=%d outside 1 .. %d", B, Lmax, NELE_SSDRC_MAX_SAMPLES);
        return -1;
    }
    return ss_layout(B, Lmax).total;
}

extern "C" int nele_ssdrc_params_default(nele_ssdrc_params* p) {
    NELE_CHECK_ARG(p, "nele_ssdrc_params_default: null params");
    *p = nele_ssdrc_params{};
    p->shape = 1;
    p->compress = 1;
    p->lifter_q = 20;
    p->n_knots = 4;
    p->beta = 0.25;
    p->preemph = 0.3;
    p->attack = 1e-4;
    p->release = 0.15;
    p->e0_ratio = 0.3;
    const double kx[4] = {-100.0, -60.0, -30.0, 0.0}, ky[4] = {-100.0, -45.0, -15.0, 0.0};
    for (int j = 0; j < 4; ++j) {
        p->knot_in_db[j] = kx[j];
        p->knot_out_db[j] = ky[j];
    }
    return NELE_OK;
}

extern "C" int nele_ssdrc_shape(const float* x, const int* lengths, int B, int Lmax, const nele_ssdrc_params* params, double* s, void* ws,
                                void* stream) {
    if (int st = ss_check("nele_ssdrc_shape", x, s, B, Lmax, params, ws)) return st;
    return ss_launch_shape("nele_ssdrc_shape", x, lengths, B, Lmax, params, s, (char*)ws, as_stream(stream));
}

extern "C" int nele_ssdrc_compress(const double* s, const int* lengths, int B, int Lmax, const nele_ssdrc_params* params, double* y, double* ehat,
                                   void* ws, void* stream) {
    if (int st = ss_check("nele_ssdrc_compress", s, y, B, Lmax, params, ws)) return st;
    return ss_launch_compress("nele_ssdrc_compress", s, lengths, B, Lmax, params, y, ehat, (char*)ws, true, as_stream(stream));
}

extern "C" int nele_ssdrc(const float* x, const int* lengths, int B, int Lmax, const nele_ssdrc_params* params, float* y, void* ws, void* stream) {
    if (int st = ss_check("nele_ssdrc", x, y, B, Lmax, params, ws)) return st;
    const hipStream_t st = as_stream(stream);
    char* w = (char*)ws;
    double* s1 = (double*)(w + ss_layout(B, Lmax).s1);
    if (int rc = ss_launch_shape("nele_ssdrc", x, lengths, B, Lmax, params, s1, w, st)) return rc;
    if (params->compress)
        if (int rc = ss_launch_compress("nele_ssdrc", s1, lengths, B, Lmax, params, s1, nullptr, w, !params->shape, st)) return rc;
    NELE_PROF("ssdrc_final", st, hipLaunchKernelGGL(ssdrc_final_kernel, dim3(B), dim3(1024), 0, st, x, (const double*)s1, lengths, Lmax, y));
    NELE_CHECK_LAUNCH("nele_ssdrc");
    return NELE_OK;
}
