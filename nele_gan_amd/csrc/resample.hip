// Rational-ratio polyphase FIR resampler: audio at any sample rate to the rate the rest of the library works at.  The reference loads at
// the file's own rate and asserts 16 kHz (dataloader.py:34-37 `librosa.load(..., sr=None); assert sr==16000`), so this is an addition to
// it, not a parity item.  The operation is the one DESIGN.md section 12 fixes (scipy.signal.resample_poly's convention):
//   half = zeros max(up, down);  h[0 .. 2 half] = up firwin(2 half + 1, 1 / max(up, down), window = ('kaiser', beta))      (host, float64)
//   hp[p][k] = h[p + k up], zero behind h's end;  K = ceil((2 half + 1) / up)                                              (host, float64)
//   y[n] = (float)(gain sum_{k < K} hp[p][k] x[q - k]),  c = n down + half,  p = c mod up,  q = c div up                  (resample_kernel)
// resample_kernel: one workgroup per (tile of RS_TILE consecutive outputs, row), a lane per output.  The tile's input span
// x[q_first - K + 1 .. q_last] goes to LDS as float64 (zeros outside the row); a lane then walks its own table row hp[p][.] - from LDS
// when the whole table fits RS_TAB_LDS_BYTES (small `up`: 48 -> 16 kHz has ONE row that every lane shares, an LDS broadcast), else
// from global memory (a 226 KB table at 44.1 -> 16 kHz: it lives in L2, a lane's row is contiguous) - and sums K fused multiply-adds in k
// order.  Every lane runs all K terms (out-of-row samples and padded taps are zeros in the operands, nothing is skipped), so a row's
// bits depend on its samples alone: not on R, Lmax_out, row_ids or where a tile starts.  n down is 64-bit (2^31 is passed after 4.9 M
// outputs at 160 / 441).  No atomics, no workspace.
#include "common.h"
#include "resample_poly.h"
#include <cmath>
#include <vector>
#include "../../include/nele_hip.h"

template <bool TAB_LDS>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const float* __restrict__ x, long long x_stride, const int* __restrict__ lengths_in,
                                                           const int* __restrict__ row_ids, int Lmax_out, int up, int down, int K, int half,
                                                           int span, const double* __restrict__ hp, double gain, float* __restrict__ y,
                                                           long long y_stride, int* __restrict__ lengths_out) {
    extern __shared__ double rs_lds[];                       // xs[span], then (TAB_LDS) the table [up][K]
    double* xs = rs_lds;
    double* tab = rs_lds + span;
    const int tid = threadIdx.x;
    const int row = row_ids ? row_ids[blockIdx.y] : (int)blockIdx.y;
    const long long cap = x_stride < (long long)NELE_RESAMPLE_MAX_SAMPLES ? x_stride : (long long)NELE_RESAMPLE_MAX_SAMPLES;
    const int len = (int)min(max((long long)lengths_in[row], 0LL), cap);
    const long long n_out = ((long long)len * up + down - 1) / down;
    const long long n0 = (long long)blockIdx.x * RS_TILE, n = n0 + tid;
    float* yr = y + (long long)row * y_stride;
    if (blockIdx.x == 0 && tid == 0) lengths_out[row] = (int)min(n_out, 2147483647LL);
    if (n0 >= n_out) {                                       // (workgroup-uniform) a tile behind the row's end: zeros
        if (n < Lmax_out) yr[n] = 0.f;
        return;
    }
    const float* xr = x + (long long)row * x_stride;
    const long long base = (n0 * down + half) / up - (K - 1);                // xs[i] = x[base + i]
    for (int i = tid; i < span; i += RS_TILE) {
        const long long g = base + i;
        xs[i] = (g >= 0 && g < len) ? (double)xr[g] : 0.0;
    }
    if (TAB_LDS)
        for (int i = tid; i < up * K; i += RS_TILE) tab[i] = hp[i];
    __syncthreads();
    if (n >= Lmax_out) return;
    double acc = 0.0;
    if (n < n_out) {
        const long long c = n * down + half;
        const int p = (int)(c % up);
        const double* __restrict__ hrow = (TAB_LDS ? (const double*)tab : hp) + (size_t)p * K;
        const double* __restrict__ xq = xs + (int)(c / up - base);            // x[q]; x[q - k] = xq[-k], 0 <= index < span
        acc = rs_dot(hrow, xq, K);
    }
    yr[n] = n < n_out ? (float)(gain * acc) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------- host
static int rs_check_design(const char* name, int up, int down, int zeros, int layout) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(zeros >= 1 && zeros <= RS_MAX_ZEROS, "%s: zeros=%d outside 1 .. %d", name, zeros, RS_MAX_ZEROS);
    NELE_CHECK_ARG(layout == 0 || layout == 1, "%s: layout=%d is neither 0 (natural order) nor 1 (polyphase table)", name, layout);
    return NELE_OK;
}

// modified Bessel function I0 by its power series sum_k ((x / 2)^k / k!)^2 (all terms positive: no cancellation; x <= 20 needs ~45 terms)
static double rs_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

extern "C" long long nele_resample_out_len(long long n_in, int up, int down) {
    if (rs_check_ratio("nele_resample_out_len", up, down)) return -1;
    if (n_in < 0 || n_in > (long long)NELE_RESAMPLE_MAX_SAMPLES) {
        nele_set_error(NELE_ERR_INVALID_ARG, "nele_resample_out_len: n_in=%lld outside 0 .. %d", n_in, NELE_RESAMPLE_MAX_SAMPLES);
        return -1;
    }
    return (n_in * up + down - 1) / down;
}

extern "C" long long nele_resample_taps_count(int up, int down, int zeros, int layout) {
    if (rs_check_design("nele_resample_taps_count", up, down, zeros, layout)) return -1;
    const int half = rs_half(up, down, zeros);
    return layout == 0 ? 2LL * half + 1 : (long long)up * rs_K(up, half);
}

extern "C" int nele_resample_tile(void) { return RS_TILE; }

extern "C" int nele_resample_taps(int up, int down, int zeros, double beta, int layout, double* out_host) {
    if (int st = rs_check_design("nele_resample_taps", up, down, zeros, layout)) return st;
    NELE_CHECK_ARG(beta >= 0.0 && beta <= 20.0, "nele_resample_taps: beta=%g outside 0 .. 20", beta);       // (false for NaN)
    NELE_CHECK_ARG(out_host, "nele_resample_taps: null output");
    const int M = up > down ? up : down, half = rs_half(up, down, zeros), nt = 2 * half + 1;
    std::vector<double> h((size_t)nt);
    if (M == 1) {                                            // cutoff at the Nyquist frequency: sinc at the integers - the unit impulse
        for (int k = 0; k < nt; ++k) h[k] = k == half ? 1.0 : 0.0;
    } else {
        const double fc = 1.0 / (double)M, i0b = rs_i0(beta);
        long double sum = 0.0L;
        for (int k = 0; k < nt; ++k) {
            const double m = (double)(k - half), t = m / (double)half, a = M_PI * fc * m;
            const double sinc = k == half ? 1.0 : sin(a) / a;
            h[k] = fc * sinc * (rs_i0(beta * sqrt(fmax(1.0 - t * t, 0.0))) / i0b);
            sum += (long double)h[k];
        }
        const double s = (double)sum;
        for (int k = 0; k < nt; ++k) h[k] = (double)up * (h[k] / s);
    }
    if (layout == 0) {
        for (int k = 0; k < nt; ++k) out_host[k] = h[k];
    } else {
        const int K = rs_K(up, half);
        for (int p = 0; p < up; ++p)
            for (int k = 0; k < K; ++k) {
                const long long j = (long long)p + (long long)k * up;
                out_host[(size_t)p * K + k] = j < nt ? h[(size_t)j] : 0.0;
            }
    }
    return NELE_OK;
}

extern "C" int nele_resample_var(const float* x, long long x_stride, const int* lengths_in, const int* row_ids, int R, int Lmax_out, int up, int down,
                                 int K, const double* hp_dev, double gain, float* y, long long y_stride, int* lengths_out, void* stream) {
    const char* name = "nele_resample_var";
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(x && lengths_in && hp_dev && y && lengths_out, "%s: null input, lengths_in, table, output or lengths_out", name);
    NELE_CHECK_ARG(R >= 1 && R <= 65535, "%s: R=%d outside 1 .. 65535", name, R);
    NELE_CHECK_ARG(Lmax_out >= 1 && Lmax_out <= NELE_RESAMPLE_MAX_SAMPLES, "%s: Lmax_out=%d outside 1 .. %d", name, Lmax_out, NELE_RESAMPLE_MAX_SAMPLES);
    NELE_CHECK_ARG(x_stride >= 1 && y_stride >= Lmax_out, "%s: x_stride=%lld below 1 or y_stride=%lld below Lmax_out=%d", name, x_stride, y_stride,
                   Lmax_out);
    NELE_CHECK_ARG(std::isfinite(gain), "%s: gain is not finite", name);
    const int zeros = rs_zeros_of(up, down, K);
    NELE_CHECK_ARG(zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RS_MAX_ZEROS);
    const int half = rs_half(up, down, zeros), span = rs_span(up, down, K);
    const bool tab_lds = (long long)up * K * (long long)sizeof(double) <= RS_TAB_LDS_BYTES;
    const size_t lds = ((size_t)span + (tab_lds ? (size_t)up * K : 0)) * sizeof(double);
    const dim3 grid((unsigned)((Lmax_out + RS_TILE - 1) / RS_TILE), (unsigned)R);
    const hipStream_t st = as_stream(stream);
    if (tab_lds)
        NELE_PROF("resample", st, hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_TILE), lds, st, x, x_stride, lengths_in, row_ids, Lmax_out, up,
                                                     down, K, half, span, hp_dev, gain, y, y_stride, lengths_out));
    else
        NELE_PROF("resample", st, hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_TILE), lds, st, x, x_stride, lengths_in, row_ids, Lmax_out, up,
                                                     down, K, half, span, hp_dev, gain, y, y_stride, lengths_out));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
