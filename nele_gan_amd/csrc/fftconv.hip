// Room impulse responses for a batch, one per row (reference eval_metrics.py:124-167): scipy.signal.lfilter(h, [1], x) as a uniformly
// partitioned overlap-save convolution - 256-sample blocks, 512-point float64 transforms (fft512_wave, two real blocks per complex
// transform as in the STFT kernel) - and the per-row level normalisation / clip() that follows it.
//   nele_rir_bank_prepare : R impulse responses -> their partition spectra H_p (p < ceil(taps / 256)), once
//   nele_fir_fft_var      : y[b] = lfilter(h[rir_index[b]], [1], x[b][:lengths[b]]), exact zeros behind lengths[b]
//   nele_norm_clip_var    : nele_norm_clip with a length, a summand shift and an output shift per row
// A spectrum is 256 double2: slot k = bin k for k = 1..255, slot 0 = (bin 0, bin 256) - both are real.  Products are therefore taken
// slot by slot, component-wise in slot 0.
// Spectra of the input blocks live in the caller's workspace (HBM) between the two kernels: a row's partition sum needs the last
// P = 63 block spectra (1 s of RIR) = 258 KB, more than a CU's 160 KB of LDS, and 256 rows of 250 blocks are 262 MB (DESIGN.md
// "Rooms").  The multiply-accumulate kernel reads each of them once per 8 output blocks.
#include "common.h"
#include "fft512.h"
#include "ws_arena.h"

#define FC_BLK 256                     // samples per block = slots per spectrum
#define FC_TILE 8                      // output blocks per workgroup of the multiply-accumulate kernel (4 waves x 2 blocks per inverse)
#define FC_SPEC_BYTES ((long long)FC_BLK * (long long)sizeof(double2))
#define FC_HDR_BYTES 256                // bank: int R, int Pmax | at 256: double2 H[R][Pmax][256] | behind them: int npart[R]

__host__ __device__ static inline const int* fc_bank_npart(const void* bank, int R, int Pmax) {
    return (const int*)((const char*)bank + FC_HDR_BYTES + (size_t)R * Pmax * FC_BLK * sizeof(double2));
}

// One wave: the packed spectra of two real 512-sample segments a, b (seg(0, n), seg(1, n)) from ONE complex transform of a + i b
// (fft512_packed_split).  Xb may be NULL.
template <class Seg>
__device__ __forceinline__ void fc_forward_pair(Seg seg, double2* __restrict__ xw, const double2* __restrict__ tw, int lane,
                                                double2* __restrict__ Xa, double2* __restrict__ Xb) {
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = fftw_n(lane, r);
        v[r] = make_double2(seg(0, n), seg(1, n));
    }
    fft512_wave<false>(v, xw, tw, lane);
    fft512_wave_store(v, xw, lane);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int k = 64 * m + lane;
        double2 xa, xb;
        fft512_packed_split(xw, k, xa, xb);
        Xa[k] = xa;
        if (Xb) Xb[k] = xb;
    }
}

// grid (ceil(Pmax / 8), R), block 256: wave w of workgroup g transforms partitions 8 g + 2 w and + 1 of RIR r (taps [256 p, 256 p + 256)
// in the first half of the segment, zeros in the second; partitions behind taps[r] come out as zeros).
__global__ __launch_bounds__(256) void fc_bank_kernel(const double* __restrict__ rirs, const int* __restrict__ taps, int R, int Lhmax,
                                                      int Pmax, int* __restrict__ hdr, double2* __restrict__ H) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[4][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();
    const int r = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nt = min(max(taps[r], 1), Lhmax);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (r == 0) { hdr[0] = R; hdr[1] = Pmax; }
        const_cast<int*>(fc_bank_npart(hdr, R, Pmax))[r] = (nt + FC_BLK - 1) / FC_BLK;
    }
    const int p = blockIdx.x * 8 + 2 * w;
    if (p >= Pmax) return;
    const double* h = rirs + (size_t)r * Lhmax;
    auto seg = [&](int which, int n) -> double {
        const int i = (p + which) * FC_BLK + n;
        return (n < FC_BLK && i < nt) ? h[i] : 0.0;
    };
    double2* Hr = H + ((size_t)r * Pmax + p) * FC_BLK;
    fc_forward_pair(seg, xws[w], tw, lane, Hr, (p + 1 < Pmax) ? Hr + FC_BLK : nullptr);
}

__device__ __forceinline__ int fc_row_length(const int* lengths, int b, int Lmax) {
    return lengths ? min(max(lengths[b], 0), Lmax) : Lmax;
}

// X[b][j] = spectrum of the samples [256 (j - 1), 256 (j + 1)) of row b (zero outside [0, lengths[b])), j < ceil(lengths[b] / 256).
// grid (ceil(ceil(T / 2) / 4), B), block 256: one wave per pair of blocks.
__global__ __launch_bounds__(256) void fc_forward_kernel(const float* __restrict__ x, int Lmax, const int* __restrict__ lengths, int T,
                                                         double2* __restrict__ X) {
    __shared__ double2 tw[256];
    __shared__ double2 xws[4][FFTW_SLOTS];
    fft512_fill_twiddles(tw);
    __syncthreads();
    const int b = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int len = fc_row_length(lengths, b, Lmax);
    const int Tb = (len + FC_BLK - 1) / FC_BLK;
    const int j = (blockIdx.x * 4 + w) * 2;
    if (j >= Tb) return;
    const float* xb = x + (size_t)b * Lmax;
    auto seg = [&](int which, int n) -> double {
        const int i = (j + which - 1) * FC_BLK + n;
        return (i >= 0 && i < len) ? (double)xb[i] : 0.0;
    };
    double2* Xr = X + ((size_t)b * T + j) * FC_BLK;
    fc_forward_pair(seg, xws[w], tw, lane, Xr, (j + 1 < Tb) ? Xr + FC_BLK : nullptr);
}

// acc += x h, slot by slot: complex, except slot 0 which holds two real bins
__device__ __forceinline__ void fc_mac(double2& acc, const double2 x, const double2 h, bool slot0) {
    const double re = fma(x.x, h.x, acc.x);
    const double im = fma(x.y, h.x, fma(x.x, h.y, acc.y));
    acc.x = slot0 ? re : fma(-x.y, h.y, re);
    acc.y = slot0 ? fma(x.y, h.y, acc.y) : im;
}

// Y_j = sum_{p = 0}^{min(P, j + 1) - 1} X_{j - p} H_p in ascending p for the 8 output blocks j0 .. j0 + 7 of row b, thread t owning slot t:
// per p one H_p and ONE new X (the 8 spectra an iteration needs are 8 consecutive blocks; the one that leaves and the one that enters
// share a ring position).  Then 4 inverse transforms, wave w taking Y_{j0 + 2 w} + i Y_{j0 + 2 w + 1}, of which the last 256 samples are
// the output.  Nothing here depends on another row, on B or on the bank's other entries: a row's bits are its own.
// grid (ceil(T / 8), B), block 256.
__global__ __launch_bounds__(256) void fc_mac_inverse_kernel(const double2* __restrict__ X, int T, int Lmax, const int* __restrict__ lengths,
                                                             const int* __restrict__ hdr, const double2* __restrict__ H,
                                                             const int* __restrict__ rir_index, double* __restrict__ y) {
    __shared__ double2 tw[256];
    __shared__ double2 ys[4][FFTW_SLOTS];                    // wave w: Y_{2w} at [0, 256), Y_{2w+1} at [256, 512); then its exchange buffer
    const int b = blockIdx.y, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int j0 = blockIdx.x * FC_TILE;
    const int len = fc_row_length(lengths, b, Lmax);
    const int Tb = (len + FC_BLK - 1) / FC_BLK;
    const int R = hdr[0], Pmax = hdr[1];
    const int ri = rir_index ? rir_index[b] : 0;
    double* yb = y + (size_t)b * Lmax;
    if (j0 >= Tb || ri < 0 || ri >= R) {                    // behind the row's end (or no such RIR): exact zeros
        for (int i = j0 * FC_BLK + t; i < min(Lmax, (j0 + FC_TILE) * FC_BLK); i += 256) yb[i] = 0.0;
        return;
    }
    fft512_fill_twiddles(tw);
    const int P = min(fc_bank_npart(hdr, R, Pmax)[ri], Pmax);
    const int pend = min(P, j0 + FC_TILE);                   // X_i = 0 for i < 0
    const double2* Xb = X + (size_t)b * T * FC_BLK + t;
    const double2* Hb = H + (size_t)ri * Pmax * FC_BLK + t;
    const double2 zero = make_double2(0.0, 0.0);
    auto ldx = [&](int i) -> double2 { return (i >= 0 && i < Tb) ? Xb[(size_t)i * FC_BLK] : zero; };
    double2 acc[FC_TILE], ring[FC_TILE];                     // ring[i & 7] = X_i
#pragma unroll
    for (int jj = 0; jj < FC_TILE; ++jj) {
        acc[jj] = zero;
        ring[jj] = ldx(j0 + jj);
    }
    const bool slot0 = (t == 0);
    for (int p0 = 0; p0 < pend; p0 += FC_TILE) {
#pragma unroll
        for (int pp = 0; pp < FC_TILE; ++pp) {
            const int p = p0 + pp;
            if (p < pend) {
                const double2 h = Hb[(size_t)p * FC_BLK];
                const double2 nx = ldx(j0 - p - 1);
#pragma unroll
                for (int jj = 0; jj < FC_TILE; ++jj) fc_mac(acc[jj], ring[(jj - pp) & 7], h, slot0);
                ring[(7 - pp) & 7] = nx;
            }
        }
    }
#pragma unroll
    for (int jj = 0; jj < FC_TILE; ++jj) ys[jj >> 1][(jj & 1) * FC_BLK + t] = acc[jj];
    __syncthreads();
    // W = Ya + i Yb on all 512 bins (Y[512 - k] = conj Y[k]), in the transform's input order
    double2* xw = ys[w];
    const double2 a0 = xw[0], b0 = xw[FC_BLK];
    double2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = fftw_n(lane, r);
        const int k = (n <= 256) ? n : 512 - n;
        v[r] = fft512_packed_join(xw[k & 255], xw[FC_BLK + (k & 255)], a0, b0, n);
    }
    fftw_wave_sync();                                        // the wave's reads of Y precede the transform's writes to the same LDS
    fft512_wave<true>(v, xw, tw, lane);
    const int ja = j0 + 2 * w;
#pragma unroll
    for (int m = 4; m < 8; ++m) {                            // v[m] = 512 (ya + i yb)[64 m + lane]: keep samples 256 .. 511
        const int ia = ja * FC_BLK + 64 * (m - 4) + lane, ib = ia + FC_BLK;
        if (ia < Lmax) yb[ia] = (ia < len) ? v[m].x * (1.0 / 512.0) : 0.0;
        if (ib < Lmax) yb[ib] = (ib < len) ? v[m].y * (1.0 / 512.0) : 0.0;
    }
}

// nele_norm_clip (reverb.hip) per row: n = lengths[b] samples, v[i] = a[b][i] (+ add[b][i + add_shift[b]]), i < n; rms and clip() over
// those n; out[b][i] = v'[i + out_shift[b]] for i + out_shift[b] < n, exact zeros behind, up to N.
__global__ __launch_bounds__(1024) void norm_clip_var_kernel(const double* __restrict__ a64, const float* __restrict__ a32,
                                                             const float* __restrict__ add, int N, const int* __restrict__ lengths,
                                                             const int* __restrict__ add_shift, const int* __restrict__ out_shift,
                                                             double target, float* __restrict__ out, double* __restrict__ out64,
                                                             int* __restrict__ nclip) {
    __shared__ double red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = fc_row_length(lengths, b, N);
    const int sa = add_shift ? max(add_shift[b], 0) : 0, so = out_shift ? max(out_shift[b], 0) : 0;
    auto val = [&](int i) {
        double v = a64 ? a64[(size_t)b * N + i] : (double)a32[(size_t)b * N + i];
        if (add && i + sa < N) v += (double)add[(size_t)b * N + i + sa];
        return v;
    };
    double scale_num = 1.0, scale_den = 1.0;
    if (target > 0.0 && n > 0) {
        double s = 0.0;
        for (int i = tid; i < n; i += 1024) { const double v = val(i); s += v * v; }
        s = block_sum(s, red);
        scale_den = sqrt(s / (double)n);
        scale_num = target;
    }
    double mx = -1e300, mn = 1e300;
    for (int i = tid; i < n; i += 1024) {
        double v = val(i);
        if (target > 0.0) v = v / scale_den * scale_num;
        mx = fmax(mx, v); mn = fmin(mn, v);
    }
    mx = block_max(mx, red);
    mn = -block_max(-mn, red);
    int steps = 0;
    if (n > 0) {
        double small = 0.05, hi = mx, lo = mn;
        while ((hi >= 1.0 || lo < -1.0) && steps < 4096) { hi = hi / (1.0 + small); lo = lo / (1.0 + small); small = small + 0.05; ++steps; }
    }
    for (int i = tid; i < N; i += 1024) {
        double v = 0.0;
        if (i + so < n) {
            v = val(i + so);
            if (target > 0.0) v = v / scale_den * scale_num;
            double small = 0.05;
            for (int s_ = 0; s_ < steps; ++s_) { v = v / (1.0 + small); small = small + 0.05; }
        }
        if (out) out[(size_t)b * N + i] = (float)v;
        if (out64) out64[(size_t)b * N + i] = v;
    }
    if (nclip && tid == 0) nclip[b] = steps;
}

static inline int fc_blocks(int L) { return (L + FC_BLK - 1) / FC_BLK; }

extern "C" long long nele_rir_bank_bytes(int R, int Lhmax) {
    if (R <= 0 || Lhmax <= 0) {
        nele_set_error(NELE_ERR_INVALID_ARG, "nele_rir_bank_bytes: R=%d and Lhmax=%d must be positive", R, Lhmax);
        return -1;
    }
    return FC_HDR_BYTES + (long long)R * fc_blocks(Lhmax) * FC_SPEC_BYTES + (long long)ws_round256((size_t)R * sizeof(int));
}

extern "C" int nele_rir_bank_prepare(const double* rirs, const int* taps, int R, int Lhmax, void* bank, void* stream) {
    NELE_CHECK_ARG(rirs && taps && bank, "nele_rir_bank_prepare: null rirs, taps or bank");
    NELE_CHECK_ARG(R > 0 && R <= 65535 && Lhmax > 0, "nele_rir_bank_prepare: R=%d must be in 1..65535 and Lhmax=%d positive", R, Lhmax);
    NELE_CHECK_ARG(((uintptr_t)bank & 255) == 0, "nele_rir_bank_prepare: bank must be 256-byte aligned");
    const int Pmax = fc_blocks(Lhmax);
    int* hdr = (int*)bank;
    double2* H = (double2*)((char*)bank + FC_HDR_BYTES);
    hipLaunchKernelGGL(fc_bank_kernel, dim3((Pmax + 7) / 8, R), dim3(256), 0, as_stream(stream), rirs, taps, R, Lhmax, Pmax, hdr, H);
    NELE_CHECK_LAUNCH("nele_rir_bank_prepare");
    return NELE_OK;
}

extern "C" long long nele_fir_fft_workspace_bytes(int B, int Lmax) {
    if (B <= 0 || Lmax <= 0) {
        nele_set_error(NELE_ERR_INVALID_ARG, "nele_fir_fft_workspace_bytes: B=%d and Lmax=%d must be positive", B, Lmax);
        return -1;
    }
    return (long long)B * fc_blocks(Lmax) * FC_SPEC_BYTES;
}

extern "C" int nele_fir_fft_var(const float* x, int B, int Lmax, const int* lengths, const void* bank, const int* rir_index, double* y,
                                void* workspace, void* stream) {
    NELE_CHECK_ARG(x && bank && y && workspace, "nele_fir_fft_var: null x, bank, y or workspace");
    NELE_CHECK_ARG(B > 0 && B <= 65535 && Lmax > 0, "nele_fir_fft_var: B=%d must be in 1..65535 and Lmax=%d positive", B, Lmax);
    NELE_CHECK_ARG(((uintptr_t)bank & 255) == 0 && ((uintptr_t)workspace & 15) == 0,
                   "nele_fir_fft_var: bank must be 256-byte and workspace 16-byte aligned");
    const int T = fc_blocks(Lmax);
    const int* hdr = (const int*)bank;
    double2* X = (double2*)workspace;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(fc_forward_kernel, dim3(((T + 1) / 2 + 3) / 4, B), dim3(256), 0, s, x, Lmax, lengths, T, X);
    NELE_CHECK_LAUNCH("nele_fir_fft_var");
    hipLaunchKernelGGL(fc_mac_inverse_kernel, dim3((T + FC_TILE - 1) / FC_TILE, B), dim3(256), 0, s, (const double2*)X, T, Lmax, lengths, hdr,
                       (const double2*)((const char*)bank + FC_HDR_BYTES), rir_index, y);
    NELE_CHECK_LAUNCH("nele_fir_fft_var");
    return NELE_OK;
}

extern "C" int nele_norm_clip_var(const double* a64, const float* a32, const float* add, int B, int N, const int* lengths,
                                  const int* add_shift, const int* out_shift, double target_rms, float* out, double* out64, int* nclip,
                                  void* stream) {
    NELE_CHECK_ARG((a64 != nullptr) != (a32 != nullptr), "nele_norm_clip_var: exactly one of a64 / a32 must be given");
    NELE_CHECK_ARG((out || out64) && B > 0 && N > 0, "nele_norm_clip_var: bad arguments");
    hipLaunchKernelGGL(norm_clip_var_kernel, dim3(B), dim3(1024), 0, as_stream(stream), a64, a32, add, N, lengths, add_shift, out_shift,
                       target_rms, out, out64, nclip);
    NELE_CHECK_LAUNCH("nele_norm_clip_var");
    return NELE_OK;
}
