// The up-converter of the real-time path that carries the band above 8 kHz past the enhancer (nele_hbup_*; DESIGN.md section 24;
// tests/highband_ref.py restates it in numpy).  Per stream, with zeros before its start, lam samples at 16 kHz and L at the device rate:
//   d[n] = fmaf(-g, low[n - lam], enh[n])          float32: what the enhancer added to g times the band it worked on
//   u[m] = the stream up-converter's output for d  (section 15: float64 sum, k ascending, rs_dot of csrc/resample_poly.h)
//   y[m] = fmaf(g, x[m - L], (float)u[m])          float32
// The up-converter is linear, so this is up(enh) + g (x delayed by L - up(low delayed by lam)): the plain wrapper's output plus what the
// 16 kHz path cannot carry.
//   hbup_hop_kernel  : rss_hop_kernel's scheme (csrc/resample_stream.hip) - one workgroup per stream and call, looping over the call's
//                      tiles of 256 outputs, the table and the tile's span of d in LDS as float64, rs_dot unchanged.  Its own text is
//                      the staging, which computes d on the fly, and the epilogue, which adds the delayed input.
// The record of a slot is float32 [K - 1 | lam | L]: the last K - 1 of d, the last lam of low, the last L of x.  It is rewritten behind
// the last tile, gathered through LDS in chunks of the staging space: the new value of an entry comes from the call's rows or from an
// entry at or behind it in the record, so chunks in ascending order never read what an earlier chunk wrote.  No index grows with the
// stream's age.  State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses
// workgroups.
#include "common.h"
#include "resample_poly.h"
#include "slot_state.h"
#include "../../include/nele_hip.h"
#include "../../include/nele_hip_ext7.h"

namespace {

constexpr long long HB_HDR_BYTES = SLOT_GEOM_HDR_BYTES;     // int [0] = max_streams, [1] = K, [2] = up, [3] = down, [4] = lam, [5] = L
constexpr int HB_STAGE_MAX = 2048;                          // doubles of staging space the record's move may ask for beyond the span
__host__ __device__ constexpr long long hb_rec_bytes(int K, int lam, int L) { return slot_al(4LL * ((K - 1) + lam + L)); }

struct HbArgs {
    unsigned char* state;
    int S, up, down, K, lam, L;
    int r0;                      // half - D down: c_rel of the call's first output
    int span;                    // doubles of d a tile reads
    int stage;                   // doubles of staging space, >= span
    int n16, n_out;              // samples per row in this call, at 16 kHz and at the device rate
    const double* hp;            // [up][K]
    const float* enh;            // [S] rows of enh_stride
    long long enh_stride;
    const float* low;            // [S] rows of low_stride
    long long low_stride;
    const float* x;              // [S] rows of x_stride
    long long x_stride;
    const float* gain;           // [S] or null (1)
    const unsigned char* active; // [S] or null (all)
    float* y;                    // [S] rows of y_stride
    long long y_stride;
};

__global__ __launch_bounds__(RS_TILE) void hbup_hop_kernel(HbArgs a) {
    extern __shared__ double hb_lds[];                     // ds[stage], then the table [up][K]
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    if (!slot_hdr_matches(a.state, a.S, a.K, a.up, a.down, a.lam, a.L)) return;   // not the state _init laid out: touch nothing
    const int K = a.K, H = K - 1, up = a.up, down = a.down, lam = a.lam, L = a.L;
    float* rec = reinterpret_cast<float*>(a.state + HB_HDR_BYTES + (size_t)b * hb_rec_bytes(K, lam, L));
    float* dh = rec;                                       // d[-H .. -1] of the call's row
    float* lowh = rec + H;                                 // low[-lam .. -1]
    float* xh = rec + H + lam;                             // x[-L .. -1]
    const float* er = a.enh + (size_t)b * a.enh_stride;
    const float* lr = a.low + (size_t)b * a.low_stride;
    const float* xr = a.x + (size_t)b * a.x_stride;
    float* yr = a.y + (size_t)b * a.y_stride;
    const float g = a.gain ? a.gain[b] : 1.0f;
    auto d_at = [&](int n) -> float {                      // 0 <= n < n16
        const float lo = n < lam ? lowh[n] : lr[n - lam];
        return fmaf(-g, lo, er[n]);
    };
    double* ds = hb_lds;
    double* tab = hb_lds + a.stage;
    for (int i = t; i < up * K; i += RS_TILE) tab[i] = a.hp[i];
    const int tiles = (a.n_out + RS_TILE - 1) / RS_TILE;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = tile * RS_TILE;
        const int base = (int)((a.r0 + (long long)j0 * down) / up) - H;          // ds[i] = d[base + i], base >= -H
        for (int i = t; i < a.span; i += RS_TILE) {
            const int n = base + i;
            ds[i] = n < 0 ? (double)dh[H + n] : (n < a.n16 ? (double)d_at(n) : 0.0);
        }
        __syncthreads();
        const int j = j0 + t;
        if (j < a.n_out) {
            const long long c = a.r0 + (long long)j * down;
            const int p = (int)(c % up);
            const double* __restrict__ hrow = tab + (size_t)p * K;
            const double* __restrict__ dq = ds + ((int)(c / up) - base);       // d[q]; d[q - k] = dq[-k], 0 <= index < span
            const float xdel = j < L ? xh[j] : xr[j - L];
            yr[j] = fmaf(g, xdel, (float)rs_dot(hrow, dq, K));
        }
        __syncthreads();                                   // ds is the next tile's (and the record's) staging space
    }
    float* ms = reinterpret_cast<float*>(ds);
    const int R = H + lam + L, cap = 2 * a.stage;
    for (int c0 = 0; c0 < R; c0 += cap) {
        const int c1 = c0 + cap < R ? c0 + cap : R;
        for (int i = c0 + t; i < c1; i += RS_TILE) {       // the last H, lam, L samples of history + row; every read at or behind entry i
            float v;
            if (i < H) {
                const int n = a.n16 - H + i;
                v = n < 0 ? dh[H + n] : d_at(n);
            } else if (i < H + lam) {
                const int n = a.n16 - lam + (i - H);
                v = n < 0 ? lowh[lam + n] : lr[n];
            } else {
                const int m = a.n_out - L + (i - H - lam);
                v = m < 0 ? xh[L + m] : xr[m];
            }
            ms[i - c0] = v;
        }
        __syncthreads();
        for (int i = c0 + t; i < c1; i += RS_TILE) rec[i] = ms[i - c0];
        __syncthreads();
    }
}

inline bool hb_K_ok(int K) { return K >= 1 && K <= RS_TAB_LDS_BYTES / 8; }
inline bool hb_lags_ok(int lag16, int lag_dev) { return lag16 >= 0 && lag16 <= NELE_HBUP_MAX_LAG16 && lag_dev >= 0 && lag_dev <= NELE_HBUP_MAX_LAG; }

int hb_check(const char* name, const void* state, long long state_bytes, int S, int up, int down, int K, int lag16, int lag_dev, int* zeros) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    auto params = [&]() -> int {
        *zeros = hb_K_ok(K) ? rs_zeros_of(up, down, K) : 0;
        NELE_CHECK_ARG(*zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RS_MAX_ZEROS);
        NELE_CHECK_ARG((long long)up * K * 8 <= RS_TAB_LDS_BYTES, "%s: the table of up=%d, K=%d is %lld bytes, above the %d a stream converter takes",
                       name, up, K, (long long)up * K * 8, RS_TAB_LDS_BYTES);
        NELE_CHECK_ARG((RS_TILE * (long long)up) % down == 0,
                       "%s: a hop of 256 samples at 16 kHz is %.4f samples at the other rate (256 up %% down != 0 for up=%d, down=%d): the "
                       "carried band needs a whole number",
                       name, (double)RS_TILE * up / down, up, down);
        NELE_CHECK_ARG(lag16 >= 0 && lag16 <= NELE_HBUP_MAX_LAG16, "%s: lag16=%d outside 0 .. %d", name, lag16, NELE_HBUP_MAX_LAG16);
        NELE_CHECK_ARG(lag_dev >= 0 && lag_dev <= NELE_HBUP_MAX_LAG, "%s: lag_dev=%d outside 0 .. %d", name, lag_dev, NELE_HBUP_MAX_LAG);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_hbup_state_bytes(S, K, lag16, lag_dev), "nele_hbup_state_bytes", K);
}

// slots == null: every record; write_hdr: the header too
int hb_reset(const char* name, void* state, int S, int up, int down, int K, int lag16, int lag_dev, const unsigned char* slots, bool write_hdr,
             void* stream) {
    const int hdr[6] = {S, K, up, down, lag16, lag_dev};
    return slot_state_reset(name, state, HB_HDR_BYTES, hb_rec_bytes(K, lag16, lag_dev), S, slots, write_hdr ? 6 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_hbup_record_bytes(int K, int lag16, int lag_dev) {
    if (!hb_K_ok(K) || !hb_lags_ok(lag16, lag_dev) || (K - 1) + lag16 + lag_dev == 0) return -1;
    return hb_rec_bytes(K, lag16, lag_dev);
}

extern "C" long long nele_hbup_state_bytes(int max_streams, int K, int lag16, int lag_dev) {
    const long long rec = nele_hbup_record_bytes(K, lag16, lag_dev);
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || rec < 0) return -1;
    return HB_HDR_BYTES + (long long)max_streams * rec;
}

extern "C" int nele_hbup_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev, void* stream) {
    int zeros = 0;
    if (int st = hb_check("nele_hbup_init", state, state_bytes, max_streams, up, down, K, lag16, lag_dev, &zeros)) return st;
    return hb_reset("nele_hbup_init", state, max_streams, up, down, K, lag16, lag_dev, nullptr, true, stream);
}

extern "C" int nele_hbup_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev,
                               const unsigned char* slots, void* stream) {
    int zeros = 0;
    if (int st = hb_check("nele_hbup_reset", state, state_bytes, max_streams, up, down, K, lag16, lag_dev, &zeros)) return st;
    return hb_reset("nele_hbup_reset", state, max_streams, up, down, K, lag16, lag_dev, slots, false, stream);
}

extern "C" int nele_hbup_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int lag16, int lag_dev,
                             const double* hp_dev, const float* enh, long long enh_stride, const float* low, long long low_stride, const float* x,
                             long long x_stride, const float* gain, const unsigned char* active, int nh, float* y, long long y_stride, void* stream) {
    const char* name = "nele_hbup_hop";
    int zeros = 0;
    if (int st = hb_check(name, state, state_bytes, max_streams, up, down, K, lag16, lag_dev, &zeros)) return st;
    NELE_CHECK_ARG(hp_dev && enh && low && x && y, "%s: null table, enh, low, x or y", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    const long long n16 = (long long)nh * RS_TILE, n_out = n16 * up / down;
    NELE_CHECK_ARG(n16 <= NELE_RESAMPLE_MAX_SAMPLES && n_out <= NELE_RESAMPLE_MAX_SAMPLES, "%s: nh=%d hops of 256 -> %lld samples are more than 2^30 per call",
                   name, nh, (long long)RS_TILE * up / down);
    NELE_CHECK_ARG(enh_stride >= n16 && low_stride >= n16, "%s: enh_stride=%lld or low_stride=%lld below nh 256=%lld", name, enh_stride, low_stride, n16);
    NELE_CHECK_ARG(x_stride >= n_out && y_stride >= n_out, "%s: x_stride=%lld or y_stride=%lld below nh 256 up / down=%lld", name, x_stride, y_stride,
                   n_out);
    const int half = rs_half(up, down, zeros), D = half / down;
    HbArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.up = up;
    a.down = down;
    a.K = K;
    a.lam = lag16;
    a.L = lag_dev;
    a.r0 = half - D * down;
    a.span = rs_span(up, down, K);
    const int whole = ((K - 1) + lag16 + lag_dev + 1) / 2, want = whole < HB_STAGE_MAX ? whole : HB_STAGE_MAX;   // the record in one chunk, up to 16 KiB
    a.stage = a.span > want ? a.span : want;
    a.n16 = (int)n16;
    a.n_out = (int)n_out;
    a.hp = hp_dev;
    a.enh = enh;
    a.enh_stride = enh_stride;
    a.low = low;
    a.low_stride = low_stride;
    a.x = x;
    a.x_stride = x_stride;
    a.gain = gain;
    a.active = active;
    a.y = y;
    a.y_stride = y_stride;
    const size_t lds = ((size_t)a.stage + (size_t)up * K) * sizeof(double);     // <= 49040 + 16384 bytes: inside the 64 KiB of a plain launch
    NELE_PROF("highband", as_stream(stream), hipLaunchKernelGGL(hbup_hop_kernel, dim3(max_streams), dim3(RS_TILE), lds, as_stream(stream), a));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
