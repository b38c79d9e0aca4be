// The up-converter on a hop schedule that carries the band above 8 kHz past the enhancer (nele_hbsched_*; DESIGN.md section 25;
// tests/highband_sched_ref.py restates it in numpy): csrc/highband.hip's operation for the device rates at which a 256-sample hop at
// 16 kHz is NOT a whole number of device samples - 44.1 kHz and its family - and, as the case P = 1, for the others.  Per stream, with
// zeros before its start, lam = 256 lag_hops samples at 16 kHz and Lx at the device rate:
//   d[n] = fmaf(-g, low[n - lam], enh[n])          float32: what the enhancer added to g times the band it worked on
//   u[m] = section 20's scheduled up-conversion of d from the lead L0 - s  (float64 sum, k ascending, rs_dot of csrc/resample_poly.h)
//   y[m] = fmaf(g, x[m - Lx], (float)u[m])         float32
// The path's delay (D_down + lam) up / down + D_up is not a whole number of device samples on a schedule; s = (-(D_down + lam) up) mod
// down ticks of 1 / down more make it one, Lx, and they cost nothing: the scheduled converter keeps its sub-sample timing as an
// integer, the slot's lead, and a slot that starts at L0 - s instead of L0 takes every polyphase sum s / down of a device sample later.
//   hbsched_hop_kernel : sched_hop_kernel's scheme (csrc/resample_sched.hip) - one workgroup per slot and call, looping over the call's
//                        tiles of 256 outputs, the tile's span of d in LDS as float64, the table from global memory (L2) or, where it
//                        is at most RS_TAB_LDS_BYTES, from LDS, rs_dot unchanged, the guard on the lead - with hbup_hop_kernel's
//                        staging, which computes d on the fly, its epilogue, which adds the delayed input, and its record move.
// The record of a slot is a 16-byte head (int lead, three reserved ints), then float32 [H | lam | Lx]: the last H = K - 1 + E of d, the
// last lam of low, the last Lx of x.  It is rewritten behind the last tile, gathered through LDS in chunks of the staging space: the new
// value of an entry comes from the call's rows or from an entry at or behind it in the record, so chunks in ascending order never read
// what an earlier chunk wrote.  No index grows with the stream's age.  State is read and written with plain loads and stores by the
// slot's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "resample_poly.h"
#include "slot_state.h"
#include "../../include/nele_hip.h"
#include "../../include/nele_hip_ext3.h"
#include "../../include/nele_hip_ext7.h"
#include "../../include/nele_hip_ext8.h"

namespace {

constexpr long long HBS_HDR_BYTES = SLOT_GEOM_HDR_BYTES;    // int [0] = max_streams, [1] = K, [2] = up, [3] = down, [4] = H, [5] = L0 - s, [6] = lam, [7] = Lx
constexpr int HBS_HEAD_BYTES = 16;                          // a record: int lead, three reserved ints, then float [H + lam + Lx]
constexpr int HBS_MAX_H = 4096;                             // nele_sched_stream_record_bytes' limit
constexpr int HBS_STAGE_MAX = 2048;                         // doubles of staging space the record's move may ask for beyond the span
__host__ __device__ constexpr long long hbs_rec_bytes(int H, int lam, int Lx) { return slot_al(HBS_HEAD_BYTES + 4LL * (H + lam + Lx)); }

struct HbsPlan {
    int K, D_up, s, L0, E, H, lam, Lx, rnum, P, hop_min, hop_max;      // L0: the shifted lead L0 - s
};

struct HbsArgs {
    unsigned char* state;
    int S, up, down, K, H, E, L0, lam, Lx;
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

template <bool TAB_LDS>
__global__ __launch_bounds__(RS_TILE) void hbsched_hop_kernel(HbsArgs a) {
    extern __shared__ double hbs_lds[];                    // ds[stage], then (TAB_LDS) the table [up][K]
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) return;                  // neither read nor written
    const int* hdr = reinterpret_cast<const int*>(a.state);
    if (!slot_hdr_matches(a.state, a.S, a.K, a.up, a.down) || hdr[4] != a.H || hdr[5] != a.L0 || hdr[6] != a.lam || hdr[7] != a.Lx)
        return;                                            // not the state _init laid out: touch nothing
    const int K = a.K, H = a.H, up = a.up, down = a.down, lam = a.lam, Lx = a.Lx;
    int* head = reinterpret_cast<int*>(a.state + HBS_HDR_BYTES + (size_t)b * hbs_rec_bytes(H, lam, Lx));
    float* rec = reinterpret_cast<float*>(head + HBS_HEAD_BYTES / 4);
    float* dh = rec;                                       // buf[0 .. H) of buf = d's history ++ d of the call's row
    float* lowh = rec + H;                                 // low[-lam .. -1]
    float* xh = rec + H + lam;                             // x[-Lx .. -1]
    float* yr = a.y + (size_t)b * a.y_stride;
    const int L = head[0];
    // section 20's guard: inside these bounds every read of d lies in 0 .. H + n16 - 1 of buf; outside them the slot's lead is not this
    // call's: NaN, and the record stays
    if (L < -a.E * up || (long long)L + (long long)(a.n_out - 1) * down >= (long long)a.n16 * up) {
        for (int j = t; j < a.n_out; j += RS_TILE) yr[j] = __int_as_float(0x7fc00000);
        return;
    }
    const float* er = a.enh + (size_t)b * a.enh_stride;
    const float* lr = a.low + (size_t)b * a.low_stride;
    const float* xr = a.x + (size_t)b * a.x_stride;
    const float g = a.gain ? a.gain[b] : 1.0f;
    auto d_at = [&](int n) -> float {                      // 0 <= n < n16
        const float lo = n < lam ? lowh[n] : lr[n - lam];
        return fmaf(-g, lo, er[n]);
    };
    double* ds = hbs_lds;
    const double* tab = a.hp;
    if (TAB_LDS) {
        double* tl = hbs_lds + a.stage;
        for (int i = t; i < up * K; i += RS_TILE) tl[i] = a.hp[i];
        tab = tl;
    }
    const long long c0 = (long long)L + (long long)a.E * up;                              // >= 0; c0 + j down = c_rel + E up: the same phase, q + E
    const int tiles = (a.n_out + RS_TILE - 1) / RS_TILE;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = tile * RS_TILE;
        const int base = (int)((c0 + (long long)j0 * down) / up);                         // ds[i] = buf[base + i]; d[q - k] of output j is buf[q + K - 1 - k]
        for (int i = t; i < a.span; i += RS_TILE) {
            const int n = base + i - H;
            ds[i] = n < 0 ? (double)dh[H + n] : (n < a.n16 ? (double)d_at(n) : 0.0);
        }
        __syncthreads();
        const int j = j0 + t;
        if (j < a.n_out) {
            const long long c = c0 + (long long)j * down;
            const int p = (int)(c % up);
            const double* __restrict__ hrow = tab + (size_t)p * K;
            const double* __restrict__ dq = ds + ((int)(c / up) - base + K - 1);          // dq[-k], 0 <= index < span
            const float xdel = j < Lx ? xh[j] : xr[j - Lx];
            yr[j] = fmaf(g, xdel, (float)rs_dot(hrow, dq, K));
        }
        __syncthreads();                                   // ds is the next tile's (and the record's) staging space
    }
    float* ms = reinterpret_cast<float*>(ds);
    const int R = H + lam + Lx, cap = 2 * a.stage;
    for (int r0 = 0; r0 < R; r0 += cap) {
        const int r1 = r0 + cap < R ? r0 + cap : R;
        for (int i = r0 + t; i < r1; i += RS_TILE) {       // the last H, lam, Lx samples of history + row; every read at or behind entry i
            float v;
            if (i < H) {
                const int n = a.n16 - H + i;
                v = n < 0 ? dh[H + n] : d_at(n);
            } else if (i < H + lam) {
                const int n = a.n16 - lam + (i - H);
                v = n < 0 ? lowh[lam + n] : lr[n];
            } else {
                const int m = a.n_out - Lx + (i - H - lam);
                v = m < 0 ? xh[Lx + m] : xr[m];
            }
            ms[i - r0] = v;
        }
        __syncthreads();
        for (int i = r0 + t; i < r1; i += RS_TILE) rec[i] = ms[i - r0];
        __syncthreads();
    }
    if (t == 0) head[0] = (int)((long long)L + (long long)a.n_out * down - (long long)a.n16 * up);
}

inline bool hbs_sizes_ok(int H, int lam, int Lx) {
    return H >= 0 && H <= HBS_MAX_H && lam >= 0 && lam <= NELE_HBUP_MAX_LAG16 && Lx >= 0 && Lx <= NELE_HBUP_MAX_LAG;
}

// section 25: the scheduled up-converter's plan (nele_sched_stream_plan: K, D, L0, the schedule) with the lead L0 - s; E and H from it
int hbs_plan(const char* name, int up, int down, int zeros, int s, HbsPlan* p) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(up > down, "%s: up=%d / down=%d is a device rate at or below 16 kHz: no band above the 16 kHz path's to carry", name, up, down);
    NELE_CHECK_ARG(zeros >= 1 && zeros <= RS_MAX_ZEROS, "%s: zeros=%d outside 1 .. %d", name, zeros, RS_MAX_ZEROS);
    NELE_CHECK_ARG(s >= 0 && s < down, "%s: s=%d outside 0 .. down - 1 = %d", name, s, down - 1);
    int info[NELE_SCHED_INFO];
    if (nele_sched_stream_plan(up, down, zeros, 0, info) != NELE_OK)                       // what is left to refuse: the delay against the hop
        return nele_set_error(NELE_ERR_INVALID_ARG, "%s: the up-converter's delay is longer than the shortest hop (up=%d, down=%d, zeros=%d)", name,
                              up, down, zeros);
    p->K = info[NELE_SCHED_I_K];
    p->D_up = info[NELE_SCHED_I_D];
    p->rnum = info[NELE_SCHED_I_RNUM];
    p->P = info[NELE_SCHED_I_P];
    p->hop_min = info[NELE_SCHED_I_HOP_MIN];
    p->hop_max = info[NELE_SCHED_I_HOP_MAX];
    const int W = down - down / p->P;                                                       // section 20: the swing of the lead
    p->s = s;
    p->L0 = info[NELE_SCHED_I_L0] - s;
    p->E = W - p->L0 > 0 ? (W - p->L0 + up - 1) / up : 0;
    p->H = p->K - 1 + p->E;
    return NELE_OK;
}

int hbs_check(const char* name, const void* state, long long state_bytes, int S, int up, int down, int K, int s, int lam, int Lx, HbsPlan* p) {
    if (int st = rs_check_ratio(name, up, down)) return st;
    *p = HbsPlan{};
    const int zeros = K >= 1 && K <= HBS_MAX_H ? rs_zeros_of(up, down, K) : 0;
    if (zeros) (void)hbs_plan(name, up, down, zeros, s, p);                              // H sizes the state; params() reports what is wrong
    auto params = [&]() -> int {
        NELE_CHECK_ARG(zeros, "%s: K=%d is not the table width of up=%d, down=%d for any zeros in 1 .. %d", name, K, up, down, RS_MAX_ZEROS);
        if (int st = hbs_plan(name, up, down, zeros, s, p)) return st;
        NELE_CHECK_ARG(lam >= 0 && lam <= NELE_HBUP_MAX_LAG16 && lam % RS_TILE == 0, "%s: lam=%d is not a whole number of hops in 0 .. %d", name, lam,
                       NELE_HBUP_MAX_LAG16);
        NELE_CHECK_ARG(Lx >= 0 && Lx <= NELE_HBUP_MAX_LAG, "%s: Lx=%d outside 0 .. %d", name, Lx, NELE_HBUP_MAX_LAG);
        const long long rest = ((long long)Lx - p->D_up) * down - s - (long long)lam * up;   // D_down up
        NELE_CHECK_ARG(rest >= 0 && rest % up == 0,
                       "%s: Lx=%d is not (D_down + lam) up / down + D_up + s / down for any D_down >= 0 (up=%d, down=%d, D_up=%d, s=%d, lam=%d)", name,
                       Lx, up, down, p->D_up, s, lam);
        p->lam = lam;
        p->Lx = Lx;
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_hbsched_state_bytes(S, p->H, lam, Lx), "nele_hbsched_state_bytes", p->H);
}

// slots == null: every record; write_hdr: the header too
int hbs_reset(const char* name, void* state, int S, int up, int down, int K, const HbsPlan& p, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[8] = {S, K, up, down, p.H, p.L0, p.lam, p.Lx};
    return slot_state_reset(name, state, HBS_HDR_BYTES, hbs_rec_bytes(p.H, p.lam, p.Lx), S, slots, write_hdr ? 8 : 0, hdr, stream, p.L0);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" int nele_hbsched_plan(int up, int down, int zeros, int lag_hops, int d_down, int* info_host) {
    const char* name = "nele_hbsched_plan";
    NELE_CHECK_ARG(info_host, "%s: null info_host", name);
    if (int st = rs_check_ratio(name, up, down)) return st;
    NELE_CHECK_ARG(lag_hops >= 1 && lag_hops * RS_TILE <= NELE_HBUP_MAX_LAG16, "%s: lag_hops=%d outside 1 .. %d", name, lag_hops,
                   NELE_HBUP_MAX_LAG16 / RS_TILE);
    NELE_CHECK_ARG(d_down >= 0 && d_down <= RS_TILE, "%s: d_down=%d outside 0 .. %d, a down-converter's delay at 16 kHz", name, d_down, RS_TILE);
    const int lam = lag_hops * RS_TILE;
    const long long through = (long long)(d_down + lam) * up;                             // the 16 kHz side's delay in ticks of 1 / down
    const int s = (int)((down - through % down) % down);
    HbsPlan p{};
    if (int st = hbs_plan(name, up, down, zeros, s, &p)) return st;
    const long long Lx = (through + s) / down + p.D_up;
    NELE_CHECK_ARG(Lx <= NELE_HBUP_MAX_LAG, "%s: lag_hops=%d is a lag of %lld samples at the device rate, above %d", name, lag_hops, Lx,
                   NELE_HBUP_MAX_LAG);
    info_host[NELE_HBSCHED_I_K] = p.K;
    info_host[NELE_HBSCHED_I_D_UP] = p.D_up;
    info_host[NELE_HBSCHED_I_S] = s;
    info_host[NELE_HBSCHED_I_L0] = p.L0;
    info_host[NELE_HBSCHED_I_E] = p.E;
    info_host[NELE_HBSCHED_I_H] = p.H;
    info_host[NELE_HBSCHED_I_LAM] = lam;
    info_host[NELE_HBSCHED_I_LX] = (int)Lx;
    info_host[NELE_HBSCHED_I_RNUM] = p.rnum;
    info_host[NELE_HBSCHED_I_P] = p.P;
    info_host[NELE_HBSCHED_I_HOP_MIN] = p.hop_min;
    info_host[NELE_HBSCHED_I_HOP_MAX] = p.hop_max;
    return NELE_OK;
}

extern "C" long long nele_hbsched_record_bytes(int H, int lam, int Lx) {
    if (!hbs_sizes_ok(H, lam, Lx)) return -1;
    return hbs_rec_bytes(H, lam, Lx);
}

extern "C" long long nele_hbsched_state_bytes(int max_streams, int H, int lam, int Lx) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || !hbs_sizes_ok(H, lam, Lx)) return -1;
    return HBS_HDR_BYTES + (long long)max_streams * hbs_rec_bytes(H, lam, Lx);
}

extern "C" int nele_hbsched_init(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx, void* stream) {
    const char* name = "nele_hbsched_init";
    HbsPlan p;
    if (int st = hbs_check(name, state, state_bytes, max_streams, up, down, K, s, lam, Lx, &p)) return st;
    return hbs_reset(name, state, max_streams, up, down, K, p, nullptr, true, stream);
}

extern "C" int nele_hbsched_reset(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx,
                                  const unsigned char* slots, void* stream) {
    const char* name = "nele_hbsched_reset";
    HbsPlan p;
    if (int st = hbs_check(name, state, state_bytes, max_streams, up, down, K, s, lam, Lx, &p)) return st;
    return hbs_reset(name, state, max_streams, up, down, K, p, slots, false, stream);
}

extern "C" int nele_hbsched_hop(void* state, long long state_bytes, int max_streams, int up, int down, int K, int s, int lam, int Lx,
                                const double* hp_dev, const float* enh, long long enh_stride, const float* low, long long low_stride, const float* x,
                                long long x_stride, const float* gain, const unsigned char* active, int nh, int pos, float* y, long long y_stride,
                                void* stream) {
    const char* name = "nele_hbsched_hop";
    HbsPlan p;
    if (int st = hbs_check(name, state, state_bytes, max_streams, up, down, K, s, lam, Lx, &p)) return st;
    NELE_CHECK_ARG(hp_dev && enh && low && x && y, "%s: null table, enh, low, x or y", name);
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", name, nh);
    NELE_CHECK_ARG(pos >= 0 && pos < p.P, "%s: pos=%d outside 0 .. %d, the schedule's period less one", name, pos, p.P - 1);
    const long long n16 = (long long)nh * RS_TILE;
    const long long n_out = ((long long)pos + nh) * p.rnum / p.P - (long long)pos * p.rnum / p.P;      // nele_sched_stream_widths
    NELE_CHECK_ARG(n16 <= NELE_RESAMPLE_MAX_SAMPLES && n_out <= NELE_RESAMPLE_MAX_SAMPLES, "%s: nh=%d hops are %lld -> %lld samples, more than 2^30 per call",
                   name, nh, n16, n_out);
    NELE_CHECK_ARG(enh_stride >= n16 && low_stride >= n16, "%s: enh_stride=%lld or low_stride=%lld below nh 256=%lld", name, enh_stride, low_stride, n16);
    NELE_CHECK_ARG(x_stride >= n_out && y_stride >= n_out, "%s: x_stride=%lld or y_stride=%lld below the call's %lld samples at the device rate", name,
                   x_stride, y_stride, n_out);
    HbsArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.up = up;
    a.down = down;
    a.K = K;
    a.H = p.H;
    a.E = p.E;
    a.L0 = p.L0;
    a.lam = lam;
    a.Lx = Lx;
    a.span = rs_span(up, down, K);
    const int whole = (p.H + lam + Lx + 1) / 2, want = whole < HBS_STAGE_MAX ? whole : HBS_STAGE_MAX;      // the record in one chunk, up to 16 KiB
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
    const bool tab_lds = (long long)up * K * 8 <= RS_TAB_LDS_BYTES;
    // up > down: the span is at most 255 + K + 1 <= 385 doubles, the staging space 16 KiB, with the largest LDS table 32 KiB
    const size_t lds = ((size_t)a.stage + (tab_lds ? (size_t)up * K : 0)) * sizeof(double);
    const hipStream_t st = as_stream(stream);
    if (tab_lds)
        NELE_PROF("highband_sched", st, hipLaunchKernelGGL(hbsched_hop_kernel<true>, dim3(max_streams), dim3(RS_TILE), lds, st, a));
    else
        NELE_PROF("highband_sched", st, hipLaunchKernelGGL(hbsched_hop_kernel<false>, dim3(max_streams), dim3(RS_TILE), lds, st, a));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
