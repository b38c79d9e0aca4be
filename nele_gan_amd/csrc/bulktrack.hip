// A bulk-delay search that follows the delay when it moves after the lock (nele_track_*, include/nele_hip_track.h): the delay line and
// the search of csrc/bulkdelay.hip, with the search restarted from a cleared state behind every lock, over and over; a background search
// that locks elsewhere moves the delay, one that locks where the slot already is confirms it, one that runs out of patience gives up.
// The arithmetic is DESIGN.md section 18 (the search step itself section 16, csrc/bulk_search.h: the same code as nele_bulk_hop's);
// tests/track_ref.py restates it in numpy.
//   bulk_track_hop_kernel    : one workgroup per stream and call, looping over the call's hops
//   bulk_track_set_kernel    : nele_track_set_delay, one workgroup per slot (it clears the search state)
//   bulk_track_status_kernel : nele_track_status, one workgroup per slot
// Per hop: thread t moves sample t through the delay line; unless the slot rests (a workgroup-uniform branch) the search step runs and
// thread 0 takes the decision; a lock, a move, a confirmation or a give-up clears the ring and C_q with 16-byte stores spread over the
// 256 threads (the rest of the search state lives in registers and LDS over a call).  State is read and written with plain loads and
// stores by the stream's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "bulk_search.h"
#include "../../include/nele_hip_track.h"

namespace {

constexpr long long TRK_HDR_BYTES = SLOT_GEOM_HDR_BYTES;   // int [0] = max_streams, [1] = blocks (what nele_track_init was given)
// per-stream record, byte offsets.  A cleared record is a fresh slot, so cand, delay and last_move are kept plus one (0 = none).
constexpr long long TRK_O_META = 0;                        // int [16]: TRK_M_*
constexpr long long TRK_O_CONF = 64;                       // double: conf of the last evaluated hop
constexpr long long TRK_O_E = 256;                         // double [64]: e_q of the last evaluated hop
constexpr long long TRK_O_XPREV = TRK_O_E + 8 * BULK_MAXQ;          // float [256]: the previous hop of `played`
constexpr long long TRK_O_SD = TRK_O_XPREV + 4 * BULK_BLK;          // double [257 (+ 7)]: S_d
constexpr long long TRK_O_SX = TRK_O_SD + 8 * 264;                  // double [257 (+ 7)]: S_x
constexpr long long TRK_O_LINE = slot_al(TRK_O_SX + 8 * 264);       // float [Q][256]: the delay line, hop of k hops ago at (lhead - k) mod Q
__host__ __device__ constexpr long long trk_o_x(int Q) { return TRK_O_LINE + 4LL * BULK_BLK * Q; }      // double2 [Q][256]: X_q at (head + q) % Q
__host__ __device__ constexpr long long trk_o_c(int Q) { return trk_o_x(Q) + 16LL * BULK_BLK * Q; }     // double2 [Q][256]: C_q, right behind the ring
__host__ __device__ constexpr long long trk_rec_bytes(int Q) { return slot_al(trk_o_c(Q) + 16LL * BULK_BLK * Q); }
enum {
    TRK_M_HEAD = 0, TRK_M_LHEAD = 1, TRK_M_N = 2, TRK_M_CAND1 = 3, TRK_M_RUN = 4, TRK_M_DELAY1 = 5, TRK_M_AGE = 6, TRK_M_SLEEP = 7,
    TRK_M_MOVES = 8, TRK_M_CONFIRMS = 9, TRK_M_GAVEUPS = 10, TRK_M_LASTMOVE1 = 11, TRK_M_HOPS = 12
};
enum { TRK_NONE = 0, TRK_LOCK = 1, TRK_CONFIRM = 2, TRK_MOVE = 3 };

struct TrackArgs {
    unsigned char* state;
    int S, Q;
    const float* mic;            // [S][ld]
    const float* played;
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double lambda, ratio;
    int hold, patience, rest;
    float* aligned;              // [S][ld]
    unsigned char* moved;        // [S] or null
};

__device__ __forceinline__ int sat_inc(int v) { return v < 0x7fffffff ? v + 1 : v; }

// the ring and C_q of one record (contiguous, 8192 Q bytes) <- 0: 2 Q 16-byte stores per thread
__device__ __forceinline__ void track_clear_sums(unsigned char* rec, int Q, int t) {
    double2* p = reinterpret_cast<double2*>(rec + trk_o_x(Q));
    const int n16 = 2 * BULK_BLK * Q;
    for (int i = t; i < n16; i += 256) p[i] = make_double2(0.0, 0.0);
}

__global__ __launch_bounds__(256) void bulk_track_hop_kernel(TrackArgs a) {
    __shared__ BulkSearchLds lds;
    __shared__ int s_dec[2];                               // thread 0's decision: the delay, TRK_*
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) {                        // neither read nor written; no move fell in this call
        if (t == 0 && a.moved) a.moved[b] = 0;
        return;
    }
    if (!slot_hdr_matches(a.state, a.S, a.Q)) return;      // not the state nele_track_init laid out for (S, Q): touch nothing
    const int Q = a.Q;
    unsigned char* rec = a.state + TRK_HDR_BYTES + (size_t)b * trk_rec_bytes(Q);
    int* meta = reinterpret_cast<int*>(rec + TRK_O_META);
    float* line = reinterpret_cast<float*>(rec + TRK_O_LINE);
    BulkSearchRec R;
    R.confp = reinterpret_cast<double*>(rec + TRK_O_CONF);
    R.erec = reinterpret_cast<double*>(rec + TRK_O_E);
    R.xprev = reinterpret_cast<float*>(rec + TRK_O_XPREV);
    R.Sdp = reinterpret_cast<double*>(rec + TRK_O_SD);
    R.Sxp = reinterpret_cast<double*>(rec + TRK_O_SX);
    R.ring = reinterpret_cast<double2*>(rec + trk_o_x(Q));
    R.Cst = reinterpret_cast<double2*>(rec + trk_o_c(Q));
    const bool slot0 = (t == 0);

    // every thread keeps the slot's integers: they are workgroup-uniform (cand and run: thread 0's are the ones that count)
    BulkSearchRegs g;
    g.head = min(max(meta[TRK_M_HEAD], 0), Q - 1);
    int lhead = min(max(meta[TRK_M_LHEAD], 0), Q - 1);
    g.n = meta[TRK_M_N];
    g.cand = meta[TRK_M_CAND1] - 1;
    g.run = meta[TRK_M_RUN];
    int delay = min(meta[TRK_M_DELAY1], Q) - 1;
    int age = meta[TRK_M_AGE], sleep = meta[TRK_M_SLEEP];
    int moves = meta[TRK_M_MOVES], confirms = meta[TRK_M_CONFIRMS], gaveups = meta[TRK_M_GAVEUPS];
    int last_move = meta[TRK_M_LASTMOVE1] - 1, hops = meta[TRK_M_HOPS];
    int moved_here = 0;
    g.sd = g.sx = g.sd_ny = g.sx_ny = 0.0;
    bulk_search_load(lds, R, g, t);
    const float* micb = a.mic + (size_t)b * a.ld;
    const float* plb = a.played + (size_t)b * a.ld;
    float* outb = a.aligned + (size_t)b * a.ld;
    __syncthreads();

    for (int h = 0; h < a.nh; ++h) {
        const size_t col = (size_t)h * BULK_BLK;
        // ---- 1. push x onto the delay line (thread t: sample t of every hop, so its own earlier stores are what it reads back)
        const float xv = plb[col + t];
        lhead = (lhead + 1 == Q) ? 0 : lhead + 1;
        line[(size_t)lhead * BULK_BLK + t] = xv;
        // ---- 2. the background search, unless it rests (workgroup-uniform)
        if (sleep > 0) {
            sleep -= 1;
        } else {
            int qs = 0, kind = TRK_NONE;
            const bool evaluated = bulk_search_step(lds, R, g, Q, xv, micb[col + t], a.lambda, a.ratio, t, qs);
            age = sat_inc(age);
            if (evaluated) {
                if (slot0) {
                    int nd = delay, k = TRK_NONE;
                    if (g.run >= a.hold) {
                        if (delay < 0) {
                            nd = max(qs - 1, 0);
                            k = TRK_LOCK;
                        } else if (qs - delay >= 0 && qs - delay <= 2) {
                            k = TRK_CONFIRM;               // aligned, the main tap still lies in 0 .. 767
                        } else {
                            nd = max(qs - 1, 0);
                            k = TRK_MOVE;
                        }
                    }
                    s_dec[0] = nd;
                    s_dec[1] = k;
                }
                __syncthreads();                           // (thread 0's reads of ebuf are behind it too)
                delay = s_dec[0];
                kind = s_dec[1];
            }
            if (kind == TRK_CONFIRM) confirms = sat_inc(confirms);
            if (kind == TRK_MOVE) {
                moves = sat_inc(moves);
                last_move = hops;
                moved_here = 1;
            }
            bool clear = kind != TRK_NONE;
            if (!clear && delay >= 0 && age >= a.patience) {
                gaveups = sat_inc(gaveups);
                clear = true;
            }
            if (clear) {
                // the search state as reset leaves it; the delay line, delay, e, conf, the counters and the hop count are kept
                __syncthreads();                           // every wave's C_q stores and ring reads of this hop precede the zeros
                track_clear_sums(rec, Q, t);
                lds.xbuf[t] = 0.0f;                        // x_prev (its next reader is behind the next step's first barrier, as are the
                g.sd = g.sx = g.sd_ny = g.sx_ny = 0.0;     // next stores to the ring and C_q)
                g.head = 0;
                g.n = 0;
                g.cand = -1;
                g.run = 0;
                age = 0;
                sleep = a.rest;
            }
        }
        hops = sat_inc(hops);
        // ---- 3. the output hop: zeros before the first lock, then the delay line's entry of `delay` hops ago
        float y = 0.0f;
        if (delay == 0) {
            y = xv;
        } else if (delay > 0) {
            int lp = lhead - delay;
            if (lp < 0) lp += Q;
            y = line[(size_t)lp * BULK_BLK + t];
        }
        outb[col + t] = y;
    }
    bulk_search_store(lds, R, g, t);
    if (slot0) {
        meta[TRK_M_HEAD] = g.head;
        meta[TRK_M_LHEAD] = lhead;
        meta[TRK_M_N] = g.n;
        meta[TRK_M_CAND1] = g.cand + 1;
        meta[TRK_M_RUN] = g.run;
        meta[TRK_M_DELAY1] = delay + 1;
        meta[TRK_M_AGE] = age;
        meta[TRK_M_SLEEP] = sleep;
        meta[TRK_M_MOVES] = moves;
        meta[TRK_M_CONFIRMS] = confirms;
        meta[TRK_M_GAVEUPS] = gaveups;
        meta[TRK_M_LASTMOVE1] = last_move + 1;
        meta[TRK_M_HOPS] = hops;
        if (a.moved) a.moved[b] = (unsigned char)moved_here;
    }
}

// grid S, block 256: lock the slot and clear its search state (x_prev, S_d, S_x, the ring, C_q and the search's integers)
__global__ __launch_bounds__(256) void bulk_track_set_kernel(unsigned char* state, int S, int Q, const unsigned char* __restrict__ slots,
                                                              const int* __restrict__ delay_hops) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    if (slots && !slots[b]) return;
    const int d = delay_hops[b];
    if (d < 0 || d >= Q) return;                           // out of range: the slot stays as it is
    unsigned char* rec = state + TRK_HDR_BYTES + (size_t)b * trk_rec_bytes(Q);
    track_clear_sums(rec, Q, t);
    double2* p = reinterpret_cast<double2*>(rec + TRK_O_XPREV);
    for (int i = t; i < (int)((TRK_O_LINE - TRK_O_XPREV) / 16); i += 256) p[i] = make_double2(0.0, 0.0);
    if (t == 0) {
        int* meta = reinterpret_cast<int*>(rec + TRK_O_META);
        meta[TRK_M_HEAD] = 0;
        meta[TRK_M_N] = 0;
        meta[TRK_M_CAND1] = 0;
        meta[TRK_M_RUN] = 0;
        meta[TRK_M_DELAY1] = d + 1;
        meta[TRK_M_AGE] = 0;
        meta[TRK_M_SLEEP] = 0;
    }
}

// grid S, block 64
__global__ __launch_bounds__(64) void bulk_track_status_kernel(const unsigned char* __restrict__ state, int S, int Q, int* __restrict__ info,
                                                               double* __restrict__ energies, double* __restrict__ conf) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    const unsigned char* rec = state + TRK_HDR_BYTES + (size_t)b * trk_rec_bytes(Q);
    const int* meta = reinterpret_cast<const int*>(rec + TRK_O_META);
    if (t == 0) {
        if (info) {
            int* o = info + (size_t)b * NELE_TRACK_INFO;
            o[NELE_TRACK_I_DELAY] = min(meta[TRK_M_DELAY1], Q) - 1;
            o[NELE_TRACK_I_HOPS] = meta[TRK_M_HOPS];
            o[NELE_TRACK_I_AGE] = meta[TRK_M_AGE];
            o[NELE_TRACK_I_SLEEP] = meta[TRK_M_SLEEP];
            o[NELE_TRACK_I_MOVES] = meta[TRK_M_MOVES];
            o[NELE_TRACK_I_CONFIRMS] = meta[TRK_M_CONFIRMS];
            o[NELE_TRACK_I_GAVEUPS] = meta[TRK_M_GAVEUPS];
            o[NELE_TRACK_I_LAST_MOVE] = meta[TRK_M_LASTMOVE1] - 1;
        }
        if (conf) conf[b] = *reinterpret_cast<const double*>(rec + TRK_O_CONF);
    }
    if (energies && t < Q) energies[(size_t)b * Q + t] = reinterpret_cast<const double*>(rec + TRK_O_E)[t];
}

int track_check(const char* name, const void* state, long long state_bytes, int S, int Q) {
    auto params = [&]() -> int {
        NELE_CHECK_ARG(Q >= 2 && Q <= BULK_MAXQ, "%s: blocks=%d must be in 2 .. %d", name, Q, BULK_MAXQ);
        return NELE_OK;
    };
    return slot_state_check(name, state, state_bytes, S, params, nele_track_state_bytes(S, Q), "nele_track_state_bytes", Q);
}

// slots == null: every record; write_hdr: the header too
int track_reset(const char* name, void* state, int S, int Q, const unsigned char* slots, bool write_hdr, void* stream) {
    const int hdr[2] = {S, Q};
    return slot_state_reset(name, state, TRK_HDR_BYTES, trk_rec_bytes(Q), S, slots, write_hdr ? 2 : 0, hdr, stream);
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_track_state_bytes(int max_streams, int blocks) {
    if (max_streams <= 0 || max_streams > SLOT_MAX_STREAMS || blocks < 2 || blocks > BULK_MAXQ) return -1;
    return TRK_HDR_BYTES + (long long)max_streams * trk_rec_bytes(blocks);
}

extern "C" long long nele_track_stream_record_bytes(int blocks) {
    if (blocks < 2 || blocks > BULK_MAXQ) return -1;
    return trk_rec_bytes(blocks);
}

extern "C" int nele_track_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream) {
    int st = track_check("nele_track_init", state, state_bytes, max_streams, blocks);
    if (st) return st;
    return track_reset("nele_track_init", state, max_streams, blocks, nullptr, true, stream);
}

extern "C" int nele_track_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream) {
    int st = track_check("nele_track_reset", state, state_bytes, max_streams, blocks);
    if (st) return st;
    return track_reset("nele_track_reset", state, max_streams, blocks, slots, false, stream);
}

extern "C" int nele_track_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                                    const int* delay_hops, void* stream) {
    int st = track_check("nele_track_set_delay", state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(delay_hops, "nele_track_set_delay: null delay_hops");
    hipLaunchKernelGGL(bulk_track_set_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), (unsigned char*)state, max_streams, blocks, slots,
                       delay_hops);
    NELE_CHECK_LAUNCH("nele_track_set_delay");
    return NELE_OK;
}

extern "C" int nele_track_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                              const unsigned char* active, int nh, double lambda, double ratio, int hold, int patience, int rest,
                              float* aligned, unsigned char* moved, void* stream) {
    int st = track_check("nele_track_hop", state, state_bytes, max_streams, blocks);
    if (st) return st;
    NELE_CHECK_ARG(mic, "nele_track_hop: null mic");
    NELE_CHECK_ARG(played, "nele_track_hop: null played");
    NELE_CHECK_ARG(aligned, "nele_track_hop: null aligned");
    NELE_CHECK_ARG(nh >= 1 && nh <= (1 << 20), "nele_track_hop: nh=%d must be in 1 .. 1048576", nh);
    NELE_CHECK_ARG(lambda > 0.0 && lambda < 1.0, "nele_track_hop: lambda=%g must be in (0, 1)", lambda);
    NELE_CHECK_ARG(ratio > 1.0 && ratio <= 1e300, "nele_track_hop: ratio=%g must be finite and > 1", ratio);
    NELE_CHECK_ARG(hold >= 1, "nele_track_hop: hold=%d must be >= 1", hold);
    NELE_CHECK_ARG(patience >= 1, "nele_track_hop: patience=%d must be >= 1", patience);
    NELE_CHECK_ARG(rest >= 0, "nele_track_hop: rest=%d must be >= 0", rest);
    TrackArgs a{};
    a.state = (unsigned char*)state;
    a.S = max_streams;
    a.Q = blocks;
    a.mic = mic;
    a.played = played;
    a.ld = (long long)nh * BULK_BLK;
    a.active = active;
    a.nh = nh;
    a.lambda = lambda;
    a.ratio = ratio;
    a.hold = hold;
    a.patience = patience;
    a.rest = rest;
    a.aligned = aligned;
    a.moved = moved;
    hipLaunchKernelGGL(bulk_track_hop_kernel, dim3(max_streams), dim3(256), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH("nele_track_hop");
    return NELE_OK;
}

extern "C" int nele_track_status(const void* state, long long state_bytes, int max_streams, int blocks, int* info, double* energies,
                                 double* conf, void* stream) {
    int st = track_check("nele_track_status", state, state_bytes, max_streams, blocks);
    if (st) return st;
    hipLaunchKernelGGL(bulk_track_status_kernel, dim3(max_streams), dim3(64), 0, as_stream(stream), (const unsigned char*)state, max_streams, blocks,
                       info, energies, conf);
    NELE_CHECK_LAUNCH("nele_track_status");
    return NELE_OK;
}
