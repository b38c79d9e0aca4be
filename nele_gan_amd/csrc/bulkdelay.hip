// Bulk-delay search and alignment ahead of the echo canceller (nele_bulk_* and nele_track_*, include/nele_hip_ext.h): per stream slot, the
// whole number of hops by which `played` reaches the microphone late, found from SCOT-weighted cross-spectra against the last Q far-end
// blocks, and a delay line that hands `played` on late by it.  256-sample hops, 512-point float64 transforms (fft512.h), the packed
// spectra of csrc/aec.hip (256 double2: slot k = bin k, slot 0 = (bin 0, bin 256), products component-wise in slot 0).  The arithmetic is
// DESIGN.md section 16 and, for what happens behind the lock, section 18; tests/bulk_ref.py and tests/track_ref.py restate it in numpy.
//   bulk_hop_kernel<TRACK>    : one workgroup per stream and call, looping over the call's hops
//   bulk_set_kernel<TRACK>    : nele_bulk_set_delay (one thread per slot), nele_track_set_delay (one workgroup per slot: it clears the
//                               search state)
//   bulk_status_kernel<TRACK> : nele_bulk_status, nele_track_status, one workgroup per slot
// One record layout, one delay line and one search step (csrc/bulk_search.h) for the two sets of entry points; TRACK is what differs:
//   plain (nele_bulk_*)     : the slot searches until it locks, once.  From then on a workgroup-uniform branch leaves only the delay line,
//                             and a slot that comes into a call locked neither loads nor stores search state.
//   tracking (nele_track_*) : the search is started again from a cleared state behind every lock, over and over; a background search
//                             that locks elsewhere moves the delay, one that locks where the slot already is confirms it, one that runs
//                             out of patience gives up.  Unless the slot rests (a workgroup-uniform branch) the search step runs and
//                             thread 0 takes the decision; a lock, a move, a confirmation or a give-up clears the ring and C_q with
//                             16-byte stores spread over the 256 threads (the rest of the search state lives in registers and LDS over
//                             a call).
// Every operand is the stream's own, every sum has a fixed order: a slot's bits do not depend on the hop grouping, on B or on the other
// slots.  State is read and written with plain loads and stores by the stream's own workgroup; no atomics, nothing crosses workgroups.
#include "common.h"
#include "fft512.h"
#include "slot_state.h"
#include "bulk_search.h"
#include "../../include/nele_hip_ext.h"

namespace {

constexpr long long BULK_HDR_BYTES = SLOT_GEOM_HDR_BYTES;  // int [0] = max_streams, [1] = blocks (what *_init was given)
// per-stream record, byte offsets.  A cleared record is a fresh slot, so cand, delay and last_move are kept plus one (0 = none).
constexpr long long BULK_O_META = 0;                       // int [16]: BULK_M_*
constexpr long long BULK_O_CONF = 64;                      // double: conf of the last evaluated hop
constexpr long long BULK_O_E = 256;                        // double [64]: e_q of the last evaluated hop
constexpr long long BULK_O_XPREV = BULK_O_E + 8 * BULK_MAXQ;        // float [256]: the previous hop of `played` while searching
constexpr long long BULK_O_SD = BULK_O_XPREV + 4 * BULK_BLK;        // double [257 (+ 7)]: S_d
constexpr long long BULK_O_SX = BULK_O_SD + 8 * 264;                // double [257 (+ 7)]: S_x
constexpr long long BULK_O_LINE = slot_al(BULK_O_SX + 8 * 264);     // float [Q][256]: the delay line, hop of k hops ago at (lhead - k) mod Q
__host__ __device__ constexpr long long bulk_o_x(int Q) { return BULK_O_LINE + 4LL * BULK_BLK * Q; }    // double2 [Q][256]: X_q at (head + q) % Q
__host__ __device__ constexpr long long bulk_o_c(int Q) { return bulk_o_x(Q) + 16LL * BULK_BLK * Q; }   // double2 [Q][256]: C_q, right behind the ring
__host__ __device__ constexpr long long bulk_rec_bytes(int Q) { return slot_al(bulk_o_c(Q) + 16LL * BULK_BLK * Q); }
static_assert(bulk_rec_bytes(2) == 6144 + 9216 * 2 && bulk_rec_bytes(BULK_MAXQ) == 6144 + 9216 * BULK_MAXQ,
              "what nele_bulk_stream_record_bytes and nele_track_stream_record_bytes have always returned");
enum {                                                     // a plain search writes 0 .. 5 only: the others stay zero
    BULK_M_HEAD = 0, BULK_M_LHEAD = 1, BULK_M_N = 2, BULK_M_CAND1 = 3, BULK_M_RUN = 4, BULK_M_DELAY1 = 5, BULK_M_AGE = 6, BULK_M_SLEEP = 7,
    BULK_M_MOVES = 8, BULK_M_CONFIRMS = 9, BULK_M_GAVEUPS = 10, BULK_M_LASTMOVE1 = 11, BULK_M_HOPS = 12
};
enum { TRK_NONE = 0, TRK_LOCK = 1, TRK_CONFIRM = 2, TRK_MOVE = 3 };

struct BulkArgs {
    unsigned char* state;
    int S, Q;
    const float* mic;            // [S][ld]
    const float* played;
    long long ld;
    const unsigned char* active; // [S] or null (all)
    int nh;
    double lambda, ratio;
    int hold, patience, rest;    // (patience, rest: tracking)
    float* aligned;              // [S][ld]
    unsigned char* moved;        // [S] or null (tracking)
    int* delay_hops;             // [S] or null (plain)
};

__device__ __forceinline__ int sat_inc(int v) { return v < 0x7fffffff ? v + 1 : v; }

// the ring and C_q of one record (contiguous, 8192 Q bytes) <- 0: 2 Q 16-byte stores per thread
__device__ __forceinline__ void bulk_clear_sums(unsigned char* rec, int Q, int t) {
    double2* p = reinterpret_cast<double2*>(rec + bulk_o_x(Q));
    const int n16 = 2 * BULK_BLK * Q;
    for (int i = t; i < n16; i += 256) p[i] = make_double2(0.0, 0.0);
}

template <bool TRACK>
__global__ __launch_bounds__(256) void bulk_hop_kernel(BulkArgs a) {
    __shared__ BulkSearchLds lds;
    __shared__ int s_dec[TRACK ? 2 : 1];                   // thread 0's decision: the delay and, tracking, TRK_*
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= a.S) return;
    if (a.active && !a.active[b]) {                        // neither read nor written; tracking: no move fell in this call
        if constexpr (TRACK)
            if (t == 0 && a.moved) a.moved[b] = 0;
        return;
    }
    if (!slot_hdr_matches(a.state, a.S, a.Q)) return;      // not the state *_init laid out for (S, Q): touch nothing
    const int Q = a.Q;
    unsigned char* rec = a.state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q);
    int* meta = reinterpret_cast<int*>(rec + BULK_O_META);
    float* line = reinterpret_cast<float*>(rec + BULK_O_LINE);
    BulkSearchRec R;
    R.confp = reinterpret_cast<double*>(rec + BULK_O_CONF);
    R.erec = reinterpret_cast<double*>(rec + BULK_O_E);
    R.xprev = reinterpret_cast<float*>(rec + BULK_O_XPREV);
    R.Sdp = reinterpret_cast<double*>(rec + BULK_O_SD);
    R.Sxp = reinterpret_cast<double*>(rec + BULK_O_SX);
    R.ring = reinterpret_cast<double2*>(rec + bulk_o_x(Q));
    R.Cst = reinterpret_cast<double2*>(rec + bulk_o_c(Q));
    const bool slot0 = (t == 0);

    // every thread keeps the slot's integers: they are workgroup-uniform (cand and run: thread 0's are the ones that count)
    BulkSearchRegs g;
    g.head = min(max(meta[BULK_M_HEAD], 0), Q - 1);
    int lhead = min(max(meta[BULK_M_LHEAD], 0), Q - 1);
    g.n = meta[BULK_M_N];
    g.cand = meta[BULK_M_CAND1] - 1;
    g.run = meta[BULK_M_RUN];
    int delay = min(meta[BULK_M_DELAY1], Q) - 1;
    int age = 0, sleep = 0, moves = 0, confirms = 0, gaveups = 0, last_move = -1, hops = 0, moved_here = 0;
    if constexpr (TRACK) {
        age = meta[BULK_M_AGE], sleep = meta[BULK_M_SLEEP];
        moves = meta[BULK_M_MOVES], confirms = meta[BULK_M_CONFIRMS], gaveups = meta[BULK_M_GAVEUPS];
        last_move = meta[BULK_M_LASTMOVE1] - 1, hops = meta[BULK_M_HOPS];
    }
    const bool searched = TRACK || delay < 0;              // plain: the search state is read, and written back, only by a slot that came in searching
    g.sd = g.sx = g.sd_ny = g.sx_ny = 0.0;
    if (searched) bulk_search_load(lds, R, g, t);
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
        if constexpr (!TRACK) {
            if (delay < 0) {
                // ---- 2. the search step; the lock is a run of `hold` hops (thread 0 decides), once: nothing is cleared
                int qs = 0;
                if (bulk_search_step(lds, R, g, Q, xv, micb[col + t], a.lambda, a.ratio, t, qs)) {
                    if (slot0) s_dec[0] = (g.run >= a.hold) ? max(qs - 1, 0) : -1;
                    __syncthreads();
                    delay = s_dec[0];
                }
            }
        } else {
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
                                k = TRK_CONFIRM;           // aligned, the main tap still lies in 0 .. 767
                            } else {
                                nd = max(qs - 1, 0);
                                k = TRK_MOVE;
                            }
                        }
                        s_dec[0] = nd;
                        s_dec[1] = k;
                    }
                    __syncthreads();                       // (thread 0's reads of ebuf are behind it too)
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
                    __syncthreads();                       // every wave's C_q stores and ring reads of this hop precede the zeros
                    bulk_clear_sums(rec, Q, t);
                    lds.xbuf[t] = 0.0f;                    // x_prev (its next reader is behind the next step's first barrier, as are the
                    g.sd = g.sx = g.sd_ny = g.sx_ny = 0.0; // next stores to the ring and C_q)
                    g.head = 0;
                    g.n = 0;
                    g.cand = -1;
                    g.run = 0;
                    age = 0;
                    sleep = a.rest;
                }
            }
            hops = sat_inc(hops);
        }
        // ---- 3. the output hop: zeros before the (first) lock, then the delay line's entry of `delay` hops ago
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
    if (searched) bulk_search_store(lds, R, g, t);
    if (slot0) {
        meta[BULK_M_LHEAD] = lhead;
        if (searched) {
            meta[BULK_M_HEAD] = g.head;
            meta[BULK_M_N] = g.n;
            meta[BULK_M_CAND1] = g.cand + 1;
            meta[BULK_M_RUN] = g.run;
            meta[BULK_M_DELAY1] = delay + 1;
        }
        if constexpr (TRACK) {
            meta[BULK_M_AGE] = age;
            meta[BULK_M_SLEEP] = sleep;
            meta[BULK_M_MOVES] = moves;
            meta[BULK_M_CONFIRMS] = confirms;
            meta[BULK_M_GAVEUPS] = gaveups;
            meta[BULK_M_LASTMOVE1] = last_move + 1;
            meta[BULK_M_HOPS] = hops;
            if (a.moved) a.moved[b] = (unsigned char)moved_here;
        } else {
            if (a.delay_hops) a.delay_hops[b] = delay;
        }
    }
}

// Lock the slot at delay_hops[b].  Plain: one thread per slot, only the delay is written.  Tracking: grid S, block 256, the search state
// (x_prev, S_d, S_x, the ring, C_q and the search's integers) is cleared as well.
template <bool TRACK>
__global__ __launch_bounds__(256) void bulk_set_kernel(unsigned char* state, int S, int Q, const unsigned char* __restrict__ slots,
                                                        const int* __restrict__ delay_hops) {
    const int b = TRACK ? blockIdx.x : blockIdx.x * blockDim.x + threadIdx.x;
    const int t = TRACK ? threadIdx.x : 0;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    if (slots && !slots[b]) return;
    const int d = delay_hops[b];
    if (d < 0 || d >= Q) return;                           // out of range: the slot stays as it is
    unsigned char* rec = state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q);
    int* meta = reinterpret_cast<int*>(rec + BULK_O_META);
    if constexpr (TRACK) {
        bulk_clear_sums(rec, Q, t);
        double2* p = reinterpret_cast<double2*>(rec + BULK_O_XPREV);
        for (int i = t; i < (int)((BULK_O_LINE - BULK_O_XPREV) / 16); i += 256) p[i] = make_double2(0.0, 0.0);
    }
    if (t == 0) {
        if constexpr (TRACK) {
            meta[BULK_M_HEAD] = 0;
            meta[BULK_M_N] = 0;
            meta[BULK_M_CAND1] = 0;
            meta[BULK_M_RUN] = 0;
            meta[BULK_M_AGE] = 0;
            meta[BULK_M_SLEEP] = 0;
        }
        meta[BULK_M_DELAY1] = d + 1;
    }
}

// grid S, block 64.  ints: plain delay_hops [S], tracking info [S][NELE_TRACK_INFO]; hops_searched: plain only
template <bool TRACK>
__global__ __launch_bounds__(64) void bulk_status_kernel(const unsigned char* __restrict__ state, int S, int Q, int* __restrict__ ints,
                                                         int* __restrict__ hops_searched, double* __restrict__ energies,
                                                         double* __restrict__ conf) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= S || !slot_hdr_matches(state, S, Q)) return;
    const unsigned char* rec = state + BULK_HDR_BYTES + (size_t)b * bulk_rec_bytes(Q);
    const int* meta = reinterpret_cast<const int*>(rec + BULK_O_META);
    if (t == 0) {
        if constexpr (TRACK) {
            if (ints) {
                int* o = ints + (size_t)b * NELE_TRACK_INFO;
                o[NELE_TRACK_I_DELAY] = min(meta[BULK_M_DELAY1], Q) - 1;
                o[NELE_TRACK_I_HOPS] = meta[BULK_M_HOPS];
                o[NELE_TRACK_I_AGE] = meta[BULK_M_AGE];
                o[NELE_TRACK_I_SLEEP] = meta[BULK_M_SLEEP];
                o[NELE_TRACK_I_MOVES] = meta[BULK_M_MOVES];
                o[NELE_TRACK_I_CONFIRMS] = meta[BULK_M_CONFIRMS];
                o[NELE_TRACK_I_GAVEUPS] = meta[BULK_M_GAVEUPS];
                o[NELE_TRACK_I_LAST_MOVE] = meta[BULK_M_LASTMOVE1] - 1;
            }
        } else {
            if (ints) ints[b] = min(meta[BULK_M_DELAY1], Q) - 1;
            if (hops_searched) hops_searched[b] = meta[BULK_M_N];
        }
        if (conf) conf[b] = *reinterpret_cast<const double*>(rec + BULK_O_CONF);
    }
    if (energies && t < Q) energies[(size_t)b * Q + t] = reinterpret_cast<const double*>(rec + BULK_O_E)[t];
}

// ---- the host side, once for both sets of entry points.  An entry point's own name and its *_state_bytes' name are in the messages.
struct BulkEntry {
    const char* name;
    const char* bytes_fn;
    bool track;
};
constexpr BulkEntry plain(const char* name) { return {name, "nele_bulk_state_bytes", false}; }
constexpr BulkEntry tracking(const char* name) { return {name, "nele_track_state_bytes", true}; }

long long bulk_state_bytes(int S, int Q) {
    if (S <= 0 || S > SLOT_MAX_STREAMS || Q < 2 || Q > BULK_MAXQ) return -1;
    return BULK_HDR_BYTES + (long long)S * bulk_rec_bytes(Q);
}

long long bulk_stream_record_bytes(int Q) {
    if (Q < 2 || Q > BULK_MAXQ) return -1;
    return bulk_rec_bytes(Q);
}

int bulk_check(BulkEntry e, const void* state, long long state_bytes, int S, int Q) {
    auto params = [&]() -> int {
        NELE_CHECK_ARG(Q >= 2 && Q <= BULK_MAXQ, "%s: blocks=%d must be in 2 .. %d", e.name, Q, BULK_MAXQ);
        return NELE_OK;
    };
    return slot_state_check(e.name, state, state_bytes, S, params, bulk_state_bytes(S, Q), e.bytes_fn, Q);
}

// slots == null: every record; write_hdr (*_init): the header too
int bulk_reset(BulkEntry e, void* state, long long state_bytes, int S, int Q, const unsigned char* slots, bool write_hdr, void* stream) {
    int st = bulk_check(e, state, state_bytes, S, Q);
    if (st) return st;
    const int hdr[2] = {S, Q};
    return slot_state_reset(e.name, state, BULK_HDR_BYTES, bulk_rec_bytes(Q), S, slots, write_hdr ? 2 : 0, hdr, stream);
}

int bulk_set_delay(BulkEntry e, void* state, long long state_bytes, int S, int Q, const unsigned char* slots, const int* delay_hops,
                   void* stream) {
    int st = bulk_check(e, state, state_bytes, S, Q);
    if (st) return st;
    NELE_CHECK_ARG(delay_hops, "%s: null delay_hops", e.name);
    if (e.track)
        hipLaunchKernelGGL(bulk_set_kernel<true>, dim3(S), dim3(256), 0, as_stream(stream), (unsigned char*)state, S, Q, slots, delay_hops);
    else
        hipLaunchKernelGGL(bulk_set_kernel<false>, dim3((S + 255) / 256), dim3(256), 0, as_stream(stream), (unsigned char*)state, S, Q, slots,
                           delay_hops);
    NELE_CHECK_LAUNCH(e.name);
    return NELE_OK;
}

// a.state, S, Q, mic, played, active, nh, the settings and the outputs as the entry point was given them (plain: patience 1, rest 0)
int bulk_hop(BulkEntry e, long long state_bytes, BulkArgs a, void* stream) {
    int st = bulk_check(e, a.state, state_bytes, a.S, a.Q);
    if (st) return st;
    NELE_CHECK_ARG(a.mic, "%s: null mic", e.name);
    NELE_CHECK_ARG(a.played, "%s: null played", e.name);
    NELE_CHECK_ARG(a.aligned, "%s: null aligned", e.name);
    NELE_CHECK_ARG(a.nh >= 1 && a.nh <= (1 << 20), "%s: nh=%d must be in 1 .. 1048576", e.name, a.nh);
    NELE_CHECK_ARG(a.lambda > 0.0 && a.lambda < 1.0, "%s: lambda=%g must be in (0, 1)", e.name, a.lambda);
    NELE_CHECK_ARG(a.ratio > 1.0 && a.ratio <= 1e300, "%s: ratio=%g must be finite and > 1", e.name, a.ratio);
    NELE_CHECK_ARG(a.hold >= 1, "%s: hold=%d must be >= 1", e.name, a.hold);
    NELE_CHECK_ARG(a.patience >= 1, "%s: patience=%d must be >= 1", e.name, a.patience);
    NELE_CHECK_ARG(a.rest >= 0, "%s: rest=%d must be >= 0", e.name, a.rest);
    a.ld = (long long)a.nh * BULK_BLK;
    if (e.track)
        hipLaunchKernelGGL(bulk_hop_kernel<true>, dim3(a.S), dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(bulk_hop_kernel<false>, dim3(a.S), dim3(256), 0, as_stream(stream), a);
    NELE_CHECK_LAUNCH(e.name);
    return NELE_OK;
}

int bulk_status(BulkEntry e, const void* state, long long state_bytes, int S, int Q, int* ints, int* hops_searched, double* energies,
                double* conf, void* stream) {
    int st = bulk_check(e, state, state_bytes, S, Q);
    if (st) return st;
    if (e.track)
        hipLaunchKernelGGL(bulk_status_kernel<true>, dim3(S), dim3(64), 0, as_stream(stream), (const unsigned char*)state, S, Q, ints, hops_searched,
                           energies, conf);
    else
        hipLaunchKernelGGL(bulk_status_kernel<false>, dim3(S), dim3(64), 0, as_stream(stream), (const unsigned char*)state, S, Q, ints, hops_searched,
                           energies, conf);
    NELE_CHECK_LAUNCH(e.name);
    return NELE_OK;
}

}  // namespace

// ============================================================================================ C ABI
extern "C" long long nele_bulk_state_bytes(int max_streams, int blocks) { return bulk_state_bytes(max_streams, blocks); }
extern "C" long long nele_track_state_bytes(int max_streams, int blocks) { return bulk_state_bytes(max_streams, blocks); }
extern "C" long long nele_bulk_stream_record_bytes(int blocks) { return bulk_stream_record_bytes(blocks); }
extern "C" long long nele_track_stream_record_bytes(int blocks) { return bulk_stream_record_bytes(blocks); }

extern "C" int nele_bulk_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream) {
    return bulk_reset(plain("nele_bulk_init"), state, state_bytes, max_streams, blocks, nullptr, true, stream);
}
extern "C" int nele_track_init(void* state, long long state_bytes, int max_streams, int blocks, void* stream) {
    return bulk_reset(tracking("nele_track_init"), state, state_bytes, max_streams, blocks, nullptr, true, stream);
}

extern "C" int nele_bulk_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream) {
    return bulk_reset(plain("nele_bulk_reset"), state, state_bytes, max_streams, blocks, slots, false, stream);
}
extern "C" int nele_track_reset(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots, void* stream) {
    return bulk_reset(tracking("nele_track_reset"), state, state_bytes, max_streams, blocks, slots, false, stream);
}

extern "C" int nele_bulk_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                                   const int* delay_hops, void* stream) {
    return bulk_set_delay(plain("nele_bulk_set_delay"), state, state_bytes, max_streams, blocks, slots, delay_hops, stream);
}
extern "C" int nele_track_set_delay(void* state, long long state_bytes, int max_streams, int blocks, const unsigned char* slots,
                                    const int* delay_hops, void* stream) {
    return bulk_set_delay(tracking("nele_track_set_delay"), state, state_bytes, max_streams, blocks, slots, delay_hops, stream);
}

extern "C" int nele_bulk_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                             const unsigned char* active, int nh, double lambda, double ratio, int hold, float* aligned, int* delay_hops,
                             void* stream) {
    return bulk_hop(plain("nele_bulk_hop"), state_bytes,
                    {(unsigned char*)state, max_streams, blocks, mic, played, 0, active, nh, lambda, ratio, hold, 1, 0, aligned, nullptr, delay_hops},
                    stream);
}
extern "C" int nele_track_hop(void* state, long long state_bytes, int max_streams, int blocks, const float* mic, const float* played,
                              const unsigned char* active, int nh, double lambda, double ratio, int hold, int patience, int rest,
                              float* aligned, unsigned char* moved, void* stream) {
    return bulk_hop(tracking("nele_track_hop"), state_bytes,
                    {(unsigned char*)state, max_streams, blocks, mic, played, 0, active, nh, lambda, ratio, hold, patience, rest, aligned, moved,
                     nullptr},
                    stream);
}

extern "C" int nele_bulk_status(const void* state, long long state_bytes, int max_streams, int blocks, int* delay_hops, int* hops_searched,
                                double* energies, double* conf, void* stream) {
    return bulk_status(plain("nele_bulk_status"), state, state_bytes, max_streams, blocks, delay_hops, hops_searched, energies, conf, stream);
}
extern "C" int nele_track_status(const void* state, long long state_bytes, int max_streams, int blocks, int* info, double* energies,
                                 double* conf, void* stream) {
    return bulk_status(tracking("nele_track_status"), state, state_bytes, max_streams, blocks, info, nullptr, energies, conf, stream);
}
