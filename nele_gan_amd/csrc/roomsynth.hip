// Shoebox room impulse responses by the image-source method, float64 (include/nele_hip.h nele_rir_synth).  The
// reference ships no room and no generator of one: an addition, not a parity item.
//   image = ((ux, lx), (uy, ly), (uz, lz));  delta_a = (1 - 2u) s_a + 2 l L_a - m_a;  g_a = beta[a][0]^|l - u| beta[a][1]^|l|
//   d = |delta|,  A = g_x g_y g_z / (4 pi d),  tau = d fs / c
//   h[n] = sum over the images with |n - tau| <= W of A sinc(n - tau) 0.5 (1 + cos(pi (n - tau) / W))
// rir_synth_kernel is a gather: one workgroup per (room, tile of RIRS_TILE taps), a thread per tap.  A tile is reached only by the
// images in the shell dlo <= d <= dhi (the tile's first and last tap -/+ W samples, widened by 1e-9 so that rounding can only add
// candidates: the test |n - tau| <= W itself is made per tap on the tau every thread reads).  The workgroup walks the (x image,
// y image) pairs of the disc rho <= dhi in a fixed order, RIRS_PAIRS at a time.  A pair admits, per z parity, the z images with
// zlo <= |delta_z| <= zhi, zhi^2 = dhi^2 - rho^2, zlo^2 = dlo^2 - rho^2: two index intervals from four divisions, no search - so the
// enumeration costs one unit of work per pair of the 2-D disc and one per image of the shell, never one per lattice point of the ball.
// A prefix sum over the 4 intervals of each pair numbers the batch's images; entry e of a chunk of RIRS_CAP is then built by thread
// e mod 256 (a binary search over the 257 offsets finds its interval): distance, amplitude and ALL the trigonometry happen here, once
// per image -
//   sin(pi (n - tau)) = (-1)^(n - k) (-sin(pi f)),  k = rint(tau), f = tau - k            -> S = (-1)^k (-sinpi(f)) A / pi
//   cos(pi (n - tau) / W) = cos(pi n / W) cos(pi tau / W) + sin(pi n / W) sin(pi tau / W)  -> hc, hs = half of cospi, sinpi (tau / W)
// - and a tap's term is (S / x) (p0 + hc pc + hs ps), x = n - tau, with p0, pc, ps = (-1)^n (0.5, cospi, sinpi ((n mod 2W) / W)) held
// by the tap's thread: a reciprocal (v_rcp_f64 and two Newton steps) and four fused multiply-adds.  Every thread sums its tap over the
// chunk in list order; the list's order is a function of the room alone (a wider shell only inserts entries that no tap of the
// narrower one accepts), so a tap's bits do not depend on R, r, N, taps or the other rooms.  No atomics, no workspace.
// The axis with the smallest size plays z (most images per metre: they are the ones found without a test).  beta^k comes from a
// table of RIRS_PTAB powers per wall built with pow() by each workgroup that walks more than 4 batches of pairs (pow() itself beyond
// the table and in the early tiles, whose few images do not repay 6 pow() per thread: the same values, so the same bits).
#include "common.h"
#include <cmath>
#include "../../include/nele_hip.h"

#define RIRS_TILE 256                  // taps per workgroup = threads per workgroup
#define RIRS_PAIRS 64                  // (x image, y image) pairs per batch: 4 z intervals each, one per thread
#define RIRS_CAP 512                   // images per LDS chunk
#define RIRS_PTAB 256                  // tabulated powers per wall
#define RIRS_WIDEN 1e-9                // relative widening of the shell's radii

__device__ __forceinline__ int rirs_check(const double* __restrict__ q) {
    int st = 0;
    double dist2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double L = q[a], s = q[3 + a], m = q[6 + a];
        const bool size_ok = L >= NELE_RIR_MIN_SIZE_M && L <= NELE_RIR_MAX_SIZE_M;              // (false for NaN)
        if (!size_ok) st |= NELE_RIR_BAD_SIZE;
        else if (!(s > 0.0 && s < L && m > 0.0 && m < L)) st |= NELE_RIR_BAD_POSITION;
        dist2 += (s - m) * (s - m);
        for (int w = 0; w < 2; ++w) {
            const double b = q[9 + 2 * a + w];
            if (!(b >= 0.0 && b <= 1.0)) st |= NELE_RIR_BAD_BETA;
        }
    }
    if (!(dist2 >= 1e-4)) st |= NELE_RIR_BAD_POSITION;
    return st;
}

// images (u, l) of one axis with |b_u + 2 L l| <= lim: l = lo .. lo + cnt - 1
__device__ __forceinline__ void rirs_range(double b, double twoL, double lim, int& lo, int& cnt) {
    lo = (int)ceil((-lim - b) / twoL);
    const int hi = (int)floor((lim - b) / twoL);
    cnt = max(hi - lo + 1, 0);
}

// tab == nullptr: a tile with few pairs builds no table (its entries are pow()'s own values, so the bits are the same either way)
__device__ __forceinline__ double rirs_pow(const double* __restrict__ tab, double beta, int k) {
    return (tab && k < RIRS_PTAB) ? tab[k] : pow(beta, (double)k);
}
// g(u, l) = beta0^|l - u| beta1^|l|
__device__ __forceinline__ double rirs_gain(const double* __restrict__ tab0, const double* __restrict__ tab1, double beta0, double beta1, int u, int l) {
    return rirs_pow(tab0, beta0, abs(l - u)) * rirs_pow(tab1, beta1, abs(l));
}

__global__ __launch_bounds__(RIRS_TILE) void rir_synth_kernel(const double* __restrict__ rooms, const int* __restrict__ taps, int N, int ntiles,
                                                              double fs, double c, int W, double* __restrict__ out, int* __restrict__ status) {
    __shared__ double e_tau[RIRS_CAP], e_S[RIRS_CAP], e_hc[RIRS_CAP], e_hs[RIRS_CAP], e_A[RIRS_CAP];
    __shared__ double ptab[6][RIRS_PTAB];
    __shared__ double u_rho2[RIRS_PAIRS], u_g[RIRS_PAIRS];
    __shared__ int u_lo[RIRS_TILE], u_off[RIRS_TILE + 1], wave_tot[RIRS_TILE / 64];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int tile = ntiles - 1 - (int)blockIdx.x;           // the late tiles hold the most images: they start first
    const double* __restrict__ q = rooms + (size_t)r * 16;
    const int st = rirs_check(q);
    const int nt = min(max(taps[r], 0), N);
    const int n0 = tile * RIRS_TILE, n = n0 + tid;
    double* __restrict__ o = out + (size_t)r * N;
    if (tile == 0 && tid == 0) status[r] = st;
    if (st != 0 || n0 >= nt) {                               // (workgroup-uniform)
        if (n < N) o[n] = 0.0;
        return;
    }
    // the axis with the smallest size plays z
    int az = 2;
    if (q[1] < q[az]) az = 1;
    if (q[0] < q[az]) az = 0;
    const int ax = (az + 1) % 3, ay = (az + 2) % 3;
    const double twoLx = 2.0 * q[ax], twoLy = 2.0 * q[ay], twoLz = 2.0 * q[az];
    const double bx0 = q[3 + ax] - q[6 + ax], bx1 = -q[3 + ax] - q[6 + ax];
    const double by0 = q[3 + ay] - q[6 + ay], by1 = -q[3 + ay] - q[6 + ay];
    const double bz0 = q[3 + az] - q[6 + az], bz1 = -q[3 + az] - q[6 + az];
    const double betx0 = q[9 + 2 * ax], betx1 = q[10 + 2 * ax], bety0 = q[9 + 2 * ay], bety1 = q[10 + 2 * ay];
    const double betz0 = q[9 + 2 * az], betz1 = q[10 + 2 * az];
    // the tile's shell
    const double Wd = (double)W, m_per_sample = c / fs, sample_per_m = fs / c;
    const int n1 = min(n0 + RIRS_TILE, nt) - 1;
    const double dhi = (double)(n1 + W) * m_per_sample * (1.0 + RIRS_WIDEN);
    const double dlo = n0 > W ? (double)(n0 - W) * m_per_sample * (1.0 - RIRS_WIDEN) : 0.0;
    const double dhi2 = dhi * dhi, dlo2 = dlo * dlo;
    int lox0, nx0, lox1, nx1, loy0, ny0, loy1, ny1;
    rirs_range(bx0, twoLx, dhi, lox0, nx0);
    rirs_range(bx1, twoLx, dhi, lox1, nx1);
    rirs_range(by0, twoLy, dhi, loy0, ny0);
    rirs_range(by1, twoLy, dhi, loy1, ny1);
    const long long NY = (long long)ny0 + ny1, NP = ((long long)nx0 + nx1) * NY;
    const bool np32 = NP <= 0x7fffffffLL;                    // (uniform) pair indices fit 32 bits: no 64-bit division per pair
    // beta^k: six tables of pow()'s values, worth their 6 pow() per thread only where the tile walks more than a few batches of pairs
    const bool use_tab = NP > 4 * RIRS_PAIRS;                // (uniform)
    const double* tx0 = use_tab ? ptab[0] : nullptr; const double* tx1 = use_tab ? ptab[1] : nullptr;
    const double* ty0 = use_tab ? ptab[2] : nullptr; const double* ty1 = use_tab ? ptab[3] : nullptr;
    const double* tz0 = use_tab ? ptab[4] : nullptr; const double* tz1 = use_tab ? ptab[5] : nullptr;
    if (use_tab) {
        const double kk = (double)tid;                       // RIRS_PTAB == RIRS_TILE: one exponent per thread
        ptab[0][tid] = pow(betx0, kk); ptab[1][tid] = pow(betx1, kk);
        ptab[2][tid] = pow(bety0, kk); ptab[3][tid] = pow(bety1, kk);
        ptab[4][tid] = pow(betz0, kk); ptab[5][tid] = pow(betz1, kk);
    }
    // the tap of this thread
    const bool live = n < nt;
    double p0, pc, ps;
    {
        const double sgn = (n & 1) ? -1.0 : 1.0;
        double sn, cn;
        sincospi((double)(n % (2 * W)) / Wd, &sn, &cn);
        p0 = 0.5 * sgn; pc = sgn * cn; ps = sgn * sn;
    }
    const double nd = (double)n;
    double acc = 0.0;
    const int lane = tid & 63, wv = tid >> 6;
    const int pl = tid >> 2, uz_t = (tid >> 1) & 1, side = tid & 1;
    __syncthreads();                                         // ptab

    for (long long pb = 0; pb < NP; pb += RIRS_PAIRS) {
        // ---- the batch's pairs: the z intervals of each (4 threads per pair: z parity x sign of delta_z)
        int cnt = 0, lo = 0;
        const long long p = pb + pl;
        if (p < NP) {
            const int ix = np32 ? (int)((unsigned)p / (unsigned)NY) : (int)(p / NY), iy = (int)(p - (long long)ix * NY);
            const int ux = ix >= nx0, lx = ux ? lox1 + (ix - nx0) : lox0 + ix;
            const int uy = iy >= ny0, ly = uy ? loy1 + (iy - ny0) : loy0 + iy;
            const double dx = (ux ? bx1 : bx0) + twoLx * (double)lx, dy = (uy ? by1 : by0) + twoLy * (double)ly;
            const double rho2 = dx * dx + dy * dy, zhi2 = dhi2 - rho2;
            if (zhi2 >= 0.0) {
                const double zhi = sqrt(zhi2), zlo2 = dlo2 - rho2, b = uz_t ? bz1 : bz0;
                if (zlo2 <= 0.0) {                           // the disc's inner part: one interval
                    if (side == 0) rirs_range(b, twoLz, zhi, lo, cnt);
                } else {
                    const double zlo = sqrt(zlo2);
                    const int loA = (int)ceil((-zhi - b) / twoLz), hiA = (int)floor((-zlo - b) / twoLz);
                    const int loB = max((int)ceil((zlo - b) / twoLz), hiA + 1), hiB = (int)floor((zhi - b) / twoLz);
                    lo = side ? loB : loA;
                    cnt = max((side ? hiB : hiA) - lo + 1, 0);
                }
                if ((tid & 3) == 0) {
                    u_rho2[pl] = rho2;
                    u_g[pl] = rirs_gain(tx0, tx1, betx0, betx1, ux, lx) * rirs_gain(ty0, ty1, bety0, bety1, uy, ly);
                }
            }
        }
        int v = cnt;                                         // inclusive scan over the workgroup
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int t = __shfl_up(v, s, 64);
            if (lane >= s) v += t;
        }
        if (lane == 63) wave_tot[wv] = v;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wave_tot[w];
        u_off[tid + 1] = before + v;
        u_lo[tid] = lo;
        if (tid == 0) u_off[0] = 0;
        __syncthreads();
        const int total = u_off[RIRS_TILE];

        for (int base = 0; base < total; base += RIRS_CAP) {
            const int cc = min(RIRS_CAP, total - base);
            // ---- the chunk's images, one per thread: everything that is per image
            for (int e = tid; e < cc; e += RIRS_TILE) {
                const int g = base + e;
                int jl = 0, jh = RIRS_TILE;                  // u_off[jl] <= g < u_off[jh]
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int mid = (jl + jh) >> 1;
                    if (u_off[mid] <= g) jl = mid; else jh = mid;
                }
                const int l = u_lo[jl] + (g - u_off[jl]), uz = (jl >> 1) & 1, jp = jl >> 2;
                const double dz = (uz ? bz1 : bz0) + twoLz * (double)l;
                const double d = sqrt(u_rho2[jp] + dz * dz);
                const double A = u_g[jp] * rirs_gain(tz0, tz1, betz0, betz1, uz, l) / (4.0 * M_PI * d);
                const double tau = d * fs / c;
                const double k = rint(tau), f = tau - k;
                const double sp = sinpi(f);
                double sw, cw;
                sincospi(tau / Wd, &sw, &cw);
                e_tau[e] = tau;
                e_A[e] = A;
                e_S[e] = (((long long)k & 1) ? sp : -sp) * A * M_1_PI;
                e_hc[e] = 0.5 * cw;
                e_hs[e] = 0.5 * sw;
            }
            __syncthreads();
            // ---- every tap over the chunk in list order
            if (live) {
                for (int e = 0; e < cc; ++e) {
                    const double x = nd - e_tau[e];
                    if (fabs(x) <= Wd) {
                        if (x == 0.0) {
                            acc += e_A[e];
                        } else {
                            double rc = __builtin_amdgcn_rcp(x);
                            rc = fma(fma(-x, rc, 1.0), rc, rc);
                            rc = fma(fma(-x, rc, 1.0), rc, rc);
                            const double hann = fma(e_hs[e], ps, fma(e_hc[e], pc, p0));
                            acc = fma(e_S[e] * rc, hann, acc);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (n < N) o[n] = live ? acc : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------- host
static int rirs_check_shape(const char* name, int R, int N) {
    NELE_CHECK_ARG(R >= 1 && R <= 65535, "%s: R=%d outside 1 .. 65535", name, R);
    NELE_CHECK_ARG(N >= 1, "%s: N=%d is not positive", name, N);
    return NELE_OK;
}

extern "C" long long nele_rir_synth_workspace_bytes(int R, int N) {
    if (rirs_check_shape("nele_rir_synth_workspace_bytes", R, N)) return -1;
    return 0;
}

extern "C" int nele_rir_synth_tile(void) { return RIRS_TILE; }

extern "C" int nele_rir_synth(const double* rooms, const int* taps, int R, int N, double fs, double c, int half_width, double* out, int* status,
                              void* workspace, void* stream) {
    const char* name = "nele_rir_synth";
    (void)workspace;
    NELE_CHECK_ARG(rooms && taps && out && status, "%s: null rooms, taps, out or status", name);
    if (int st = rirs_check_shape(name, R, N)) return st;
    NELE_CHECK_ARG(half_width >= 1 && half_width <= 4096, "%s: half_width=%d outside 1 .. 4096", name, half_width);
    NELE_CHECK_ARG(std::isfinite(fs) && std::isfinite(c) && fs > 0.0 && c > 0.0, "%s: fs=%g or c=%g is not finite and positive", name, fs, c);
    NELE_CHECK_ARG(((double)N + (double)half_width) * c / fs <= NELE_RIR_MAX_DISTANCE_M, "%s: N=%d taps at fs=%g, c=%g reach beyond %g m", name, N, fs,
                   c, (double)NELE_RIR_MAX_DISTANCE_M);
    const int ntiles = (N + RIRS_TILE - 1) / RIRS_TILE;
    const hipStream_t st = as_stream(stream);
    NELE_PROF("rir_synth", st, hipLaunchKernelGGL(rir_synth_kernel, dim3((unsigned)ntiles, (unsigned)R), dim3(RIRS_TILE), 0, st, rooms, taps, N, ntiles,
                                                  fs, c, half_width, out, status));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
