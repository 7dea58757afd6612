// gs_gbr.hip -- Gaussianised Blackwell-Rao likelihood from the sample bank
// (Rudjord et al. 2009), gfx950.
//
// The bank of gs_brs.hip keeps the scales X of every kept sample; with
// draws it also keeps the D_l draws,
//   Dl [nchains][cap][Jp]   Dl[c][i][j] = the D_l trace ring's value at column
//                           cols[j] of chain c's i-th kept sample, 0 for j >= Ju
// packed by k_gbr_pack with the slot rule and the row index of k_brs_pack (row i
// of Dl belongs to row i of X and r; a row whose r is NaN is skipped here too).
//
// The fit works on the Jg inverse-Gamma columns of the bank (gcol [Jg]: their
// positions in [0, Ju); alpha [Jg] the shape; half [Jg] = 0.5 where the recorded
// scale is the diagonal of the TEB block's Psi, else 1: beta = half X), each with
// a grid of G nodes uniform in log D,
//   lD_g = fma(g, h, lo),  g = 0 .. G - 1,  8 <= G <= 256.
// The caller puts node 1 at log(a min D) and node G - 2 at log(b max D): the
// usable interval is [lD_1, lD_{G-2}], u = (log D - lo) / h in [1, G - 2]; the end
// nodes 0 and G - 1, where a one-sided cumulative is 0 and x is infinite, lie
// outside it and are never read by the interpolation.
//
// k_gbr_marg, one workgroup per (column, chain), thread g: with t = fma(-beta,
// exp(-lD_g), alpha log beta) the online rule of gs_br.hip over the chain's rows
// in row order (beta and log beta of 256 rows staged in LDS at a time),
//   S == 0:  m = t, S = 1
//   else     d = t - m, w = exp(-|d|);  d > 0: S = fma(S, w, 1), m = t;  else S = S + w
// into m, S [nchains][Jg][G]; cnt [nchains] counts the rows whose r is not NaN.
// A chain's partial depends on that chain's rows alone.  k_gbr_marg_finish, one
// thread per (column, g), merges the chains in chain order with the rule of
// gs_brs.hip (M = max, S = S1 exp(m1 - M) + S2 exp(m2 - M), an empty side the
// identity) and writes, every step one rounded operation, N = sum_c cnt_c,
//   logp = (((M + log S) - log N) - lgamma(alpha)) - (alpha + 1) lD_g.
//
// k_gbr_tables, one thread per column, every sum in g order: with q_g = exp((logp_g
// + lD_g) - mx), mx the column's largest logp_g + lD_g,
//   FL_0 = 0, FL_g = FL_{g-1} + (0.5 (q_{g-1} + q_g)) h      (from the left)
//   FR_{G-1} = 0, FR_g = FR_{g+1} + (0.5 (q_g + q_{g+1})) h  (from the right)
//   ms = FL_{G-1},  mass = exp(mx) ms          (reported, never enforced)
//   x_g = FL_g / ms <= 1/2 ? normcdfinv(FL_g / ms) : -normcdfinv(FR_g / ms)
//   sx_g = h exp((((lD_g + logp_g) - (mx + log ms)) + x_g^2 / 2) + log(2 pi) / 2)
// (the slope dx / du formed in logs: the tails do not underflow), and the slope
// of logp by differences, sp_g = (logp_{g+1} - logp_{g-1}) / 2 (one-sided at the
// ends).  Tables tx [Jg][G][2] = (x, sx) and tp [Jg][G][2] = (logp, sp).
//
// The transform T_j(D): u = (log D - lo) (1 / h), k = int(u) clamped to [1, G - 3],
// t = u - k, the cubic Hermite through nodes k and k + 1,
//   h00 = (1 + 2 t)(1 - t)^2, h10 = t (1 - t)^2, h01 = t^2 (3 - 2 t), h11 = t^2 (t - 1)
//   T = fma(h00, y_k, fma(h10, s_k, fma(h01, y_{k+1}, h11 s_{k+1})));
// D is outside when not (1 <= u <= G - 2) (a NaN or non-positive D included), and
// when x at node k or k + 1 is not finite: the cumulatives are linear sums, so for
// a marginal much narrower than the grid (alpha of thousands) they underflow in
// the far tails and the usable interval shrinks to the nodes with a finite x.
//
// k_gbr_moments (the hot path), one workgroup (4 waves) per (chain, row block,
// pair ta <= tb of tiles of HC = 64 columns).  The block is walked in passes of
// PR = 64 rows: thread (column sc = tid & 63, rows tid >> 6 + 4 e) reads Dl of the
// columns of ta (and of tb) and writes x = T_j(Dl) to s_keep [64 rows][128] (row
// stride KS = 144 doubles; ta's columns at 0, tb's at 64; a row whose r is NaN, a
// row >= n and a column >= Jg are kept as zeros) -- x never goes to memory.  The
// contraction is that of k_brh_gram: rows 4 per v_mfma_f64_16x16x4_f64, ascending;
// A = 16 columns of ta x 4 rows (lane l: column l & 15, row l >> 4), B = 4 rows x
// 16 columns of tb (lane l: row l >> 4, column l & 15), D column-of-ta (l >> 4) + 4
// reg, column-of-tb l & 15; wave w owns columns 16 w .. 16 w + 15 of ta against
// all 64 of tb: 4 accumulators (16 doubles) per lane, carried over the passes of
// the block.  Both operands come from s_keep, 2 rows x 16 columns per ds_read_b64
// half (dword 288 row + 2 column, 288 = 32 mod 64: conflict-free).  A pair ta ==
// tb skips the 16 x 16 tiles below the diagonal, and its threads 0 .. 63 add their
// column of s_keep in row order into S1.  The row blocks are a function of (n,
// Jg) alone (gs_gbr_info); a workgroup writes D[a][b], a <= b, to work [chain]
// [block][Jq][Jq] at [a][b] and [b][a] (Jq = Jg rounded up to 4).  k_gbr_combine
// adds a chain's blocks in block order from 0.0 into S1 [nchains][Jg] and S2
// [nchains][Jg][Jg]: S2 is exactly symmetric, there are no float atomics, and for
// given (n, Jg, tables) a chain's sums depend on that chain's rows alone.
//
// k_gbr_eval, one thread per (model, column): x and logp of a theory's D through
// the same Hermite code; out = 1, x = logp = 0 where D is outside.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string>

#include "gibbs_capi.h"
#include "gs_common.h"
#include "gs_launch.h"

using gs_detail::set_error;

namespace {

constexpr int BS = 256;       // threads per workgroup
constexpr int PR = 64;        // rows per pass
constexpr int HC = 64;        // columns per tile
constexpr int NB = HC / 16;   // 16-column MFMA tiles of tb (a wave owns one of ta)
constexpr int KS = 2 * HC + 16;    // row stride of the kept tiles (doubles)
constexpr int RT = 256;       // rows per staged tile of the marginals
constexpr int GMIN = 8, GMAX = 256;
constexpr int BLK_MIN = 256;  // rows a row block holds at least (but for the last)
constexpr int WG_AIM = 32;    // (row block, tile pair) workgroups per chain aimed at
static_assert(PR == 16 * (BS / 64) && HC == 16 * (BS / 64) && KS % 32 == 16 && HC == 64, "tile shapes");

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }

__global__ __launch_bounds__(BS) void k_gbr_pack(double* __restrict__ Dl, int nchains, int cap, int Jp, int Ju, int nsb,
                                                 const int* __restrict__ cols, const double* __restrict__ trace,
                                                 int capacity, int slot0, int row0) {
    const int i = blockIdx.x / nchains, chain = blockIdx.x % nchains;
    int slot = slot0 + i;
    if (slot >= capacity) slot -= capacity;                    // slot0 < capacity and nsteps <= capacity: one wrap
    const double* rowp = trace + ((long long)slot * nchains + chain) * nsb;
    double* out = Dl + ((long long)chain * cap + row0 + i) * Jp;
    for (int j = threadIdx.x; j < Jp; j += BS) {
        double v = 0.0;
        if (j < Ju) {
            const int col = cols[j];
            if (col >= 0 && col < nsb) v = rowp[col];
        }
        out[j] = v;
    }
}

// grid (Jg, nchains), blockDim = G rounded up to a multiple of 64
__global__ __launch_bounds__(BS) void k_gbr_marg(const double* __restrict__ X, const double* __restrict__ r, int cap, int n,
                                                 int Jp, int Jg, const int* __restrict__ gcol,
                                                 const double* __restrict__ alpha, const double* __restrict__ half,
                                                 const double* __restrict__ glo, const double* __restrict__ gh, int G,
                                                 double* __restrict__ om, double* __restrict__ oS,
                                                 long long* __restrict__ cnt) {
    __shared__ double s_b[RT];
    __shared__ double s_lb[RT];
    __shared__ unsigned long long s_cnt;
    const int t = threadIdx.x, nt = blockDim.x;
    const int j = blockIdx.x, chain = blockIdx.y;
    const double a = alpha[j], fac = half[j];
    const int col = gcol[j];
    const bool active = t < G;
    const double rD = active ? exp(-fma((double)t, gh[j], glo[j])) : 0.0;
    const double* Xc = X + (long long)chain * cap * Jp + col;
    const double* rc = r + (long long)chain * cap;
    if (t == 0) s_cnt = 0ULL;
    unsigned long long good = 0ULL;
    double m = 0.0, S = 0.0;
    for (int t0 = 0; t0 < n; t0 += RT) {
        const int tn = n - t0 < RT ? n - t0 : RT;
        __syncthreads();                                       // the previous tile has been read
        for (int q = t; q < tn; q += nt) {
            const double rv = rc[t0 + q];
            const double b = Xc[(long long)(t0 + q) * Jp] * fac;
            const bool live = rv == rv;
            if (live) ++good;
            s_b[q] = b;
            s_lb[q] = (live && pos_finite(b)) ? log(b) : qnan();
        }
        __syncthreads();
        if (active) {
            for (int q = 0; q < tn; ++q) {
                const double lb = s_lb[q];
                if (lb == lb) {
                    const double tv = fma(-s_b[q], rD, a * lb);
                    if (S == 0.0) {
                        m = tv;
                        S = 1.0;
                    } else {
                        const double d = tv - m;
                        const double w = exp(-fabs(d));
                        if (d > 0.0) {
                            S = fma(S, w, 1.0);
                            m = tv;
                        } else {
                            S = S + w;
                        }
                    }
                }
            }
        }
    }
    if (active) {
        const long long e = ((long long)chain * Jg + j) * G + t;
        om[e] = m;
        oS[e] = S;
    }
    if (j == 0) {                                              // integer count: the order does not matter
        if (good) atomicAdd(&s_cnt, good);
        __syncthreads();
        if (t == 0) cnt[chain] = (long long)s_cnt;
    }
}

__global__ __launch_bounds__(BS) void k_gbr_marg_finish(const double* __restrict__ fm, const double* __restrict__ fS,
                                                        const long long* __restrict__ cnt, int C, int Jg, int G,
                                                        const double* __restrict__ alpha, const double* __restrict__ glo,
                                                        const double* __restrict__ gh, double* __restrict__ logp) {
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    const long long ne = (long long)Jg * G;
    if (e >= ne) return;
    const int j = (int)(e / G), g = (int)(e - (long long)j * G);
    long long N = 0;
    for (int c = 0; c < C; ++c) N += cnt[c];
    double M = 0.0, S = 0.0;
    for (int c = 0; c < C; ++c) {
        const double m2 = fm[c * ne + e], S2 = fS[c * ne + e];
        if (S2 == 0.0) continue;
        if (S == 0.0) {
            M = m2;
            S = S2;
            continue;
        }
        const double mx = fmax(M, m2);
        const double e1 = exp(sub(M, mx)), e2 = exp(sub(m2, mx));
        S = add(mul(S, e1), mul(S2, e2));
        M = mx;
    }
    double out = qnan();
    if (N > 0 && S > 0.0) {
        const double a = alpha[j];
        const double lD = fma((double)g, gh[j], glo[j]);
        out = sub(sub(sub(add(M, log(S)), log((double)N)), lgamma(a)), mul(add(a, 1.0), lD));
    }
    logp[e] = out;
}

__global__ __launch_bounds__(BS) void k_gbr_tables(const double* __restrict__ logp, int Jg, int G,
                                                   const double* __restrict__ glo, const double* __restrict__ gh,
                                                   double* __restrict__ tx, double* __restrict__ tp,
                                                   double* __restrict__ mass) {
    const int j = blockIdx.x * BS + threadIdx.x;
    if (j >= Jg) return;
    const double lo = glo[j], h = gh[j];
    const double* lp = logp + (long long)j * G;
    double* ox = tx + (long long)j * G * 2;
    double* op = tp + (long long)j * G * 2;
    double mx = add(lp[0], lo);
    for (int g = 1; g < G; ++g) mx = fmax(mx, add(lp[g], fma((double)g, h, lo)));
    // from the left: FL_g is parked in ox[2 g]
    double acc = 0.0;
    double q0 = exp(sub(add(lp[0], lo), mx));
    ox[0] = 0.0;
    for (int g = 1; g < G; ++g) {
        const double q1 = exp(sub(add(lp[g], fma((double)g, h, lo)), mx));
        acc = add(acc, mul(mul(0.5, add(q0, q1)), h));
        ox[2 * g] = acc;
        q0 = q1;
    }
    const double ms = acc;
    const double lms = add(mx, log(ms));
    mass[j] = mul(exp(mx), ms);
    const double hl2pi = 0.91893853320467274178;               // log(2 pi) / 2
    // from the right
    acc = 0.0;
    double q1 = 0.0;
    for (int g = G - 1; g >= 0; --g) {
        const double lD = fma((double)g, h, lo);
        const double q = exp(sub(add(lp[g], lD), mx));
        if (g < G - 1) acc = add(acc, mul(mul(0.5, add(q, q1)), h));
        q1 = q;
        const double fl = ox[2 * g] / ms, fr = acc / ms;
        const double x = fl <= 0.5 ? normcdfinv(fl) : -normcdfinv(fr);
        const double ls = add(add(sub(add(lD, lp[g]), lms), mul(0.5, mul(x, x))), hl2pi);
        const bool fin = fabs(x) < __longlong_as_double(0x7ff0000000000000LL);
        ox[2 * g] = x;
        ox[2 * g + 1] = fin ? mul(h, exp(ls)) : 0.0;
    }
    for (int g = 0; g < G; ++g) {
        const int gl = g > 0 ? g - 1 : 0, gr = g < G - 1 ? g + 1 : G - 1;
        op[2 * g] = lp[g];
        op[2 * g + 1] = sub(lp[gr], lp[gl]) / (double)(gr - gl);
    }
}

// u of log D on a column's grid: the cell k in [1, G - 3] and t = u - k; false when D is outside
__device__ __forceinline__ bool locate(double D, double lo, double rh, int G, int& k, double& t) {
    const double u = pos_finite(D) ? mul(sub(log(D), lo), rh) : qnan();
    const bool in = u >= 1.0 && u <= (double)(G - 2);
    int kk = in ? (int)u : 1;
    kk = kk > G - 3 ? G - 3 : kk;
    k = kk;
    t = in ? sub(u, (double)kk) : 0.0;
    return in;
}

// a cell whose nodes' x are not both finite (the cumulative of a very narrow marginal
// underflows in the tails) is not usable: D there is outside
__device__ __forceinline__ bool cell_ok(const double* p) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    return fabs(p[0]) < inf && fabs(p[2]) < inf;
}

// the cubic Hermite through (y0, s0) at t = 0 and (y1, s1) at t = 1
__device__ __forceinline__ double hermite(double y0, double s0, double y1, double s1, double t) {
    const double omt = sub(1.0, t);
    const double o2 = mul(omt, omt), t2 = mul(t, t);
    const double h00 = mul(fma(2.0, t, 1.0), o2), h10 = mul(t, o2);
    const double h01 = mul(t2, fma(-2.0, t, 3.0)), h11 = mul(t2, sub(t, 1.0));
    return fma(h00, y0, fma(h10, s0, fma(h01, y1, mul(h11, s1))));
}

__global__ __launch_bounds__(BS) void k_gbr_moments(const double* __restrict__ Dl, const double* __restrict__ r, int cap,
                                                    int n, int Jp, int Jg, int Jq, const int* __restrict__ gcol,
                                                    const double* __restrict__ tx, const double* __restrict__ glo,
                                                    const double* __restrict__ gh, int G, double* __restrict__ part2,
                                                    double* __restrict__ part1, int nblk, int RB, int nct) {
    __shared__ __attribute__((aligned(16))) double s_keep[PR * KS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, kq = lane >> 4;
    const int npair = nct * (nct + 1) / 2;
    int bi = blockIdx.x;
    int pr = bi % npair; bi /= npair;
    const int blk = bi % nblk, chain = bi / nblk;
    int ta = 0;
    while (pr >= nct - ta) { pr -= nct - ta; ++ta; }           // pairs (ta, ta), (ta, ta + 1), ... in order
    const int tb = ta + pr;
    const bool diag = ta == tb;
    const int a0 = ta * HC, b0 = tb * HC;
    const int bo = diag ? 0 : HC;                              // tb's columns within s_keep
    const int row_s = blk * RB;
    const int nrows = n - row_s < RB ? n - row_s : RB;          // > 0: nblk = ceil(n / RB)
    const int ca0 = a0 + 16 * wave;                             // the wave's first column of ta
    const int hn = (Jq - b0 + 15) / 16 < NB ? (Jq - b0 + 15) / 16 : NB;   // 16-column tiles of tb that hold a column
    const int h0 = diag ? wave : 0;                            // the first of them this wave computes
    const bool gram = ca0 < Jq;
    const double* Dc = Dl + (long long)chain * cap * Jp;
    const double* rc = r + (long long)chain * cap;
    const int npass = (nrows + PR - 1) / PR;
    const int sc = tid & (HC - 1), sr = tid >> 6;

    // the thread's column of ta and of tb: its bank column and its grid
    const int ja = a0 + sc, jb = b0 + sc;
    const bool hasa = ja < Jg, hasb = !diag && jb < Jg;
    const int cola = hasa ? gcol[ja] : 0, colb = hasb ? gcol[jb] : 0;
    const double loa = hasa ? glo[ja] : 0.0, rha = hasa ? 1.0 / gh[ja] : 0.0;
    const double lob = hasb ? glo[jb] : 0.0, rhb = hasb ? 1.0 / gh[jb] : 0.0;
    const double* txa = tx + (long long)(hasa ? ja : 0) * G * 2;
    const double* txb = tx + (long long)(hasb ? jb : 0) * G * 2;

    f64x4 nacc[NB];
#pragma unroll
    for (int h = 0; h < NB; ++h) nacc[h] = f64x4{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0;

    for (int pass = 0; pass < npass; ++pass) {
#pragma unroll 4
        for (int e = 0; e < PR / 4; ++e) {
            const int row = sr + 4 * e;
            const int lr = pass * PR + row;                    // row within the block
            const double rv = lr < nrows ? rc[row_s + lr] : qnan();
            const bool live = rv == rv;
            double xa = 0.0, xb = 0.0;
            if (live && hasa) {
                int k;
                double t;
                const bool in = locate(Dc[(long long)(row_s + lr) * Jp + cola], loa, rha, G, k, t);
                const double* p = txa + 2 * k;
                xa = (in && cell_ok(p)) ? hermite(p[0], p[1], p[2], p[3], t) : qnan();
            }
            if (live && hasb) {
                int k;
                double t;
                const bool in = locate(Dc[(long long)(row_s + lr) * Jp + colb], lob, rhb, G, k, t);
                const double* p = txb + 2 * k;
                xb = (in && cell_ok(p)) ? hermite(p[0], p[1], p[2], p[3], t) : qnan();
            }
            s_keep[row * KS + sc] = xa;
            if (!diag) s_keep[row * KS + HC + sc] = xb;
        }
        __syncthreads();
        if (diag && tid < HC) {
            const double* kp = s_keep + tid;
            for (int row = 0; row < PR; ++row) s1 = add(s1, kp[row * KS]);
        }
        const int prow = nrows - pass * PR;                     // rows of this pass (the rest hold x = 0)
        const int nks = ((prow < PR ? prow : PR) + 3) / 4;
        if (gram) {
            const double* xp = s_keep + kq * KS + rl;
            for (int ks = 0; ks < nks; ++ks) {
                const double xa = xp[4 * ks * KS + 16 * wave];
                double xb[NB];
#pragma unroll
                for (int h = 0; h < NB; ++h) xb[h] = xp[4 * ks * KS + bo + 16 * h];
#pragma unroll
                for (int h = 0; h < NB; ++h)
                    if (h >= h0 && h < hn) nacc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb[h], nacc[h], 0, 0, 0);
            }
        }
        __syncthreads();                                       // the kept tiles have been read
    }
    if (diag && tid < HC && ja < Jq) part1[((long long)chain * nblk + blk) * Jq + ja] = s1;
    if (!gram) return;
    double* po = part2 + ((long long)chain * nblk + blk) * Jq * Jq;
#pragma unroll
    for (int h = 0; h < NB; ++h)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int a = ca0 + kq + 4 * g, b = b0 + 16 * h + rl;
            if (h >= h0 && h < hn && a < Jq && b < Jq && a <= b) {
                const double v = nacc[h][g];
                po[(long long)a * Jq + b] = v;
                po[(long long)b * Jq + a] = v;
            }
        }
}

// one thread per (chain, a, b) of S2, then per (chain, a) of S1: the blocks in block order
__global__ __launch_bounds__(BS) void k_gbr_combine(const double* __restrict__ part2, const double* __restrict__ part1,
                                                    int Jg, int Jq, int nblk, long long total2, long long total,
                                                    double* __restrict__ S2, double* __restrict__ S1) {
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    if (e >= total) return;
    double v = 0.0;
    if (e < total2) {
        const long long jj = (long long)Jg * Jg;
        const long long chain = e / jj, o = e - chain * jj;
        const long long a = o / Jg, b = o - a * Jg;
        for (int q = 0; q < nblk; ++q) v = add(v, part2[((chain * nblk + q) * Jq + a) * Jq + b]);
        S2[e] = v;
    } else {
        const long long f = e - total2;
        const long long chain = f / Jg, a = f - chain * Jg;
        for (int q = 0; q < nblk; ++q) v = add(v, part1[(chain * nblk + q) * Jq + a]);
        S1[f] = v;
    }
}

__global__ __launch_bounds__(BS) void k_gbr_eval(const double* __restrict__ theory, long long total, int nsb, int Jg,
                                                 const int* __restrict__ tcol, const double* __restrict__ tx,
                                                 const double* __restrict__ tp, const double* __restrict__ glo,
                                                 const double* __restrict__ gh, int G, double* __restrict__ xo,
                                                 double* __restrict__ lpo, int* __restrict__ out) {
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    if (e >= total) return;
    const long long km = e / Jg;
    const int j = (int)(e - km * Jg);
    int k;
    double t;
    bool in = locate(theory[km * nsb + tcol[j]], glo[j], 1.0 / gh[j], G, k, t);
    const double* p = tx + ((long long)j * G + k) * 2;
    in = in && cell_ok(p);
    double x = 0.0, lp = 0.0;
    if (in) {
        const double* q = tp + ((long long)j * G + k) * 2;
        x = hermite(p[0], p[1], p[2], p[3], t);
        lp = hermite(q[0], q[1], q[2], q[3], t);
    }
    xo[e] = x;
    lpo[e] = lp;
    out[e] = in ? 0 : 1;
}

// the row blocks of the moments pass: a function of (n, Jg) alone
void blocks_of(int n, int Jg, int* nblk, int* RB, int* nct) {
    const int Jq = (Jg + 3) / 4 * 4;
    const int nc = (Jq + HC - 1) / HC;
    const int npair = nc * (nc + 1) / 2;
    const int aim = WG_AIM / npair > 1 ? WG_AIM / npair : 1;
    int nb = (n + BLK_MIN - 1) / BLK_MIN;
    nb = nb < 1 ? 1 : (nb > aim ? aim : nb);
    const int rb = ((n > 0 ? (n + nb - 1) / nb : 1) + PR - 1) / PR * PR;
    *RB = rb;
    *nblk = n > 0 ? (n + rb - 1) / rb : 1;
    *nct = nc;
}

int check_fit(const char* what, long long nchains, long long cap, int n, int Ju, int Jg, int G) {
    if (nchains < 1 || nchains > 65535) return set_error(std::string(what) + ": nchains in [1, 65535] needed");
    if (cap < 1) return set_error(std::string(what) + ": bank capacity cap >= 1 needed");
    if (nchains * cap > 0x7fffffffLL) return set_error(std::string(what) + ": too many bank rows (nchains * cap)");
    if (n < 1 || n > cap) return set_error(std::string(what) + ": rows n must lie in [1, cap]");
    if (Ju < 1 || Jg < 1 || Jg > Ju) return set_error(std::string(what) + ": columns 1 <= Jg <= Ju needed");
    if (Jg > 32768) return set_error(std::string(what) + ": more than 32768 Gaussianised columns");
    if (G < GMIN || G > GMAX) return set_error(std::string(what) + ": grid points G out of range [8, 256]");
    return 0;
}

}  // namespace

extern "C" {

int gs_gbr_info(int n, int Jg, int* nblk, int* block_rows, int* column_tile) {
    if (!nblk || !block_rows || !column_tile) return set_error("gs_gbr_info: null argument");
    if (n < 0 || Jg < 1) return set_error("gs_gbr_info: n >= 0 and Jg >= 1 needed");
    int nct;
    blocks_of(n, Jg, nblk, block_rows, &nct);
    *column_tile = HC;
    return 0;
}

int gs_gbr_append(double* Dl, int nchains, int cap, int Ju, int nspec, int maxbins, const int* cols,
                  const double* trace, int capacity, uint32_t first_iteration, int nsteps, int row0, void* stream) {
    if (!Dl) return set_error("gs_gbr_append: null bank");
    if (nchains < 1 || cap < 1 || Ju < 1) return set_error("gs_gbr_append: nchains, cap and Ju >= 1 needed");
    if ((long long)nchains * cap > 0x7fffffffLL) return set_error("gs_gbr_append: too many bank rows (nchains * cap)");
    if (nspec < 1 || nspec > 32 || maxbins < 1)
        return set_error("gs_gbr_append: maxbins >= 1 and nspec in [1, 32] out of range");
    if ((long long)nchains * nspec * maxbins > (1LL << 28)) return set_error("gs_gbr_append: too many series");
    if (Ju > nspec * maxbins) return set_error("gs_gbr_append: used columns Ju out of range [1, nspec * maxbins]");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_gbr_append: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    if (row0 < 0 || (long long)row0 + nsteps > cap)
        return set_error("gs_gbr_append: rows row0 .. row0 + nsteps - 1 must lie in the bank (row0 + nsteps <= cap)");
    if (nsteps == 0) return 0;
    if (!cols || !trace) return set_error("gs_gbr_append: null columns or D_l trace");
    const long long nb = (long long)nsteps * nchains;
    if (nb > 0x7fffffffLL) return set_error("gs_gbr_append: too many (row, chain) workgroups for one launch");
    const int Jp = (Ju + 3) / 4 * 4;
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    hipLaunchKernelGGL(k_gbr_pack, dim3((unsigned)nb), dim3(BS), 0, (hipStream_t)stream, Dl, nchains, cap, Jp, Ju,
                       nspec * maxbins, cols, trace, capacity, slot0, row0);
    GS_LAUNCH_CHECK("k_gbr_pack");
    return 0;
}

int gs_gbr_marginals(const double* X, const double* r, int nchains, int cap, int n, int Ju, int Jg, const int* gcol,
                     const double* alpha, const double* half, const double* glo, const double* gh, int G, double* m,
                     double* S, long long* cnt, void* stream) {
    if (!X || !r) return set_error("gs_gbr_marginals: null bank");
    if (check_fit("gs_gbr_marginals", nchains, cap, n, Ju, Jg, G)) return -1;
    if (!gcol || !alpha || !half || !glo || !gh || !m || !S || !cnt)
        return set_error("gs_gbr_marginals: null table or output");
    const int Jp = (Ju + 3) / 4 * 4;
    hipLaunchKernelGGL(k_gbr_marg, dim3((unsigned)Jg, (unsigned)nchains), dim3((unsigned)((G + 63) / 64 * 64)), 0,
                       (hipStream_t)stream, X, r, cap, n, Jp, Jg, gcol, alpha, half, glo, gh, G, m, S, cnt);
    GS_LAUNCH_CHECK("k_gbr_marg");
    return 0;
}

int gs_gbr_marginals_finish(const double* m, const double* S, const long long* cnt, int C, int Jg, int G,
                            const double* alpha, const double* glo, const double* gh, double* logp, void* stream) {
    if (!m || !S || !cnt || !alpha || !glo || !gh || !logp) return set_error("gs_gbr_marginals_finish: null argument");
    if (C < 1 || Jg < 1 || Jg > 32768) return set_error("gs_gbr_marginals_finish: C >= 1 and Jg in [1, 32768] needed");
    if (G < GMIN || G > GMAX) return set_error("gs_gbr_marginals_finish: grid points G out of range [8, 256]");
    if ((long long)C * Jg * G > (1LL << 36)) return set_error("gs_gbr_marginals_finish: too many partials");
    const long long ne = (long long)Jg * G;
    hipLaunchKernelGGL(k_gbr_marg_finish, dim3((unsigned)((ne + BS - 1) / BS)), dim3(BS), 0, (hipStream_t)stream, m, S,
                       cnt, C, Jg, G, alpha, glo, gh, logp);
    GS_LAUNCH_CHECK("k_gbr_marg_finish");
    return 0;
}

int gs_gbr_tables(const double* logp, int Jg, int G, const double* glo, const double* gh, double* tx, double* tp,
                  double* mass, void* stream) {
    if (!logp || !glo || !gh || !tx || !tp || !mass) return set_error("gs_gbr_tables: null argument");
    if (Jg < 1 || Jg > 32768) return set_error("gs_gbr_tables: Jg in [1, 32768] needed");
    if (G < GMIN || G > GMAX) return set_error("gs_gbr_tables: grid points G out of range [8, 256]");
    hipLaunchKernelGGL(k_gbr_tables, dim3((unsigned)((Jg + BS - 1) / BS)), dim3(BS), 0, (hipStream_t)stream, logp, Jg, G,
                       glo, gh, tx, tp, mass);
    GS_LAUNCH_CHECK("k_gbr_tables");
    return 0;
}

int gs_gbr_moments_work_bytes(int nchains, int n, int Jg, long long* bytes) {
    if (!bytes) return set_error("gs_gbr_moments_work_bytes: null argument");
    if (nchains < 1 || nchains > 65535 || n < 0 || Jg < 1 || Jg > 32768)
        return set_error("gs_gbr_moments_work_bytes: nchains in [1, 65535], n >= 0 and Jg in [1, 32768] needed");
    int nblk, RB, nct;
    blocks_of(n, Jg, &nblk, &RB, &nct);
    const long long Jq = (Jg + 3LL) / 4 * 4;
    *bytes = 8LL * nchains * nblk * (Jq * Jq + Jq);             // nblk <= 32: below 2^63
    return 0;
}

int gs_gbr_moments(const double* Dl, const double* r, int nchains, int cap, int n, int Ju, int Jg, const int* gcol,
                   const double* tx, const double* glo, const double* gh, int G, void* work, long long work_bytes,
                   double* S1, double* S2, void* stream) {
    if (!Dl || !r) return set_error("gs_gbr_moments: null bank");
    if (check_fit("gs_gbr_moments", nchains, cap, n, Ju, Jg, G)) return -1;
    if (!gcol || !tx || !glo || !gh || !work || !S1 || !S2) return set_error("gs_gbr_moments: null table, workspace or output");
    long long need = 0;
    if (gs_gbr_moments_work_bytes(nchains, n, Jg, &need)) return -1;
    if (work_bytes < need) return set_error("gs_gbr_moments: the workspace is smaller than gs_gbr_moments_work_bytes");
    int nblk, RB, nct;
    blocks_of(n, Jg, &nblk, &RB, &nct);
    const int Jp = (Ju + 3) / 4 * 4, Jq = (Jg + 3) / 4 * 4;
    const long long nb = (long long)nchains * nblk * (nct * (nct + 1LL) / 2);
    if (nb > 0x7fffffffLL) return set_error("gs_gbr_moments: too many (chain, block, tile pair) workgroups");
    double* part2 = (double*)work;
    double* part1 = part2 + (long long)nchains * nblk * Jq * Jq;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gbr_moments, dim3((unsigned)nb), dim3(BS), 0, st, Dl, r, cap, n, Jp, Jg, Jq, gcol, tx, glo, gh,
                       G, part2, part1, nblk, RB, nct);
    GS_LAUNCH_CHECK("k_gbr_moments");
    const long long total2 = (long long)nchains * Jg * Jg, total = total2 + (long long)nchains * Jg;
    hipLaunchKernelGGL(k_gbr_combine, dim3((unsigned)((total + BS - 1) / BS)), dim3(BS), 0, st, (const double*)part2,
                       (const double*)part1, Jg, Jq, nblk, total2, total, S2, S1);
    GS_LAUNCH_CHECK("k_gbr_combine");
    return 0;
}

int gs_gbr_eval(const double* theory, int K, int nspec, int maxbins, int Jg, const int* tcol, const double* tx,
                const double* tp, const double* glo, const double* gh, int G, double* x, double* logp, int* outside,
                void* stream) {
    if (!theory || !tcol || !tx || !tp || !glo || !gh || !x || !logp || !outside)
        return set_error("gs_gbr_eval: null argument");
    if (K < 1 || nspec < 1 || nspec > 32 || maxbins < 1) return set_error("gs_gbr_eval: K, maxbins >= 1 and nspec in [1, 32] needed");
    if (Jg < 1 || Jg > nspec * maxbins) return set_error("gs_gbr_eval: columns Jg out of range [1, nspec * maxbins]");
    if (G < GMIN || G > GMAX) return set_error("gs_gbr_eval: grid points G out of range [8, 256]");
    const long long total = (long long)K * Jg;
    if (total > (1LL << 36)) return set_error("gs_gbr_eval: too many (model, column) pairs");
    hipLaunchKernelGGL(k_gbr_eval, dim3((unsigned)((total + BS - 1) / BS)), dim3(BS), 0, (hipStream_t)stream, theory,
                       total, nspec * maxbins, Jg, tcol, tx, tp, glo, gh, G, x, logp, outside);
    GS_LAUNCH_CHECK("k_gbr_eval");
    return 0;
}

}  // extern "C"
