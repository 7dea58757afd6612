// gs_brl.hip -- streaming Blackwell-Rao likelihood of theory spectra (gfx950).
//
// The Blackwell-Rao estimate of the likelihood of a theory spectrum D^th
// (Chu et al. 2005) averages the joint density of the centered conditional
// over the sky samples of all chains,
//   L(D^th | d) ~ 1/(C n) sum_{c,i} prod_b P(D^th_b | s_{c,i}),
// where P is the inverse-Gamma density of an independent spectrum and the 2x2
// inverse-Wishart density of the TEB block (TT, EE, TE).  Both are linear in
// the scale the C_l draw records in the scale ring (gs_cls_scale_trace) once
// the theory is fixed, so for K theory spectra the log density of sample
// (iteration i, chain c) under model k is, up to a constant cst_k of the model,
//   t_{i,c,k} = r_{i,c} - sum_j x_{i,c,j} Y_{k,j}
//   r_{i,c}   = sum_j coef_j log(arg_j)             (model-independent)
// with j over the Ju *used* columns of the ring row (column = spectrum *
// maxbins + bin, nsb = nspec * maxbins columns per row), x_j the ring value of
// column cols[j], and per used column (tables of engine.br_likelihood_tables):
//   kind 1  an inverse-Gamma bin: arg = x = beta, coef = alpha_b = n_b / 2 - 1,
//           Y = 1 / D
//   kind 2  the TT column of a TEB block, Psi = [[a, c], [c, dd]] with a = x,
//           dd and c its partners at column + maxbins and column + 3 maxbins:
//           arg = fma(a, dd, -(c * c)), coef = nu_b / 2, Y = EE / (2 det D)
//   kind 0  the EE and TE columns of a used block: no logarithm,
//           Y = TT / (2 det D) and -TE / det D
// Unused columns of the ring are never read.
//
// State (caller-owned device buffer of gs_brl_bytes bytes, fp64):
//   header   8 doubles: [0] int64 n, the iterations added; [1] uint32 launch
//            ticket; the rest reserved (0)
//   m, S, Q  [nchains][K] each: the running maximum of t, S = sum_i exp(t_i - m)
//            and Q = sum_i exp(2 (t_i - m));  S == 0: no sample yet
//   bad      int64 [nchains]: rows skipped for the chain
// gs_brl_reset zeroes all of it.
//
// k_brl_update.  One workgroup (256 threads) owns one chain, a tile of TK =
// 128 models and every row of the launch, in tiles of TR = 32 rows.  Per row
// tile it walks the used columns in chunks of JC = 16: x [rows][chunk] and Y
// [models][chunk] go through LDS (the next chunk's global loads are issued
// before the current chunk's FMAs and stored after them), and every thread
// keeps a 4 x 4 block of dot products (rows 4 (t / 32) + p, models t % 32 +
// 32 q) in registers -- 16 independent fma chains.  Order of operations:
//   lg_j = log(arg_j)      once per (row, chain, column) of a workgroup, while
//                          the chunk is staged; a row is *bad* for the chain
//                          when a kind 1 column has x <= 0 or not finite, or a
//                          kind 2 column has arg <= 0 or not finite
//   r    = fma(coef_j, lg_j, r)   over the columns with kind != 0, j ascending, from 0.0
//   dot  = fma(x_j, Y_kj, dot)    over j = 0 .. Ju - 1 ascending, from 0.0: ONE
//                                 chain per (row, model), never split
//   t    = r - dot
// and then, per model in iteration order (bad rows are skipped and counted in
// bad[chain], once per row):
//   S == 0:  m = t, S = 1, Q = 1
//   else     d = t - m,  w = exp(-|d|)
//            d > 0:  S = fma(S, w, 1), Q = fma(Q, w * w, 1), m = t     (w * w rounded once)
//            else    S = S + w,        Q = fma(w, w, Q)
// (m, S, Q) stay in registers across the row tiles: the state is read and
// written once per launch.  Neither the row tiling, the chunking, the model
// tile nor the chain count enters the order, so the state's bits depend only
// on the rows and their iteration order.  The last workgroup's ticket
// advances n, as in k_br_update.
//
// k_brl_finish, one thread per model over C chains in chain order; chains with
// S_c == 0 are left out; n is the header's count; every step one rounded
// operation in the order written (no contraction):
//   M    = max_c m_c
//   e_c  = exp(m_c - M)
//   s    = sum_c S_c e_c,   q = sum_c Q_c (e_c e_c)
//   loglike_k          = ((M + log s) - log(C n)) + cst_k
//   chain_loglike[c,k] = ((m_c + log S_c) - log n) + cst_k        (NaN: S_c == 0)
//   neff_k             = (s s) / q
// NaN for n == 0 or when no chain has a sample.  tests/_br_likelihood.py
// restates update and finish.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string>

#include "gibbs_capi.h"
#include "gs_common.h"
#include "gs_launch.h"

using gs_detail::set_error;
using gs_detail::nblk;

namespace {

constexpr int HDR = 8;       // header doubles
constexpr int BS = 256;      // threads per workgroup
constexpr int TR = 32;       // rows per row tile
constexpr int TK = 128;      // models per workgroup
constexpr int JC = 16;       // used columns per LDS chunk
constexpr int RM = 4;        // rows per thread
constexpr int MM = 4;        // models per thread
constexpr int XE = TR * JC / BS;   // x elements a thread stages per chunk
constexpr int YE = TK * JC / BS;   // Y elements a thread stages per chunk
static_assert(TR >= JC, "the dot tile reuses the Y chunk's LDS");
static_assert((BS / 32) * RM == TR && 32 * MM == TK, "thread blocking covers the tile");

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }

// one chunk's global values, in flight while the previous chunk is contracted
struct Chunk {
    double x[XE], dd[XE], c[XE], Y[YE];
    int kd[XE];
    double coef;
    int kind;
};

__global__ __launch_bounds__(BS) void k_brl_update(double* __restrict__ state, int nchains, int nsb, int maxbins,
                                                   int K, int Ju, const int* __restrict__ cols,
                                                   const int* __restrict__ kind, const double* __restrict__ coef,
                                                   const double* __restrict__ Y, const double* __restrict__ scales,
                                                   int cap, int slot0, int nsteps, int nkt) {
    __shared__ double s_x[JC][TR + 1];
    __shared__ double s_lg[JC][TR + 1];
    __shared__ double s_Y[TR][TK + 1];          // Y chunk [j][model]; after the last chunk the dot tile [row][model]
    __shared__ double s_coef[JC];
    __shared__ int s_kind[JC];
    __shared__ double s_r[TR];
    const int t = threadIdx.x;
    const int kt = blockIdx.x % nkt, chain = blockIdx.x / nkt;
    const int k0 = kt * TK;
    const long long n0 = *(volatile const long long*)state;
    const long long nck = (long long)nchains * K;
    double* fm = state + HDR;
    double* fS = fm + nck;
    double* fQ = fS + nck;
    const int ml = t & 31, rg = t >> 5;
    const bool owner = t < TK && k0 + t < K;    // this thread folds model k0 + t
    const long long ek = (long long)chain * K + k0 + t;
    double m = owner ? fm[ek] : 0.0, S = owner ? fS[ek] : 0.0, Q = owner ? fQ[ek] : 0.0;
    long long nbad = 0;
    const int nchunk = (Ju + JC - 1) / JC;

    for (int t0 = 0; t0 < nsteps; t0 += TR) {
        const int tn = nsteps - t0 < TR ? nsteps - t0 : TR;
        Chunk g;
        // global loads of chunk ch into registers (nothing waits on them here)
        auto load = [&](int ch) {
            const int j0 = ch * JC;
#pragma unroll
            for (int e = 0; e < XE; ++e) {
                const int idx = t + BS * e, jj = idx & (JC - 1), row = idx / JC, j = j0 + jj;
                g.x[e] = 0.0; g.dd[e] = 0.0; g.c[e] = 0.0; g.kd[e] = 0;
                if (j < Ju && row < tn) {
                    int slot = slot0 + t0 + row;
                    if (slot >= cap) slot -= cap;              // slot0 < cap and nsteps <= cap: one wrap
                    const int col = cols[j];
                    const double* rowp = scales + ((long long)slot * nchains + chain) * nsb;
                    const int kd = kind[j];
                    g.kd[e] = kd;
                    if (col >= 0 && col < nsb) g.x[e] = rowp[col];
                    if (kd == 2) {
                        const bool in = col >= 0 && col + 3 * maxbins < nsb;
                        g.dd[e] = in ? rowp[col + maxbins] : qnan();
                        g.c[e] = in ? rowp[col + 3 * maxbins] : qnan();
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < YE; ++e) {
                const int idx = t + BS * e, jj = idx & (JC - 1), km = idx / JC, j = j0 + jj;
                g.Y[e] = (j < Ju && k0 + km < K) ? Y[(long long)(k0 + km) * Ju + j] : 0.0;
            }
            g.kind = 0; g.coef = 0.0;
            if (t < JC && j0 + t < Ju) { g.kind = kind[j0 + t]; g.coef = coef[j0 + t]; }
        };
        // the loaded chunk into LDS, with the logarithm of every (row, column) that has one
        auto store = [&]() {
#pragma unroll
            for (int e = 0; e < XE; ++e) {
                const int idx = t + BS * e, jj = idx & (JC - 1), row = idx / JC;
                double lg = 0.0;
                if (g.kd[e] == 1) {
                    lg = pos_finite(g.x[e]) ? log(g.x[e]) : qnan();
                } else if (g.kd[e] == 2) {
                    const double det = fma(g.x[e], g.dd[e], -(g.c[e] * g.c[e]));
                    lg = pos_finite(det) ? log(det) : qnan();
                }
                s_x[jj][row] = g.x[e];
                s_lg[jj][row] = lg;
            }
#pragma unroll
            for (int e = 0; e < YE; ++e) {
                const int idx = t + BS * e, jj = idx & (JC - 1), km = idx / JC;
                s_Y[jj][km] = g.Y[e];
            }
            if (t < JC) { s_kind[t] = g.kind; s_coef[t] = g.coef; }
        };

        double acc[RM][MM];
#pragma unroll
        for (int p = 0; p < RM; ++p)
#pragma unroll
            for (int q = 0; q < MM; ++q) acc[p][q] = 0.0;
        double r = 0.0;
        bool badrow = false;

        __syncthreads();                                       // the previous tile's fold has read the dot tile
        for (int ch = -1; ch < nchunk; ++ch) {
            // chunk ch + 1 leaves for the registers, chunk ch is contracted from
            // LDS, then chunk ch + 1 takes its place
            if (ch + 1 < nchunk) load(ch + 1);
            if (ch >= 0) {
                const int jn = Ju - ch * JC < JC ? Ju - ch * JC : JC;
                if (t < tn) {                                  // r of row t, j ascending
                    for (int jj = 0; jj < jn; ++jj) {
                        if (s_kind[jj] != 0) {
                            const double lg = s_lg[jj][t];
                            if (lg == lg) r = fma(s_coef[jj], lg, r);
                            else badrow = true;
                        }
                    }
                }
                if (rg * RM < tn) {
#pragma unroll 2
                    for (int jj = 0; jj < jn; ++jj) {
                        double xv[RM], yv[MM];
#pragma unroll
                        for (int p = 0; p < RM; ++p) xv[p] = s_x[jj][rg * RM + p];
#pragma unroll
                        for (int q = 0; q < MM; ++q) yv[q] = s_Y[jj][ml + 32 * q];
#pragma unroll
                        for (int p = 0; p < RM; ++p)
#pragma unroll
                            for (int q = 0; q < MM; ++q) acc[p][q] = fma(xv[p], yv[q], acc[p][q]);
                    }
                }
            }
            __syncthreads();                                   // chunk ch has been read
            if (ch + 1 < nchunk) {
                store();
                __syncthreads();
            }
        }
        // the dot tile and the rows' r (NaN: skipped) for the fold
#pragma unroll
        for (int p = 0; p < RM; ++p)
#pragma unroll
            for (int q = 0; q < MM; ++q) s_Y[rg * RM + p][ml + 32 * q] = acc[p][q];
        if (t < TR) {
            s_r[t] = (t < tn && !badrow) ? r : qnan();
            if (t < tn && badrow) ++nbad;
        }
        __syncthreads();
        if (owner) {
            for (int i = 0; i < tn; ++i) {
                const double ri = s_r[i];
                if (ri == ri) {
                    const double tv = ri - s_Y[i][t];
                    if (S == 0.0) {
                        m = tv;
                        S = 1.0;
                        Q = 1.0;
                    } else {
                        const double d = tv - m;
                        const double w = exp(-fabs(d));
                        if (d > 0.0) {
                            const double ww = w * w;
                            S = fma(S, w, 1.0);
                            Q = fma(Q, ww, 1.0);
                            m = tv;
                        } else {
                            S = S + w;
                            Q = fma(w, w, Q);
                        }
                    }
                }
            }
        }
    }
    if (owner) {
        fm[ek] = m;
        fS[ek] = S;
        fQ[ek] = Q;
    }
    if (kt == 0 && t < TR && nbad) {
        unsigned long long* bad = (unsigned long long*)(fQ + nck);
        atomicAdd(&bad[chain], (unsigned long long)nbad);
    }
    // the last workgroup to finish advances n: every workgroup read it at its start
    __syncthreads();
    if (t == 0) {
        __threadfence();
        unsigned* ticket = (unsigned*)(state + 1);
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            *(long long*)state = n0 + nsteps;
            *ticket = 0u;
        }
    }
}

__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }

__global__ __launch_bounds__(BS) void k_brl_finish(const double* __restrict__ state, int C, int K,
                                                   const double* __restrict__ cst, double* __restrict__ loglike,
                                                   double* __restrict__ chain_loglike, double* __restrict__ neff) {
    const int k = blockIdx.x * BS + threadIdx.x;
    if (k >= K) return;
    const long long n = *(const long long*)state;
    const long long nck = (long long)C * K;
    const double* fm = state + HDR;
    const double* fS = fm + nck;
    const double* fQ = fS + nck;
    const double ck = cst[k];
    bool any = false;
    double M = 0.0;
    for (int c = 0; c < C; ++c) {
        const long long e = (long long)c * K + k;
        const bool has = n > 0 && fS[e] > 0.0;
        if (has) {
            M = any ? fmax(M, fm[e]) : fm[e];
            any = true;
        }
        chain_loglike[e] = has ? add(sub(add(fm[e], log(fS[e])), log((double)n)), ck) : qnan();
    }
    double ll = qnan(), ne = qnan();
    if (any) {
        double s = 0.0, q = 0.0;
        for (int c = 0; c < C; ++c) {
            const long long e = (long long)c * K + k;
            if (fS[e] > 0.0) {
                const double ex = exp(sub(fm[e], M));
                s = add(s, mul(fS[e], ex));
                q = add(q, mul(fQ[e], mul(ex, ex)));
            }
        }
        ll = add(sub(add(M, log(s)), log(mul((double)C, (double)n))), ck);
        ne = __ddiv_rn(mul(s, s), q);
    }
    loglike[k] = ll;
    neff[k] = ne;
}

int check_dims(const char* what, long long nchains, int K) {
    if (nchains < 1) return set_error(std::string(what) + ": nchains >= 1 needed");
    if (K < 1) return set_error(std::string(what) + ": models K >= 1 needed");
    if (nchains * K > (1LL << 28)) return set_error(std::string(what) + ": too many (chain, model) pairs");
    return 0;
}

long long state_bytes(long long nchains, int K) { return 8LL * (HDR + 3 * nchains * K + nchains); }

}  // namespace

extern "C" {

int gs_brl_bytes(int nchains, int K, long long* bytes) {
    if (!bytes) return set_error("gs_brl_bytes: null argument");
    if (check_dims("gs_brl_bytes", nchains, K)) return -1;
    *bytes = state_bytes(nchains, K);
    return 0;
}

int gs_brl_reset(void* state, int nchains, int K, void* stream) {
    if (!state) return set_error("gs_brl_reset: null state");
    if (check_dims("gs_brl_reset", nchains, K)) return -1;
    GS_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(nchains, K), (hipStream_t)stream));
    return 0;
}

int gs_brl_update(void* state, int nchains, int nspec, int maxbins, int K, int Ju, const int* cols, const int* kind,
                  const double* coef, const double* Y, const double* scales, int capacity, uint32_t first_iteration,
                  int nsteps, void* stream) {
    if (!state) return set_error("gs_brl_update: null state");
    if (check_dims("gs_brl_update", nchains, K)) return -1;
    if (nspec < 1 || nspec > 32 || maxbins < 1)
        return set_error("gs_brl_update: maxbins >= 1 and nspec in [1, 32] out of range");
    if ((long long)nchains * nspec * maxbins > (1LL << 28)) return set_error("gs_brl_update: too many series");
    if (Ju < 1 || Ju > nspec * maxbins) return set_error("gs_brl_update: used columns Ju out of range [1, nspec * maxbins]");
    if (nsteps == 0) return 0;
    if (!cols || !kind || !coef || !Y || !scales) return set_error("gs_brl_update: null table or scale trace");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_brl_update: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    const int nkt = (K + TK - 1) / TK;
    const long long nb = (long long)nkt * nchains;
    if (nb > 0x7fffffffLL) return set_error("gs_brl_update: too many (chain, model tile) workgroups for one launch");
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    hipLaunchKernelGGL(k_brl_update, dim3((unsigned)nb), dim3(BS), 0, (hipStream_t)stream, (double*)state, nchains,
                       nspec * maxbins, maxbins, K, Ju, cols, kind, coef, Y, scales, capacity, slot0, nsteps, nkt);
    GS_LAUNCH_CHECK("k_brl_update");
    return 0;
}

int gs_brl_finish(const void* state, int C, int K, const double* cst, double* loglike, double* chain_loglike,
                  double* neff, void* stream) {
    if (!state) return set_error("gs_brl_finish: null state");
    if (check_dims("gs_brl_finish", C, K)) return -1;
    if (!cst || !loglike || !chain_loglike || !neff) return set_error("gs_brl_finish: null cst or output");
    hipLaunchKernelGGL(k_brl_finish, dim3(nblk(K, BS)), dim3(BS), 0, (hipStream_t)stream, (const double*)state, C, K,
                       cst, loglike, chain_loglike, neff);
    GS_LAUNCH_CHECK("k_brl_finish");
    return 0;
}

}  // extern "C"
