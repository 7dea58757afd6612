// gs_wf.hip -- Rao-Blackwellised posterior sky map of the full-sky samplers (gfx950).
//
// On the full sky the centered CR draw is s = M_l d + L_l z per l
// (block_params_from<F, 0>, gs_block.h), so E[s | D_l, d] = M_l d and
// Cov[s | D_l, d] = Sigma_l = L_l L_l^T in closed form, and the posterior of the
// map follows from the D_l chain alone (law of total expectation / variance):
//   E[s_lm | d]   = mean_i M_l^i d_lm
//   Var[s_lm | d] = mean_i Sigma_l^i + Var_i(M_l^i d_lm)
//   E[sigma_l | d] = mean_i (Sigma_l^i + M_l^i S_l M_l^i^T / (2l+1)),  S_l = sum_m d_lm d_lm^T
// Plan-independent in the sense of gs_summary.hip: every table is an argument.
// MODE 0 (the centered operator) whatever sampler produced the D_l.
//
// Per (chain, l) the state keeps NFLD values, F = 3 (F <= 2: per field f):
//   op   0..4    Welford means of M00, M01, M10, M11, M22          (M_f)
//   cm   5..11   co-moment sums of the pairs (M00,M00), (M00,M01), (M01,M01),
//                (M10,M10), (M10,M11), (M11,M11), (M22,M22)        ((M_f,M_f))
//   sg   12..15  means of s00, s11, s01, s22 (from the Cholesky entries)  (s_f)
//   pw   16..19  means of the per-l power TT, EE, BB, TE           (per field)
// State (caller-owned device buffer of gs_wf_bytes bytes, fp64 unless noted):
//   header   8 doubles: [0] int64 k, the samples accumulated per chain; rest 0
//   planes   [NFLD][C][L+1], l fastest: lane g = chain (L+1) + l of plane q is
//            element q C (L+1) + g, so a wave reads and writes whole lines
// gs_wf_reset zeroes all of it.
//
// k_wf_update, one thread per (chain, l), rows in iteration order, sample number
// t = count_after - nsteps + i + 1 of row i (the count is the host's):
//   r = 1 / t;  d_q = x_q - mean_q;  mean_q += d_q r;  e_q = x_q - mean_q
//   cm(a, b) += d_a e_b;            mean-only fields: mean += (x - mean) r
// Rows go in register tiles of TL = 8 whose D_l loads are issued together before
// any arithmetic (the bin indices of an l do not depend on the row and are
// loaded once); a tail of fewer than TL rows takes the TL = 1 form, the same
// arithmetic in the same order.  No atomics and no cross-lane work: the state's
// bits depend neither on how the iterations are cut into launches, nor on the
// ring capacity or a wrap, nor on the launch geometry, nor on the other chains.
//
// k_wf_finish, one thread per (field, real-layout slot) over the C chains of k
// samples each (k from the header).  A slot's series is m^i = sum_g M_fg^i d_g,
// g over the fields coupled to f (T and E for f in {T, E} of F = 3, else f).
// Chains merge in chain order by Chan's update, for every mean and co-moment:
//   nA = k;  for c = 1 .. C-1:  da = a_c - a_A;  nAB = nA + k;
//     cm_A(a, b) += cm_c(a, b) + da db (nA k / nAB);  a_A += da (k / nAB);  nA = nAB
//   alm_mean = sum_g Mbar_fg d_g
//   alm_var  = Sigmabar_ff + sum_gh cm_A(fg, fh) d_g d_h / (C k - 1)   (NaN when C k < 2)
//   chain_alm_mean[c] = sum_g M_fg,c d_g
//   rhat as k_summary_finish on the series: with q_c = sum_gh cm_c(fg, fh) d_g d_h,
//     W = mean_c q_c / (k - 1),  B/k = sum_c (m_c - mean_c m_c)^2 / (C - 1),
//     var+ = mean_c q_c / k + B/k,  rhat = sqrt(var+ / W)
//   (NaN for C = 1, k < 2 or W == 0).
//
// k_wf_power, one thread per l, chains pooled in chain order as above:
//   power_of_mean = Mbar S Mbar^T / (2l+1)   [nspec][L+1] (TE included for F = 3)
//   mean_power    = the pooled mean of pw    [nspec][L+1]
//   op_mean       = the pooled operator      [nop][L+1]
// S_l [nspec][L+1] (spectrum order: TT, EE, BB, TE = sum d_T d_E for F = 3) comes
// from k_wf_moments, one thread per l adding its rows in the order m = 0 .. l
// (m > 0: re before im), once per data tensor.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <string>

#include "gibbs_capi.h"
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_block.h"

using gs_detail::set_error;
using gs_detail::nblk;
using gs_detail::with_F;

namespace {

constexpr int HDR = 8;       // header doubles
constexpr int BS = 64;       // one wave per workgroup (update, power, moments)
constexpr int BSF = 256;     // finish
constexpr int TL = 8;        // rows per register tile

template <int F>
struct WF {
    static constexpr int NS = F == 3 ? 4 : F;         // spectra = Sigma entries = powers
    static constexpr int NOP = F == 3 ? 5 : F;        // operator entries
    static constexpr int NCM = F == 3 ? 7 : F;        // co-moment pairs
    static constexpr int OP = 0, CM = NOP, SG = NOP + NCM, PW = NOP + NCM + NS;
    static constexpr int NFLD = NOP + NCM + 2 * NS;
};

inline int nfld_of(int F) { return F == 3 ? WF<3>::NFLD : 4 * F; }

__device__ __forceinline__ void mean_step(double x, double r, double& mean) { mean = mean + (x - mean) * r; }

// one row of one (chain, l) into the accumulators
template <int F>
__device__ __forceinline__ void wf_row(int ell, double b, const double (&dq)[WF<F>::NS], double k0, double k1,
                                       double k2, const double (&A)[WF<F>::NS], double w2, double r,
                                       double (&acc)[WF<F>::NFLD]) {
    using W = WF<F>;
    double p[gs_block::NP];
    block_params_from<F, 0>(ell, b, dq, k0, k1, k2, p);
    if constexpr (F == 3) {
        double d[5], e[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            d[q] = p[q] - acc[W::OP + q];
            acc[W::OP + q] = acc[W::OP + q] + d[q] * r;
            e[q] = p[q] - acc[W::OP + q];
        }
        acc[W::CM + 0] = acc[W::CM + 0] + d[0] * e[0];
        acc[W::CM + 1] = acc[W::CM + 1] + d[0] * e[1];
        acc[W::CM + 2] = acc[W::CM + 2] + d[1] * e[1];
        acc[W::CM + 3] = acc[W::CM + 3] + d[2] * e[2];
        acc[W::CM + 4] = acc[W::CM + 4] + d[2] * e[3];
        acc[W::CM + 5] = acc[W::CM + 5] + d[3] * e[3];
        acc[W::CM + 6] = acc[W::CM + 6] + d[4] * e[4];
        const double M00 = p[0], M01 = p[1], M10 = p[2], M11 = p[3], M22 = p[4];
        const double s00 = p[5] * p[5], s01 = p[6] * p[5], s11 = p[6] * p[6] + p[7] * p[7], s22 = p[8] * p[8];
        const double att = A[0], aee = A[1], abb = A[2], ate = A[3];
        const double qtt = (M00 * M00) * att + 2.0 * (M00 * M01) * ate + (M01 * M01) * aee;
        const double qee = (M10 * M10) * att + 2.0 * (M10 * M11) * ate + (M11 * M11) * aee;
        const double qte = (M00 * M10) * att + (M00 * M11 + M01 * M10) * ate + (M01 * M11) * aee;
        const double qbb = (M22 * M22) * abb;
        mean_step(s00, r, acc[W::SG + 0]);
        mean_step(s11, r, acc[W::SG + 1]);
        mean_step(s01, r, acc[W::SG + 2]);
        mean_step(s22, r, acc[W::SG + 3]);
        mean_step(s00 + qtt / w2, r, acc[W::PW + 0]);
        mean_step(s11 + qee / w2, r, acc[W::PW + 1]);
        mean_step(s22 + qbb / w2, r, acc[W::PW + 2]);
        mean_step(s01 + qte / w2, r, acc[W::PW + 3]);
    } else {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const double M = p[f], s = p[F + f] * p[F + f];
            const double d = M - acc[W::OP + f];
            acc[W::OP + f] = acc[W::OP + f] + d * r;
            acc[W::CM + f] = acc[W::CM + f] + d * (M - acc[W::OP + f]);
            mean_step(s, r, acc[W::SG + f]);
            mean_step(s + (M * M) * A[f] / w2, r, acc[W::PW + f]);
        }
    }
}

// TLN rows from the ring: every load first, then the arithmetic in row order
template <int F, int TLN>
__device__ __forceinline__ void wf_tile(const double* __restrict__ tr, long long row_stride, int cap, int& slot,
                                        const int (&bq)[WF<F>::NS], int maxbins, int ell, double b, double k0,
                                        double k1, double k2, const double (&A)[WF<F>::NS], double w2, long long& t,
                                        double (&acc)[WF<F>::NFLD]) {
    constexpr int NS = WF<F>::NS;
    double dq[TLN][NS];
#pragma unroll
    for (int i = 0; i < TLN; ++i) {
        const double* row = tr + (long long)slot * row_stride;
#pragma unroll
        for (int q = 0; q < NS; ++q) dq[i][q] = row[q * maxbins + max(bq[q], 0)];
        slot = slot + 1 == cap ? 0 : slot + 1;
    }
#pragma unroll
    for (int i = 0; i < TLN; ++i) {
#pragma unroll
        for (int q = 0; q < NS; ++q) dq[i][q] = bq[q] < 0 ? 0.0 : dq[i][q];
        t = t + 1;
        wf_row<F>(ell, b, dq[i], k0, k1, k2, A, w2, 1.0 / (double)t, acc);
    }
}

template <int F>
__global__ __launch_bounds__(BS) void k_wf_update(double* __restrict__ state, int C, int L, int maxbins,
                                                  const double* __restrict__ bl, const int* __restrict__ ell2bin,
                                                  double k0, double k1, double k2, const double* __restrict__ mom,
                                                  const double* __restrict__ trace, int cap, int slot0, int nsteps,
                                                  long long count_after) {
    using W = WF<F>;
    constexpr int NS = W::NS;
    const int Lp1 = L + 1;
    const long long nl = (long long)C * Lp1;
    const long long g = (long long)blockIdx.x * BS + threadIdx.x;
    if (g < nl) {
        const int chain = (int)(g / Lp1), ell = (int)(g % Lp1);
        int bq[NS];
        double A[NS], acc[W::NFLD];
#pragma unroll
        for (int q = 0; q < NS; ++q) bq[q] = ell2bin[q * Lp1 + ell];
#pragma unroll
        for (int q = 0; q < NS; ++q) A[q] = mom[q * Lp1 + ell];
        const double b = bl[ell], w2 = 2.0 * ell + 1.0;
        double* fld = state + HDR + g;
#pragma unroll
        for (int q = 0; q < W::NFLD; ++q) acc[q] = fld[q * nl];
        // chain's rows: trace[slot][chain][spectrum][bin]
        const double* tr = trace + (long long)chain * NS * maxbins;
        const long long row_stride = (long long)C * NS * maxbins;
        long long t = count_after - nsteps;          // samples before this launch's first row
        int slot = slot0, i = 0;
        for (; i + TL <= nsteps; i += TL)
            wf_tile<F, TL>(tr, row_stride, cap, slot, bq, maxbins, ell, b, k0, k1, k2, A, w2, t, acc);
        for (; i < nsteps; ++i)
            wf_tile<F, 1>(tr, row_stride, cap, slot, bq, maxbins, ell, b, k0, k1, k2, A, w2, t, acc);
#pragma unroll
        for (int q = 0; q < W::NFLD; ++q) fld[q * nl] = acc[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *(long long*)state = count_after;
}

// multipole of slot r of the real m-major layout:
// slots 0..L are a_l0; pair i = (r + L + 1) / 2 = g(m) + (l - m), g(m) = m (2L + 3 - m) / 2
__device__ __forceinline__ int slot_ell(long long r, int L) {
    if (r <= L) return (int)r;
    const long long i = (r + L + 1) / 2;
    const double c = 2.0 * L + 3.0;
    long long m = (long long)((c - sqrt(fmax(c * c - 8.0 * (double)i, 0.0))) * 0.5);
    m = m < 1 ? 1 : (m > L ? L : m);
    while (m > 1 && m * (2LL * L + 3 - m) / 2 > i) --m;
    while (m < L && (m + 1) * (2LL * L + 2 - m) / 2 <= i) ++m;
    return (int)(i - m * (2LL * L + 1 - m) / 2);
}

template <int F>
__global__ __launch_bounds__(BSF) void k_wf_finish(const double* __restrict__ state, int C, int L,
                                                   const double* __restrict__ d_alm, double* __restrict__ mean_out,
                                                   double* __restrict__ var_out, double* __restrict__ chain_mean,
                                                   double* __restrict__ rhat_out) {
    using W = WF<F>;
    const int Lp1 = L + 1;
    const long long NR = (long long)Lp1 * Lp1, n = (long long)F * NR, nl = (long long)C * Lp1;
    const long long k = *(const long long*)state;
    const double* fld = state + HDR;
    const double kd = (double)k, Cd = (double)C, qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long i = (long long)blockIdx.x * BSF + threadIdx.x; i < n; i += (long long)gridDim.x * BSF) {
        const int f = (int)(i / NR);
        const long long r = i % NR;
        const int ell = slot_ell(r, L);
        // the operator row of field f: entries (ia, ib) on the data (x0, x1), their
        // co-moments (caa, cab, cbb) and Sigma_ff; one entry when f couples to itself only
        const bool two = F == 3 && f < 2;
        int ia, ib, caa, cab, cbb, sg;
        double x0, x1 = 0.0;
        if (two) {
            ia = W::OP + 2 * f; ib = ia + 1;
            caa = W::CM + 3 * f; cab = caa + 1; cbb = caa + 2;
            sg = W::SG + f;
            x0 = d_alm[r];
            x1 = d_alm[NR + r];
        } else {
            ia = ib = W::OP + (F == 3 ? 4 : f);
            caa = cab = cbb = W::CM + (F == 3 ? 6 : f);
            sg = W::SG + (F == 3 ? 3 : f);
            x0 = d_alm[i];
        }
        const double x00 = x0 * x0, x01 = 2.0 * (x0 * x1), x11 = x1 * x1;
        double nA = kd, aA = 0.0, bA = 0.0, CAA = 0.0, CAB = 0.0, CBB = 0.0, sA = 0.0;
        double sum_m = 0.0, sum_q = 0.0;
        for (int c = 0; c < C; ++c) {
            const long long o = (long long)c * Lp1 + ell;
            const double a = fld[ia * nl + o], qaa = fld[caa * nl + o], s = fld[sg * nl + o];
            double b = 0.0, qab = 0.0, qbb = 0.0;
            if (two) { b = fld[ib * nl + o]; qab = fld[cab * nl + o]; qbb = fld[cbb * nl + o]; }
            const double mc = two ? a * x0 + b * x1 : a * x0;
            const double qc = two ? qaa * x00 + qab * x01 + qbb * x11 : qaa * x00;
            chain_mean[(long long)c * n + i] = k >= 1 ? mc : qnan;
            sum_m = sum_m + mc;
            sum_q = sum_q + qc;
            if (c == 0) {
                aA = a; bA = b; CAA = qaa; CAB = qab; CBB = qbb; sA = s;
            } else {
                const double da = a - aA, db = b - bA, nAB = nA + kd, w = kd / nAB, wn = nA * kd / nAB;
                CAA = CAA + qaa + (da * da) * wn;
                CAB = CAB + qab + (da * db) * wn;
                CBB = CBB + qbb + (db * db) * wn;
                aA = aA + da * w;
                bA = bA + db * w;
                sA = sA + (s - sA) * w;
                nA = nAB;
            }
        }
        const long long N = (long long)C * k;
        const double quad = two ? CAA * x00 + CAB * x01 + CBB * x11 : CAA * x00;
        mean_out[i] = k >= 1 ? (two ? aA * x0 + bA * x1 : aA * x0) : qnan;
        var_out[i] = (k >= 1 && N >= 2) ? sA + quad / (double)(N - 1) : qnan;
        double rhat = qnan;
        if (C > 1 && k >= 2) {
            const double m = sum_m / Cd;
            double sb2 = 0.0;
            for (int c = 0; c < C; ++c) {
                const long long o = (long long)c * Lp1 + ell;
                const double a = fld[ia * nl + o], b = two ? fld[ib * nl + o] : 0.0;
                const double dm = (two ? a * x0 + b * x1 : a * x0) - m;
                sb2 = sb2 + dm * dm;
            }
            const double Wv = sum_q / (kd - 1.0) / Cd, g0 = sum_q / kd / Cd;
            const double varp = g0 + sb2 / (Cd - 1.0);
            if (Wv > 0.0) rhat = sqrt(varp / Wv);
        }
        rhat_out[i] = rhat;
    }
}

// the pooled mean of plane q at l over the C chains (Chan's mean update, equal counts)
__device__ __forceinline__ double pooled_mean(const double* __restrict__ fld, int q, long long nl, int C, int Lp1,
                                              int ell, double kd) {
    double mA = fld[q * nl + ell], nA = kd;
    for (int c = 1; c < C; ++c) {
        const double nAB = nA + kd;
        mA = mA + (fld[q * nl + (long long)c * Lp1 + ell] - mA) * (kd / nAB);
        nA = nAB;
    }
    return mA;
}

template <int F>
__global__ __launch_bounds__(BS) void k_wf_power(const double* __restrict__ state, int C, int L,
                                                 const double* __restrict__ mom, double* __restrict__ pom,
                                                 double* __restrict__ mp, double* __restrict__ opm) {
    using W = WF<F>;
    const int Lp1 = L + 1;
    const int ell = blockIdx.x * BS + threadIdx.x;
    if (ell > L) return;
    const long long k = *(const long long*)state, nl = (long long)C * Lp1;
    const double* fld = state + HDR;
    const double kd = (double)k, w2 = 2.0 * ell + 1.0, qnan = __longlong_as_double(0x7ff8000000000000LL);
    double M[W::NOP], A[W::NS];
#pragma unroll
    for (int q = 0; q < W::NOP; ++q) M[q] = k >= 1 ? pooled_mean(fld, W::OP + q, nl, C, Lp1, ell, kd) : qnan;
#pragma unroll
    for (int q = 0; q < W::NS; ++q) A[q] = mom[q * Lp1 + ell];
#pragma unroll
    for (int q = 0; q < W::NOP; ++q) opm[q * Lp1 + ell] = M[q];
#pragma unroll
    for (int q = 0; q < W::NS; ++q) mp[q * Lp1 + ell] = k >= 1 ? pooled_mean(fld, W::PW + q, nl, C, Lp1, ell, kd) : qnan;
    if constexpr (F == 3) {
        const double att = A[0], aee = A[1], abb = A[2], ate = A[3];
        pom[0 * Lp1 + ell] = ((M[0] * M[0]) * att + 2.0 * (M[0] * M[1]) * ate + (M[1] * M[1]) * aee) / w2;
        pom[1 * Lp1 + ell] = ((M[2] * M[2]) * att + 2.0 * (M[2] * M[3]) * ate + (M[3] * M[3]) * aee) / w2;
        pom[2 * Lp1 + ell] = (M[4] * M[4]) * abb / w2;
        pom[3 * Lp1 + ell] = ((M[0] * M[2]) * att + (M[0] * M[3] + M[1] * M[2]) * ate + (M[1] * M[3]) * aee) / w2;
    } else {
#pragma unroll
        for (int f = 0; f < F; ++f) pom[f * Lp1 + ell] = (M[f] * M[f]) * A[f] / w2;
    }
}

template <int F>
__global__ __launch_bounds__(BS) void k_wf_moments(int L, const double* __restrict__ d, double* __restrict__ mom) {
    constexpr int NS = WF<F>::NS;
    const int ell = blockIdx.x * BS + threadIdx.x;
    if (ell > L) return;
    const long long NR = (long long)(L + 1) * (L + 1);
    double a[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) a[q] = 0.0;
    for (int m = 0; m <= ell; ++m) {
        const long long r = m == 0 ? (long long)ell : 2 * ((long long)m * (2 * L + 1 - m) / 2 + ell) - (L + 1);
        const int nv = m == 0 ? 1 : 2;
        for (int c = 0; c < nv; ++c) {
            double dv[F];
#pragma unroll
            for (int f = 0; f < F; ++f) dv[f] = d[f * NR + r + c];
#pragma unroll
            for (int f = 0; f < F; ++f) a[f] = a[f] + dv[f] * dv[f];
            if constexpr (F == 3) a[3] = a[3] + dv[0] * dv[1];
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) mom[q * (L + 1) + ell] = a[q];
}

int check_dims(const char* what, int F, long long C, int L) {
    if (F < 1 || F > 3) return set_error(std::string(what) + ": nfields out of range [1, 3]");
    if (C < 1 || C > (1LL << 24)) return set_error(std::string(what) + ": nchains out of range (need 1 <= C <= 2^24)");
    if (L < 0 || L > 16384) return set_error(std::string(what) + ": lmax out of range [0, 16384]");
    // one launch of 64-lane workgroups covers every (chain, l)
    if (C * (L + 1) > (1LL << 26)) return set_error(std::string(what) + ": nchains * (lmax + 1) too large");
    return 0;
}

long long state_bytes(int F, long long C, int L) { return 8LL * (HDR + (long long)nfld_of(F) * C * (L + 1)); }

}  // namespace

extern "C" {

int gs_wf_bytes(int nfields, int nchains, int lmax, long long* bytes) {
    if (!bytes) return set_error("gs_wf_bytes: null bytes");
    if (check_dims("gs_wf_bytes", nfields, nchains, lmax)) return -1;
    *bytes = state_bytes(nfields, nchains, lmax);
    return 0;
}

int gs_wf_reset(void* state, int nfields, int nchains, int lmax, void* stream) {
    if (!state) return set_error("gs_wf_reset: null state");
    if (check_dims("gs_wf_reset", nfields, nchains, lmax)) return -1;
    GS_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(nfields, nchains, lmax), (hipStream_t)stream));
    return 0;
}

int gs_wf_moments(int lmax, int nfields, const double* d_alm, double* moments, void* stream) {
    if (check_dims("gs_wf_moments", nfields, 1, lmax)) return -1;
    if (!d_alm) return set_error("gs_wf_moments: null d_alm");
    if (!moments) return set_error("gs_wf_moments: null moments");
    with_F(nfields, [&](auto f) {
        hipLaunchKernelGGL((k_wf_moments<decltype(f)::value>), dim3(nblk(lmax + 1, BS)), dim3(BS), 0,
                           (hipStream_t)stream, lmax, d_alm, moments);
    });
    GS_LAUNCH_CHECK("k_wf_moments");
    return 0;
}

int gs_wf_update(void* state, int nfields, int nchains, int lmax, int maxbins, const double* bl, const int* ell2bin,
                 double k0, double k1, double k2, const double* moments, const double* trace, int capacity,
                 uint32_t first_iteration, int nsteps, long long count_after, void* stream) {
    if (!state) return set_error("gs_wf_update: null state");
    if (check_dims("gs_wf_update", nfields, nchains, lmax)) return -1;
    if (maxbins < 1) return set_error("gs_wf_update: maxbins out of range (need maxbins >= 1)");
    if (nsteps == 0) return 0;
    if (!bl) return set_error("gs_wf_update: null bl");
    if (!ell2bin) return set_error("gs_wf_update: null ell2bin");
    if (!moments) return set_error("gs_wf_update: null moments");
    if (!trace) return set_error("gs_wf_update: null trace");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_wf_update: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    if (count_after < nsteps) return set_error("gs_wf_update: count_after out of range (need count_after >= nsteps)");
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    const unsigned nb = nblk((long long)nchains * (lmax + 1), BS);
    with_F(nfields, [&](auto f) {
        hipLaunchKernelGGL((k_wf_update<decltype(f)::value>), dim3(nb), dim3(BS), 0, (hipStream_t)stream,
                           (double*)state, nchains, lmax, maxbins, bl, ell2bin, k0, k1, k2, moments, trace, capacity,
                           slot0, nsteps, count_after);
    });
    GS_LAUNCH_CHECK("k_wf_update");
    return 0;
}

int gs_wf_finish(const void* state, int nfields, int C, int lmax, const double* d_alm, double* alm_mean,
                 double* alm_var, double* chain_alm_mean, double* alm_rhat, void* stream) {
    if (!state) return set_error("gs_wf_finish: null state");
    if (check_dims("gs_wf_finish", nfields, C, lmax)) return -1;
    if (!d_alm) return set_error("gs_wf_finish: null d_alm");
    if (!alm_mean) return set_error("gs_wf_finish: null alm_mean");
    if (!alm_var) return set_error("gs_wf_finish: null alm_var");
    if (!chain_alm_mean) return set_error("gs_wf_finish: null chain_alm_mean");
    if (!alm_rhat) return set_error("gs_wf_finish: null alm_rhat");
    const long long n = (long long)nfields * (lmax + 1) * (lmax + 1);
    const unsigned nb = std::min(nblk(n, BSF), 16384u);
    with_F(nfields, [&](auto f) {
        hipLaunchKernelGGL((k_wf_finish<decltype(f)::value>), dim3(nb), dim3(BSF), 0, (hipStream_t)stream,
                           (const double*)state, C, lmax, d_alm, alm_mean, alm_var, chain_alm_mean, alm_rhat);
    });
    GS_LAUNCH_CHECK("k_wf_finish");
    return 0;
}

int gs_wf_power(const void* state, int nfields, int C, int lmax, const double* moments, double* power_of_mean,
                double* mean_power, double* op_mean, void* stream) {
    if (!state) return set_error("gs_wf_power: null state");
    if (check_dims("gs_wf_power", nfields, C, lmax)) return -1;
    if (!moments) return set_error("gs_wf_power: null moments");
    if (!power_of_mean) return set_error("gs_wf_power: null power_of_mean");
    if (!mean_power) return set_error("gs_wf_power: null mean_power");
    if (!op_mean) return set_error("gs_wf_power: null op_mean");
    with_F(nfields, [&](auto f) {
        hipLaunchKernelGGL((k_wf_power<decltype(f)::value>), dim3(nblk(lmax + 1, BS)), dim3(BS), 0,
                           (hipStream_t)stream, (const double*)state, C, lmax, moments, power_of_mean, mean_power,
                           op_mean);
    });
    GS_LAUNCH_CHECK("k_wf_power");
    return 0;
}

}  // extern "C"
