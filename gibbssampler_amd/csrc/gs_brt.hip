// gs_brt.hip -- Blackwell-Rao sample bank: the likelihood of theory spectra that
// live on the device (gfx950).  The two ends of BlackwellRaoSamples.loglike /
// loglike_grad that engine.br_likelihood_tables and engine.br_likelihood_grad run
// on the host in numpy, as kernels: theory D -> tables (Y, cst) in front of
// gs_brs_eval, and xbar -> d loglike / d D behind gs_brs_grad_finish.  Nothing is
// read back and nothing is allocated: a call sequence over these kernels and the
// unchanged gs_brs_* / gs_brl_finish can be captured in a hipGraph.
//
// Per used column j (the bank's tables; they do not depend on a theory):
//   cols[j]  the entry spectrum * maxbins + bin of D (and of the scale ring)
//   kind[j]  1 an inverse-Gamma bin, 2 the TT column of a TEB block, 0 the EE or
//            TE column of a block (its TT column does the block's work)
//   part [2][Ju]  kind 2: the positions j' of the block's EE and TE columns
//   cons [2][Ju]  h = n_b / 2 (n_b = l1^2 - l0^2; alpha + 1 = h, nu = 2 h - 3) and
//                 c0, the part of the column's cst term that no theory enters:
//                 kind 1: -lgamma(alpha);  kind 2: -nu log 2 - logGamma_2(nu / 2)
//   inv [nspec * maxbins]  the position j of an entry of D, -1 for an unused one
//
// k_brt_tables, one workgroup per model k, one thread per used column (bin or TEB
// block; the kind 0 threads idle), 256 columns at a time.  Every line one rounded
// operation in the order of engine.br_likelihood_tables, so Y has the host's bits:
//   kind 1:  Y_j = 1 / D                         term = c0 - h log D
//   kind 2:  det = TT EE - TE TE                 term = c0 - h log det
//            Y_TT = (EE / 2) / det,  Y_EE = (TT / 2) / det,  Y_TE = -TE / det
// Y [K][Ju] is the layout k_brs_eval / k_brs_grad read (row stride Ju; the bank's
// padding columns Ju .. Jp - 1 exist in X alone, where they are 0).  The terms of a
// chunk go through LDS and THREAD 0 ADDS THEM IN COLUMN ORDER from 0.0, one rounded
// addition each: cst[k] has a fixed summation order and no atomics.  (The host
// adds the same terms with math.fsum; the two differ by at most (Ju - 1) 2^-53 sum
// |terms| plus the 1 ulp of the device's log.)
// The validity decision of samplers._br_theory_values, as a flag instead of a
// raise: a used value that is not finite, a kind 1 D <= 0, a block with TT <= 0, EE
// <= 0 or det <= 0 (not positive definite) sets bad[k] = 1; then cst[k] and the
// whole row Y[k][.] are NaN (the row is rewritten after the flag is known), the
// evaluator's t is NaN for every sample and loglike[k] is NaN.  An index of the
// tables that points outside D or outside [0, Ju) is treated the same way and
// never dereferenced.
//
// k_brt_mref: mref[k] = max_c m[c][k] over the chains with S[c][k] > 0 of a state
// in the layout of gs_brl_bytes, 0 where no chain holds a sample -- the reference
// gs_brs_grad takes, as loglike_grad forms it with torch.
//
// k_brt_chain, one thread per (model, entry e of D): the chain rule of
// engine.br_likelihood_grad, every line one rounded operation in that function's
// order (the host's bits for the same xbar):
//   unused entry: grad = 0.0 exactly,  mean = NaN
//   kind 1:  grad = xbar / (D D) - h / D
//   kind 2:  I = D^-1 = [[EE, -TE], [-TE, TT]] / det,  A = I Psi,  Psi = [[xbar_TT,
//            xbar_TE], [xbar_TE, xbar_EE]]
//            grad_TT = (A00 I00 + A01 I01) / 2 - h I00
//            grad_EE = (A10 I01 + A11 I11) / 2 - h I11
//            grad_TE = (A00 I01 + A01 I11) - 2 h I01
//            written by the block's TT thread; the kind 0 threads write mean alone
//   mean[k][e] = xbar[k][j] (the likelihood-weighted mean scale, optional output)
// A bad model's used entries are NaN in grad.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string>

#include "gibbs_capi.h"
#include "gs_common.h"
#include "gs_launch.h"

using gs_detail::set_error;

namespace {

constexpr int HDR = 8;        // header doubles of the gs_brl state
constexpr int BS = 256;       // threads per workgroup

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool finite(double v) { return fabs(v) < __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double quo(double a, double b) { return __ddiv_rn(a, b); }

// the entries of a block whose TT column is j: false when an index leaves its array
__device__ __forceinline__ bool block_cols(int j, int Ju, int nsb, const int* __restrict__ cols,
                                           const int* __restrict__ part, int& jee, int& jte, int& ctt, int& cee,
                                           int& cte) {
    jee = part[j];
    jte = part[Ju + j];
    ctt = cols[j];
    if (jee < 0 || jee >= Ju || jte < 0 || jte >= Ju || ctt < 0 || ctt >= nsb) return false;
    cee = cols[jee];
    cte = cols[jte];
    return cee >= 0 && cee < nsb && cte >= 0 && cte < nsb;
}

__global__ __launch_bounds__(BS) void k_brt_tables(const double* __restrict__ D, int nsb, int Ju,
                                                   const int* __restrict__ cols, const int* __restrict__ kind,
                                                   const int* __restrict__ part, const double* __restrict__ cons,
                                                   double* __restrict__ Y, double* __restrict__ cst,
                                                   int* __restrict__ bad) {
    __shared__ double s_term[BS];
    __shared__ int s_kd[BS];
    __shared__ int s_bad;
    const int t = threadIdx.x, k = blockIdx.x;
    const double* Dk = D + (long long)k * nsb;
    double* Yk = Y + (long long)k * Ju;
    if (t == 0) s_bad = 0;
    __syncthreads();
    double acc = 0.0;
    for (int j0 = 0; j0 < Ju; j0 += BS) {
        const int j = j0 + t;
        double term = 0.0;
        int kd = 0;
        bool ok = true;
        if (j < Ju) {
            kd = kind[j];
            const double h = cons[j], c0 = cons[Ju + j];
            if (kd == 1) {
                const int col = cols[j];
                const double d = (col >= 0 && col < nsb) ? Dk[col] : qnan();
                ok = pos_finite(d);
                Yk[j] = quo(1.0, d);
                term = sub(c0, mul(h, log(d)));
            } else if (kd == 2) {
                int jee, jte, ctt, cee, cte;
                if (block_cols(j, Ju, nsb, cols, part, jee, jte, ctt, cee, cte)) {
                    const double tt = Dk[ctt], ee = Dk[cee], te = Dk[cte];
                    const double det = sub(mul(tt, ee), mul(te, te));
                    ok = pos_finite(tt) && pos_finite(ee) && finite(te) && pos_finite(det);
                    Yk[j] = quo(mul(0.5, ee), det);
                    Yk[jee] = quo(mul(0.5, tt), det);
                    Yk[jte] = quo(-te, det);
                    term = sub(c0, mul(h, log(det)));
                } else {
                    ok = false;
                }
            } else if (kd != 0) {
                ok = false;
            }
        }
        if (!ok) s_bad = 1;                                    // every writer stores the same value
        s_term[t] = term;
        s_kd[t] = kd;
        __syncthreads();
        if (t == 0) {
            const int jn = Ju - j0 < BS ? Ju - j0 : BS;
            for (int jj = 0; jj < jn; ++jj)
                if (s_kd[jj] != 0) acc = add(acc, s_term[jj]);
        }
        __syncthreads();
    }
    const bool isbad = s_bad != 0;                             // behind the loop's closing barrier
    if (isbad)
        for (int j = t; j < Ju; j += BS) Yk[j] = qnan();
    if (t == 0) {
        cst[k] = isbad ? qnan() : acc;
        bad[k] = isbad ? 1 : 0;
    }
}

__global__ __launch_bounds__(BS) void k_brt_mref(const double* __restrict__ state, int C, int K,
                                                 double* __restrict__ mref) {
    const int k = blockIdx.x * BS + threadIdx.x;
    if (k >= K) return;
    const double* fm = state + HDR;
    const double* fS = fm + (long long)C * K;
    bool any = false;
    double M = 0.0;
    for (int c = 0; c < C; ++c) {
        if (fS[(long long)c * K + k] > 0.0) {
            const double v = fm[(long long)c * K + k];
            // torch.amax: a NaN wins
            M = any ? ((v != v || M != M) ? qnan() : fmax(M, v)) : v;
            any = true;
        }
    }
    mref[k] = M;
}

__global__ __launch_bounds__(BS) void k_brt_chain(const double* __restrict__ D, const double* __restrict__ xbar,
                                                  const int* __restrict__ bad, int nsb, int Ju, long long total,
                                                  const int* __restrict__ cols, const int* __restrict__ kind,
                                                  const int* __restrict__ part, const double* __restrict__ cons,
                                                  const int* __restrict__ inv, double* __restrict__ grad,
                                                  double* __restrict__ mean) {
    const long long i = (long long)blockIdx.x * BS + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i / nsb), e = (int)(i - (long long)k * nsb);
    const int j = inv[e];
    if (j < 0 || j >= Ju) {
        grad[i] = 0.0;
        if (mean) mean[i] = qnan();
        return;
    }
    const double* Dk = D + (long long)k * nsb;
    const double* xk = xbar + (long long)k * Ju;
    double* gk = grad + (long long)k * nsb;
    if (mean) mean[i] = xk[j];
    const bool isbad = bad[k] != 0;
    const int kd = kind[j];
    const double h = cons[j];
    if (kd == 1) {
        const double d = Dk[e];
        gk[e] = isbad ? qnan() : sub(quo(xk[j], mul(d, d)), quo(h, d));
    } else if (kd == 2) {
        int jee, jte, ctt, cee, cte;
        if (!block_cols(j, Ju, nsb, cols, part, jee, jte, ctt, cee, cte) || ctt != e) {
            gk[e] = qnan();                                    // tables that do not describe a block
            return;
        }
        if (isbad) {
            gk[ctt] = qnan(); gk[cee] = qnan(); gk[cte] = qnan();
            return;
        }
        const double tt = Dk[ctt], ee = Dk[cee], te = Dk[cte];
        const double ptt = xk[j], pee = xk[jee], pte = xk[jte];
        const double det = sub(mul(tt, ee), mul(te, te));
        const double i00 = quo(ee, det), i11 = quo(tt, det), i01 = quo(-te, det);
        const double a00 = add(mul(i00, ptt), mul(i01, pte)), a01 = add(mul(i00, pte), mul(i01, pee));
        const double a10 = add(mul(i01, ptt), mul(i11, pte)), a11 = add(mul(i01, pte), mul(i11, pee));
        gk[ctt] = sub(mul(0.5, add(mul(a00, i00), mul(a01, i01))), mul(h, i00));
        gk[cee] = sub(mul(0.5, add(mul(a10, i01), mul(a11, i11))), mul(h, i11));
        gk[cte] = sub(add(mul(a00, i01), mul(a01, i11)), mul(mul(2.0, h), i01));
    }
    // kind 0: the block's TT thread writes this entry
}

int check_dims(const char* what, int K, int nspec, int maxbins, int Ju) {
    if (K < 1) return set_error(std::string(what) + ": models K >= 1 needed");
    if (nspec < 1 || nspec > 32 || maxbins < 1)
        return set_error(std::string(what) + ": maxbins >= 1 and nspec in [1, 32] out of range");
    if ((long long)nspec * maxbins > (1LL << 24)) return set_error(std::string(what) + ": too many entries per theory");
    if (Ju < 1 || Ju > nspec * maxbins)
        return set_error(std::string(what) + ": used columns Ju out of range [1, nspec * maxbins]");
    if ((long long)K * nspec * maxbins > (1LL << 37)) return set_error(std::string(what) + ": theory [K][nspec][maxbins] too large");
    return 0;
}

}  // namespace

extern "C" {

int gs_brt_tables(const double* D, int K, int nspec, int maxbins, int Ju, const int* cols, const int* kind,
                  const int* part, const double* cons, double* Y, double* cst, int* bad, void* stream) {
    if (!D || !Y || !cst || !bad) return set_error("gs_brt_tables: null theory or output");
    if (!cols || !kind || !part || !cons) return set_error("gs_brt_tables: null table");
    if (check_dims("gs_brt_tables", K, nspec, maxbins, Ju)) return -1;
    hipLaunchKernelGGL(k_brt_tables, dim3((unsigned)K), dim3(BS), 0, (hipStream_t)stream, D, nspec * maxbins, Ju, cols,
                       kind, part, cons, Y, cst, bad);
    GS_LAUNCH_CHECK("k_brt_tables");
    return 0;
}

int gs_brt_mref(const void* state, int C, int K, double* mref, void* stream) {
    if (!state || !mref) return set_error("gs_brt_mref: null argument");
    if (C < 1 || K < 1) return set_error("gs_brt_mref: C and K >= 1 needed");
    if ((long long)C * K > (1LL << 28)) return set_error("gs_brt_mref: too many (chain, model) pairs");
    hipLaunchKernelGGL(k_brt_mref, dim3((unsigned)((K + BS - 1) / BS)), dim3(BS), 0, (hipStream_t)stream,
                       (const double*)state, C, K, mref);
    GS_LAUNCH_CHECK("k_brt_mref");
    return 0;
}

int gs_brt_chain(const double* D, const double* xbar, const int* bad, int K, int nspec, int maxbins, int Ju,
                 const int* cols, const int* kind, const int* part, const double* cons, const int* inv, double* grad,
                 double* mean, void* stream) {
    if (!D || !xbar || !bad || !grad) return set_error("gs_brt_chain: null theory, xbar, bad or grad");
    if (!cols || !kind || !part || !cons || !inv) return set_error("gs_brt_chain: null table");
    if (check_dims("gs_brt_chain", K, nspec, maxbins, Ju)) return -1;
    const long long total = (long long)K * nspec * maxbins;
    hipLaunchKernelGGL(k_brt_chain, dim3((unsigned)((total + BS - 1) / BS)), dim3(BS), 0, (hipStream_t)stream, D, xbar,
                       bad, nspec * maxbins, Ju, total, cols, kind, part, cons, inv, grad, mean);
    GS_LAUNCH_CHECK("k_brt_chain");
    return 0;
}

}  // extern "C"
