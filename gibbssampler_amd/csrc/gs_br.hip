// gs_br.hip -- streaming Blackwell-Rao marginal posteriors of the D_l (gfx950).
//
// The centered C_l draw samples D_b | s from an inverse-Gamma(alpha_b, beta_b):
// beta_b is the scale the draw records in the scale trace (gs_cls_scale_trace)
// and alpha_b depends on the bin alone.  The Blackwell-Rao estimate of the
// marginal posterior averages that conditional density over the sky samples,
//   P(D | d) ~ 1/N sum_i IG(D; alpha, beta_i),
//   log IG(D; alpha, beta) = alpha log beta - beta / D - lgamma(alpha) - (alpha + 1) log D,
// on a grid of G values of D per (spectrum, bin), 1 <= G <= 64.
//
// A *series* is one (chain, spectrum, bin), s = (chain * nspec + spectrum) *
// maxbins + bin, ns = nchains * nspec * maxbins, nsb = nspec * maxbins; an
// *element* is one (series, grid point), e = s * G + g, g fastest.
// Inputs shared by the update and the finish (device, fp64):
//   grid  [nsb][G]   D_g > 0
//   alpha [nsb]      the shape; NaN: the series is skipped and finishes as NaN
//   half_mask        bit k set: the recorded scale of spectrum k is twice the
//                    conditional's scale (the diagonal of the TEB block's
//                    inverse-Wishart scale Psi: beta = Psi_ii / 2, exact)
//
// State (caller-owned device buffer of gs_br_bytes bytes):
//   header   8 doubles: [0] int64 n, the iterations added (one count for the
//            whole state); [1] uint32 launch ticket; the rest reserved (0)
//   m        [ns * G]  running maximum of t_i
//   S        [ns * G]  sum_i exp(t_i - m);  S == 0: no sample yet
//   bad      int64 [nchains][nspec]  rows skipped: beta <= 0 or not finite
// with t_i = alpha log beta_i - beta_i / D_g.  The part of the log density that
// does not depend on the sample, -lgamma(alpha) - (alpha + 1) log D_g, is not
// streamed: the finish adds it.  gs_br_reset zeroes all of it.
//
// k_br_update, per element in iteration order:
//   rD   = 1 / D_g                               (once per launch)
//   lb_i = log(beta_i)                           (once per series and row: staged)
//   t    = fma(-beta_i, rD, alpha * lb_i)
//   S == 0:  m = t, S = 1
//   else     d = t - m,  w = exp(-|d|);  d > 0:  S = fma(S, w, 1), m = t;  else  S = S + w
// A workgroup owns BS consecutive elements, i.e. the grid points of up to
// BS / G + 2 consecutive series.  Per tile of TS rows it stages beta and
// log(beta) of those series in LDS -- consecutive lanes read consecutive
// doubles of a ring row, and the logarithm is evaluated once per (series, row),
// not once per grid point -- and then every lane runs the recursion above over
// the tile's rows, reading its series' pair from LDS (the lanes of one series
// read one address: a broadcast).  The order of the operations on an element
// is the iteration order whatever the launch or the tile carries, so the
// state's bits do not depend on how the iterations were cut into launches.
//
// k_br_finish, one thread per (spectrum, bin, g) over C chains in chain order;
// chains with S_c == 0 are left out; n is the header's count:
//   M      = max_c m_c
//   sum    = sum_c S_c exp(m_c - M)
//   logpdf = (((M + log sum) - log(C n)) - lgamma(alpha)) - (alpha + 1) log D_g
// NaN when alpha is NaN, n == 0 or no chain has a sample.  k_br_mass, one
// thread per (spectrum, bin), in g order:
//   mass = sum_{g < G - 1} 0.5 (exp(logpdf_g) + exp(logpdf_g+1)) (D_g+1 - D_g)
// Every operation of the two is a single rounded add / multiply in the order
// written here (no contraction): tests/_blackwell_rao.py restates them.
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
constexpr int BS = 256;      // elements per workgroup
constexpr int TS = 8;        // rows per staged tile
constexpr int NSER = BS + 1; // series a workgroup can touch (G = 1: BS; G > 1: at most BS / G + 2)

__global__ __launch_bounds__(BS) void k_br_update(double* __restrict__ state, long long ns, int nsb, int maxbins,
                                                  int nspec, int G, const double* __restrict__ grid,
                                                  const double* __restrict__ alpha, unsigned half_mask,
                                                  const double* __restrict__ scales, int cap, int slot0,
                                                  int nsteps) {
    __shared__ double s_b[TS][NSER];
    __shared__ double s_lb[TS][NSER];
    const long long n0 = *(volatile const long long*)state;
    const long long ne = ns * G;
    double* fm = state + HDR;
    double* fS = fm + ne;
    const long long e0 = (long long)blockIdx.x * BS, e = e0 + threadIdx.x;
    const long long s_lo = e0 / G;
    const long long e_hi = (e0 + BS - 1 < ne - 1) ? e0 + BS - 1 : ne - 1;
    const int nser = (int)(e_hi / G - s_lo) + 1;           // <= NSER
    const bool in = e < ne;
    const long long s = in ? e / G : s_lo;
    const int g = in ? (int)(e - s * G) : 0;
    const int sl = (int)(s - s_lo);
    const int sb = (int)(s % nsb);
    const double a = in ? alpha[sb] : __longlong_as_double(0x7ff8000000000000LL);
    const bool active = in && a == a;
    const double rD = active ? 1.0 / grid[(long long)sb * G + g] : 0.0;
    double m = active ? fm[e] : 0.0, S = active ? fS[e] : 0.0;
    long long nbad = 0;
    for (int t0 = 0; t0 < nsteps; t0 += TS) {
        const int tn = nsteps - t0 < TS ? nsteps - t0 : TS;
        __syncthreads();                                   // the previous tile has been read
        for (int idx = threadIdx.x; idx < tn * nser; idx += BS) {
            const int j = idx / nser, q = idx - j * nser;
            const long long sq = s_lo + q;
            int slot = slot0 + t0 + j;
            if (slot >= cap) slot -= cap;                  // slot0 < cap and nsteps <= cap: one wrap
            const int sp = (int)((sq % nsb) / maxbins);
            double b = scales[(long long)slot * ns + sq];
            if ((half_mask >> sp) & 1u) b *= 0.5;
            const bool ok = b > 0.0 && b < __longlong_as_double(0x7ff0000000000000LL);
            s_b[j][q] = b;
            s_lb[j][q] = ok ? log(b) : __longlong_as_double(0x7ff8000000000000LL);
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < tn; ++j) {
                const double lb = s_lb[j][sl];
                if (lb == lb) {
                    const double t = fma(-s_b[j][sl], rD, a * lb);
                    if (S == 0.0) {
                        m = t;
                        S = 1.0;
                    } else {
                        const double d = t - m;
                        const double w = exp(-fabs(d));
                        if (d > 0.0) {
                            S = fma(S, w, 1.0);
                            m = t;
                        } else {
                            S = S + w;
                        }
                    }
                } else if (g == 0) {
                    ++nbad;
                }
            }
        }
    }
    if (active) {
        fm[e] = m;
        fS[e] = S;
        if (nbad) {
            unsigned long long* bad = (unsigned long long*)(fS + ne);
            atomicAdd(&bad[s / maxbins], (unsigned long long)nbad);     // s / maxbins = chain * nspec + spectrum
        }
    }
    // the last workgroup to finish advances n: every workgroup read it at its start
    __syncthreads();
    if (threadIdx.x == 0) {
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

__global__ __launch_bounds__(BS) void k_br_finish(const double* __restrict__ state, int C, long long nsb, int G,
                                                  const double* __restrict__ grid, const double* __restrict__ alpha,
                                                  double* __restrict__ logpdf) {
    const long long eg = (long long)blockIdx.x * BS + threadIdx.x;      // (spectrum, bin, g)
    const long long neg = nsb * G;
    if (eg >= neg) return;
    const long long n = *(const long long*)state;
    const long long ne = (long long)C * neg;
    const double* fm = state + HDR;
    const double* fS = fm + ne;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double a = alpha[eg / G];
    double out = qnan;
    if (a == a && n > 0) {
        bool any = false;
        double M = 0.0;
        for (int c = 0; c < C; ++c) {
            const long long e = c * neg + eg;
            if (fS[e] > 0.0) {
                M = any ? fmax(M, fm[e]) : fm[e];
                any = true;
            }
        }
        if (any) {
            double sum = 0.0;
            for (int c = 0; c < C; ++c) {
                const long long e = c * neg + eg;
                if (fS[e] > 0.0) sum = add(sum, mul(fS[e], exp(sub(fm[e], M))));
            }
            const double lse = add(M, log(sum));
            const double norm = log(mul((double)C, (double)n));
            out = sub(sub(sub(lse, norm), lgamma(a)), mul(add(a, 1.0), log(grid[eg])));
        }
    }
    logpdf[eg] = out;
}

__global__ __launch_bounds__(BS) void k_br_mass(long long nsb, int G, const double* __restrict__ grid,
                                                const double* __restrict__ logpdf, double* __restrict__ mass) {
    const long long sb = (long long)blockIdx.x * BS + threadIdx.x;
    if (sb >= nsb) return;
    const double* D = grid + sb * G;
    const double* lp = logpdf + sb * G;
    double acc = lp[0] == lp[0] ? 0.0 : lp[0];             // a NaN series has a NaN mass
    double p0 = exp(lp[0]);
    for (int g = 0; g + 1 < G; ++g) {
        const double p1 = exp(lp[g + 1]);
        acc = add(acc, mul(mul(0.5, add(p0, p1)), sub(D[g + 1], D[g])));
        p0 = p1;
    }
    mass[sb] = acc;
}

int check_dims(const char* what, long long nchains, int nspec, int maxbins, int G) {
    if (nchains < 1 || nspec < 1 || nspec > 32 || maxbins < 1)
        return set_error(std::string(what) + ": nchains, maxbins >= 1 and nspec in [1, 32] out of range");
    if (G < 1 || G > 64) return set_error(std::string(what) + ": grid points G out of range [1, 64]");
    if (nchains * nspec * maxbins > (1LL << 28)) return set_error(std::string(what) + ": too many series");
    return 0;
}

long long state_bytes(long long nchains, int nspec, int maxbins, int G) {
    const long long ne = nchains * nspec * maxbins * G;
    return 8LL * (HDR + 2 * ne + nchains * nspec);
}

}  // namespace

extern "C" {

int gs_br_bytes(int nchains, int nspec, int maxbins, int G, long long* bytes) {
    if (!bytes) return set_error("gs_br_bytes: null argument");
    if (check_dims("gs_br_bytes", nchains, nspec, maxbins, G)) return -1;
    *bytes = state_bytes(nchains, nspec, maxbins, G);
    return 0;
}

int gs_br_reset(void* state, int nchains, int nspec, int maxbins, int G, void* stream) {
    if (!state) return set_error("gs_br_reset: null state");
    if (check_dims("gs_br_reset", nchains, nspec, maxbins, G)) return -1;
    GS_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(nchains, nspec, maxbins, G), (hipStream_t)stream));
    return 0;
}

int gs_br_update(void* state, int nchains, int nspec, int maxbins, int G, const double* grid, const double* alpha,
                 unsigned half_mask, const double* scales, int capacity, uint32_t first_iteration, int nsteps,
                 void* stream) {
    if (!state) return set_error("gs_br_update: null state");
    if (check_dims("gs_br_update", nchains, nspec, maxbins, G)) return -1;
    if (nsteps == 0) return 0;
    if (!grid || !alpha || !scales) return set_error("gs_br_update: null grid, alpha or scale trace");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_br_update: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    const long long ns = (long long)nchains * nspec * maxbins, ne = ns * G;
    const unsigned nb = nblk(ne, BS);
    if ((ne + BS - 1) / BS != nb) return set_error("gs_br_update: too many series for one launch");
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    hipLaunchKernelGGL(k_br_update, dim3(nb), dim3(BS), 0, (hipStream_t)stream, (double*)state, ns, nspec * maxbins,
                       maxbins, nspec, G, grid, alpha, half_mask, scales, capacity, slot0, nsteps);
    GS_LAUNCH_CHECK("k_br_update");
    return 0;
}

int gs_br_finish(const void* state, int C, int nspec, int maxbins, int G, const double* grid, const double* alpha,
                 double* logpdf, double* mass, void* stream) {
    if (!state) return set_error("gs_br_finish: null state");
    if (check_dims("gs_br_finish", C, nspec, maxbins, G)) return -1;
    if (!grid || !alpha || !logpdf || !mass) return set_error("gs_br_finish: null grid, alpha or output");
    const long long nsb = (long long)nspec * maxbins;
    hipLaunchKernelGGL(k_br_finish, dim3(nblk(nsb * G, BS)), dim3(BS), 0, (hipStream_t)stream, (const double*)state,
                       C, nsb, G, grid, alpha, logpdf);
    GS_LAUNCH_CHECK("k_br_finish");
    hipLaunchKernelGGL(k_br_mass, dim3(nblk(nsb, BS)), dim3(BS), 0, (hipStream_t)stream, nsb, G, grid,
                       (const double*)logpdf, mass);
    GS_LAUNCH_CHECK("k_br_mass");
    return 0;
}

}  // extern "C"
