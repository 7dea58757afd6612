// gs_summary.hip -- streaming posterior summaries of the D_l chains (gfx950).
//
// A *series* is one (chain, spectrum, bin); ns = nchains * nspec * maxbins and
// series s = (chain * nspec + spectrum) * maxbins + bin, so consecutive lanes
// read consecutive doubles of a trace row.  K = max_lag, 0 <= K <= 64.
//
// State (caller-owned device buffer of gs_summary_bytes bytes, fp64 unless noted):
//   header   8 doubles: [0] int64 n, the samples summarised (one count for the
//            whole state); [1] uint32 launch ticket; the rest reserved (0)
//   fields   [6 + 3K][ns], series fastest:
//              0 r      the series' first summarised sample
//              1 mean   Welford mean of x
//              2 M2     Welford sum of squared deviations
//              3 min    4 max
//              5 S      sum of y_t, y_t = x_t - r
//              6 + (j-1)       P_j = sum_{t > j} y_t y_{t-j},  j = 1..K
//              6 + K + i       head[i] = y_{i+1}, the first K values
//              6 + 2K + i      ring[i] = y_{n-i}, the last K values (0 newest)
//   counts   int64 [nchains][nacc] accept counts
// gs_summary_reset zeroes all of it (head / ring entries that do not exist yet
// read as 0, so their lag products add +0).
//
// k_summary_update, per series in iteration order (t = n + 1, n + 2, ...):
//   r = x_1;  d = x_t - mean;  mean += d / t;  M2 += d (x_t - mean);
//   S += y_t;  P_j = fma(y_t, y_{t-j}, P_j)
// The order of the adds into every accumulator is the iteration order whatever
// the launch carries, so the state's bits do not depend on how the iterations
// were cut into launches.  The lag products run in register tiles: the previous
// K values and TL rows live in VGPRs with static indexing (a launch's tail of
// fewer than TL rows takes the TL = 1 form: the same adds in the same order),
// and P, head and ring are read and written once per launch.  K > 32 runs two
// passes of 32 lags over the launch's rows so that one pass holds 64 previous
// values + 32 sums + the tile (about 210 VGPRs; the grid is two waves per SIMD
// at the flagship shape, so occupancy is not what limits it).
//
// k_summary_finish, one thread per (spectrum, bin) over C chains of n samples:
//   s_c^2   = M2_c / (n - 1)                      chain_var
//   g_0,c   = M2_c / n
//   delta_c = mean_c - r_c
//   g_j,c   = (P_j - delta_c ((S - sum head[0..j)) + (S - sum ring[0..j)))
//              + (n - j) delta_c^2) / n           (NaN when n <= j)
//   mean    = mean_c mean_c
//   var     = (sum_c M2_c + n sum_c (mean_c - mean)^2) / (C n - 1)
//   W       = mean_c s_c^2
//   B/n     = sum_c (mean_c - mean)^2 / (C - 1)   (taken as 0 in var+ when C = 1)
//   var+    = mean_c g_0,c + B/n                  (mean_c g_0,c = (n-1)/n W)
//   rhat    = sqrt(var+ / W)                      (NaN when C = 1)
//   rho_j   = 1 - (mean_c g_0,c - mean_c g_j,c) / var+     (C = 1: g_j / g_0)
//   Geyer:  G_k = rho_2k + rho_2k+1 for 2k + 1 <= min(K, n - 1), stop at the
//           first G_k < 0 (or NaN), G_k <- min(G_k, G_k-1);
//           tau = -1 + 2 sum G_k;  ess = C n / tau (NaN without a pair);
//           ess_truncated = 1 when no negative pair was met
//   W == 0: rhat, ess and rho are NaN (ess_truncated 0); mean and var are exact.
// Every operation of the finish is a single rounded add / multiply / divide in
// the order written here (no contraction): tests/_summary.py restates it.
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
constexpr int NFIX = 6;      // r, mean, M2, min, max, S
constexpr int BS = 64;       // one wave per workgroup
constexpr int TL = 8;        // rows per register tile
enum { F_R = 0, F_MEAN = 1, F_M2 = 2, F_MIN = 3, F_MAX = 4, F_S = 5 };

__host__ __device__ inline long long nfields_of(int K) { return NFIX + 3LL * K; }

// TLN rows y[0..TLN) (iteration order) into the JB lag sums P (lags J0 + 1 ..
// J0 + JB); prev[i] = the value i + 1 rows before y[0].  Shifts prev by TLN.
template <int KP, int JB, int J0, int TLN>
__device__ __forceinline__ void lag_tile(double (&prev)[KP], double (&P)[JB], const double (&y)[TLN]) {
    static_assert(J0 + JB <= KP, "lags past the kept values");
#pragma unroll
    for (int t = 0; t < TLN; ++t) {
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int j = J0 + jj + 1;       // y_{t-j}: inside the tile when t >= j, else prev[j - t - 1]
            const double partner = t >= j ? y[t >= j ? t - j : 0] : prev[t >= j ? 0 : j - t - 1];
            P[jj] = fma(y[t], partner, P[jj]);
        }
    }
#pragma unroll
    for (int i = KP - 1; i >= 0; --i) prev[i] = (i >= TLN) ? prev[i >= TLN ? i - TLN : 0] : y[i >= TLN ? 0 : TLN - 1 - i];
}

// one pass: lags j0 + 1 .. j0 + JB of series s over the launch's rows
template <int KP, int JB, int J0>
__device__ __forceinline__ void lag_pass(double* __restrict__ fld, long long ns, long long s, int K,
                                         const double* __restrict__ trace, int cap, int slot0, int nsteps, double r,
                                         bool store_ring) {
    double prev[KP], P[JB];
#pragma unroll
    for (int i = 0; i < KP; ++i) prev[i] = i < K ? fld[(NFIX + 2LL * K + i) * ns + s] : 0.0;
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) P[jj] = (J0 + jj) < K ? fld[(NFIX + J0 + jj) * ns + s] : 0.0;
    int slot = slot0, i = 0;
    for (; i + TL <= nsteps; i += TL) {
        double y[TL];
#pragma unroll
        for (int t = 0; t < TL; ++t) {
            y[t] = trace[(long long)slot * ns + s] - r;
            slot = slot + 1 == cap ? 0 : slot + 1;
        }
        lag_tile<KP, JB, J0, TL>(prev, P, y);
    }
    for (; i < nsteps; ++i) {
        double y[1];
        y[0] = trace[(long long)slot * ns + s] - r;
        slot = slot + 1 == cap ? 0 : slot + 1;
        lag_tile<KP, JB, J0, 1>(prev, P, y);
    }
#pragma unroll
    for (int jj = 0; jj < JB; ++jj)
        if (J0 + jj < K) fld[(NFIX + J0 + jj) * ns + s] = P[jj];
    if (store_ring) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) fld[(NFIX + 2LL * K + k) * ns + s] = prev[k];
    }
}

// grid: nbs workgroups of series, then the workgroups of the accept counts
template <int KP>
__global__ __launch_bounds__(BS) void k_summary_update(double* __restrict__ state, long long ns, int K,
                                                       const double* __restrict__ trace, int cap, int slot0,
                                                       int nsteps, const int32_t* __restrict__ acc,
                                                       long long acc_stride, long long nca, unsigned nbs) {
    const long long n0 = *(volatile const long long*)state;
    double* fld = state + HDR;
    if (blockIdx.x < nbs) {
        const long long s = (long long)blockIdx.x * BS + threadIdx.x;
        if (s < ns) {
            // moments, S and the head: one pass over the rows
            double r = fld[F_R * ns + s], mean = fld[F_MEAN * ns + s], M2 = fld[F_M2 * ns + s];
            double mn = fld[F_MIN * ns + s], mx = fld[F_MAX * ns + s], S = fld[F_S * ns + s];
            int slot = slot0;
            for (int i = 0; i < nsteps; ++i) {
                const double x = trace[(long long)slot * ns + s];
                slot = slot + 1 == cap ? 0 : slot + 1;
                const long long t = n0 + i;          // samples before this one
                if (t == 0) {
                    r = x;
                    mn = x;
                    mx = x;
                }
                const double y = x - r;
                const double d = x - mean;
                mean += d / (double)(t + 1);
                M2 += d * (x - mean);
                mn = fmin(mn, x);
                mx = fmax(mx, x);
                S += y;
                if (t < K) fld[(NFIX + K + t) * ns + s] = y;
            }
            fld[F_R * ns + s] = r;
            fld[F_MEAN * ns + s] = mean;
            fld[F_M2 * ns + s] = M2;
            fld[F_MIN * ns + s] = mn;
            fld[F_MAX * ns + s] = mx;
            fld[F_S * ns + s] = S;
            if (K > 0) {
                if constexpr (KP <= 32) {
                    lag_pass<KP, KP, 0>(fld, ns, s, K, trace, cap, slot0, nsteps, r, true);
                } else {
                    lag_pass<KP, 32, 0>(fld, ns, s, K, trace, cap, slot0, nsteps, r, false);
                    lag_pass<KP, 32, 32>(fld, ns, s, K, trace, cap, slot0, nsteps, r, true);
                }
            }
        }
    } else if (acc != nullptr) {
        const long long a = (long long)(blockIdx.x - nbs) * BS + threadIdx.x;
        if (a < nca) {
            long long* cnt = (long long*)(fld + nfields_of(K) * ns);
            long long sum = 0;
            for (int i = 0; i < nsteps; ++i) sum += acc[(long long)i * acc_stride + a];
            cnt[a] += sum;
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

__global__ __launch_bounds__(BS) void k_summary_finish(const double* __restrict__ state, int C, long long nsb, int K,
                                                       double* __restrict__ pooled, double* __restrict__ chain_mean,
                                                       double* __restrict__ chain_var, double* __restrict__ acf,
                                                       double* __restrict__ gamma) {
    const long long sb = (long long)blockIdx.x * BS + threadIdx.x;
    if (sb >= nsb) return;
    const long long n = *(const long long*)state;
    const double* fld = state + HDR;
    const long long ns = (long long)C * nsb;
    const double nd = (double)n, Cd = (double)C, qnan = __longlong_as_double(0x7ff8000000000000LL);
    double sum_mean = 0.0, sum_M2 = 0.0, sum_var = 0.0, sum_g0 = 0.0, mn = 0.0, mx = 0.0;
    for (int c = 0; c < C; ++c) {
        const long long s = c * nsb + sb;
        const double m = fld[F_MEAN * ns + s], M2 = fld[F_M2 * ns + s];
        const double v = n >= 2 ? M2 / sub(nd, 1.0) : qnan;
        chain_mean[s] = m;
        chain_var[s] = v;
        sum_mean = add(sum_mean, m);
        sum_M2 = add(sum_M2, M2);
        sum_var = add(sum_var, v);
        sum_g0 = add(sum_g0, M2 / nd);
        const double lo = fld[F_MIN * ns + s], hi = fld[F_MAX * ns + s];
        mn = c == 0 ? lo : fmin(mn, lo);
        mx = c == 0 ? hi : fmax(mx, hi);
    }
    const double mean = sum_mean / Cd;
    double sb2 = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = sub(fld[F_MEAN * ns + c * nsb + sb], mean);
        sb2 = add(sb2, mul(d, d));
    }
    const double W = sum_var / Cd, g0 = sum_g0 / Cd;
    const double var = n >= 1 && (long long)C * n >= 2 ? add(sum_M2, mul(nd, sb2)) / sub(mul(Cd, nd), 1.0) : qnan;
    const double Bn = C > 1 ? sb2 / sub(Cd, 1.0) : 0.0;
    const double varp = add(g0, Bn);
    const bool degenerate = !(W > 0.0);          // W == 0, or NaN (n < 2)
    const double rhat = (C > 1 && !degenerate) ? sqrt(varp / W) : qnan;
    // per-chain autocovariances; acf[j] collects sum_c g_j,c in chain order
    for (int c = 0; c < C; ++c) {
        const long long s = c * nsb + sb;
        const double delta = sub(fld[F_MEAN * ns + s], fld[F_R * ns + s]);
        const double S = fld[F_S * ns + s], d2 = mul(delta, delta);
        const double gc0 = n >= 1 ? fld[F_M2 * ns + s] / nd : qnan;
        gamma[((long long)c * (K + 1)) * nsb + sb] = gc0;
        acf[sb] = c == 0 ? gc0 : add(acf[sb], gc0);
        double hs = 0.0, ts = 0.0;
        for (int j = 1; j <= K; ++j) {
            double g = qnan;
            if (n > j) {
                hs = add(hs, fld[(NFIX + K + j - 1) * ns + s]);
                ts = add(ts, fld[(NFIX + 2LL * K + j - 1) * ns + s]);
                const double cross = mul(delta, add(sub(S, hs), sub(S, ts)));
                const double num = add(sub(fld[(NFIX + j - 1) * ns + s], cross), mul(sub(nd, (double)j), d2));
                g = num / nd;
            }
            gamma[((long long)c * (K + 1) + j) * nsb + sb] = g;
            acf[j * nsb + sb] = c == 0 ? g : add(acf[j * nsb + sb], g);
        }
    }
    for (int j = 0; j <= K; ++j) {
        const double gbar = acf[j * nsb + sb] / Cd;
        acf[j * nsb + sb] = degenerate ? qnan : sub(1.0, sub(g0, gbar) / varp);
    }
    // Geyer's initial monotone positive sequence
    double ess = qnan, trunc = 0.0;
    if (!degenerate) {
        const long long jmax = (long long)K < n - 1 ? (long long)K : n - 1;
        double sum = 0.0, last = 0.0;
        int npairs = 0;
        trunc = 1.0;
        for (long long k = 0; 2 * k + 1 <= jmax; ++k) {
            double G = add(acf[2 * k * nsb + sb], acf[(2 * k + 1) * nsb + sb]);
            if (!(G >= 0.0)) {
                trunc = 0.0;
                break;
            }
            if (npairs > 0) G = fmin(G, last);
            last = G;
            sum = add(sum, G);
            ++npairs;
        }
        if (npairs > 0) ess = mul(Cd, nd) / add(-1.0, mul(2.0, sum));
    }
    pooled[0 * nsb + sb] = mean;
    pooled[1 * nsb + sb] = var;
    pooled[2 * nsb + sb] = mn;
    pooled[3 * nsb + sb] = mx;
    pooled[4 * nsb + sb] = ess;
    pooled[5 * nsb + sb] = trunc;
    pooled[6 * nsb + sb] = rhat;
}

int check_dims(const char* what, long long nchains, int nspec, int maxbins, int nacc, int max_lag) {
    if (nchains < 1 || nspec < 1 || maxbins < 1 || nacc < 0)
        return set_error(std::string(what) + ": nchains, nspec, maxbins >= 1 and nacc >= 0 out of range");
    if (max_lag < 0 || max_lag > 64) return set_error(std::string(what) + ": max_lag out of range [0, 64]");
    if (nchains * nspec * maxbins > (1LL << 40)) return set_error(std::string(what) + ": too many series");
    return 0;
}

long long state_bytes(long long nchains, int nspec, int maxbins, int nacc, int K) {
    const long long ns = nchains * nspec * maxbins;
    return 8LL * (HDR + nfields_of(K) * ns + nchains * nacc);
}

}  // namespace

extern "C" {

int gs_summary_bytes(int nchains, int nspec, int maxbins, int nacc, int max_lag, long long* bytes) {
    if (!bytes) return set_error("gs_summary_bytes: null argument");
    if (check_dims("gs_summary_bytes", nchains, nspec, maxbins, nacc, max_lag)) return -1;
    *bytes = state_bytes(nchains, nspec, maxbins, nacc, max_lag);
    return 0;
}

int gs_summary_reset(void* state, int nchains, int nspec, int maxbins, int nacc, int max_lag, void* stream) {
    if (!state) return set_error("gs_summary_reset: null state");
    if (check_dims("gs_summary_reset", nchains, nspec, maxbins, nacc, max_lag)) return -1;
    GS_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(nchains, nspec, maxbins, nacc, max_lag),
                            (hipStream_t)stream));
    return 0;
}

int gs_summary_update(void* state, int nchains, int nspec, int maxbins, int nacc, int max_lag, const double* trace,
                      int capacity, uint32_t first_iteration, int nsteps, const int32_t* accept_trace,
                      long long accept_stride, void* stream) {
    if (!state) return set_error("gs_summary_update: null state");
    if (check_dims("gs_summary_update", nchains, nspec, maxbins, nacc, max_lag)) return -1;
    if (nsteps == 0) return 0;
    if (!trace) return set_error("gs_summary_update: null trace");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_summary_update: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    if (accept_trace && (nacc < 1 || accept_stride < 0))
        return set_error("gs_summary_update: an accept trace needs nacc >= 1 and a stride >= 0");
    const long long ns = (long long)nchains * nspec * maxbins, nca = accept_trace ? (long long)nchains * nacc : 0;
    const unsigned nbs = nblk(ns, BS), nba = nca ? nblk(nca, BS) : 0;
    if ((ns + BS - 1) / BS != nbs) return set_error("gs_summary_update: too many series for one launch");
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    const int KP = max_lag <= 8 ? 8 : max_lag <= 16 ? 16 : max_lag <= 32 ? 32 : 64;
#define GS_SUMMARY_LAUNCH(KPV)                                                                                   \
    hipLaunchKernelGGL((k_summary_update<KPV>), dim3(nbs + nba), dim3(BS), 0, (hipStream_t)stream, (double*)state, \
                       ns, max_lag, trace, capacity, slot0, nsteps, accept_trace, accept_stride, nca, nbs)
    if (KP == 8) GS_SUMMARY_LAUNCH(8);
    else if (KP == 16) GS_SUMMARY_LAUNCH(16);
    else if (KP == 32) GS_SUMMARY_LAUNCH(32);
    else GS_SUMMARY_LAUNCH(64);
#undef GS_SUMMARY_LAUNCH
    GS_LAUNCH_CHECK("k_summary_update");
    return 0;
}

int gs_summary_finish(const void* state, int C, int nspec, int maxbins, int max_lag, double* pooled,
                      double* chain_mean, double* chain_var, double* acf, double* gamma, void* stream) {
    if (!state) return set_error("gs_summary_finish: null state");
    if (check_dims("gs_summary_finish", C, nspec, maxbins, 0, max_lag)) return -1;
    if (!pooled || !chain_mean || !chain_var || !acf || !gamma) return set_error("gs_summary_finish: null output");
    const long long nsb = (long long)nspec * maxbins;
    hipLaunchKernelGGL(k_summary_finish, dim3(nblk(nsb, BS)), dim3(BS), 0, (hipStream_t)stream,
                       (const double*)state, C, nsb, max_lag, pooled, chain_mean, chain_var, acf, gamma);
    GS_LAUNCH_CHECK("k_summary_finish");
    return 0;
}

}  // extern "C"
