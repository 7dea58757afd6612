// gs_smap.hip -- streaming posterior mean and variance of the sky map (gfx950).
//
// A plan-independent moment accumulator over a batch of fp64 series: C chains
// of length n, n = F (L+1)^2 for a real-layout a_lm or ncomp N_pix for a map.
//
// State (caller-owned device buffer of gs_smap_bytes bytes, fp64 unless noted):
//   header   8 doubles: [0] int64 k, the samples accumulated per chain; the
//            rest reserved (0)
//   mean     [C][n]   Welford mean of every element
//   M2       [C][n]   Welford sum of squared deviations
// gs_smap_reset zeroes all of it.
//
// k_smap_update, one thread per element, k = count_after given by the host:
//   d = x - mean;  mean = mean + d / k;  M2 = fma(d, x - mean, M2)
// No atomics and no reduction: an element's result is the same whatever the
// launch geometry and whichever of the paths below touches it, and chain b of a
// C-chain state equals a one-chain state fed chain b's data bit for bit.
//
// The update is a pure stream (3 loads + 2 stores of 8 B per element) over a
// state larger than the last-level cache, so it moves 16 bytes per lane
// wherever alignment allows (8-byte accesses stream at 0.54-0.70x the 16-byte
// rate on this chip).  The header keeps mean[0] 16-byte aligned when the state
// is; row c of mean starts at element 8 + c n, which is odd for odd c n (e.g.
// F = 3 with an even L), so a row is cut into
//   head   its first element when the mean row starts 8 bytes off a 16-byte
//          boundary (one thread, 8-byte accesses)
//   pairs  (i, i + 1) from there on: the mean pair is 16-byte aligned by
//          construction; the M2 pair and the x pair are moved as 16 bytes when
//          their own address is aligned and as two 8-byte accesses otherwise
//          (M2: odd C n; x: the caller's pointer and chain stride) -- a
//          row-uniform, hence wave-uniform, branch
//   tail   the last element when an odd one is left
// The state traffic is NOT marked non-temporal: on gfx950 a non-temporal load
// only bypasses the per-CU L1 (which a once-touched stream does not use either
// way) and a non-temporal store still leaves its line in L2, so the hint would
// not keep the state out of the caches that x lives in, and at 16 B per lane it
// measures 0-3 % slower than the plain access.  x is read plainly
// too: the next CR step reads it again.
//
// k_smap_finish, one thread per element over the C chains of k samples each
// (k read from the header), chains merged in chain order by Chan's update:
//   nA = k, mA = mean_0, MA = M2_0;  for c = 1 .. C-1:
//     d = mean_c - mA;  nAB = nA + k;  mA += d (k / nAB);
//     MA += M2_c + d^2 (nA k / nAB);  nA = nAB
//   mean = mA;  var = MA / (N - 1), N = C k   (NaN when N < 2; k < 1: both NaN)
//   chain_mean[c] = mean_c
//   rhat as k_summary_finish (gs_summary.hip): with m = mean_c mean_c,
//     W = mean_c M2_c / (k - 1),  B/k = sum_c (mean_c - m)^2 / (C - 1),
//     var+ = mean_c M2_c / k + B/k,  rhat = sqrt(var+ / W)
//   (NaN for C = 1, k < 2 or W == 0).
//
// k_smap_power, real m-major a_lm states (slots 0..L
// are a_l0, then (sqrt2 Re, sqrt2 Im) pairs at 2 i - (L+1), i = m (2L+1-m)/2 + l,
// so the squares of the slots of one l add up to (2l+1) C_l with no further
// factor).  One lane per (field, l), m = 0, 1, .. l in order, Re before Im:
//   power_of_mean = sum_m mean^2 / (2l+1)
//   mean_power    = power_of_mean + sum_m var / (2l+1)
// the spectrum of the posterior mean map and the posterior mean of the map's
// spectrum (auto spectra only: TE would need a cross accumulator).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <string>

#include "gibbs_capi.h"
#include "gs_common.h"
#include "gs_launch.h"

using gs_detail::set_error;
using gs_detail::nblk;

namespace {

constexpr int HDR = 8;       // header doubles
constexpr int BS = 256;
constexpr int WAVE = 64;
typedef double double2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void welford(double x, double kd, double& mean, double& M2) {
    const double d = x - mean;
    mean = mean + d / kd;
    M2 = fma(d, x - mean, M2);
}

__device__ __forceinline__ void welford_at(double* __restrict__ mean, double* __restrict__ M2,
                                           const double* __restrict__ x, long long i, double kd) {
    double m = mean[i], q = M2[i];
    welford(x[i], kd, m, q);
    mean[i] = m;
    M2[i] = q;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grid: x = workgroups over a row's pairs (grid-stride), y = chains (grid-stride)
__global__ __launch_bounds__(BS) void k_smap_update(double* __restrict__ state, int C, long long n,
                                                    const double* __restrict__ x, long long xs, long long count) {
    const double kd = (double)count;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        double* mean = state + HDR + (long long)c * n;
        double* M2 = state + HDR + ((long long)C + c) * n;
        const double* xr = x + (long long)c * xs;
        const long long h = aligned16(mean) ? 0 : 1;
        const long long npair = (n - h) / 2;
        const bool ax = aligned16(xr + h), aq = aligned16(M2 + h);
        for (long long p = (long long)blockIdx.x * BS + threadIdx.x; p < npair; p += (long long)gridDim.x * BS) {
            const long long i = h + 2 * p;              // i + 1 <= h + 2 npair - 1 <= n - 1
            double2v m = *(const double2v*)(mean + i);
            double2v q, v;
            if (aq) q = *(const double2v*)(M2 + i);
            else { q.x = M2[i]; q.y = M2[i + 1]; }
            if (ax) v = *(const double2v*)(xr + i);
            else { v.x = xr[i]; v.y = xr[i + 1]; }
            double m0 = m.x, m1 = m.y, q0 = q.x, q1 = q.y;
            welford(v.x, kd, m0, q0);
            welford(v.y, kd, m1, q1);
            m.x = m0; m.y = m1; q.x = q0; q.y = q1;
            *(double2v*)(mean + i) = m;
            if (aq) *(double2v*)(M2 + i) = q;
            else { M2[i] = q.x; M2[i + 1] = q.y; }
        }
        if (blockIdx.x == 0) {
            if (threadIdx.x == 0 && h == 1) welford_at(mean, M2, xr, 0, kd);
            if (threadIdx.x == 1 && h + 2 * npair < n) welford_at(mean, M2, xr, n - 1, kd);
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *(long long*)state = count;
}

__global__ __launch_bounds__(BS) void k_smap_finish(const double* __restrict__ state, int C, long long n,
                                                    double* __restrict__ mean_out, double* __restrict__ var_out,
                                                    double* __restrict__ chain_mean, double* __restrict__ rhat_out) {
    const long long k = *(const long long*)state;
    const double* mean = state + HDR;
    const double* M2 = state + HDR + (long long)C * n;
    const double kd = (double)k, Cd = (double)C, qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long i = (long long)blockIdx.x * BS + threadIdx.x; i < n; i += (long long)gridDim.x * BS) {
        double nA = kd, mA = mean[i], MA = M2[i];
        double sum_mean = mA, sum_M2 = MA;
        chain_mean[i] = mA;
        for (int c = 1; c < C; ++c) {
            const double mc = mean[(long long)c * n + i], qc = M2[(long long)c * n + i];
            chain_mean[(long long)c * n + i] = mc;
            const double d = mc - mA, nAB = nA + kd;
            mA = mA + d * (kd / nAB);
            MA = MA + qc + (d * d) * (nA * kd / nAB);
            nA = nAB;
            sum_mean = sum_mean + mc;
            sum_M2 = sum_M2 + qc;
        }
        const long long N = (long long)C * k;
        mean_out[i] = k >= 1 ? mA : qnan;
        var_out[i] = (k >= 1 && N >= 2) ? MA / (double)(N - 1) : qnan;
        double rhat = qnan;
        if (C > 1 && k >= 2) {
            const double m = sum_mean / Cd;
            double sb2 = 0.0;
            for (int c = 0; c < C; ++c) {
                const double d = mean[(long long)c * n + i] - m;
                sb2 = sb2 + d * d;
            }
            const double W = sum_M2 / (kd - 1.0) / Cd, g0 = sum_M2 / kd / Cd;
            const double varp = g0 + sb2 / (Cd - 1.0);
            if (W > 0.0) rhat = sqrt(varp / W);
        }
        rhat_out[i] = rhat;
    }
}

// one wave per (field, 64-l tile), lanes = l, loop over m (the slot -> l map of k_alm2cl)
__global__ __launch_bounds__(BS) void k_smap_power(int L, int F, const double* __restrict__ mean,
                                                   const double* __restrict__ var, double* __restrict__ pom,
                                                   double* __restrict__ mp) {
    const int ntile = (L + WAVE) / WAVE;
    const int w = blockIdx.x * (BS / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (w >= F * ntile) return;
    const int f = w / ntile, ell = (w % ntile) * WAVE + lane;
    if (ell > L) return;
    const long long nr = (long long)(L + 1) * (L + 1);
    const double* a = mean + f * nr;
    const double* v = var + f * nr;
    double s = a[ell] * a[ell], t = v[ell];
    for (int m = 1; m <= ell; ++m) {
        const long long r = 2 * ((long long)m * (2 * L + 1 - m) / 2 + ell) - (L + 1);
        s = s + a[r] * a[r];
        s = s + a[r + 1] * a[r + 1];
        t = t + v[r];
        t = t + v[r + 1];
    }
    const double w2 = 2.0 * ell + 1.0, p = s / w2;
    pom[(long long)f * (L + 1) + ell] = p;
    mp[(long long)f * (L + 1) + ell] = p + t / w2;
}

int check_dims(const char* what, long long C, long long n) {
    if (C < 1) return set_error(std::string(what) + ": C out of range (need C >= 1)");
    if (n < 1) return set_error(std::string(what) + ": n out of range (need n >= 1)");
    if (C > (1LL << 24) || n > (1LL << 40) || C * n > (1LL << 40))
        return set_error(std::string(what) + ": C * n too large");
    return 0;
}

long long state_bytes(long long C, long long n) { return 8LL * (HDR + 2 * C * n); }

}  // namespace

extern "C" {

int gs_smap_bytes(int C, long long n, long long* bytes) {
    if (!bytes) return set_error("gs_smap_bytes: null bytes");
    if (check_dims("gs_smap_bytes", C, n)) return -1;
    *bytes = state_bytes(C, n);
    return 0;
}

int gs_smap_reset(void* state, int C, long long n, void* stream) {
    if (!state) return set_error("gs_smap_reset: null state");
    if (check_dims("gs_smap_reset", C, n)) return -1;
    GS_CHECK(hipMemsetAsync(state, 0, (size_t)state_bytes(C, n), (hipStream_t)stream));
    return 0;
}

int gs_smap_update(void* state, int C, long long n, const double* x, long long x_chain_stride, long long count_after,
                   void* stream) {
    if (!state) return set_error("gs_smap_update: null state");
    if (!x) return set_error("gs_smap_update: null x");
    if (check_dims("gs_smap_update", C, n)) return -1;
    if (x_chain_stride < 0) return set_error("gs_smap_update: x_chain_stride out of range (need >= 0)");
    if (count_after < 1) return set_error("gs_smap_update: count_after out of range (need count_after >= 1)");
    if (((uintptr_t)state & 7) || ((uintptr_t)x & 7)) return set_error("gs_smap_update: state and x must be 8-byte aligned");
    // a few workgroups per CU whatever C: rows of many pairs are walked grid-stride
    const long long want = std::max<long long>(1, (n / 2 + BS - 1) / BS);
    const unsigned gx = (unsigned)std::min<long long>(want, std::max<long long>(1, 8192 / C));
    const unsigned gy = (unsigned)std::min<long long>(C, 65535);
    hipLaunchKernelGGL(k_smap_update, dim3(gx, gy), dim3(BS), 0, (hipStream_t)stream, (double*)state, C, n, x,
                       x_chain_stride, count_after);
    GS_LAUNCH_CHECK("k_smap_update");
    return 0;
}

int gs_smap_finish(const void* state, int C, long long n, double* mean, double* var, double* chain_mean, double* rhat,
                   void* stream) {
    if (!state) return set_error("gs_smap_finish: null state");
    if (!mean) return set_error("gs_smap_finish: null mean");
    if (!var) return set_error("gs_smap_finish: null var");
    if (!chain_mean) return set_error("gs_smap_finish: null chain_mean");
    if (!rhat) return set_error("gs_smap_finish: null rhat");
    if (check_dims("gs_smap_finish", C, n)) return -1;
    hipLaunchKernelGGL(k_smap_finish, dim3(std::min(nblk(n, BS), 16384u)), dim3(BS), 0, (hipStream_t)stream,
                       (const double*)state, C, n, mean, var, chain_mean, rhat);
    GS_LAUNCH_CHECK("k_smap_finish");
    return 0;
}

int gs_smap_power(int L, int F, const double* mean, const double* var, double* power_of_mean, double* mean_power,
                  void* stream) {
    if (L < 0 || L > 16384) return set_error("gs_smap_power: L out of range [0, 16384]");
    if (F < 1 || F > 3) return set_error("gs_smap_power: F out of range [1, 3]");
    if (!mean) return set_error("gs_smap_power: null mean");
    if (!var) return set_error("gs_smap_power: null var");
    if (!power_of_mean) return set_error("gs_smap_power: null power_of_mean");
    if (!mean_power) return set_error("gs_smap_power: null mean_power");
    const int ntile = (L + WAVE) / WAVE;
    hipLaunchKernelGGL(k_smap_power, dim3(nblk((long long)F * ntile, BS / WAVE)), dim3(BS), 0, (hipStream_t)stream, L,
                       F, mean, var, power_of_mean, mean_power);
    GS_LAUNCH_CHECK("k_smap_power");
    return 0;
}

}  // extern "C"
