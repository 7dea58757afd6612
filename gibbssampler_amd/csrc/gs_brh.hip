// gs_brh.hip -- Blackwell-Rao sample bank: the curvature of the likelihood in the
// tables, the likelihood-weighted covariance of the bank's scale columns, on the
// fp64 matrix cores (gfx950).
//
// With t_cik = r_ci - sum_j x_cij Y_kj and w_cik = exp(t_cik - M_k) (gs_brs.hip),
//   d^2 loglike_k / dY_ka dY_kb = Cov_w(x_a, x_b)
//     = sum_ci w_cik (x_cia - xbar_ka)(x_cib - xbar_kb) / sum_ci w_cik.
// k_brh_gram forms the centred numerators per chain,
//   num2[c][k][a][b] = sum_i exp(t_cik - mref_k) u_cia u_cib,  u_cia = fl(x_cia - center_ka)
// (center: the caller's xbar of the complete bank, gs_brs_grad_finish's output.
// Raw second moments minus xbar xbar^T cancel by the square of the scales' relative
// spread; the centred products do not, and fl(x - c) is relatively exact).
//
// One workgroup (4 waves) per (chain, block of HR = 1024 bank rows, tile of MT = 4
// models, pair (ta <= tb) of tiles of HC = 64 columns).  The block is walked in
// passes of PR = 64 rows.  A pass first recomputes t of its 64 rows exactly as
// k_brs_eval and k_brs_grad do: the same stages of JC = 32 columns over ALL Jp
// columns, X [64 rows][32] and Y [16 models][32] through LDS (row stride 34), one
// v_mfma_f64_16x16x4_f64 per 4 columns and wave, the columns ascending through one
// accumulator per (row, model) -- an accumulator's bits depend on its row's X and
// its model's Y alone, so the 12 model rows of the tile that hold zeros change
// nothing.  While a stage of tile ta or tb passes through LDS it is also kept in
// s_keep [64 rows][128] (row stride KS = 144 doubles; ta's columns at 0, tb's at
// 64; a row whose r is NaN is kept as zeros, and so are rows >= n).  After the last
// stage a lane holds t of rows 16 wave + (l >> 4) + 4 g and model l & 15 and writes
//   w = exp((r - dot) - mref_k)      (0 for a NaN r, a row >= n, a model >= K)
// into s_w [4 models][64 rows] (row stride 66, over the staging buffers).  The
// second contraction runs over the pass's rows, 4 per MFMA, rows ascending, per
// model m: A = 16 columns of ta x 4 rows, w u (lane l: column l & 15, row l >> 4), B
// = 4 rows x 16 columns of tb, u (lane l: row l >> 4, column l & 15), D column-of-ta
// (l >> 4) + 4 reg, column-of-tb l & 15.  Wave w owns columns 16 w .. 16 w + 15 of ta
// against all 64 of tb for the 4 models: 16 accumulators (64 doubles) per lane,
// carried across the passes of the block.  Both operands come from s_keep with one
// pattern, 2 rows x 16 columns per ds_read_b64 half (dword 288 row + 2 column, 288
// = 32 mod 64: conflict-free); the centre is subtracted and the weight applied in
// registers, each one rounded operation.  A pair ta == tb skips the 16 x 16 tiles
// below the diagonal.
// Each symmetric pair is computed once: the workgroup writes D[a][b] for a <= b to
// work [chain][block][K][Jp][Jp] at [a][b] and at [b][a].  k_brh_combine adds a
// chain's blocks in block order from 0.0 and writes 0 in the padding rows and
// columns.  No float atomics: for given (n, Ju, mref_k, center_k) the tile
// num2[c][k] depends on chain c's rows and model k's Y alone.
// k_brh_finish, the chains in chain order, every step one rounded operation, den_k
// as k_brs_grad_finish forms it:
//   M = max m_c over S_c > 0,  den = sum_c S_c exp(m_c - M)
//   cov[k][a][b] = (sum_c num2[c][k][a][b]) / den     (NaN where no chain holds a sample)
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
constexpr int PR = 64;        // rows per pass (16 per wave)
constexpr int JC = 32;        // columns per LDS stage (gs_brs.hip's)
constexpr int LDW = JC + 2;   // LDS row stride of a stage (doubles)
constexpr int SE = PR * JC / BS;   // elements of X a thread stages
constexpr int HR = 1024;      // bank rows per workgroup
constexpr int MT = 4;         // models per workgroup
constexpr int HC = 64;        // columns per tile
constexpr int NB = HC / 16;   // 16-column MFMA tiles of tb (a wave owns one of ta)
constexpr int KS = 2 * HC + 16;    // row stride of the kept X tiles (doubles)
constexpr int WS = PR + 2;    // row stride of the weights (doubles)
constexpr long long WORK_MAX = 1LL << 36;   // bytes of workspace one call may ask for
static_assert(SE * BS == PR * JC && HR % PR == 0 && PR == 16 * (BS / 64) && HC == 16 * (BS / 64), "tile shapes");
static_assert(HC % JC == 0 && KS % 32 == 16 && MT <= BS / JC && MT * WS <= 2 * PR * LDW, "LDS layout");

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }

__global__ __launch_bounds__(BS) void k_brh_gram(const double* __restrict__ X, const double* __restrict__ r, int cap,
                                                 int n, int Jp, int Ju, int K, const double* __restrict__ Y,
                                                 const double* __restrict__ mref, const double* __restrict__ center,
                                                 double* __restrict__ part, int nblk, int nkt, int nct) {
    __shared__ __attribute__((aligned(16))) double lds[2 * PR * LDW + PR * KS];
    double* s_x = lds;
    double* s_y = lds + PR * LDW;
    double* s_w = lds;                                         // after a pass's last stage
    double* s_keep = lds + 2 * PR * LDW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, kq = lane >> 4;
    const int npair = nct * (nct + 1) / 2;
    int bi = blockIdx.x;
    const int kt = bi % nkt; bi /= nkt;
    int pr = bi % npair; bi /= npair;
    const int blk = bi % nblk, chain = bi / nblk;
    int ta = 0;
    while (pr >= nct - ta) { pr -= nct - ta; ++ta; }           // pairs (ta, ta), (ta, ta + 1), ... in order
    const int tb = ta + pr;
    const bool diag = ta == tb;
    const int k0 = kt * MT, a0 = ta * HC, b0 = tb * HC;
    const int bo = diag ? 0 : HC;                              // tb's columns within s_keep
    const int row_s = blk * HR;
    const int nrows = n - row_s < HR ? n - row_s : HR;          // > 0: nblk = ceil(n / HR)
    const int nm = K - k0 < MT ? K - k0 : MT;                   // models of this workgroup
    const int ca0 = a0 + 16 * wave;                             // the wave's first column of ta
    const int hn = (Jp - b0 + 15) / 16 < NB ? (Jp - b0 + 15) / 16 : NB;   // 16-column tiles of tb that hold a column
    const int h0 = diag ? wave : 0;                            // the first of them this wave computes
    const bool gram = ca0 < Jp;
    const double* Xc = X + (long long)chain * cap * Jp;
    const double* rc = r + (long long)chain * cap;
    const int nchunk = (Jp + JC - 1) / JC;
    const int npass = (nrows + PR - 1) / PR;
    const int total = npass * nchunk;
    const int sc = tid & (JC - 1), sr = tid / JC;

    double vx[SE], vy = 0.0;
    unsigned vok = 0u;                                         // bit e: row e of the issued stage has a finite r
    auto issue = [&](int s) {
        const int pass = s / nchunk, ch = s - pass * nchunk;
        const int j = ch * JC + sc;
        if (ch == 0) {
            vok = 0u;
#pragma unroll
            for (int e = 0; e < SE; ++e) {
                const int lr = pass * PR + sr + (BS / JC) * e;
                const double rv = lr < nrows ? rc[row_s + lr] : qnan();
                if (rv == rv) vok |= 1u << e;
            }
        }
#pragma unroll
        for (int e = 0; e < SE; ++e) {
            const int lr = pass * PR + sr + (BS / JC) * e;     // row within the block
            vx[e] = (j < Jp && lr < nrows) ? Xc[(long long)(row_s + lr) * Jp + j] : 0.0;
        }
        // Y: model rows 0 .. 15 of the tile, rows >= nm zero (two rows of 32 columns per thread pass)
        vy = (j < Ju && sr < nm) ? Y[(long long)(k0 + sr) * Ju + j] : 0.0;
    };

    // the lane's centres: column ca0 + rl of ta, columns b0 + 16 h + rl of tb, per model
    double mr = 0.0, ca[MT], cb[MT][NB];
    if (rl < nm) mr = mref[k0 + rl];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int ja = ca0 + rl;
        ca[m] = (m < nm && ja < Ju) ? center[(long long)(k0 + m) * Ju + ja] : 0.0;
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            const int jb = b0 + 16 * h + rl;
            cb[m][h] = (m < nm && jb < Ju) ? center[(long long)(k0 + m) * Ju + jb] : 0.0;
        }
    }
    f64x4 acc;
    f64x4 nacc[MT][NB];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int h = 0; h < NB; ++h) nacc[m][h] = f64x4{0.0, 0.0, 0.0, 0.0};
    double rr[4];

    issue(0);
    for (int s = 0; s < total; ++s) {
        const int pass = s / nchunk, ch = s - pass * nchunk;
        const bool ina = ch * JC >= a0 && ch * JC < a0 + HC;    // a stage of tile ta
        const bool inb = !diag && ch * JC >= b0 && ch * JC < b0 + HC;
#pragma unroll
        for (int e = 0; e < SE; ++e) {
            const int row = sr + (BS / JC) * e;
            s_x[row * LDW + sc] = vx[e];
            const double kx = ((vok >> e) & 1u) ? vx[e] : 0.0;
            if (ina) s_keep[row * KS + ch * JC - a0 + sc] = kx;
            if (inb) s_keep[row * KS + HC + ch * JC - b0 + sc] = kx;
        }
        s_y[sr * LDW + sc] = vy;                               // model rows 0 .. 7
        s_y[(sr + BS / JC) * LDW + sc] = 0.0;                  // model rows 8 .. 15 (MT <= 8)
        __syncthreads();
        if (s + 1 < total) issue(s + 1);
        const int wrow = pass * PR + 16 * wave;                 // the wave's first row within the block
        const bool live = wrow < nrows;
        if (ch == 0) {
            acc = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int lr = wrow + kq + 4 * g;
                rr[g] = lr < nrows ? rc[row_s + lr] : qnan();
            }
        }
        if (live) {
            const int left = Jp - ch * JC;
            const int nks = (left < JC ? left : JC) / 4;
            const double* ap = s_x + (16 * wave + rl) * LDW + kq;
            const double* bp = s_y + rl * LDW + kq;
            for (int ks = 0; ks < nks; ++ks)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * ks], bp[4 * ks], acc, 0, 0, 0);
        }
        __syncthreads();                                       // the stage has been read
        if (ch == nchunk - 1) {
            if (rl < MT) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double ri = rr[g];
                    double w = 0.0;
                    if (live && ri == ri && rl < nm) w = exp((ri - acc[g]) - mr);
                    s_w[rl * WS + 16 * wave + kq + 4 * g] = w;
                }
            }
            __syncthreads();
            const int prow = nrows - pass * PR;                 // rows of this pass (the rest hold w = 0, x = 0)
            const int nks = ((prow < PR ? prow : PR) + 3) / 4;
            if (gram) {
                const double* wp = s_w + kq;
                const double* xp = s_keep + kq * KS + rl;
                for (int ks = 0; ks < nks; ++ks) {
                    const double xa = xp[4 * ks * KS + 16 * wave];
                    double xb[NB], wv[MT];
#pragma unroll
                    for (int h = 0; h < NB; ++h) xb[h] = xp[4 * ks * KS + bo + 16 * h];
#pragma unroll
                    for (int m = 0; m < MT; ++m) wv[m] = wp[m * WS + 4 * ks];
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if (m < nm) {
                            const double a = mul(wv[m], sub(xa, ca[m]));
#pragma unroll
                            for (int h = 0; h < NB; ++h)
                                if (h >= h0 && h < hn)
                                    nacc[m][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sub(xb[h], cb[m][h]), nacc[m][h],
                                                                                     0, 0, 0);
                        }
                    }
                }
            }
            __syncthreads();                                   // the weights and the kept tiles have been read
        }
    }
    if (!gram) return;
    double* po = part + ((long long)chain * nblk + blk) * K * Jp * Jp;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int h = 0; h < NB; ++h)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int a = ca0 + kq + 4 * g, b = b0 + 16 * h + rl;
                if (m < nm && h >= h0 && h < hn && a < Jp && b < Jp && a <= b) {
                    double* pk = po + (long long)(k0 + m) * Jp * Jp;
                    const double v = nacc[m][h][g];
                    pk[(long long)a * Jp + b] = v;
                    pk[(long long)b * Jp + a] = v;
                }
            }
}

// one thread per (chain, model, a, b): the blocks of a chain in block order
__global__ __launch_bounds__(BS) void k_brh_combine(const double* __restrict__ part, int K, int Jp, int Ju, int nblk,
                                                    long long total, double* __restrict__ num2) {
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    if (e >= total) return;
    const long long kjj = (long long)K * Jp * Jp;
    const long long chain = e / kjj, o = e - chain * kjj;
    const int b = (int)(o % Jp), a = (int)((o / Jp) % Jp);
    double v = 0.0;
    if (a < Ju && b < Ju)
        for (int q = 0; q < nblk; ++q) v = add(v, part[(chain * nblk + q) * kjj + o]);
    num2[e] = v;
}

// grid (tiles of BS entries, models): the chains in chain order
__global__ __launch_bounds__(BS) void k_brh_finish(const double* __restrict__ num2, const double* __restrict__ state,
                                                   int C, int K, int Jp, int Ju, double* __restrict__ cov) {
    const int k = blockIdx.y;
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    if (e >= (long long)Ju * Ju) return;
    const int a = (int)(e / Ju), b = (int)(e % Ju);
    const long long nck = (long long)C * K;
    const double* fm = state + HDR;
    const double* fS = fm + nck;
    bool any = false;
    double M = 0.0;
    for (int c = 0; c < C; ++c) {
        if (fS[(long long)c * K + k] > 0.0) {
            const double v = fm[(long long)c * K + k];
            M = any ? fmax(M, v) : v;
            any = true;
        }
    }
    double den = 0.0;
    for (int c = 0; c < C; ++c) {
        const double S = fS[(long long)c * K + k];
        if (S > 0.0) den = add(den, mul(S, exp(sub(fm[(long long)c * K + k], M))));
    }
    double v = 0.0;
    for (int c = 0; c < C; ++c) v = add(v, num2[(((long long)c * K + k) * Jp + a) * Jp + b]);
    cov[(long long)k * Ju * Ju + e] = any ? v / den : qnan();
}

int nblocks(int n) { return (n + HR - 1) / HR; }

}  // namespace

extern "C" {

int gs_brs_hess_info(int* block_rows, int* model_tile, int* column_tile) {
    if (!block_rows || !model_tile || !column_tile) return set_error("gs_brs_hess_info: null argument");
    *block_rows = HR;
    *model_tile = MT;
    *column_tile = HC;
    return 0;
}

int gs_brs_hess_work_bytes(int nchains, int n, int K, int Ju, long long* bytes) {
    if (!bytes) return set_error("gs_brs_hess_work_bytes: null argument");
    if (nchains < 1 || n < 0) return set_error("gs_brs_hess_work_bytes: nchains >= 1 and n >= 0 needed");
    if (K < 1 || Ju < 1) return set_error("gs_brs_hess_work_bytes: models K >= 1 and used columns Ju >= 1 needed");
    const long long Jp = (Ju + 3LL) / 4 * 4;
    // every factor is below 2^31 and is checked before the next product
    const long long tiles = (long long)nchains * (n > 0 ? nblocks(n) : 1);
    if (Jp * Jp > WORK_MAX / 8 || tiles > WORK_MAX / (8 * Jp * Jp) || tiles * K > WORK_MAX / (8 * Jp * Jp))
        return set_error("gs_brs_hess_work_bytes: 8 nchains ceil(n / block_rows) K Jp^2 bytes exceed the 64 GiB one "
                         "call may ask for (the pass is sized for a few models: split K)");
    *bytes = 8LL * tiles * K * Jp * Jp;
    return 0;
}

int gs_brs_hess(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                const double* mref, const double* center, void* work, long long work_bytes, double* num2,
                void* stream) {
    if (!X || !r) return set_error("gs_brs_hess: null bank");
    if (!num2) return set_error("gs_brs_hess: null num2");
    if (nchains < 1) return set_error("gs_brs_hess: nchains >= 1 needed");
    if (cap < 1) return set_error("gs_brs_hess: bank capacity cap >= 1 needed");
    if (Ju < 1) return set_error("gs_brs_hess: used columns Ju >= 1 needed");
    if ((long long)nchains * cap > 0x7fffffffLL) return set_error("gs_brs_hess: too many bank rows (nchains * cap)");
    if (K < 1) return set_error("gs_brs_hess: models K >= 1 needed");
    if (n < 0 || n > cap) return set_error("gs_brs_hess: rows n must lie in [0, cap]");
    long long need = 0;
    if (gs_brs_hess_work_bytes(nchains, n, K, Ju, &need)) return -1;
    const int Jp = (Ju + 3) / 4 * 4;
    const long long total = (long long)nchains * K * Jp * Jp;  // <= need / 8
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        GS_CHECK(hipMemsetAsync(num2, 0, (size_t)(8LL * total), st));
        return 0;
    }
    if (!Y || !mref || !center || !work) return set_error("gs_brs_hess: null Y, mref, center or workspace");
    if (work_bytes < need) return set_error("gs_brs_hess: the workspace is smaller than gs_brs_hess_work_bytes");
    const int nblk = nblocks(n), nkt = (K + MT - 1) / MT, nct = (Jp + HC - 1) / HC;
    const long long nb = (long long)nchains * nblk * nkt * (nct * (nct + 1LL) / 2);
    if (nb > 0x7fffffffLL) return set_error("gs_brs_hess: too many (chain, block, model tile, tile pair) workgroups");
    hipLaunchKernelGGL(k_brh_gram, dim3((unsigned)nb), dim3(BS), 0, st, X, r, cap, n, Jp, Ju, K, Y, mref, center,
                       (double*)work, nblk, nkt, nct);
    GS_LAUNCH_CHECK("k_brh_gram");
    hipLaunchKernelGGL(k_brh_combine, dim3((unsigned)((total + BS - 1) / BS)), dim3(BS), 0, st, (const double*)work,
                       K, Jp, Ju, nblk, total, num2);
    GS_LAUNCH_CHECK("k_brh_combine");
    return 0;
}

int gs_brs_hess_finish(const double* num2, const void* state, int C, int K, int Ju, double* cov, void* stream) {
    if (!num2 || !state || !cov) return set_error("gs_brs_hess_finish: null argument");
    if (C < 1 || K < 1 || Ju < 1) return set_error("gs_brs_hess_finish: C, K and Ju >= 1 needed");
    if ((long long)C * K > (1LL << 28)) return set_error("gs_brs_hess_finish: too many (chain, model) pairs");
    if (K > 65535) return set_error("gs_brs_hess_finish: more than 65535 models in one call");
    const int Jp = (Ju + 3) / 4 * 4;
    const long long tiles = ((long long)Ju * Ju + BS - 1) / BS;
    if (tiles > 0x7fffffffLL) return set_error("gs_brs_hess_finish: cov [K][Ju][Ju] too large");
    hipLaunchKernelGGL(k_brh_finish, dim3((unsigned)tiles, (unsigned)K), dim3(BS), 0, (hipStream_t)stream, num2,
                       (const double*)state, C, K, Jp, Ju, cov);
    GS_LAUNCH_CHECK("k_brh_finish");
    return 0;
}

}  // extern "C"
