// gs_brs.hip -- Blackwell-Rao sample bank: the kept samples of a run, compressed
// to the used columns, and an fp64 matrix-core evaluator that scores any theory
// spectra against them afterwards (gfx950).
//
// gs_brl.hip needs its K theory spectra before the run.  The bank keeps what
// that estimator reads of every sample instead -- the Ju used columns of the
// scale ring row and the model-independent term r -- so that
//   t_{c,i,k} = r_{c,i} - sum_j X_{c,i,j} Y_{k,j}
// can be formed for theory tables Y [K][Ju] (engine.br_likelihood_tables) named
// after the run.  cols, kind and coef are the tables of gs_brl.hip; they depend
// on the bins and the mask, not on the theory.
//
// Bank (caller-owned device buffers, fp64), Jp = Ju rounded up to a multiple of 4:
//   X [nchains][cap][Jp]   X[c][i][j] = the ring's value at column cols[j] of
//                          chain c's i-th kept sample; columns j >= Ju are 0
//   r [nchains][cap]       sum_j coef_j log(arg_j) as k_brl_update forms it (same
//                          arg of kinds 1 and 2, one fma chain over j ascending
//                          from 0.0); NaN for a bad row (a kind 1 x or a kind 2
//                          arg <= 0 or not finite)
// Chain-major: the rows of a workgroup belong to one chain.
//
// k_brs_pack, one workgroup per (ring row, chain) of a launch: the threads copy
// the used columns into X and stage log(arg) of 256 columns at a time in LDS,
// thread 0 runs the fma chain.  A bank row's bits depend only on its ring row.
//
// k_brs_eval, one workgroup (4 waves) per (chain, slice of SL = 256 bank rows,
// tile of TMOD = 64 models).  The slice is walked in passes of PR = 64 rows,
// wave w owning rows 16 w .. 16 w + 15 of a pass, and a pass in stages of JC = 32
// columns: X [64 rows][32] and Y [64 models][32] go through LDS (row stride 34
// doubles: the 32 lanes of a ds_read_b64 half, 16 rows x 2 columns, fall on 32
// different 8-B banks), the next stage's global loads are issued before this
// stage's MFMAs.  Per 4 columns a wave issues one v_mfma_f64_16x16x4_f64 per
// 16-model tile: A = 16 rows x 4 columns (lane l: row l & 15, column l >> 4), B
// = 4 columns x 16 models (lane l: column l >> 4, model l & 15), D row (l >> 4) +
// 4 reg, column l & 15.  The columns run j = 0 .. Jp - 1 ascending through one
// accumulator per (row, model).  After the last stage of a pass a lane holds
//   t = r - dot
// of rows 16 w + (l >> 4) + 4 g, g = 0 .. 3, for each of its models, and folds
// them in that (row) order into the lane's running (m, S, Q) of the model with
// the rule of gs_brl.hip:
//   S == 0:  m = t, S = 1, Q = 1
//   else     d = t - m,  w = exp(-|d|)
//            d > 0:  S = fma(S, w, 1), Q = fma(Q, w * w, 1), m = t
//            else    S = S + w,        Q = fma(w, w, Q)
// Rows with a NaN r, rows >= n and models >= K are never folded.  At the end of
// the slice the 16 lane states of a model merge in a fixed order -- lane groups
// l >> 4 = 0 .. 3 of a wave, then waves 0 .. 3 -- into one partial triple per
// (chain, slice, model).  The merge of (m1, S1, Q1) and (m2, S2, Q2), every step
// one rounded operation, an empty side (S == 0) the identity:
//   M = max(m1, m2), e1 = exp(m1 - M), e2 = exp(m2 - M)
//   S = S1 e1 + S2 e2,  Q = Q1 (e1 e1) + Q2 (e2 e2)
// k_brs_combine merges a chain's slices in slice order, counts the chain's rows
// with a NaN r, and writes a state in the layout of gs_brl.hip (header with n;
// m, S, Q [nchains][K]; bad [nchains]) for gs_brl_finish.  No float atomics:
// for a given (n, Ju) the triple of (chain c, model k) depends on chain c's rows
// and model k's Y alone, not on K, the tile's other models or the other chains.
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
constexpr int SL = 256;       // bank rows per slice
constexpr int PR = 64;        // rows per pass (16 per wave)
constexpr int TMOD = 64;      // models per workgroup
constexpr int NQ = TMOD / 16; // 16-model MFMA tiles per workgroup
constexpr int JC = 32;        // columns per LDS stage
constexpr int LDW = JC + 2;   // LDS row stride (doubles)
constexpr int SE = PR * JC / BS;   // elements of X (and of Y) a thread stages
static_assert(PR == TMOD && SE * BS == PR * JC && SL % PR == 0 && PR == 16 * (BS / 64), "tile shapes");
static_assert(2 * PR * LDW >= 16 * TMOD * 3 + 4 * TMOD * 3, "the lane states reuse the staging LDS");

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }

__global__ __launch_bounds__(BS) void k_brs_pack(double* __restrict__ X, double* __restrict__ r, int nchains, int cap,
                                                 int Jp, int Ju, int nsb, int maxbins, const int* __restrict__ cols,
                                                 const int* __restrict__ kind, const double* __restrict__ coef,
                                                 const double* __restrict__ scales, int capacity, int slot0, int row0) {
    __shared__ double s_lg[BS];
    __shared__ double s_cf[BS];
    __shared__ int s_kd[BS];
    const int t = threadIdx.x;
    const int i = blockIdx.x / nchains, chain = blockIdx.x % nchains;
    int slot = slot0 + i;
    if (slot >= capacity) slot -= capacity;                    // slot0 < capacity and nsteps <= capacity: one wrap
    const double* rowp = scales + ((long long)slot * nchains + chain) * nsb;
    const long long brow = (long long)chain * cap + row0 + i;
    double* xo = X + brow * Jp;
    double racc = 0.0;
    bool bad = false;
    for (int j0 = 0; j0 < Jp; j0 += BS) {
        const int j = j0 + t;
        double x = 0.0, lg = 0.0, cf = 0.0;
        int kd = 0;
        if (j < Ju) {
            const int col = cols[j];
            kd = kind[j];
            cf = coef[j];
            if (col >= 0 && col < nsb) x = rowp[col];
            if (kd == 1) {
                lg = pos_finite(x) ? log(x) : qnan();
            } else if (kd == 2) {
                const bool in = col >= 0 && col + 3 * maxbins < nsb;
                const double dd = in ? rowp[col + maxbins] : qnan();
                const double c = in ? rowp[col + 3 * maxbins] : qnan();
                const double det = fma(x, dd, -(c * c));
                lg = pos_finite(det) ? log(det) : qnan();
            }
        }
        if (j < Jp) xo[j] = x;
        s_lg[t] = lg;
        s_cf[t] = cf;
        s_kd[t] = kd;
        __syncthreads();
        if (t == 0) {
            const int jn = Ju - j0 < BS ? Ju - j0 : BS;
            for (int jj = 0; jj < jn; ++jj) {
                if (s_kd[jj] != 0) {
                    const double l = s_lg[jj];
                    if (l == l) racc = fma(s_cf[jj], l, racc);
                    else bad = true;
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) r[brow] = bad ? qnan() : racc;
}

// (m, S, Q) <- (m, S, Q) merged with (m2, S2, Q2)
__device__ __forceinline__ void merge(double& m, double& S, double& Q, double m2, double S2, double Q2) {
    if (S2 == 0.0) return;
    if (S == 0.0) {
        m = m2; S = S2; Q = Q2;
        return;
    }
    const double M = fmax(m, m2);
    const double e1 = exp(sub(m, M)), e2 = exp(sub(m2, M));
    S = add(mul(S, e1), mul(S2, e2));
    Q = add(mul(Q, mul(e1, e1)), mul(Q2, mul(e2, e2)));
    m = M;
}

__global__ __launch_bounds__(BS) void k_brs_eval(const double* __restrict__ X, const double* __restrict__ r, int cap,
                                                 int n, int Jp, int Ju, int K, const double* __restrict__ Y,
                                                 double* __restrict__ part, int nslice, int nkt) {
    __shared__ __attribute__((aligned(16))) double lds[2 * PR * LDW];
    double* s_x = lds;
    double* s_y = lds + PR * LDW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, kq = lane >> 4;
    const int kt = blockIdx.x % nkt, slice = (blockIdx.x / nkt) % nslice, chain = blockIdx.x / (nkt * nslice);
    const int k0 = kt * TMOD;
    const int row_s = slice * SL;
    const int nrows = n - row_s < SL ? n - row_s : SL;          // > 0: nslice = ceil(n / SL)
    const int nq = K - k0 >= TMOD ? NQ : (K - k0 + 15) / 16;    // 16-model tiles that hold a model
    const double* Xc = X + (long long)chain * cap * Jp;
    const double* rc = r + (long long)chain * cap;
    const int nchunk = (Jp + JC - 1) / JC;
    const int npass = (nrows + PR - 1) / PR;
    const int total = npass * nchunk;
    const int sc = tid & (JC - 1), sr = tid / JC;

    double vx[SE], vy[SE];
    // global loads of stage s into registers (nothing waits on them here)
    auto issue = [&](int s) {
        const int pass = s / nchunk, ch = s - pass * nchunk;
        const int j = ch * JC + sc;
#pragma unroll
        for (int e = 0; e < SE; ++e) {
            const int lr = pass * PR + sr + (BS / JC) * e;     // row within the slice
            vx[e] = (j < Jp && lr < nrows) ? Xc[(long long)(row_s + lr) * Jp + j] : 0.0;
            const int km = k0 + sr + (BS / JC) * e;
            vy[e] = (j < Ju && km < K) ? Y[(long long)km * Ju + j] : 0.0;
        }
    };

    double m[NQ], S[NQ], Q[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { m[q] = 0.0; S[q] = 0.0; Q[q] = 0.0; }
    f64x4 acc[NQ];
    double rr[4];

    issue(0);
    for (int s = 0; s < total; ++s) {
        const int pass = s / nchunk, ch = s - pass * nchunk;
#pragma unroll
        for (int e = 0; e < SE; ++e) {
            s_x[(sr + (BS / JC) * e) * LDW + sc] = vx[e];
            s_y[(sr + (BS / JC) * e) * LDW + sc] = vy[e];
        }
        __syncthreads();
        if (s + 1 < total) issue(s + 1);
        const int wrow = pass * PR + 16 * wave;                 // the wave's first row within the slice
        const bool live = wrow < nrows;
        if (ch == 0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
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
            for (int ks = 0; ks < nks; ++ks) {
                const double a = ap[4 * ks];
                double b[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) b[q] = bp[16 * q * LDW + 4 * ks];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc[q], 0, 0, 0);
            }
        }
        __syncthreads();                                       // the stage has been read
        if (ch == nchunk - 1 && live) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double ri = rr[g];
                if (ri == ri) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        if (q < nq && k0 + 16 * q + rl < K) {
                            const double tv = ri - acc[q][g];
                            if (S[q] == 0.0) {
                                m[q] = tv;
                                S[q] = 1.0;
                                Q[q] = 1.0;
                            } else {
                                const double d = tv - m[q];
                                const double w = exp(-fabs(d));
                                if (d > 0.0) {
                                    const double ww = w * w;
                                    S[q] = fma(S[q], w, 1.0);
                                    Q[q] = fma(Q[q], ww, 1.0);
                                    m[q] = tv;
                                } else {
                                    S[q] = S[q] + w;
                                    Q[q] = fma(w, w, Q[q]);
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    // the lane states [wave][lane group][model][3] take the staging LDS (the last
    // stage's reads are behind the loop's closing barrier)
    double* s_st = lds;
    double* s_wv = lds + 16 * TMOD * 3;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double* o = s_st + ((wave * 4 + kq) * TMOD + 16 * q + rl) * 3;
        o[0] = m[q]; o[1] = S[q]; o[2] = Q[q];
    }
    __syncthreads();
    {
        // thread (wave w, model): lane groups 0 .. 3 of wave w, in order
        const int w = tid >> 6, mdl = tid & 63;
        double am = 0.0, aS = 0.0, aQ = 0.0;
        for (int g = 0; g < 4; ++g) {
            const double* o = s_st + ((w * 4 + g) * TMOD + mdl) * 3;
            merge(am, aS, aQ, o[0], o[1], o[2]);
        }
        double* o = s_wv + (w * TMOD + mdl) * 3;
        o[0] = am; o[1] = aS; o[2] = aQ;
    }
    __syncthreads();
    if (tid < TMOD && k0 + tid < K) {
        double am = 0.0, aS = 0.0, aQ = 0.0;
        for (int w = 0; w < BS / 64; ++w) {
            const double* o = s_wv + (w * TMOD + tid) * 3;
            merge(am, aS, aQ, o[0], o[1], o[2]);
        }
        double* po = part + ((long long)chain * nslice + slice) * 3 * K + k0 + tid;
        po[0] = am;
        po[K] = aS;
        po[2LL * K] = aQ;
    }
}

// grid (model blocks, chains): the slices of a chain in slice order; the first
// model block of a chain counts its NaN rows, the first workgroup writes the header
__global__ __launch_bounds__(BS) void k_brs_combine(const double* __restrict__ part, const double* __restrict__ r,
                                                    int cap, int n, int nchains, int K, int nslice,
                                                    double* __restrict__ state) {
    __shared__ unsigned long long s_bad;
    const int t = threadIdx.x, chain = blockIdx.y;
    const int k = blockIdx.x * BS + t;
    const long long nck = (long long)nchains * K;
    double* fm = state + HDR;
    double* fS = fm + nck;
    double* fQ = fS + nck;
    if (k < K) {
        double am = 0.0, aS = 0.0, aQ = 0.0;
        for (int s = 0; s < nslice; ++s) {
            const double* po = part + ((long long)chain * nslice + s) * 3 * K + k;
            merge(am, aS, aQ, po[0], po[K], po[2LL * K]);
        }
        const long long e = (long long)chain * K + k;
        fm[e] = am;
        fS[e] = aS;
        fQ[e] = aQ;
    }
    if (blockIdx.x == 0) {
        if (t == 0) s_bad = 0ULL;
        __syncthreads();
        unsigned long long cnt = 0ULL;
        const double* rc = r + (long long)chain * cap;
        for (int i = t; i < n; i += BS) {
            const double v = rc[i];
            if (!(v == v)) ++cnt;
        }
        if (cnt) atomicAdd(&s_bad, cnt);
        __syncthreads();
        if (t == 0) ((unsigned long long*)(fQ + nck))[chain] = s_bad;
        if (chain == 0 && t < HDR) {
            if (t == 0) *(long long*)state = (long long)n;
            else state[t] = 0.0;
        }
    }
}

// ---- likelihood gradient: a second pass over the bank ---------------------------
// d loglike_k / d Y_kj = -xbar_kj, xbar_kj = sum_ci w_cik x_cij / sum_ci w_cik with
// w_cik = exp(t_cik - M_k).  k_brs_grad forms the numerators per chain,
//   num[c][k][j] = sum_i exp(t_cik - mref_k) X[c][i][j],
// one workgroup (4 waves) per (chain, block of GR = 1024 bank rows, tile of TMOD
// = 64 models, tile of CT = 128 columns).  The block is walked in passes of PR =
// 64 rows.  A pass first recomputes t of its 64 rows x 64 models exactly as
// k_brs_eval does (the same stages of JC = 32 columns over ALL Jp columns, the
// same MFMA order: the same bits); while a stage of the workgroup's own column
// tile passes through LDS it is also kept in s_keep [64 rows][CT] (row stride KS =
// 144 doubles; a row whose r is NaN is kept as zeros, and so are rows >= n).
// After the last stage a lane holds t of rows 16 wave + (l >> 4) + 4 g and models
// 16 q + (l & 15) and writes
//   w = exp((r - dot) - mref_k)      (0 for a NaN r, a row >= n, a model >= K)
// transposed into s_w [64 models][64 rows] (row stride WS = 66, over the staging
// buffers).  The second contraction runs over the pass's rows, 4 per MFMA, rows
// ascending: A = 16 models x 4 rows from s_w (lane l: model l & 15, row l >> 4), B =
// 4 rows x 16 columns from s_keep (lane l: row l >> 4, column l & 15), D model (l >>
// 4) + 4 reg, column l & 15.  Wave w owns columns 32 w .. 32 w + 31 of the tile for
// all 64 models: 8 accumulators (32 doubles) per lane, carried across the passes
// of the block.  Both reads are conflict-free: the 32 lanes of a ds_read_b64 half
// fall on 16 models x 2 rows of s_w (dword 132 model + 2 row) and on 2 rows x 16
// columns of s_keep (dword 288 row + 2 column, 288 = 32 mod 64).
// The block's tile goes to work [chain][block][K][Jp]; k_brs_grad_combine adds a
// chain's blocks in block order from 0.0 and writes 0 in the padding columns.  No
// float atomics: for given (n, Ju, mref_k) the row num[c][k][.] depends on chain
// c's rows and model k's Y alone.
// k_brs_grad_finish, one workgroup per model, the chains in chain order, every
// step one rounded operation:
//   M = max m_c over S_c > 0,  e_c = S_c exp(m_c - M),  den = sum_c e_c
//   xbar[k][j] = (sum_c num[c][k][j]) / den,  chain_w[c][k] = e_c / den
// (NaN where no chain holds a sample; chain_w = 0 for an empty chain among others).
constexpr int GR = 1024;      // bank rows per workgroup of the gradient pass
constexpr int CT = 128;       // columns per output tile
constexpr int KS = CT + 16;   // row stride of the kept X tile (doubles)
constexpr int WS = PR + 2;    // row stride of the transposed weights (doubles)
constexpr int NH = CT / (16 * (BS / 64));   // 16-column MFMA tiles per wave
static_assert(GR % PR == 0 && CT % JC == 0 && NH * 16 * (BS / 64) == CT, "gradient tile shapes");
static_assert(TMOD * WS <= 2 * PR * LDW, "the weights reuse the staging LDS");

__global__ __launch_bounds__(BS) void k_brs_grad(const double* __restrict__ X, const double* __restrict__ r, int cap,
                                                 int n, int Jp, int Ju, int K, const double* __restrict__ Y,
                                                 const double* __restrict__ mref, double* __restrict__ part,
                                                 int nblk, int nkt, int nct) {
    __shared__ __attribute__((aligned(16))) double lds[2 * PR * LDW + PR * KS];
    double* s_x = lds;
    double* s_y = lds + PR * LDW;
    double* s_w = lds;                                         // after a pass's last stage
    double* s_keep = lds + 2 * PR * LDW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, kq = lane >> 4;
    int bi = blockIdx.x;
    const int kt = bi % nkt; bi /= nkt;
    const int ct = bi % nct; bi /= nct;
    const int blk = bi % nblk, chain = bi / nblk;
    const int k0 = kt * TMOD, c0 = ct * CT;
    const int row_s = blk * GR;
    const int nrows = n - row_s < GR ? n - row_s : GR;          // > 0: nblk = ceil(n / GR)
    const int nq = K - k0 >= TMOD ? NQ : (K - k0 + 15) / 16;    // 16-model tiles that hold a model
    const int cw = c0 + 32 * wave;                              // the wave's first column
    const int hn = cw >= Jp ? 0 : (Jp - cw > 16 ? NH : 1);      // its 16-column tiles that hold a column
    const double* Xc = X + (long long)chain * cap * Jp;
    const double* rc = r + (long long)chain * cap;
    const int nchunk = (Jp + JC - 1) / JC;
    const int npass = (nrows + PR - 1) / PR;
    const int total = npass * nchunk;
    const int sc = tid & (JC - 1), sr = tid / JC;

    double vx[SE], vy[SE];
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
            const int km = k0 + sr + (BS / JC) * e;
            vy[e] = (j < Ju && km < K) ? Y[(long long)km * Ju + j] : 0.0;
        }
    };

    double mr[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) mr[q] = (k0 + 16 * q + rl < K) ? mref[k0 + 16 * q + rl] : 0.0;
    f64x4 acc[NQ];
    f64x4 nacc[NQ][NH];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int h = 0; h < NH; ++h) nacc[q][h] = f64x4{0.0, 0.0, 0.0, 0.0};
    double rr[4];

    issue(0);
    for (int s = 0; s < total; ++s) {
        const int pass = s / nchunk, ch = s - pass * nchunk;
        const bool mine = ch * JC >= c0 && ch * JC < c0 + CT;   // a stage of the workgroup's column tile
#pragma unroll
        for (int e = 0; e < SE; ++e) {
            s_x[(sr + (BS / JC) * e) * LDW + sc] = vx[e];
            s_y[(sr + (BS / JC) * e) * LDW + sc] = vy[e];
            if (mine) s_keep[(sr + (BS / JC) * e) * KS + ch * JC - c0 + sc] = ((vok >> e) & 1u) ? vx[e] : 0.0;
        }
        __syncthreads();
        if (s + 1 < total) issue(s + 1);
        const int wrow = pass * PR + 16 * wave;                 // the wave's first row within the block
        const bool live = wrow < nrows;
        if (ch == 0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
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
            for (int ks = 0; ks < nks; ++ks) {
                const double a = ap[4 * ks];
                double b[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) b[q] = bp[16 * q * LDW + 4 * ks];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (q < nq) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc[q], 0, 0, 0);
            }
        }
        __syncthreads();                                       // the stage has been read
        if (ch == nchunk - 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double ri = rr[g];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double w = 0.0;
                    if (live && ri == ri && q < nq && k0 + 16 * q + rl < K) w = exp((ri - acc[q][g]) - mr[q]);
                    s_w[(16 * q + rl) * WS + 16 * wave + kq + 4 * g] = w;
                }
            }
            __syncthreads();
            const int prow = nrows - pass * PR;                 // rows of this pass (the rest hold w = 0, x = 0)
            const int nks = ((prow < PR ? prow : PR) + 3) / 4;
            if (hn > 0) {
                const double* ap = s_w + rl * WS + kq;
                const double* bp = s_keep + kq * KS + 32 * wave + rl;
                for (int ks = 0; ks < nks; ++ks) {
                    double a[NQ], b[NH];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) a[q] = ap[16 * q * WS + 4 * ks];
#pragma unroll
                    for (int h = 0; h < NH; ++h) b[h] = bp[4 * ks * KS + 16 * h];
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int h = 0; h < NH; ++h)
                            if (q < nq && h < hn)
                                nacc[q][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[h], nacc[q][h], 0, 0, 0);
                }
            }
            __syncthreads();                                   // the weights and the kept tile have been read
        }
    }
    double* po = part + ((long long)chain * nblk + blk) * K * Jp;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int km = k0 + 16 * q + kq + 4 * g, j = cw + 16 * h + rl;
                if (q < nq && h < hn && km < K && j < Jp) po[(long long)km * Jp + j] = nacc[q][h][g];
            }
}

// one thread per (chain, model, column): the blocks of a chain in block order
__global__ __launch_bounds__(BS) void k_brs_grad_combine(const double* __restrict__ part, int K, int Jp, int Ju,
                                                         int nblk, long long total, double* __restrict__ num) {
    const long long e = (long long)blockIdx.x * BS + threadIdx.x;
    if (e >= total) return;
    const long long kj = (long long)K * Jp;
    const long long chain = e / kj, o = e - chain * kj;
    double a = 0.0;
    if ((int)(o % Jp) < Ju)
        for (int b = 0; b < nblk; ++b) a = add(a, part[(chain * nblk + b) * kj + o]);
    num[e] = a;
}

__global__ __launch_bounds__(BS) void k_brs_grad_finish(const double* __restrict__ num, const double* __restrict__ state,
                                                        int C, int K, int Jp, int Ju, double* __restrict__ xbar,
                                                        double* __restrict__ chain_w) {
    const int t = threadIdx.x, k = blockIdx.x;
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
    for (int j = t; j < Ju; j += BS) {
        double a = 0.0;
        for (int c = 0; c < C; ++c) a = add(a, num[((long long)c * K + k) * Jp + j]);
        xbar[(long long)k * Ju + j] = any ? a / den : qnan();
    }
    for (int c = t; c < C; c += BS) {
        const double S = fS[(long long)c * K + k];
        double w = 0.0;
        if (S > 0.0) w = mul(S, exp(sub(fm[(long long)c * K + k], M))) / den;
        chain_w[(long long)c * K + k] = any ? w : qnan();
    }
}

int nblocks(int n) { return (n + GR - 1) / GR; }

int check_bank(const char* what, long long nchains, long long cap, int Ju) {
    if (nchains < 1) return set_error(std::string(what) + ": nchains >= 1 needed");
    if (cap < 1) return set_error(std::string(what) + ": bank capacity cap >= 1 needed");
    if (Ju < 1) return set_error(std::string(what) + ": used columns Ju >= 1 needed");
    if (nchains * cap > 0x7fffffffLL) return set_error(std::string(what) + ": too many bank rows (nchains * cap)");
    return 0;
}

int nslices(int n) { return (n + SL - 1) / SL; }

}  // namespace

extern "C" {

int gs_brs_info(int* slice_rows, int* model_tile) {
    if (!slice_rows || !model_tile) return set_error("gs_brs_info: null argument");
    *slice_rows = SL;
    *model_tile = TMOD;
    return 0;
}

int gs_brs_work_bytes(int nchains, int n, int K, long long* bytes) {
    if (!bytes) return set_error("gs_brs_work_bytes: null argument");
    if (nchains < 1 || n < 0) return set_error("gs_brs_work_bytes: nchains >= 1 and n >= 0 needed");
    if (K < 1) return set_error("gs_brs_work_bytes: models K >= 1 needed");
    *bytes = 8LL * 3 * nchains * (long long)(n > 0 ? nslices(n) : 1) * K;
    return 0;
}

int gs_brs_append(double* X, double* r, int nchains, int cap, int Ju, int nspec, int maxbins, const int* cols,
                  const int* kind, const double* coef, const double* scales, int capacity, uint32_t first_iteration,
                  int nsteps, int row0, void* stream) {
    if (!X || !r) return set_error("gs_brs_append: null bank");
    if (check_bank("gs_brs_append", nchains, cap, Ju)) return -1;
    if (nspec < 1 || nspec > 32 || maxbins < 1)
        return set_error("gs_brs_append: maxbins >= 1 and nspec in [1, 32] out of range");
    if ((long long)nchains * nspec * maxbins > (1LL << 28)) return set_error("gs_brs_append: too many series");
    if (Ju > nspec * maxbins) return set_error("gs_brs_append: used columns Ju out of range [1, nspec * maxbins]");
    if (capacity < 1 || nsteps < 0 || nsteps > capacity || first_iteration < 1)
        return set_error("gs_brs_append: need capacity >= 1, 0 <= nsteps <= capacity, first_iteration >= 1");
    if (row0 < 0 || (long long)row0 + nsteps > cap)
        return set_error("gs_brs_append: rows row0 .. row0 + nsteps - 1 must lie in the bank (row0 + nsteps <= cap)");
    if (nsteps == 0) return 0;
    if (!cols || !kind || !coef || !scales) return set_error("gs_brs_append: null table or scale trace");
    const long long nb = (long long)nsteps * nchains;
    if (nb > 0x7fffffffLL) return set_error("gs_brs_append: too many (row, chain) workgroups for one launch");
    const int Jp = (Ju + 3) / 4 * 4;
    const int slot0 = (int)((first_iteration - 1) % (uint32_t)capacity);
    hipLaunchKernelGGL(k_brs_pack, dim3((unsigned)nb), dim3(BS), 0, (hipStream_t)stream, X, r, nchains, cap, Jp, Ju,
                       nspec * maxbins, maxbins, cols, kind, coef, scales, capacity, slot0, row0);
    GS_LAUNCH_CHECK("k_brs_pack");
    return 0;
}

int gs_brs_eval(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                void* work, long long work_bytes, void* state, void* stream) {
    if (!X || !r) return set_error("gs_brs_eval: null bank");
    if (!state) return set_error("gs_brs_eval: null state");
    if (check_bank("gs_brs_eval", nchains, cap, Ju)) return -1;
    if (K < 1) return set_error("gs_brs_eval: models K >= 1 needed");
    if ((long long)nchains * K > (1LL << 28)) return set_error("gs_brs_eval: too many (chain, model) pairs");
    if (n < 0 || n > cap) return set_error("gs_brs_eval: rows n must lie in [0, cap]");
    if (nchains > 65535) return set_error("gs_brs_eval: more than 65535 chains in one bank");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                                              // an empty state: the finish gives NaN
        GS_CHECK(hipMemsetAsync(state, 0, (size_t)(8LL * (HDR + 3LL * nchains * K + nchains)), st));
        return 0;
    }
    if (!Y || !work) return set_error("gs_brs_eval: null Y or workspace");
    const int nslice = nslices(n), nkt = (K + TMOD - 1) / TMOD;
    if (work_bytes < 8LL * 3 * nchains * (long long)nslice * K)
        return set_error("gs_brs_eval: the workspace is smaller than gs_brs_work_bytes");
    const long long nb = (long long)nchains * nslice * nkt;
    if (nb > 0x7fffffffLL) return set_error("gs_brs_eval: too many (chain, slice, model tile) workgroups");
    const int Jp = (Ju + 3) / 4 * 4;
    hipLaunchKernelGGL(k_brs_eval, dim3((unsigned)nb), dim3(BS), 0, st, X, r, cap, n, Jp, Ju, K, Y, (double*)work,
                       nslice, nkt);
    GS_LAUNCH_CHECK("k_brs_eval");
    const unsigned kb = (unsigned)((K + BS - 1) / BS);
    hipLaunchKernelGGL(k_brs_combine, dim3(kb, (unsigned)nchains), dim3(BS), 0, st, (const double*)work, r, cap, n,
                       nchains, K, nslice, (double*)state);
    GS_LAUNCH_CHECK("k_brs_combine");
    return 0;
}

int gs_brs_grad_info(int* block_rows, int* model_tile, int* column_tile) {
    if (!block_rows || !model_tile || !column_tile) return set_error("gs_brs_grad_info: null argument");
    *block_rows = GR;
    *model_tile = TMOD;
    *column_tile = CT;
    return 0;
}

int gs_brs_grad_work_bytes(int nchains, int n, int K, int Ju, long long* bytes) {
    if (!bytes) return set_error("gs_brs_grad_work_bytes: null argument");
    if (nchains < 1 || n < 0) return set_error("gs_brs_grad_work_bytes: nchains >= 1 and n >= 0 needed");
    if (K < 1 || Ju < 1) return set_error("gs_brs_grad_work_bytes: models K >= 1 and used columns Ju >= 1 needed");
    const long long Jp = (Ju + 3LL) / 4 * 4;
    *bytes = 8LL * nchains * (long long)(n > 0 ? nblocks(n) : 1) * K * Jp;
    return 0;
}

int gs_brs_grad(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                const double* mref, void* work, long long work_bytes, double* num, void* stream) {
    if (!X || !r) return set_error("gs_brs_grad: null bank");
    if (!num) return set_error("gs_brs_grad: null num");
    if (check_bank("gs_brs_grad", nchains, cap, Ju)) return -1;
    if (K < 1) return set_error("gs_brs_grad: models K >= 1 needed");
    if ((long long)nchains * K > (1LL << 28)) return set_error("gs_brs_grad: too many (chain, model) pairs");
    if (n < 0 || n > cap) return set_error("gs_brs_grad: rows n must lie in [0, cap]");
    const int Jp = (Ju + 3) / 4 * 4;
    const long long total = (long long)nchains * K * Jp;
    if (total > (1LL << 37)) return set_error("gs_brs_grad: num [nchains][K][Jp] too large");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        GS_CHECK(hipMemsetAsync(num, 0, (size_t)(8LL * total), st));
        return 0;
    }
    if (!Y || !mref || !work) return set_error("gs_brs_grad: null Y, mref or workspace");
    const int nblk = nblocks(n), nkt = (K + TMOD - 1) / TMOD, nct = (Jp + CT - 1) / CT;
    if (work_bytes < 8LL * nblk * total)
        return set_error("gs_brs_grad: the workspace is smaller than gs_brs_grad_work_bytes");
    const long long nb = (long long)nchains * nblk * nkt * nct;
    if (nb > 0x7fffffffLL) return set_error("gs_brs_grad: too many (chain, block, model tile, column tile) workgroups");
    hipLaunchKernelGGL(k_brs_grad, dim3((unsigned)nb), dim3(BS), 0, st, X, r, cap, n, Jp, Ju, K, Y, mref,
                       (double*)work, nblk, nkt, nct);
    GS_LAUNCH_CHECK("k_brs_grad");
    hipLaunchKernelGGL(k_brs_grad_combine, dim3((unsigned)((total + BS - 1) / BS)), dim3(BS), 0, st,
                       (const double*)work, K, Jp, Ju, nblk, total, num);
    GS_LAUNCH_CHECK("k_brs_grad_combine");
    return 0;
}

int gs_brs_grad_finish(const double* num, const void* state, int C, int K, int Ju, double* xbar, double* chain_w,
                       void* stream) {
    if (!num || !state || !xbar || !chain_w) return set_error("gs_brs_grad_finish: null argument");
    if (C < 1 || K < 1 || Ju < 1) return set_error("gs_brs_grad_finish: C, K and Ju >= 1 needed");
    if ((long long)C * K > (1LL << 28)) return set_error("gs_brs_grad_finish: too many (chain, model) pairs");
    const int Jp = (Ju + 3) / 4 * 4;
    hipLaunchKernelGGL(k_brs_grad_finish, dim3((unsigned)K), dim3(BS), 0, (hipStream_t)stream, num,
                       (const double*)state, C, K, Jp, Ju, xbar, chain_w);
    GS_LAUNCH_CHECK("k_brs_grad_finish");
    return 0;
}

}  // extern "C"
