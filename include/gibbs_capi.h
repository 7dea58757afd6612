/*
 * gibbs_capi.h -- C-ABI of libgibbs_hip.so, the MI355X-native Gibbs hot path.
 *
 * Plain pointers and sizes only.  All array pointers passed to gs_* compute
 * calls are DEVICE pointers (caller-owned, e.g. torch tensor.data_ptr());
 * gs_model_desc carries HOST pointers that are copied once at plan creation.
 * Every compute call is asynchronous on the given hipStream_t (passed as
 * void*, NULL = default stream) and returns 0 on success, <0 on error with a
 * message in gs_last_error().  A plan is bound to the device that was current
 * when it was created; it is not thread-safe.  No call allocates, copies
 * host<->device or synchronises, so every step is capturable in a hipGraph.
 *
 * Reference interfaces replaced (Gabriel-Ducrocq/GibbsSampler, file:line):
 *   gs_var_expand            utils.generate_var_cl             utils.py:114-147,
 *                            variance_expension.generate_var_cl_cython  variance_expension.pyx:8-33
 *   gs_real_to_complex       utils.real_to_complex             utils.py:49-60, variance_expension.pyx:84-100
 *   gs_complex_to_real       utils.complex_to_real             utils.py:63-76, variance_expension.pyx:65-81
 *   gs_remove_monopole_dipole  remove_monopole_dipole_contributions  variance_expension.pyx:103-111
 *   gs_alm2cl                hp.alm2cl on real-layout a_lm     CenteredGibbs.py:30,61
 *   gs_unfold_bins           utils.unfold_bins                 utils.py:150-162
 *   gs_block_params          per-l Sigma/Cholesky of the CR    CenteredGibbs.py:324-337 (centered),
 *                            NonCenteredGibbs.py:141-151 (non-centered); TEB 3x3 semantics of the
 *                            cp38 helpers compute_inverse_and_cholesky / compute_sigma_and_chol
 *   gs_cr_sweep              the Gaussian CR draw + alm2cl/sufficient-statistic reduction
 *                            CenteredGibbs.py:340-353, NonCenteredGibbs.py:160-176
 *   gs_cls_draw              PolarizedCenteredClsSampler.sample CenteredGibbs.py:54-93 (+ TEB inverse-Wishart)
 *   gs_nc_mh                 PolarizationNonCenteredClsSampler.sample NonCenteredGibbs.py:292-445 (all_sph)
 *   gs_stats_to_noncentered  ASIS non-centering s_nc = C^-1/2 s  ASIS.py:185-189
 *   gs_step_centered / gs_step_noncentered / gs_step_asis
 *                            one iteration of GibbsSampler.run_polarization GibbsSampler.py:142-173,
 *                            NonCenteredGibbs.run_polarization NonCenteredGibbs.py:546-560,
 *                            ASIS.run_polarization ASIS.py:158-206
 *
 * Layouts (fp64):
 *   real a_lm layout, NR = (L+1)^2 per field (utils.py:49-76); alm arrays are
 *   [nchains][nfields][NR]; data d_alm is [nfields][NR] (shared by chains).
 *   binned spectra: [nchains][nspec][maxbins] (maxbins = max over spectra).
 *   statistics: [nchains][nstat][L+1], see GS_NSTAT_* below.
 *   fields: nfields=1 (T), 2 (E,B), 3 (T,E,B); spectra: [TT] / [EE,BB] /
 *   [TT,EE,BB,TE].
 *
 * RNG: replay mode when the variate pointer is non-NULL (host-drawn numpy
 * variates in the reference's draw order); native mode otherwise
 * (Philox4x32-10 keyed by (seed, global chain id), counter = (element,
 * field, tag|substep, iteration); independent of launch geometry).
 */
#ifndef GIBBS_CAPI_H
#define GIBBS_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 1

#define GS_MODE_CENTERED 0
#define GS_MODE_NONCENTERED 1

#define GS_QUIRK_ASIS_RECENTRE_CENTERED 1   /* ASIS.py:203 re-centres the centered map */

/* number of per-l statistics per chain, by nfields:
 *  1: [ssTT, dTsT]
 *  2: [ssEE, ssBB, dEsE, dBsB]
 *  3: [ssTT, ssEE, ssBB, ssTE, dTsT, dEsT, dEsE, dBsB]
 * ss = sum over the slots of l of s_X s_Y ; dXsY = sum of d_X s_Y. */
#define GS_NSTAT_1 2
#define GS_NSTAT_2 4
#define GS_NSTAT_3 8
#define GS_NPARAM 10   /* doubles per (chain, l) in a block-parameter table */

typedef struct gs_plan gs_plan;

typedef struct gs_model_desc {
    int lmax;                 /* L                                           */
    int nside;                /* HEALPix N_side (Npix = 12 N_side^2)          */
    int nfields;              /* 1, 2 or 3                                    */
    int nchains;              /* chains batched in this plan                  */
    int chain0;               /* global id of the plan's first chain (RNG key) */
    int quirks;               /* GS_QUIRK_* bit set                           */
    int n_iter_metropolis;    /* MH attempts per block (NonCenteredGibbs.py:427) */
    const double* bl;         /* host [L+1] beam b_l                          */
    const double* noise_var;  /* host [nfields] per-pixel noise variance      */
    const int* bins[4];       /* host bin edges per spectrum                  */
    int nbin_edges[4];        /* number of edges (= nbins + 1)                */
    const int* blocks[4];     /* host MH block edges per spectrum (nullable)  */
    int nblock_edges[4];
    const double* prop_var[4];/* host [nbins-2] MH proposal variances (nullable) */
} gs_model_desc;

int gs_abi_version(void);
const char* gs_last_error(void);

/* Library options: named settings read when a plan, SHT or masked context is
 * created (the library reads no environment variables).  Speed-only shape
 * selectors (every value gives the same bits) and the variant switches the
 * bit-identity tests compare, plus the f2 / table workspace budgets:
 *   GS_SWEEP_TW          1 | 2 | 4  CR-sweep workgroup shape (tiles x chunks;
 *                                   2 suits --skymap store, 1 the default)
 *   GS_SWEEP_PACK        0 | 1      packed diagonal workgroups of the native no-map
 *                                   throughput sweep at GS_SWEEP_TW=1 (default 1)
 *   GS_SWEEP_THROUGHPUT  1          few-chain plans use the throughput form
 *   GS_NC_RAW            0 | 1      raw-moment statistics of native NC sweeps
 *   GS_NC_PIPE           0 | 1      pipelined multi-step NC graphs (gs_nc_steps)
 *   GS_MH_SPLIT          0 | 1      NC MH in one / two workgroups per chain
 *   GS_CLS_PRE, GS_CLS_PRE_MANY  0 | 1  C_l-draw variates inside the sweep
 *   GS_F2_GROUP_BYTES, GS_F2_BATCH_BYTES  f2 workspace budgets (bytes)
 *   GS_SHT_LDS_FFT_MAX, GS_SHT_SEG, GS_SHT_SYN, GS_SHT_ANA, GS_SHT_MERGE_RINGS,
 *   GS_SHT_CONST_RINGS, GS_SHT_BLOCKS_MFMA, GS_SHT_BLK_STAGE, GS_SHT_FUSED_AUX,
 *   GS_SHT_MFMA_MAX_GB, GS_SHT_RING_TW2  SHT launch shapes / paths (gs_sht.hip
 *                        documents each)
 * gs_option_set(name, NULL) unsets; an unknown name is an error. */
int gs_option_set(const char* name, const char* value);
const char* gs_option_get(const char* name);   /* NULL when unset or unknown */

int gs_plan_create(const gs_model_desc* desc, gs_plan** out);
int gs_plan_destroy(gs_plan* plan);
/* query sizes of the plan's layouts */
int gs_plan_info(const gs_plan* plan, int* maxbins, int* nstat, int* nblocks_total, int* nspec);
/* tiling of the CR sweep: tasks per chain, m-rows per task */
int gs_plan_sweep_info(const gs_plan* plan, int* ntask, int* rows_per_task);
/* the packed grid of the native no-map throughput sweep (option GS_SWEEP_PACK):
 * per chain, the workgroups that run the packed form and the one-entry chunk
 * groups they absorb; both 0 where the plan keeps the plain grid alone */
int gs_plan_sweep_pack_info(const gs_plan* plan, int* npacked, int* nabsorbed);
/* the form of the NC MH decision launch: reg_form 1 when the plan takes the
 * register / LDS-resident kernel (one multipole per thread), 0 otherwise */
int gs_plan_mh_info(const gs_plan* plan, int* reg_form);

/* ---- stand-alone layout / expansion helpers (no plan needed) ---------------- */
int gs_var_expand(int lmax, int n, const double* dl, double* var, void* stream);
int gs_real_to_complex(int lmax, int n, const double* re, double* cplx_interleaved, void* stream);
int gs_complex_to_real(int lmax, int n, const double* cplx_interleaved, double* re, void* stream);
int gs_remove_monopole_dipole(int lmax, int n, double* alm, void* stream);
int gs_alm2cl(int lmax, int n, const double* x, const double* y, double* cl, void* stream);
int gs_unfold_bins(int n, const double* binned, const int* bins, int nbins, double* out, void* stream);

/* ---- plan-level hot-path stages ------------------------------------------- */
/* per-(chain, l) (M, Cholesky) table of the CR: s = M d + Lchol z */
int gs_block_params(gs_plan* plan, int mode, const double* dl_binned, double* params, void* stream);
/* fused CR draw + statistics: writes s (nullable => not stored) and stats */
int gs_cr_sweep(gs_plan* plan, const double* d_alm, const double* params, const double* z_replay,
                uint64_t seed, uint32_t iteration, uint32_t substep,
                double* s_out, double* stats, void* stream);
/* statistics (alm2cl auto/cross + data correlations) of a given s
 * [nchains][nfields][NR] -- hp.alm2cl of CenteredGibbs.py:30,61 */
int gs_sweep_stats(gs_plan* plan, const double* d_alm, const double* s, double* stats, void* stream);
/* centered C_l draw (inverse-Gamma; TEB: inverse-Wishart TT/EE/TE) */
int gs_cls_draw(gs_plan* plan, const double* stats, const double* invgamma_replay,
                uint64_t seed, uint32_t iteration, double* dl_binned_out, void* stream);
/* Scale trace of the centered C_l draw: a caller-owned DEVICE ring scales
 * [capacity][nchains][nspec][maxbins] (fp64, the layout of the D_l trace ring)
 * attached to the plan.  While it is attached, every C_l draw of the plan --
 * gs_cls_draw, gs_step_centered[_fused], gs_step_asis[_fused] -- records, in
 * the launch that holds the sums and in slot (iteration - 1) % capacity, the
 * scale of the conditional it samples (CenteredGibbs.py:54-93):
 *   inverse-Gamma spectra (T alone; EE, BB of EB; BB of TEB): beta_b =
 *     sum_{l in b} l(l+1)/(4 pi) sum_m s_lm^2, the bits that multiply the
 *     variate (a replayed draw is dl == scales * invgamma_replay bit for bit);
 *   the TEB block: the entries of the inverse-Wishart scale Psi_b =
 *     sum_{l in b} l(l+1)/(2 pi) sum_m s_lm s_lm^T -- Psi_TT in the TT slot,
 *     Psi_EE in the EE slot, Psi_TE in the TE slot;
 *   bins 0, 1 and the bins past a spectrum's count: 0.
 * scales NULL detaches the ring; with none attached the draw stores nothing
 * more and every output keeps its bits.  A captured graph holds the pointer as
 * a kernel argument, so attach or detach between captures: the call fails
 * while `stream` (the stream the steps are launched on) is being captured. */
int gs_cls_scale_trace(gs_plan* plan, double* scales, int capacity, void* stream);
/* non-centered Metropolis-within-Gibbs over blocks (in/out dl_binned) */
/* proposals of the NC Metropolis step (NonCenteredGibbs.py:292-330) into caller
 * buffers [nchains][nspec][maxbins] (prop, log proposal ratio) and, when
 * u_acc_out != NULL, the native accept uniforms [nchains][nacc]; used by the
 * pixel-domain (masked) MH whose block loop needs a full SHT per block. */
int gs_mh_propose(gs_plan* plan, const double* dl, const double* u_prop, uint64_t seed, uint32_t iteration,
                  double* prop_out, double* logr_out, double* u_acc_out, void* stream);
int gs_nc_mh(gs_plan* plan, const double* stats, double* dl_binned,
             const double* u_prop_replay, const double* u_accept_replay,
             uint64_t seed, uint32_t iteration, int32_t* accept_out, void* stream);
/* Warm-up adaptation of the NC Metropolis proposal scales (Robbins-Monro, per
 * chain and MH block).  State: a log-scale lam and a step count n, both
 * [nchains][nblocks] with nblocks = nblocks_total / n_iter_metropolis and block
 * j in the order of the accept flags (flags j * n_iter_metropolis ... of a
 * chain belong to block j).  gs_mh_adapt, after the decisions of one step:
 *   abar = mean of the block's accept flags,  n <- n + 1,
 *   lam <- clamp(lam + n^-kappa (abar - target), -20, 20),
 *   sd[chain][spectrum][bin] = sd0[spectrum][bin] exp(lam[chain][block of bin])
 * with sd0 the sqrt of the plan's proposal variances.
 * gs_mh_adapt_enable allocates the state (lam = 0, n = 0) and the per-chain
 * table and makes every proposal-drawing launch of the plan read that table
 * (at lam = 0 it holds sd0: the same proposals, bit for bit); a second call
 * only changes target / kappa.  It synchronises the device: call it outside
 * a capture.  A plan without MH blocks or proposal variances is an error.
 * gs_mh_adapt is two small launches on the stream (capturable, no host
 * synchronisation): call it after the step's decide launch and before the
 * next launch that draws proposals.  Not calling it freezes the scales.
 * gs_mh_scale_get / _set copy lam (and n, nullable) from / to DEVICE buffers;
 * set rebuilds the table by the code gs_mh_adapt uses, so restored scales give
 * the same table bit for bit.  gs_mh_proposal_sd copies the table the
 * proposals read to sd_out [nchains][nspec][maxbins] (adaptation on or off). */
int gs_mh_adapt_enable(gs_plan* plan, double target, double kappa);
int gs_mh_adapt(gs_plan* plan, const int32_t* accept, void* stream);
int gs_mh_scale_get(gs_plan* plan, double* log_scale, int32_t* count, void* stream);
int gs_mh_scale_set(gs_plan* plan, const double* log_scale, const int32_t* count, void* stream);
int gs_mh_proposal_sd(gs_plan* plan, double* sd_out, void* stream);
/* stats of s_nc = A(C)^+ s with A = chol(C(dl_binned)) (ASIS non-centering) */
int gs_stats_to_noncentered(gs_plan* plan, const double* dl_binned, double* stats, void* stream);
/* s <- T_l s for T_l = A(C(dl_new)) [A(C(dl_old))^+ unless dl_old NULL] */
int gs_recentre(gs_plan* plan, const double* dl_new, const double* dl_old, double* s, void* stream);

/* ---- fused iterations ------------------------------------------------------ */
int gs_step_centered(gs_plan* plan, const double* d_alm, double* dl_binned, double* s_out,
                     const double* z_replay, const double* invgamma_replay,
                     uint64_t seed, uint32_t iteration, void* stream);
/* native RNG, device iteration counter on (graph-captured steps): gs_step_centered
 * with the D_l trace record (trace nullable: [capacity][nchains][nspec][maxbins],
 * slot (iteration - 1) % capacity) and the counter advance in the C_l-draw launch */
int gs_step_centered_fused(gs_plan* plan, const double* d_alm, double* dl_binned, double* s_out,
                           uint64_t seed, uint32_t iteration, double* trace, int capacity, void* stream);
/* the same for gs_step_asis (native): trace record and counter advance in the MH launch */
int gs_step_asis_fused(gs_plan* plan, const double* d_alm, double* dl_binned, double* s_out,
                       uint64_t seed, uint32_t iteration, int32_t* accept_out, double* dl_tmp_out, int recentre,
                       double* trace, int capacity, void* stream);
int gs_step_noncentered(gs_plan* plan, const double* d_alm, double* dl_binned, double* s_out,
                        const double* z_replay, const double* u_prop_replay, const double* u_accept_replay,
                        uint64_t seed, uint32_t iteration, int32_t* accept_out, void* stream);
/* the three stages of gs_step_noncentered, for callers that schedule them:
 *   gs_nc_prologue  the MH proposals (and native accept uniforms) of dl
 *                   (NonCenteredGibbs.py:292-330) and, for plans of more than 4
 *                   chains, the NC block parameters of dl (:134-176)
 *   gs_nc_sweep     the CR draw + sufficient statistics; plans of <= 4 chains
 *                   compute the NC operator of dl per l inside the sweep
 *   gs_nc_decide    the Metropolis-within-Gibbs decisions (NonCenteredGibbs.py:401-445)
 * Native RNG, plans of more than 4 chains: the prologue launches the block
 * parameters only and the proposals / accept uniforms are drawn by the launch
 * that reduces the statistics (gs_nc_sweep with finish = 1, or gs_nc_finish);
 * the decide calls fail if that launch has not run since the prologue.  With
 * GS_NC_MH_PARAMS=1 at plan creation, inside a captured multi-step graph
 * (gs_graph_step offset > 0) the previous step's gs_nc_decide_fused wrote this
 * step's parameters and the prologue launches nothing.  GS_NC_PRO_DEFER=0: all
 * in the prologue (the same values either way). */
int gs_nc_prologue(gs_plan* plan, const double* dl_binned, const double* u_prop_replay, uint64_t seed,
                   uint32_t iteration, void* stream);
/* Raw-moment statistics (native draws; option GS_NC_RAW=0 at plan creation turns
 * them off).  The NC draw is s = P d + Q z with P, Q the operator of the chain's
 * D_l, so the per-l statistics sum s s^T and sum d s^T follow from the
 * state-independent moments sum z z^T, sum d z^T and sum d d^T.  gs_nc_sweep
 * with z_replay NULL accumulates the first two (it reads no operator unless
 * s_out is given), and the statistics finish applies the operator of dl_binned
 * to them and to the data moments; the step then has no parameter launch unless
 * the map is stored.
 * gs_data_moments computes sum_m d d^T per l of the data tensor d_alm
 * [nfields][(lmax+1)^2] into the plan and remembers the pointer.  Call it once
 * per data tensor.  gs_nc_sweep makes the call itself when it is handed a
 * pointer other than the remembered one, but it cannot see an in-place change:
 * after writing new values into the same d_alm buffer, call gs_data_moments
 * again before the next step. */
int gs_data_moments(gs_plan* plan, const double* d_alm, void* stream);
int gs_nc_sweep(gs_plan* plan, const double* d_alm, const double* dl_binned, double* s_out, const double* z_replay,
                uint64_t seed, uint32_t iteration, int finish, void* stream);
/* finish = 0 leaves the statistics as per-task partials; gs_nc_finish reduces them
 * (fixed order) -- lets a caller bracket the sweep kernel alone with timing events */
int gs_nc_finish(gs_plan* plan, void* stream);
/* copies the statistics the last gs_nc_sweep / gs_nc_finish reduced (the rows the
 * MH reads) to stats_out [nchains][nstat][lmax+1] */
int gs_nc_stats(gs_plan* plan, double* stats_out, void* stream);
int gs_nc_decide(gs_plan* plan, double* dl_binned, const double* u_accept_replay, uint64_t seed, uint32_t iteration,
                 int32_t* accept_out, void* stream);
/* gs_nc_decide with the step's bookkeeping fused into the same launch (native
 * RNG, for graph-captured steps): after the decisions each chain's workgroup
 * records its D_l in trace (nullable; trace[(it-1) % capacity]) and, with the
 * device counter on, the last workgroup advances the counter (ticket; every
 * workgroup read it at its start). */
int gs_nc_decide_fused(gs_plan* plan, double* dl_binned, uint64_t seed, uint32_t iteration, int32_t* accept_out,
                       double* trace, int capacity, void* stream);
/* The pipelined NC schedule (native RNG, raw-moment statistics, no stored map;
 * option GS_NC_PIPE=0 at plan creation turns it off).  Such a sweep reads the
 * data and the counters only, never the chain's D_l, so the sweep of step i + 1
 * runs while the statistics finish and the MH of step i run; only finish -> MH
 * -> finish stays serial.
 * gs_nc_pipe_prepare sets *on to whether the plan pipelines and, the first time
 * it does, allocates a second buffer of statistic partials, a side stream and
 * the fork / join events: call it outside a stream capture.
 * gs_nc_steps emits nsteps whole steps on `stream` and the plan's side stream
 * (joined back into `stream` before it returns: capturable into one hipGraph).
 * It needs the device iteration counter: step i reads base + i, and the last
 * step's decide launch advances the base by nsteps after every sweep has read
 * it; gs_graph_step is back at (0, 1) afterwards.  Step i writes its accept
 * flags to accept + i * accept_stride (stride 0: one buffer), records D_l in
 * trace (nullable) as gs_nc_decide_fused does and, with adapt != 0, runs
 * gs_mh_adapt on its flags before the next step's proposals.  time_every > 0:
 * the sweep of every time_every-th step is bracketed for gs_sweep_timing on the
 * side stream that runs it (the time includes sharing the GPU with the previous
 * step's finish and MH); 0 leaves the timing state alone.  The results are those
 * of nsteps times gs_nc_prologue, gs_nc_sweep, gs_nc_decide_fused, bit for bit. */
int gs_nc_pipe_prepare(gs_plan* plan, int* on);
int gs_nc_steps(gs_plan* plan, const double* d_alm, double* dl_binned, uint64_t seed, int nsteps,
                int32_t* accept_out, long long accept_stride, double* trace, int capacity, int adapt,
                int time_every, void* stream);
/* dl_tmp_out: nullable, receives the centered draw; recentre: 0 lazy (s_out keeps the
 * centered CR draw), 1 materialise the re-centred map in s_out */
int gs_step_asis(gs_plan* plan, const double* d_alm, double* dl_binned, double* s_out,
                 const double* z_replay, const double* invgamma_replay,
                 const double* u_prop_replay, const double* u_accept_replay,
                 uint64_t seed, uint32_t iteration, int32_t* accept_out, double* dl_tmp_out,
                 int recentre, void* stream);

/* hipGraph support: with the device counter enabled every RNG-consuming
 * kernel reads the iteration as a device base word plus the step's offset
 * (the host iteration argument is ignored), so a captured graph replays as
 * the next iterations.  gs_graph_step(offset, advance) sets the offset of the
 * steps launched next (0 after gs_iteration_counter) and how far the fused
 * entry points' last launch advances the base (1 after gs_iteration_counter:
 * one captured step per replay; a graph of K steps passes offsets 0..K-1 and
 * advance K on its last step, 0 on the others -- one ticket per replay).
 * gs_advance_iteration increments the base by one from the stream. */
int gs_iteration_counter(gs_plan* plan, int enable, uint32_t start);
int gs_graph_step(gs_plan* plan, uint32_t offset, uint32_t advance);
int gs_advance_iteration(gs_plan* plan, void* stream);
/* trace[(it-1) % capacity][nchains][nspec][maxbins] <- dl_binned (history of GibbsSampler.py:172-173) */
int gs_record_trace(gs_plan* plan, const double* dl_binned, double* trace, int capacity, uint32_t iteration,
                    void* stream);

/* ---- streaming posterior summaries of the D_l chains (gs_summary.hip) ----------
 * Plan-independent: they summarise any trace tensor [capacity][nchains][nspec]
 * [maxbins] (fp64; the layout of gs_record_trace and of the fused steps' trace
 * ring).  A series is one (chain, spectrum, bin); the state is a caller-owned
 * DEVICE buffer of gs_summary_bytes bytes (8-byte aligned) holding, per series
 * in fp64, the first sample r, the Welford mean and M2, min, max, S = sum y_t
 * with y_t = x_t - r, the lag products P_j = sum_{t > j} y_t y_{t-j} for
 * j = 1..max_lag (0 <= max_lag <= 64) and the first and last max_lag values of
 * y, then int64 accept counts [nchains][nacc]; one int64 sample count n for
 * the whole state (gs_summary.hip documents the layout and every formula).
 * gs_summary_reset zeroes the state.
 * gs_summary_update adds the nsteps consecutive iterations first_iteration,
 * first_iteration + 1, ... (iteration it lies in slot (it - 1) % capacity;
 * nsteps <= capacity, first_iteration >= 1) in one launch, in iteration order
 * per series: the state's bits do not depend on how the iterations were cut
 * into launches.  accept_trace (nullable): int32 flags, step i of this call at
 * accept_trace + i * accept_stride, [nchains][nacc]; they are added into the
 * counts.  Successive updates of one state must be ordered on one stream.
 * gs_summary_finish, one thread per (spectrum, bin) over the C chains of a
 * state (C need not be a plan's chain count: a state whose per-series fields
 * were all-gathered along the chain axis is summarised over every rank's
 * chains).  Outputs, DEVICE fp64 with nsb = nspec * maxbins fastest:
 *   pooled     [7][nsb]  mean, variance, min, max, ess, ess_truncated (0 / 1), rhat
 *   chain_mean [C][nsb], chain_var [C][nsb]
 *   acf        [max_lag + 1][nsb]  the multi-chain autocorrelation rho_j
 *   gamma      [C][max_lag + 1][nsb]  per-chain autocovariances (divisor n)
 * rhat is Gelman-Rubin's sqrt(var+ / W); ess = C n / tau with Geyer's initial
 * monotone positive sequence over the pairs rho_2k + rho_2k+1 up to max_lag,
 * ess_truncated = 1 when no negative pair ended the sum (ess is then an upper
 * estimate).  W == 0: rhat, ess and rho are NaN; C == 1: rhat is NaN; n <= j:
 * gamma_j is NaN. */
int gs_summary_bytes(int nchains, int nspec, int maxbins, int nacc, int max_lag, long long* bytes /* HOST */);
int gs_summary_reset(void* state, int nchains, int nspec, int maxbins, int nacc, int max_lag, void* stream);
int gs_summary_update(void* state, int nchains, int nspec, int maxbins, int nacc, int max_lag, const double* trace,
                      int capacity, uint32_t first_iteration, int nsteps, const int32_t* accept_trace,
                      long long accept_stride, void* stream);
int gs_summary_finish(const void* state, int C, int nspec, int maxbins, int max_lag, double* pooled,
                      double* chain_mean, double* chain_var, double* acf, double* gamma, void* stream);

/* ---- streaming posterior mean and variance of the sky map (gs_smap.hip) ---------
 * Plan-independent moments of a batch of fp64 series: C chains of length n
 * (n = F (L+1)^2 for a real-layout a_lm, ncomp N_pix for a map).  The state is
 * a caller-owned DEVICE buffer of gs_smap_bytes bytes (8-byte aligned; 16-byte
 * aligned for the widest accesses): 8 header doubles (int64 samples per chain
 * first), then the Welford mean [C][n] and M2 [C][n].
 * gs_smap_reset zeroes the state.
 * gs_smap_update adds one sample of every chain, chain c at x + c *
 * x_chain_stride (elements; n contiguous doubles), as sample number
 * count_after (1 for the first after a reset): d = x - mean; mean += d / k;
 * M2 += d (x - mean).  The count comes from the host, so nothing is read back
 * and the call is capturable; it allocates nothing.  One thread owns an
 * element and there are no atomics: the state's bits depend neither on the
 * launch geometry nor on C (chain b of a C-chain state = a one-chain state fed
 * chain b's data).  Successive updates of one state must be ordered on one
 * stream.
 * gs_smap_finish merges the C chains of a state in chain order (Chan's pairwise
 * update; C need not be the updating context's chain count: per-chain fields
 * all-gathered along the chain axis are merged over every rank's chains) with
 * the header's count k per chain.  Outputs, DEVICE fp64: mean [n], var [n] =
 * M2_total / (C k - 1) (NaN when C k < 2), chain_mean [C][n], rhat [n]
 * (Gelman-Rubin as gs_summary_finish; NaN for C = 1, k < 2 or W == 0).
 * gs_smap_power, for a real-layout a_lm state's pooled mean and var [F][(L+1)^2]:
 * per field and l, power_of_mean [F][L+1] = sum_m mean^2 / (2l+1), the spectrum
 * of the posterior mean map, and mean_power [F][L+1] = power_of_mean +
 * sum_m var / (2l+1), the posterior mean of the map's spectrum (auto spectra
 * only), summed in the fixed order m = 0, 1, .. l. */
int gs_smap_bytes(int C, long long n, long long* bytes /* HOST */);
int gs_smap_reset(void* state, int C, long long n, void* stream);
int gs_smap_update(void* state, int C, long long n, const double* x, long long x_chain_stride, long long count_after,
                   void* stream);
int gs_smap_finish(const void* state, int C, long long n, double* mean, double* var, double* chain_mean, double* rhat,
                   void* stream);
int gs_smap_power(int lmax, int nfields, const double* mean, const double* var, double* power_of_mean,
                  double* mean_power, void* stream);

/* ---- Rao-Blackwellised posterior sky map of the full-sky samplers (gs_wf.hip) ----
 * On the full sky the centered CR draw is s = M_l d + L_l z per l, so the
 * posterior of the map follows from the D_l chain alone: E[s_lm | d] = mean_i
 * M_l^i d_lm, Var[s_lm | d] = mean_i Sigma_l^i + Var_i(M_l^i d_lm), E[sigma_l | d]
 * = mean_i (Sigma_l^i + M_l^i S_l M_l^i^T / (2l+1)) with S_l = sum_m d_lm d_lm^T.
 * Plan-independent: any trace ring [capacity][nchains][nspec][maxbins] (nspec =
 * 1, 2, 4 for nfields = 1, 2, 3) is accumulated through the centered operator
 * (GS_MODE_CENTERED whatever sampler drew the D_l) of the DEVICE tables bl [L+1]
 * and ell2bin [nspec][L+1] (int32, -1: unbinned, read as D_l = 0) and the noise
 * weights k0..k2 = N_pix / (4 pi noise_var_f).  The state is a caller-owned DEVICE
 * buffer of gs_wf_bytes bytes (8-byte aligned): 8 header doubles (int64 samples
 * per chain first), then planes [nfld][nchains][L+1], l fastest -- the Welford
 * means of the operator entries (nfields 3: M00, M01, M10, M11, M22; else M_f),
 * the co-moment sums of the pairs that enter a slot's variance, the means of
 * Sigma (s00, s11, s01, s22; else s_f) and of the per-l power (TT, EE, BB, TE;
 * else per field); nfld = 20 for nfields 3, 4 nfields otherwise (gs_wf.hip
 * documents the layout and every formula).
 * gs_wf_reset zeroes the state.
 * gs_wf_moments: the data moments S_l [nspec][L+1] of a real-layout d_alm
 * [nfields][(L+1)^2] in spectrum order (TE = sum d_T d_E), rows added in the
 * order m = 0 .. l; once per data tensor.
 * gs_wf_update adds the nsteps consecutive iterations first_iteration,
 * first_iteration + 1, ... (iteration it lies in slot (it - 1) % capacity;
 * nsteps <= capacity, first_iteration >= 1) in one launch, one thread per
 * (chain, l), in iteration order; count_after is the samples per chain after
 * this call (given by the host: nothing is read back, the call is capturable
 * and allocates nothing).  No atomics: the state's bits depend neither on how
 * the iterations were cut into launches, nor on the capacity or a wrap, nor on
 * the launch geometry, nor on the other chains.  Successive updates of one
 * state must be ordered on one stream.
 * gs_wf_finish, one thread per (field, slot) of d_alm, merges the C chains in
 * chain order (Chan's update; C need not be the updating context's chain count:
 * planes all-gathered along the chain axis are merged over every rank's
 * chains).  Outputs, DEVICE fp64: alm_mean, alm_var, alm_rhat [nfields][(L+1)^2],
 * chain_alm_mean [C][nfields][(L+1)^2]; alm_var is NaN when C k < 2, alm_rhat
 * (Gelman-Rubin as gs_summary_finish on the series (M^i d)_f) for C = 1, k < 2
 * or W == 0.
 * gs_wf_power, one thread per l: power_of_mean [nspec][L+1] = Mbar S Mbar^T /
 * (2l+1), mean_power [nspec][L+1], the pooled mean of the streamed power, and
 * op_mean [nop][L+1] (nop = 5 for nfields 3, else nfields), the pooled operator:
 * the posterior-averaged Wiener-filter transfer function. */
int gs_wf_bytes(int nfields, int nchains, int lmax, long long* bytes /* HOST */);
int gs_wf_reset(void* state, int nfields, int nchains, int lmax, void* stream);
int gs_wf_moments(int lmax, int nfields, const double* d_alm, double* moments, void* stream);
int gs_wf_update(void* state, int nfields, int nchains, int lmax, int maxbins, const double* bl, const int* ell2bin,
                 double k0, double k1, double k2, const double* moments, const double* trace, int capacity,
                 uint32_t first_iteration, int nsteps, long long count_after, void* stream);
int gs_wf_finish(const void* state, int nfields, int C, int lmax, const double* d_alm, double* alm_mean,
                 double* alm_var, double* chain_alm_mean, double* alm_rhat, void* stream);
int gs_wf_power(const void* state, int nfields, int C, int lmax, const double* moments, double* power_of_mean,
                double* mean_power, double* op_mean, void* stream);

/* ---- streaming Blackwell-Rao marginal posteriors of the D_l (gs_br.hip) -------
 * The centered C_l draw samples D_b | s from an inverse-Gamma(alpha_b, beta_b)
 * (PolarizedCenteredClsSampler.sample, CenteredGibbs.py:54-93); the Blackwell-Rao
 * estimate averages that density over the sky samples,
 *   P(D_b | d) ~ 1/N sum_i IG(D_b; alpha_b, beta_b,i),
 * on a grid of G values per (spectrum, bin), 1 <= G <= 64.  Plan-independent:
 * any scale ring [capacity][nchains][nspec][maxbins] (gs_cls_scale_trace) is
 * accumulated.  DEVICE fp64 inputs: grid [nspec][maxbins][G] (D_g > 0,
 * increasing) and alpha [nspec][maxbins], the shape of each bin's conditional
 * -- n_b / 2 - 1 with n_b = l1^2 - l0^2 for the inverse-Gamma spectra, n_b / 2
 * - 2 for TT and EE of the TEB block (the diagonal of an inverse-Wishart(Psi,
 * nu = n_b - 3) in two dimensions is inverse-Gamma((nu - 1) / 2, Psi_ii / 2)),
 * NaN for TE, bins 0, 1 and unused bins, which are skipped and finish as NaN.
 * half_mask: bit k set halves the recorded scale of spectrum k (TEB: TT and EE).
 * The state is a caller-owned DEVICE buffer of gs_br_bytes bytes: 8 header
 * doubles (int64 iteration count first), then per (chain, spectrum, bin, g),
 * g fastest, the running maximum m and S = sum_i exp(t_i - m) of
 * t_i = alpha log beta_i - beta_i / D_g (two planes: all m, then all S;
 * 16 B x nchains x nspec x maxbins x G), then int64 bad [nchains][nspec], the
 * rows skipped because beta <= 0 or not finite.  gs_br_reset zeroes it.
 * gs_br_update adds iterations first_iteration ... first_iteration + nsteps - 1
 * (iteration it in slot (it - 1) % capacity; nsteps <= capacity) in one launch,
 * per state element in iteration order: the state's bits do not depend on how
 * the iterations were cut into launches.  Successive updates of one state must
 * be ordered on one stream.
 * gs_br_finish, over the C chains of a state (a state whose planes were
 * all-gathered along the chain axis is finished over every rank's chains):
 *   logpdf [nspec][maxbins][G] = logsumexp_c,i t - log(C n) - lgamma(alpha)
 *                                - (alpha + 1) log D_g
 *   mass   [nspec][maxbins]    the trapezoid integral of exp(logpdf) over the
 *                              bin's grid (near 1 when the grid covers the posterior)
 * gs_br.hip documents the layout and the order of every operation. */
int gs_br_bytes(int nchains, int nspec, int maxbins, int G, long long* bytes /* HOST */);
int gs_br_reset(void* state, int nchains, int nspec, int maxbins, int G, void* stream);
int gs_br_update(void* state, int nchains, int nspec, int maxbins, int G, const double* grid, const double* alpha,
                 unsigned half_mask, const double* scales, int capacity, uint32_t first_iteration, int nsteps,
                 void* stream);
int gs_br_finish(const void* state, int C, int nspec, int maxbins, int G, const double* grid, const double* alpha,
                 double* logpdf, double* mass, void* stream);

/* ---- streaming Blackwell-Rao likelihood of theory spectra (gs_brl.hip) ---------
 * The joint Blackwell-Rao estimate (Chu et al. 2005) for K fixed theory spectra,
 *   L(D^th_k | d) ~ 1/(C n) sum_{c,i} prod_b P(D^th_k,b | s_c,i),
 * P the inverse-Gamma density of an independent bin and the 2x2 inverse-Wishart
 * density of a TEB block (TT, EE, TE).  With x the row of the scale ring
 * [capacity][nchains][nspec][maxbins] (gs_cls_scale_trace) of one (iteration,
 * chain) and j over the Ju used columns, the log density up to a per-model
 * constant is t = r - sum_j x_j Y_kj with r = sum_j coef_j log(arg_j).  DEVICE
 * tables (built by the host, engine.br_likelihood_tables):
 *   cols [Ju] int32  ascending used columns (spectrum * maxbins + bin); the
 *                    other columns of the ring are never read
 *   kind [Ju] int32  0: no logarithm; 1: arg = x; 2: the TT column of a TEB
 *                    block, arg = x * x[col + maxbins] - x[col + 3 maxbins]^2
 *   coef [Ju] fp64   alpha_b (kind 1), nu_b / 2 (kind 2)
 *   Y    [K][Ju] fp64
 * The state is a caller-owned DEVICE buffer of gs_brl_bytes bytes: 8 header
 * doubles (int64 iteration count first), the planes m, S, Q [nchains][K] (24 B
 * per chain and model: running maximum of t, sum exp(t - m), sum exp(2 (t -
 * m))) and int64 bad [nchains], the rows skipped for a chain because a kind 1
 * value or a kind 2 determinant was <= 0 or not finite.  gs_brl_reset zeroes it.
 * gs_brl_update adds iterations first_iteration ... first_iteration + nsteps - 1
 * (iteration it in slot (it - 1) % capacity; nsteps <= capacity) in one launch;
 * every dot product is one fma chain over j ascending and every (chain, model)
 * is folded in iteration order, so the state's bits do not depend on how the
 * iterations were cut into launches, on the chain count or on K.  Successive
 * updates of one state must be ordered on one stream.
 * gs_brl_finish over the C chains of a state (planes all-gathered along the
 * chain axis: every rank's chains), cst [K] the models' constants (DEVICE):
 *   loglike [K], chain_loglike [C][K] (one chain's own estimate), neff [K] =
 *   (sum w)^2 / sum w^2 over the samples' weights, in [1, C n].
 * gs_brl.hip documents the layout and the order of every operation. */
int gs_brl_bytes(int nchains, int K, long long* bytes /* HOST */);
int gs_brl_reset(void* state, int nchains, int K, void* stream);
int gs_brl_update(void* state, int nchains, int nspec, int maxbins, int K, int Ju, const int* cols, const int* kind,
                  const double* coef, const double* Y, const double* scales, int capacity, uint32_t first_iteration,
                  int nsteps, void* stream);
int gs_brl_finish(const void* state, int C, int K, const double* cst, double* loglike, double* chain_loglike,
                  double* neff, void* stream);

/* ---- Blackwell-Rao sample bank (gs_brs.hip) -------------------------------------
 * The samples of a run kept for evaluating theory spectra named afterwards: what
 * gs_brl_update reads of every scale ring row, compressed to the Ju used columns.
 * Caller-owned DEVICE buffers, Jp = Ju rounded up to a multiple of 4:
 *   X [nchains][cap][Jp]  the ring's value at column cols[j] (columns >= Ju: 0)
 *   r [nchains][cap]      sum_j coef_j log(arg_j), formed as gs_brl_update forms
 *                         it; NaN for a row that estimator skips
 * cols, kind, coef: the tables of gs_brl_update (they do not depend on a theory).
 * gs_brs_append packs iterations first_iteration ... first_iteration + nsteps - 1
 * of the ring (slot rule of gs_brl_update, nsteps <= capacity) into bank rows
 * row0 ... row0 + nsteps - 1 of every chain, one launch; a bank row's bits depend
 * on its ring row alone.
 * gs_brs_eval scores Y [K][Ju] (engine.br_likelihood_tables) against bank rows
 * [0, n) on the fp64 matrix cores and writes a state in the layout of gs_brl_bytes
 * (header with n; m, S, Q [nchains][K]; bad [nchains]) for gs_brl_finish.  work: a
 * DEVICE buffer of gs_brs_work_bytes(nchains, n, K) bytes (per-slice partials).
 * The rows of a chain are folded in slices of slice_rows (gs_brs_info) and merged
 * in a fixed order: for given (n, Ju) the result of (chain, model) is bit-identical
 * whatever K, the other models and the other chains are; it differs from the
 * streaming state by the re-ordering of the n weights.  gs_brs.hip documents the
 * layout and the order of every operation. */
int gs_brs_info(int* slice_rows /* HOST */, int* model_tile /* HOST */);
int gs_brs_work_bytes(int nchains, int n, int K, long long* bytes /* HOST */);
int gs_brs_append(double* X, double* r, int nchains, int cap, int Ju, int nspec, int maxbins, const int* cols,
                  const int* kind, const double* coef, const double* scales, int capacity, uint32_t first_iteration,
                  int nsteps, int row0, void* stream);
int gs_brs_eval(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                void* work, long long work_bytes, void* state, void* stream);

/* The gradient of the bank's likelihood with respect to the tables: with w_cik =
 * exp(t_cik - M_k), d loglike_k / d Y_kj = -xbar_kj, xbar_kj = sum_ci w_cik x_cij /
 * sum_ci w_cik, the likelihood-weighted mean of the bank's scale columns under
 * theory k (engine.br_likelihood_grad carries it to d loglike / d D^th).
 * gs_brs_grad, a second pass over bank rows [0, n) after gs_brs_eval: mref [K]
 * (DEVICE; the caller's M_k, max_c m_c of the evaluated -- possibly gathered --
 * state), num [nchains][K][Jp] (DEVICE, output):
 *   num[c][k][j] = sum_i exp(t_cik - mref_k) x_cij,
 * t recomputed on the fp64 matrix cores with the bits of gs_brs_eval, the sum over
 * the rows a second MFMA contraction.  Rows whose r is NaN are never touched; the
 * padding columns j >= Ju are written as 0; n = 0 zeroes num.  work: a DEVICE
 * buffer of gs_brs_grad_work_bytes(nchains, n, K, Ju) bytes -- one [K][Jp] tile
 * per chain and block of block_rows rows, 8 nchains ceil(n / block_rows) K Jp
 * bytes -- whose blocks are added in block order.  gs_brs_grad_info: block_rows,
 * the model tile and the column tile (a workgroup recomputes t once per column
 * tile of its models).  For given (n, Ju, mref_k) the row num[c][k][.] is
 * bit-identical whatever K, the other models and the other chains are.
 * gs_brs_grad_finish over the C chains of num [C][K][Jp] and a state in the
 * layout of gs_brl_bytes (both possibly all-gathered along the chain axis), in
 * chain order, every step one rounded operation:
 *   M_k = max m_c over S_c > 0,  den_k = sum_c S_c exp(m_c - M_k)
 *   xbar [K][Ju] = (sum_c num[c][k][j]) / den_k
 *   chain_w [C][K] = S_c exp(m_c - M_k) / den_k, the share of a chain in the estimate
 * NaN where no chain holds a sample. */
int gs_brs_grad_info(int* block_rows /* HOST */, int* model_tile /* HOST */, int* column_tile /* HOST */);
int gs_brs_grad_work_bytes(int nchains, int n, int K, int Ju, long long* bytes /* HOST */);
int gs_brs_grad(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                const double* mref, void* work, long long work_bytes, double* num, void* stream);
int gs_brs_grad_finish(const double* num, const void* state, int C, int K, int Ju, double* xbar, double* chain_w,
                       void* stream);

/* The curvature of the bank's likelihood in the tables (gs_brh.hip):
 *   d^2 loglike_k / dY_ka dY_kb = Cov_w(x_a, x_b)
 *     = sum_ci w_cik (x_cia - xbar_ka)(x_cib - xbar_kb) / sum_ci w_cik,
 * the likelihood-weighted covariance of the bank's scale columns under theory k
 * (engine.br_likelihood_hess carries it to the Hessian in D^th).
 * gs_brs_hess, a third pass over bank rows [0, n) after gs_brs_grad_finish: mref
 * [K] as gs_brs_grad takes it, center [K][Ju] (DEVICE; the caller's xbar of the
 * complete -- possibly gathered -- bank), num2 [nchains][K][Jp][Jp] (DEVICE,
 * output):
 *   num2[c][k][a][b] = sum_i exp(t_cik - mref_k) u_cia u_cib,  u_cia = fl(x_cia - center_ka),
 * t recomputed with the bits of gs_brs_eval, the sum over the rows an MFMA
 * contraction of w u against u.  The moments are centred before they are
 * multiplied: raw second moments minus xbar xbar^T would cancel by the square of
 * the scales' relative spread.  Each symmetric pair is computed once and written
 * twice: num2[c][k] is bit-symmetric.  Rows whose r is NaN and rows >= n are never
 * touched, whatever their X holds; padding rows and columns >= Ju are written as
 * 0; n = 0 zeroes num2.  work: a DEVICE buffer of gs_brs_hess_work_bytes(nchains,
 * n, K, Ju) bytes -- one [K][Jp][Jp] tile per chain and block of block_rows rows,
 * 8 nchains ceil(n / block_rows) K Jp^2 bytes -- whose blocks are added in block
 * order from 0.0; the call fails when that exceeds 64 GiB (the pass is sized for
 * a few models: K = 1 ... 16).  gs_brs_hess_info: block_rows, the model tile (a
 * workgroup recomputes t once for that many models) and the column tile (a
 * workgroup owns one pair of column tiles a <= b).  For given (n, Ju, mref_k,
 * center_k) the tile num2[c][k] is bit-identical whatever K, the other models and
 * the other chains are.
 * gs_brs_hess_finish over the C chains of num2 [C][K][Jp][Jp] and a state in the
 * layout of gs_brl_bytes (both possibly all-gathered along the chain axis), in
 * chain order, every step one rounded operation, den_k as gs_brs_grad_finish
 * forms it:
 *   cov [K][Ju][Ju] = (sum_c num2[c][k][a][b]) / den_k
 * NaN where no chain holds a sample. */
int gs_brs_hess_info(int* block_rows /* HOST */, int* model_tile /* HOST */, int* column_tile /* HOST */);
int gs_brs_hess_work_bytes(int nchains, int n, int K, int Ju, long long* bytes /* HOST */);
int gs_brs_hess(const double* X, const double* r, int nchains, int cap, int n, int Ju, int K, const double* Y,
                const double* mref, const double* center, void* work, long long work_bytes, double* num2,
                void* stream);
int gs_brs_hess_finish(const double* num2, const void* state, int C, int K, int Ju, double* cov, void* stream);

/* ---- Gaussianised Blackwell-Rao likelihood (gs_gbr.hip) -------------------------
 * Rudjord et al. 2009: each inverse-Gamma column of the bank is mapped through its
 * own Blackwell-Rao marginal to a standard normal x_j(D_j) and a Gaussian is
 * fitted to the transformed draws.  All buffers DEVICE, fp64 unless noted.
 * gs_gbr_append packs the D_l trace ring (the layout and the slot rule of the
 * scale ring of gs_brs_append) into Dl [nchains][cap][Jp] at the used columns cols
 * [Ju], rows row0 ... row0 + nsteps - 1: row i of Dl belongs to row i of X and r.
 * The fit's Jg columns: gcol [Jg] (int32, positions in [0, Ju)), alpha [Jg], half
 * [Jg] (beta = half X: 0.5 for TT and EE of a TEB block, else 1), and a grid of G
 * nodes, 8 <= G <= 256, uniform in log D: lD_g = glo_j + g gh_j.  Nodes 1 and G - 2
 * bound the usable interval; nodes 0 and G - 1 lie outside it.
 * gs_gbr_marginals: per chain the online log-sum-exp (m, S) [nchains][Jg][G] of
 * log IG(D_g; alpha_j, beta_cij) over rows [0, n) in row order, and cnt [nchains]
 * (int64), the rows whose r is not NaN; a chain's partial depends on its rows
 * alone.  gs_gbr_marginals_finish merges C chains (possibly all-gathered) in
 * chain order into logp [Jg][G].
 * gs_gbr_tables: the cumulative trapezoid in log D from both sides, mass [Jg], and
 * the tables tx [Jg][G][2] = (x, dx/du) and tp [Jg][G][2] = (logp, dlogp/du), u
 * the node coordinate.
 * gs_gbr_moments: per chain S1 [nchains][Jg] = sum_i x_i and S2 [nchains][Jg][Jg]
 * = sum_i x_i x_i^T over the rows whose r is not NaN, x_ij the cubic Hermite of
 * log Dl_ij through tx, evaluated into LDS and contracted on the fp64 matrix
 * cores (upper-triangular tile pairs, rows ascending; S2 exactly symmetric).
 * work: gs_gbr_moments_work_bytes(nchains, n, Jg) bytes, one [Jq][Jq] + [Jq] tile
 * per chain and row block, the blocks added in block order from 0.0;
 * gs_gbr_info: the row blocks (at most 32) and their rows, a function of (n, Jg)
 * alone, and the column tile.  For given (n, Jg, tables) a chain's sums are
 * bit-identical whatever the other chains are.
 * gs_gbr_eval: x [K][Jg], logp [K][Jg] and outside [K][Jg] (int32: 1 where D is
 * off the usable interval; x = logp = 0 there) of theory [K][nspec][maxbins] at
 * the entries tcol [Jg] (int32), the Hermite code of the fit.
 * gs_gbr.hip documents the layout and the order of every operation. */
int gs_gbr_info(int n, int Jg, int* nblk /* HOST */, int* block_rows /* HOST */, int* column_tile /* HOST */);
int gs_gbr_append(double* Dl, int nchains, int cap, int Ju, int nspec, int maxbins, const int* cols,
                  const double* trace, int capacity, uint32_t first_iteration, int nsteps, int row0, void* stream);
int gs_gbr_marginals(const double* X, const double* r, int nchains, int cap, int n, int Ju, int Jg, const int* gcol,
                     const double* alpha, const double* half, const double* glo, const double* gh, int G, double* m,
                     double* S, long long* cnt, void* stream);
int gs_gbr_marginals_finish(const double* m, const double* S, const long long* cnt, int C, int Jg, int G,
                            const double* alpha, const double* glo, const double* gh, double* logp, void* stream);
int gs_gbr_tables(const double* logp, int Jg, int G, const double* glo, const double* gh, double* tx, double* tp,
                  double* mass, void* stream);
int gs_gbr_moments_work_bytes(int nchains, int n, int Jg, long long* bytes /* HOST */);
int gs_gbr_moments(const double* Dl, const double* r, int nchains, int cap, int n, int Ju, int Jg, const int* gcol,
                   const double* tx, const double* glo, const double* gh, int G, void* work, long long work_bytes,
                   double* S1, double* S2, void* stream);
int gs_gbr_eval(const double* theory, int K, int nspec, int maxbins, int Jg, const int* tcol, const double* tx,
                const double* tp, const double* glo, const double* gh, int G, double* x, double* logp, int* outside,
                void* stream);

/* The bank's likelihood of theory spectra that live on the device (gs_brt.hip):
 * engine.br_likelihood_tables and engine.br_likelihood_grad as kernels, so that
 * theory -> loglike (-> gradient) runs without a host round trip.  D [K][nspec]
 * [maxbins] (DEVICE) the theories; cols, kind [Ju] the bank's tables; per used
 * column j (DEVICE, they do not depend on a theory):
 *   part [2][Ju]  kind 2 (a block's TT column): the positions of its EE and TE columns
 *   cons [2][Ju]  n_b / 2, and the theory-free part of the column's cst term
 *                 (kind 1: -lgamma(alpha); kind 2: -nu log 2 - logGamma_2(nu / 2))
 *   inv [nspec * maxbins]  the position j of an entry of D, -1 for an unused one
 * gs_brt_tables writes Y [K][Ju] (the layout gs_brs_eval reads) with the bits of
 * engine.br_likelihood_tables, cst [K] (the terms added in column order from 0.0
 * by one thread) and bad [K] (int32): 1 where the host would raise -- a used value
 * not finite, a variance <= 0, a TEB block with TT EE - TE^2 <= 0; such a model's
 * Y row and cst are NaN, so its loglike is NaN.
 * gs_brt_mref: mref [K] = max_c m_c over S_c > 0 of a state in the layout of
 * gs_brl_bytes (0 where no chain holds a sample), the reference gs_brs_grad takes.
 * gs_brt_chain carries xbar [K][Ju] of gs_brs_grad_finish to grad [K][nspec]
 * [maxbins] = d loglike_k / d D with the bits of engine.br_likelihood_grad: exactly
 * 0.0 on the unused entries, NaN on the used entries of a bad model.  mean (or
 * NULL): [K][nspec][maxbins], xbar scattered to its entries, NaN elsewhere. */
int gs_brt_tables(const double* D, int K, int nspec, int maxbins, int Ju, const int* cols, const int* kind,
                  const int* part, const double* cons, double* Y, double* cst, int* bad, void* stream);
int gs_brt_mref(const void* state, int C, int K, double* mref, void* stream);
int gs_brt_chain(const double* D, const double* xbar, const int* bad, int K, int nspec, int maxbins, int Ju,
                 const int* cols, const int* kind, const int* part, const double* cons, const int* inv, double* grad,
                 double* mean, void* stream);

/* device-side timing of the dominant kernel: with enable = 1 every later CR-sweep
 * launch is bracketed by hipEvents on its stream (also while the stream is
 * captured into a hipGraph: external event-record nodes, timed at each replay);
 * enable = 2 / 3 pause / resume (launches in between are not bracketed);
 * enable = 0 returns the summed duration and the number of launches timed */
int gs_sweep_timing(gs_plan* plan, int enable, double* total_ms, int* count);

/* ---- HEALPix RING spherical-harmonic transforms (gs_sht.hip) ------------
 * Replace healpy's hp.alm2map / hp.map2alm as called by the masked CR
 * variants: CenteredGibbs.py:204,298,505,513,698,717,751,773,791,812,
 * NonCenteredGibbs.py:155,350, utils.adjoint_synthesis_hp utils.py:79-111.
 * ncomp: 1 = T (spin 0), 2 = (E,B) <-> (Q,U) (spin 2), 3 = (T,E,B) <-> (T,Q,U).
 * alm layout: GS_ALM_REAL (real m-major, (L+1)^2 doubles per component,
 * utils.py:49-76) or GS_ALM_COMPLEX (healpy order, (L+1)(L+2)/2 complex
 * interleaved per component).  maps: [ncomp][12 nside^2] RING order.
 * map2alm = (4 pi / Npix) x adjoint of alm2map (healpy, uniform weights);
 * niter adds healpy's Jacobi refinements a += map2alm(m - alm2map(a)).
 * One SHT plan serves one stream at a time (it owns the ring-phase workspace). */
#define GS_ALM_REAL 0
#define GS_ALM_COMPLEX 1
typedef struct gs_sht gs_sht;
int gs_sht_create(int nside, int lmax, gs_sht** out);
int gs_sht_destroy(gs_sht* sht);
int gs_sht_info(const gs_sht* sht, int* nside, int* lmax, long long* npix, long long* device_bytes);
int gs_sht_alm2map(gs_sht* sht, int ncomp, int layout, const double* alm, double* maps, void* stream);
int gs_sht_map2alm(gs_sht* sht, int ncomp, int layout, const double* maps, double* alm, int niter, void* stream);
/* Fused forms of the masked CR's transform pairs (real layout, iter 0):
 *   alm2map_beamed   = hp.alm2map(almxfl(alm, b_l))       (CenteredGibbs.py:698-699,752-753)
 *   map2alm_weighted = hp.map2alm(weights * maps, iter=0) (CenteredGibbs.py:298-299,510-513)
 * bit-identical to a separate per-l / per-pixel multiply followed by the plain
 * transform (the product is rounded once, on the transform's input load). */
int gs_sht_alm2map_beamed(gs_sht* sht, int ncomp, const double* alm_real, const double* bl, double* maps, void* stream);
int gs_sht_map2alm_weighted(gs_sht* sht, int ncomp, const double* maps, const double* weights, double* alm_real,
                            void* stream);
/* Batches of maps (one per chain; the reference runs its chains as separate
 * SLURM tasks, job-script.sh:6-8, each calling hp.alm2map / hp.map2alm):
 * alm [nmap][ncomp][n], maps [nmap][ncomp][Npix] contiguous; one launch per
 * stage serves every map (small maps fill the GPU), and map b of a batch is
 * bit-identical to the same map transformed alone.  bl (nullable, real layout):
 * per-l beam on the synthesis input (hp.alm2map(almxfl(alm, b_l))); weights
 * (nullable; real layout, niter 0): [ncomp][Npix] shared by the batch, the
 * analysis of weights * maps (hp.map2alm(N^-1 m)).  gs_sht_reserve sizes the
 * plan's per-map workspace for nmap maps ahead of a graph capture (a larger
 * batch inside a capture is an error). */
int gs_sht_reserve(gs_sht* sht, int nmap, void* stream);
/* on = 1: the plan's Legendre stage runs on the fp64 matrix cores from a
 * plan-time table of lambda (8 B per (l, m, ring pair): 0.54 GB at N_side 256,
 * 4.3 GB at N_side 512; budget GS_SHT_MFMA_MAX_GB, default 16; the spin-2 F1 /
 * F2 are formed in the kernels) -- a dense contraction per m whose inner
 * dimension every map of a batch shares.
 * Every transform of the plan then uses it (a map's result does not depend on
 * the batch size); on = 0 returns to the on-the-fly recurrence kernels.
 * Small maps only (plans without split-ring FFTs).  _info: state, table bytes. */
int gs_sht_set_mfma(gs_sht* sht, int on);
int gs_sht_mfma_info(const gs_sht* sht, int* on, long long* table_bytes);
int gs_sht_alm2map_batch(gs_sht* sht, int nmap, int ncomp, int layout, const double* alm, const double* bl,
                         double* maps, void* stream);
/* the masked PCG operator's transform pair in one call: alm_out =
 * map2alm(weights x alm2map(bl x alm_in)), real layout, niter 0 (the
 * reference's hp.map2alm(N^-1 hp.alm2map(almxfl(s, b_l))) of its PCG fwd_op,
 * CenteredGibbs.py:448-491).  On the matrix-core table path with the
 * multi-component ring stage the per-ring synthesis, weighting and analysis run
 * in one workgroup and the maps never reach HBM (bit-identical to the two
 * calls); otherwise the two calls through maps_scratch ([nmap][ncomp][Npix],
 * may be NULL only on the fused path). */
int gs_sht_apply_weighted_batch(gs_sht* sht, int nmap, int ncomp, const double* alm_in, const double* bl,
                                const double* weights, double* maps_scratch, double* alm_out, void* stream);
int gs_sht_map2alm_batch(gs_sht* sht, int nmap, int ncomp, int layout, const double* maps, const double* weights,
                         double* alm, int niter, void* stream);

/* ---- masked (pixel-domain) constrained realisation (gs_masked.hip) -------
 * Replaces PolarizedCenteredConstrainedRealization's masked samplers:
 *   GS_MCR_AUX        sample_gibbs_change_variable  CenteredGibbs.py:676-729
 *   GS_MCR_OVERRELAX  overrelaxation_sampler        CenteredGibbs.py:733-825
 *   GS_MCR_MALA       sample_mala                   CenteredGibbs.py:560-603 (EB only)
 *   GS_MCR_AUX_MALA   the ula composition of sample CenteredGibbs.py:832-836
 * A context runs a batch of B = desc.nchains chains (0 -> 1) on one data set:
 * the reference's independent chains (its SLURM array, job-script.sh:6-8) as
 * one batch whose transforms are batched SHTs; `chain` arguments are the global
 * id of the batch's first chain (chain b has id chain + b), and chain b's
 * results equal a one-chain context's for id chain + b bit for bit when both
 * contexts run the same Legendre stage (desc.sht_mode resolved to the same
 * path: "auto" = 0 picks the matrix-core tables from 4 chains on small maps and
 * the recurrence otherwise, so pass 1 or 2 explicitly to compare a batch with a
 * one-chain run; the two paths agree to ~1e-12 relative).
 * maps / inv_noise (create): DEVICE [3][Npix] rows T, Q, U (inv_noise
 * mask-multiplied, CenteredGibbs.py:266-274; the T row is read only for
 * nfields = 3), shared by the batch.  Every per-chain argument is [B][...]
 * contiguous: dl DEVICE unbinned D_l [B][nspec][L+1]; s [B][F][(L+1)^2] real
 * layout, updated in place; v [B][F][Npix] the auxiliary map (needed across
 * calls only by GS_MCR_OVERRELAX; may be NULL).  Replay variates (NULL =
 * native Philox streams), per chain: zv [B][n][F][Npix] pixel normals, zs
 * [B][n][F][NR] slot normals in the reference's draw order (AUX: per inner
 * iteration v then s; OVERRELAX: initial v, then per iteration s, v, s; MALA:
 * zm [B][F][NR], um [B]).  accept (device int32 [B], optional): 1 for the
 * auxiliary samplers, the MALA decisions otherwise; log_ratio (device double
 * [B], optional). */
#define GS_MCR_AUX 0
#define GS_MCR_OVERRELAX 1
#define GS_MCR_MALA 2
#define GS_MCR_AUX_MALA 3
typedef struct gs_masked gs_masked;
typedef struct gs_masked_desc {
    int lmax, nside, nfields;      /* nfields 1 (T), 2 (E,B) or 3 (T,E,B)         */
    const double* bl;              /* HOST [L+1] beam                             */
    int n_gibbs;                   /* inner iterations (CenteredGibbs.py:250)     */
    double alpha;                  /* over-relaxation, -0.995 (CenteredGibbs.py:244) */
    double tau;                    /* MALA step, 0.02 (CenteredGibbs.py:294)      */
    double noise_pol0;             /* noise_pol[0] of the MALA sigma (571-572)    */
    double mu_eps;                 /* mu = max(N^-1) + mu_eps; 0 -> 1e-14 (pol,   */
                                   /* CenteredGibbs.py:276); TT: 1e-7              */
                                   /* (ConstrainedRealization.py:44)              */
    int adj_iter;                  /* map2alm iterations of the data term          */
                                   /* b A^T N^-1 d and of the aux s|v analysis:    */
                                   /* 0 (pol: iter=0) or 3 (TT: adjoint_synthesis_hp */
                                   /* and healpy's default, CenteredGibbs.py:208)  */
    int nchains;                   /* chains of the batch (0 or 1: one chain)     */
    int sht_mode;                  /* Legendre stage: 0 auto (the matrix-core    */
                                   /* table path for batches of >= 4 chains when  */
                                   /* its table fits), 1 on-the-fly recurrence,   */
                                   /* 2 the matrix-core table path                */
} gs_masked_desc;
int gs_masked_create(const gs_masked_desc* desc, const double* maps, const double* inv_noise, gs_masked** out);
int gs_masked_destroy(gs_masked* ctx);
/* Diagnostic (no reference counterpart): the context's N^-1 ring-pair classes,
 * computed once at create -- counts[0] pairs without weight, counts[1] pairs
 * with a ring whose weights vary, counts[2] pairs whose weights are one number
 * per ring (isotropic noise on rings the mask leaves whole: the PCG operator's
 * ring stage and the f2 Gram pass take their constant-ring forms there). */
int gs_masked_ring_classes(const gs_masked* ctx, int* counts /* HOST [3] */);
int gs_masked_info(const gs_masked* ctx, double* mu3 /* HOST [3] */, double* second_part_grad /* DEVICE [F][NR] */);
int gs_masked_nchains(const gs_masked* ctx);   /* chains of the batch; -1 for a null context */
int gs_masked_sht_tables(const gs_masked* ctx); /* 1: the matrix-core table path is on, 0: off */
int gs_masked_gradient(gs_masked* ctx, const double* dl, const double* s, double* grad, double* pix, void* stream);
/* f4: temperature full-sky CR from pixel data (nfields = 1 context):
 * centered CenteredConstrainedRealization.sample_no_mask (CenteredGibbs.py:108-132)
 * or non-centered NonCenteredConstrainedRealization.sample_no_mask
 * (NonCenteredGibbs.py:22-38); zv [Npix] / zs [NR] replay normals (reference
 * order: zs then zv) or NULL for the native streams; s_out [NR]. */
int gs_masked_tt_fullsky(gs_masked* ctx, int noncentered, const double* dl, const double* zv, const double* zs,
                         uint64_t seed, uint32_t iteration, int chain, double* s_out, void* stream);
int gs_masked_cr(gs_masked* ctx, int kind, const double* dl, double* s, double* v, const double* zv, const double* zs,
                 const double* zm, const double* um, uint64_t seed, uint32_t iteration, int chain, int32_t* accept,
                 double* log_ratio, void* stream);
/* f1: the PCG CR (sample_mask, CenteredGibbs.py:448-491).  rhs = b A^T N^-1 d
 * + b adjoint_synthesis_hp(sqrt(N^-1) z_pix) (map2alm iter=3, utils.py:79-111)
 * + C^-1/2 z_slot; solve (C^+ + b A^T N^-1 A b) x = rhs by preconditioned CG
 * (per-l preconditioner (C^+ + b^2 nbar/w)^-1) until |r| <= tol |rhs|.
 * zv [F][Npix], zs [F][NR]: replay normals (reference order z_Q, z_U, z_E,
 * z_B) or NULL for the native streams.  The CG recurrence's scalars stay on
 * the device; the host launches batches of iterations sized from the residual's
 * decay and synchronises once per batch (no host round trip per iteration).
 * Batched contexts solve every chain's system at once (per-chain scalars and
 * convergence; rhs / x [B][F][NR]); iters / rel_residual are HOST [B].
 * gs_masked_pcg_info: host synchronisations of the last solve; _info2 also the
 * CG iterations launched (>= every chain's count: a converged chain's kernels
 * return at once, its transforms still run until the batch's last chain
 * converges). */
int gs_masked_pcg_rhs(gs_masked* ctx, const double* dl, const double* zv, const double* zs, uint64_t seed,
                      uint32_t iteration, int chain, double* rhs, void* stream);
int gs_masked_pcg_solve(gs_masked* ctx, const double* dl, const double* rhs, double* x, int x_is_guess, double tol,
                        int maxiter, int* iters, double* rel_residual, void* stream);
int gs_masked_pcg_info(const gs_masked* ctx, int* host_syncs);
int gs_masked_pcg_info2(const gs_masked* ctx, int* host_syncs, int* launched);
/* The last solve's transformed chain-iterations: the sum over its launched CG
 * iterations of the chains still unconverged at the last state read (the batch
 * transforms only those; launched x B without that compaction). */
int gs_masked_pcg_work(const gs_masked* ctx, long long* chain_iterations /* HOST */);
/* out = Q x, the PCG system operator (C^+ + b A^T N^-1 A b) applied to x
 * (qcinv opfilt_pp fwd_op, CenteredGibbs.py:631,655). */
int gs_masked_pcg_apply(gs_masked* ctx, const double* dl, const double* x, double* out, void* stream);
/* RJPO accept step (sample_mask_rj, CenteredGibbs.py:606-674): x is the PCG
 * solution of Q x = rhs started from -s (gs_masked_pcg_solve with x = -s as the
 * guess, :645-650); log_ratio = -sum (rhs - Q x) . (s - x) (:657-669), accept
 * when log u < log_ratio (:670) and then s <- x.  um: device [1] replay uniform
 * or NULL for the native stream (Philox(0, 0, TAG_RJ_U, iteration)); accept,
 * log_ratio: device int32 [1] / double [1] or NULL.  Nothing is read back. */
int gs_masked_rj_accept(gs_masked* ctx, const double* dl, const double* rhs, const double* x, double* s,
                        const double* um, uint64_t seed, uint32_t iteration, int chain, int32_t* accept,
                        double* log_ratio, void* stream);
/* f2: pixel-domain non-centered likelihood (NonCenteredGibbs.py:333-355):
 * lik = -1/2 sum_pix N^-1 (d - A b C^1/2(D) s_nc)^2 (device double).
 * gs_masked_center: out = C^1/2 in (dir = +1) or C^+1/2 in (dir = -1) per slot
 * (EB sqrt(var) / sqrt(inv_var), NonCenteredGibbs.py:236-237; TEB chol(C)). */
int gs_masked_center(gs_masked* ctx, const double* dl, int dir, const double* in, double* out, void* stream);
int gs_masked_nc_loglik(gs_masked* ctx, const double* dl, const double* s_nc, double* lik, void* stream);
/* f2: one Metropolis sweep of the pixel-domain non-centered likelihood over K
 * blocks (PolarizationNonCenteredClsSampler.sample / NonCenteredClsSampler.sample
 * with all_sph=False, NonCenteredGibbs.py:401-445 with :333-355), decided on
 * the device in block order without a host round trip and without one SHT per
 * block: the per-block map changes come from one shared-recurrence block
 * synthesis and one weighted Gram pass.  F = 1 (T) or 2 (EB).
 * blk [F][lmax+1]: block (0..K-1, decision order: spectra in MH order) of each
 * (field, l), -1 outside every block; blk_lmax [K]: largest l of each block
 * (-1: empty); blk_field [K]; blk_bins [2K]: bin range [lo, hi) of each block;
 * s_nc [F][(lmax+1)^2]; dl_cur / dl_prop [F][lmax+1]: unbinned current and
 * proposed D_l; logr / prop_binned / binned [F][maxbins] (binned in/out:
 * accepted blocks take the proposal's bins); u_acc [K * n_iter] accept
 * uniforms in decision order; accept_out [K * n_iter]. */
int gs_masked_pixel_mh(gs_masked* ctx, int K, int n_iter, int maxbins, const int* blk, const int* blk_lmax,
                       const int* blk_field, const int* blk_bins, const double* s_nc, const double* dl_cur,
                       const double* dl_prop, const double* logr, const double* u_acc, const double* prop_binned,
                       double* binned, int32_t* accept_out, void* stream);

/* Gaussian sky draw for synthetic data (the synalm + smoothalm half of
 * healpy.synfast, main_polarization.py:38): alm[f] = beam[f][l] * (C_l^1/2 z)[f]
 * per real slot.  cl [nspec][lmax+1] is C_l (not D_l): nfields 1: TT;
 * 2: EE, BB; 3: TT, EE, BB, TE (TEB uses the Cholesky factor of the (T, E)
 * block).  beam [nfields][lmax+1]; z [nfields][(lmax+1)^2] unit normals
 * supplied by the caller; alm [nfields][(lmax+1)^2].  Device pointers. */
int gs_synalm(int lmax, int nfields, const double* cl, const double* beam, const double* z, double* alm,
              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIBBS_CAPI_H */
