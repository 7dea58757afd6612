"""Device-resident batched Gibbs engine over the HIP C-ABI.

One ``GibbsPlan`` holds a model (beam, noise, bins, MH blocks) on one GPU and
runs ``nchains`` independent chains in lock-step; every per-iteration array
stays in HBM (torch tensors used purely as device buffers) and each
iteration is a handful of asynchronous kernel launches on the current HIP
stream (capturable in a hipGraph).

RNG modes
  * ``native``: counter-based Philox streams on the device, keyed by
    (seed, global chain id) -- results do not depend on the GPU count.
  * ``replay``: numpy's legacy global RNG drawn on the host in the
    reference's exact order and uploaded, so a run reproduces
    the reference's numbers for the same ``np.random.seed``.
"""
import ctypes
import math

import numpy as np
import torch
from scipy.stats import invgamma

from . import _capi as C

SPECTRA = {1: ("TT",), 2: ("EE", "BB"), 3: ("TT", "EE", "BB", "TE")}
# defaults of the Gaussianised Blackwell-Rao likelihood (interpolation error): nodes per column, span
GBR_POINTS = 128
GBR_SPAN = (0.5, 8.0)
FIELDS = {1: ("TT",), 2: ("EE", "BB"), 3: ("TT", "EE", "BB")}
MH_ORDER = {1: ("TT",), 2: ("EE", "BB"), 3: ("EE", "BB", "TT", "TE")}


def _require_gpu():
    if not torch.cuda.is_available():
        raise C.GibbsHipError("gibbssampler_amd needs a ROCm GPU (MI355X); no CPU fallback")


class GibbsPlan:
    def __init__(self, lmax, nside, nfields, nchains, bl, noise_var, bins, blocks=None,
                 proposal_variances=None, chain0=0, quirks=C.GS_QUIRK_ASIS_RECENTRE_CENTERED,
                 n_iter_metropolis=1, device=None):
        _require_gpu()
        self.lib = C.load()
        self.L = int(lmax)
        self.nside = int(nside)
        self.Npix = 12 * self.nside ** 2
        self.F = int(nfields)
        self.nchains = int(nchains)
        self.chain0 = int(chain0)
        self.spectra = SPECTRA[self.F]
        self.fields = FIELDS[self.F]
        self.n_iter_metropolis = int(n_iter_metropolis)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self.bins = {s: np.asarray(bins[s], dtype=np.int32) for s in self.spectra}
        self.blocks = None if blocks is None else {s: np.asarray(blocks[s], dtype=np.int32) for s in self.spectra}
        self.proposal_variances = None if proposal_variances is None else \
            {s: np.asarray(proposal_variances[s], dtype=np.float64) for s in self.spectra}
        self.bl = np.ascontiguousarray(bl, dtype=np.float64)
        self.noise_var = np.ascontiguousarray(noise_var, dtype=np.float64)
        if self.bl.shape != (self.L + 1,):
            raise ValueError("bl must have lmax+1 entries")
        desc = C.GsModelDesc()
        desc.lmax, desc.nside, desc.nfields, desc.nchains = self.L, self.nside, self.F, self.nchains
        desc.chain0, desc.quirks, desc.n_iter_metropolis = self.chain0, int(quirks), self.n_iter_metropolis
        keep = [self.bl, self.noise_var]
        desc.bl = self.bl.ctypes.data_as(C.c_double_p)
        desc.noise_var = self.noise_var.ctypes.data_as(C.c_double_p)
        for k, s in enumerate(self.spectra):
            b = np.ascontiguousarray(self.bins[s], dtype=np.int32)
            keep.append(b)
            desc.bins[k] = b.ctypes.data_as(C.c_int_p)
            desc.nbin_edges[k] = len(b)
            if self.blocks is not None:
                bk = np.ascontiguousarray(self.blocks[s], dtype=np.int32)
                keep.append(bk)
                desc.blocks[k] = bk.ctypes.data_as(C.c_int_p)
                desc.nblock_edges[k] = len(bk)
            if self.proposal_variances is not None:
                pv = np.ascontiguousarray(self.proposal_variances[s], dtype=np.float64)
                if len(pv) != len(b) - 1 - 2:
                    raise ValueError(f"proposal_variances[{s}] must have nbins-2 entries")
                keep.append(pv)
                desc.prop_var[k] = pv.ctypes.data_as(C.c_double_p)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            C.check(self.lib.gs_plan_create(ctypes.byref(desc), ctypes.byref(h)), "gs_plan_create")
        self._h = h
        mb, ns, nacc, nsp = (ctypes.c_int() for _ in range(4))
        C.check(self.lib.gs_plan_info(h, ctypes.byref(mb), ctypes.byref(ns), ctypes.byref(nacc), ctypes.byref(nsp)))
        self.maxbins, self.nstat, self.nacc, self.nspec = mb.value, ns.value, nacc.value, nsp.value
        self.NR = (self.L + 1) ** 2
        nt, rpt = ctypes.c_int(), ctypes.c_int()
        C.check(self.lib.gs_plan_sweep_info(h, ctypes.byref(nt), ctypes.byref(rpt)))
        self.ntask, self.rows_per_task = nt.value, rpt.value
        # packed diagonal workgroups of the no-map throughput sweep, absorbed one-entry groups (per chain)
        C.check(self.lib.gs_plan_sweep_pack_info(h, ctypes.byref(nt), ctypes.byref(rpt)))
        self.sweep_packed, self.sweep_absorbed = nt.value, rpt.value
        # the NC MH decides in the register form (one multipole per thread) rather than the LDS-phase kernel
        C.check(self.lib.gs_plan_mh_info(h, ctypes.byref(nt)))
        self.mh_reg_form = bool(nt.value)
        # host-side replay helpers (data independent)
        ell = np.arange(self.L + 1, dtype=np.float64)
        expo = (2 * ell + 1) / 2
        self._alphas = {}
        for s in self.spectra:
            b = self.bins[s]
            a = np.array([np.sum(expo[b[i]:b[i + 1]]) - 1 for i in range(len(b) - 1)])
            a[0] = 1
            self._alphas[s] = a
        self.adapting = False
        self.scale_trace = None         # the attached scale ring (cls_scale_trace)
        self._acc_layout = []
        if self.blocks is not None:
            for s in MH_ORDER[self.F]:
                self._acc_layout.append((s, (len(self.blocks[s]) - 1) * self.n_iter_metropolis))

    def __del__(self):
        try:
            C.park(dict(self.__dict__))       # inside a capture: tensors freed after it
            if getattr(self, "_h", None) is not None and self.lib is not None:
                C.release(self.lib.gs_plan_destroy, self._h)
                self._h = None
        except Exception:
            pass

    # ---- buffers ---------------------------------------------------------------
    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def dl_tensor(self, dls):
        """dict spec -> binned D (same for all chains) or list of dicts -> [nchains, nspec, maxbins]."""
        out = np.zeros((self.nchains, self.nspec, self.maxbins))
        per_chain = dls if isinstance(dls, (list, tuple)) else [dls] * self.nchains
        for c, d in enumerate(per_chain):
            for k, s in enumerate(self.spectra):
                v = np.asarray(d[s], dtype=np.float64)
                out[c, k, :len(v)] = v
        return torch.from_numpy(out).to(self.device)

    def dl_dicts(self, t):
        a = t.detach().cpu().numpy()
        return [{s: a[c, k, :len(self.bins[s]) - 1].copy() for k, s in enumerate(self.spectra)}
                for c in range(self.nchains)]

    def data_tensor(self, d_alm):
        """dict field -> real-layout alm (or array [F, NR]) -> device [F, NR]."""
        if isinstance(d_alm, dict):
            arr = np.stack([np.asarray(d_alm[f], dtype=np.float64) for f in self.fields])
        else:
            arr = np.asarray(d_alm, dtype=np.float64).reshape(self.F, self.NR)
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)

    def split_accept(self, acc):
        a = acc.detach().cpu().numpy()
        out, off = {}, 0
        for s, n in self._acc_layout:
            out[s] = a[:, off:off + n]
            off += n
        return out

    # ---- replay variates (numpy legacy global RNG, reference order) -------------
    def replay_cr_normals(self):
        z = np.stack([np.stack([np.random.normal(size=self.NR) for _ in range(self.F)])
                      for _ in range(self.nchains)])
        return torch.from_numpy(z).to(self.device)

    def replay_invgamma(self):
        v = np.zeros((self.nchains, self.nspec, self.maxbins))
        for c in range(self.nchains):
            for k, s in enumerate(self.spectra):
                x = invgamma.rvs(a=self._alphas[s])
                v[c, k, :len(x)] = x
        return torch.from_numpy(v).to(self.device)

    def replay_mh_uniforms(self):
        up = np.zeros((self.nchains, self.nspec, self.maxbins))
        ua = np.zeros((self.nchains, max(self.nacc, 1)))
        for c in range(self.nchains):
            for s in MH_ORDER[self.F]:
                k = self.spectra.index(s)
                nb = len(self.bins[s]) - 1
                up[c, k, 2:nb] = np.random.uniform(size=nb - 2)
            ua[c, :self.nacc] = np.random.uniform(size=self.nacc)
        return torch.from_numpy(up).to(self.device), torch.from_numpy(ua).to(self.device)

    # ---- stages ---------------------------------------------------------------
    def _s(self):
        return C.stream_ptr()

    def block_params(self, mode, dl, out=None):
        out = self.zeros(self.nchains, self.L + 1, C.GS_NPARAM) if out is None else out
        C.check(self.lib.gs_block_params(self._h, mode, C.ptr(dl), C.ptr(out), self._s()), "gs_block_params")
        return out

    def cr_sweep(self, d, params, z=None, seed=0, iteration=0, substep=0, s_out=None, store=True, stats=None):
        if store and s_out is None:
            s_out = self.zeros(self.nchains, self.F, self.NR)
        stats = self.zeros(self.nchains, self.nstat, self.L + 1) if stats is None else stats
        C.check(self.lib.gs_cr_sweep(self._h, C.ptr(d), C.ptr(params), C.ptr(z), int(seed), int(iteration),
                                     int(substep), C.ptr(s_out) if store else None, C.ptr(stats), self._s()),
                "gs_cr_sweep")
        return s_out, stats

    def sweep_stats(self, d, s, stats=None):
        """per-l statistics of a given map s [nchains, F, NR] (no draw)."""
        stats = self.zeros(self.nchains, self.nstat, self.L + 1) if stats is None else stats
        C.check(self.lib.gs_sweep_stats(self._h, C.ptr(d), C.ptr(s), C.ptr(stats), self._s()), "gs_sweep_stats")
        return stats

    def cls_draw(self, stats, variates=None, seed=0, iteration=0, out=None):
        out = self.zeros(self.nchains, self.nspec, self.maxbins) if out is None else out
        C.check(self.lib.gs_cls_draw(self._h, C.ptr(stats), C.ptr(variates), int(seed), int(iteration),
                                     C.ptr(out), self._s()), "gs_cls_draw")
        return out

    def cls_scale_trace(self, scales, capacity=1):
        """Attach the scale trace ring [capacity, nchains, nspec, maxbins] every
        C_l draw of the plan records its conditional's scale in (slot
        (iteration - 1) % capacity), or detach it (scales None).  Refused while
        the current stream is being captured (gs_cls_scale_trace)."""
        if scales is not None and scales.numel() < int(capacity) * self.nchains * self.nspec * self.maxbins:
            raise ValueError("cls_scale_trace: the ring is smaller than capacity rows")
        C.check(self.lib.gs_cls_scale_trace(self._h, C.ptr(scales), int(capacity), self._s()), "gs_cls_scale_trace")
        self.scale_trace = scales

    def mh_propose(self, dl, u_prop=None, seed=0, iteration=0, with_uniforms=False):
        """(prop, logr[, native accept uniforms]) of the NC MH step (no decisions)."""
        prop = self.zeros(self.nchains, self.nspec, self.maxbins)
        logr = self.zeros(self.nchains, self.nspec, self.maxbins)
        ua = self.zeros(self.nchains, max(self.nacc, 1)) if with_uniforms else None
        C.check(self.lib.gs_mh_propose(self._h, C.ptr(dl), C.ptr(u_prop), int(seed), int(iteration), C.ptr(prop),
                                       C.ptr(logr), C.ptr(ua), self._s()), "gs_mh_propose")
        return prop, logr, ua

    def nc_mh(self, stats, dl, u_prop=None, u_acc=None, seed=0, iteration=0, accept=None):
        accept = self.zeros(self.nchains, max(self.nacc, 1), dtype=torch.int32) if accept is None else accept
        C.check(self.lib.gs_nc_mh(self._h, C.ptr(stats), C.ptr(dl), C.ptr(u_prop), C.ptr(u_acc), int(seed),
                                  int(iteration), C.ptr(accept), self._s()), "gs_nc_mh")
        return accept

    # ---- warm-up adaptation of the proposal scales (gs_mh_adapt_*) -------------------
    @property
    def nblocks_mh(self):
        """MH blocks per chain, in the order of the accept flags."""
        return self.nacc // self.n_iter_metropolis

    def mh_block_layout(self):
        """[(spectrum, first block, blocks)] of the [nchains, nblocks_mh] scale arrays."""
        out, off = [], 0
        for s, n in self._acc_layout:
            out.append((s, off, n // self.n_iter_metropolis))
            off += n // self.n_iter_metropolis
        return out

    def mh_adapt_enable(self, target=0.25, kappa=0.6):
        """Per-chain proposal table and Robbins-Monro state (log-scale 0, count 0);
        every proposal-drawing launch reads the per-chain table from here on."""
        C.check(self.lib.gs_mh_adapt_enable(self._h, float(target), float(kappa)), "gs_mh_adapt_enable")
        self.adapting = True

    def mh_adapt(self, accept):
        """One adaptation step from a step's accept flags [nchains, nacc] (capturable)."""
        C.check(self.lib.gs_mh_adapt(self._h, C.ptr(accept), self._s()), "gs_mh_adapt")

    def mh_scale_get(self):
        """(log-scale fp64, count int32), device tensors [nchains, nblocks_mh]."""
        lam = self.zeros(self.nchains, self.nblocks_mh)
        cnt = self.zeros(self.nchains, self.nblocks_mh, dtype=torch.int32)
        C.check(self.lib.gs_mh_scale_get(self._h, C.ptr(lam), C.ptr(cnt), self._s()), "gs_mh_scale_get")
        return lam, cnt

    def mh_scale_set(self, log_scale, count=None):
        """Set the log-scales (and counts) and rebuild the per-chain table from them."""
        lam = torch.as_tensor(log_scale, dtype=torch.float64).to(self.device).contiguous()
        if tuple(lam.shape) != (self.nchains, self.nblocks_mh):
            raise ValueError("log_scale must be [nchains, nblocks_mh]")
        cnt = None
        if count is not None:
            cnt = torch.as_tensor(count).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(cnt.shape) != (self.nchains, self.nblocks_mh):
                raise ValueError("count must be [nchains, nblocks_mh]")
        C.check(self.lib.gs_mh_scale_set(self._h, C.ptr(lam), C.ptr(cnt), self._s()), "gs_mh_scale_set")

    def mh_proposal_sd(self):
        """The proposal standard deviations the draws read, [nchains, nspec, maxbins]."""
        sd = self.zeros(self.nchains, self.nspec, self.maxbins)
        C.check(self.lib.gs_mh_proposal_sd(self._h, C.ptr(sd), self._s()), "gs_mh_proposal_sd")
        return sd

    def stats_to_noncentered(self, dl, stats):
        C.check(self.lib.gs_stats_to_noncentered(self._h, C.ptr(dl), C.ptr(stats), self._s()), "gs_stats_to_nc")
        return stats

    def recentre(self, dl_new, s, dl_old=None):
        C.check(self.lib.gs_recentre(self._h, C.ptr(dl_new), C.ptr(dl_old), C.ptr(s), self._s()), "gs_recentre")
        return s

    # ---- fused iterations -----------------------------------------------------------
    def step_centered(self, d, dl, s_out, z=None, igvar=None, seed=0, iteration=0):
        C.check(self.lib.gs_step_centered(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), C.ptr(z), C.ptr(igvar),
                                          int(seed), int(iteration), self._s()), "gs_step_centered")

    def step_centered_fused(self, d, dl, s_out, seed=0, iteration=0, trace=None, capacity=0):
        """gs_step_centered with the trace record and device-counter advance in the
        C_l-draw launch (graph-captured native steps)."""
        C.check(self.lib.gs_step_centered_fused(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), int(seed), int(iteration),
                                                C.ptr(trace), int(capacity), self._s()), "gs_step_centered_fused")

    def step_asis_fused(self, d, dl, s_out, seed=0, iteration=0, accept=None, dl_tmp=None, recentre=False,
                        trace=None, capacity=0):
        """gs_step_asis with the trace record and device-counter advance in the MH launch."""
        C.check(self.lib.gs_step_asis_fused(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), int(seed), int(iteration),
                                            C.ptr(accept), C.ptr(dl_tmp), 1 if recentre else 0, C.ptr(trace),
                                            int(capacity), self._s()), "gs_step_asis_fused")

    def step_noncentered(self, d, dl, s_out, z=None, u_prop=None, u_acc=None, seed=0, iteration=0, accept=None):
        C.check(self.lib.gs_step_noncentered(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), C.ptr(z), C.ptr(u_prop),
                                             C.ptr(u_acc), int(seed), int(iteration), C.ptr(accept), self._s()),
                "gs_step_noncentered")

    def data_moments(self, d):
        """Per-l moments of the data tensor d for the raw-moment NC statistics
        (gs_data_moments): once per tensor, and again after changing d in place."""
        C.check(self.lib.gs_data_moments(self._h, C.ptr(d), self._s()), "gs_data_moments")

    # the three stages of step_noncentered (for pipelined schedules)
    def nc_prologue(self, dl, u_prop=None, seed=0, iteration=0):
        C.check(self.lib.gs_nc_prologue(self._h, C.ptr(dl), C.ptr(u_prop), int(seed), int(iteration), self._s()),
                "gs_nc_prologue")

    def nc_sweep(self, d, dl, s_out, z=None, seed=0, iteration=0, finish=True):
        C.check(self.lib.gs_nc_sweep(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), C.ptr(z), int(seed), int(iteration),
                                     int(bool(finish)), self._s()), "gs_nc_sweep")

    def nc_finish(self):
        C.check(self.lib.gs_nc_finish(self._h, self._s()), "gs_nc_finish")

    def nc_stats(self, out=None):
        """The statistic rows [nchains, nstat, L+1] of the last NC sweep (what the MH reads)."""
        out = self.zeros(self.nchains, self.nstat, self.L + 1) if out is None else out
        C.check(self.lib.gs_nc_stats(self._h, C.ptr(out), self._s()), "gs_nc_stats")
        return out

    def nc_decide(self, dl, u_acc=None, seed=0, iteration=0, accept=None):
        C.check(self.lib.gs_nc_decide(self._h, C.ptr(dl), C.ptr(u_acc), int(seed), int(iteration), C.ptr(accept),
                                      self._s()), "gs_nc_decide")

    def nc_decide_fused(self, dl, seed=0, iteration=0, accept=None, trace=None, capacity=0):
        C.check(self.lib.gs_nc_decide_fused(self._h, C.ptr(dl), int(seed), int(iteration), C.ptr(accept),
                                            C.ptr(trace), int(capacity), self._s()), "gs_nc_decide_fused")

    def nc_pipe_prepare(self):
        """Whether multi-step native NC graphs pipeline (gs_nc_pipe_prepare; option
        GS_NC_PIPE); the first call allocates: not inside a capture."""
        on = ctypes.c_int()
        C.check(self.lib.gs_nc_pipe_prepare(self._h, ctypes.byref(on)), "gs_nc_pipe_prepare")
        return bool(on.value)

    def nc_steps(self, d, dl, nsteps, seed=0, accept=None, accept_stride=0, trace=None, capacity=0, adapt=False,
                 time_every=0):
        """nsteps pipelined native NC steps without a stored map (gs_nc_steps):
        step i writes its flags to accept[i * accept_stride ...] (elements)."""
        C.check(self.lib.gs_nc_steps(self._h, C.ptr(d), C.ptr(dl), int(seed), int(nsteps), C.ptr(accept),
                                     int(accept_stride), C.ptr(trace), int(capacity), 1 if adapt else 0,
                                     int(time_every), self._s()), "gs_nc_steps")

    def step_asis(self, d, dl, s_out, z=None, igvar=None, u_prop=None, u_acc=None, seed=0, iteration=0,
                  accept=None, dl_tmp=None, recentre=False):
        C.check(self.lib.gs_step_asis(self._h, C.ptr(d), C.ptr(dl), C.ptr(s_out), C.ptr(z), C.ptr(igvar),
                                      C.ptr(u_prop), C.ptr(u_acc), int(seed), int(iteration), C.ptr(accept),
                                      C.ptr(dl_tmp), 1 if recentre else 0, self._s()), "gs_step_asis")

    # ---- hipGraph support ---------------------------------------------------------------
    def iteration_counter(self, enable, start=1):
        C.check(self.lib.gs_iteration_counter(self._h, 1 if enable else 0, int(start)), "gs_iteration_counter")

    def graph_step(self, offset, advance):
        """Offset of the next captured step from the device base, and the advance
        its last launch applies (gs_graph_step)."""
        C.check(self.lib.gs_graph_step(self._h, int(offset), int(advance)), "gs_graph_step")

    def advance_iteration(self):
        C.check(self.lib.gs_advance_iteration(self._h, self._s()), "gs_advance_iteration")

    def record_trace(self, dl, trace, capacity, iteration=0):
        C.check(self.lib.gs_record_trace(self._h, C.ptr(dl), C.ptr(trace), int(capacity), int(iteration), self._s()),
                "gs_record_trace")

    # ---- timing of the dominant kernel (hipEvents on the launch stream) ---------------
    def sweep_timing(self, enable):
        """True: start bracketing every CR sweep with hipEvents; False: stop and
        return (total ms, launches); "pause" / "resume" keep the launches timed so far."""
        mode = {True: 1, False: 0, "pause": 2, "resume": 3}[enable]
        tot = ctypes.c_double()
        n = ctypes.c_int()
        C.check(self.lib.gs_sweep_timing(self._h, mode, ctypes.byref(tot), ctypes.byref(n)))
        return tot.value, n.value


class SummaryState:
    """Streaming posterior summary of D_l chains over the gs_summary_* C-ABI
    (gs_summary.hip documents the state layout and the formulas): a flat fp64
    device tensor ``data`` = 8 header doubles (int64 sample count first), the
    per-series fields [6 + 3 max_lag, nchains, nspec * maxbins] and the int64
    accept counts [nchains, nacc].  Plan-independent: any trace tensor
    [capacity, nchains, nspec, maxbins] can be summarised."""
    HDR = 8
    POOLED = ("mean", "var", "min", "max", "ess", "ess_truncated", "rhat")

    def __init__(self, nchains, nspec, maxbins, nacc, max_lag, device=None, data=None):
        _require_gpu()
        self.lib = C.load()
        self.nchains, self.nspec, self.maxbins = int(nchains), int(nspec), int(maxbins)
        self.nacc, self.max_lag = int(nacc), int(max_lag)
        nb = ctypes.c_longlong()
        C.check(self.lib.gs_summary_bytes(*self._dims(), ctypes.byref(nb)), "gs_summary_bytes")
        self.nfields = 6 + 3 * self.max_lag
        self.ns = self.nchains * self.nspec * self.maxbins
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        if data is None:
            self.data = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
        else:
            self.data = torch.as_tensor(data, dtype=torch.float64).to(dev).contiguous().clone()
            if self.data.numel() * 8 != nb.value:
                raise ValueError("summary state: size does not match its dimensions")

    def _dims(self):
        return self.nchains, self.nspec, self.maxbins, self.nacc, self.max_lag

    def reset(self):
        C.check(self.lib.gs_summary_reset(C.ptr(self.data), *self._dims(), C.stream_ptr()), "gs_summary_reset")

    def update(self, trace, capacity, first_iteration, nsteps, accept=None, accept_stride=0):
        """Add iterations first_iteration .. first_iteration + nsteps - 1 from the
        trace ring (iteration it in slot (it - 1) % capacity) and, with accept
        (int32, step i at accept + i * accept_stride elements), their flags."""
        if trace.numel() < int(capacity) * self.ns:
            raise ValueError("summary update: the trace is smaller than capacity rows")
        if accept is not None and accept.numel() < (int(nsteps) - 1) * int(accept_stride) + self.nchains * self.nacc:
            raise ValueError("summary update: the accept trace is smaller than nsteps steps")
        C.check(self.lib.gs_summary_update(C.ptr(self.data), *self._dims(), C.ptr(trace), int(capacity),
                                           int(first_iteration), int(nsteps), C.ptr(accept), int(accept_stride),
                                           C.stream_ptr()), "gs_summary_update")

    @property
    def n(self):
        """Samples summarised (reads the device count: synchronises)."""
        return int(self.data[:1].view(torch.int64).item())

    def fields(self):
        """The per-series fields as a view [6 + 3 max_lag, nchains, nspec * maxbins]."""
        return self.data[self.HDR:self.HDR + self.nfields * self.ns].view(self.nfields, self.nchains, -1)

    def accept_counts(self):
        """int64 [nchains, nacc] (a view of the state)."""
        return self.data[self.HDR + self.nfields * self.ns:].view(torch.int64).view(self.nchains, self.nacc)

    def finish(self, gather=None):
        """Run the finish; device tensors: the POOLED names [nspec, maxbins],
        chain_mean / chain_var [C, nspec, maxbins], acf [max_lag + 1, nspec,
        maxbins], gamma [C, max_lag + 1, nspec, maxbins] and n.  gather
        (ShardContext.gather): the fields are all-gathered along the chain axis
        first and the finish runs over every rank's chains."""
        data, nch = self.data, self.nchains
        if gather is not None:
            body = gather(self.fields().contiguous(), dim=1)
            nch = int(body.shape[1])
            data = torch.cat([self.data[:self.HDR], body.reshape(-1)])
        K, dev = self.max_lag, self.data.device
        z = lambda *shape: torch.zeros(*shape, self.nspec, self.maxbins, dtype=torch.float64, device=dev)
        pooled, cm, cv, acf, gamma = z(7), z(nch), z(nch), z(K + 1), z(nch, K + 1)
        C.check(self.lib.gs_summary_finish(C.ptr(data), nch, self.nspec, self.maxbins, K, C.ptr(pooled), C.ptr(cm),
                                           C.ptr(cv), C.ptr(acf), C.ptr(gamma), C.stream_ptr()), "gs_summary_finish")
        out = {k: pooled[i] for i, k in enumerate(self.POOLED)}
        out.update(chain_mean=cm, chain_var=cv, acf=acf, gamma=gamma, n=self.n)
        return out


class SkymapMoments:
    """Streaming posterior mean and variance of a batch of fp64 series over the
    gs_smap_* C-ABI (gs_smap.hip documents the state layout and the formulas):
    a flat fp64 device tensor ``data`` = 8 header doubles (int64 samples per
    chain first), the Welford mean [nchains, n] and M2 [nchains, n].
    Plan-independent: n = F (L+1)^2 for a real-layout a_lm, ncomp N_pix for a
    map.  The sample count is kept on the host as well, so an update reads
    nothing back; ``data=`` restores a state saved from ``data`` (or rebuilt
    from ``fields()`` behind its header)."""
    HDR = 8

    def __init__(self, nchains, n, device=None, data=None):
        _require_gpu()
        self.lib = C.load()
        self.nchains, self.len = int(nchains), int(n)
        nb = ctypes.c_longlong()
        C.check(self.lib.gs_smap_bytes(self.nchains, self.len, ctypes.byref(nb)), "gs_smap_bytes")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        if data is None:
            self.data = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
            self._count = 0
        else:
            self.data = torch.as_tensor(data, dtype=torch.float64).to(dev).contiguous().clone()
            if self.data.numel() * 8 != nb.value:
                raise ValueError("skymap moments: size does not match its dimensions")
            self._count = int(self.data[:1].view(torch.int64).item())

    def reset(self):
        C.check(self.lib.gs_smap_reset(C.ptr(self.data), self.nchains, self.len, C.stream_ptr()), "gs_smap_reset")
        self._count = 0

    def update(self, x, count_after=None):
        """Add one sample of every chain: x [nchains, ...] (float64, contiguous
        over the trailing axes, n elements per chain; the chain stride is read
        from the tensor).  count_after: this sample's number (default: one more
        than the last update's; pass it when the call is captured in a graph)."""
        if x.dtype != torch.float64 or not x.is_cuda:
            raise ValueError("skymap moments: x must be a float64 device tensor")
        if x.dim() < 1 or x.shape[0] != self.nchains or x.numel() != self.nchains * self.len:
            raise ValueError(f"skymap moments: x must be [{self.nchains}, ...] with {self.len} elements per chain")
        if not x[0].is_contiguous():
            raise ValueError("skymap moments: x must be contiguous over its trailing axes")
        k = self._count + 1 if count_after is None else int(count_after)
        C.check(self.lib.gs_smap_update(C.ptr(self.data), self.nchains, self.len, ctypes.c_void_p(x.data_ptr()),
                                        int(x.stride(0)) if self.nchains > 1 else self.len, k, C.stream_ptr()),
                "gs_smap_update")
        self._count = k

    @property
    def n(self):
        """Samples per chain (reads the device count: synchronises)."""
        return int(self.data[:1].view(torch.int64).item())

    def fields(self):
        """The per-chain fields as a view [2, nchains, n]: mean, M2."""
        return self.data[self.HDR:].view(2, self.nchains, self.len)

    def finish(self, gather=None):
        """Device tensors: mean, var, rhat [n], chain_mean [C, n] and n (samples
        per chain).  gather (ShardContext.gather): the fields are all-gathered
        along the chain axis first and the finish runs over every rank's chains."""
        data, nch = self.data, self.nchains
        if gather is not None:
            body = gather(self.fields().contiguous(), dim=1)
            nch = int(body.shape[1])
            data = torch.cat([self.data[:self.HDR], body.reshape(-1)])
        z = lambda *shape: torch.zeros(*shape, self.len, dtype=torch.float64, device=self.data.device)
        mean, var, cm, rhat = z(), z(), z(nch), z()
        C.check(self.lib.gs_smap_finish(C.ptr(data), nch, self.len, C.ptr(mean), C.ptr(var), C.ptr(cm), C.ptr(rhat),
                                        C.stream_ptr()), "gs_smap_finish")
        return dict(mean=mean, var=var, chain_mean=cm, rhat=rhat, n=self.n)

    def power(self, L, F, gather=None, finished=None):
        """Real-layout a_lm states (n = F (L+1)^2): device tensors power_of_mean
        and mean_power [F, L+1] (gs_smap_power) of the pooled mean and variance
        (``finished``: a finish() result to reuse)."""
        if int(F) * (int(L) + 1) ** 2 != self.len:
            raise ValueError("skymap moments: power needs n = F (L+1)^2")
        fin = self.finish(gather) if finished is None else finished
        pom = torch.zeros(int(F), int(L) + 1, dtype=torch.float64, device=self.data.device)
        mp = torch.zeros_like(pom)
        C.check(self.lib.gs_smap_power(int(L), int(F), C.ptr(fin["mean"]), C.ptr(fin["var"]), C.ptr(pom), C.ptr(mp),
                                       C.stream_ptr()), "gs_smap_power")
        return dict(power_of_mean=pom, mean_power=mp)


class WienerPosterior:
    """Rao-Blackwellised posterior sky map of a full-sky run over the gs_wf_*
    C-ABI (gs_wf.hip documents the state layout and the formulas): from the
    D_l trace ring alone, through the closed-form centered operator M_l(D_l),
    Sigma_l(D_l) of the plan's tables -- the beam bl [L+1], the bins {spectrum:
    edges} and the noise weights N_pix / (4 pi noise_var_f).  ``data`` is a flat
    fp64 device tensor: 8 header doubles (int64 samples per chain first), then
    the planes [NFLD, nchains, L+1].  The sample count is kept on the host as
    well, so an update reads nothing back; ``data=`` restores a saved state."""
    HDR = 8

    def __init__(self, nfields, lmax, nchains, bl, bins, noise_weights, maxbins=None, device=None, data=None):
        _require_gpu()
        self.lib = C.load()
        self.F, self.L, self.nchains = int(nfields), int(lmax), int(nchains)
        self.spectra = SPECTRA[self.F]
        self.nspec, self.nop = len(self.spectra), 5 if self.F == 3 else self.F
        self.nfld = 20 if self.F == 3 else 4 * self.F
        self.NR = (self.L + 1) ** 2
        nb = ctypes.c_longlong()
        C.check(self.lib.gs_wf_bytes(self.F, self.nchains, self.L, ctypes.byref(nb)), "gs_wf_bytes")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        bl = np.ascontiguousarray(bl, dtype=np.float64)
        if bl.shape != (self.L + 1,):
            raise ValueError("wiener posterior: bl must have lmax + 1 entries")
        kap = [float(v) for v in np.atleast_1d(noise_weights)]
        if len(kap) != self.F or not all(v > 0 for v in kap):
            raise ValueError("wiener posterior: one positive noise weight per field is needed")
        self.kappa = kap + [0.0] * (3 - self.F)
        e2b = np.full((self.nspec, self.L + 1), -1, dtype=np.int32)
        nbins = []
        for k, s in enumerate(self.spectra):
            e = np.asarray(bins[s], dtype=np.int64)
            if len(e) < 2 or e[0] < 0 or np.any(np.diff(e) < 0) or e[-1] > self.L + 1:
                raise ValueError(f"wiener posterior: invalid bin edges for {s}")
            nbins.append(len(e) - 1)
            for i in range(len(e) - 1):
                e2b[k, e[i]:e[i + 1]] = i
        self.maxbins = max(nbins) if maxbins is None else int(maxbins)
        if self.maxbins < max(nbins):
            raise ValueError("wiener posterior: maxbins is smaller than a spectrum's bin count")
        self.bl = torch.from_numpy(bl).to(dev)
        self.ell2bin = torch.from_numpy(e2b).to(dev)
        self.moments = None
        if data is None:
            self.data = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
            self._count = 0
        else:
            self.data = torch.as_tensor(data, dtype=torch.float64).to(dev).contiguous().clone()
            if self.data.numel() * 8 != nb.value:
                raise ValueError("wiener posterior: size does not match its dimensions")
            self._count = int(self.data[:1].view(torch.int64).item())

    @classmethod
    def from_plan(cls, plan, nchains=None, data=None):
        """The tables of a GibbsPlan (its beam, bins and noise weights)."""
        kap = plan.Npix / (4.0 * math.pi * plan.noise_var[:plan.F])
        return cls(plan.F, plan.L, plan.nchains if nchains is None else nchains, plan.bl, plan.bins, kap,
                   maxbins=plan.maxbins, device=plan.device, data=data)

    def reset(self):
        C.check(self.lib.gs_wf_reset(C.ptr(self.data), self.F, self.nchains, self.L, C.stream_ptr()), "gs_wf_reset")
        self._count = 0

    def _check_d(self, d_alm):
        if d_alm.dtype != torch.float64 or not d_alm.is_cuda or d_alm.numel() != self.F * self.NR:
            raise ValueError(f"wiener posterior: d_alm must be a float64 device tensor [{self.F}, (L+1)^2]")

    def data_moments(self, d_alm):
        """S_l = sum_m d_lm d_lm^T [nspec, L+1] of the data tensor (gs_wf_moments),
        kept for update() and power(): once per data tensor."""
        self._check_d(d_alm)
        mom = torch.zeros(self.nspec, self.L + 1, dtype=torch.float64, device=self.data.device)
        C.check(self.lib.gs_wf_moments(self.L, self.F, C.ptr(d_alm), C.ptr(mom), C.stream_ptr()), "gs_wf_moments")
        self.moments = mom
        return mom

    def update(self, trace, capacity, first_iteration, nsteps, count_after=None):
        """Add iterations first_iteration .. first_iteration + nsteps - 1 from the
        trace ring [capacity, nchains, nspec, maxbins] (iteration it in slot
        (it - 1) % capacity).  count_after: the samples per chain after this
        call (default: nsteps more than after the last one)."""
        if self.moments is None:
            raise RuntimeError("wiener posterior: data_moments(d_alm) first")
        if trace.dtype != torch.float64 or not trace.is_cuda:
            raise ValueError("wiener posterior: the trace must be a float64 device tensor")
        if trace.numel() < int(capacity) * self.nchains * self.nspec * self.maxbins:
            raise ValueError("wiener posterior update: the trace is smaller than capacity rows")
        k = self._count + int(nsteps) if count_after is None else int(count_after)
        C.check(self.lib.gs_wf_update(C.ptr(self.data), self.F, self.nchains, self.L, self.maxbins, C.ptr(self.bl),
                                      C.ptr(self.ell2bin), *self.kappa, C.ptr(self.moments), C.ptr(trace),
                                      int(capacity), int(first_iteration), int(nsteps), k, C.stream_ptr()),
                "gs_wf_update")
        if int(nsteps) > 0:
            self._count = k

    @property
    def n(self):
        """Samples per chain (reads the device count: synchronises)."""
        return int(self.data[:1].view(torch.int64).item())

    def fields(self):
        """The per-(chain, l) planes as a view [NFLD, nchains, L+1]."""
        return self.data[self.HDR:].view(self.nfld, self.nchains, self.L + 1)

    def _gathered(self, gather):
        if gather is None:
            return self.data, self.nchains
        body = gather(self.fields().contiguous(), dim=1)
        return torch.cat([self.data[:self.HDR], body.reshape(-1)]), int(body.shape[1])

    def finish(self, d_alm, gather=None):
        """Device tensors: alm_mean, alm_var, alm_rhat [F, (L+1)^2], chain_alm_mean
        [C, F, (L+1)^2] and n (samples per chain).  gather (ShardContext.gather):
        the planes are all-gathered along the chain axis first and the finish
        runs over every rank's chains."""
        self._check_d(d_alm)
        data, nch = self._gathered(gather)
        z = lambda *shape: torch.zeros(*shape, self.F, self.NR, dtype=torch.float64, device=self.data.device)
        mean, var, cm, rhat = z(), z(), z(nch), z()
        C.check(self.lib.gs_wf_finish(C.ptr(data), self.F, nch, self.L, C.ptr(d_alm), C.ptr(mean), C.ptr(var),
                                      C.ptr(cm), C.ptr(rhat), C.stream_ptr()), "gs_wf_finish")
        return dict(alm_mean=mean, alm_var=var, chain_alm_mean=cm, alm_rhat=rhat, n=self.n)

    def power(self, gather=None):
        """Device tensors power_of_mean, mean_power [nspec, L+1] (TE included for
        F = 3) and op_mean [nop, L+1], the posterior-averaged operator."""
        if self.moments is None:
            raise RuntimeError("wiener posterior: data_moments(d_alm) first")
        data, nch = self._gathered(gather)
        z = lambda n: torch.zeros(n, self.L + 1, dtype=torch.float64, device=self.data.device)
        pom, mp, op = z(self.nspec), z(self.nspec), z(self.nop)
        C.check(self.lib.gs_wf_power(C.ptr(data), self.F, nch, self.L, C.ptr(self.moments), C.ptr(pom), C.ptr(mp),
                                     C.ptr(op), C.stream_ptr()), "gs_wf_power")
        return dict(power_of_mean=pom, mean_power=mp, op_mean=op)


def br_shapes(nfields, bins, maxbins=None):
    """The shape table of the centered conditionals (gs_br.hip): (alpha [nspec,
    maxbins], half_mask).  With n_b = l1^2 - l0^2: alpha = n_b / 2 - 1 for the
    inverse-Gamma spectra; n_b / 2 - 2 for TT and EE of the TEB block, whose
    recorded scale Psi_ii is twice the conditional's (half_mask bits); NaN for
    TE, bins 0 and 1 and the bins past a spectrum's count."""
    spectra = SPECTRA[int(nfields)]
    nb = [len(bins[s]) - 1 for s in spectra]
    maxbins = max(nb) if maxbins is None else int(maxbins)
    alpha = np.full((len(spectra), maxbins), np.nan)
    half = 0
    for k, s in enumerate(spectra):
        if nfields == 3 and s == "TE":
            continue
        b = np.asarray(bins[s], dtype=np.float64)
        n_b = b[1:] ** 2 - b[:-1] ** 2
        iw = nfields == 3 and s in ("TT", "EE")
        alpha[k, :nb[k]] = 0.5 * n_b - (2.0 if iw else 1.0)
        alpha[k, :2] = np.nan
        half |= (1 << k) if iw else 0
    return alpha, half


class BlackwellRaoState:
    """Streaming Blackwell-Rao marginal posteriors over the gs_br_* C-ABI
    (gs_br.hip documents the state and the order of operations): a flat fp64
    device tensor ``data`` = 8 header doubles (int64 iteration count first), the
    planes m and S [2, nchains, nspec * maxbins * G] and the int64 counts of
    skipped rows [nchains, nspec].  grid [nspec, maxbins, G] and alpha [nspec,
    maxbins] (br_shapes) are kept on the device.  Plan-independent: any scale
    ring [capacity, nchains, nspec, maxbins] can be accumulated."""
    HDR = 8

    def __init__(self, nchains, grid, alpha, half_mask=0, device=None, data=None):
        _require_gpu()
        self.lib = C.load()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.grid = torch.as_tensor(grid, dtype=torch.float64).to(dev).contiguous()
        self.alpha = torch.as_tensor(alpha, dtype=torch.float64).to(dev).contiguous()
        if self.grid.dim() != 3 or tuple(self.alpha.shape) != tuple(self.grid.shape[:2]):
            raise ValueError("Blackwell-Rao state: grid must be [nspec, maxbins, G] and alpha [nspec, maxbins]")
        self.nchains, self.half_mask = int(nchains), int(half_mask)
        self.nspec, self.maxbins, self.G = (int(v) for v in self.grid.shape)
        nb = ctypes.c_longlong()
        C.check(self.lib.gs_br_bytes(*self._dims(), ctypes.byref(nb)), "gs_br_bytes")
        self.ne = self.nchains * self.nspec * self.maxbins * self.G
        if data is None:
            self.data = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
        else:
            self.data = torch.as_tensor(data, dtype=torch.float64).to(dev).contiguous().clone()
            if self.data.numel() * 8 != nb.value:
                raise ValueError("Blackwell-Rao state: size does not match its dimensions")

    def _dims(self):
        return self.nchains, self.nspec, self.maxbins, self.G

    def reset(self):
        C.check(self.lib.gs_br_reset(C.ptr(self.data), *self._dims(), C.stream_ptr()), "gs_br_reset")

    def update(self, scales, capacity, first_iteration, nsteps):
        """Add iterations first_iteration .. first_iteration + nsteps - 1 from the
        scale ring (iteration it in slot (it - 1) % capacity)."""
        if scales.numel() < int(capacity) * self.nchains * self.nspec * self.maxbins:
            raise ValueError("Blackwell-Rao update: the scale ring is smaller than capacity rows")
        C.check(self.lib.gs_br_update(C.ptr(self.data), *self._dims(), C.ptr(self.grid), C.ptr(self.alpha),
                                      self.half_mask, C.ptr(scales), int(capacity), int(first_iteration), int(nsteps),
                                      C.stream_ptr()), "gs_br_update")

    @property
    def n(self):
        """Iterations added (reads the device count: synchronises)."""
        return int(self.data[:1].view(torch.int64).item())

    def fields(self):
        """The planes m and S as a view [2, nchains, nspec * maxbins * G]."""
        return self.data[self.HDR:self.HDR + 2 * self.ne].view(2, self.nchains, -1)

    def bad(self):
        """int64 [nchains, nspec]: rows skipped for a scale <= 0 or not finite (a view)."""
        return self.data[self.HDR + 2 * self.ne:].view(torch.int64).view(self.nchains, self.nspec)

    def finish(self, gather=None):
        """Device tensors logpdf [nspec, maxbins, G] and mass [nspec, maxbins], and
        n.  gather (ShardContext.gather): the planes are all-gathered along the
        chain axis first and the finish runs over every rank's chains."""
        data, nch = self.data, self.nchains
        if gather is not None:
            body = gather(self.fields().contiguous(), dim=1)
            nch = int(body.shape[1])
            data = torch.cat([self.data[:self.HDR], body.reshape(-1)])
        dev = self.data.device
        logpdf = torch.zeros(self.nspec, self.maxbins, self.G, dtype=torch.float64, device=dev)
        mass = torch.zeros(self.nspec, self.maxbins, dtype=torch.float64, device=dev)
        C.check(self.lib.gs_br_finish(C.ptr(data), nch, self.nspec, self.maxbins, self.G, C.ptr(self.grid),
                                      C.ptr(self.alpha), C.ptr(logpdf), C.ptr(mass), C.stream_ptr()), "gs_br_finish")
        return {"logpdf": logpdf, "mass": mass, "n": self.n}


def br_likelihood_mask(nfields, bins, maxbins=None, lrange=None):
    """The bins a Blackwell-Rao likelihood can use, bool [nspec, maxbins]: every
    drawn bin (b >= 2, below the spectrum's count), with lrange = (lmin, lmax)
    only those wholly inside it (l0 >= lmin and l1 - 1 <= lmax)."""
    spectra = SPECTRA[int(nfields)]
    nb = [len(bins[s]) - 1 for s in spectra]
    maxbins = max(nb) if maxbins is None else int(maxbins)
    mask = np.zeros((len(spectra), maxbins), dtype=bool)
    for k, s in enumerate(spectra):
        b = np.asarray(bins[s], dtype=np.int64)
        ok = np.ones(nb[k], dtype=bool)
        if lrange is not None:
            ok = (b[:-1] >= lrange[0]) & (b[1:] - 1 <= lrange[1])
        mask[k, :nb[k]] = ok
        mask[k, :2] = False
    return mask


def br_likelihood_tables(nfields, bins, theory, mask):
    """The tables of the streaming Blackwell-Rao likelihood (gs_brl.hip), numpy
    fp64 on the host: theory [K, nspec, maxbins] (D^th per model; read on the
    used bins only), mask bool [nspec, maxbins] (the used bins; bins 0, 1 and
    those past a spectrum's count never count; the TEB block TT, EE, TE is
    used as a whole, by TT's row).  Returns {cols [Ju] int32 ascending, kind
    [Ju] int32, coef [Ju], Y [K, Ju], cst [K]}: with x the scale ring's row,
    log P(D^th_k | s) = sum_j coef_j log(arg_j) - sum_j x_j Y_kj + cst_k.
    With n_b = l1^2 - l0^2:
      inverse-Gamma bin (kind 1): coef = alpha = n_b / 2 - 1, Y = 1 / D,
        cst += -lgamma(alpha) - (alpha + 1) log D
      TEB block, inverse-Wishart(Psi, nu = n_b - 3), det = TT EE - TE^2:
        TT column (kind 2, arg = |Psi|): coef = nu / 2, Y = EE / (2 det)
        EE column (kind 0): Y = TT / (2 det);  TE column (kind 0): Y = -TE / det
        cst += -nu log 2 - logGamma_2(nu / 2) - (n_b / 2) log det,
        logGamma_2(x) = log(pi) / 2 + lgamma(x) + lgamma(x - 1 / 2)."""
    F = int(nfields)
    spectra = SPECTRA[F]
    theory = np.asarray(theory, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    if theory.ndim != 3 or theory.shape[1:] != mask.shape or mask.shape[0] != len(spectra):
        raise ValueError("br_likelihood_tables: theory must be [K, nspec, maxbins] and mask [nspec, maxbins]")
    K, nspec, maxbins = theory.shape
    used = mask & br_likelihood_mask(F, bins, maxbins)
    block = (0, 1, 3) if F == 3 else ()
    for k in block[1:]:
        used[k] = used[0]
    Ju = int(used.sum())
    cols = np.flatnonzero(used.reshape(-1)).astype(np.int32)
    kind = np.zeros(Ju, dtype=np.int32)
    coef = np.zeros(Ju)
    Y = np.zeros((K, Ju))
    cst = [[] for _ in range(K)]
    pos = {int(c): j for j, c in enumerate(cols)}
    with np.errstate(all="ignore"):
        for sp, s in enumerate(spectra):
            if sp in block[1:]:
                continue
            e = np.asarray(bins[s], dtype=np.float64)
            for b in np.flatnonzero(used[sp]):
                n_b = e[b + 1] ** 2 - e[b] ** 2
                j = pos[sp * maxbins + int(b)]
                if sp in block:
                    nu = n_b - 3.0
                    tt, ee, te = theory[:, 0, b], theory[:, 1, b], theory[:, 3, b]
                    det = tt * ee - te * te
                    kind[j], coef[j] = 2, 0.5 * nu
                    Y[:, j] = 0.5 * ee / det
                    Y[:, pos[maxbins + int(b)]] = 0.5 * tt / det
                    Y[:, pos[3 * maxbins + int(b)]] = -te / det
                    lg2 = 0.5 * math.log(math.pi) + math.lgamma(0.5 * nu) + math.lgamma(0.5 * nu - 0.5)
                    term = -nu * math.log(2.0) - lg2 - 0.5 * n_b * np.log(det)
                else:
                    alpha = 0.5 * n_b - 1.0
                    D = theory[:, sp, b]
                    kind[j], coef[j] = 1, alpha
                    Y[:, j] = 1.0 / D
                    term = -math.lgamma(alpha) - (alpha + 1.0) * np.log(D)
                for k in range(K):
                    cst[k].append(float(term[k]))
    return {"cols": cols, "kind": kind, "coef": coef, "Y": Y, "cst": np.array([math.fsum(v) for v in cst])}


def br_likelihood_grad(nfields, bins, theory, mask, xbar):
    """The gradient of the Blackwell-Rao log likelihood with respect to the
    theory spectra, numpy fp64 on the host: [K, nspec, maxbins], exactly 0 on
    the bins that are not used.  theory and mask as br_likelihood_tables takes
    them; xbar [K, Ju] is the likelihood-weighted mean of the used scale
    columns under each theory (columns in the order of the tables' cols), so
    that d loglike_k / d Y_kj = -xbar_kj and the rest is the chain rule through
    Y(D) and cst(D) of br_likelihood_tables.  With n_b = l1^2 - l0^2:
      inverse-Gamma bin: d / dD = xbar / D^2 - (alpha + 1) / D
      TEB block, Psi = [[xbar_TT, xbar_TE], [xbar_TE, xbar_EE]], D = [[TT, TE],
        [TE, EE]]:  G = D^-1 Psi D^-1 / 2 - (n_b / 2) D^-1,
        d / dTT = G_00, d / dEE = G_11, d / dTE = 2 G_01."""
    F = int(nfields)
    spectra = SPECTRA[F]
    theory = np.asarray(theory, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    if theory.ndim != 3 or mask.ndim != 2 or theory.shape[1:] != mask.shape or mask.shape[0] != len(spectra):
        raise ValueError("br_likelihood_grad: theory must be [K, nspec, maxbins] and mask [nspec, maxbins]")
    K, nspec, maxbins = theory.shape
    used = mask & br_likelihood_mask(F, bins, maxbins)
    block = (0, 1, 3) if F == 3 else ()
    for k in block[1:]:
        used[k] = used[0]
    cols = np.flatnonzero(used.reshape(-1))
    xbar = np.asarray(xbar, dtype=np.float64)
    if xbar.ndim != 2 or xbar.shape != (K, len(cols)):
        raise ValueError(f"br_likelihood_grad: xbar must be [K, Ju] = [{K}, {len(cols)}] (the mask's used columns)")
    pos = {int(c): j for j, c in enumerate(cols)}
    grad = np.zeros((K, nspec, maxbins))
    with np.errstate(all="ignore"):
        for sp, s in enumerate(spectra):
            if sp in block[1:]:
                continue
            e = np.asarray(bins[s], dtype=np.float64)
            for b in np.flatnonzero(used[sp]):
                n_b = e[b + 1] ** 2 - e[b] ** 2
                b = int(b)
                if sp in block:
                    tt, ee, te = theory[:, 0, b], theory[:, 1, b], theory[:, 3, b]
                    ptt, pee, pte = (xbar[:, pos[q * maxbins + b]] for q in (0, 1, 3))
                    det = tt * ee - te * te
                    i00, i11, i01 = ee / det, tt / det, -te / det          # D^-1
                    a00, a01 = i00 * ptt + i01 * pte, i00 * pte + i01 * pee  # D^-1 Psi
                    a10, a11 = i01 * ptt + i11 * pte, i01 * pte + i11 * pee
                    grad[:, 0, b] = 0.5 * (a00 * i00 + a01 * i01) - 0.5 * n_b * i00
                    grad[:, 1, b] = 0.5 * (a10 * i01 + a11 * i11) - 0.5 * n_b * i11
                    grad[:, 3, b] = (a00 * i01 + a01 * i11) - n_b * i01
                else:
                    D = theory[:, sp, b]
                    grad[:, sp, b] = xbar[:, pos[sp * maxbins + b]] / (D * D) - (0.5 * n_b) / D
    return grad


def _br_used(name, nfields, theory, mask, bins):
    """(theory [K, nspec, maxbins], used bool [nspec, maxbins], cols [Ju], block) as
    br_likelihood_tables reads them."""
    F = int(nfields)
    theory = np.asarray(theory, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    if theory.ndim != 3 or mask.ndim != 2 or theory.shape[1:] != mask.shape or mask.shape[0] != len(SPECTRA[F]):
        raise ValueError(f"{name}: theory must be [K, nspec, maxbins] and mask [nspec, maxbins]")
    used = mask & br_likelihood_mask(F, bins, theory.shape[2])
    block = (0, 1, 3) if F == 3 else ()
    for k in block[1:]:
        used[k] = used[0]
    return theory, used, np.flatnonzero(used.reshape(-1)), block


def br_likelihood_hess(nfields, bins, theory, mask, xbar, cov):
    """The Hessian of the Blackwell-Rao log likelihood with respect to the theory
    spectra, numpy fp64 on the host: H [K, Ju, Ju], parameter j the theory entry
    at the tables' cols[j] (spectrum * maxbins + bin).  theory, mask and xbar as
    br_likelihood_grad takes them; cov [K, Ju, Ju] is the likelihood-weighted
    covariance of the used scale columns under each theory, d^2 loglike_k / dY_ka
    dY_kb.  H = J^T cov J + L with J = dY / dD and L the Hessian of the single-
    sample log density with the scale held at xbar, both block diagonal (a bin's Y
    depends on that bin's D alone).  With n_b = l1^2 - l0^2:
      inverse-Gamma bin (Y = 1 / D): J = -1 / D^2, L = (n_b / 2) / D^2 - 2 xbar / D^3
      TEB block, D = [[TT, TE], [TE, EE]], Psi = [[xbar_TT, xbar_TE], [xbar_TE,
        xbar_EE]], over the basis E_TT, E_EE, E_TE (both off-diagonal entries 1),
        sum_j x_j Y_j = tr(Psi D^-1) / 2:
        J[j, U] = -tr(E_j D^-1 U D^-1) / 2
        L[U, V] = -tr((D^-1 U D^-1 V + D^-1 V D^-1 U) D^-1 Psi) / 2 + (n_b / 2) tr(D^-1 U D^-1 V)
    The upper triangle is computed and mirrored: H is exactly symmetric."""
    theory, used, cols, block = _br_used("br_likelihood_hess", nfields, theory, mask, bins)
    spectra = SPECTRA[int(nfields)]
    K, nspec, maxbins = theory.shape
    Ju = len(cols)
    xbar, cov = np.asarray(xbar, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    if xbar.shape != (K, Ju) or cov.shape != (K, Ju, Ju):
        raise ValueError(f"br_likelihood_hess: xbar must be [K, Ju] = [{K}, {Ju}] and cov [K, Ju, Ju] (the mask's used "
                         "columns)")
    pos = {int(c): j for j, c in enumerate(cols)}
    J = np.zeros((K, Ju, Ju))
    L = np.zeros((K, Ju, Ju))
    flat = theory.reshape(K, -1)
    ig, ig_nb, tri, tri_nb = [], [], [], []                     # parameter indices and n_b of the bins, by kind
    for sp, s in enumerate(spectra):
        if sp in block[1:]:
            continue
        e = np.asarray(bins[s], dtype=np.float64)
        for b in np.flatnonzero(used[sp]):
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if sp in block:
                tri.append([pos[q * maxbins + int(b)] for q in (0, 1, 3)])
                tri_nb.append(n_b)
            else:
                ig.append(pos[sp * maxbins + int(b)])
                ig_nb.append(n_b)
    with np.errstate(all="ignore"):
        if ig:
            j = np.array(ig)
            D = flat[:, cols[j]]
            J[:, j, j] = -1.0 / (D * D)
            L[:, j, j] = (0.5 * np.array(ig_nb)) / (D * D) - 2.0 * xbar[:, j] / (D * D * D)
        if tri:
            idx = np.array(tri)                                      # [nb, 3]: TT, EE, TE
            nb2 = 0.5 * np.array(tri_nb)
            basis = np.array([[[1.0, 0.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 1.0]], [[0.0, 1.0], [1.0, 0.0]]])
            tt, ee, te = (flat[:, cols[idx[:, q]]] for q in range(3))    # [K, nb]
            det = tt * ee - te * te
            Di = np.stack([np.stack([ee / det, -te / det], axis=-1), np.stack([-te / det, tt / det], axis=-1)], axis=-2)
            pt, pe, pc = (xbar[:, idx[:, q]] for q in range(3))
            Psi = np.stack([np.stack([pt, pc], axis=-1), np.stack([pc, pe], axis=-1)], axis=-2)   # [K, nb, 2, 2]
            WU = np.einsum("knab,ubc->knuac", Di, basis)                 # D^-1 U
            W = np.einsum("knuab,knbc->knuac", WU, Di)                   # D^-1 U D^-1
            P = np.einsum("knab,knbc->knac", Di, Psi)                    # D^-1 Psi
            Jb = -0.5 * np.einsum("uab,knvba->knuv", basis, W)           # [K, nb, j, U]
            UV = np.einsum("knuab,knvbc->knuvac", WU, WU)                # D^-1 U D^-1 V
            sym = UV + UV.transpose(0, 1, 3, 2, 4, 5)
            Lb = -0.5 * np.einsum("knuvab,knba->knuv", sym, P) + nb2[None, :, None, None] * np.einsum("knuvaa->knuv", UV)
            iu3 = np.triu_indices(3, 1)
            Lb[:, :, iu3[1], iu3[0]] = Lb[:, :, iu3[0], iu3[1]]
            J[:, idx[:, :, None], idx[:, None, :]] = Jb
            L[:, idx[:, :, None], idx[:, None, :]] = Lb
        # J^T cov J through J's at most 3 entries per column (no dense product): nbr[j] the
        # parameters of j's block, Jc[k, j, m] = J[k, nbr[j, m], j]
        ar = np.arange(Ju)
        nbr = np.repeat(ar[:, None], 3, axis=1)
        live = np.zeros((Ju, 3), dtype=bool)
        live[:, 0] = True
        if tri:
            for q in range(3):
                nbr[idx[:, q]] = idx
                live[idx[:, q]] = True
        Jc = J[:, nbr, ar[:, None]] * live
        CJ = sum(cov[:, :, nbr[:, m]] * Jc[:, None, :, m] for m in range(3))
        H = sum(CJ[:, nbr[:, m], :] * Jc[:, :, m, None] for m in range(3)) + L
    iu = np.triu_indices(Ju, 1)
    H[:, iu[1], iu[0]] = H[:, iu[0], iu[1]]
    return H


def br_likelihood_fisher(nfields, bins, mask, hess):
    """Fisher errors from the Hessian of br_likelihood_hess, numpy fp64 on the host:
    {fisher [K, Ju, Ju] = -hess, cov [K, Ju, Ju] its inverse, sigma {spectrum: [K,
    nbins]} the square roots of cov's diagonal (NaN off the used bins)}.  Raises
    ValueError naming the model when -hess has no Cholesky factor (it is not
    positive definite, or not finite); no eigenvalue is clipped."""
    spectra = SPECTRA[int(nfields)]
    mask = np.asarray(mask, dtype=bool)
    if mask.ndim != 2 or mask.shape[0] != len(spectra):
        raise ValueError("br_likelihood_fisher: mask must be bool [nspec, maxbins]")
    nspec, maxbins = mask.shape
    _, used, cols, _ = _br_used("br_likelihood_fisher", nfields, np.ones((1, nspec, maxbins)), mask, bins)
    hess = np.asarray(hess, dtype=np.float64)
    Ju = len(cols)
    if hess.ndim != 3 or hess.shape[1:] != (Ju, Ju):
        raise ValueError(f"br_likelihood_fisher: hess must be [K, Ju, Ju] = [K, {Ju}, {Ju}] (the mask's used columns)")
    K = hess.shape[0]
    fisher = -hess
    cov = np.empty_like(fisher)
    eye = np.eye(Ju)
    for k in range(K):
        try:
            if not np.all(np.isfinite(fisher[k])):
                raise np.linalg.LinAlgError("not finite")
            c = np.linalg.cholesky(fisher[k])
        except np.linalg.LinAlgError:
            raise ValueError(f"Blackwell-Rao Fisher matrix: -hess of model {k} is not positive definite (no Cholesky "
                             "factor): the theory is not at a maximum of the likelihood") from None
        ci = np.linalg.solve(c, eye)
        cov[k] = ci.T @ ci
    sig = np.full((K, nspec * maxbins), np.nan)
    sig[:, cols] = np.sqrt(np.einsum("kjj->kj", cov))
    sig = sig.reshape(K, nspec, maxbins)
    return {"fisher": fisher, "cov": cov,
            "sigma": {s: sig[:, k, :len(bins[s]) - 1].copy() for k, s in enumerate(spectra)}}


class BlackwellRaoLikelihood:
    """Streaming Blackwell-Rao likelihood of K theory spectra over the gs_brl_*
    C-ABI (gs_brl.hip documents the state and the order of operations): a flat
    fp64 device tensor ``data`` = 8 header doubles (int64 iteration count
    first), the planes m, S, Q [3, nchains, K] and the int64 counts of skipped
    rows [nchains].  tables: br_likelihood_tables' dict (kept on the device).
    Plan-independent: any scale ring [capacity, nchains, nspec, maxbins] can be
    accumulated."""
    HDR = 8
    TABLES = ("cols", "kind", "coef", "Y", "cst")

    def __init__(self, nchains, nspec, maxbins, tables, device=None, data=None):
        _require_gpu()
        self.lib = C.load()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.nchains, self.nspec, self.maxbins = int(nchains), int(nspec), int(maxbins)
        host = {k: torch.as_tensor(tables[k]).cpu() for k in self.TABLES}
        cols, kind = host["cols"].to(torch.int64), host["kind"].to(torch.int64)
        self.Ju = int(cols.numel())
        nsb = self.nspec * self.maxbins
        if host["Y"].dim() != 2 or self.Ju < 1 or host["Y"].shape[1] != self.Ju or kind.numel() != self.Ju or \
                host["coef"].numel() != self.Ju or host["cst"].numel() != host["Y"].shape[0]:
            raise ValueError("Blackwell-Rao likelihood: tables must be cols, kind, coef [Ju], Y [K, Ju] and cst [K]")
        # what the kernel indexes the ring with
        if int(cols.min()) < 0 or int(cols.max()) >= nsb or (self.Ju > 1 and bool((cols[1:] <= cols[:-1]).any())):
            raise ValueError("Blackwell-Rao likelihood: cols must ascend within [0, nspec * maxbins)")
        if bool(((kind < 0) | (kind > 2)).any()) or bool((cols[kind == 2] + 3 * self.maxbins >= nsb).any()):
            raise ValueError("Blackwell-Rao likelihood: kind must be 0, 1 or 2 (2: a TT column of four spectra)")
        self.K = int(host["Y"].shape[0])
        self.cols = host["cols"].to(torch.int32).to(dev).contiguous()
        self.kind = host["kind"].to(torch.int32).to(dev).contiguous()
        self.coef, self.Y, self.cst = (host[k].to(torch.float64).to(dev).contiguous() for k in ("coef", "Y", "cst"))
        nb = ctypes.c_longlong()
        C.check(self.lib.gs_brl_bytes(self.nchains, self.K, ctypes.byref(nb)), "gs_brl_bytes")
        if data is None:
            self.data = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
        else:
            self.data = torch.as_tensor(data, dtype=torch.float64).to(dev).contiguous().clone()
            if self.data.numel() * 8 != nb.value:
                raise ValueError("Blackwell-Rao likelihood state: size does not match its dimensions")

    def tables(self):
        """The tables as host tensors (what a state_dict carries)."""
        return {k: getattr(self, k).cpu().clone() for k in self.TABLES}

    def reset(self):
        C.check(self.lib.gs_brl_reset(C.ptr(self.data), self.nchains, self.K, C.stream_ptr()), "gs_brl_reset")

    def update(self, scales, capacity, first_iteration, nsteps):
        """Add iterations first_iteration .. first_iteration + nsteps - 1 from the
        scale ring (iteration it in slot (it - 1) % capacity)."""
        if scales.numel() < int(capacity) * self.nchains * self.nspec * self.maxbins:
            raise ValueError("Blackwell-Rao likelihood update: the scale ring is smaller than capacity rows")
        C.check(self.lib.gs_brl_update(C.ptr(self.data), self.nchains, self.nspec, self.maxbins, self.K, self.Ju,
                                       C.ptr(self.cols), C.ptr(self.kind), C.ptr(self.coef), C.ptr(self.Y),
                                       C.ptr(scales), int(capacity), int(first_iteration), int(nsteps),
                                       C.stream_ptr()), "gs_brl_update")

    @property
    def n(self):
        """Iterations added (reads the device count: synchronises)."""
        return int(self.data[:1].view(torch.int64).item())

    def fields(self):
        """The planes m, S and Q as a view [3, nchains, K]."""
        return self.data[self.HDR:self.HDR + 3 * self.nchains * self.K].view(3, self.nchains, self.K)

    def bad(self):
        """int64 [nchains]: rows skipped for a scale or a block determinant <= 0 or
        not finite (a view)."""
        return self.data[self.HDR + 3 * self.nchains * self.K:].view(torch.int64)

    def finish(self, gather=None):
        """Device tensors loglike [K], chain_loglike [C, K] and neff [K], and n.
        gather (ShardContext.gather): the planes are all-gathered along the
        chain axis first and the finish runs over every rank's chains."""
        data, nch = self.data, self.nchains
        if gather is not None:
            body = gather(self.fields().contiguous(), dim=1)
            nch = int(body.shape[1])
            data = torch.cat([self.data[:self.HDR], body.reshape(-1)])
        dev = self.data.device
        loglike = torch.zeros(self.K, dtype=torch.float64, device=dev)
        chain = torch.zeros(nch, self.K, dtype=torch.float64, device=dev)
        neff = torch.zeros(self.K, dtype=torch.float64, device=dev)
        C.check(self.lib.gs_brl_finish(C.ptr(data), nch, self.K, C.ptr(self.cst), C.ptr(loglike), C.ptr(chain),
                                       C.ptr(neff), C.stream_ptr()), "gs_brl_finish")
        return {"loglike": loglike, "chain_loglike": chain, "neff": neff, "n": self.n}


class BlackwellRaoSamples:
    """Blackwell-Rao sample bank over the gs_brs_* C-ABI (gs_brs.hip documents the
    layout and the order of operations): the scales of the used bins of every
    kept sample, X [nchains, capacity, Jp] and r [nchains, capacity] on the
    device, filled from a scale ring during a run (append) and scored against
    any theory spectra afterwards (loglike) -- the theory need not be known
    before the run, unlike BlackwellRaoLikelihood's.  mask: bool [nspec,
    maxbins], the used bins (the TEB block as a whole).  The tables cols, kind
    and coef are those of br_likelihood_tables; they do not depend on a theory."""
    HDR = 8

    def __init__(self, nchains, nfields, bins, mask, capacity, device=None, draws=False):
        _require_gpu()
        self.lib = C.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.nchains, self.nfields = int(nchains), int(nfields)
        self.draws = bool(draws)
        spectra = SPECTRA[self.nfields]
        self.bins = {s: np.asarray(bins[s], dtype=np.int64).copy() for s in spectra}
        self.mask = np.array(mask, dtype=bool)
        if self.mask.ndim != 2 or self.mask.shape[0] != len(spectra):
            raise ValueError("Blackwell-Rao sample bank: mask must be bool [nspec, maxbins]")
        self.nspec, self.maxbins = self.mask.shape
        one = np.ones((1, self.nspec, self.maxbins))
        if self.nfields == 3:
            one[:, 3] = 0.0
        tab = br_likelihood_tables(self.nfields, self.bins, one, self.mask)
        self.Ju = int(len(tab["cols"]))
        if self.Ju < 1:
            raise ValueError("Blackwell-Rao sample bank: no bin is used (empty used set)")
        self.Jp = (self.Ju + 3) // 4 * 4
        self.cols = torch.from_numpy(tab["cols"]).to(torch.int32).to(self.device).contiguous()
        self.kind = torch.from_numpy(tab["kind"]).to(torch.int32).to(self.device).contiguous()
        self.coef = torch.from_numpy(tab["coef"]).to(torch.float64).to(self.device).contiguous()
        sl, tm = ctypes.c_int(), ctypes.c_int()
        C.check(self.lib.gs_brs_info(ctypes.byref(sl), ctypes.byref(tm)), "gs_brs_info")
        self.slice_rows, self.model_tile = sl.value, tm.value
        self.capacity = 0
        self._n = 0
        self.X = self.r = self.Dl = None
        self._brt = None            # the tables and workspaces of loglike_t / loglike_grad_t, built on first use
        self.reserve(max(int(capacity), 1))

    def nbytes(self, capacity):
        """Device bytes of a bank of `capacity` rows per chain."""
        return 8 * self.nchains * int(capacity) * ((2 if self.draws else 1) * self.Jp + 1)

    def reserve(self, capacity):
        """Grow the bank to `capacity` rows per chain (rows [0, n) are kept)."""
        capacity = int(capacity)
        if capacity <= self.capacity:
            return
        if self.nchains * capacity > 2 ** 31 - 1:
            raise ValueError("Blackwell-Rao sample bank: nchains * capacity exceeds 2^31 - 1 rows")
        need = self.nbytes(capacity)
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise RuntimeError(f"Blackwell-Rao sample bank: {need} bytes ({self.nchains} chains x {capacity} rows x "
                               f"{need // (8 * self.nchains * capacity)} values) do not fit in the {free} bytes of free device memory")
        X = torch.zeros(self.nchains, capacity, self.Jp, dtype=torch.float64, device=self.device)
        r = torch.zeros(self.nchains, capacity, dtype=torch.float64, device=self.device)
        if self._n:
            X[:, :self._n].copy_(self.X[:, :self._n])
            r[:, :self._n].copy_(self.r[:, :self._n])
        if self.draws:
            Dl = torch.zeros(self.nchains, capacity, self.Jp, dtype=torch.float64, device=self.device)
            if self._n:
                Dl[:, :self._n].copy_(self.Dl[:, :self._n])
            self.Dl = Dl
        self.X, self.r, self.capacity = X, r, capacity

    @property
    def n(self):
        """Rows (kept samples per chain) in the bank."""
        return self._n

    def append(self, scales, ring_capacity, first_iteration, nsteps, trace=None):
        """Append iterations first_iteration .. first_iteration + nsteps - 1 of the
        scale ring (iteration it in slot (it - 1) % ring_capacity) at rows n ..; a
        bank with draws also packs the same rows of the D_l trace ring `trace` (the
        scale ring's layout and slots) into Dl (gs_gbr_append)."""
        if scales.numel() < int(ring_capacity) * self.nchains * self.nspec * self.maxbins:
            raise ValueError("Blackwell-Rao sample bank append: the scale ring is smaller than ring_capacity rows")
        if self.draws:
            if trace is None or trace.numel() < int(ring_capacity) * self.nchains * self.nspec * self.maxbins:
                raise ValueError("Blackwell-Rao sample bank append: a bank with draws needs the D_l trace ring of "
                                 "ring_capacity rows")
            C.check(self.lib.gs_gbr_append(C.ptr(self.Dl), self.nchains, self.capacity, self.Ju, self.nspec,
                                           self.maxbins, C.ptr(self.cols), C.ptr(trace), int(ring_capacity),
                                           int(first_iteration), int(nsteps), self._n, C.stream_ptr()), "gs_gbr_append")
        C.check(self.lib.gs_brs_append(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self.Ju, self.nspec,
                                       self.maxbins, C.ptr(self.cols), C.ptr(self.kind), C.ptr(self.coef),
                                       C.ptr(scales), int(ring_capacity), int(first_iteration), int(nsteps), self._n,
                                       C.stream_ptr()), "gs_brs_append")
        self._n += int(nsteps)

    def tables(self, theory):
        """br_likelihood_tables of a theory ({spectrum: [K, nbins]} or [K, nspec,
        maxbins]; checked as run(br_likelihood=)'s) with the bank's mask."""
        from .samplers import br_theory
        th = br_theory("Blackwell-Rao sample bank", theory, self.nfields, self.bins, self.mask)
        return br_likelihood_tables(self.nfields, self.bins, th, self.mask)

    def evaluate(self, Y):
        """The gs_brl state (header, m, S, Q [nchains, K], bad [nchains]) of Y [K,
        Ju] over rows [0, n): a flat fp64 device tensor."""
        Y = torch.as_tensor(Y, dtype=torch.float64).to(self.device).contiguous()
        if Y.dim() != 2 or Y.shape[1] != self.Ju or Y.shape[0] < 1:
            raise ValueError(f"Blackwell-Rao sample bank: Y must be [K, Ju] = [K, {self.Ju}]")
        K = int(Y.shape[0])
        nb, wb = ctypes.c_longlong(), ctypes.c_longlong()
        C.check(self.lib.gs_brl_bytes(self.nchains, K, ctypes.byref(nb)), "gs_brl_bytes")
        C.check(self.lib.gs_brs_work_bytes(self.nchains, self._n, K, ctypes.byref(wb)), "gs_brs_work_bytes")
        state = torch.empty(nb.value // 8, dtype=torch.float64, device=self.device)
        work = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brs_eval(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self._n, self.Ju, K,
                                     C.ptr(Y), C.ptr(work), wb.value, C.ptr(state), C.stream_ptr()), "gs_brs_eval")
        return state

    def fields(self, state):
        """The planes m, S and Q of an evaluate() state as a view [3, nchains, K]."""
        K = (state.numel() - self.HDR - self.nchains) // (3 * self.nchains)
        return state[self.HDR:self.HDR + 3 * self.nchains * K].view(3, self.nchains, K)

    def loglike(self, theory, gather=None):
        """The Blackwell-Rao likelihood of K theory spectra over the bank, numpy:
        {loglike [K], chain_loglike [C, K], neff [K], n, bad [nchains]} as
        runner.br_likelihood() gives them.  gather (ShardContext.gather): the
        state planes are all-gathered along the chain axis before the finish."""
        tab = self.tables(theory)
        K = int(tab["Y"].shape[0])
        state = self.evaluate(tab["Y"])
        cst = torch.from_numpy(np.ascontiguousarray(tab["cst"])).to(self.device)
        bad = state[self.HDR + 3 * self.nchains * K:].view(torch.int64).cpu().numpy().copy()
        nch = self.nchains
        if gather is not None:
            body = gather(self.fields(state).contiguous(), dim=1)
            nch = int(body.shape[1])
            state = torch.cat([state[:self.HDR], body.reshape(-1)])
        loglike = torch.zeros(K, dtype=torch.float64, device=self.device)
        chain = torch.zeros(nch, K, dtype=torch.float64, device=self.device)
        neff = torch.zeros(K, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brl_finish(C.ptr(state), nch, K, C.ptr(cst), C.ptr(loglike), C.ptr(chain), C.ptr(neff),
                                       C.stream_ptr()), "gs_brl_finish")
        return {"loglike": loglike.cpu().numpy(), "chain_loglike": chain.cpu().numpy(), "neff": neff.cpu().numpy(),
                "n": self._n, "bad": bad}

    def grad_numerators(self, Y, mref):
        """num [nchains, K, Jp] (device): num[c, k, j] = sum_i exp(t_cik - mref_k)
        X[c, i, j] over rows [0, n), a second pass over the bank (gs_brs_grad);
        Y [K, Ju], mref [K]."""
        Y = torch.as_tensor(Y, dtype=torch.float64).to(self.device).contiguous()
        mref = torch.as_tensor(mref, dtype=torch.float64).to(self.device).contiguous()
        if Y.dim() != 2 or Y.shape[1] != self.Ju or Y.shape[0] < 1 or tuple(mref.shape) != (Y.shape[0],):
            raise ValueError(f"Blackwell-Rao sample bank: Y must be [K, Ju] = [K, {self.Ju}] and mref [K]")
        K = int(Y.shape[0])
        wb = ctypes.c_longlong()
        C.check(self.lib.gs_brs_grad_work_bytes(self.nchains, self._n, K, self.Ju, ctypes.byref(wb)),
                "gs_brs_grad_work_bytes")
        work = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        num = torch.empty(self.nchains, K, self.Jp, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brs_grad(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self._n, self.Ju, K,
                                     C.ptr(Y), C.ptr(mref), C.ptr(work), wb.value, C.ptr(num), C.stream_ptr()),
                "gs_brs_grad")
        return num

    def loglike_grad(self, theory, gather=None):
        """loglike(theory) and its gradient with respect to the theory spectra,
        numpy: everything loglike returns (the same bits), and
          grad          {spectrum: [K, nbins]}, d loglike_k / d D^th (0 on the bins
                        that are not used)
          mean_scale    [K, nspec, maxbins], the likelihood-weighted mean of the
                        bank's scales under each theory (NaN off the used set)
          chain_weight  [C, K], the share of each chain in the estimate
        (NaN for an empty bank).  A second pass over the bank forms the weighted
        sums on the matrix cores (gs_brs.hip); engine.br_likelihood_grad is the
        chain rule.  gather (ShardContext.gather): the state planes, and then the
        per-chain numerators, are all-gathered along the chain axis."""
        return self._grad_pass(theory, gather)[0]

    def _grad_pass(self, theory, gather):
        """loglike_grad's dict, and what the Hessian pass goes on from (device: Y,
        mref, the gathered state and xbar; the checked theory)."""
        from .samplers import br_theory
        th = br_theory("Blackwell-Rao sample bank", theory, self.nfields, self.bins, self.mask)
        tab = br_likelihood_tables(self.nfields, self.bins, th, self.mask)
        K = int(tab["Y"].shape[0])
        Y = torch.from_numpy(np.ascontiguousarray(tab["Y"])).to(self.device)
        state = self.evaluate(Y)
        cst = torch.from_numpy(np.ascontiguousarray(tab["cst"])).to(self.device)
        bad = state[self.HDR + 3 * self.nchains * K:].view(torch.int64).cpu().numpy().copy()
        nch = self.nchains
        if gather is not None:
            body = gather(self.fields(state).contiguous(), dim=1)
            nch = int(body.shape[1])
            state = torch.cat([state[:self.HDR], body.reshape(-1)])
        loglike = torch.zeros(K, dtype=torch.float64, device=self.device)
        chain = torch.zeros(nch, K, dtype=torch.float64, device=self.device)
        neff = torch.zeros(K, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brl_finish(C.ptr(state), nch, K, C.ptr(cst), C.ptr(loglike), C.ptr(chain), C.ptr(neff),
                                       C.stream_ptr()), "gs_brl_finish")
        # M_k over every (gathered) chain that holds a sample: the weights' reference
        m, S = (state[self.HDR + p * nch * K:self.HDR + (p + 1) * nch * K].view(nch, K) for p in (0, 1))
        mref = torch.where(S > 0, m, torch.full_like(m, float("-inf"))).amax(dim=0)
        mref = torch.where(torch.isinf(mref), torch.zeros_like(mref), mref)
        num = self.grad_numerators(Y, mref)
        if gather is not None:
            num = gather(num, dim=0).contiguous()
        xbar = torch.zeros(K, self.Ju, dtype=torch.float64, device=self.device)
        cw = torch.zeros(nch, K, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brs_grad_finish(C.ptr(num), C.ptr(state), nch, K, self.Ju, C.ptr(xbar), C.ptr(cw),
                                            C.stream_ptr()), "gs_brs_grad_finish")
        xb = xbar.cpu().numpy()
        g = br_likelihood_grad(self.nfields, self.bins, th, self.mask, xb)
        spectra = SPECTRA[self.nfields]
        mean = np.full((K, self.nspec * self.maxbins), np.nan)
        mean[:, self.cols.cpu().numpy().astype(np.int64)] = xb
        out = {"loglike": loglike.cpu().numpy(), "chain_loglike": chain.cpu().numpy(), "neff": neff.cpu().numpy(),
               "n": self._n, "bad": bad,
               "grad": {s: g[:, k, :len(self.bins[s]) - 1].copy() for k, s in enumerate(spectra)},
               "mean_scale": mean.reshape(K, self.nspec, self.maxbins), "chain_weight": cw.cpu().numpy()}
        return out, {"theory": th, "Y": Y, "mref": mref, "state": state, "nch": nch, "xbar": xbar}


    def hess_numerators(self, Y, mref, center):
        """num2 [nchains, K, Jp, Jp] (device): num2[c, k, a, b] = sum_i exp(t_cik -
        mref_k) u_cia u_cib over rows [0, n), u_cia = X[c, i, a] - center[k, a], a
        third pass over the bank (gs_brs_hess); Y [K, Ju], mref [K], center [K, Ju]
        (the likelihood-weighted mean scales of the complete bank)."""
        Y = torch.as_tensor(Y, dtype=torch.float64).to(self.device).contiguous()
        mref = torch.as_tensor(mref, dtype=torch.float64).to(self.device).contiguous()
        center = torch.as_tensor(center, dtype=torch.float64).to(self.device).contiguous()
        if Y.dim() != 2 or Y.shape[1] != self.Ju or Y.shape[0] < 1 or tuple(mref.shape) != (Y.shape[0],) or \
                tuple(center.shape) != tuple(Y.shape):
            raise ValueError(f"Blackwell-Rao sample bank: Y and center must be [K, Ju] = [K, {self.Ju}] and mref [K]")
        K = int(Y.shape[0])
        wb = ctypes.c_longlong()
        C.check(self.lib.gs_brs_hess_work_bytes(self.nchains, self._n, K, self.Ju, ctypes.byref(wb)),
                "gs_brs_hess_work_bytes")
        work = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        num2 = torch.empty(self.nchains, K, self.Jp, self.Jp, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brs_hess(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self._n, self.Ju, K,
                                     C.ptr(Y), C.ptr(mref), C.ptr(center), C.ptr(work), wb.value, C.ptr(num2),
                                     C.stream_ptr()), "gs_brs_hess")
        return num2

    def loglike_hess(self, theory, gather=None):
        """loglike_grad(theory) and the Hessian with respect to the theory spectra,
        numpy: everything loglike_grad returns (the same bits), and
          hess       [K, Ju, Ju], d^2 loglike_k / d D^th_a d D^th_b over the used
                     theory entries
          scale_cov  [K, Ju, Ju], the likelihood-weighted covariance of the bank's
                     used scale columns under each theory
          params     [(spectrum, bin)] of each row and column of the two
        (NaN for an empty bank).  A third pass over the bank forms the centred
        second moments on the matrix cores (gs_brh.hip), centred on the gradient
        pass's mean scales; engine.br_likelihood_hess is the chain rule.  gather
        (ShardContext.gather): the state planes, the per-chain numerators and then
        the per-chain second moments are all-gathered along the chain axis."""
        out, g = self._grad_pass(theory, gather)
        K = int(g["Y"].shape[0])
        num2 = self.hess_numerators(g["Y"], g["mref"], g["xbar"])
        if gather is not None:
            num2 = gather(num2, dim=0).contiguous()
        cov = torch.zeros(K, self.Ju, self.Ju, dtype=torch.float64, device=self.device)
        C.check(self.lib.gs_brs_hess_finish(C.ptr(num2), C.ptr(g["state"]), g["nch"], K, self.Ju, C.ptr(cov),
                                            C.stream_ptr()), "gs_brs_hess_finish")
        cv = cov.cpu().numpy()
        spectra = SPECTRA[self.nfields]
        out["hess"] = br_likelihood_hess(self.nfields, self.bins, g["theory"], self.mask, g["xbar"].cpu().numpy(), cv)
        out["scale_cov"] = cv
        out["params"] = [(spectra[int(c) // self.maxbins], int(c) % self.maxbins) for c in self.cols.cpu().numpy()]
        return out

    def fisher(self, theory, gather=None):
        """Fisher errors of the theory spectra at `theory` (a maximum of the
        likelihood), numpy: {fisher [K, Ju, Ju] = -hess of loglike_hess, cov [K, Ju,
        Ju] its inverse, sigma {spectrum: [K, nbins]} (NaN off the used bins)}.
        Raises ValueError naming the model when -hess is not positive definite."""
        return br_likelihood_fisher(self.nfields, self.bins, self.mask, self.loglike_hess(theory, gather)["hess"])

    # -- theories on the device (gs_brt.hip) -----------------------------------------
    def _brt_tables(self):
        """The theory-free tables of gs_brt.hip (device; built once): part, cons,
        inv, and the fiducial [nspec, maxbins] a dict theory's missing spectra take."""
        if self._brt is not None:
            return self._brt
        spectra = SPECTRA[self.nfields]
        cols = self.cols.cpu().numpy().astype(np.int64)
        kind = self.kind.cpu().numpy()
        pos = {int(c): j for j, c in enumerate(cols)}
        part = np.full((2, self.Ju), -1, dtype=np.int32)
        cons = np.zeros((2, self.Ju))
        for j, c in enumerate(cols):
            sp, b = divmod(int(c), self.maxbins)
            if kind[j] == 0:
                continue
            e = np.asarray(self.bins[spectra[sp]], dtype=np.float64)
            n_b = e[b + 1] ** 2 - e[b] ** 2
            cons[0, j] = 0.5 * n_b
            if kind[j] == 2:
                nu = n_b - 3.0
                part[0, j], part[1, j] = pos[self.maxbins + b], pos[3 * self.maxbins + b]
                lg2 = 0.5 * math.log(math.pi) + math.lgamma(0.5 * nu) + math.lgamma(0.5 * nu - 0.5)
                cons[1, j] = -nu * math.log(2.0) - lg2
            else:
                cons[1, j] = -math.lgamma(0.5 * n_b - 1.0)
        inv = np.full(self.nspec * self.maxbins, -1, dtype=np.int32)
        inv[cols] = np.arange(self.Ju, dtype=np.int32)
        fid = np.ones((self.nspec, self.maxbins))
        if self.nfields == 3:
            fid[3] = 0.0
        dev = self.device
        self._brt = {"part": torch.from_numpy(part).to(dev).contiguous(), "cons": torch.from_numpy(cons).to(dev).contiguous(),
                     "inv": torch.from_numpy(inv).to(dev).contiguous(), "fiducial": torch.from_numpy(fid).to(dev),
                     "ws": {}}
        return self._brt

    @property
    def fiducial(self):
        """Device tensor [nspec, maxbins]: what loglike_t / loglike_grad_t put where a
        dict theory names no spectrum (and past a spectrum's bins) -- 1 and TE = 0,
        the values samplers.br_theory pads with, until it is overwritten in place."""
        return self._brt_tables()["fiducial"]

    def _brt_workspace(self, K, grad):
        """The buffers of one K (kept on the object; rebuilt when the bank has grown)."""
        tb = self._brt_tables()
        ws = tb["ws"].get(K)
        dev, f64 = self.device, torch.float64
        if ws is None or ws["n"] != self._n:
            nb, wb = ctypes.c_longlong(), ctypes.c_longlong()
            C.check(self.lib.gs_brl_bytes(self.nchains, K, ctypes.byref(nb)), "gs_brl_bytes")
            C.check(self.lib.gs_brs_work_bytes(self.nchains, self._n, K, ctypes.byref(wb)), "gs_brs_work_bytes")
            ws = {"n": self._n, "wb": wb.value,
                  "D": torch.empty(K, self.nspec, self.maxbins, dtype=f64, device=dev),
                  "Y": torch.zeros(K, self.Ju, dtype=f64, device=dev), "cst": torch.zeros(K, dtype=f64, device=dev),
                  "bad_model": torch.zeros(K, dtype=torch.int32, device=dev),
                  "state": torch.zeros(nb.value // 8, dtype=f64, device=dev),
                  "work": torch.zeros(wb.value // 8, dtype=f64, device=dev),
                  "loglike": torch.zeros(K, dtype=f64, device=dev),
                  "chain_loglike": torch.zeros(self.nchains, K, dtype=f64, device=dev),
                  "neff": torch.zeros(K, dtype=f64, device=dev)}
            tb["ws"][K] = ws
        if grad and "grad" not in ws:
            gb = ctypes.c_longlong()
            C.check(self.lib.gs_brs_grad_work_bytes(self.nchains, self._n, K, self.Ju, ctypes.byref(gb)),
                    "gs_brs_grad_work_bytes")
            ws.update(gb=gb.value, gwork=torch.zeros(gb.value // 8, dtype=f64, device=dev),
                      mref=torch.zeros(K, dtype=f64, device=dev),
                      num=torch.zeros(self.nchains, K, self.Jp, dtype=f64, device=dev),
                      xbar=torch.zeros(K, self.Ju, dtype=f64, device=dev),
                      chain_weight=torch.zeros(self.nchains, K, dtype=f64, device=dev),
                      grad=torch.zeros(K, self.nspec, self.maxbins, dtype=f64, device=dev),
                      mean_scale=torch.zeros(K, self.nspec, self.maxbins, dtype=f64, device=dev))
        return ws

    def _brt_theory(self, theory):
        """(K, D [K, nspec, maxbins] contiguous fp64 on the bank's device) of a tensor
        or a dict of tensors; a dict is packed into the workspace of its K over the
        fiducial.  Shapes are checked, values are not (gs_brt_tables flags them)."""
        spectra = SPECTRA[self.nfields]
        if isinstance(theory, dict):
            if not theory or set(theory) - set(spectra):
                raise ValueError(f"Blackwell-Rao sample bank: theory names spectra of {list(spectra)}")
            vals = {s: v if v.dim() == 2 else v.reshape(1, -1) for s, v in theory.items()}
            K = int(next(iter(vals.values())).shape[0])
            for s, v in vals.items():
                nb = len(self.bins[s]) - 1
                if not torch.is_tensor(v) or tuple(v.shape) != (K, nb) or v.device != self.device:
                    raise ValueError(f"Blackwell-Rao sample bank: theory[{s}] must be a tensor [K, nbins] = [{K}, {nb}] "
                                     "on the bank's device")
            if K < 1:
                raise ValueError("Blackwell-Rao sample bank: at least one theory spectrum (K >= 1) is needed")
            D = self._brt_workspace(K, False)["D"]
            D.copy_(self.fiducial.unsqueeze(0).expand_as(D))
            for k, s in enumerate(spectra):
                if s in vals:
                    D[:, k, :vals[s].shape[1]].copy_(vals[s])
            return K, D
        if not torch.is_tensor(theory) or theory.dim() != 3 or tuple(theory.shape[1:]) != (self.nspec, self.maxbins) or \
                theory.shape[0] < 1 or theory.device != self.device:
            raise ValueError("Blackwell-Rao sample bank: theory must be a tensor [K, nspec, maxbins] = "
                             f"[K, {self.nspec}, {self.maxbins}] on the bank's device (or a dict of tensors)")
        K = int(theory.shape[0])
        th = theory.detach()
        if th.dtype != torch.float64 or not th.is_contiguous():
            D = self._brt_workspace(K, False)["D"]
            D.copy_(th)
            th = D
        return K, th

    def _brt_pass(self, theory, gather, grad):
        tb = self._brt_tables()
        K, D = self._brt_theory(theory)
        ws = self._brt_workspace(K, grad)
        st = C.stream_ptr()
        lib = self.lib
        C.check(lib.gs_brt_tables(C.ptr(D), K, self.nspec, self.maxbins, self.Ju, C.ptr(self.cols), C.ptr(self.kind),
                                  C.ptr(tb["part"]), C.ptr(tb["cons"]), C.ptr(ws["Y"]), C.ptr(ws["cst"]),
                                  C.ptr(ws["bad_model"]), st), "gs_brt_tables")
        state = ws["state"]
        C.check(lib.gs_brs_eval(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self._n, self.Ju, K,
                                C.ptr(ws["Y"]), C.ptr(ws["work"]), ws["wb"], C.ptr(state), st), "gs_brs_eval")
        bad = state[self.HDR + 3 * self.nchains * K:].view(torch.int64)
        nch = self.nchains
        loglike, chain, neff = ws["loglike"], ws["chain_loglike"], ws["neff"]
        if gather is not None:
            body = gather(self.fields(state).contiguous(), dim=1)
            nch = int(body.shape[1])
            state = torch.cat([state[:self.HDR], body.reshape(-1)])
            chain = torch.zeros(nch, K, dtype=torch.float64, device=self.device)
        C.check(lib.gs_brl_finish(C.ptr(state), nch, K, C.ptr(ws["cst"]), C.ptr(loglike), C.ptr(chain), C.ptr(neff), st),
                "gs_brl_finish")
        out = {"loglike": loglike, "chain_loglike": chain, "neff": neff, "n": self._n, "bad": bad,
               "bad_model": ws["bad_model"]}
        if not grad:
            return out
        C.check(lib.gs_brt_mref(C.ptr(state), nch, K, C.ptr(ws["mref"]), st), "gs_brt_mref")
        num, cw = ws["num"], ws["chain_weight"]
        C.check(lib.gs_brs_grad(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, self._n, self.Ju, K,
                                C.ptr(ws["Y"]), C.ptr(ws["mref"]), C.ptr(ws["gwork"]), ws["gb"], C.ptr(num), st),
                "gs_brs_grad")
        if gather is not None:
            num = gather(num, dim=0).contiguous()
            cw = torch.zeros(nch, K, dtype=torch.float64, device=self.device)
        C.check(lib.gs_brs_grad_finish(C.ptr(num), C.ptr(state), nch, K, self.Ju, C.ptr(ws["xbar"]), C.ptr(cw), st),
                "gs_brs_grad_finish")
        C.check(lib.gs_brt_chain(C.ptr(D), C.ptr(ws["xbar"]), C.ptr(ws["bad_model"]), K, self.nspec, self.maxbins,
                                 self.Ju, C.ptr(self.cols), C.ptr(self.kind), C.ptr(tb["part"]), C.ptr(tb["cons"]),
                                 C.ptr(tb["inv"]), C.ptr(ws["grad"]), C.ptr(ws["mean_scale"]), st), "gs_brt_chain")
        out.update(grad=ws["grad"], mean_scale=ws["mean_scale"], chain_weight=cw)
        return out

    def loglike_t(self, theory, gather=None):
        """loglike() of theories that live on the device, with no host round trip:
        theory a tensor [K, nspec, maxbins] or {spectrum: tensor [K, nbins]} (packed
        on the device over `fiducial`) on the bank's device.  Returns loglike [K],
        chain_loglike [C, K], neff [K] and bad [nchains] as device tensors, n, and
        bad_model [K] (int32): 1 for a theory loglike() would refuse (a used value
        not finite or a variance <= 0, a TEB block not positive definite) -- its
        loglike is NaN, nothing is raised.  The tables are built by gs_brt.hip; the
        evaluator and the finish are loglike()'s.  Nothing is read back, nothing
        synchronises and, after the first call with a K, nothing is allocated: with
        gather=None the call can be captured in a torch.cuda.graph after one warm-up
        call.  The tensors returned are the bank's workspace of that K: the next call
        with the same K overwrites them (clone what has to outlive it), and
        appending rows replaces them."""
        return self._brt_pass(theory, gather, False)

    def loglike_grad_t(self, theory, gather=None):
        """loglike_grad() of theories that live on the device: everything loglike_t
        returns, and grad [K, nspec, maxbins] (d loglike_k / d D^th: exactly 0 off
        the used bins, NaN for a bad model), mean_scale [K, nspec, maxbins] and
        chain_weight [C, K], device tensors of the bank's workspace under loglike_t's
        rules.  The chain rule runs in gs_brt.hip."""
        return self._brt_pass(theory, gather, True)

    def loglike_torch(self, theory):
        """loglike [K] of a device tensor theory [K, nspec, maxbins], differentiable:
        a torch.autograd.Function over loglike_grad_t whose backward is grad_out[:,
        None, None] * grad of the same pass (no second evaluation).  A theory that
        does not require a gradient takes loglike_t alone.  The result is a fresh
        tensor.  Second derivatives are not provided: loglike_hess has them."""
        return _BankLoglike.apply(theory, self)

    # -- Gaussianised Blackwell-Rao likelihood (gs_gbr.hip) ----------------------------
    def gaussianize(self, points=None, span=GBR_SPAN, gather=None):
        """The Gaussianised Blackwell-Rao likelihood (Rudjord et al. 2009) fitted to
        the bank, an engine.GaussianizedBlackwellRao: each inverse-Gamma column (all
        of them for EE/BB and TT; TT, EE and BB of a TEB run, whose TE has no
        one-dimensional marginal and is marginalised over) is mapped through its own
        Blackwell-Rao marginal to a standard normal x_j(D_j), and a Gaussian (mu, C)
        is fitted to the transformed draws of the bank.  Needs a bank with draws
        (br_samples={"draws": True}).  points: G nodes per column (default
        GBR_POINTS), geometric in D, of which nodes 1 .. G - 2 cover [a min D, b max
        D] of the column's kept draws, span = (a, b) with a < 1 < b; the end nodes
        lie outside that interval (default GBR_SPAN: b = 8 keeps the heavy right
        tail of the low-l marginals on the grid).  gather (ShardContext.gather): the extremes, the
        per-chain marginal partials and the per-chain moment sums are all-gathered
        along the chain axis, and every rank fits the same likelihood.  Raises
        ValueError when the kept samples are not more than the columns or the
        covariance is not positive definite."""
        if not self.draws:
            raise ValueError("Blackwell-Rao sample bank: gaussianize needs the D_l draws in the bank "
                             "(run(br_samples={..., 'draws': True}))")
        G = GBR_POINTS if points is None else int(points)
        a, b = (float(v) for v in span)
        if not 8 <= G <= 256:
            raise ValueError("gaussianize: points must lie in [8, 256]")
        if not (0.0 < a < 1.0 < b and math.isfinite(b)):
            raise ValueError("gaussianize: span = (a, b) needs 0 < a < 1 < b")
        n = self._n
        if n < 1:
            raise ValueError("gaussianize: the bank is empty; more kept samples than columns are needed")
        col = gbr_columns(self.nfields, self.bins, self.mask)
        Jg = len(col["gcol"])
        dev, f64 = self.device, torch.float64
        gcol = torch.from_numpy(col["gcol"]).to(dev)
        alpha = torch.from_numpy(col["alpha"]).to(dev)
        half = torch.from_numpy(col["half"]).to(dev)
        # the extremes of the kept draws per column (rows whose r is NaN are skipped rows)
        good = ~torch.isnan(self.r[:, :n])
        gl = gcol.long()
        d = self.Dl[:, :n][:, :, gl]
        lo = torch.where(good[:, :, None], d, torch.full_like(d, float("inf"))).amin(dim=(0, 1))
        hi = torch.where(good[:, :, None], d, torch.full_like(d, float("-inf"))).amax(dim=(0, 1))
        del d
        if gather is not None:
            lo, hi = gather(lo[None], dim=0).amin(dim=0), gather(hi[None], dim=0).amax(dim=0)
        glo, gh = gbr_grid(lo.cpu().numpy(), hi.cpu().numpy(), G, a, b)
        glo_d, gh_d = torch.from_numpy(glo).to(dev), torch.from_numpy(gh).to(dev)
        st = C.stream_ptr()
        lib = self.lib
        m = torch.zeros(self.nchains, Jg, G, dtype=f64, device=dev)
        S = torch.zeros(self.nchains, Jg, G, dtype=f64, device=dev)
        cnt = torch.zeros(self.nchains, dtype=torch.int64, device=dev)
        C.check(lib.gs_gbr_marginals(C.ptr(self.X), C.ptr(self.r), self.nchains, self.capacity, n, self.Ju, Jg,
                                     C.ptr(gcol), C.ptr(alpha), C.ptr(half), C.ptr(glo_d), C.ptr(gh_d), G, C.ptr(m),
                                     C.ptr(S), C.ptr(cnt), st), "gs_gbr_marginals")
        part = {"m": m, "S": S, "cnt": cnt}
        if gather is not None:
            m, S, cnt = (gather(v, dim=0).contiguous() for v in (m, S, cnt))
        logp = torch.zeros(Jg, G, dtype=f64, device=dev)
        C.check(lib.gs_gbr_marginals_finish(C.ptr(m), C.ptr(S), C.ptr(cnt), int(m.shape[0]), Jg, G, C.ptr(alpha),
                                            C.ptr(glo_d), C.ptr(gh_d), C.ptr(logp), st), "gs_gbr_marginals_finish")
        tx = torch.zeros(Jg, G, 2, dtype=f64, device=dev)
        tp = torch.zeros(Jg, G, 2, dtype=f64, device=dev)
        mass = torch.zeros(Jg, dtype=f64, device=dev)
        C.check(lib.gs_gbr_tables(C.ptr(logp), Jg, G, C.ptr(glo_d), C.ptr(gh_d), C.ptr(tx), C.ptr(tp), C.ptr(mass), st),
                "gs_gbr_tables")
        wb = ctypes.c_longlong()
        C.check(lib.gs_gbr_moments_work_bytes(self.nchains, n, Jg, ctypes.byref(wb)), "gs_gbr_moments_work_bytes")
        work = torch.empty(wb.value // 8, dtype=f64, device=dev)
        S1 = torch.zeros(self.nchains, Jg, dtype=f64, device=dev)
        S2 = torch.zeros(self.nchains, Jg, Jg, dtype=f64, device=dev)
        C.check(lib.gs_gbr_moments(C.ptr(self.Dl), C.ptr(self.r), self.nchains, self.capacity, n, self.Ju, Jg,
                                   C.ptr(gcol), C.ptr(tx), C.ptr(glo_d), C.ptr(gh_d), G, C.ptr(work), wb.value,
                                   C.ptr(S1), C.ptr(S2), st), "gs_gbr_moments")
        part.update(S1=S1, S2=S2)
        if gather is not None:
            S1, S2 = gather(S1, dim=0).contiguous(), gather(S2, dim=0).contiguous()
        fit = gbr_finish(cnt.cpu().numpy(), S1.cpu().numpy(), S2.cpu().numpy())
        out = GaussianizedBlackwellRao(self.nfields, self.bins, self.mask, col["tcol"], glo, gh, tx, tp, fit["mu"],
                                       fit["chol"], fit["logdet"], fit["n"], mass, device=dev)
        out.cov, out.chain_sums, out.logp = fit["cov"], part, logp
        return out

    # -- checkpoints and files -------------------------------------------------------
    def state(self):
        """Host tensors of rows [0, n) and the mask (what a state_dict carries)."""
        st = {"X": self.X[:, :self._n].cpu().clone(), "r": self.r[:, :self._n].cpu().clone(),
              "mask": torch.from_numpy(self.mask.copy())}
        if self.draws:
            st["Dl"] = self.Dl[:, :self._n].cpu().clone()
        return st

    @classmethod
    def from_state(cls, st, nfields, bins, capacity=None, device=None):
        """A bank holding the rows of state() (capacity: rows to make room for)."""
        X, r = torch.as_tensor(st["X"], dtype=torch.float64), torch.as_tensor(st["r"], dtype=torch.float64)
        n = int(r.shape[1])
        Dl = st.get("Dl") if hasattr(st, "get") else None
        self = cls(int(r.shape[0]), nfields, bins, np.asarray(st["mask"], dtype=bool), max(n, int(capacity or 0)),
                   device=device, draws=Dl is not None)
        if X.dim() != 3 or tuple(X.shape) != (self.nchains, n, self.Jp):
            raise ValueError("Blackwell-Rao sample bank state: X must be [nchains, n, Jp] of the mask's used columns")
        if Dl is not None:
            Dl = torch.as_tensor(Dl, dtype=torch.float64)
            if tuple(Dl.shape) != tuple(X.shape):
                raise ValueError("Blackwell-Rao sample bank state: Dl must have the shape of X")
            self.Dl[:, :n].copy_(Dl)
        self.X[:, :n].copy_(X)
        self.r[:, :n].copy_(r)
        self._n = n
        return self

    def save(self, path):
        """Write rows [0, n), the tables, the bins, the mask and nfields to an
        .npz file (numeric arrays only: loads with allow_pickle=False)."""
        st = self.state()
        extra = {"Dl": st["Dl"].numpy()} if self.draws else {}
        np.savez(path, X=st["X"].numpy(), r=st["r"].numpy(), mask=self.mask, nfields=np.int64(self.nfields),
                 cols=self.cols.cpu().numpy(), kind=self.kind.cpu().numpy(), coef=self.coef.cpu().numpy(),
                 **{"bins_" + s: b for s, b in self.bins.items()}, **extra)

    @classmethod
    def load(cls, path, device=None):
        """The bank of a save()d file."""
        with np.load(path, allow_pickle=False) as f:
            F = int(f["nfields"])
            bins = {s: f["bins_" + s] for s in SPECTRA[F]}
            st = {"X": f["X"], "r": f["r"], "mask": f["mask"]}
            if "Dl" in f.files:
                st["Dl"] = f["Dl"]
            self = cls.from_state(st, F, bins, device=device)
            if not np.array_equal(f["cols"], self.cols.cpu().numpy()):
                raise ValueError("Blackwell-Rao sample bank file: its columns do not match its bins and mask")
        return self




def gbr_columns(nfields, bins, mask):
    """The columns the Gaussianised Blackwell-Rao likelihood uses of a bank with
    the used bins `mask`, numpy: gcol [Jg] int32 (positions among the bank's Ju
    used columns), tcol [Jg] int32 (their entries of a theory [nspec * maxbins]),
    alpha [Jg] and half [Jg] (beta = half x recorded scale) as br_shapes gives
    them -- every inverse-Gamma column; of a TEB block TT and EE through their
    inverse-Gamma marginals (alpha = n_b / 2 - 2, beta = Psi_ii / 2), TE left out."""
    F = int(nfields)
    mask = np.asarray(mask, dtype=bool)
    maxbins = mask.shape[1]
    _, _, cols, _ = _br_used("gbr_columns", F, np.ones((1,) + mask.shape), mask, bins)
    alpha, half_mask = br_shapes(F, bins, maxbins)
    a = alpha.reshape(-1)[cols]
    keep = np.flatnonzero(np.isfinite(a))
    if len(keep) == 0:
        raise ValueError("gbr_columns: no inverse-Gamma column is used")
    tcol = cols[keep]
    half = np.where((half_mask >> (tcol // maxbins)) & 1, 0.5, 1.0)
    return {"gcol": keep.astype(np.int32), "tcol": tcol.astype(np.int32), "alpha": np.ascontiguousarray(a[keep]),
            "half": half.astype(np.float64)}


def gbr_grid(dmin, dmax, G, a, b):
    """(glo, gh [Jg]) of the node rule lD_g = glo + g gh: node 1 at log(a dmin), node
    G - 2 at log(b dmax), so that every D in [a dmin, b dmax] has 1 <= u <= G - 2."""
    dmin, dmax = np.asarray(dmin, dtype=np.float64), np.asarray(dmax, dtype=np.float64)
    if not (np.all(np.isfinite(dmin)) and np.all(np.isfinite(dmax)) and np.all(dmin > 0)):
        raise ValueError("gaussianize: the kept draws of a column are not positive and finite (or there are none)")
    l1, l2 = np.log(a * dmin), np.log(b * dmax)
    gh = (l2 - l1) / (G - 3)
    return np.ascontiguousarray(l1 - gh), np.ascontiguousarray(gh)


def gbr_finish(cnt, S1, S2):
    """The Gaussian fit from the per-chain sums, numpy fp64 on the host, the chains
    in chain order: N = sum cnt, mu = S1 / N, cov = (S2 - N mu mu^T) / (N - 1), its
    lower Cholesky factor and log determinant.  Raises ValueError when N <= Jg or
    cov is not positive definite."""
    cnt = np.asarray(cnt, dtype=np.int64)
    S1, S2 = np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    Jg = S1.shape[1]
    N = int(cnt.sum())
    if N <= Jg:
        raise ValueError(f"Gaussianised Blackwell-Rao: {N} kept samples for {Jg} columns: more kept samples than "
                         "columns are needed")
    s1, s2 = np.zeros(Jg), np.zeros((Jg, Jg))
    for c in range(S1.shape[0]):
        s1 = s1 + S1[c]
        s2 = s2 + S2[c]
    mu = s1 / N
    cov = (s2 - N * np.outer(mu, mu)) / (N - 1)
    try:
        if not np.all(np.isfinite(cov)):
            raise np.linalg.LinAlgError("not finite")
        chol = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(f"Gaussianised Blackwell-Rao: the covariance of the {Jg} transformed columns over {N} kept "
                         "samples is not positive definite: more kept samples than columns are needed") from None
    return {"n": N, "mu": mu, "cov": cov, "chol": chol, "logdet": 2.0 * float(np.sum(np.log(np.diag(chol))))}


class GaussianizedBlackwellRao:
    """The Gaussianised Blackwell-Rao likelihood of BlackwellRaoSamples.gaussianize
    (gs_gbr.hip documents the tables): per column the tables x(D) and log p(D) on a
    grid uniform in log D, the mean mu and the lower Cholesky factor of the
    covariance of the transformed draws (on the device), and
      log L(D) = sum_j log p_j(D_j) - (x - mu)^T C^-1 (x - mu) / 2 + x^T x / 2 - log det C / 2.
    For a TEB run this is the likelihood of (TT, EE, BB) with TE marginalised: the
    theory's TE values are ignored.  It evaluates without the bank."""

    def __init__(self, nfields, bins, mask, tcol, glo, gh, tx, tp, mu, chol, logdet, n, mass, device=None):
        _require_gpu()
        self.lib = C.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.nfields = int(nfields)
        spectra = SPECTRA[self.nfields]
        self.bins = {s: np.asarray(bins[s], dtype=np.int64).copy() for s in spectra}
        self.mask = np.array(mask, dtype=bool)
        self.nspec, self.maxbins = self.mask.shape
        dev, f64 = self.device, torch.float64
        tcol = np.asarray(tcol, dtype=np.int32)
        self.Jg = int(len(tcol))
        if self.Jg < 1 or tcol.min() < 0 or tcol.max() >= self.nspec * self.maxbins:
            raise ValueError("Gaussianised Blackwell-Rao: tcol must lie in [0, nspec * maxbins)")
        self.tcol = torch.from_numpy(tcol).to(dev).contiguous()
        self.glo, self.gh, self.tx, self.tp, self.mu, self.chol, self._mass = (
            torch.as_tensor(v, dtype=f64).to(dev).contiguous() for v in (glo, gh, tx, tp, mu, chol, mass))
        self.G = int(self.tx.shape[1])
        if tuple(self.tx.shape) != (self.Jg, self.G, 2) or tuple(self.tp.shape) != (self.Jg, self.G, 2) or \
                tuple(self.chol.shape) != (self.Jg, self.Jg) or tuple(self.mu.shape) != (self.Jg,) or \
                tuple(self.glo.shape) != (self.Jg,) or tuple(self.gh.shape) != (self.Jg,):
            raise ValueError("Gaussianised Blackwell-Rao: tables must be tx, tp [Jg, G, 2], glo, gh, mu [Jg] and chol "
                             "[Jg, Jg]")
        self.logdet, self.n = float(logdet), int(n)
        self.mass = self._mass.cpu().numpy()

    def loglike_t(self, theory):
        """Device tensors loglike [K], marginal [K] (sum_j log p_j) and outside [K]
        (columns whose D lies off the usable interval; loglike is -inf there), n
        and mass [Jg], of theory [K, nspec, maxbins] on this object's device: no
        host round trip.  x and log p come from gs_gbr_eval; the triangular solve
        and the norms go through torch."""
        if not torch.is_tensor(theory) or theory.dim() != 3 or tuple(theory.shape[1:]) != (self.nspec, self.maxbins) \
                or theory.shape[0] < 1 or theory.device != self.device:
            raise ValueError("Gaussianised Blackwell-Rao: theory must be a tensor [K, nspec, maxbins] = "
                             f"[K, {self.nspec}, {self.maxbins}] on the likelihood's device")
        th = theory.detach().to(torch.float64).contiguous()
        K = int(th.shape[0])
        dev, f64 = self.device, torch.float64
        x = torch.empty(K, self.Jg, dtype=f64, device=dev)
        lp = torch.empty(K, self.Jg, dtype=f64, device=dev)
        out = torch.empty(K, self.Jg, dtype=torch.int32, device=dev)
        C.check(self.lib.gs_gbr_eval(C.ptr(th), K, self.nspec, self.maxbins, self.Jg, C.ptr(self.tcol), C.ptr(self.tx),
                                     C.ptr(self.tp), C.ptr(self.glo), C.ptr(self.gh), self.G, C.ptr(x), C.ptr(lp),
                                     C.ptr(out), C.stream_ptr()), "gs_gbr_eval")
        outside = out.sum(dim=1)
        marginal = lp.sum(dim=1)
        z = torch.linalg.solve_triangular(self.chol, (x - self.mu).T.contiguous(), upper=False).T.contiguous()
        corr = 0.5 * ((x * x).sum(dim=1) - (z * z).sum(dim=1)) - 0.5 * self.logdet
        ll = torch.where(outside > 0, torch.full_like(marginal, float("-inf")), marginal + corr)
        return {"loglike": ll, "marginal": marginal, "outside": outside, "n": self.n, "mass": self._mass}

    def loglike(self, theory):
        """loglike_t of K theory spectra given as BlackwellRaoSamples.loglike takes
        them, numpy: {loglike [K], marginal [K], outside [K], n, mass [Jg]}.  For a TEB
        run a dict theory may leave TE out; TE values that are given are not read."""
        from .samplers import _br_theory_array, _br_theory_values
        name = "Gaussianised Blackwell-Rao"
        if self.nfields == 3 and isinstance(theory, dict) and "TE" not in theory:
            theory = dict(theory, TE=np.zeros_like(np.atleast_2d(np.asarray(theory["TT"], dtype=np.float64))))
        th = _br_theory_array(name, theory, SPECTRA[self.nfields], self.bins, self.nspec, self.maxbins)
        if self.nfields == 3:
            th[:, 3] = 0.0                  # TE is marginalised: its theory values are ignored
        _br_theory_values(name, th, self.mask, self.nfields)
        out = self.loglike_t(torch.from_numpy(np.ascontiguousarray(th)).to(self.device))
        return {"loglike": out["loglike"].cpu().numpy(), "marginal": out["marginal"].cpu().numpy(),
                "outside": out["outside"].cpu().numpy(), "n": self.n, "mass": self.mass.copy()}

    def save(self, path):
        """Write the tables, mu and the factor to an .npz file (numeric arrays only)."""
        np.savez(path, nfields=np.int64(self.nfields), mask=self.mask, tcol=self.tcol.cpu().numpy(),
                 glo=self.glo.cpu().numpy(), gh=self.gh.cpu().numpy(), tx=self.tx.cpu().numpy(),
                 tp=self.tp.cpu().numpy(), mu=self.mu.cpu().numpy(), chol=self.chol.cpu().numpy(),
                 logdet=np.float64(self.logdet), n=np.int64(self.n), mass=self.mass,
                 **{"bins_" + s: b for s, b in self.bins.items()})

    @classmethod
    def load(cls, path, device=None):
        """The likelihood of a save()d file."""
        with np.load(path, allow_pickle=False) as f:
            F = int(f["nfields"])
            bins = {s: f["bins_" + s] for s in SPECTRA[F]}
            return cls(F, bins, f["mask"], f["tcol"], f["glo"], f["gh"], f["tx"], f["tp"], f["mu"], f["chol"],
                       float(f["logdet"]), int(f["n"]), f["mass"], device=device)


class _BankLoglike(torch.autograd.Function):
    """BlackwellRaoSamples.loglike_torch: forward runs loglike_grad_t once and keeps
    a copy of grad; backward scales its rows.  once_differentiable: a second
    backward raises."""

    @staticmethod
    def forward(ctx, theory, bank):
        if not ctx.needs_input_grad[0]:
            return bank.loglike_t(theory)["loglike"].clone()
        out = bank.loglike_grad_t(theory)
        ctx.save_for_backward(out["grad"].clone())
        ctx.dtype = theory.dtype
        return out["loglike"].clone()

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out.requires_grad or torch.is_grad_enabled():
            raise RuntimeError("Blackwell-Rao sample bank: loglike_torch is differentiable once; the second derivatives "
                               "are loglike_hess(theory)['hess']")
        grad, = ctx.saved_tensors
        return (grad_out.to(grad.dtype)[:, None, None] * grad).to(ctx.dtype), None


def stats_layout(F):
    """Names of the statistic rows (include/gibbs_capi.h GS_NSTAT_*)."""
    return {1: ["ssTT", "dTsT"], 2: ["ssEE", "ssBB", "dEsE", "dBsB"],
            3: ["ssTT", "ssEE", "ssBB", "ssTE", "dTsT", "dEsT", "dEsE", "dBsB"]}[F]

