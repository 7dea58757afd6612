"""Batched full-sky Gibbs drivers on the device (the loops of the reference drivers).

``BatchedRunner`` runs ``nchains`` chains of one of the three samplers in
lock-step on one GPU:

  * ``centered``    GibbsSampler.run_polarization (GibbsSampler.py:118-180): an
                    initial CR (ula=True, GibbsSampler.py:41,136-138), then per
                    iteration CR (closed form, CenteredGibbs.py:317-353 -- the
                    exact full-sky limit of the PCG branch) + inverse-Gamma /
                    inverse-Wishart C_l draw.  History includes the start.
  * ``noncentered`` NonCenteredGibbs.run_polarization (NonCenteredGibbs.py:529-571),
                    all_sph: non-centered CR + MH blocks.  History includes the start.
  * ``asis``        ASIS.run_polarization (ASIS.py:134-226): centered CR, centered
                    C_l draw, non-centering, NC MH, re-centring.  History
                    excludes the start (ASIS.py:150-206).

Everything stays in HBM; only the returned histories are copied back.
"""
import contextlib
import gc
import time

import numpy as np
import torch

from . import _capi as C
from .engine import BlackwellRaoLikelihood, BlackwellRaoSamples, BlackwellRaoState, GibbsPlan, MH_ORDER, SummaryState, \
    WienerPosterior

INIT_ITER = 0xFFFFFFFF
ADAPT_KAPPA = 0.6       # Robbins-Monro step n^-kappa of the warm-up adaptation


def check_warmup(kind, rng, n_warmup, target_accept=0.25):
    """Argument check of run(n_warmup=...): the warm-up adapts the NC Metropolis
    proposal scales, which only the native NC / ASIS samplers have."""
    n_warmup = int(n_warmup)
    if n_warmup < 0:
        raise ValueError("n_warmup must be >= 0")
    if n_warmup > 0:
        if kind == "centered":
            raise ValueError("n_warmup > 0: the centered sampler has no Metropolis step to adapt")
        if rng != "native":
            raise ValueError("n_warmup > 0 needs rng='native' (a replayed run reproduces the reference's "
                             "fixed proposal scales)")
        if not 0.0 < float(target_accept) < 1.0:
            raise ValueError("target_accept must lie in (0, 1)")
    return n_warmup


def check_summary(summary, keep_history=True):
    """run(summary=...): None / False (off), True, or {max_lag: 32, start: None};
    returns None or (max_lag, start)."""
    if summary is None or summary is False:
        if not keep_history:
            raise ValueError("keep_history=False needs summary= (nothing else would be kept of the run)")
        return None
    opts = {} if summary is True else dict(summary)
    bad = set(opts) - {"max_lag", "start"}
    if bad:
        raise ValueError(f"summary: unknown options {sorted(bad)}")
    max_lag = int(opts.get("max_lag", 32))
    if not 0 <= max_lag <= 64:
        raise ValueError("summary: max_lag must lie in [0, 64]")
    start = opts.get("start")
    if start is not None and int(start) < 0:
        raise ValueError("summary: start must be >= 0")
    return max_lag, None if start is None else int(start)


def check_skymap_summary(opt):
    """run(skymap_summary=...) of the masked drivers: None / False (off), True,
    or {start: None, pixels: False, every: 1}; returns None or the dict
    {start, pixels, every} (start None -> 0: every iteration is summarised)."""
    if opt is None or opt is False:
        return None
    opts = {} if opt is True else dict(opt)
    bad = set(opts) - {"start", "pixels", "every"}
    if bad:
        raise ValueError(f"skymap_summary: unknown options {sorted(bad)}")
    start = opts.get("start")
    start = 0 if start is None else int(start)
    if start < 0:
        raise ValueError("skymap_summary: start must be >= 0")
    every = int(opts.get("every", 1))
    if every < 1:
        raise ValueError("skymap_summary: every must be >= 1")
    return {"start": start, "pixels": bool(opts.get("pixels", False)), "every": every}


def check_wiener_posterior(opt):
    """run(wiener_posterior=...): None / False (off), True or {start: None};
    returns None or {"start": int or None} (None: the iteration the warm-up
    ends at, as the summary's)."""
    if opt is None or opt is False:
        return None
    opts = {} if opt is True else dict(opt)
    bad = set(opts) - {"start"}
    if bad:
        raise ValueError(f"wiener_posterior: unknown options {sorted(bad)}")
    start = opts.get("start")
    if start is not None and int(start) < 0:
        raise ValueError("wiener_posterior: start must be >= 0")
    return {"start": None if start is None else int(start)}


def check_blackwell_rao(br, nfields, bins, dls_init=None, maxbins=None):
    """run(blackwell_rao=...): None / False (off), {"grid": array [nspec, maxbins,
    G]} or {"points": G, "span": (lo, hi)} (a geometric grid dls_init[bin] * lo
    ... * hi per bin), either with an optional "start" (as the summary's).
    Returns None or {grid, alpha, half_mask, start}; grid is None when the
    points form is given without dls_init (the constructors' early check)."""
    from .engine import SPECTRA, br_shapes
    if br is None or br is False:
        return None
    if not isinstance(br, dict):
        raise ValueError("blackwell_rao: a dict {grid} or {points, span} is needed")
    bad = set(br) - {"grid", "points", "span", "start"}
    if bad:
        raise ValueError(f"blackwell_rao: unknown options {sorted(bad)}")
    if ("grid" in br) == ("points" in br):
        raise ValueError("blackwell_rao: give either grid or points (with span)")
    start = br.get("start")
    if start is not None and int(start) < 0:
        raise ValueError("blackwell_rao: start must be >= 0")
    spectra = SPECTRA[int(nfields)]
    alpha, half = br_shapes(nfields, bins, maxbins)
    nspec, maxbins = alpha.shape
    used = ~np.isnan(alpha)
    if "grid" in br:
        if "span" in br:
            raise ValueError("blackwell_rao: span belongs to the points form")
        grid = np.array(br["grid"], dtype=np.float64)
        if grid.ndim != 3 or grid.shape[:2] != (nspec, maxbins):
            raise ValueError(f"blackwell_rao: grid must be [nspec, maxbins, G] = [{nspec}, {maxbins}, G]")
        G = grid.shape[2]
        if not 1 <= G <= 64:
            raise ValueError("blackwell_rao: the grid points G must lie in [1, 64]")
        g = grid[used]
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise ValueError("blackwell_rao: grid values must be positive and finite")
        if G > 1 and not np.all(np.diff(g, axis=1) > 0):
            raise ValueError("blackwell_rao: grid values must increase along the last axis")
        grid[~used] = 1.0
    else:
        G = int(br["points"])
        if not 1 <= G <= 64:
            raise ValueError("blackwell_rao: points G must lie in [1, 64]")
        lo, hi = (float(v) for v in br.get("span", (0.25, 4.0)))
        if not (0.0 < lo <= hi and np.isfinite(hi)) or (G > 1 and lo == hi):
            raise ValueError("blackwell_rao: span must be (lo, hi) with 0 < lo < hi")
        grid = None
        if dls_init is not None:
            d0 = dls_init[0] if isinstance(dls_init, (list, tuple)) else dls_init
            grid = np.ones((nspec, maxbins, G))
            fac = np.geomspace(lo, hi, G)
            for k, s in enumerate(spectra):
                v = np.asarray(d0[s], dtype=np.float64)
                u = used[k, :len(v)]
                if not (np.all(np.isfinite(v[u])) and np.all(v[u] > 0)):
                    raise ValueError(f"blackwell_rao: dls_init[{s}] must be positive on the drawn bins to centre "
                                     "a grid on it (give grid= instead)")
                grid[k, :len(v)][u] = v[u, None] * fac
    return {"grid": grid, "alpha": alpha, "half_mask": half, "start": None if start is None else int(start)}


def _br_theory_array(name, th, spectra, bins, nspec, maxbins):
    """theory {spectrum: [K, nbins]} or [K, nspec, maxbins] -> fp64 [K, nspec, maxbins]."""
    if isinstance(th, dict):
        if set(th) != set(spectra):
            raise ValueError(f"{name}: theory needs the spectra {list(spectra)}")
        rows = [np.atleast_2d(np.asarray(th[s], dtype=np.float64)) for s in spectra]
        K = rows[0].shape[0]
        theory = np.ones((K, nspec, maxbins))
        for k, (s, v) in enumerate(zip(spectra, rows)):
            nb = len(bins[s]) - 1
            if v.ndim != 2 or v.shape != (K, nb):
                raise ValueError(f"{name}: theory[{s}] must be [K, nbins] = [{K}, {nb}]")
            theory[:, k, :nb] = v
    else:
        theory = np.array(th, dtype=np.float64)
        if theory.ndim != 3 or theory.shape[1:] != (nspec, maxbins):
            raise ValueError(f"{name}: theory must be [K, nspec, maxbins] = [K, {nspec}, {maxbins}]")
    if theory.shape[0] < 1:
        raise ValueError(f"{name}: at least one theory spectrum (K >= 1) is needed")
    return theory


def _br_used_mask(name, opts, F, spectra, bins, drawn):
    """The used bins of the options' lrange or mask (default: every drawn bin)."""
    from .engine import br_likelihood_mask
    nspec, maxbins = drawn.shape
    if "mask" in opts:
        mk = opts["mask"]
        if isinstance(mk, dict):
            mask = np.zeros((nspec, maxbins), dtype=bool)
            for k, s in enumerate(spectra):
                v = np.asarray(mk[s], dtype=bool)
                mask[k, :len(v)] = v
        else:
            mask = np.array(mk, dtype=bool)
            if mask.shape != (nspec, maxbins):
                raise ValueError(f"{name}: mask must be [nspec, maxbins] = [{nspec}, {maxbins}]")
        mask &= drawn
    else:
        lr = opts.get("lrange")
        if lr is not None and not (len(lr) == 2 and lr[0] <= lr[1]):
            raise ValueError(f"{name}: lrange must be (lmin, lmax) with lmin <= lmax")
        mask = br_likelihood_mask(F, bins, maxbins, lr)
    if F == 3 and not (np.array_equal(mask[0], mask[1]) and np.array_equal(mask[0], mask[3])):
        raise ValueError(f"{name}: the TEB block is used as a whole: the mask of TT, EE and TE must agree")
    if not mask.any():
        raise ValueError(f"{name}: no bin is used (empty used set)")
    return mask


def _br_theory_values(name, theory, mask, F):
    """A theory on the used bins: finite; positive but for TE; TEB blocks positive definite."""
    pos = mask.copy()                       # every used spectrum but TE is a variance
    if F == 3:
        pos[3] = False
    tp = theory[:, pos]
    if not (np.all(np.isfinite(theory[:, mask])) and np.all(tp > 0)):
        raise ValueError(f"{name}: theory values must be finite, and positive but for TE, on the used bins")
    if F == 3:
        m0 = mask[0]
        det = theory[:, 0, m0] * theory[:, 1, m0] - theory[:, 3, m0] ** 2
        if not np.all(det > 0):
            raise ValueError(f"{name}: a used TEB block of the theory must be positive definite "
                             "(det = TT EE - TE^2 > 0)")


def check_br_likelihood(opts, nfields, bins, maxbins=None):
    """run(br_likelihood=...): None / False (off) or {"theory": {spectrum: [K,
    nbins]} or an array [K, nspec, maxbins], "lrange": (lmin, lmax) or "mask":
    bool [nspec, maxbins] or {spectrum: [nbins]} (default: every drawn bin),
    "start": as the summary's}.  Returns None or {tables, mask, K, start}
    (tables: engine.br_likelihood_tables)."""
    from .engine import SPECTRA, br_likelihood_mask, br_likelihood_tables
    if opts is None or opts is False:
        return None
    if not isinstance(opts, dict) or "theory" not in opts:
        raise ValueError("br_likelihood: a dict {theory[, lrange | mask][, start]} is needed")
    bad = set(opts) - {"theory", "lrange", "mask", "start"}
    if bad:
        raise ValueError(f"br_likelihood: unknown options {sorted(bad)}")
    if "lrange" in opts and "mask" in opts:
        raise ValueError("br_likelihood: give either lrange or mask")
    start = opts.get("start")
    if start is not None and int(start) < 0:
        raise ValueError("br_likelihood: start must be >= 0")
    F = int(nfields)
    spectra = SPECTRA[F]
    drawn = br_likelihood_mask(F, bins, maxbins)
    nspec, maxbins = drawn.shape
    theory = _br_theory_array("br_likelihood", opts["theory"], spectra, bins, nspec, maxbins)
    mask = _br_used_mask("br_likelihood", opts, F, spectra, bins, drawn)
    _br_theory_values("br_likelihood", theory, mask, F)
    return {"tables": br_likelihood_tables(F, bins, theory, mask), "mask": mask, "K": theory.shape[0],
            "start": None if start is None else int(start)}


def check_br_samples(opts, nfields, bins, maxbins=None):
    """run(br_samples=...): None / False (off), True or {"lrange": (lmin, lmax) or
    "mask": bool [nspec, maxbins] or {spectrum: [nbins]} (default: every drawn
    bin), "start": as the summary's, "draws": bool (default False: keep the D_l
    draws beside the scales, what bank.gaussianize needs)} -- the bins whose
    scales the sample bank keeps.  Returns None or {mask, start, draws}."""
    from .engine import SPECTRA, br_likelihood_mask
    if opts is None or opts is False:
        return None
    if opts is True:
        opts = {}
    if not isinstance(opts, dict):
        raise ValueError("br_samples: True or a dict {[lrange | mask][, start]} is needed")
    bad = set(opts) - {"lrange", "mask", "start", "draws"}
    if bad:
        raise ValueError(f"br_samples: unknown options {sorted(bad)}")
    if not isinstance(opts.get("draws", False), (bool, np.bool_)):
        raise ValueError("br_samples: draws must be True or False")
    if "lrange" in opts and "mask" in opts:
        raise ValueError("br_samples: give either lrange or mask")
    start = opts.get("start")
    if start is not None and int(start) < 0:
        raise ValueError("br_samples: start must be >= 0")
    F = int(nfields)
    drawn = br_likelihood_mask(F, bins, maxbins)
    mask = _br_used_mask("br_samples", opts, F, SPECTRA[F], bins, drawn)
    return {"mask": mask, "start": None if start is None else int(start), "draws": bool(opts.get("draws", False))}


def br_theory(name, theory, nfields, bins, mask):
    """A theory {spectrum: [K, nbins]} or [K, nspec, maxbins] as fp64 [K, nspec,
    maxbins], checked on the used bins `mask` with check_br_likelihood's rules."""
    from .engine import SPECTRA
    F = int(nfields)
    mask = np.asarray(mask, dtype=bool)
    theory = _br_theory_array(name, theory, SPECTRA[F], bins, mask.shape[0], mask.shape[1])
    _br_theory_values(name, theory, mask, F)
    return theory


def warmup_of_state(st):
    """(n_warmup, target_accept, log_scale, count) of a state_dict(); states
    written before the adaptation existed (no such keys) are 'not adapting'."""
    if st.get("mh_log_scale") is None:
        return 0, 0.25, None, None
    return int(st.get("mh_n_warmup", 0)), float(st.get("mh_target_accept", 0.25)), st["mh_log_scale"], \
        st.get("mh_count")


def tuned_variances(proposal_variances, blocks, bins, layout, log_scale_mean):
    """sd0^2 exp(2 lam) per spectrum and bin >= 2 (the form proposal_variances=
    takes): layout [(spectrum, first block, blocks)] of log_scale_mean."""
    out = {}
    for s, off, nb in layout:
        pv = np.array(proposal_variances[s], dtype=np.float64)
        nbins = len(bins[s]) - 1
        edges = np.clip(np.asarray(blocks[s], dtype=np.int64), 0, nbins)
        for k in range(nb):
            lo, hi = max(int(edges[k]), 2), int(edges[k + 1])
            if hi > lo:
                pv[lo - 2:hi - 2] *= np.exp(2.0 * float(log_scale_mean[off + k]))
        out[s] = pv
    return out


@contextlib.contextmanager
def _capture(g):
    """torch.cuda.graph(g), capture-safe for other objects' teardown:
    - the cyclic collector is paused from before the capture opens until after
      it has closed (torch.cuda.graph's own gc.collect() in __enter__ still runs:
      an explicit collect ignores gc.disable);
    - any destructor that does run inside (a plain refcount drop in the
      captured code, or an explicit gc.collect()) parks its device resources
      in _capi's graveyard instead of calling HIP; they are released after the
      capture (_capi.end_capture)."""
    was = gc.isenabled()
    gc.disable()
    C.begin_capture()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        C.end_capture()
        if was:
            gc.enable()


class BatchedRunner:
    def __init__(self, kind, lmax, nside, nfields, nchains, bl, noise_var, bins, d_alm, blocks=None,
                 proposal_variances=None, rng="native", seed=0, chain0=0, quirks=1, n_iter_metropolis=1,
                 materialize_recentre=False, store_skymap=True):
        if kind not in ("centered", "noncentered", "asis"):
            raise ValueError(kind)
        if rng not in ("native", "replay"):
            raise ValueError(rng)
        self.kind, self.rng, self.seed = kind, rng, int(seed)
        self.quirks = int(quirks)
        self.plan = GibbsPlan(lmax, nside, nfields, nchains, bl, noise_var, bins, blocks=blocks,
                              proposal_variances=proposal_variances, chain0=chain0, quirks=quirks,
                              n_iter_metropolis=n_iter_metropolis)
        p = self.plan
        self.d = p.data_tensor(d_alm)
        if kind == "noncentered" and rng == "native":
            p.data_moments(self.d)
        self.s = p.zeros(p.nchains, p.F, p.NR) if store_skymap else None
        self.dl = None
        self.dl_tmp = p.zeros(p.nchains, p.nspec, p.maxbins)
        self.accept = p.zeros(p.nchains, max(p.nacc, 1), dtype=torch.int32)
        self.materialize_recentre = materialize_recentre
        self.iteration = 0
        self.graph = None
        # warm-up adaptation of the MH proposal scales: iterations 1 .. n_warmup adapt
        self.n_warmup = 0
        self.target_accept = 0.25
        self._gather = None
        # streaming summary of the D_l chains (run(summary=...)): the device state
        # and the iteration after which it summarises
        self._summary = None
        self.summary_start = 0
        # streaming Blackwell-Rao posteriors (run(blackwell_rao=...)): the device
        # state, the iteration after which it accumulates, and the scale history
        # of run(keep_scales=True)
        self._br = None
        self.br_start = 0
        self.h_scales = None
        # streaming Blackwell-Rao likelihood of theory spectra (run(br_likelihood=...)):
        # the device state with its tables and the iteration after which it accumulates
        self._brl = None
        self.brl_start = 0
        # Blackwell-Rao sample bank (run(br_samples=...)): the kept samples' used
        # scales on the device and the iteration after which they are kept
        self._brs = None
        self.brs_start = 0
        # Rao-Blackwellised posterior sky map (run(wiener_posterior=...)): the
        # device state and the iteration after which it accumulates
        self._wf = None
        self.wf_start = 0

    def __del__(self):
        # dropped inside another sampler's capture: keep the kept hipGraphs, the
        # copy stream and the tensors alive until that capture has ended
        # (their destructors call HIP, which is illegal while a capture is open)
        try:
            C.park(dict(self.__dict__))
        except Exception:
            pass

    # -- one iteration ---------------------------------------------------------------
    def _replay(self):
        p = self.plan
        z = p.replay_cr_normals()
        ig = up = ua = None
        if self.kind in ("centered", "asis"):
            ig = p.replay_invgamma()
        if self.kind in ("noncentered", "asis"):
            up, ua = p.replay_mh_uniforms()
        return z, ig, up, ua

    def init(self, dls_init):
        p = self.plan
        if self.dl is None:
            self.dl = p.dl_tensor(dls_init)
        else:
            # keep the buffer a captured graph points at; a re-init drops the graph
            # (its device iteration counter belongs to the previous run)
            self.dl.copy_(p.dl_tensor(dls_init))
        self.graph = None
        p.iteration_counter(False)
        self.iteration = 0
        if self.kind == "centered":
            # the reference's initial CR (GibbsSampler.py:136-138) -- consumes its draws
            z = p.replay_cr_normals() if self.rng == "replay" else None
            params = p.block_params(0, self.dl)
            p.cr_sweep(self.d, params, z=z, seed=self.seed, iteration=INIT_ITER, s_out=self.s,
                       store=self.s is not None)

    # -- checkpoint / resume -----------------------------------------------------------
    def state_dict(self):
        """The chains' whole state between iterations, as host tensors and plain
        values (``torch.save`` / ``torch.load(weights_only=True)`` round-trip it):
        D_l, the last accept flags, ASIS's D_l before the MH, the sky map when
        stored, and the iteration count.  The native streams are counter-based
        (seed, chain id, iteration), so a restored runner continues the same
        trajectory bit for bit.  Replay runs draw from numpy's global RNG: its
        state is saved too (``numpy_rng_*``) and restored by load_state_dict."""
        if self.dl is None:
            raise RuntimeError("state_dict: the runner has not been initialised (run() or init() first)")
        p = self.plan
        st = {"kind": self.kind, "rng": self.rng, "seed": self.seed, "iteration": int(self.iteration),
              "chain0": p.chain0, "nchains": p.nchains, "lmax": p.L, "nfields": p.F,
              "dl": self.dl.cpu().clone(), "dl_tmp": self.dl_tmp.cpu().clone(), "accept": self.accept.cpu().clone(),
              "s": None if self.s is None else self.s.cpu().clone()}
        if p.adapting:
            # the proposal log-scales, their step counts and where the warm-up ends
            lam, cnt = p.mh_scale_get()
            st.update(mh_log_scale=lam.cpu(), mh_count=cnt.cpu(), mh_n_warmup=int(self.n_warmup),
                      mh_target_accept=float(self.target_accept))
        if self._summary is not None:
            st.update(summary_state=self._summary.data.cpu().clone(), summary_max_lag=self._summary.max_lag,
                      summary_start=int(self.summary_start))
        if self._br is not None:
            br = self._br
            st.update(br_state=br.data.cpu().clone(), br_grid=br.grid.cpu().clone(), br_alpha=br.alpha.cpu().clone(),
                      br_half_mask=int(br.half_mask), br_start=int(self.br_start))
        if self._brl is not None:
            bl = self._brl
            st.update(brl_state=bl.data.cpu().clone(), brl_start=int(self.brl_start),
                      **{"brl_" + k: v for k, v in bl.tables().items()})
        if self._brs is not None:
            st.update(brs_start=int(self.brs_start), **{"brs_" + k: v for k, v in self._brs.state().items()})
        if self._wf is not None:
            st.update(wf_state=self._wf.data.cpu().clone(), wf_start=int(self.wf_start))
        if self.rng == "replay":
            name, keys, pos, has_gauss, cached = np.random.get_state()
            st.update(numpy_rng_keys=torch.from_numpy(np.asarray(keys, dtype=np.int64)), numpy_rng_pos=int(pos),
                      numpy_rng_has_gauss=int(has_gauss), numpy_rng_cached=float(cached))
        return st

    def load_state_dict(self, st):
        """Restore a state_dict() (same kind, chains, l_max, fields and RNG mode);
        the device buffers are kept (a kept graph still points at them)."""
        p = self.plan
        want = {"kind": self.kind, "rng": self.rng, "chain0": p.chain0, "nchains": p.nchains, "lmax": p.L,
                "nfields": p.F}
        bad = {k: (st.get(k), v) for k, v in want.items() if st.get(k) != v}
        if bad:
            raise ValueError(f"load_state_dict: state does not match this runner: {bad}")
        dl = st["dl"].to(self.dl_tmp.device)
        if self.dl is None:
            self.dl = dl.clone()
        else:
            self.dl.copy_(dl)
        self.dl_tmp.copy_(st["dl_tmp"])
        self.accept.copy_(st["accept"])
        if self.s is not None and st.get("s") is not None:
            self.s.copy_(st["s"])
        if int(st["seed"]) != self.seed:
            # the kept chunk graphs of run() hold the old seed as a kernel
            # argument: drop them, so the resumed run captures with the new one
            self.__dict__.pop("_run_graphs", None)
        self.seed = int(st["seed"])
        self.iteration = int(st["iteration"])
        self.graph = None
        p.iteration_counter(False)
        nw, target, lam, cnt = warmup_of_state(st)
        if lam is not None:
            self._adapt_enable(target)
            p.mh_scale_set(lam, cnt)
        # a state without scales (older checkpoints) is "not adapting": no warm-up
        # is left, and the plan's proposal table stays as it is
        self.n_warmup = nw
        # a state without a summary (older checkpoints included) is "no summary"
        if st.get("summary_state") is not None:
            self._summary_alloc(int(st["summary_max_lag"]), data=st["summary_state"])
            self.summary_start = int(st["summary_start"])
        else:
            self._summary = None
        # likewise a state without Blackwell-Rao keys is "off"
        if st.get("br_state") is not None:
            self._br = BlackwellRaoState(p.nchains, st["br_grid"], st["br_alpha"], int(st["br_half_mask"]),
                                         device=p.device, data=st["br_state"])
            self.br_start = int(st["br_start"])
        else:
            self._br = None
        # and one without the likelihood's keys
        if st.get("brl_state") is not None:
            self._brl = BlackwellRaoLikelihood(p.nchains, p.nspec, p.maxbins,
                                               {k: st["brl_" + k] for k in BlackwellRaoLikelihood.TABLES},
                                               device=p.device, data=st["brl_state"])
            self.brl_start = int(st["brl_start"])
        else:
            self._brl = None
        # and one without the sample bank's keys
        if st.get("brs_X") is not None:
            self._brs = BlackwellRaoSamples.from_state({k: st["brs_" + k] for k in ("X", "r", "mask", "Dl")
                                                        if st.get("brs_" + k) is not None}, p.F, p.bins,
                                                       device=p.device)
            self.brs_start = int(st["brs_start"])
        else:
            self._brs = None
        # and one without the posterior sky map's
        if st.get("wf_state") is not None:
            self._wf_alloc(data=st["wf_state"])
            self.wf_start = int(st["wf_start"])
        else:
            self._wf = None
        if self.rng == "replay" and "numpy_rng_keys" in st:
            np.random.set_state(("MT19937", st["numpy_rng_keys"].numpy().astype(np.uint32), st["numpy_rng_pos"],
                                 st["numpy_rng_has_gauss"], st["numpy_rng_cached"]))

    # -- hipGraph: capture one whole iteration, replay it per step ------------------
    def capture_graph(self, trace=None, trace_capacity=None):
        """Capture one iteration (plus an optional device-side trace record) in a
        hipGraph; subsequent ``step()`` calls replay it.  Native RNG only: the
        iteration counter lives on the device and advances inside the graph."""
        if self.rng != "native":
            raise ValueError("graph capture needs the native (counter-based) RNG")
        p = self.plan
        p.iteration_counter(True, self.iteration + 1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _capture(g):
            if self.kind == "noncentered":
                # NC: prologue, sweep (+ statistics), MH decisions with the trace record
                # and the counter advance fused into the decision launch
                p.nc_prologue(self.dl, seed=self.seed)
                p.nc_sweep(self.d, self.dl, self.s, seed=self.seed)
                p.nc_decide_fused(self.dl, seed=self.seed, accept=self.accept, trace=trace,
                                  capacity=trace_capacity or 0)
            elif self.kind == "centered":
                # centered: the trace record and the counter advance ride in the C_l draw
                p.step_centered_fused(self.d, self.dl, self.s, seed=self.seed, trace=trace,
                                      capacity=trace_capacity or 0)
            else:
                # ASIS: the trace record and the counter advance ride in the MH launch
                p.step_asis_fused(self.d, self.dl, self.s, seed=self.seed, accept=self.accept, dl_tmp=self.dl_tmp,
                                  recentre=self.materialize_recentre, trace=trace, capacity=trace_capacity or 0)
        self.graph = g
        self.graph_steps = 1
        return g

    def _adapt_enable(self, target):
        """Per-chain proposal table on (or a new target): graphs captured before
        hold the old table / target as kernel arguments and are dropped."""
        p = self.plan
        if p.adapting and float(target) == self.target_accept:
            return
        p.mh_adapt_enable(target, ADAPT_KAPPA)
        self.target_accept = float(target)
        self.__dict__.pop("_run_graphs", None)
        self.graph = None

    def tuned_proposal_variances(self, gather=None):
        """Per spectrum the [nbins-2] variances sd0^2 exp(2 mean_chains(log-scale)),
        i.e. the geometric mean of the chains' scales, in the form
        ``proposal_variances=`` accepts (a preliminary run's output for the
        production run).  gather: ShardContext.gather -- the mean is over every
        rank's chains (default: the gather of the last run())."""
        p = self.plan
        if not p.adapting:
            return {s: np.array(v, dtype=np.float64) for s, v in p.proposal_variances.items()}
        lam, _ = p.mh_scale_get()
        gather = gather if gather is not None else self._gather
        if gather is not None:
            lam = gather(lam, dim=0)
        return tuned_variances(p.proposal_variances, p.blocks, p.bins, p.mh_block_layout(),
                               lam.mean(dim=0).cpu().numpy())

    # -- streaming summary ---------------------------------------------------------------
    def _summary_alloc(self, max_lag, data=None):
        """The summary state for max_lag (kept across runs of the same max_lag and
        zeroed; replaced otherwise), or the restored state `data`."""
        p, sm = self.plan, self._summary
        if data is not None:
            self._summary = SummaryState(p.nchains, p.nspec, p.maxbins, max(p.nacc, 1), max_lag, device=p.device,
                                         data=data)
        elif sm is not None and sm.max_lag == max_lag:
            sm.reset()
        else:
            self._summary = SummaryState(p.nchains, p.nspec, p.maxbins, max(p.nacc, 1), max_lag, device=p.device)

    def _summary_update(self, trace, capacity, it0, k, acc=None, acc_stride=0):
        """Summarise iterations it0 + 1 .. it0 + k (in the trace ring; step i's
        flags at acc[i]) except those up to summary_start."""
        first = max(it0, self.summary_start) + 1
        n = it0 + k - first + 1
        if n <= 0:
            return
        if acc is not None and self.kind != "centered":
            acc = acc[first - it0 - 1:] if acc_stride else acc
        else:
            acc = None
        self._summary.update(trace, capacity, first, n, accept=acc, accept_stride=acc_stride)

    def summary(self, gather=None):
        """The posterior summary of the last run(summary=...): per spectrum a dict
        of numpy arrays -- mean, var, min, max, ess, ess_truncated, rhat [nbins],
        chain_mean, chain_var [chains, nbins], acf [max_lag + 1, nbins] -- and
        n, the samples per chain.  gather (ShardContext.gather; default: the
        gather of the last run()): the per-chain state is all-gathered along the
        chain axis and the statistics are over every rank's chains."""
        if self._summary is None:
            raise RuntimeError("summary: the last run() kept no summary (run(summary=True))")
        p = self.plan
        out = self._summary.finish(gather if gather is not None else self._gather)
        n = out.pop("n")
        out.pop("gamma")
        host = {k: v.cpu().numpy() for k, v in out.items()}
        res = {}
        for i, s in enumerate(p.spectra):
            nb = len(p.bins[s]) - 1
            res[s] = {k: v[..., i, :nb].copy() for k, v in host.items()}
            res[s]["ess_truncated"] = res[s]["ess_truncated"] != 0
            res[s]["n"] = n
        return res

    # -- streaming Blackwell-Rao posteriors -----------------------------------------------
    def _br_update(self, scales, capacity, it0, k):
        """Accumulate iterations it0 + 1 .. it0 + k (in the scale ring) except
        those up to br_start."""
        first = max(it0, self.br_start) + 1
        n = it0 + k - first + 1
        if n > 0:
            self._br.update(scales, capacity, first, n)

    def blackwell_rao(self, gather=None):
        """The Blackwell-Rao marginal posteriors of the last run(blackwell_rao=...):
        per spectrum a dict of numpy arrays -- grid, logpdf [nbins, G], mass,
        alpha [nbins] -- with n, the iterations per chain, and bad, the rows
        this rank's chains skipped for a non-positive or non-finite scale.
        logpdf is log P(D_b = grid | d); NaN where no one-dimensional
        conditional exists (TE, bins 0 and 1).  gather as in summary()."""
        if self._br is None:
            raise RuntimeError("blackwell_rao: the last run() kept no Blackwell-Rao state (run(blackwell_rao=...))")
        p, br = self.plan, self._br
        out = br.finish(gather if gather is not None else self._gather)
        lp, mass = out["logpdf"].cpu().numpy(), out["mass"].cpu().numpy()
        grid, alpha, bad = br.grid.cpu().numpy(), br.alpha.cpu().numpy(), br.bad().cpu().numpy()
        res = {}
        for i, s in enumerate(p.spectra):
            nb = len(p.bins[s]) - 1
            res[s] = {"grid": grid[i, :nb].copy(), "logpdf": lp[i, :nb].copy(), "mass": mass[i, :nb].copy(),
                      "alpha": alpha[i, :nb].copy(), "n": out["n"], "bad": int(bad[:, i].sum())}
        return res

    # -- streaming Blackwell-Rao likelihood -----------------------------------------------
    def _brl_update(self, scales, capacity, it0, k):
        """As _br_update, for the likelihood state and brl_start."""
        first = max(it0, self.brl_start) + 1
        n = it0 + k - first + 1
        if n > 0:
            self._brl.update(scales, capacity, first, n)

    def br_likelihood(self, gather=None):
        """The Blackwell-Rao likelihood of the theory spectra of the last
        run(br_likelihood=...), numpy: loglike [K] = log L(D^th_k | d) over all
        chains, chain_loglike [C, K] (each chain's own estimate), neff [K] (the
        effective number of samples that carry the estimate, in [1, C n]), n,
        the iterations per chain, and bad [chains of this rank], the rows
        skipped for a non-positive or non-finite scale.  gather as in summary()."""
        if self._brl is None:
            raise RuntimeError("br_likelihood: the last run() kept no likelihood state (run(br_likelihood=...))")
        out = self._brl.finish(gather if gather is not None else self._gather)
        res = {k: out[k].cpu().numpy() for k in ("loglike", "chain_loglike", "neff")}
        res.update(n=out["n"], bad=self._brl.bad().cpu().numpy().copy())
        return res

    # -- Blackwell-Rao sample bank ---------------------------------------------------------
    def _brs_append(self, scales, capacity, it0, k, trace=None):
        """As _br_update, for the sample bank and brs_start; trace: the D_l trace ring
        beside the scale ring (read only by a bank that keeps the draws)."""
        first = max(it0, self.brs_start) + 1
        n = it0 + k - first + 1
        if n > 0:
            self._brs.append(scales, capacity, first, n, trace if self._brs.draws else None)

    def br_samples(self):
        """The sample bank of the last run(br_samples=...) (engine.BlackwellRaoSamples:
        loglike(theory, gather), save(path))."""
        if self._brs is None:
            raise RuntimeError("br_samples: the last run() kept no sample bank (run(br_samples=...))")
        return self._brs

    # -- Rao-Blackwellised posterior sky map -------------------------------------------------
    def _wf_alloc(self, data=None):
        """The posterior sky map's state (kept across runs and zeroed), or the
        restored state `data`."""
        if data is None and self._wf is not None:
            self._wf.reset()
            return
        self._wf = WienerPosterior.from_plan(self.plan, data=data)
        self._wf.data_moments(self.d)

    def _wf_update(self, trace, capacity, it0, k):
        """As _br_update, on the D_l trace ring and wf_start."""
        first = max(it0, self.wf_start) + 1
        n = it0 + k - first + 1
        if n > 0:
            self._wf.update(trace, capacity, first, n)

    def wiener_posterior(self, gather=None):
        """The Rao-Blackwellised posterior sky map of the last
        run(wiener_posterior=...), numpy: alm_mean, alm_var, alm_rhat [F, (L+1)^2],
        chain_alm_mean [C, F, (L+1)^2], power_of_mean, mean_power [nspec, L+1]
        (TE included for TEB), op_mean [nop, L+1] (the posterior-averaged
        Wiener-filter operator: M00, M01, M10, M11, M22 for TEB, M_f otherwise)
        and n, the samples per chain.  gather as in summary()."""
        if self._wf is None:
            raise RuntimeError("wiener_posterior: the last run() kept no posterior sky map "
                               "(run(wiener_posterior=True))")
        gather = gather if gather is not None else self._gather
        out = self._wf.finish(self.d, gather)
        out.update(self._wf.power(gather))
        return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}

    def summary_accept_counts(self, gather=None):
        """(counts per spectrum {s: int64 [chains, flags]}, n) of the summarised
        iterations (None for the centered sampler)."""
        if self._summary is None or self.kind == "centered":
            return None, 0
        p = self.plan
        cnt = self._summary.accept_counts()
        gather = gather if gather is not None else self._gather
        if gather is not None:
            cnt = gather(cnt.contiguous(), dim=0)
        cnt = cnt.cpu().numpy()
        out, off = {}, 0
        for s in MH_ORDER[p.F]:
            n = (len(p.blocks[s]) - 1) * p.n_iter_metropolis
            out[s] = cnt[:, off:off + n]
            off += n
        return out, self._summary.n

    def capture_steps(self, nsteps, trace=None, trace_capacity=None, time_sweeps=False, time_every=1,
                      accept_trace=None, adapt=False):
        """Native RNG: capture ``nsteps`` whole iterations in ONE hipGraph (one
        replay = nsteps steps).  time_sweeps: bracket the CR-sweep kernel of every
        ``time_every``-th step by event-record nodes (plan.sweep_timing), so the
        sweep's duration is measured on its own stream inside the replay (an event
        node costs ~5 us of the step); collect with plan.sweep_timing(False).
        NC steps without a stored map are emitted pipelined by the library
        (plan.nc_steps; option GS_NC_PIPE): a timed sweep then shares the GPU with
        the previous step's finish and MH, and its time includes that."""
        if self.rng != "native":
            raise ValueError("capture_steps: native RNG runs only")
        p = self.plan
        p.iteration_counter(True, self.iteration + 1)
        # NC without a stored map: the sweeps do not depend on the chains' state, and
        # the library emits the steps pipelined (sweep i + 1 beside finish and MH of
        # step i, gs_nc_steps); a stored map, ASIS and centered keep the serial order
        pipe = self.kind == "noncentered" and self.s is None and \
            (accept_trace is None or accept_trace[0].is_contiguous()) and p.nc_pipe_prepare()
        torch.cuda.synchronize()
        if time_sweeps:
            p.sweep_timing(True)
        g = torch.cuda.CUDAGraph()
        try:
            with _capture(g):
                if pipe:
                    acc = self.accept if accept_trace is None else accept_trace
                    p.nc_steps(self.d, self.dl, nsteps, seed=self.seed, accept=acc,
                               accept_stride=0 if accept_trace is None else accept_trace.stride(0), trace=trace,
                               capacity=trace_capacity or 0, adapt=adapt, time_every=time_every if time_sweeps else 0)
                for i in range(0 if pipe else nsteps):
                    # step i reads base + i; only the last step's last launch advances
                    # the base (by nsteps): one counter ticket per replay
                    p.graph_step(i, nsteps if i == nsteps - 1 else 0)
                    if time_sweeps:
                        p.sweep_timing("resume" if i % time_every == 0 else "pause")
                    # accept_trace [nsteps, nchains, nacc]: step i writes its own slot
                    acc = self.accept if accept_trace is None else accept_trace[i]
                    if self.kind == "noncentered":
                        p.nc_prologue(self.dl, seed=self.seed)
                        p.nc_sweep(self.d, self.dl, self.s, seed=self.seed, finish=False)
                        p.nc_finish()
                        p.nc_decide_fused(self.dl, seed=self.seed, accept=acc, trace=trace,
                                          capacity=trace_capacity or 0)
                    elif self.kind == "centered":
                        p.step_centered_fused(self.d, self.dl, self.s, seed=self.seed, trace=trace,
                                              capacity=trace_capacity or 0)
                    else:
                        p.step_asis_fused(self.d, self.dl, self.s, seed=self.seed, accept=acc,
                                          dl_tmp=self.dl_tmp, recentre=self.materialize_recentre, trace=trace,
                                          capacity=trace_capacity or 0)
                    if adapt:
                        # after this step's decisions, before the next launch that
                        # draws proposals (prologue, sweep / finish front, ASIS's
                        # statistics launch): all later on this stream
                        p.mh_adapt(acc)
        finally:
            # back to one step per replay even when a launch raised inside the capture
            p.graph_step(0, 1)
        self.graph = g
        self.graph_steps = nsteps
        self.graph_pipelined = bool(pipe)
        return g

    def _launch_step(self, it, z=None, ig=None, up=None, ua=None):
        p = self.plan
        if self.kind == "centered":
            p.step_centered(self.d, self.dl, self.s, z=z, igvar=ig, seed=self.seed, iteration=it)
        elif self.kind == "noncentered":
            p.step_noncentered(self.d, self.dl, self.s, z=z, u_prop=up, u_acc=ua, seed=self.seed, iteration=it,
                               accept=self.accept)
        else:
            p.step_asis(self.d, self.dl, self.s, z=z, igvar=ig, u_prop=up, u_acc=ua, seed=self.seed, iteration=it,
                        accept=self.accept, dl_tmp=self.dl_tmp, recentre=self.materialize_recentre)

    def step(self):
        if getattr(self, "graph", None) is not None:
            self.graph.replay()
            self.iteration += getattr(self, "graph_steps", 1)
            return
        p = self.plan
        it = self.iteration + 1
        z = ig = up = ua = None
        if self.rng == "replay":
            z, ig, up, ua = self._replay()
        self._launch_step(it, z, ig, up, ua)
        self.iteration = it

    # -- a whole run --------------------------------------------------------------------
    def run(self, dls_init, n_iter, timings=False, gather=None, graph_chunk=32, resume=None, n_warmup=0,
            target_accept=0.25, summary=None, keep_history=True, blackwell_rao=None, keep_scales=False,
            br_likelihood=None, br_samples=None, wiener_posterior=None):
        """n_iter iterations from dls_init; returns (histories, accepts[, step
        times]).  gather: ShardContext.gather of a torchrun job -- the device
        histories of every rank are all-gathered along the chain axis (global
        chain order) before the one copy to the host.  resume: a state_dict()
        to continue from instead of starting at dls_init (the history's first
        row is then the restored D_l, i.e. the previous run's last row).
        n_warmup: the first n_warmup iterations adapt the MH proposal scale of
        every (chain, block) towards the acceptance rate target_accept
        (Robbins-Monro on the log-scale, on the device); the scales are frozen
        for the rest, an ordinary MH chain.  The histories keep their shape
        (warm-up rows included); runner.n_warmup is the iteration the warm-up
        ends at.  A resumed state carries its own warm-up bookkeeping and goes
        on with it; n_warmup > 0 with a resume adds that many warm-up iterations.
        summary: None, True or {max_lag: 32, start: None} -- a streaming summary
        of the D_l chains (moments, autocovariances up to max_lag, ESS, R-hat;
        runner.summary()) updated on the device from the trace ring after every
        chunk replay (eager / replay-RNG steps: after every step).  Iterations up
        to `start` (default: the iteration the warm-up ends at) and the initial
        row are not summarised.  A resumed state that carries a summary continues
        it; a run without resume starts a new one.  keep_history=False (needs a
        summary): no history is allocated on the device or the host and the
        histories and accepts are returned as None.
        blackwell_rao: None, {"grid": [nspec, maxbins, G]} or {"points": G, "span":
        (lo, hi)}, either with "start" (as the summary's) -- the streaming
        Blackwell-Rao marginal posterior of every drawn bin on a grid of G <= 64
        values (runner.blackwell_rao()): the C_l draw records the scale of its
        conditional in a ring beside the trace ring, and the state is updated
        from it after every chunk replay / eager step.  Centered and ASIS only.
        It also lifts the need for a summary of keep_history=False.  A resumed
        state that carries one continues it.  keep_scales: keep the scale history
        {spectrum: [n_iter, chains, nbins]} in runner.h_scales (row i belongs to
        the run's iteration i + 1; the start has no scale).
        br_likelihood: None or {"theory": {spectrum: [K, nbins]} or [K, nspec,
        maxbins], "lrange": (lmin, lmax) or "mask": ..., "start": ...} -- the
        streaming Blackwell-Rao likelihood of K fixed theory spectra over the
        used bins (runner.br_likelihood()): the joint inverse-Gamma /
        inverse-Wishart density of the theory under every sample's conditional,
        accumulated from the same scale ring after every chunk replay / eager
        step into 24 B per (chain, model).  Centered and ASIS only; it too
        lifts the need for a summary of keep_history=False, and a resumed
        state that carries one continues it.
        br_samples: None, True or {"lrange": (lmin, lmax) or "mask": ..., "start":
        ...} -- the Blackwell-Rao sample bank (runner.br_samples()): the scales
        of the used bins of every iteration after `start` are packed from the
        same scale ring into a bank on the device after every chunk replay /
        eager step, 8 (Ju + 1) bytes per chain and iteration over Ju used
        columns, and bank.loglike(theory) scores theory spectra that need not be
        known before the run.  Centered and ASIS only; it lifts the need for a
        summary of keep_history=False, and a resumed state that carries a bank
        continues it (a state_dict holds the whole bank on the host).
        wiener_posterior: None, True or {"start": ...} -- the Rao-Blackwellised
        posterior sky map (runner.wiener_posterior()): the closed-form centered
        operator M_l(D_l), Sigma_l(D_l) of every iteration after `start` (as
        the summary's) is accumulated from the D_l trace ring after every chunk
        replay / eager step, O(chains L) per iteration and 160 B per (chain, l)
        for TEB.  Every sampler kind; it lifts the need for a summary of
        keep_history=False, and a resumed state that carries one continues it."""
        p = self.plan
        n_warmup = check_warmup(self.kind, self.rng, n_warmup, target_accept)
        br_opts = check_blackwell_rao(blackwell_rao, p.F, p.bins, dls_init, p.maxbins)
        brl_opts = check_br_likelihood(br_likelihood, p.F, p.bins, p.maxbins)
        if (br_opts is not None or keep_scales) and self.kind == "noncentered":
            raise NotImplementedError("blackwell_rao / keep_scales: the non-centered sampler has no centered "
                                      "conditional draw (use the centered or the ASIS sampler)")
        if brl_opts is not None and self.kind == "noncentered":
            raise NotImplementedError("br_likelihood: the non-centered sampler has no centered conditional draw "
                                      "(use the centered or the ASIS sampler)")
        brs_opts = check_br_samples(br_samples, p.F, p.bins, p.maxbins)
        if brs_opts is not None and self.kind == "noncentered":
            raise NotImplementedError("br_samples: the non-centered sampler has no centered conditional draw "
                                      "(use the centered or the ASIS sampler)")
        wf_opts = check_wiener_posterior(wiener_posterior)
        sm_opts = check_summary(summary, keep_history or br_opts is not None or brl_opts is not None or
                                brs_opts is not None or wf_opts is not None)
        if p.scale_trace is not None:
            p.cls_scale_trace(None)         # left attached by a run that raised
        self._gather = gather
        if resume is not None:
            self.load_state_dict(resume)
            if n_warmup > 0:
                self._adapt_enable(target_accept)
                self.n_warmup = self.iteration + n_warmup
        else:
            self.init(dls_init)
            self.n_warmup = n_warmup
            if n_warmup > 0:
                self._adapt_enable(target_accept)
                p.mh_scale_set(torch.zeros(p.nchains, p.nblocks_mh, dtype=torch.float64),
                               torch.zeros(p.nchains, p.nblocks_mh, dtype=torch.int32))
        if resume is None or self._summary is None:
            # a new summary (a resumed state that carries one continues it instead)
            if sm_opts is None:
                self._summary = None
            else:
                self._summary_alloc(sm_opts[0])
                self.summary_start = self.n_warmup if sm_opts[1] is None else sm_opts[1]
        if resume is None or self._br is None:
            if br_opts is None:
                self._br = None
            else:
                if br_opts["grid"] is None:
                    raise ValueError("blackwell_rao: the points form needs dls_init to centre its grid on")
                self._br = BlackwellRaoState(p.nchains, br_opts["grid"], br_opts["alpha"], br_opts["half_mask"],
                                             device=p.device)
                self.br_start = self.n_warmup if br_opts["start"] is None else br_opts["start"]
        if resume is None or self._brl is None:
            if brl_opts is None:
                self._brl = None
            else:
                self._brl = BlackwellRaoLikelihood(p.nchains, p.nspec, p.maxbins, brl_opts["tables"], device=p.device)
                self.brl_start = self.n_warmup if brl_opts["start"] is None else brl_opts["start"]
        if resume is None or self._brs is None:
            self._brs = None
            if brs_opts is not None:
                self.brs_start = self.n_warmup if brs_opts["start"] is None else brs_opts["start"]
                self._brs = BlackwellRaoSamples(p.nchains, p.F, p.bins, brs_opts["mask"],
                                                self.iteration + n_iter - max(self.iteration, self.brs_start),
                                                device=p.device, draws=brs_opts["draws"])
        if resume is None or self._wf is None:
            if wf_opts is None:
                self._wf = None
            else:
                self._wf_alloc()
                self.wf_start = self.n_warmup if wf_opts["start"] is None else wf_opts["start"]
        sm, br, brl, brs, wf = self._summary, self._br, self._brl, self._brs, self._wf
        if brs is not None and brs_opts is not None and brs.draws != brs_opts["draws"]:
            raise ValueError("br_samples: the resumed sample bank was kept with draws=%s; a run that continues it cannot "
                             "change that" % brs.draws)
        if brs is not None:
            if self.kind == "noncentered":
                raise NotImplementedError("br_samples: the non-centered sampler has no centered conditional draw")
            # room for this run's iterations after brs_start
            brs.reserve(brs.n + max(self.iteration + n_iter - max(self.iteration, self.brs_start), 0))
        if br is not None and self.kind == "noncentered":
            raise NotImplementedError("blackwell_rao: the non-centered sampler has no centered conditional draw")
        if brl is not None and self.kind == "noncentered":
            raise NotImplementedError("br_likelihood: the non-centered sampler has no centered conditional draw")
        if sm is None and br is None and brl is None and brs is None and wf is None and not keep_history:
            raise ValueError("keep_history=False needs a summary")
        with_scales = br is not None or brl is not None or brs is not None or keep_scales
        self.h_scales = None
        Hs = p.zeros(n_iter, p.nchains, p.nspec, p.maxbins) if keep_scales else None
        # steps of this run that adapt; warm-up and frozen steps never share a graph
        n_adapt = min(max(self.n_warmup - self.iteration, 0), n_iter)
        with_start = self.kind != "asis"
        H = A = None
        if keep_history:
            H = p.zeros(n_iter + (1 if with_start else 0), p.nchains, p.nspec, p.maxbins)
            A = p.zeros(n_iter, p.nchains, max(p.nacc, 1), dtype=torch.int32)
            if with_start:
                H[0].copy_(self.dl)
        t_steps = []
        if self.rng == "native" and graph_chunk and n_iter > 0:
            # the iterations as replays of captured hipGraphs of `chunk` steps
            # (device-side D_l / accept traces, no host synchronisation inside a
            # chunk); step times = chunk time / steps from events on the stream.
            # The graphs (and the trace buffers they write) are kept per chunk
            # length across run() calls: a later run replays them without
            # capturing again (the device counter base is set before each run)
            chunk = min(int(graph_chunk), n_iter)
            off = 1 if with_start else 0
            cache = self.__dict__.setdefault("_run_graphs", {})
            if cache.get("chunk") != chunk:
                cache.clear()
                cache["chunk"] = chunk
                cache["trace"] = p.zeros(chunk, p.nchains, p.nspec, p.maxbins)
                cache["acc"] = p.zeros(chunk, p.nchains, max(p.nacc, 1), dtype=torch.int32)
            trace, acc_tr = cache["trace"], cache["acc"]
            # the scale ring beside the trace ring; graphs captured with it attached
            # hold its pointer and are cached under keys of their own
            sc_tr = cache.setdefault("scales", p.zeros(chunk, p.nchains, p.nspec, p.maxbins)) if with_scales else None
            # single-rank runs: each finished chunk of the histories goes to pinned
            # host memory on a copy stream while the next chunk computes (only the
            # last chunk's transfer is left after the loop)
            if gather is None and keep_history:
                Hh = torch.empty(H.shape, dtype=H.dtype, pin_memory=True)
                Ah = torch.empty(A.shape, dtype=A.dtype, pin_memory=True)
            if gather is None and (keep_history or keep_scales):
                cs = cache.setdefault("copy_stream", torch.cuda.Stream())
            if gather is None and keep_scales:
                Sh = torch.empty(Hs.shape, dtype=Hs.dtype, pin_memory=True)
            p.iteration_counter(True, self.iteration + 1)
            p.cls_scale_trace(sc_tr, chunk)
            done = 0
            while done < n_iter:
                adapt = done < n_adapt
                k = min(chunk, (n_adapt if adapt else n_iter) - done)
                key = ("adapt", k) if adapt else k
                if with_scales:
                    key = ("scales", key)
                if key not in cache:
                    cache[key] = self.capture_steps(k, trace=trace, trace_capacity=chunk, accept_trace=acc_tr,
                                                    adapt=adapt)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                # the trace record of iteration it goes to slot (it - 1) % chunk: a
                # run resumed at an iteration that is not a multiple of chunk starts
                # mid-ring
                r0 = self.iteration % chunk
                e0.record()
                cache[key].replay()
                self.iteration += k
                e1.record()
                if sm is not None:
                    # one launch on the run's stream: the chunk's rows of the ring
                    # and its accept flags (the captured graphs are not touched)
                    self._summary_update(trace, chunk, self.iteration - k, k, acc_tr, acc_tr.stride(0))
                if wf is not None:
                    self._wf_update(trace, chunk, self.iteration - k, k)
                if br is not None:
                    self._br_update(sc_tr, chunk, self.iteration - k, k)
                if brl is not None:
                    self._brl_update(sc_tr, chunk, self.iteration - k, k)
                if brs is not None:
                    self._brs_append(sc_tr, chunk, self.iteration - k, k, trace)
                if keep_scales:
                    Hs[done:done + k].copy_(sc_tr[:k] if r0 == 0 else sc_tr[(torch.arange(k) + r0) % chunk])
                h0, h1 = (0 if done == 0 else off + done), off + done + k
                if keep_history:
                    if r0 == 0:
                        H[off + done:h1].copy_(trace[:k])
                    else:
                        H[off + done:h1].copy_(trace[(torch.arange(k) + r0) % chunk])
                    A[done:done + k].copy_(acc_tr[:k])
                if gather is None and keep_history:
                    ev = torch.cuda.Event()
                    ev.record()
                    cs.wait_event(ev)
                    with torch.cuda.stream(cs):
                        Hh[h0:h1].copy_(H[h0:h1], non_blocking=True)
                        Ah[done:done + k].copy_(A[done:done + k], non_blocking=True)
                if gather is None and keep_scales:
                    ev = torch.cuda.Event()
                    ev.record()
                    cs.wait_event(ev)
                    with torch.cuda.stream(cs):
                        Sh[done:done + k].copy_(Hs[done:done + k], non_blocking=True)
                if timings:
                    e1.synchronize()
                    t_steps += [e0.elapsed_time(e1) * 1e-3 / k] * k
                done += k
            # the last step's flags, as the eager path leaves them in runner.accept
            if self.kind != "centered":
                self.accept.copy_(acc_tr[k - 1][:, :self.accept.shape[1]])
            self.graph = None
            p.iteration_counter(False)
            p.cls_scale_trace(None)
            n_iter = 0
            if gather is None and (keep_history or keep_scales):
                cs.synchronize()
            if gather is None and keep_history:
                H, A = Hh, Ah
            if gather is None and keep_scales:
                Hs = Sh
        # eager steps: a one-row scale ring, as the chain's D_l is a one-row trace
        sc1 = p.zeros(1, p.nchains, p.nspec, p.maxbins) if with_scales and n_iter > 0 else None
        if sc1 is not None:
            p.cls_scale_trace(sc1, 1)
        for i in range(n_iter):
            t0 = time.perf_counter() if timings else 0.0
            self.step()
            if i < n_adapt:
                p.mh_adapt(self.accept)
            if br is not None:
                self._br_update(sc1, 1, self.iteration - 1, 1)
            if brl is not None:
                self._brl_update(sc1, 1, self.iteration - 1, 1)
            if brs is not None:
                self._brs_append(sc1, 1, self.iteration - 1, 1, self.dl)
            if keep_scales:
                Hs[i].copy_(sc1[0])
            if sm is not None:
                # the chain's D_l as a one-row trace
                self._summary_update(self.dl, 1, self.iteration - 1, 1, self.accept, 0)
            if wf is not None:
                self._wf_update(self.dl, 1, self.iteration - 1, 1)
            if keep_history:
                H[i + (1 if with_start else 0)].copy_(self.dl)
                if self.kind != "centered":
                    A[i].copy_(self.accept)
            if timings:
                torch.cuda.synchronize()
                t_steps.append(time.perf_counter() - t0)
        if sc1 is not None:
            p.cls_scale_trace(None)
        if keep_scales:
            Sn = (Hs if gather is None else gather(Hs, dim=1)).cpu().numpy()
            self.h_scales = {s: Sn[:, :, k, :len(p.bins[s]) - 1] for k, s in enumerate(p.spectra)}
        if not keep_history:
            if timings:
                torch.cuda.synchronize()
                return None, None, np.array(t_steps)
            return None, None
        if gather is not None:
            H = gather(H, dim=1)
            if self.kind != "centered":
                A = gather(A, dim=1)
        Hn = H.cpu().numpy()
        hist = {s: Hn[:, :, k, :len(p.bins[s]) - 1] for k, s in enumerate(p.spectra)}
        acc = None
        if self.kind != "centered":
            An = A.cpu().numpy()
            acc, off = {}, 0
            for s in MH_ORDER[p.F]:
                n = (len(p.blocks[s]) - 1) * p.n_iter_metropolis
                acc[s] = An[:, :, off:off + n]
                off += n
        if timings:
            return hist, acc, np.array(t_steps)
        return hist, acc

    def skymap(self):
        """Current sky map [nchains, F, (L+1)^2] as the reference would hold it
        (for ASIS with lazy re-centring the re-centred map is materialised here)."""
        if self.s is None:
            return None
        s = self.s.clone()
        if self.kind == "asis" and not self.materialize_recentre and self.iteration > 0:
            # ASIS.py:203 quirk: s <- A(C_new) s; corrected: s <- A(C_new) A(C_tmp)^+ s
            quirk = bool(self.quirks & C.GS_QUIRK_ASIS_RECENTRE_CENTERED)
            self.plan.recentre(self.dl, s, None if quirk else self.dl_tmp)
        return s

