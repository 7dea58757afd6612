"""Test-side restatement of the warm-up adaptation of the NC Metropolis proposal
scales (numpy, fp64), and an oracle chain that runs it.

The recursion, per chain c and MH block j (blocks in the order of the accept
flags: the spectra in MH order, each spectrum's blocks in turn):

    abar = mean of the block's n_iter_metropolis accept flags of this step
    n   <- n + 1
    lam <- clip(lam + n^-kappa (abar - target), -lmax, lmax)
    sd[c][spectrum][bin] = sd0[spectrum][bin] exp(lam[c][block of bin])

The oracle chain is built on oracle.harmonic (cr_normals -> cr_apply ->
sweep_stats -> nc_mh, as tools/gen_golden_longchain.py): every chain owns a
copy of the model whose proposal_variances[s] = sd_c^2 for the step
(sqrt(x^2) == x in binary fp64, so nc_mh sees the same sd).
"""
import copy

import numpy as np

from oracle import harmonic as H

MH_ORDER = {1: ("TT",), 2: ("EE", "BB"), 3: ("EE", "BB", "TT", "TE")}
KAPPA, TARGET, LAM_MAX = 0.6, 0.25, 20.0


def block_layout(model):
    """[(spectrum, first block, blocks)] of the flat per-chain block axis."""
    out, off = [], 0
    for s in MH_ORDER[model.nfields]:
        nb = len(model.blocks[s]) - 1
        out.append((s, off, nb))
        off += nb
    return out


def rm_update(lam, n, abar, target=TARGET, kappa=KAPPA, lam_max=LAM_MAX):
    """One Robbins-Monro step; lam, n, abar arrays of one shape.  Returns (lam, n)."""
    n = np.asarray(n, dtype=np.int64) + 1
    step = np.power(n.astype(np.float64), -kappa) * (np.asarray(abar, dtype=np.float64) - target)
    return np.clip(np.asarray(lam, dtype=np.float64) + step, -lam_max, lam_max), n


def block_means(flags, n_mh):
    """accept flags [..., nblocks * n_mh] -> acceptance per block [..., nblocks]."""
    f = np.asarray(flags, dtype=np.float64)
    return f.reshape(f.shape[:-1] + (f.shape[-1] // n_mh, n_mh)).mean(axis=-1)


def recursion(flag_history, n_mh, target=TARGET, kappa=KAPPA, lam_max=LAM_MAX, lam0=None, n0=None):
    """The recursion over a flag history [T, ..., nblocks * n_mh]; returns (lam, n)."""
    ab = block_means(flag_history, n_mh)
    lam = np.zeros(ab.shape[1:]) if lam0 is None else np.array(lam0, dtype=np.float64)
    n = np.zeros(ab.shape[1:], dtype=np.int64) if n0 is None else np.array(n0, dtype=np.int64)
    for t in range(ab.shape[0]):
        lam, n = rm_update(lam, n, ab[t], target, kappa, lam_max)
    return lam, n


def expand_sd(model, lam_chain):
    """dict spectrum -> sd[nbins - 2] of one chain: sd0 exp(lam of the bin's block)
    (block edges clipped to the bin count; bins of no block keep sd0)."""
    out = {}
    for s, off, nb in block_layout(model):
        sd = np.sqrt(np.asarray(model.proposal_variances[s], dtype=np.float64))
        nbins = model.nbins(s)
        e = np.clip(np.asarray(model.blocks[s], dtype=np.int64), 0, nbins)
        for k in range(nb):
            lo, hi = max(int(e[k]), 2), int(e[k + 1])
            if hi > lo:
                sd[lo - 2:hi - 2] = sd[lo - 2:hi - 2] * np.exp(lam_chain[off + k])
        out[s] = sd
    return out


def flat_flags(model, acc):
    """nc_mh's accept dict -> the flat flag row of the device layout."""
    return np.concatenate([np.asarray(acc[s], dtype=np.int64) for s in MH_ORDER[model.nfields]])


def oracle_chain(model, init, seed, chain, n_steps, n_warmup, n_mh=1, target=TARGET, kappa=KAPPA):
    """One non-centered chain with the adaptation on for its first n_warmup
    steps.  Returns (history {s: [n_steps + 1, nbins]}, flags [n_steps, nacc],
    lam [nblocks], n [nblocks])."""
    F = model.nfields
    nblk = sum(nb for _, _, nb in block_layout(model))
    lam, n = np.zeros(nblk), np.zeros(nblk, dtype=np.int64)
    dl = {s: np.array(init[s], dtype=np.float64) for s in model.spectra}
    hist = {s: [dl[s].copy()] for s in model.spectra}
    flags = []
    m = copy.copy(model)
    for it in range(1, n_steps + 1):
        sd = expand_sd(model, lam)
        m.proposal_variances = {s: sd[s] ** 2 for s in model.spectra}
        M, Lc = H.noncentered_params(m, m.unfold(dl))
        z = np.stack([H.cr_normals(seed, chain, it, 0, f, m.L) for f in range(F)])
        st = H.sweep_stats(m, H.cr_apply(m, M, Lc, m.d_alm, z), m.d_alm)
        dl, acc = H.nc_mh(m, dl, st, seed=seed, chain=chain, iteration=it, n_iter=n_mh)
        fl = flat_flags(model, acc)
        flags.append(fl)
        if it <= n_warmup:
            lam, n = rm_update(lam, n, block_means(fl, n_mh), target, kappa)
        for s in model.spectra:
            hist[s].append(np.asarray(dl[s], dtype=np.float64).copy())
    return {s: np.stack(v) for s, v in hist.items()}, np.stack(flags), lam, n


def small_problem(F, bb_blocks="per_bin", var_scale=1.0, L=40, nside=16):
    """tests._util.make_problem at L 40 / N_side 16 with the reference's blocking:
    TT, EE and TE one whole-range block each, BB one block per bin
    (bb_blocks="per_bin"), or BB blocks of several bins whose last edge lies
    past the bin count and is clipped ("wide")."""
    from tests._util import make_problem
    model, init = make_problem(L, nside, F)
    if "BB" in model.spectra:
        nb = model.nbins("BB")
        if bb_blocks == "per_bin":
            model.blocks["BB"] = np.arange(2, nb + 1)
        else:
            model.blocks["BB"] = np.array([2, 7, 12, 20, nb + 11])
    model.proposal_variances = {s: np.asarray(v) * var_scale for s, v in model.proposal_variances.items()}
    return model, init
