"""Multi-block / binned Metropolis layouts for every spectrum, and the oracle
chains that run them (numpy, fp64; oracle.harmonic only).

The reference's default blocking (gibbssampler_amd.problem.default_blocks) keeps
TT, EE and TE as one whole-range block each, so with it the T / E phases of the
NC Metropolis kernels decide one block per spectrum.  The layouts here give the
T / E spectra several blocks: narrow ones (at most MH_SMALL multipoles, one
thread each) beside wide ones, more wide blocks than the LDS-phase kernel
decides together, binned spectra, bins of no block, and a last block edge past
the bin count.

Two properties of the plan shape the layouts:
  * a TEB plan requires TT, EE and TE to share their bins (the centered
    inverse-Wishart draw is per bin), so at F = 3 the three spectra use the TT
    recipe; at F = 1 / F = 2 each spectrum has its own;
  * blocks are an array of edges (block k = bins [e_k, e_k+1)), so consecutive
    blocks always touch: bins of no block can only lie before the first edge
    or after the last one.

Used by tests/test_gpu_mh_blocking.py, tests/test_gpu_longchain_small.py,
tests/test_longchain_fixtures_cpu.py and tools/gen_golden_longchain_small.py.
"""
import numpy as np

from gibbssampler_amd.problem import SPECTRA, synthetic_problem
from oracle import harmonic as H

L_SMALL, NSIDE_SMALL = 130, 64
MH_ORDER = {1: ("TT",), 2: ("EE", "BB"), 3: ("EE", "BB", "TT", "TE")}
# binned_mixed: (unbinned up to this l, bin width above it), own recipe of each spectrum
BIN_RECIPE = {"TT": (40, 3), "EE": (50, 4), "BB": (60, 7), "TE": (30, 5)}
# the recipe's proposal variances scaled so that both branches of the accept
# decision occur with a margin (chosen with the oracle alone): per-bin EE
# proposals are accepted ~99.7 % of the time at the recipe's scale; blocks of
# 21-22 multipoles with per-bin scales reject every TT proposal
PV_SCALE = {"EE": 300.0}
PV_SCALE_MANY_WIDE = {"TT": 0.02, "TE": 0.1}
LAYOUTS = ("per_bin", "binned_mixed", "many_wide", "near_singular")


def binned_edges(lmax, upto, width):
    """Bin edges: one bin per l below `upto`, then bins of `width` multipoles (the last one shorter)."""
    e = list(range(0, upto + 1)) + list(range(upto + width, lmax + 1, width))
    if e[-1] != lmax + 1:
        e.append(lmax + 1)
    return np.array(e, dtype=np.int64)


def mixed_bins(lmax, F, upto=None, shared=True):
    """The bins of binned_mixed.  F = 3: TT, EE and TE share the TT recipe (the
    plan refuses a TEB model whose T / E spectra are binned differently:
    shared=False builds that model)."""
    out = {}
    for s in SPECTRA[F]:
        u, w = BIN_RECIPE["TT" if (F == 3 and shared and s != "BB") else s]
        out[s] = binned_edges(lmax, u if upto is None else upto, w)
    return out


def unbinned(lmax, F):
    return {s: np.arange(0, lmax + 2) for s in SPECTRA[F]}


def per_bin_bins(lmax, F):
    """T / E spectra unbinned, BB binned by its binned_mixed recipe."""
    b = unbinned(lmax, F)
    if "BB" in b:
        b["BB"] = binned_edges(lmax, *BIN_RECIPE["BB"])
    return b


def per_bin_blocks(bins):
    """One block per bin from bin 2, and one more edge: the last block is empty
    after clipping to the bin count.  BB: [2, 30) first, then per bin."""
    out = {}
    for s, b in bins.items():
        nb = len(b) - 1
        out[s] = np.concatenate([[2], np.arange(30, nb + 2)]) if s == "BB" else np.arange(2, nb + 2)
    return out


def mixed_blocks(bins, wide=20, wide_bb=45):
    """One wide block of `wide` - 2 bins, one block per bin up to bin nb - 5, then
    [nb - 5, nb - 1) and [nb - 1, nb + 7): the last edge lies past the bin count.
    Two used bins of each T / E spectrum belong to no block: bins 2 and 3 of TT
    and TE (the wide block starts at bin 4), the last two bins of EE (its last
    blocks are [nb - 5, nb - 2) and nothing after)."""
    out = {}
    for s, b in bins.items():
        nb = len(b) - 1
        k = wide_bb if s == "BB" else wide
        first = 4 if s in ("TT", "TE") else 2
        k += first - 2                              # the wide block keeps its width
        tail = [nb - 2] if s == "EE" else [nb - 1, nb + 7]
        out[s] = np.concatenate([[first], np.arange(k, nb - 4), tail]).astype(np.int64)
    return out


def many_wide_blocks(bins):
    """TT / EE / TE: six blocks of 21-22 multipoles (unbinned); BB as per_bin."""
    out = per_bin_blocks(bins)
    for s in bins:
        if s != "BB":
            nb = len(bins[s]) - 1
            out[s] = np.round(np.linspace(2, nb, 7)).astype(np.int64)
    return out


def build(layout, F=3, lmax=L_SMALL, nside=NSIDE_SMALL, upto=None, wide=20, wide_bb=45):
    """(problem dict of synthetic_problem, start D_l) of a layout."""
    if layout in ("per_bin", "near_singular"):
        bins = per_bin_bins(lmax, F)
        blocks = per_bin_blocks(bins)
    elif layout == "binned_mixed":
        bins = mixed_bins(lmax, F, upto)
        blocks = mixed_blocks(bins, wide, wide_bb)
    elif layout == "many_wide":
        bins = per_bin_bins(lmax, F)
        blocks = many_wide_blocks(bins)
    else:
        raise ValueError(layout)
    P = synthetic_problem(lmax, nside, F, seed=0, bins=bins, blocks=blocks)
    for s, f in {**PV_SCALE, **(PV_SCALE_MANY_WIDE if layout == "many_wide" else {})}.items():
        if s in P["proposal_variances"]:
            P["proposal_variances"][s] = P["proposal_variances"][s] * f
    start = {s: np.array(v, dtype=np.float64) for s, v in P["dls_init"].items()}
    if layout == "near_singular":
        # every third bin starts close to the edge of the positive-definite cone
        k = np.arange(2, len(start["TE"]), 3)
        start["TE"][k] = 0.98 * np.sqrt(start["TT"][k] * start["EE"][k])
    return P, start


def model_of(P):
    return H.Model(P["lmax"], P["nside"], P["nfields"], P["bl"], P["noise_var"], P["bins"], P["blocks"],
                   P["proposal_variances"], P["d_alm"])


def wide_blocks(bins, blocks, small):
    """Blocks of a spectrum that cover more than `small` multipoles (after clipping)."""
    nb = len(bins) - 1
    e = np.clip(np.asarray(blocks), 0, nb)
    return int(sum(1 for k in range(len(e) - 1) if e[k + 1] > e[k] and bins[e[k + 1]] - bins[e[k]] > small))


# ---- oracle chains ---------------------------------------------------------------------------
def _sweep(m, params, dl, seed, chain, it):
    M, Lc = params(m, m.unfold(dl))
    z = np.stack([H.cr_normals(seed, chain, it, 0, f, m.L) for f in range(m.nfields)])
    return H.sweep_stats(m, H.cr_apply(m, M, Lc, m.d_alm, z), m.d_alm)


def oracle_step(m, kind, dl, seed, chain, it, n_mh=1):
    """One iteration of one chain: (new D_l dict, accept dict or None).
    noncentered: NonCenteredGibbs.py:134-176, 401-445; centered: CenteredGibbs.py
    CR and C_l draw; asis: ASIS.py:134-226 (the re-centring acts on the map only,
    which the next iteration's CR replaces)."""
    if kind == "noncentered":
        return H.nc_mh(m, dl, _sweep(m, H.noncentered_params, dl, seed, chain, it), seed=seed, chain=chain,
                       iteration=it, n_iter=n_mh)
    st = _sweep(m, H.centered_params, dl, seed, chain, it)
    drawn = H.centered_cls_draw(m, st, seed=seed, chain=chain, iteration=it)
    if kind == "centered":
        return drawn, None
    st_nc = H.transform_stats(st, H.chol_pinv(H.cov_chol(m, m.unfold(drawn))))
    return H.nc_mh(m, drawn, st_nc, seed=seed, chain=chain, iteration=it, n_iter=n_mh)


def oracle_chain(m, kind, start, seed, chain, niter, n_mh=1):
    """(D_l history {s: [niter, nbins]}, flags {s: [niter, blocks * n_mh]} or None)."""
    dl = {s: np.array(start[s], dtype=np.float64) for s in m.spectra}
    hist = {s: [] for s in m.spectra}
    flags = {s: [] for s in m.spectra}
    for it in range(1, niter + 1):
        dl, acc = oracle_step(m, kind, dl, seed, chain, it, n_mh)
        for s in m.spectra:
            hist[s].append(np.asarray(dl[s], dtype=np.float64).copy())
            if acc is not None:
                flags[s].append(np.asarray(acc[s], dtype=np.int32))
    return ({s: np.stack(v) for s, v in hist.items()},
            None if kind == "centered" else {s: np.stack(v) for s, v in flags.items()})


def count_psd_failures(m, start, seed, chain, niter):
    """Over a noncentered oracle chain: per iteration and T / E spectrum, the
    blocks whose proposal fails the positive-definiteness test (H._psd_ok) and
    the blocks that accept.  Returns {s: [niter, 2]} (failed, accepted)."""
    calls = []
    orig = H._psd_ok

    def spy(model, un, ells):
        ok = orig(model, un, ells)
        calls.append(ok)
        return ok

    out = {s: [] for s in m.spectra}
    dl = {s: np.array(start[s], dtype=np.float64) for s in m.spectra}
    H._psd_ok = spy
    try:
        for it in range(1, niter + 1):
            del calls[:]
            dl, acc = oracle_step(m, "noncentered", dl, seed, chain, it)
            pos = 0
            for s in MH_ORDER[m.nfields]:          # nc_mh calls _psd_ok once per block, in this order
                n = len(acc[s])
                out[s].append((int(n - sum(calls[pos:pos + n])), int(np.sum(acc[s]))))
                pos += n
            assert pos == len(calls)
    finally:
        H._psd_ok = orig
    return {s: np.array(v) for s, v in out.items()}
