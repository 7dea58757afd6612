"""Test-side restatement of the Blackwell-Rao likelihood gradient
(gibbssampler_amd/csrc/gs_brs.hip, k_brs_grad ...), numpy, on tests/_br_samples.py.

From rows [T, C, nsb] and the tables of engine.br_likelihood_tables, with t of
_br_samples.terms (longdouble, NaN rows for the bad samples):
    M[k] = max_ci t,  w[c, i, k] = exp(t - M)          (longdouble, no running state)
    xbar[k, j] = sum_ci w x[c, i, j] / sum_ci w         d loglike_k / d Y_kj = -xbar_kj
    abar[k, j] = sum_ci w |x[c, i, j]| / sum_ci w       (the magnitude the error scales with)
    share[c, k] = sum_i w / sum_ci w
    loglike[k] = (M + log sum_ci w) - log(C T) + cst[k]
NaN where no sample is good.  All sums run over every (chain, row) at once."""
import numpy as np

from tests import _br_likelihood as R
from tests import _br_samples as B

LD = np.longdouble


def weights(rows, tables, maxbins):
    """{xbar, abar [K, Ju], share [C, K], loglike [K]} (fp64; loglike_ld: the
    longdouble value) of rows [T, C, nsb]."""
    T, C = rows.shape[:2]
    t, _ = B.terms(rows, tables, maxbins)                      # [C, T, K]
    K = t.shape[2]
    cols = np.asarray(tables["cols"], dtype=np.int64)
    x = np.stack([[R.row_parts(rows[i, c], tables, maxbins)[1] for i in range(T)] for c in range(C)]).astype(LD)
    good = ~np.isnan(t[:, :, 0])                               # [C, T]
    Ju = len(cols)
    if not good.any():
        nan = np.full((K, Ju), np.nan)
        return {"xbar": nan, "abar": nan.copy(), "share": np.full((C, K), np.nan), "loglike": np.full(K, np.nan),
                "loglike_ld": np.full(K, np.nan, dtype=LD)}
    tg, xg = t[good], x[good]                                  # [N, K], [N, Ju]
    M = tg.max(axis=0)
    w = np.exp(tg - M[None, :])                                # [N, K]
    den = w.sum(axis=0)
    xbar = (w.T @ xg) / den[:, None]
    abar = (w.T @ np.abs(xg)) / den[:, None]
    share = np.zeros((C, K), dtype=LD)
    cidx = np.nonzero(good)[0]
    for c in range(C):
        share[c] = w[cidx == c].sum(axis=0) / den
    ll = (M + np.log(den)) - np.log(LD(C) * LD(T)) + np.asarray(tables["cst"]).astype(LD)
    return {"xbar": xbar.astype(np.float64), "abar": abar.astype(np.float64), "share": share.astype(np.float64),
            "loglike": ll.astype(np.float64), "loglike_ld": ll}


def xbar_bound(rows, tables, maxbins):
    """(bx [K], bw [K]): |d xbar_kj| <= bx_k abar_kj and |d chain_weight| <= bw_k.
    Each weight exp(t - M) carries the evaluator's per-sample bound delta_k = (Ju +
    16) 2^-52 T_k on t and on M: a relative 2 delta_k on numerator and denominator
    terms alike (it does not cancel: the t of the two passes round alike but the
    bound does not use that).  The C n products and their sums in any order add 2 C
    n 2^-52, the per-chain merge, the final sum and the division 16 2^-52 more."""
    T, C = rows.shape[:2]
    delta, _ = B.bounds(rows, tables, maxbins)
    return 2 * delta + (2 * C * T + 16) * 2.0 ** -52, 2 * delta + 2 * C * T * 2.0 ** -52
