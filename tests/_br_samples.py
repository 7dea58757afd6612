"""Test-side restatement of the Blackwell-Rao sample bank's evaluator
(gibbssampler_amd/csrc/gs_brs.hip), numpy, on tests/_br_likelihood.py.

From rows [T, C, nsb] (the scale ring's rows of every kept sample) and the
tables of engine.br_likelihood_tables:
    t[c, i, k] = r[c, i] - sum_j x[c, i, j] Y[k, j]     (row_parts' x and log(arg);
                 both sums in longdouble; a bad row is left out and counted)
    m[c, k] = max_i t,  S = sum_i exp(t - m),  Q = sum_i exp(2 (t - m))
directly -- no running state, no order: the sums run in longdouble -- and then
_br_likelihood.finish.  The device differs from this by the rounding of each t
(the streaming estimator's per-sample bound) and by the order in which it adds
the n weights of a chain."""
import numpy as np

from tests import _br_likelihood as R

LD = np.longdouble


def terms(rows, tables, maxbins):
    """(t [C, T, K] longdouble with NaN rows for the bad samples, bad [C])."""
    coef, Y = np.asarray(tables["coef"]).astype(LD), np.asarray(tables["Y"]).astype(LD)
    T, C = rows.shape[:2]
    t = np.full((C, T, Y.shape[0]), np.nan, dtype=LD)
    bad = np.zeros(C, dtype=np.int64)
    for i in range(T):
        for c in range(C):
            ok, x, lg = R.row_parts(rows[i, c], tables, maxbins)
            if not ok:
                bad[c] += 1
                continue
            t[c, i] = np.sum(coef * lg.astype(LD)) - Y @ x.astype(LD)
    return t, bad


def state(rows, tables, maxbins):
    """(m, S, Q [C, K] fp64, bad [C], n) of rows [T, C, nsb]."""
    t, bad = terms(rows, tables, maxbins)
    C, T, K = t.shape
    m, S, Q = np.zeros((C, K)), np.zeros((C, K)), np.zeros((C, K))
    for c in range(C):
        tc = t[c][~np.isnan(t[c, :, 0])]
        if tc.shape[0] == 0:
            continue
        mc = tc.max(axis=0)
        m[c] = mc.astype(np.float64)
        d = tc - m[c].astype(LD)[None, :]
        S[c] = np.sum(np.exp(d), axis=0).astype(np.float64)
        Q[c] = np.sum(np.exp(2 * d), axis=0).astype(np.float64)
    return m, S, Q, bad, T


def loglike(rows, tables, maxbins):
    """{loglike [K], chain_loglike [C, K], neff [K], n, bad} of rows [T, C, nsb]."""
    m, S, Q, bad, n = state(rows, tables, maxbins)
    ll, cl, ne = R.finish(m, S, Q, n, np.asarray(tables["cst"], dtype=np.float64))
    return {"loglike": ll, "chain_loglike": cl, "neff": ne, "n": n, "bad": bad}


def bounds(rows, tables, maxbins):
    """(delta [K], slack): delta_k = (Ju + 16) 2^-52 T_k, the per-sample bound of
    the streaming test, and slack = n 2^-52 for the re-ordered sum of n weights.
    |d loglike|, |d chain_loglike| <= delta + slack; |d neff| <= neff (4 delta +
    2 slack)."""
    Ju = len(tables["cols"])
    return (Ju + 16) * 2.0 ** -52 * R.term_bound(rows, tables, maxbins), rows.shape[0] * 2.0 ** -52
