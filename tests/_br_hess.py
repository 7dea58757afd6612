"""Test-side restatement of the Blackwell-Rao likelihood Hessian
(gibbssampler_amd/csrc/gs_brh.hip, engine.br_likelihood_hess), numpy longdouble, on
tests/_br_grad.py.

From rows [T, C, nsb] and the tables of engine.br_likelihood_tables, with the
weights w = exp(t - M) of _br_grad.weights (t of _br_samples.terms, NaN rows left
out) and xbar its weighted mean:
    u[c, i, j]    = x[c, i, j] - xbar[k, j]                   (longdouble)
    cov[k, a, b]  = sum_ci w u_a u_b / sum_ci w               d^2 loglike_k / dY_ka dY_kb
    abar2[k, a, b] = sum_ci w |u_a| |u_b| / sum_ci w          (the magnitude the error scales with)
    neff[k]       = (sum w)^2 / sum w^2
All sums run over every (chain, row) at once.  hessian() is the chain rule to the
theory spectra in longdouble, J written out from the tables' Y_TT = EE / (2 det),
Y_EE = TT / (2 det), Y_TE = -TE / det."""
import numpy as np

from tests import _br_grad as G
from tests import _br_likelihood as R
from tests import _br_samples as B

LD = np.longdouble
EPS = 2.0 ** -52


def moments(rows, tables, maxbins):
    """{xbar [K, Ju], cov, abar2 [K, Ju, Ju], neff [K]} fp64, cov_ld and xbar_ld the
    longdouble values, of rows [T, C, nsb]; ref: _br_grad.weights' dict."""
    T, C = rows.shape[:2]
    ref = G.weights(rows, tables, maxbins)
    t, _ = B.terms(rows, tables, maxbins)                      # [C, T, K]
    K = t.shape[2]
    x = np.stack([[R.row_parts(rows[i, c], tables, maxbins)[1] for i in range(T)] for c in range(C)]).astype(LD)
    good = ~np.isnan(t[:, :, 0])
    Ju = x.shape[2]
    if not good.any():
        nan = np.full((K, Ju, Ju), np.nan)
        return {"ref": ref, "xbar": ref["xbar"], "cov": nan, "abar2": nan.copy(), "neff": np.full(K, np.nan),
                "cov_ld": nan.astype(LD), "xbar_ld": ref["xbar"].astype(LD)}
    tg, xg = t[good], x[good]                                  # [N, K], [N, Ju]
    w = np.exp(tg - tg.max(axis=0)[None, :])
    den = w.sum(axis=0)
    xbar = (w.T @ xg) / den[:, None]
    cov = np.empty((K, Ju, Ju), dtype=LD)
    abar2 = np.empty((K, Ju, Ju), dtype=LD)
    for k in range(K):
        u = xg - xbar[k][None, :]
        wu = w[:, k][:, None] * u
        cov[k] = (wu.T @ u) / den[k]
        abar2[k] = (np.abs(wu).T @ np.abs(u)) / den[k]
    neff = den * den / (w * w).sum(axis=0)
    return {"ref": ref, "xbar": xbar.astype(np.float64), "cov": cov.astype(np.float64),
            "abar2": abar2.astype(np.float64), "neff": neff.astype(np.float64), "cov_ld": cov, "xbar_ld": xbar}


def cov_bound(rows, tables, maxbins):
    """bc [K]: |d cov_kab| <= bc_k abar2_kab.  The gradient's bound (_br_grad.xbar_bound)
    with the product of two centred columns in place of one column: a relative 2
    delta_k on every weight, 2 C n 2^-52 for the products and their sums in any order,
    and 32 2^-52 for the two rounded subtractions of the centre, the weight's product,
    the per-chain merge, the final sum and the division."""
    T, C = rows.shape[:2]
    delta, _ = B.bounds(rows, tables, maxbins)
    return 2 * delta + (2 * C * T + 32) * EPS


def _blocks(F, bins, mask, cols, maxbins):
    """[(n_b, [j]) for an inverse-Gamma bin, (n_b, [jTT, jEE, jTE]) for a TEB block]."""
    from gibbssampler_amd.engine import SPECTRA
    pos = {int(c): j for j, c in enumerate(cols)}
    out = []
    for sp, s in enumerate(SPECTRA[F]):
        e = np.asarray(bins[s], dtype=np.float64)
        for b in range(maxbins):
            if sp * maxbins + b not in pos:
                continue
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if F == 3 and s != "BB":
                if s == "TT":
                    out.append((n_b, [pos[b], pos[maxbins + b], pos[3 * maxbins + b]]))
            else:
                out.append((n_b, [pos[sp * maxbins + b]]))
    return out


BASIS = np.array([[[1.0, 0.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 1.0]], [[0.0, 1.0], [1.0, 0.0]]]).astype(LD)


def _tr(a, b):
    return np.sum(a * b.T)


def chain_rule(F, bins, theory, mask, cols, xbar, cov, dxbar=None, dcov=None):
    """(H, mag) [K, Ju, Ju] longdouble: H = J^T cov J + L, and mag = |J|^T |cov| |J| +
    (L's formula with every product in absolute value), the magnitude of H's terms.
    With dxbar [K, Ju] and dcov [K, Ju, Ju] (entrywise bounds on xbar and cov) H is
    instead the bound |J|^T dcov |J| + |dL| pushed through entrywise."""
    K, nspec, maxbins = theory.shape
    Ju = len(cols)
    flat = np.asarray(theory, dtype=np.float64).reshape(K, -1)[:, cols].astype(LD)     # D of parameter j
    xbar, cov = np.asarray(xbar).astype(LD), np.asarray(cov).astype(LD)
    bound = dxbar is not None
    H = np.zeros((K, Ju, Ju), dtype=LD)
    mag = np.zeros((K, Ju, Ju), dtype=LD)
    for k in range(K):
        J = np.zeros((Ju, Ju), dtype=LD)
        L = np.zeros((Ju, Ju), dtype=LD)
        La = np.zeros((Ju, Ju), dtype=LD)
        dL = np.zeros((Ju, Ju), dtype=LD)
        for n_b, idx in _blocks(F, bins, mask, cols, maxbins):
            if len(idx) == 1:
                j = idx[0]
                D = flat[k, j]
                J[j, j] = -1 / (D * D)
                L[j, j] = (LD(n_b) / 2) / (D * D) - 2 * xbar[k, j] / D ** 3
                La[j, j] = (LD(n_b) / 2) / (D * D) + 2 * abs(xbar[k, j]) / abs(D) ** 3
                if bound:
                    dL[j, j] = 2 * dxbar[k, j] / abs(D) ** 3
                continue
            tt, ee, te = flat[k, idx[0]], flat[k, idx[1]], flat[k, idx[2]]
            det = tt * ee - te * te
            d2 = det * det
            # rows Y_TT, Y_EE, Y_TE; columns d / dTT, d / dEE, d / dTE
            Jb = np.array([[-ee * ee / (2 * d2), -te * te / (2 * d2), ee * te / d2],
                           [-te * te / (2 * d2), -tt * tt / (2 * d2), tt * te / d2],
                           [te * ee / d2, te * tt / d2, -(tt * ee + te * te) / d2]], dtype=LD)
            J[np.ix_(idx, idx)] = Jb
            Di = np.array([[ee, -te], [-te, tt]], dtype=LD) / det
            Psi = np.array([[xbar[k, idx[0]], xbar[k, idx[2]]], [xbar[k, idx[2]], xbar[k, idx[1]]]], dtype=LD)
            aDi, aPsi = np.abs(Di), np.abs(Psi)
            if bound:
                dPsi = np.array([[dxbar[k, idx[0]], dxbar[k, idx[2]]], [dxbar[k, idx[2]], dxbar[k, idx[1]]]], dtype=LD)
            for u in range(3):
                for v in range(3):
                    uv = Di @ BASIS[u] @ Di @ BASIS[v]
                    vu = Di @ BASIS[v] @ Di @ BASIS[u]
                    M = (uv + vu) @ Di
                    L[idx[u], idx[v]] = -_tr(M, Psi) / 2 + (LD(n_b) / 2) * np.trace(uv)
                    auv = aDi @ BASIS[u] @ aDi @ BASIS[v]
                    avu = aDi @ BASIS[v] @ aDi @ BASIS[u]
                    La[idx[u], idx[v]] = _tr((auv + avu) @ aDi, aPsi) / 2 + (LD(n_b) / 2) * np.trace(auv)
                    if bound:
                        dL[idx[u], idx[v]] = _tr(np.abs(M), dPsi) / 2
        aJ = np.abs(J)
        mag[k] = aJ.T @ np.abs(cov[k]) @ aJ + La
        H[k] = (aJ.T @ np.asarray(dcov[k]).astype(LD) @ aJ + dL) if bound else (J.T @ cov[k] @ J + L)
    return H, mag


def hessian(F, bins, theory, mask, cols, xbar, cov):
    """The longdouble Hessian in D [K, Ju, Ju] and the magnitude of its terms."""
    return chain_rule(F, bins, theory, mask, cols, xbar, cov)


def hessian_bound(F, bins, theory, mask, cols, xbar, cov, dxbar, dcov):
    """|d hess| [K, Ju, Ju] for |d xbar| <= dxbar and |d cov| <= dcov entrywise: the
    device's errors pushed through J and L, plus 64 2^-52 of the magnitude of H's
    terms for the fp64 chain rule itself (each entry is a sum of at most 9 products of
    three factors and L's few terms, every factor a handful of rounded operations)."""
    b, _ = chain_rule(F, bins, theory, mask, cols, xbar, cov, dxbar, dcov)
    _, mag = chain_rule(F, bins, theory, mask, cols, xbar, cov)
    return (b + 64 * EPS * mag).astype(np.float64)
