"""Test-side restatement of the streaming Blackwell-Rao likelihood
(gibbssampler_amd/csrc/gs_brl.hip), numpy.

tables = engine.br_likelihood_tables(...): cols, kind, coef [Ju], Y [K, Ju],
cst [K].  A row is the scale ring's [nsb] values of one (iteration, chain);
x_j = row[cols[j]].

update, per (chain, model) in iteration order:
    arg_j = x_j (kind 1) or a dd - c^2 of the block (kind 2: a = x_j, dd and c
            at cols[j] + maxbins and cols[j] + 3 maxbins)
    bad row (a kind 1 x <= 0 or not finite, a kind 2 arg <= 0 or not finite):
            skipped for the chain, counted in bad[chain]
    r   = sum_j coef_j log(arg_j),  dot_k = sum_j x_j Y_kj     (both summed in
          longdouble from fp64 logarithms and products formed in longdouble:
          the restatement's own summation error is negligible)
    t   = r - dot_k
    S == 0:  m = t, S = 1, Q = 1
    else     d = t - m, w = exp(-|d|);  d > 0: S = S w + 1, Q = Q w^2 + 1, m = t
                                        else   S = S + w,   Q = Q + w^2
finish, per model over the chains with S > 0 in chain order, n iterations:
    M = max m_c;  s = sum S_c e^(m_c - M);  q = sum Q_c e^(2 (m_c - M))
    loglike = ((M + log s) - log(C n)) + cst
    chain_loglike[c] = ((m_c + log S_c) - log n) + cst
    neff = s^2 / q
NaN for n == 0 or no chain with a sample.
"""
import numpy as np

LD = np.longdouble


class State:
    def __init__(self, nchains, K):
        self.m = np.zeros((nchains, K))
        self.S = np.zeros((nchains, K))
        self.Q = np.zeros((nchains, K))
        self.bad = np.zeros(nchains, dtype=np.int64)
        self.n = 0


def row_parts(row, tables, maxbins):
    """(ok, x [Ju], lg [Ju]) of one ring row [nsb]: lg = log(arg) where kind != 0."""
    cols, kind = np.asarray(tables["cols"], dtype=np.int64), np.asarray(tables["kind"])
    x = row[cols]
    arg = np.ones_like(x)
    k1, k2 = kind == 1, kind == 2
    arg[k1] = x[k1]
    if k2.any():
        dd, c = row[cols[k2] + maxbins], row[cols[k2] + 3 * maxbins]
        with np.errstate(all="ignore"):
            arg[k2] = x[k2] * dd - c * c
    live = k1 | k2
    ok = bool(np.all((arg[live] > 0) & np.isfinite(arg[live])))
    lg = np.zeros_like(x)
    if ok:
        lg[live] = np.log(arg[live])
    return ok, x, lg


def update(st, rows, tables, maxbins):
    """Add rows [T, C, nsb] (iteration order) to st."""
    coef, Y = np.asarray(tables["coef"]).astype(LD), np.asarray(tables["Y"]).astype(LD)
    T, C = rows.shape[:2]
    for i in range(T):
        for c in range(C):
            ok, x, lg = row_parts(rows[i, c], tables, maxbins)
            if not ok:
                st.bad[c] += 1
                continue
            r = np.sum(coef * lg.astype(LD))
            t = (r - Y @ x.astype(LD)).astype(np.float64)
            for k in range(t.shape[0]):
                if st.S[c, k] == 0.0:
                    st.m[c, k], st.S[c, k], st.Q[c, k] = t[k], 1.0, 1.0
                    continue
                d = t[k] - st.m[c, k]
                w = np.exp(-abs(d))
                if d > 0:
                    st.S[c, k] = st.S[c, k] * w + 1.0
                    st.Q[c, k] = st.Q[c, k] * (w * w) + 1.0
                    st.m[c, k] = t[k]
                else:
                    st.S[c, k] += w
                    st.Q[c, k] += w * w
    st.n += T
    return st


def finish(m, S, Q, n, cst):
    """m, S, Q [C, K] -> (loglike [K], chain_loglike [C, K], neff [K])."""
    C, K = m.shape
    has = S > 0
    with np.errstate(all="ignore"):
        M = np.where(has, m, -np.inf).max(axis=0)
        s, q = np.zeros(K), np.zeros(K)
        for c in range(C):
            e = np.exp(m[c] - M)
            s = np.where(has[c], s + S[c] * e, s)
            q = np.where(has[c], q + Q[c] * (e * e), q)
        ll = ((M + np.log(s)) - np.log(float(C) * float(n))) + cst
        cl = ((m + np.log(S)) - np.log(float(n))) + cst[None, :]
        ne = (s * s) / q
    none = ~has.any(axis=0) | (n == 0)
    return np.where(none, np.nan, ll), np.where(~has | (n == 0), np.nan, cl), np.where(none, np.nan, ne)


def term_bound(rows, tables, maxbins):
    """T_k [K] = max over the (good) rows and chains of sum_j (|coef_j log arg_j|
    + |x_j| |Y_kj|), plus |cst_k|: the magnitudes whose rounding sets the error."""
    coef, Y, cst = (np.asarray(tables[k], dtype=np.float64) for k in ("coef", "Y", "cst"))
    best = np.zeros(Y.shape[0])
    for i in range(rows.shape[0]):
        for c in range(rows.shape[1]):
            ok, x, lg = row_parts(rows[i, c], tables, maxbins)
            if ok:
                best = np.maximum(best, np.sum(np.abs(coef * lg)) + np.abs(Y) @ np.abs(x))
    return best + np.abs(cst)


def synthetic(F, bins, K, T, C, seed, mask=None):
    """A synthetic scale history and theory set for the bins {spectrum: edges}:
    rows [T, C, nspec, maxbins] (inverse-Gamma scales near alpha D, TEB blocks
    Psi near nu D with a random correlation; NaN in every column that is not
    used), theory [K, nspec, maxbins] (a fiducial times per-model, per-bin
    factors around 1; model 1 has TE of the opposite sign) and the used mask."""
    from gibbssampler_amd.engine import SPECTRA, br_likelihood_mask
    spectra = SPECTRA[F]
    rng = np.random.default_rng(seed)
    drawn = br_likelihood_mask(F, bins)
    mask = drawn if mask is None else (np.asarray(mask, dtype=bool) & drawn)
    nspec, maxbins = drawn.shape
    fid = 10.0 ** rng.uniform(-2, 3, size=(nspec, maxbins))
    rho0 = rng.uniform(-0.6, 0.6, size=maxbins)
    theory = fid[None] * np.exp(0.3 * rng.normal(size=(K, nspec, maxbins)) / np.sqrt(np.arange(K) + 1.0)[:, None, None])
    rows = np.full((T, C, nspec, maxbins), np.nan)
    jit = lambda n_b: 1.0 + rng.normal(size=(T, C)) / np.sqrt(n_b)
    for sp, s in enumerate(spectra):
        e = np.asarray(bins[s], dtype=np.float64)
        for b in np.flatnonzero(mask[sp]):
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if F == 3 and s != "BB":
                if s != "TT":
                    continue
                theory[:, 3, b] = rho0[b] * np.sqrt(theory[:, 0, b] * theory[:, 1, b]) * rng.uniform(0.5, 1.0, size=K)
                if K > 1:
                    theory[1, 3, b] *= -1.0
                a, dd = n_b * fid[0, b] * np.abs(jit(n_b)), n_b * fid[1, b] * np.abs(jit(n_b))
                rows[:, :, 0, b], rows[:, :, 1, b] = a, dd
                rows[:, :, 3, b] = np.sqrt(a * dd) * np.clip(rho0[b] + 0.1 * rng.normal(size=(T, C)), -0.9, 0.9)
            else:
                rows[:, :, sp, b] = (0.5 * n_b) * fid[sp, b] * np.abs(jit(n_b)) + 1e-6 * fid[sp, b]
    return rows, theory, mask


def from_device(fields):
    """engine.BlackwellRaoLikelihood.fields() [3, C, K] (numpy) -> (m, S, Q)."""
    return fields[0], fields[1], fields[2]
