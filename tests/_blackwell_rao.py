"""Test-side restatement of the streaming Blackwell-Rao accumulator
(gibbssampler_amd/csrc/gs_br.hip), numpy fp64.

An element is one (chain, series, grid point); a series is one (spectrum,
bin).  With alpha the series' shape, D_g its grid and beta_i the scale row i
records (halved where `half` is set: the TEB block's Psi_ii / 2):

update, per element in iteration order (rows with beta <= 0 or not finite are
skipped and counted; series with alpha = NaN are never touched):
    rD = 1 / D_g
    t  = alpha * log(beta_i) - beta_i * rD
    S == 0:  m = t, S = 1
    else     d = t - m,  w = exp(-|d|);  d > 0:  S = S * w + 1, m = t;  else  S = S + w
(the device fuses -beta_i * rD into the product's sum and S * w + 1 into one
rounding each; numpy rounds twice, which the comparison's tolerance covers).

finish, per (series, g) over the C chains in chain order, chains with S == 0
left out, n the iterations added:
    M      = max_c m_c
    sum    = sum_c S_c exp(m_c - M)
    logpdf = (((M + log sum) - log(C n)) - lgamma(alpha)) - (alpha + 1) log D_g
    mass   = sum_{g < G - 1} 0.5 (exp(logpdf_g) + exp(logpdf_g+1)) (D_g+1 - D_g)     in g order
NaN where alpha is NaN, n == 0 or no chain has a sample.
"""
import numpy as np
from scipy.special import gammaln


class State:
    def __init__(self, nchains, nsb, G):
        self.m = np.zeros((nchains, nsb, G))
        self.S = np.zeros((nchains, nsb, G))
        self.bad = np.zeros((nchains, nsb), dtype=np.int64)
        self.n = 0


def betas_of(rows, half=None):
    """rows [T, C, nsb] recorded scales -> the conditionals' scales."""
    b = np.array(rows, dtype=np.float64)
    if half is not None:
        b[..., np.asarray(half, dtype=bool)] *= 0.5
    return b


def update(st, rows, alpha, grid, half=None):
    """Add rows [T, C, nsb] (iteration order) to st; alpha [nsb], grid [nsb, G]."""
    beta = betas_of(rows, half)
    active = ~np.isnan(alpha)
    rD = 1.0 / grid
    with np.errstate(all="ignore"):
        for i in range(beta.shape[0]):
            b = beta[i]                                          # [C, nsb]
            ok = active[None, :] & (b > 0) & np.isfinite(b)
            st.bad += (active[None, :] & ~ok).astype(np.int64)
            lb = np.log(np.where(ok, b, 1.0))
            t = (alpha[None, :] * lb)[:, :, None] - b[:, :, None] * rD[None]
            okg = np.broadcast_to(ok[:, :, None], t.shape)
            first = okg & (st.S == 0.0)
            d = t - st.m
            w = np.exp(-np.abs(d))
            up = okg & ~first & (d > 0)
            dn = okg & ~first & ~(d > 0)
            S = np.where(first, 1.0, np.where(up, st.S * w + 1.0, np.where(dn, st.S + w, st.S)))
            st.m = np.where(first | up, t, st.m)
            st.S = S
    st.n += beta.shape[0]
    return st


def finish(m, S, n, alpha, grid):
    """m, S [C, nsb, G] -> (logpdf [nsb, G], mass [nsb])."""
    C, nsb, G = m.shape
    has = S > 0
    with np.errstate(all="ignore"):
        M = np.where(has, m, -np.inf).max(axis=0)
        tot = np.zeros((nsb, G))
        for c in range(C):
            tot = np.where(has[c], tot + S[c] * np.exp(m[c] - M), tot)
        lp = (((M + np.log(tot)) - np.log(float(C) * float(n))) - gammaln(alpha)[:, None]) \
            - (alpha[:, None] + 1.0) * np.log(grid)
        lp = np.where(np.isnan(alpha)[:, None] | ~has.any(axis=0) | (n == 0), np.nan, lp)
    return lp, trapezoid_mass(lp, grid)


def trapezoid_mass(lp, grid):
    """The finish's mass [nsb] of logpdf [nsb, G] (g order; NaN for a NaN series)."""
    with np.errstate(all="ignore"):
        mass = np.where(np.isnan(lp[:, 0]), np.nan, 0.0)
        p = np.exp(lp)
        for g in range(lp.shape[1] - 1):
            mass = mass + (0.5 * (p[:, g] + p[:, g + 1])) * (grid[:, g + 1] - grid[:, g])
    return mass


def term_bound(rows, alpha, grid, half=None):
    """max over the rows and chains of max(alpha |log beta|, beta / D, |lgamma
    alpha| + (alpha + 1) |log D|) per (series, g): the magnitudes whose rounding
    sets the error of logpdf."""
    beta = betas_of(rows, half)
    with np.errstate(all="ignore"):
        ok = (beta > 0) & np.isfinite(beta)
        lb = np.abs(np.log(np.where(ok, beta, 1.0)))
        t1 = (alpha[None, None, :] * lb).max(axis=(0, 1))[:, None] * np.ones_like(grid)
        t2 = np.where(ok, beta, 0.0).max(axis=(0, 1))[:, None] / grid
        t3 = np.abs(gammaln(alpha))[:, None] + (alpha[:, None] + 1.0) * np.abs(np.log(grid))
    return np.maximum(np.maximum(t1, t2), t3)


def from_device(fields, nsb, G):
    """engine.BlackwellRaoState.fields() [2, C, nsb * G] (numpy) -> (m, S) [C, nsb, G]."""
    C = fields.shape[1]
    return fields[0].reshape(C, nsb, G), fields[1].reshape(C, nsb, G)
