"""Test-side restatement of the Gaussianised Blackwell-Rao likelihood
(gibbssampler_amd/csrc/gs_gbr.hip, engine.GaussianizedBlackwellRao), numpy with
longdouble sums and scipy, in the device's definitions:

  marginals   logp[j, g] = log 1/N sum_ci IG(D_g; alpha_j, beta_cij), lD_g = glo_j + g gh_j
  tables      the cumulative trapezoid of exp(logp + lD) in log D from both sides,
              x_g = ppf(FL / mass) where FL / mass <= 1/2, else -ppf(FR / mass),
              sx_g = h exp(lD + logp - log mass + x^2 / 2 + log(2 pi) / 2),
              sp_g = (logp_{g+1} - logp_{g-1}) / 2 (one-sided at the ends)
  transform   u = (log D - glo) / gh, k = floor(u) in [1, G - 3], t = u - k, the cubic
              Hermite through nodes k, k + 1; outside unless 1 <= u <= G - 2
  moments     cnt_c, S1_c = sum_i x_i, S2_c = sum_i x_i x_i^T over the rows whose r is
              not NaN
  finish      N, mu = S1 / N, cov = (S2 - N mu mu^T) / (N - 1)
  loglike     sum_j logp_j - (x - mu)^T cov^-1 (x - mu) / 2 + x^T x / 2 - log det cov / 2
No running state and no order: every sum runs in longdouble."""
import numpy as np
from scipy import special, stats

LD = np.longdouble
EPS = 2.0 ** -52


def nodes(glo, gh, G):
    """lD [Jg, G] longdouble."""
    return np.asarray(glo, dtype=LD)[:, None] + np.arange(G, dtype=LD)[None, :] * np.asarray(gh, dtype=LD)[:, None]


def marginals(beta, good, alpha, glo, gh, G):
    """logp [Jg, G] (longdouble) of beta [C, n, Jg] (the conditional's scales),
    good [C, n]; and the largest |term| per (j, g) for the bounds."""
    b = np.asarray(beta, dtype=LD)[np.asarray(good, dtype=bool)]          # [N, Jg]
    N = b.shape[0]
    a = np.asarray(alpha, dtype=LD)
    lD = nodes(glo, gh, G)
    lb = np.log(b)
    logp = np.empty(lD.shape, dtype=LD)
    tmax = np.empty(lD.shape)
    for j in range(lD.shape[0]):
        t = a[j] * lb[:, j, None] - b[:, j, None] * np.exp(-lD[j])[None, :]          # [N, G]
        m = t.max(axis=0)
        logp[j] = m + np.log(np.sum(np.exp(t - m[None, :]), axis=0)) - np.log(LD(N)) \
            - LD(special.gammaln(float(a[j]))) - (a[j] + 1) * lD[j]
        tmax[j] = (np.abs(a[j] * lb[:, j, None]) + b[:, j, None] * np.exp(-lD[j])[None, :]).max(axis=0)
    return logp, tmax, N


def logp_bound(tmax, N, alpha, glo, gh, G, nmax):
    """|d logp| <= 2^-52 (16 (T + |lgamma(alpha)| + (alpha + 1) |lD| + log N) + n): T the
    largest |alpha log beta| + beta / D_g of the column (each term of t, the rounding
    of exp(-lD), log beta and the fma: 16 units of it cover them with room), the
    finish's three subtractions in units of their operands, and n 2^-52 for the
    re-ordered sum of a chain's n weights and of the chains."""
    lD = np.abs(nodes(glo, gh, G).astype(np.float64))
    a = np.asarray(alpha, dtype=np.float64)[:, None]
    return EPS * (16 * (tmax + np.abs(special.gammaln(a)) + (a + 1) * lD + np.log(N)) + nmax)


def tables(logp, glo, gh):
    """(x, sx, sp [Jg, G], mass [Jg]) float64 from logp [Jg, G]."""
    lp = np.asarray(logp, dtype=LD)
    Jg, G = lp.shape
    lD = nodes(glo, gh, G)
    h = np.asarray(gh, dtype=LD)[:, None]
    q = np.exp(lp + lD)
    cell = 0.5 * (q[:, :-1] + q[:, 1:]) * h
    FL = np.concatenate([np.zeros((Jg, 1), dtype=LD), np.cumsum(cell, axis=1)], axis=1)
    FR = np.concatenate([np.cumsum(cell[:, ::-1], axis=1)[:, ::-1], np.zeros((Jg, 1), dtype=LD)], axis=1)
    mass = FL[:, -1]
    fl, fr = (FL / mass[:, None]).astype(np.float64), (FR / mass[:, None]).astype(np.float64)
    with np.errstate(all="ignore"):
        x = np.where(fl <= 0.5, stats.norm.ppf(fl), -stats.norm.ppf(fr))
        ls = lD + lp - np.log(mass)[:, None] + 0.5 * x.astype(LD) ** 2 + LD(0.5) * np.log(2 * LD(np.pi))
        sx = np.where(np.isfinite(x), (h * np.exp(ls)).astype(np.float64), 0.0)
    sp = np.empty((Jg, G), dtype=LD)
    sp[:, 1:-1] = 0.5 * (lp[:, 2:] - lp[:, :-2])
    sp[:, 0], sp[:, -1] = lp[:, 1] - lp[:, 0], lp[:, -1] - lp[:, -2]
    return x, sx, sp.astype(np.float64), mass.astype(np.float64)


def hermite(y0, s0, y1, s1, t):
    t = np.asarray(t, dtype=LD)
    y0, s0, y1, s1 = (np.asarray(v, dtype=LD) for v in (y0, s0, y1, s1))
    return (1 + 2 * t) * (1 - t) ** 2 * y0 + t * (1 - t) ** 2 * s0 + t * t * (3 - 2 * t) * y1 + t * t * (t - 1) * s1


def transform(D, glo, gh, tab):
    """(value [.., Jg] longdouble, inside [.., Jg], err [.., Jg]) of D [.., Jg] through
    tab [Jg, G, 2] = (node value, node slope per cell).  err bounds a device value
    computed from the same table:
      2^-52 (4 (|log D| + |glo|) / gh (1.5 |y1 - y0| + |s0| + |s1|) + 8 (|y0| + |s0| + |y1| + |s1|)):
    u's rounding (the logarithm, the subtraction and the product, 4 units of
    their magnitudes) times the largest slope of the cubic in t, and the
    Hermite's own ten operations in units of its terms."""
    D = np.asarray(D, dtype=np.float64)
    tab = np.asarray(tab, dtype=np.float64)
    G = tab.shape[1]
    with np.errstate(all="ignore"):
        lD = np.log(D.astype(LD))
        u = (lD - np.asarray(glo, dtype=LD)) / np.asarray(gh, dtype=LD)
        inside = (u >= 1) & (u <= G - 2)
    k = np.clip(np.floor(np.where(inside, u, 1)).astype(np.int64), 1, G - 3)
    t = np.where(inside, u - k, 0)
    j = np.broadcast_to(np.arange(tab.shape[0]), k.shape)
    y0, s0, y1, s1 = tab[j, k, 0], tab[j, k, 1], tab[j, k + 1, 0], tab[j, k + 1, 1]
    inside = inside & np.isfinite(y0) & np.isfinite(y1)      # a cell with an infinite node is not usable
    t = np.where(inside, t, 0)
    y0, s0, y1, s1 = (np.where(inside, v, 0.0) for v in (y0, s0, y1, s1))
    val = hermite(y0, s0, y1, s1, t)
    with np.errstate(all="ignore"):
        err = EPS * (4 * (np.abs(lD) + np.abs(glo)).astype(np.float64) / np.asarray(gh) *
                     (1.5 * np.abs(y1 - y0) + np.abs(s0) + np.abs(s1)) +
                     8 * (np.abs(y0) + np.abs(s0) + np.abs(y1) + np.abs(s1)))
    return val, inside, np.where(inside, err, 0.0)


def moments(x, good):
    """(cnt [C], S1 [C, Jg], S2 [C, Jg, Jg]) longdouble of x [C, n, Jg], good [C, n]."""
    x = np.asarray(x, dtype=LD)
    C, n, Jg = x.shape
    cnt = np.zeros(C, dtype=np.int64)
    S1, S2 = np.zeros((C, Jg), dtype=LD), np.zeros((C, Jg, Jg), dtype=LD)
    for c in range(C):
        xc = x[c][np.asarray(good[c], dtype=bool)]
        cnt[c] = xc.shape[0]
        S1[c] = xc.sum(axis=0)
        S2[c] = xc.T @ xc
    return cnt, S1, S2


def finish(cnt, S1, S2):
    """(N, mu [Jg], cov [Jg, Jg]) longdouble."""
    N = int(np.sum(cnt))
    s1, s2 = np.asarray(S1, dtype=LD).sum(axis=0), np.asarray(S2, dtype=LD).sum(axis=0)
    mu = s1 / N
    return N, mu, (s2 - N * np.outer(mu, mu)) / (N - 1)


def loglike(D, glo, gh, tx, tp, mu, cov):
    """{loglike, marginal, outside [K], x, xerr [K, Jg]} of D [K, Jg] (the theory at the
    fit's columns); the solve in float64 (numpy has no longdouble solver), the sums
    in longdouble."""
    x, inside, xerr = transform(D, glo, gh, tx)
    lp, _, lperr = transform(D, glo, gh, tp)
    outside = (~inside).sum(axis=1)
    x = np.where(inside, x, 0)
    lp = np.where(inside, lp, 0)
    marginal = lp.sum(axis=1)
    cov = np.asarray(cov, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    d = x.astype(np.float64) - mu[None, :]
    sol = np.linalg.solve(cov, d.T).T
    q1 = np.sum(d.astype(LD) * sol.astype(LD), axis=1)
    q2 = np.sum(x * x, axis=1)
    sign, logdet = np.linalg.slogdet(cov)
    ll = marginal + 0.5 * (q2 - q1) - 0.5 * LD(logdet)
    ll = np.where(outside > 0, -np.inf, ll.astype(np.float64))
    return {"loglike": ll, "marginal": marginal.astype(np.float64), "outside": outside, "x": x.astype(np.float64),
            "xerr": xerr, "lperr": lperr, "grad_x": x.astype(np.float64) - sol, "q1": q1.astype(np.float64),
            "q2": q2.astype(np.float64)}


def loglike_bound(ref, cov):
    """|d loglike| of a device value from the same tables, mu and factor:
      sum_j lperr_j + sum_j |x_j - (cov^-1 (x - mu))_j| xerr_j
        + 2^-52 (8 Jg cond(cov) q1 + (Jg + 8) (q1 + q2 + |marginal| + |log det cov|)):
    the Hermite values' own bounds carried through the gradient of the form, the
    triangular solve (backward stable: Jg units times the condition number of the
    covariance on the quadratic form) and the sums of Jg terms."""
    cov = np.asarray(cov, dtype=np.float64)
    Jg = cov.shape[0]
    cond = np.linalg.cond(cov)
    _, logdet = np.linalg.slogdet(cov)
    return ref["lperr"].sum(axis=1) + (np.abs(ref["grad_x"]) * ref["xerr"]).sum(axis=1) + \
        EPS * (8 * Jg * cond * ref["q1"] + (Jg + 8) * (ref["q1"] + ref["q2"] + np.abs(ref["marginal"]) + abs(logdet)))
