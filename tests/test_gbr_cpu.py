"""CPU: the numpy restatement of the Gaussianised Blackwell-Rao likelihood
(tests/_gbr.py) against scipy's closed forms, and the host side of the feature:
the options of run(br_samples=), the column selection and the finish."""
import numpy as np
import pytest
from scipy import stats

from tests import _gbr as GB
from tests.test_br_samples_cpu import bins_of

from gibbssampler_amd.engine import GBR_SPAN as SPAN  # noqa: E402


def one_row(alpha, beta, G, dmin, dmax):
    """The grid and the restated tables of one bank row per chain, all beta equal:
    the marginal is the inverse-Gamma itself."""
    from gibbssampler_amd.engine import gbr_grid
    alpha, beta = np.atleast_1d(alpha).astype(float), np.atleast_1d(beta).astype(float)
    glo, gh = gbr_grid(np.atleast_1d(dmin), np.atleast_1d(dmax), G, *SPAN)
    b = np.broadcast_to(beta, (3, 1, len(alpha)))
    logp, tmax, N = GB.marginals(b, np.ones((3, 1), dtype=bool), alpha, glo, gh, G)
    return glo, gh, logp, N


def test_marginal_is_invgamma():
    alpha, beta = np.array([1.5, 7.0, 40.5]), np.array([3.0, 20.0, 900.0])
    mode = beta / (alpha + 1)
    glo, gh, logp, N = one_row(alpha, beta, 64, 0.7 * mode, 1.4 * mode)
    assert N == 3
    D = np.exp(GB.nodes(glo, gh, 64).astype(np.float64))
    want = stats.invgamma.logpdf(D, alpha[:, None], scale=beta[:, None])
    assert np.allclose(logp.astype(np.float64), want, rtol=1e-12, atol=0)


def interpolation_error(G):
    """max |x(D) - ppf(cdf(D))| at off-grid D over the draws' range [dmin, dmax] (the 1e-4
    and 1 - 1e-4 quantiles), for shapes from l = 2 (alpha = 1.5) to l = 200, default span."""
    alpha, beta = np.array([1.5, 4.5, 11.5, 40.5, 200.5]), np.array([3.0, 10.0, 30.0, 900.0, 4000.0])
    lo, hi = stats.invgamma.ppf(1e-4, alpha, scale=beta), stats.invgamma.ppf(1 - 1e-4, alpha, scale=beta)
    glo, gh, logp, _ = one_row(alpha, beta, G, lo, hi)
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    tx = np.stack([x, sx], axis=-1)
    D = np.exp(np.linspace(np.log(lo), np.log(hi), 1543))                       # [1543, 5], off the nodes
    got, inside, _ = GB.transform(D, glo, gh, tx)
    assert inside.all()
    # the untruncated closed form: the mass beyond the end nodes is part of the error
    cdf = stats.invgamma.cdf(D, alpha, scale=beta)
    sf = stats.invgamma.sf(D, alpha, scale=beta)
    want = np.where(cdf <= 0.5, stats.norm.ppf(cdf), -stats.norm.ppf(sf))
    return float(np.max(np.abs(got.astype(np.float64) - want))), float(np.max(np.abs(mass - 1)))


def test_interpolation_error_and_default_points():
    """The error of x(D) (grid truncation, trapezoid cumulative and cubic Hermite) at G =
    64, 128, 256: 1.7e-1, 4.7e-2, 1.2e-2 with the default span (0.5, 8), against the
    statistical error of the covariance of the surface case (4 chains x
    200 kept samples: sqrt(2 / 800) = 0.05 on a diagonal entry).  The default G is the
    smallest of the three below it."""
    from gibbssampler_amd.engine import GBR_POINTS
    stat = np.sqrt(2.0 / 800)
    errs = {G: interpolation_error(G) for G in (64, 128, 256)}
    for G, (e, m) in errs.items():
        print(f"  G {G}: max |x - ppf(cdf)| = {e:.3e}, max |mass - 1| = {m:.3e}")
    assert errs[256][0] < errs[128][0] < errs[64][0] and errs[64][0] > stat
    assert GBR_POINTS == min(G for G, (e, _) in errs.items() if e < stat)


def fit_case(seed=5, C=3, n=40, Jg=5):
    rng = np.random.default_rng(seed)
    alpha = np.array([1.5, 2.5, 5.5, 9.5, 17.5])[:Jg]
    beta = rng.gamma(alpha + 3, 1.0, size=(C, n, Jg)) * 10
    D = beta / rng.gamma(alpha, 1.0, size=(C, n, Jg))
    good = np.ones((C, n), dtype=bool)
    good[1, 7] = False
    return alpha, beta, D, good


def test_copula_identity_and_outside():
    from gibbssampler_amd.engine import gbr_grid
    alpha, beta, D, good = fit_case()
    G = 64
    glo, gh = gbr_grid(D[good].min(axis=0), D[good].max(axis=0), G, *SPAN)
    logp, _, N = GB.marginals(beta, good, alpha, glo, gh, G)
    assert N == good.sum()
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    tx, tp = np.stack([x, sx], axis=-1), np.stack([logp.astype(np.float64), sp], axis=-1)
    # every kept draw maps to a finite x; the end nodes do not
    xd, inside, _ = GB.transform(D, glo, gh, tx)
    assert inside[good].all() and np.isfinite(xd[good].astype(np.float64)).all()
    assert np.isinf(x[:, 0]).all() and np.isinf(x[:, -1]).all() and np.isfinite(x[:, 1:-1]).all()
    th = np.median(D[good], axis=0)[None, :] * np.array([[1.0], [1.1]])
    Jg = len(alpha)
    out = GB.loglike(th, glo, gh, tx, tp, np.zeros(Jg), np.eye(Jg))
    assert np.array_equal(out["loglike"], out["marginal"]) and not out["outside"].any()
    # the interval's ends are inside, a hair beyond them is outside: -inf
    lo, hi = np.exp(glo + gh), np.exp(glo + (G - 2) * gh)
    edge = np.stack([th[0], th[0], th[0]])
    edge[0, 2], edge[1, 2], edge[2, 0] = lo[2] * (1 + 1e-9), lo[2] * (1 - 1e-6), hi[0] * (1 + 1e-6)
    cnt, S1, S2 = GB.moments(np.where(good[:, :, None], xd, 0), good)
    N, mu, cov = GB.finish(cnt, S1, S2)
    out = GB.loglike(edge, glo, gh, tx, tp, mu, cov)
    assert list(out["outside"]) == [0, 1, 1] and np.isfinite(out["loglike"][0])
    assert np.isneginf(out["loglike"][1:]).all()
    # the fitted Gaussian is close to standard normal by construction
    assert np.all(np.abs(mu.astype(np.float64)) < 0.5) and np.all(np.abs(np.diag(cov).astype(np.float64) - 1) < 0.5)


def test_finish_raises_without_enough_samples():
    from gibbssampler_amd.engine import gbr_finish
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 6))                                          # N = 6 = Jg
    cnt, S1, S2 = GB.moments(x, np.ones((2, 3), dtype=bool))
    with pytest.raises(ValueError, match="more kept samples than columns"):
        gbr_finish(cnt, S1.astype(np.float64), S2.astype(np.float64))
    x = rng.standard_normal((2, 5, 6))
    x[:, :, 5] = x[:, :, 4]                                                     # N = 10 > Jg, singular
    cnt, S1, S2 = GB.moments(x, np.ones((2, 5), dtype=bool))
    with pytest.raises(ValueError, match="more kept samples than columns"):
        gbr_finish(cnt, S1.astype(np.float64), S2.astype(np.float64))
    x = rng.standard_normal((2, 50, 6))
    cnt, S1, S2 = GB.moments(x, np.ones((2, 50), dtype=bool))
    fit = gbr_finish(cnt, S1.astype(np.float64), S2.astype(np.float64))
    N, mu, cov = GB.finish(cnt, S1, S2)
    assert fit["n"] == N == 100 and np.allclose(fit["mu"], mu.astype(np.float64), rtol=0, atol=1e-14)
    assert np.allclose(fit["cov"], np.cov(x.reshape(100, 6).T), rtol=0, atol=1e-13)
    assert np.allclose(fit["chol"] @ fit["chol"].T, fit["cov"], rtol=0, atol=1e-14)
    assert abs(fit["logdet"] - np.linalg.slogdet(fit["cov"])[1]) < 1e-13


def test_draws_option_and_columns():
    from gibbssampler_amd.engine import br_likelihood_mask, br_likelihood_tables, gbr_columns
    from gibbssampler_amd.samplers import check_br_samples
    bins = bins_of(3)
    got = check_br_samples({"lrange": (2, 8), "draws": True}, 3, bins)
    assert got["draws"] is True and got["start"] is None
    assert check_br_samples({"lrange": (2, 8)}, 3, bins)["draws"] is False
    assert check_br_samples(True, 3, bins)["draws"] is False
    with pytest.raises(ValueError, match="unknown options"):
        check_br_samples({"draws": True, "points": 64}, 3, bins)
    with pytest.raises(ValueError, match="draws must be"):
        check_br_samples({"draws": 1}, 3, bins)
    # F = 3: TE is dropped, TT and EE halve Psi, BB keeps its scale
    mask = br_likelihood_mask(3, bins, None, (2, 8))
    tab = br_likelihood_tables(3, bins, np.ones((1,) + mask.shape) * np.array([2.0, 2.0, 2.0, 0.0])[None, :, None], mask)
    col = gbr_columns(3, bins, mask)
    maxbins = mask.shape[1]
    sp = col["tcol"] // maxbins
    assert len(tab["cols"]) == 16 and len(col["gcol"]) == 11 and 3 not in sp
    assert np.array_equal(tab["cols"][col["gcol"]], col["tcol"])
    assert np.array_equal(col["half"], np.where(sp < 2, 0.5, 1.0))
    for j, c in enumerate(col["tcol"]):
        e = np.asarray(bins[("TT", "EE", "BB", "TE")[c // maxbins]], dtype=float)
        n_b = e[c % maxbins + 1] ** 2 - e[c % maxbins] ** 2
        assert col["alpha"][j] == 0.5 * n_b - (2.0 if c // maxbins < 2 else 1.0)
    # F = 2: every column
    bins2 = bins_of(2)
    mask2 = br_likelihood_mask(2, bins2)
    col2 = gbr_columns(2, bins2, mask2)
    assert len(col2["gcol"]) == mask2.sum() and np.all(col2["half"] == 1.0)
    assert np.array_equal(col2["gcol"], np.arange(mask2.sum()))


def test_narrow_marginal_shrinks_the_interval():
    """alpha = 4000 (a bin 20 multipoles wide near l = 200): the linear cumulatives
    underflow in the far tails of the grid, x is infinite at some inner nodes, and a D
    in such a cell counts as outside -- never a NaN."""
    from gibbssampler_amd.engine import gbr_grid
    rng = np.random.default_rng(11)
    alpha = np.array([4000.0, 40.0])
    beta = rng.gamma(alpha + 3, 1.0, size=(2, 400, 2))
    D = beta / rng.gamma(alpha, 1.0, size=beta.shape)
    good = np.ones((2, 400), dtype=bool)
    G = 64
    glo, gh = gbr_grid(D.min(axis=(0, 1)), D.max(axis=(0, 1)), G, 0.5, 2.0)
    logp, _, _ = GB.marginals(beta, good, alpha, glo, gh, G)
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    assert np.isinf(x[0, 1]) and np.isinf(x[0, G - 2]) and np.isfinite(x[1, 1:-1]).all()
    tx, tp = np.stack([x, sx], axis=-1), np.stack([logp.astype(np.float64), sp], axis=-1)
    xd, inside, _ = GB.transform(D, glo, gh, tx)
    assert inside.all() and np.isfinite(xd.astype(np.float64)).all()          # the kept draws stay usable
    th = np.median(D, axis=(0, 1))[None, :] * np.ones((2, 1))
    th[1, 0] = np.exp(glo[0] + 1.2 * gh[0])                                    # inside [a min D, min D]: a lost cell
    assert 0.5 * D[:, :, 0].min() < th[1, 0] < D[:, :, 0].min()
    cnt, S1, S2 = GB.moments(xd, good)
    N, mu, cov = GB.finish(cnt, S1, S2)
    out = GB.loglike(th, glo, gh, tx, tp, mu, cov)
    assert list(out["outside"]) == [0, 1] and np.isfinite(out["loglike"][0]) and np.isneginf(out["loglike"][1])
