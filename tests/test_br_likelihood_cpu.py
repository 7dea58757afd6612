"""CPU: the tables of the streaming Blackwell-Rao likelihood
(engine.br_likelihood_tables) against scipy's inverse-Gamma and inverse-Wishart
densities, the argument check of run(br_likelihood=...) and the numpy
restatement tests/_br_likelihood.py on its own (cuts of the rows)."""
import numpy as np
import pytest
from scipy.stats import invgamma, invwishart

from gibbssampler_amd.engine import SPECTRA, br_likelihood_mask, br_likelihood_tables
from gibbssampler_amd.samplers import check_br_likelihood
from tests import _br_likelihood as R

BINS_A = np.array([0, 1, 2, 3, 4, 6, 8, 9, 18, 52, 65])      # as tests/test_gpu_blackwell_rao.py
BINS_B = np.array([0, 1, 2, 4, 13, 47, 65])
SEED = 20261021


def bins_of(F):
    return {s: (BINS_B if s == "BB" and F > 1 else BINS_A) for s in SPECTRA[F]}


def scipy_loglike(F, bins, row, theory_k, mask):
    """sum over the used bins of the conditional's log density at theory_k
    ([nspec, maxbins]) for the scales of row ([nspec, maxbins]), per bin."""
    out = {}
    for sp, s in enumerate(SPECTRA[F]):
        e = np.asarray(bins[s], dtype=np.float64)
        for b in np.flatnonzero(mask[sp]):
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if F == 3 and s != "BB":
                if s == "TT":
                    D = np.array([[theory_k[0, b], theory_k[3, b]], [theory_k[3, b], theory_k[1, b]]])
                    Psi = np.array([[row[0, b], row[3, b]], [row[3, b], row[1, b]]])
                    out[(sp, b)] = invwishart.logpdf(D, df=n_b - 3.0, scale=Psi)
            else:
                out[(sp, b)] = invgamma.logpdf(theory_k[sp, b], a=0.5 * n_b - 1.0, scale=row[sp, b])
    return out


def table_loglike(tables, row, maxbins):
    ok, x, lg = R.row_parts(row.reshape(-1), tables, maxbins)
    assert ok
    ld = R.LD
    return (np.sum(tables["coef"].astype(ld) * lg.astype(ld)) - tables["Y"].astype(ld) @ x.astype(ld)
            + tables["cst"].astype(ld)).astype(np.float64)


@pytest.mark.parametrize("F", [1, 2, 3])
def test_tables_against_scipy(F):
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, K=3, T=2, C=1, seed=SEED + F)
    maxbins = mask.shape[1]
    tb = br_likelihood_tables(F, bins, theory, mask)
    assert tb["cols"].dtype == np.int32 and np.all(np.diff(tb["cols"]) > 0) and tb["Y"].shape == (3, len(tb["cols"]))
    assert np.array_equal(tb["cols"], np.flatnonzero(mask.reshape(-1)))
    assert set(np.unique(tb["kind"])) == ({0, 1, 2} if F == 3 else {1})
    # a mask that drops one bin (F = 3: one TEB block) drops exactly that bin's terms
    drop = mask.copy()
    drop[[0, 1, 3] if F == 3 else [0], 4] = False
    tb2 = br_likelihood_tables(F, bins, theory, drop)
    assert len(tb2["cols"]) == len(tb["cols"]) - (3 if F == 3 else 1)
    for i in range(rows.shape[0]):
        got, got2 = table_loglike(tb, rows[i, 0], maxbins), table_loglike(tb2, rows[i, 0], maxbins)
        for k in range(3):
            terms = scipy_loglike(F, bins, rows[i, 0], theory[k], mask)
            want = np.sum(list(terms.values()))
            np.testing.assert_allclose(got[k], want, rtol=1e-12, atol=0, err_msg=f"F {F} row {i} model {k}")
            np.testing.assert_allclose(got2[k], want - terms[(0, 4)], rtol=1e-12, atol=0)


def test_density_is_the_draw():
    """The block's density is that of the draw in cls_draw_body: W ~ Wishart(nu,
    Psi^-1) by Bartlett (chi^2_nu, chi^2_(nu-1), one normal), D = W^-1, nu =
    n_b - 3: the mean of D is Psi / (nu - 3)."""
    rng = np.random.default_rng(SEED)
    nu, Psi = 18.0 ** 2 - 9.0 ** 2 - 3.0, np.array([[5.0, 1.2], [1.2, 0.7]])
    Lc = np.linalg.cholesky(np.linalg.inv(Psi))
    N = 20000
    c1, c2, n = np.sqrt(rng.chisquare(nu, N)), np.sqrt(rng.chisquare(nu - 1.0, N)), rng.normal(size=N)
    B = np.zeros((N, 2, 2))
    B[:, 0, 0], B[:, 1, 0], B[:, 1, 1] = Lc[0, 0] * c1, Lc[1, 0] * c1 + Lc[1, 1] * n, Lc[1, 1] * c2
    D = np.linalg.inv(B @ B.transpose(0, 2, 1))
    np.testing.assert_allclose(D.mean(axis=0), Psi / (nu - 3.0), rtol=5e-3)
    np.testing.assert_allclose(D.mean(axis=0), invwishart.mean(df=nu, scale=Psi), rtol=5e-3)


def test_lrange_mask():
    bins = bins_of(3)
    m = br_likelihood_mask(3, bins)
    assert not m[:, :2].any() and m[0, 2:].all() and m[2, 2:6].all() and not m[2, 6:].any()
    # BINS_A, l ranges of bins 2..9: [2,2] [3,3] [4,5] [6,7] [8,8] [9,17] [18,51] [52,64]
    # BINS_B, bins 2..5:             [2,3] [4,12] [13,46] [47,64]
    m = br_likelihood_mask(3, bins, lrange=(3, 8))                         # BB: [2,3] and [4,12] straddle an end
    assert np.array_equal(np.flatnonzero(m[0]), [3, 4, 5, 6]) and np.array_equal(m[0], m[3]) and not m[2].any()
    m = br_likelihood_mask(3, bins, lrange=(4, 46))
    assert np.array_equal(np.flatnonzero(m[2]), [3, 4]) and np.array_equal(np.flatnonzero(m[0]), [4, 5, 6, 7])
    m = br_likelihood_mask(3, bins, lrange=(5, 20))                        # [4,5] and [18,51] straddle
    assert np.array_equal(np.flatnonzero(m[0]), [5, 6, 7]) and not m[2].any()
    got = check_br_likelihood({"theory": np.ones((1, 4, 10)) * np.array([2.0, 2.0, 1.0, 0.5])[None, :, None],
                               "lrange": (3, 8)}, 3, bins)
    assert np.array_equal(got["mask"], br_likelihood_mask(3, bins, lrange=(3, 8))) and got["K"] == 1
    assert len(got["tables"]["cols"]) == 4 * 3                             # four blocks, no BB bin
    assert check_br_likelihood(None, 3, bins) is None and check_br_likelihood(False, 3, bins) is None


def test_check_refusals():
    bins = bins_of(3)
    good = np.ones((2, 4, 10)) * np.array([2.0, 2.0, 1.0, 0.5])[None, :, None]
    ok = check_br_likelihood({"theory": good, "start": 3}, 3, bins)
    assert ok["K"] == 2 and ok["start"] == 3 and ok["tables"]["Y"].shape[0] == 2
    # the dict form is the array form
    d = {s: good[:, k, :len(bins[s]) - 1] for k, s in enumerate(SPECTRA[3])}
    okd = check_br_likelihood({"theory": d}, 3, bins)
    assert all(np.array_equal(okd["tables"][k], ok["tables"][k]) for k in ok["tables"])
    bad = lambda **kw: pytest.raises(ValueError, match=kw.pop("match"))
    with bad(match="K >= 1"):
        check_br_likelihood({"theory": good[:0]}, 3, bins)
    with bad(match="empty used set"):
        check_br_likelihood({"theory": good, "lrange": (70, 80)}, 3, bins)
    with bad(match="empty used set"):
        check_br_likelihood({"theory": good, "mask": np.zeros((4, 10), dtype=bool)}, 3, bins)
    for v in (0.0, -1.0, np.nan, np.inf):
        t = good.copy()
        t[1, 2, 3] = v                                                     # BB, a used bin
        with bad(match="positive"):
            check_br_likelihood({"theory": t}, 3, bins)
        t = good.copy()
        t[0, 1, 5] = v                                                     # EE of a used block
        with bad(match="positive"):
            check_br_likelihood({"theory": t}, 3, bins)
    t = good.copy()
    t[1, 2, 8] = -1.0                                                      # BB past its bin count: not used
    check_br_likelihood({"theory": t}, 3, bins)
    t = good.copy()
    t[:, :, :2] = -1.0                                                     # bins 0 and 1: not used
    check_br_likelihood({"theory": t}, 3, bins)
    t = good.copy()
    t[1, 3, 4] = 2.0                                                       # TE^2 = TT EE: det = 0
    with bad(match="positive definite"):
        check_br_likelihood({"theory": t}, 3, bins)
    t[1, 3, 4] = -2.5
    with bad(match="positive definite"):
        check_br_likelihood({"theory": t}, 3, bins)
    m = br_likelihood_mask(3, bins)
    m[1, 5] = False                                                        # EE dropped where TT and TE stay
    with bad(match="as a whole"):
        check_br_likelihood({"theory": good, "mask": m}, 3, bins)
    with bad(match="unknown options"):
        check_br_likelihood({"theory": good, "grid": 1}, 3, bins)
    with bad(match="lrange or mask"):
        check_br_likelihood({"theory": good, "mask": m, "lrange": (2, 9)}, 3, bins)
    with bad(match="theory"):
        check_br_likelihood({"lrange": (2, 9)}, 3, bins)
    with bad(match="start"):
        check_br_likelihood({"theory": good, "start": -1}, 3, bins)
    with bad(match=r"\[K, nspec, maxbins\]"):
        check_br_likelihood({"theory": good[:, :3]}, 3, bins)


@pytest.mark.parametrize("F", [2, 3])
def test_restatement_cuts(F):
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, K=3, T=8, C=2, seed=SEED + 10 + F)
    maxbins = mask.shape[1]
    rows[5, 1, -1 if F == 2 else 2, 3] = 0.0                              # a bad row (BB) for chain 1
    tb = br_likelihood_tables(F, bins, theory, mask)
    flat = rows.reshape(8, 2, -1)
    states = []
    for cuts in ((8,), (3, 5), (1,) * 8):
        st, at = R.State(2, 3), 0
        for k in cuts:
            R.update(st, flat[at:at + k], tb, maxbins)
            at += k
        states.append(st)
    a = states[0]
    assert a.n == 8 and np.array_equal(a.bad, [0, 1]) and np.all(a.S >= 1.0) and np.all(a.Q >= 1.0)
    for b in states[1:]:
        assert b.n == 8 and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("m", "S", "Q", "bad"))
    ll, cl, ne = R.finish(a.m, a.S, a.Q, a.n, tb["cst"])
    assert np.all(np.isfinite(ll)) and cl.shape == (2, 3) and np.all((ne >= 1.0) & (ne <= 2 * 8))
    # the estimate is the log of the mean density over the good samples' conditionals
    dens = []
    for i in range(8):
        for c in range(2):
            if (i, c) != (5, 1):
                dens.append(table_loglike(tb, rows[i, c], maxbins))
    dens = np.array(dens)
    mx = dens.max(axis=0)
    want = mx + np.log(np.exp(dens - mx).sum(axis=0)) - np.log(16.0)
    np.testing.assert_allclose(ll, want, rtol=1e-12)
    e = R.finish(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), 0, tb["cst"])
    assert all(np.all(np.isnan(v)) for v in e)
