"""CPU: the Blackwell-Rao restatement (tests/_blackwell_rao.py) against scipy, the
inverse-Wishart diagonal claim behind the TEB shapes, option validation and
the C-ABI error paths that need no GPU."""
import ctypes

import numpy as np
import pytest
from scipy import stats
from scipy.integrate import trapezoid
from scipy.special import logsumexp

from gibbssampler_amd import _capi
from oracle import harmonic as H
from tests import _blackwell_rao as B

SEED = 20261020


def synthetic(G, seed=SEED, T=9, C=3, nspec=2, nbins=5):
    rng = np.random.default_rng(seed)
    nsb = nspec * nbins
    n_b = rng.integers(5, 60, size=nsb).astype(np.float64)
    alpha = 0.5 * n_b - 1.0
    centre = 10.0 ** rng.uniform(-2, 3, size=nsb)
    rows = centre * alpha * rng.uniform(0.6, 1.6, size=(T, C, nsb))
    grid = centre[:, None] * np.geomspace(0.5, 2.0, G)[None, :] if G > 1 else centre[:, None] * np.ones((1, 1))
    return rows, alpha, grid


@pytest.mark.parametrize("G", [1, 5])
def test_restatement_against_scipy(G):
    rows, alpha, grid = synthetic(G)
    T, C, nsb = rows.shape
    st = B.update(B.State(C, nsb, G), rows, alpha, grid)
    lp, mass = B.finish(st.m, st.S, st.n, alpha, grid)
    ref = stats.invgamma.logpdf(grid[None, None], a=alpha[None, None, :, None], scale=rows[..., None])
    want = logsumexp(ref.reshape(T * C, nsb, G), axis=0) - np.log(T * C)
    np.testing.assert_allclose(lp, want, rtol=1e-12, atol=0)
    assert st.n == T and not st.bad.any()
    if G > 1:
        np.testing.assert_allclose(mass, trapezoid(np.exp(want), grid, axis=1), rtol=1e-11)
    else:
        assert np.array_equal(mass, np.zeros(nsb))


def test_order_independence_and_skips():
    rows, alpha, grid = synthetic(5)
    T, C, nsb = rows.shape
    alpha[3] = np.nan                                      # a skipped series
    rows[4, 1, 6] = 0.0                                    # a skipped row
    half = np.zeros(nsb, dtype=bool)
    half[:2] = True
    a = B.update(B.State(C, nsb, 5), rows, alpha, grid, half)
    b = B.State(C, nsb, 5)
    for lo, hi in ((0, 3), (3, 8), (8, 9)):
        B.update(b, rows[lo:hi], alpha, grid, half)
    assert np.array_equal(a.m, b.m) and np.array_equal(a.S, b.S) and a.n == b.n == T
    assert a.bad[1, 6] == 1 and a.bad.sum() == 1
    assert not a.S[:, 3].any()
    lp, mass = B.finish(a.m, a.S, a.n, alpha, grid)
    assert np.all(np.isnan(lp[3])) and np.isnan(mass[3])
    keep = np.arange(nsb) != 3
    assert np.all(np.isfinite(lp[keep])) and np.all(np.isfinite(mass[keep]))
    # halving the recorded scale is what the shape table's half bits ask for
    c = B.update(B.State(C, nsb, 5), np.where(half, 0.5, 1.0) * rows, alpha, grid)
    assert np.array_equal(a.m, c.m) and np.array_equal(a.S, c.S)


def moments_within(x, a, scale, what):
    """Sample mean and variance of x against invgamma(a, scale), within five
    standard errors estimated from the sample."""
    n = x.size
    mean, var = x.mean(), x.var()
    se_mean = np.sqrt(var / n)
    se_var = np.sqrt((np.mean((x - mean) ** 4) - var ** 2) / n)
    want_mean, want_var = scale / (a - 1.0), scale ** 2 / ((a - 1.0) ** 2 * (a - 2.0))
    print(f"{what}: mean {mean:.6g} (want {want_mean:.6g}, se {se_mean:.2g}); "
          f"var {var:.6g} (want {want_var:.6g}, se {se_var:.2g})")
    assert abs(mean - want_mean) <= 5 * se_mean, what
    assert abs(var - want_var) <= 5 * se_var, what


def test_inverse_wishart_diagonal_is_inverse_gamma():
    """diag of IW(Psi, nu = n_b - 3), p = 2, is IG((nu - 1) / 2, Psi_ii / 2): scipy's
    sampler and the oracle's own TEB draw (its nu and Psi are the ones assumed)."""
    n_b = 40
    psi = np.array([[3.0, 0.7], [0.7, 0.5]])
    a = 0.5 * (n_b - 4)
    draws = stats.invwishart(df=n_b - 3, scale=psi).rvs(size=20000, random_state=np.random.default_rng(SEED))
    moments_within(draws[:, 0, 0], a, psi[0, 0] / 2, "scipy (0,0)")
    moments_within(draws[:, 1, 1], a, psi[1, 1] / 2, "scipy (1,1)")
    # the oracle's draw: L = 6, bins 0 | 1-2 | 3-6, so bin 2 has n_b = 7^2 - 3^2 = 40
    L = 6
    bins = {s: np.array([0, 1, 3, 7]) for s in H.SPECTRA[3]}
    model = H.Model(L, 4, 3, np.ones(L + 1), [1.0, 1.0, 1.0], bins)
    rng = np.random.default_rng(SEED + 1)
    ss = np.zeros((3, 3, L + 1))
    for l in range(L + 1):
        x = rng.normal(size=(2, 2 * l + 1))
        ss[:2, :2, l] = x @ x.T
    nu, psi_b = H.iw_bin_params(model, ss)
    assert nu[2] == n_b - 3
    k0, k1 = H.chain_key(SEED, 0)
    out = np.array([[v[2] for v in (d["TT"], d["EE"])]
                    for d in (H._iw_te_draw(model, ss, k0, k1, it) for it in range(1, 2001))])
    moments_within(out[:, 0], a, psi_b[2, 0] / 2, "oracle TT")
    moments_within(out[:, 1], a, psi_b[2, 1] / 2, "oracle EE")


def test_shape_table():
    from gibbssampler_amd.engine import br_shapes
    bins = {"TT": np.array([0, 1, 2, 3, 5, 9]), "EE": np.array([0, 1, 2, 3, 5, 9]), "BB": np.array([0, 1, 2, 9]),
            "TE": np.array([0, 1, 2, 3, 5, 9])}
    alpha, half = br_shapes(3, bins)
    assert alpha.shape == (4, 5) and half == 0b0011
    assert np.array_equal(alpha[0, 2:], [0.5 * 5 - 2, 0.5 * 16 - 2, 0.5 * 56 - 2])
    assert np.array_equal(alpha[0], alpha[1], equal_nan=True)
    assert alpha[2, 2] == 0.5 * 77 - 1 and np.all(np.isnan(alpha[2, 3:])) and np.all(np.isnan(alpha[3]))
    assert np.all(np.isnan(alpha[:, :2]))
    a2, h2 = br_shapes(2, {"EE": bins["EE"], "BB": bins["BB"]}, maxbins=6)
    assert a2.shape == (2, 6) and h2 == 0 and a2[0, 4] == 0.5 * 56 - 1 and np.isnan(a2[0, 5])


def test_option_validation():
    from gibbssampler_amd.samplers import check_blackwell_rao, check_summary
    bins = {"EE": np.arange(0, 8), "BB": np.array([0, 1, 2, 4, 7])}
    init = {"EE": np.full(7, 2.0), "BB": np.full(4, 0.5)}
    assert check_blackwell_rao(None, 2, bins) is None
    o = check_blackwell_rao({"points": 5, "span": (0.5, 2.0), "start": 3}, 2, bins, init)
    assert o["grid"].shape == (2, 7, 5) and o["start"] == 3 and o["half_mask"] == 0
    np.testing.assert_allclose(o["grid"][1, 2], 0.5 * np.geomspace(0.5, 2.0, 5))
    assert check_blackwell_rao({"points": 5}, 2, bins)["grid"] is None          # no dls_init yet
    good = np.ones((2, 7, 3)) * np.array([1.0, 2.0, 3.0])
    assert check_blackwell_rao({"grid": good}, 2, bins)["grid"].shape == (2, 7, 3)
    for G in (0, 65):
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            check_blackwell_rao({"points": G}, 2, bins, init)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        check_blackwell_rao({"grid": np.ones((2, 7, 65)).cumsum(axis=2)}, 2, bins)
    with pytest.raises(ValueError, match="nspec, maxbins, G"):
        check_blackwell_rao({"grid": np.ones((2, 6, 3))}, 2, bins)
    neg = good.copy()
    neg[0, 3, 0] = -1.0
    with pytest.raises(ValueError, match="positive"):
        check_blackwell_rao({"grid": neg}, 2, bins)
    with pytest.raises(ValueError, match="increase"):
        check_blackwell_rao({"grid": good[:, :, ::-1]}, 2, bins)
    with pytest.raises(ValueError, match="unknown options"):
        check_blackwell_rao({"points": 5, "lag": 2}, 2, bins, init)
    with pytest.raises(ValueError, match="either grid or points"):
        check_blackwell_rao({"start": 2}, 2, bins, init)
    with pytest.raises(ValueError, match="span"):
        check_blackwell_rao({"points": 5, "span": (2.0, 0.5)}, 2, bins, init)
    with pytest.raises(ValueError, match="start"):
        check_blackwell_rao({"points": 5, "start": -1}, 2, bins, init)
    with pytest.raises(ValueError, match="positive on the drawn bins"):
        check_blackwell_rao({"points": 5}, 2, bins, {"EE": np.zeros(7), "BB": init["BB"]})
    # keep_history=False: with neither a summary nor Blackwell-Rao it raises as before
    with pytest.raises(ValueError, match="keep_history=False needs summary="):
        check_summary(None, False)


def test_run_record_keys():
    from gibbssampler_amd.io import run_record
    bins = {"EE": np.arange(5), "BB": np.arange(5)}
    post = {"EE": {"grid": np.ones((4, 3)), "logpdf": np.zeros((4, 3)), "mass": np.ones(4), "alpha": np.ones(4),
                   "n": 7, "bad": 0}}
    base = run_record(None, None, None, bins, bins, bins, 1.0, 1.0)
    rec = run_record(None, None, None, bins, bins, bins, 1.0, 1.0, blackwell_rao=post, h_scales={"EE": np.ones(3)})
    assert set(rec) - set(base) == {"blackwell_rao_EE", "h_scales"}
    assert set(rec["blackwell_rao_EE"]) == {"grid", "logpdf", "mass", "alpha", "n"}


def test_capi_error_paths_without_a_gpu():
    lib = _capi.load()
    nb = ctypes.c_longlong()
    assert lib.gs_br_bytes(3, 4, 7, 5, ctypes.byref(nb)) == 0
    assert nb.value == 8 * (8 + 2 * 3 * 4 * 7 * 5 + 3 * 4)
    assert lib.gs_br_bytes(3, 4, 7, 5, None) == -1 and b"null" in lib.gs_last_error()
    for G in (0, 65):
        assert lib.gs_br_bytes(3, 4, 7, G, ctypes.byref(nb)) == -1 and b"[1, 64]" in lib.gs_last_error()
    assert lib.gs_br_bytes(0, 4, 7, 5, ctypes.byref(nb)) == -1 and b"out of range" in lib.gs_last_error()
    buf = (ctypes.c_double * 16)()                          # a host stand-in: never dereferenced
    P = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gs_br_reset(None, 3, 4, 7, 5, None) == -1 and b"null state" in lib.gs_last_error()
    assert lib.gs_br_reset(P, 3, 4, 7, 65, None) == -1 and b"[1, 64]" in lib.gs_last_error()
    assert lib.gs_br_update(None, 3, 4, 7, 5, P, P, 0, P, 8, 1, 4, None) == -1
    assert b"null state" in lib.gs_last_error()
    assert lib.gs_br_update(P, 3, 4, 7, 0, P, P, 0, P, 8, 1, 4, None) == -1 and b"[1, 64]" in lib.gs_last_error()
    assert lib.gs_br_update(P, 3, 4, 7, 5, P, P, 0, P, 8, 1, 0, None) == 0          # an empty update
    assert lib.gs_br_update(P, 3, 4, 7, 5, P, P, 0, None, 8, 1, 4, None) == -1 and b"null" in lib.gs_last_error()
    assert lib.gs_br_update(P, 3, 4, 7, 5, P, P, 0, P, 8, 1, 9, None) == -1          # nsteps > capacity
    assert b"nsteps <= capacity" in lib.gs_last_error()
    assert lib.gs_br_update(P, 3, 4, 7, 5, P, P, 0, P, 8, 0, 4, None) == -1          # iterations count from 1
    assert lib.gs_br_finish(None, 3, 4, 7, 5, P, P, P, P, None) == -1 and b"null state" in lib.gs_last_error()
    assert lib.gs_br_finish(P, 3, 4, 7, 5, P, P, None, P, None) == -1 and b"null" in lib.gs_last_error()
    assert lib.gs_cls_scale_trace(None, P, 4, None) == -1 and b"null plan" in lib.gs_last_error()
