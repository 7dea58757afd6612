"""No GPU: the numpy restatement of the streaming posterior summaries
(tests/_summary.py) against direct two-pass formulas and AR(1) theory, and the
C-ABI declaration of the gs_summary_* entry points against the ctypes binding."""
import os
import re

import numpy as np
import pytest

from tests import _summary as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHI, T, C, NSB, K = 0.5, 2000, 4, 256, 32


@pytest.fixture(scope="module")
def ar1_summary():
    x = S.ar1(np.random.default_rng(20261020), T, (C, NSB), PHI)
    return x, S.summarise(x, K)


def test_restatement_on_ar1_series(ar1_summary):
    """x_t = 0.5 x_{t-1} + e_t, T 2000, 4 chains, 256 series, max_lag 32: the
    median ESS / (C T) lies within 5 % of (1 - phi) / (1 + phi) = 1 / 3, every
    R-hat is below 1.02, and the streaming gamma_j equals the direct centred
    gamma_j within 64 T 2^-52 max(gamma_0, delta^2)."""
    x, out = ar1_summary
    rel = out["ess"] / (C * T)
    print(f"ESS / (C T): median {np.median(rel):.4f}, min {rel.min():.3f}, max {rel.max():.3f}; "
          f"ess_truncated on {int(out['ess_truncated'].sum())} series; max R-hat {out['rhat'].max():.4f}")
    assert out["n"] == T
    assert abs(np.median(rel) - (1 - PHI) / (1 + PHI)) <= 0.05 * (1 - PHI) / (1 + PHI)
    assert np.all(out["rhat"] < 1.02)
    direct = S.direct_gamma(x, K)                       # [K + 1, C, NSB]
    got = np.moveaxis(out["gamma"], 1, 0)
    delta = out["chain_mean"] - x[0]
    bound = 64 * T * 2.0 ** -52 * np.maximum(direct[0], delta * delta)
    err = np.abs(got - direct)
    print(f"max |gamma - direct| / bound: {np.max(err / bound):.3e}")
    assert np.all(err <= bound)


def test_restatement_moments_and_rhat_against_direct(ar1_summary):
    """Welford mean / variance, min / max, the pooled moments and R-hat against
    numpy's two-pass forms (a few ulp of T sequential updates)."""
    x, out = ar1_summary
    tol = 8 * T * 2.0 ** -52
    np.testing.assert_allclose(out["chain_mean"], x.mean(axis=0), rtol=0, atol=tol * np.abs(x).max())
    np.testing.assert_allclose(out["chain_var"], x.var(axis=0, ddof=1), rtol=tol)
    np.testing.assert_allclose(out["mean"], x.mean(axis=(0, 1)), rtol=0, atol=tol * np.abs(x).max())
    np.testing.assert_allclose(out["var"], x.reshape(T * C, NSB).var(axis=0, ddof=1), rtol=tol)
    assert np.array_equal(out["min"], x.min(axis=(0, 1))) and np.array_equal(out["max"], x.max(axis=(0, 1)))
    W = x.var(axis=0, ddof=1).mean(axis=0)
    Bn = x.mean(axis=0).var(axis=0, ddof=1)
    np.testing.assert_allclose(out["rhat"], np.sqrt(((T - 1) / T * W + Bn) / W), rtol=1e-12)
    # one chain: rho_j = gamma_j / gamma_0, R-hat undefined
    one = S.summarise(x[:, :1], K)
    np.testing.assert_allclose(one["acf"], one["gamma"][0] / one["gamma"][0, 0], rtol=0, atol=1e-14)
    assert np.all(np.isnan(one["rhat"]))


def test_restatement_cut_into_launches_and_degenerate_series():
    """The recursion does not depend on how the rows are cut; a constant series
    gives NaN diagnostics with exact moments; n <= j gives NaN gamma_j."""
    rng = np.random.default_rng(5)
    x = S.ar1(rng, 21, (2, 6), PHI, offset=3.0)
    x[:, :, 0] = 7.25
    whole = S.update(S.State((2, 6), 12), x)
    cut = S.State((2, 6), 12)
    for a, b in ((0, 8), (8, 16), (16, 21)):
        S.update(cut, x[a:b])
    for k in S.FIXED + ("P", "head", "ring"):
        assert np.array_equal(getattr(whole, k), getattr(cut, k)), k
    out = S.finish(whole)
    assert np.isnan(out["rhat"][0]) and np.isnan(out["ess"][0]) and np.all(np.isnan(out["acf"][:, 0]))
    assert out["mean"][0] == 7.25 and out["var"][0] == 0.0 and not np.isnan(out["rhat"][1:]).any()
    short = S.summarise(x[:3], 12)
    assert np.all(np.isnan(short["gamma"][:, 3:])) and not np.isnan(short["gamma"][:, :3, 1:]).any()


def test_header_and_binding_declare_the_summary_entry_points():
    from gibbssampler_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gibbs_capi.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(gs_summary_\w+)\s*\(", src)))
    assert declared == ["gs_summary_bytes", "gs_summary_finish", "gs_summary_reset", "gs_summary_update"]
    assert sorted(n for n in _capi.EXPORTED if n.startswith("gs_summary_")) == declared
