"""Posterior sky-map summary, the parts that need no GPU: the option check, the
longdouble restatement against numpy, the per-l powers against the oracle's
alm2cl restatement, and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

from tests import _smap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_skymap_summary():
    from gibbssampler_amd.samplers import check_skymap_summary as chk
    assert chk(None) is None and chk(False) is None
    assert chk(True) == {"start": 0, "pixels": False, "every": 1}
    assert chk({}) == {"start": 0, "pixels": False, "every": 1}
    assert chk({"start": None, "pixels": True, "every": 3}) == {"start": 0, "pixels": True, "every": 3}
    assert chk({"start": 7}) == {"start": 7, "pixels": False, "every": 1}
    with pytest.raises(ValueError, match="start"):
        chk({"start": -1})
    with pytest.raises(ValueError, match="every"):
        chk({"every": 0})
    with pytest.raises(ValueError, match="unknown"):
        chk({"max_lag": 4})


@pytest.mark.parametrize("k,C", [(1, 3), (2, 1), (5, 3)])
def test_restatement_matches_numpy(k, C):
    rng = np.random.default_rng(5)
    x = 100.0 + rng.standard_normal((k, C, 37))
    ref = R.moments(x)
    flat = x.reshape(k * C, -1)
    np.testing.assert_allclose(ref["mean"].astype(float), flat.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(ref["var"].astype(float), flat.var(axis=0, ddof=1), rtol=1e-11)
    np.testing.assert_allclose(ref["chain_mean"].astype(float), x.mean(axis=0), rtol=1e-14)
    if C > 1 and k >= 2:
        W = x.var(axis=0, ddof=1).mean(axis=0)
        varp = (k - 1) / k * W + x.mean(axis=0).var(axis=0, ddof=1)
        np.testing.assert_allclose(ref["rhat"].astype(float), np.sqrt(varp / W), rtol=1e-10)
    else:
        assert np.all(np.isnan(ref["rhat"]))
    b = R.bounds(x, ref)
    assert np.all(b["mean"] > 0) and np.all(b["var"] >= 0)


def test_restatement_degenerate_counts():
    x = np.ones((1, 1, 4))
    ref = R.moments(x)
    assert np.all(np.isnan(ref["var"])) and np.all(np.isnan(ref["rhat"]))
    assert np.all(ref["mean"] == 1)


@pytest.mark.parametrize("L,l,m", [(6, 4, 0), (6, 4, 3), (5, 5, 5)])
def test_power_of_one_mode(L, l, m):
    """one non-zero (l, m): the power lands in that l only and carries the factor
    the real layout implies (the sqrt2 is in the slots: |a_lm|^2 enters as
    2 |a_lm|^2 for m > 0), checked against the oracle's alm2cl restatement."""
    from oracle import harmonic as H
    c = np.zeros(H.ncomplex(L), dtype=complex)
    c[m * (2 * L + 1 - m) // 2 + l] = 1.5 if m == 0 else 0.5 - 1.2j
    a = H.complex_to_real(c, L)
    assert np.count_nonzero(a) == (1 if m == 0 else 2)
    np.testing.assert_array_equal(R.slot_ell(L), H.slot_ell(L))
    pom, mp = R.power(a[None], np.zeros_like(a)[None], L)
    want = H.alm2cl_real(a)
    np.testing.assert_allclose(pom[0].astype(float), want, rtol=1e-15, atol=0)
    assert np.count_nonzero(pom[0]) == 1 and pom[0][l] > 0
    amp2 = abs(c).max() ** 2
    np.testing.assert_allclose(float(pom[0][l]), (1 if m == 0 else 2) * amp2 / (2 * l + 1), rtol=1e-15)
    np.testing.assert_array_equal(mp, pom)
    # a variance in the same slots adds its own share to mean_power only
    v = (a != 0).astype(float) * 0.25
    pom2, mp2 = R.power(a[None], v[None], L)
    np.testing.assert_array_equal(pom2, pom)
    np.testing.assert_allclose((mp2 - pom2)[0].astype(float), H.ell_sums(v, np.ones_like(v), L) /
                               (2 * np.arange(L + 1) + 1), rtol=1e-15)


def test_header_declares_the_smap_entry_points():
    src = open(os.path.join(ROOT, "include", "gibbs_capi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\bint\s+(gs_\w+)\s*\(", src))
    from gibbssampler_amd import _capi
    for n in ("gs_smap_bytes", "gs_smap_reset", "gs_smap_update", "gs_smap_finish", "gs_smap_power"):
        assert n in names, n
        assert n in _capi.EXPORTED, n
