"""CPU: the chain rule of the Blackwell-Rao likelihood Hessian
(engine.br_likelihood_hess), engine.br_likelihood_fisher and the longdouble
restatement tests/_br_hess.py.

Central differences of the gradient, the rule of tests/test_br_grad_cpu.py one
order up.  With u_b = log D_b of one used parameter and f_a = D_a dloglike/dD_a
(engine.br_likelihood_grad fed the restatement's xbar at the perturbed theory),
D_a D_b H_ab = df_a / du_b is compared with (f_a(u_b + h) - f_a(u_b - h)) / 2h,
the tables rebuilt by br_likelihood_tables at D_b (1 +- h).  The truncation is
O(h^2) of the derivative's terms; each f_a carries the rounding of its fp64 tables
through the weights, at most 2^-52 T_k of its terms (T_k:
_br_likelihood.term_bound), so the quotient carries 2^-52 T_k / h.  h = (2^-52
T_k)^(1/3) balances the two, and the assertion is
    |D_a D_b H_ab - quotient| <= 10 (h^2 + 2^-52 T_k / h) A_ab,
A_ab the sum of the magnitudes of the terms of D_a D_b H_ab: |D_a| |D_b| (|J|^T
(E_w |x_a| |x_b| + abar_a abar_b) |J| + L's formula with every product in absolute
value), the covariance counted as the difference of its two terms."""
import ctypes

import numpy as np
import pytest
from scipy.stats import invgamma, invwishart

from gibbssampler_amd.engine import (SPECTRA, br_likelihood_fisher, br_likelihood_grad, br_likelihood_hess,
                                     br_likelihood_mask, br_likelihood_tables)
from tests import _br_grad as G
from tests import _br_hess as H
from tests import _br_likelihood as R
from tests.test_br_likelihood_cpu import SEED, bins_of

EPS = 2.0 ** -52
LD = np.longdouble


def raw_second(flat, tb, maxbins, ref):
    """E_w |x_a| |x_b| + abar_a abar_b [K, Ju, Ju]: the magnitudes of the covariance's two terms."""
    from tests import _br_samples as B
    T, C = flat.shape[:2]
    t, _ = B.terms(flat, tb, maxbins)
    x = np.stack([[R.row_parts(flat[i, c], tb, maxbins)[1] for i in range(T)] for c in range(C)]).astype(LD)
    good = ~np.isnan(t[:, :, 0])
    tg, xg = t[good], np.abs(x[good])
    w = np.exp(tg - tg.max(axis=0)[None, :])
    out = np.einsum("nk,na,nb->kab", w, xg, xg) / w.sum(axis=0)[:, None, None]
    return (out + ref["abar"][:, :, None] * ref["abar"][:, None, :]).astype(np.float64)


def central_check(F, K, T, C, lrange=None):
    bins = bins_of(F)
    mask0 = None if lrange is None else br_likelihood_mask(F, bins, None, lrange)
    rows, theory, mask = R.synthetic(F, bins, K, T, C, SEED + F, mask0)
    maxbins = mask.shape[1]
    flat = rows.reshape(T, C, -1)
    tb = br_likelihood_tables(F, bins, theory, mask)
    cols = np.asarray(tb["cols"], dtype=np.int64)
    Ju = len(cols)
    mo = H.moments(flat, tb, maxbins)
    hess = br_likelihood_hess(F, bins, theory, mask, mo["xbar"], mo["cov"])
    assert hess.shape == (K, Ju, Ju) and np.array_equal(hess, hess.transpose(0, 2, 1))
    want, mag = H.hessian(F, bins, theory, mask, cols, mo["xbar_ld"], mo["cov_ld"])
    assert np.all(np.abs(hess - want) <= 64 * EPS * mag)          # the fp64 chain rule against the longdouble one
    _, A = H.chain_rule(F, bins, theory, mask, cols, mo["ref"]["abar"], raw_second(flat, tb, maxbins, mo["ref"]))
    Tk = R.term_bound(flat, tb, maxbins)
    h = (EPS * Tk) ** (1.0 / 3.0)
    D = theory.reshape(K, -1)[:, cols]                           # [K, Ju]
    worst, seen = 0.0, set()
    for b in range(Ju):
        f = []
        for sgn in (1.0, -1.0):
            th = theory.copy().reshape(K, -1)
            th[:, cols[b]] *= 1.0 + sgn * h
            th = th.reshape(theory.shape)
            xb = G.weights(flat, br_likelihood_tables(F, bins, th, mask), maxbins)["xbar"]
            f.append((br_likelihood_grad(F, bins, th, mask, xb).reshape(K, -1)[:, cols] * th.reshape(K, -1)[:, cols])
                     .astype(LD))
        quot = ((f[0] - f[1]) / (2 * h.astype(LD))[:, None]).astype(np.float64)    # [K, Ju]: a
        # f_a = D_a g_a: for a == b the product rule adds g_b D_b to df_b / du_b
        got = hess[:, :, b] * D * D[:, b:b + 1]
        got[:, b] += br_likelihood_grad(F, bins, theory, mask, mo["xbar"]).reshape(K, -1)[:, cols[b]] * D[:, b]
        bound = 10.0 * (h ** 2 + EPS * Tk / h)[:, None] * (A[:, :, b] * np.abs(D) * np.abs(D[:, b:b + 1])).astype(np.float64)
        worst = max(worst, float(np.max(np.abs(got - quot) / bound)))
        seen.add(SPECTRA[F][cols[b] // maxbins])
    print(f"  F {F} K {K} Ju {Ju} lrange {lrange}: max |chain rule - central difference| / bound = {worst:.4f} "
          f"(h {h.min():.2e} .. {h.max():.2e})")
    return worst, seen, theory


@pytest.mark.parametrize("F", [2, 3])
def test_central_differences(F):
    worst, seen, theory = central_check(F, 3, 5, 2)
    assert seen == set(SPECTRA[F])                               # F = 3: TT, EE and TE parameters of the blocks
    if F == 3:
        assert np.any(theory[1, 3] * theory[0, 3] < 0)          # model 1 has TE of the opposite sign
    assert worst <= 1.0


def test_central_differences_low_l():
    worst, seen, _ = central_check(3, 3, 7, 3, lrange=(2, 5))
    assert seen == {"TT", "EE", "BB", "TE"} and worst <= 1.0


@pytest.mark.parametrize("F", [1, 2, 3])
def test_single_sample_is_the_density(F):
    """n = C = 1: the weights drop out, cov = 0, and H is the second derivative of
    scipy's log density: central second differences in log D, h = 1e-4 (truncation
    h^2 and rounding 1e-16 / h^2 of the density's terms: below 1e-6 of them), and
    negative definite at the density's mode."""
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, 2, 1, 1, SEED + 7 * F)
    maxbins = mask.shape[1]
    flat = rows.reshape(1, 1, -1)
    tb = br_likelihood_tables(F, bins, theory, mask)
    cols = np.asarray(tb["cols"], dtype=np.int64)
    mo = H.moments(flat, tb, maxbins)
    assert not mo["cov"].any() and np.array_equal(mo["neff"], [1.0, 1.0])
    hess = br_likelihood_hess(F, bins, theory, mask, mo["xbar"], mo["cov"])
    _, mag = H.hessian(F, bins, theory, mask, cols, mo["xbar"], mo["cov"])
    pos = {int(c): j for j, c in enumerate(cols)}
    h = 1e-4
    mode = theory.copy()
    checked = 0
    for sp, s in enumerate(SPECTRA[F]):
        e = np.asarray(bins[s], dtype=np.float64)
        for b in np.flatnonzero(mask[sp]):
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if F == 3 and s != "BB":
                if s != "TT":
                    continue
                Psi = np.array([[rows[0, 0, 0, b], rows[0, 0, 3, b]], [rows[0, 0, 3, b], rows[0, 0, 1, b]]])
                mode[:, 0, b], mode[:, 1, b], mode[:, 3, b] = Psi[0, 0] / n_b, Psi[1, 1] / n_b, Psi[0, 1] / n_b
                par = ((0, (0, 0)), (1, (1, 1)), (3, (0, 1)))
                for k in range(2):
                    D0 = np.array([[theory[k, 0, b], theory[k, 3, b]], [theory[k, 3, b], theory[k, 1, b]]])

                    def f(su, sv, u, v):
                        D = D0.copy()
                        for sg, (i, j) in ((su, u), (sv, v)):
                            D[i, j] *= 1.0 + sg * h
                            D[j, i] = D[i, j]
                        return invwishart.logpdf(D, df=n_b - 3.0, scale=Psi)
                    for qu, u in par:
                        for qv, v in par:
                            ja, jb = pos[qu * maxbins + b], pos[qv * maxbins + b]
                            if u == v:     # (1 + h)(1 + h) on one entry: second difference in D (1 +- h) instead
                                D = [D0.copy() for _ in range(3)]
                                for sg, M in zip((1.0, 0.0, -1.0), D):
                                    M[u] *= 1.0 + sg * h
                                    M[u[1], u[0]] = M[u]
                                ff = [invwishart.logpdf(M, df=n_b - 3.0, scale=Psi) for M in D]
                                quot = (ff[0] - 2 * ff[1] + ff[2]) / h ** 2
                            else:
                                quot = (f(1, 1, u, v) - f(1, -1, u, v) - f(-1, 1, u, v) + f(-1, -1, u, v)) / (4 * h * h)
                            da, db = theory[k, qu, b], theory[k, qv, b]
                            assert abs(hess[k, ja, jb] * da * db - quot) <= 1e-5 * float(mag[k, ja, jb]) * abs(da * db), \
                                (s, b, k, qu, qv)
                            checked += 1
            else:
                j = pos[sp * maxbins + b]
                mode[:, sp, b] = rows[0, 0, sp, b] / (0.5 * n_b)   # scale / (alpha + 1)
                for k in range(2):
                    D = theory[k, sp, b]
                    ff = [invgamma.logpdf(D * (1.0 + sg * h), a=0.5 * n_b - 1.0, scale=rows[0, 0, sp, b])
                          for sg in (1.0, 0.0, -1.0)]
                    quot = (ff[0] - 2 * ff[1] + ff[2]) / h ** 2
                    assert abs(hess[k, j, j] * D * D - quot) <= 1e-5 * float(mag[k, j, j]) * D * D, (s, b, k)
                    checked += 1
    assert checked >= 2 * len(cols)
    h0 = br_likelihood_hess(F, bins, mode, mask, mo["xbar"], mo["cov"])
    for k in range(2):
        assert np.all(np.linalg.eigvalsh(h0[k]) < 0)
    fi = br_likelihood_fisher(F, bins, mask, h0)
    assert np.all(np.isfinite(fi["cov"])) and np.array_equal(fi["fisher"], -h0)


def _blocks_of(F, cols, maxbins):
    """block id [Ju] of each parameter: a TEB bin's TT, EE and TE share one."""
    return np.array([(c % maxbins) if (F == 3 and c // maxbins != 2) else 1000 + c for c in cols])


def test_symmetry_and_block_structure():
    F = 3
    bins = bins_of(F)
    mask = br_likelihood_mask(F, bins, None, (2, 8))
    rows, theory, mask = R.synthetic(F, bins, 2, 3, 2, SEED, mask)
    maxbins = mask.shape[1]
    tb = br_likelihood_tables(F, bins, theory, mask)
    cols = np.asarray(tb["cols"], dtype=np.int64)
    Ju = len(cols)
    mo = H.moments(rows.reshape(3, 2, -1), tb, maxbins)
    hess = br_likelihood_hess(F, bins, theory, mask, mo["xbar"], mo["cov"])
    assert np.array_equal(hess, hess.transpose(0, 2, 1)) and np.all(hess != 0.0)
    blk = _blocks_of(F, cols, maxbins)
    same = blk[:, None] == blk[None, :]
    assert 1 < same.sum() < Ju * Ju and (same.sum(axis=1) == 3).any() and (same.sum(axis=1) == 1).any()
    # cov = 0: H = L, exactly 0 outside the blocks
    L = br_likelihood_hess(F, bins, theory, mask, mo["xbar"], np.zeros((2, Ju, Ju)))
    assert not L[:, ~same].any() and np.all(L[:, same] != 0.0)
    # one covariance entry (a, b): J carries it to block(a) x block(b) (and the mirror) alone
    for a, b in ((0, Ju - 1), (1, 1), (Ju // 2, 2)):
        cov = np.zeros((2, Ju, Ju))
        cov[:, a, b] = cov[:, b, a] = 1.0
        d = br_likelihood_hess(F, bins, theory, mask, mo["xbar"], cov) - L
        into = (blk[:, None] == blk[a]) & (blk[None, :] == blk[b])
        into |= into.T
        assert not d[:, ~into].any() and d[:, into].any()
    # a value on an unused bin of the theory is never read
    used = np.zeros(mask.size, dtype=bool)
    used[cols] = True
    th = theory.copy()
    th[:, ~used.reshape(mask.shape)] = -7.0
    assert np.array_equal(br_likelihood_hess(F, bins, th, mask, mo["xbar"], mo["cov"]), hess)
    with pytest.raises(ValueError, match=r"\[K, nspec, maxbins\]"):
        br_likelihood_hess(F, bins, theory[0], mask, mo["xbar"], mo["cov"])
    with pytest.raises(ValueError, match=r"cov \[K, Ju, Ju\]"):
        br_likelihood_hess(F, bins, theory, mask, mo["xbar"], mo["cov"][:, :-1])
    with pytest.raises(ValueError, match=r"xbar must be \[K, Ju\]"):
        br_likelihood_hess(F, bins, theory, mask, mo["xbar"][:1], mo["cov"])


def test_fisher():
    F = 3
    bins = bins_of(F)
    mask = br_likelihood_mask(F, bins, None, (2, 5))
    Ju = 10
    rng = np.random.default_rng(SEED)
    a = rng.normal(size=(3, Ju, Ju))
    hess = -(a @ a.transpose(0, 2, 1) + Ju * np.eye(Ju))
    out = br_likelihood_fisher(F, bins, mask, hess)
    assert np.array_equal(out["fisher"], -hess)
    np.testing.assert_allclose(out["cov"] @ out["fisher"], np.broadcast_to(np.eye(Ju), (3, Ju, Ju)), atol=1e-12)
    assert set(out["sigma"]) == set(SPECTRA[F])
    tb = br_likelihood_tables(F, bins, np.ones((1,) + mask.shape) * np.array([1, 1, 1, 0.0])[None, :, None], mask)
    sig = np.full((3, mask.size), np.nan)
    sig[:, tb["cols"]] = np.sqrt(np.einsum("kjj->kj", out["cov"]))
    for k, s in enumerate(SPECTRA[F]):
        got = out["sigma"][s]
        assert got.shape == (3, len(bins[s]) - 1)
        assert np.array_equal(got, sig.reshape(3, *mask.shape)[:, k, :got.shape[1]], equal_nan=True)
    used = np.zeros(mask.size, dtype=bool)
    used[tb["cols"]] = True
    tt = used.reshape(mask.shape)[0, :out["sigma"]["TT"].shape[1]]
    assert tt.any() and not tt[:2].any() and not tt.all()
    assert np.isnan(out["sigma"]["TT"][:, ~tt]).all() and np.isfinite(out["sigma"]["TT"][:, tt]).all()
    bad = hess.copy()
    bad[1, 3, 3] = 1.0                                           # model 1: -hess has a negative diagonal entry
    with pytest.raises(ValueError, match="model 1 is not positive definite"):
        br_likelihood_fisher(F, bins, mask, bad)
    bad = hess.copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match="model 2"):
        br_likelihood_fisher(F, bins, mask, bad)
    with pytest.raises(ValueError, match=r"hess must be \[K, Ju, Ju\]"):
        br_likelihood_fisher(F, bins, mask, hess[:, :-1, :-1])


def test_restatement():
    """_br_hess.moments: the covariance is the raw second moment minus xbar xbar^T, a
    bad row is left out, abar2 dominates |cov| and neff lies in [1, C T]."""
    F = 3
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, 3, 5, 2, SEED)
    rows[2, 1, 2, 3] = 0.0                                       # a bad row of chain 1
    tb = br_likelihood_tables(F, bins, theory, mask)
    flat = rows.reshape(5, 2, -1)
    mo = H.moments(flat, tb, mask.shape[1])
    assert np.array_equal(mo["xbar"], mo["ref"]["xbar"])
    assert np.all(mo["abar2"] >= np.abs(mo["cov"])) and np.all(np.isfinite(mo["cov"]))
    assert np.all(mo["neff"] >= 1.0) and np.all(mo["neff"] <= 9.0)
    keep = np.ones((5, 2), dtype=bool)
    keep[2, 1] = False
    from tests import _br_samples as B
    t, _ = B.terms(flat, tb, mask.shape[1])
    x = flat[:, :, tb["cols"]][keep].astype(LD)
    tg = t.transpose(1, 0, 2)[keep]
    w = np.exp(tg - tg.max(axis=0))
    for k in range(3):
        raw = (w[:, k, None, None] * x[:, :, None] * x[:, None, :]).sum(axis=0) / w[:, k].sum()
        xb = mo["xbar_ld"][k]
        want = raw - xb[:, None] * xb[None, :]
        scale = np.abs(raw) + np.abs(xb[:, None] * xb[None, :])
        assert np.all(np.abs(mo["cov_ld"][k] - want) <= 64 * np.finfo(LD).eps * scale)


def test_capi_signatures():
    """The four exports of the Hessian pass: declared, bound, and checking their
    arguments on the host before any launch."""
    from gibbssampler_amd import _capi
    from tests.test_capi_cpu import declared
    names = ("gs_brs_hess_info", "gs_brs_hess_work_bytes", "gs_brs_hess", "gs_brs_hess_finish")
    sigs = {n: a for n, _, a in _capi._SIGS}
    assert all(n in declared() and n in sigs for n in names)
    VP, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert sigs["gs_brs_hess_info"] == [ctypes.POINTER(I)] * 3
    assert sigs["gs_brs_hess_work_bytes"] == [I] * 4 + [ctypes.POINTER(LL)]
    assert sigs["gs_brs_hess"] == [VP, VP] + [I] * 5 + [VP, VP, VP, VP, LL, VP, VP]
    assert sigs["gs_brs_hess_finish"] == [VP, VP, I, I, I, VP, VP]
    order = _capi.EXPORTED
    assert order.index("gs_brs_hess_info") == order.index("gs_brs_grad_finish") + 1
    lib = _capi.load()
    br, mt, ct = I(), I(), I()
    assert lib.gs_brs_hess_info(ctypes.byref(br), ctypes.byref(mt), ctypes.byref(ct)) == 0
    assert br.value >= 16 and br.value % 16 == 0 and 1 <= mt.value <= 16 and ct.value % 16 == 0 and ct.value >= 16
    assert lib.gs_brs_hess_info(None, ctypes.byref(mt), ctypes.byref(ct)) == -1
    wb = LL()
    assert lib.gs_brs_hess_work_bytes(3, 7, 5, 10, ctypes.byref(wb)) == 0 and wb.value == 8 * 3 * 5 * 12 * 12
    assert lib.gs_brs_hess_work_bytes(3, 2 * br.value + 1, 5, 10, ctypes.byref(wb)) == 0
    assert wb.value == 8 * 3 * 3 * 5 * 12 * 12
    assert lib.gs_brs_hess_work_bytes(3, 0, 5, 10, ctypes.byref(wb)) == 0 and wb.value == 8 * 3 * 5 * 12 * 12
    assert lib.gs_brs_hess_work_bytes(3, 7, 0, 10, ctypes.byref(wb)) == -1
    assert lib.gs_brs_hess_work_bytes(3, 7, 5, 10, None) == -1
    assert lib.gs_brs_hess_work_bytes(32, 8192, 1024, 116, ctypes.byref(wb)) == 0     # 26 GiB
    assert lib.gs_brs_hess_work_bytes(32, 8192, 4096, 116, ctypes.byref(wb)) == -1
    assert b"exceed" in lib.gs_last_error() and b"split K" in lib.gs_last_error()
    assert lib.gs_brs_hess(None, None, 1, 1, 0, 1, 1, None, None, None, None, 0, None, None) == -1
    assert b"null bank" in lib.gs_last_error()
    assert lib.gs_brs_hess_finish(None, None, 1, 1, 1, None, None) == -1
    assert b"null argument" in lib.gs_last_error()
