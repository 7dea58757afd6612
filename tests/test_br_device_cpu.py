"""CPU: a numpy restatement of the two kernels of gs_brt.hip (theory -> tables,
xbar -> gradient), written from DESIGN.md 'Blackwell-Rao likelihood of device
theories', held to engine.br_likelihood_tables / engine.br_likelihood_grad within
64 x 2^-52 of the terms and, for a single sample, to the derivative of scipy's
invgamma / invwishart log density (the rule of tests/test_br_grad_cpu.py).  A
guard for the kernels' authors, not a test of the kernels: tests/
test_gpu_br_device.py runs those."""
import ctypes
import math

import numpy as np
import pytest
from scipy.stats import invgamma, invwishart

from gibbssampler_amd.engine import SPECTRA, br_likelihood_grad, br_likelihood_mask, br_likelihood_tables
from tests import _br_grad as G
from tests import _br_likelihood as R
from tests.test_br_grad_cpu import magnitudes
from tests.test_br_likelihood_cpu import SEED, bins_of

EPS = 2.0 ** -52


def column_tables(F, bins, mask):
    """The theory-free tables of gs_brt.hip for the used set of `mask`: cols, kind
    [Ju], part [2, Ju] (a block's EE and TE positions), cons [2, Ju] (n_b / 2 and
    the theory-free part of the column's cst term), inv [nspec * maxbins]."""
    spectra = SPECTRA[F]
    nspec, maxbins = mask.shape
    used = mask & br_likelihood_mask(F, bins, maxbins)
    if F == 3:
        used[1] = used[3] = used[0]
    cols = np.flatnonzero(used.reshape(-1))
    Ju = len(cols)
    pos = {int(c): j for j, c in enumerate(cols)}
    kind = np.zeros(Ju, dtype=np.int32)
    part = np.full((2, Ju), -1, dtype=np.int32)
    cons = np.zeros((2, Ju))
    for j, c in enumerate(cols):
        sp, b = divmod(int(c), maxbins)
        e = np.asarray(bins[spectra[sp]], dtype=np.float64)
        n_b = e[b + 1] ** 2 - e[b] ** 2
        if F == 3 and sp in (1, 3):
            continue
        cons[0, j] = 0.5 * n_b
        if F == 3 and sp == 0:
            nu = n_b - 3.0
            kind[j] = 2
            part[:, j] = pos[maxbins + b], pos[3 * maxbins + b]
            cons[1, j] = -nu * math.log(2.0) - (0.5 * math.log(math.pi) + math.lgamma(0.5 * nu) + math.lgamma(0.5 * nu - 0.5))
        else:
            kind[j] = 1
            cons[1, j] = -math.lgamma(0.5 * n_b - 1.0)
    inv = np.full(nspec * maxbins, -1, dtype=np.int32)
    inv[cols] = np.arange(Ju)
    return {"cols": cols, "kind": kind, "part": part, "cons": cons, "inv": inv}


def tables_np(theory, ct):
    """k_brt_tables: (Y [K, Ju], cst [K], bad [K], terms [K, Ju]) of theory [K, nspec, maxbins]."""
    K = theory.shape[0]
    flat = theory.reshape(K, -1)
    cols, kind, part, (h, c0) = ct["cols"], ct["kind"], ct["part"], ct["cons"]
    Ju = len(cols)
    Y, terms = np.zeros((K, Ju)), np.zeros((K, Ju))
    bad = np.zeros(K, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(Ju):
            if kind[j] == 1:
                d = flat[:, cols[j]]
                bad |= ~(np.isfinite(d) & (d > 0))
                Y[:, j] = 1.0 / d
                terms[:, j] = c0[j] - h[j] * np.log(d)
            elif kind[j] == 2:
                jee, jte = part[:, j]
                tt, ee, te = flat[:, cols[j]], flat[:, cols[jee]], flat[:, cols[jte]]
                det = tt * ee - te * te
                bad |= ~(np.isfinite(tt) & (tt > 0) & np.isfinite(ee) & (ee > 0) & np.isfinite(te) & np.isfinite(det)
                         & (det > 0))
                Y[:, j], Y[:, jee], Y[:, jte] = (0.5 * ee) / det, (0.5 * tt) / det, -te / det
                terms[:, j] = c0[j] - h[j] * np.log(det)
    cst = np.zeros(K)
    for j in range(Ju):                                          # column order, from 0.0
        if kind[j] != 0:
            cst = cst + terms[:, j]
    Y[bad], cst[bad] = np.nan, np.nan
    return Y, cst, bad, terms


def chain_np(theory, xbar, bad, ct):
    """k_brt_chain: (grad, mean [K, nspec, maxbins]) of xbar [K, Ju]."""
    K = theory.shape[0]
    flat = theory.reshape(K, -1)
    cols, kind, part, (h, _) = ct["cols"], ct["kind"], ct["part"], ct["cons"]
    grad = np.zeros_like(flat)
    mean = np.full_like(flat, np.nan)
    mean[:, cols] = xbar
    with np.errstate(all="ignore"):
        for j in range(len(cols)):
            if kind[j] == 1:
                d = flat[:, cols[j]]
                grad[:, cols[j]] = xbar[:, j] / (d * d) - h[j] / d
            elif kind[j] == 2:
                jee, jte = part[:, j]
                tt, ee, te = flat[:, cols[j]], flat[:, cols[jee]], flat[:, cols[jte]]
                ptt, pee, pte = xbar[:, j], xbar[:, jee], xbar[:, jte]
                det = tt * ee - te * te
                i00, i11, i01 = ee / det, tt / det, -te / det
                a00, a01 = i00 * ptt + i01 * pte, i00 * pte + i01 * pee
                a10, a11 = i01 * ptt + i11 * pte, i01 * pte + i11 * pee
                grad[:, cols[j]] = 0.5 * (a00 * i00 + a01 * i01) - h[j] * i00
                grad[:, cols[jee]] = 0.5 * (a10 * i01 + a11 * i11) - h[j] * i11
                grad[:, cols[jte]] = (a00 * i01 + a01 * i11) - (2.0 * h[j]) * i01
    bd = np.flatnonzero(bad)
    if len(bd):
        grad[np.ix_(bd, cols)] = np.nan
    return grad.reshape(theory.shape), mean.reshape(theory.shape)


CASES = [(1, None), (2, None), (3, None), (3, (2, 5))]


@pytest.mark.parametrize("F,lrange", CASES)
def test_restatement_against_the_engine(F, lrange):
    bins = bins_of(F)
    mask0 = None if lrange is None else br_likelihood_mask(F, bins, None, lrange)
    rows, theory, mask = R.synthetic(F, bins, 4, 5, 2, SEED + F, mask0)
    maxbins = mask.shape[1]
    tb = br_likelihood_tables(F, bins, theory, mask)
    ct = column_tables(F, bins, mask)
    assert np.array_equal(ct["cols"], tb["cols"]) and np.array_equal(ct["kind"], tb["kind"])
    Y, cst, bad, terms = tables_np(theory, ct)
    assert not bad.any()
    assert np.all(np.abs(Y - tb["Y"]) <= 64 * EPS * np.abs(tb["Y"]))
    assert np.all(np.abs(cst - tb["cst"]) <= 64 * EPS * np.abs(terms).sum(axis=1))
    if F == 3:
        assert np.any(theory[1, 3] * theory[0, 3] < 0)           # a model of the opposite TE sign
    ref = G.weights(rows.reshape(5, 2, -1), tb, maxbins)
    want = br_likelihood_grad(F, bins, theory, mask, ref["xbar"])
    grad, mean = chain_np(theory, ref["xbar"], bad, ct)
    A = magnitudes(F, bins, theory, mask, ref["abar"])
    used = ct["inv"].reshape(mask.shape) >= 0
    assert not grad[:, ~used].any() and np.isnan(mean[:, ~used]).all()
    assert np.array_equal(mean.reshape(4, -1)[:, ct["cols"]], ref["xbar"])
    assert np.all(np.abs(grad - want)[:, used] * np.abs(theory[:, used]) <= 64 * EPS * A[:, used])


@pytest.mark.parametrize("F", [1, 2, 3])
def test_single_sample_is_the_density(F):
    """n = C = 1: the restated chain rule of the restated tables' xbar (the sample)
    is the derivative of scipy's log density, central differences with h = 1e-5."""
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, 2, 1, 1, SEED + 7 * F)
    ct = column_tables(F, bins, mask)
    x = rows[0, 0].reshape(-1)[ct["cols"]]
    xbar = np.stack([x, x])
    grad, _ = chain_np(theory, xbar, np.zeros(2, dtype=bool), ct)
    A = magnitudes(F, bins, theory, mask, np.abs(xbar))
    Y, cst, _, _ = tables_np(theory, ct)
    h = 1e-5
    total = np.zeros(2)
    for sp, s in enumerate(SPECTRA[F]):
        e = np.asarray(bins[s], dtype=np.float64)
        for b in np.flatnonzero(mask[sp]):
            n_b = e[b + 1] ** 2 - e[b] ** 2
            if F == 3 and s != "BB":
                if s != "TT":
                    continue
                Psi = np.array([[rows[0, 0, 0, b], rows[0, 0, 3, b]], [rows[0, 0, 3, b], rows[0, 0, 1, b]]])
                for k in range(2):
                    D0 = np.array([[theory[k, 0, b], theory[k, 3, b]], [theory[k, 3, b], theory[k, 1, b]]])
                    total[k] += invwishart.logpdf(D0, df=n_b - 3.0, scale=Psi)
                    for q, (i, j) in ((0, (0, 0)), (1, (1, 1)), (3, (0, 1))):
                        f = []
                        for sgn in (1.0, -1.0):
                            D = D0.copy()
                            D[i, j] *= 1.0 + sgn * h
                            D[j, i] = D[i, j]
                            f.append(invwishart.logpdf(D, df=n_b - 3.0, scale=Psi))
                        quot = (f[0] - f[1]) / (2 * h)
                        assert abs(grad[k, q, b] * theory[k, q, b] - quot) <= 1e-7 * A[k, q, b], (s, b, k, q)
            else:
                for k in range(2):
                    D = theory[k, sp, b]
                    total[k] += invgamma.logpdf(D, a=0.5 * n_b - 1.0, scale=rows[0, 0, sp, b])
                    f = [invgamma.logpdf(D * (1.0 + sgn * h), a=0.5 * n_b - 1.0, scale=rows[0, 0, sp, b])
                         for sgn in (1.0, -1.0)]
                    assert abs(grad[k, sp, b] * D - (f[0] - f[1]) / (2 * h)) <= 1e-7 * A[k, sp, b], (s, b, k)
    # and the restated tables give that density: log P = r - x . Y + cst
    tb = br_likelihood_tables(F, bins, theory, mask)
    ok, xs, lg = R.row_parts(rows[0, 0].reshape(-1), tb, mask.shape[1])
    assert ok
    got = np.sum(tb["coef"] * lg) - Y @ xs + cst
    assert np.all(np.abs(got - total) <= 1e-9 * R.term_bound(rows.reshape(1, 1, -1), tb, mask.shape[1]))


def test_bad_models_are_flagged():
    F = 3
    bins = bins_of(F)
    _, theory, mask = R.synthetic(F, bins, 4, 1, 1, SEED)
    ct = column_tables(F, bins, mask)
    th = theory.copy()
    th[0, 2, 3] = 0.0                                            # a BB bin that is not positive
    th[1, 3, 4] = 1.01 * np.sqrt(th[1, 0, 4] * th[1, 1, 4])      # TE^2 > TT EE
    th[2, 2, 0] = -1.0                                           # an unused entry: not looked at
    th[3, 1, 5] = np.inf
    Y, cst, bad, _ = tables_np(th, ct)
    assert bad.tolist() == [True, True, False, True]
    assert np.isnan(Y[[0, 1, 3]]).all() and np.isnan(cst[[0, 1, 3]]).all() and np.isfinite(Y[2]).all()
    Y2, cst2, _, _ = tables_np(theory[2:3], ct)
    assert np.array_equal(Y2[0], Y[2]) and cst2[0] == cst[2]
    grad, _ = chain_np(th, np.ones_like(Y), bad, ct)
    used = ct["inv"].reshape(mask.shape) >= 0
    assert np.isnan(grad[0][used]).all() and not grad[0][~used].any() and np.isfinite(grad[2]).all()
    from gibbssampler_amd.samplers import br_theory
    for k in (0, 1, 3):                                          # the host raises where the flag is set
        with pytest.raises(ValueError):
            br_theory("test", th[k:k + 1], F, bins, mask)
    br_theory("test", th[2:3], F, bins, mask)


def test_capi_signatures():
    """The exports of gs_brt.hip: declared, bound, and checking their arguments on
    the host before any launch."""
    from gibbssampler_amd import _capi
    from tests.test_capi_cpu import declared
    names = ("gs_brt_tables", "gs_brt_mref", "gs_brt_chain")
    sigs = {n: a for n, _, a in _capi._SIGS}
    assert all(n in declared() and n in sigs for n in names)
    VP, I = ctypes.c_void_p, ctypes.c_int
    assert sigs["gs_brt_tables"] == [VP] + [I] * 4 + [VP] * 8
    assert sigs["gs_brt_mref"] == [VP, I, I, VP, VP]
    assert sigs["gs_brt_chain"] == [VP] * 3 + [I] * 4 + [VP] * 8
    order = _capi.EXPORTED
    assert order.index("gs_brt_tables") == order.index("gs_brs_hess_finish") + 1
    lib = _capi.load()
    one = ctypes.c_void_p(8)                                     # never dereferenced: every call fails its checks
    assert lib.gs_brt_tables(None, 1, 1, 4, 1, one, one, one, one, one, one, one, None) == -1
    assert b"null theory or output" in lib.gs_last_error()
    assert lib.gs_brt_tables(one, 1, 1, 4, 1, one, None, one, one, one, one, one, None) == -1
    assert b"null table" in lib.gs_last_error()
    assert lib.gs_brt_tables(one, 0, 1, 4, 1, one, one, one, one, one, one, one, None) == -1
    assert b"K >= 1" in lib.gs_last_error()
    assert lib.gs_brt_tables(one, 1, 1, 4, 5, one, one, one, one, one, one, one, None) == -1
    assert b"Ju out of range" in lib.gs_last_error()
    assert lib.gs_brt_mref(None, 1, 1, one, None) == -1 and b"null argument" in lib.gs_last_error()
    assert lib.gs_brt_mref(one, 0, 1, one, None) == -1
    assert lib.gs_brt_chain(one, None, one, 1, 1, 4, 1, one, one, one, one, one, one, None, None) == -1
    assert b"null theory, xbar, bad or grad" in lib.gs_last_error()
    assert lib.gs_brt_chain(one, one, one, 1, 1, 4, 1, one, one, one, one, None, one, None, None) == -1
    assert b"null table" in lib.gs_last_error()
    assert lib.gs_brt_chain(one, one, one, 1, 40, 4, 1, one, one, one, one, one, one, None, None) == -1
    assert b"nspec in [1, 32]" in lib.gs_last_error()
