"""GPU: the Hessian of the Blackwell-Rao sample bank's likelihood (gs_brs_hess*,
engine.BlackwellRaoSamples.loglike_hess / fisher).

The device's scale_cov and hess are compared with tests/_br_hess.py (order-free
longdouble sums), every entry.  Bound, derived and not tuned: with delta_k = (Ju +
16) 2^-52 T_k the evaluator's per-sample bound (tests/_br_samples.bounds),
    |d cov_kab| <= (2 delta_k + (2 C n + 32) 2^-52) abar2_kab,
abar2_kab = sum w |u_a| |u_b| / sum w of the restatement: the gradient's bound with
the product of two centred columns in place of one column.  hess is held to that
bound and the gradient's bound on xbar pushed through J and L entrywise
(_br_hess.hessian_bound).

Every case but the dominated one first asserts that the restatement's neff is >= 4
for every model, so that the covariance is not trivially 0.  The banks are
_br_likelihood.synthetic's.  Its theories, 0.3 / sqrt(k + 1) in the logarithm away
from the fiducial in every bin, leave one sample with all the weight once there
are more than a few dozen columns (no seed of 24 tried gives neff >= 4 at Ju >= 28),
so the cases with Ju >= 63 pull the models towards their geometric mean (`near`:
the logarithmic distance times 0.1, the correlation TE / sqrt(TT EE) kept).
Largest |device - numpy| / bound seen on an MI355X: see DESIGN.md 'Blackwell-Rao
likelihood Hessian'."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_grad as G  # noqa: E402
from tests import _br_hess as H  # noqa: E402
from tests import _br_likelihood as R  # noqa: E402
from tests import _br_samples as B  # noqa: E402
from tests import test_gpu_br_likelihood as L  # noqa: E402
from tests import test_gpu_br_samples as S  # noqa: E402
from tests.test_gpu_br_samples import bank_of  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = L.SEED


def hess_info():
    from gibbssampler_amd import _capi as C
    br, mt, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert C.load().gs_brs_hess_info(ctypes.byref(br), ctypes.byref(mt), ctypes.byref(ct)) == 0
    assert br.value >= 16 and br.value % 16 == 0 and mt.value >= 1 and ct.value % 16 == 0
    return br.value, mt.value, ct.value


def near(F, theory, s):
    """The models pulled towards their geometric mean: log distance times s."""
    gm = np.exp(np.mean(np.log(np.abs(theory)), axis=0, keepdims=True))
    out = gm * (np.abs(theory) / gm) ** s
    if F == 3:
        out[:, 3] = theory[:, 3] / np.sqrt(theory[:, 0] * theory[:, 1]) * np.sqrt(out[:, 0] * out[:, 1])
    return out


# name: F, unbinned, one bin, lrange, T, C, seed, s (near), Ju
SHAPES = {
    "Ju1": (2, False, True, None, 40, 1, SEED + 2, 1.0, 1),
    "Ju10": (3, False, False, (2, 5), 7, 4, SEED, 1.0, 10),
    "Ju63": (1, True, False, None, 48, 4, SEED, 0.1, 63),           # a padded stage, a padded row and column
    "Ju68": (2, True, False, (2, 35), 48, 4, SEED, 0.1, 68),        # two column tiles: an off-diagonal pair
    "Ju68teb": (3, True, False, (2, 18), 256, 4, SEED + 7, 0.1, 68),  # TEB blocks across the two tiles
}
_CACHE = {}


def case(name, K=5, T=None, C=None):
    """rows [T, C, nspec, maxbins], theory, mask, bins, tables, maxbins and the restatement (computed once)."""
    from gibbssampler_amd.engine import br_likelihood_mask, br_likelihood_tables
    key = (name, K, T, C)
    if key in _CACHE:
        return _CACHE[key]
    F, unbinned, one, lrange, T0, C0, seed, s, Ju = SHAPES[name]
    T, C = T or T0, C or C0
    bins = L.bins_of(F, unbinned)
    mask = None
    if one:
        mask = np.zeros_like(br_likelihood_mask(F, bins))
        mask[-1, 3] = True
    if lrange is not None:
        mask = br_likelihood_mask(F, bins, None, lrange)
    rows, theory, mask = R.synthetic(F, bins, K, T, C, seed, mask)
    if s != 1.0:
        theory = near(F, theory, s)
    cs = {"F": F, "rows": rows, "theory": theory, "mask": mask, "bins": bins, "maxbins": mask.shape[1],
          "tables": br_likelihood_tables(F, bins, theory, mask)}
    assert len(cs["tables"]["cols"]) == Ju
    cs["ref"] = H.moments(rows.reshape(T, C, -1), cs["tables"], cs["maxbins"])
    _CACHE[key] = cs
    return cs


def check(out, rows, cs, what, ref=None, tables=None, theory=None, neff=True):
    """out = loglike_hess(theory) against the restatement of rows [T, C, nspec, maxbins]."""
    tables = cs["tables"] if tables is None else tables
    theory = cs["theory"] if theory is None else theory
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    maxbins = cs["maxbins"]
    ref = H.moments(flat, tables, maxbins) if ref is None else ref
    cols = np.asarray(tables["cols"], dtype=np.int64)
    K, Ju = ref["xbar"].shape
    if neff:
        assert np.all(ref["neff"] >= 4.0), (what, ref["neff"])
        assert np.all(np.einsum("kjj->kj", ref["cov"]) > 0)
    bx, _ = G.xbar_bound(flat, tables, maxbins)
    bc = H.cov_bound(flat, tables, maxbins)
    dx = bx[:, None] * ref["ref"]["abar"]
    dc = bc[:, None, None] * ref["abar2"]
    cov, hess = out["scale_cov"], out["hess"]
    assert cov.shape == hess.shape == (K, Ju, Ju) and len(out["params"]) == Ju, what
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(hess, hess.transpose(0, 2, 1)), what
    spectra = ("TT",) if cs["F"] == 1 else (("EE", "BB") if cs["F"] == 2 else ("TT", "EE", "BB", "TE"))
    assert out["params"] == [(spectra[c // maxbins], int(c % maxbins)) for c in cols], what
    ok = dc > 0
    assert np.array_equal(cov[~ok], ref["cov"][~ok]), what
    rc = float(np.max(np.abs(cov - ref["cov"])[ok] / dc[ok])) if ok.any() else 0.0
    want, _ = H.hessian(cs["F"], cs["bins"], theory, cs["mask"], cols, ref["xbar_ld"], ref["cov_ld"])
    want = want.astype(np.float64)
    hb = H.hessian_bound(cs["F"], cs["bins"], theory, cs["mask"], cols, ref["xbar"], ref["cov"], dx, dc)
    use = hb > 0
    assert not hess[~use].any() and not want[~use].any(), what
    rh = float(np.max(np.abs(hess - want)[use] / hb[use]))
    print(f"  {what}: max |device - reference| / bound: scale_cov {rc:.4f}, hess {rh:.4f} (Ju {Ju}, n {T}, C {C}, K {K}, "
          f"cov bound / abar2 {bc.max():.3e}, min neff {np.nanmin(ref['neff']):.2f})")
    assert rc <= 1.0 and rh <= 1.0, what
    return ref


# ---- 1. against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_hess(name):
    cs = case(name)
    _, mt, ct = hess_info()
    if name.startswith("Ju68"):
        assert ct < 68 <= ct + 4 and mt < 5                      # just above the column tile; two model tiles
    bank = bank_of(cs, cap=64)
    assert bank.Ju == SHAPES[name][-1]
    out = bank.loglike_hess(cs["theory"])
    check(out, cs["rows"], cs, name, ref=cs["ref"])
    a = bank.loglike_grad(cs["theory"])
    assert set(out) == set(a) | {"hess", "scale_cov", "params"}
    assert all(np.array_equal(a[k], out[k], equal_nan=True) for k in a if k != "grad")
    assert all(np.array_equal(a["grad"][s], out["grad"][s]) for s in a["grad"])
    fi = bank.fisher(cs["theory"]) if np.all(np.linalg.eigvalsh(-out["hess"]) > 0) else None
    if fi is not None:
        assert np.array_equal(fi["fisher"], -out["hess"]) and np.all(np.isfinite(fi["cov"]))


@pytest.fixture(scope="module")
def long_case():
    return case("Ju10", T=2 * hess_info()[0] + 5, C=2)


def test_three_blocks(long_case):
    cs = long_case
    T = cs["rows"].shape[0]
    assert T == 2 * hess_info()[0] + 5 and T % 16 != 0
    bank = bank_of(cs, cap=512)
    check(bank.loglike_hess(cs["theory"]), cs["rows"], cs, f"three blocks n {T}", ref=cs["ref"])


def test_bad_rows():
    cs = case("Ju10")
    bad = np.concatenate([cs["rows"], cs["rows"][:3]])                 # rows 7 .. 9 will be the bad ones
    bad[7, 1, 2, 2] = 0.0                                               # beta = 0 (BB) for chain 1
    bad[8, 2, 3, 4] = 2.0 * np.sqrt(bad[8, 2, 0, 4] * bad[8, 2, 1, 4])  # c^2 = 4 a dd for chain 2
    bad[9, 0, 2, 2] = np.inf                                            # the bank row holds an infinity
    bad[9, 3, 0, 3] = -np.inf
    bad[7, 0, 1, 3] = np.nan                                            # and a NaN
    bank = bank_of(cs, rows=bad, cuts=(3, 4, 3), cap=4)
    assert int(torch.isnan(bank.r).sum()) == 5 and not torch.isfinite(bank.X).all()
    assert bool(torch.isinf(bank.X[torch.isnan(bank.r)]).any())
    out = bank.loglike_hess(cs["theory"])
    assert np.array_equal(out["bad"], [2, 1, 1, 1]) and out["n"] == 10
    assert np.isfinite(out["scale_cov"]).all() and np.isfinite(out["hess"]).all()
    check(out, bad, cs, "bad rows")


def test_bad_rows_equal_bank_without_them():
    """Bad rows at the end of every chain: the result has the bits of the bank that stops before them."""
    cs = case("Ju10")
    bad = np.concatenate([cs["rows"], cs["rows"][:2]])
    for c in range(4):
        bad[7, c, 2, 2] = 0.0 if c % 2 else -1.0                        # every chain's row 7 is bad
        bad[8, c, 0, 4] = np.inf if c % 2 else np.nan                   # and row 8, with an infinity in X
    bank = bank_of(cs, rows=bad, cuts=(3, 4, 2), cap=4)
    assert int(torch.isnan(bank.r).sum()) == 8 and bool(torch.isinf(bank.X).any())
    clean = bank_of(cs, cuts=(3, 4), cap=4)
    got, want = bank.loglike_hess(cs["theory"]), clean.loglike_hess(cs["theory"])
    assert np.array_equal(got["scale_cov"], want["scale_cov"]) and np.array_equal(got["mean_scale"], want["mean_scale"],
                                                                                  equal_nan=True)
    assert np.array_equal(got["hess"], want["hess"]) and np.isfinite(got["hess"]).all()


def test_dominated():
    """One row's t is 800 above every other: its weight is exactly 1, the others underflow,
    u of that row is exactly 0, cov is exactly 0 and H is the single-sample closed form."""
    from gibbssampler_amd.engine import br_likelihood_hess
    cs = S.case(3, 5)
    rows = 3.0 * cs["rows"]
    rows[3, 1] = cs["rows"][3, 1]
    flat = rows.reshape(7, 3, -1)
    t, _ = B.terms(flat, cs["tables"], cs["maxbins"])
    rest = np.delete(t.reshape(21, -1), 1 * 7 + 3, axis=0)
    assert np.all(t[1, 3] - rest.max(axis=0) >= 800.0)
    out = bank_of(cs, rows=rows, cuts=(3, 4), cap=4).loglike_hess(cs["theory"])
    Ju = len(cs["tables"]["cols"])
    assert out["scale_cov"].shape == (5, Ju, Ju) and not out["scale_cov"].any()
    x = flat[3, 1][cs["tables"]["cols"]]
    single = br_likelihood_hess(3, cs["bins"], cs["theory"], cs["mask"], np.broadcast_to(x, (5, Ju)),
                                np.zeros((5, Ju, Ju)))
    assert np.array_equal(out["hess"], single) and np.all(np.isfinite(single))
    check(out, rows, cs, "dominated", neff=False)


def test_empty():
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = case("Ju10")
    bank = BlackwellRaoSamples(4, 3, cs["bins"], cs["mask"], 5)
    out = bank.loglike_hess(cs["theory"])
    assert out["n"] == 0 and np.isnan(out["scale_cov"]).all() and np.isnan(out["hess"]).all()
    num2 = bank.hess_numerators(cs["tables"]["Y"], np.zeros(5), np.zeros((5, 10)))
    torch.cuda.synchronize()
    assert tuple(num2.shape) == (4, 5, bank.Jp, bank.Jp) and not num2.any()
    with pytest.raises(ValueError, match="model 0"):
        bank.fisher(cs["theory"])


# ---- 2. bit equality -------------------------------------------------------------------------------------
def setup_of(bank, cs):
    """(mref [K], center [K, Ju]) of the complete bank, on the device."""
    f = S.fields(bank, cs["tables"])
    assert bool((f[1] > 0).all())
    return f[0].amax(dim=0), torch.from_numpy(np.ascontiguousarray(cs["ref"]["xbar"])).cuda()


@pytest.mark.parametrize("name", ["Ju10", "Ju68"])
def test_bit_equality(name):
    cs = case(name)
    tables = cs["tables"]
    T = cs["rows"].shape[0]
    ref = bank_of(cs, cap=64)
    mref, center = setup_of(ref, cs)
    num2 = ref.hess_numerators(tables["Y"], mref, center)
    Ju, Jp = ref.Ju, ref.Jp
    assert tuple(num2.shape) == (4, 5, Jp, Jp) and bool((num2[:, :, :Ju, :Ju] != 0).all())
    # symmetric, padding zero
    assert torch.equal(num2, num2.transpose(2, 3))
    assert (Jp > Ju) == (name == "Ju10") and not num2[:, :, Ju:].any() and not num2[:, :, :, Ju:].any()
    # model 4 of K = 5 is the same model run as K = 1 with the same reference and centre
    one = ref.hess_numerators(tables["Y"][4:5].copy(), mref[4:5].clone(), center[4:5].clone())
    assert torch.equal(one[:, 0], num2[:, 4])
    # chain 2 alone is chain 2 of the four
    solo = bank_of(cs, rows=cs["rows"][:, 2:3], cap=64)
    assert torch.equal(solo.hess_numerators(tables["Y"], mref, center)[0], num2[2])
    # another ring, other cuts and a bank with room to spare
    got = bank_of(cs, cuts=(3,) * (T // 3) + (T % 3,), cap=4, capacity=T + 12)
    assert torch.equal(got.hess_numerators(tables["Y"], mref, center), num2)
    # twice the same
    assert torch.equal(ref.hess_numerators(tables["Y"], mref, center), num2)
    a, b = ref.loglike_hess(cs["theory"]), ref.loglike_hess(cs["theory"])
    assert np.array_equal(a["hess"], b["hess"]) and np.array_equal(a["scale_cov"], b["scale_cov"])


def test_bit_equality_blocks(long_case):
    cs = long_case
    tables = cs["tables"]
    ref = bank_of(cs, cap=512)
    mref, center = setup_of(ref, cs)
    num2 = ref.hess_numerators(tables["Y"], mref, center)
    assert torch.equal(num2, num2.transpose(2, 3))
    assert torch.equal(ref.hess_numerators(tables["Y"][4:5].copy(), mref[4:5].clone(), center[4:5].clone())[:, 0],
                       num2[:, 4])
    solo = bank_of(cs, rows=cs["rows"][:, 1:], cap=512)
    assert torch.equal(solo.hess_numerators(tables["Y"], mref, center)[0], num2[1])


# ---- 3. gather -----------------------------------------------------------------------------------------------
def test_gather():
    cs = case("Ju10")
    tables = cs["tables"]
    whole = bank_of(cs, cuts=(3, 4), cap=4)
    lo = bank_of(cs, rows=cs["rows"][:, :2], cuts=(3, 4), cap=4)
    hi = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    want = whole.loglike_hess(cs["theory"])
    mref = S.fields(whole, tables)[0].amax(dim=0)
    xbar = torch.from_numpy(np.ascontiguousarray(want["mean_scale"].reshape(5, -1)[:, tables["cols"]])).cuda()
    hi_fields = hi.fields(hi.evaluate(tables["Y"]))
    hi_num = hi.grad_numerators(tables["Y"], mref)
    hi_num2 = hi.hess_numerators(tables["Y"], mref, xbar)
    calls = []

    def gather(t, dim=0):
        calls.append((tuple(t.shape), dim))
        return torch.cat([t, hi_fields if dim == 1 else (hi_num if t.dim() == 3 else hi_num2)], dim=dim)

    got = lo.loglike_hess(cs["theory"], gather)
    assert calls == [((3, 2, 5), 1), ((2, 5, lo.Jp), 0), ((2, 5, lo.Jp, lo.Jp), 0)]
    for k in ("loglike", "chain_loglike", "neff", "mean_scale", "chain_weight", "scale_cov", "hess"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert all(np.array_equal(got["grad"][s], want["grad"][s]) for s in want["grad"])
    check(got, cs["rows"], cs, "gathered", ref=cs["ref"])
    if _pd(want["hess"]):
        assert np.array_equal(lo.fisher(cs["theory"], gather)["cov"], whole.fisher(cs["theory"])["cov"])
    else:
        with pytest.raises(ValueError, match="is not positive definite"):
            lo.fisher(cs["theory"], gather)


def _pd(hess):
    return bool(np.all(np.linalg.eigvalsh(-hess) > 0))


# ---- 4. the surface -------------------------------------------------------------------------------------------
def test_surface():
    from tests.test_gpu_br_grad import _problem
    from gibbssampler_amd.samplers import br_theory
    from gibbssampler_amd.engine import br_likelihood_fisher
    model, init, theory = _problem()
    T = 40
    r = L.make_runner(model, "centered", 4)
    r.run(init, T, graph_chunk=32, br_samples=S.OPTS, keep_scales=True)
    bank = r.br_samples()
    p = r.plan
    hs = np.full((T, 4, p.nspec, p.maxbins), np.nan)
    for k, s in enumerate(model.spectra):
        hs[:, :, k, :model.nbins(s)] = r.h_scales[s]
    out = bank.loglike_hess(theory)
    tables = bank.tables(theory)
    th = br_theory("test", theory, 3, bank.bins, bank.mask)
    cs = {"F": 3, "bins": bank.bins, "mask": bank.mask, "maxbins": p.maxbins}
    check(out, hs, cs, "surface", tables=tables, theory=th, neff=False)
    a = bank.loglike_grad(theory)
    assert all(np.array_equal(a[k], out[k], equal_nan=True) for k in a if k != "grad")
    assert out["hess"].shape == (4, bank.Ju, bank.Ju) and np.all(np.isfinite(out["hess"]))
    want = None
    try:
        want = br_likelihood_fisher(3, bank.bins, bank.mask, out["hess"])
    except ValueError as e:
        with pytest.raises(ValueError, match=str(e)[:60]):
            bank.fisher(theory)
    if want is not None:
        fi = bank.fisher(theory)
        assert np.array_equal(fi["cov"], want["cov"]) and set(fi["sigma"]) == set(model.spectra)
        assert fi["sigma"]["TT"].shape == (4, model.nbins("TT"))
    with pytest.raises(ValueError, match="positive but for TE"):
        bank.loglike_hess({s: -v for s, v in theory.items()})


# ---- 5. argument checks ------------------------------------------------------------------------------------
def test_argument_checks():
    from gibbssampler_amd import _capi as C
    cs = case("Ju10")
    bank = bank_of(cs, cuts=(3, 4), cap=4, capacity=9)
    lib = bank.lib
    Y = torch.from_numpy(cs["tables"]["Y"]).cuda()
    mref = torch.zeros(5, dtype=torch.float64, device="cuda")
    cen = torch.zeros(5, bank.Ju, dtype=torch.float64, device="cuda")
    n2 = 4 * 5 * bank.Jp * bank.Jp
    work = torch.zeros(n2, dtype=torch.float64, device="cuda")
    num2 = torch.zeros(n2, dtype=torch.float64, device="cuda")
    hs = lambda X, n, Yp, cp, w, nb, o: lib.gs_brs_hess(X, C.ptr(bank.r), 4, 9, n, bank.Ju, 5, Yp, C.ptr(mref), cp, w, nb, o, None)  # noqa: E731
    full = n2 * 8
    assert hs(None, 7, C.ptr(Y), C.ptr(cen), C.ptr(work), full, C.ptr(num2)) == -1
    assert b"null bank" in lib.gs_last_error()
    assert hs(C.ptr(bank.X), 7, C.ptr(Y), C.ptr(cen), C.ptr(work), full, None) == -1
    assert b"null num2" in lib.gs_last_error()
    assert hs(C.ptr(bank.X), 7, C.ptr(Y), None, C.ptr(work), full, C.ptr(num2)) == -1
    assert b"null Y, mref, center or workspace" in lib.gs_last_error()
    assert hs(C.ptr(bank.X), 10, C.ptr(Y), C.ptr(cen), C.ptr(work), full, C.ptr(num2)) == -1
    assert b"[0, cap]" in lib.gs_last_error()
    assert hs(C.ptr(bank.X), 7, C.ptr(Y), C.ptr(cen), C.ptr(work), full - 8, C.ptr(num2)) == -1
    assert b"workspace is smaller" in lib.gs_last_error()
    assert lib.gs_brs_hess_finish(C.ptr(num2), None, 4, 5, bank.Ju, C.ptr(num2), None) == -1
    assert b"null argument" in lib.gs_last_error()
    with pytest.raises(ValueError, match=r"center must be \[K, Ju\]"):
        bank.hess_numerators(cs["tables"]["Y"], mref, cen[:, :5])
    with pytest.raises(ValueError, match=r"mref \[K\]"):
        bank.hess_numerators(cs["tables"]["Y"], mref[:4], cen)
    torch.cuda.synchronize()
    assert not num2.any() and not work.any()
