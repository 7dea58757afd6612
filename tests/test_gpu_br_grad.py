"""GPU: the gradient of the Blackwell-Rao sample bank's likelihood (gs_brs_grad*,
engine.BlackwellRaoSamples.loglike_grad).

The device's xbar (mean_scale), chain_weight and grad are compared with
tests/_br_grad.py (order-free longdouble sums).  Bound, derived and not tuned:
with delta_k = (Ju + 16) 2^-52 T_k the evaluator's per-sample bound,
    |d xbar_kj|      <= (2 delta_k + (2 C n + 16) 2^-52) abar_kj
    |d chain_weight| <=  2 delta_k + 2 C n 2^-52
abar_kj = sum w |x_j| / sum w of the restatement; through the chain rule
    |d grad| <= (xbar bound) / D^2                      inverse-Gamma bin
    |d G|    <= |D^-1| |d Psi| |D^-1| / 2 entrywise     TEB block (TE: 2 G_01)
Largest |device - numpy| / bound seen on an MI355X: see DESIGN.md 'Blackwell-Rao
likelihood gradient'."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_grad as G  # noqa: E402
from tests import _br_samples as B  # noqa: E402
from tests import test_gpu_br_likelihood as L  # noqa: E402
from tests import test_gpu_br_samples as S  # noqa: E402
from tests.test_gpu_br_samples import CASES, bank_of, case  # noqa: E402

pytestmark = pytest.mark.gpu


def grad_info():
    from gibbssampler_amd import _capi as C
    gr, tm, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert C.load().gs_brs_grad_info(ctypes.byref(gr), ctypes.byref(tm), ctypes.byref(ct)) == 0
    assert gr.value >= 16 and gr.value % 16 == 0 and tm.value % 16 == 0 and ct.value % 16 == 0
    return gr.value, tm.value, ct.value


def grad_bound(F, bins, theory, mask, cols, dx):
    """|d grad| [K, nspec, maxbins] for |d xbar| <= dx [K, Ju] through the chain rule."""
    from gibbssampler_amd.engine import SPECTRA
    K, nspec, maxbins = theory.shape
    pos = {int(c): j for j, c in enumerate(cols)}
    out = np.zeros_like(theory)
    for sp, s in enumerate(SPECTRA[F]):
        for b in range(maxbins):
            if sp * maxbins + b not in pos:
                continue
            if F == 3 and s != "BB":
                if s != "TT":
                    continue
                for k in range(K):
                    D = np.array([[theory[k, 0, b], theory[k, 3, b]], [theory[k, 3, b], theory[k, 1, b]]])
                    P = np.array([[dx[k, pos[b]], dx[k, pos[3 * maxbins + b]]],
                                  [dx[k, pos[3 * maxbins + b]], dx[k, pos[maxbins + b]]]])
                    Di = np.abs(np.linalg.inv(D))
                    A = 0.5 * Di @ P @ Di
                    out[k, 0, b], out[k, 1, b], out[k, 3, b] = A[0, 0], A[1, 1], 2.0 * A[0, 1]
            else:
                out[:, sp, b] = dx[:, pos[sp * maxbins + b]] / theory[:, sp, b] ** 2
    return out


def check(out, rows, cs, what, tables=None, theory=None):
    """out = loglike_grad(theory) against the restatement of rows [T, C, nspec, maxbins]."""
    from gibbssampler_amd.engine import SPECTRA, br_likelihood_grad
    tables = cs["tables"] if tables is None else tables
    theory = cs["theory"] if theory is None else theory
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    maxbins = cs["maxbins"]
    ref = G.weights(flat, tables, maxbins)
    bx, bw = G.xbar_bound(flat, tables, maxbins)
    cols = np.asarray(tables["cols"], dtype=np.int64)
    K, Ju = ref["xbar"].shape
    ms = out["mean_scale"]
    assert ms.shape == theory.shape and out["chain_weight"].shape == (C, K), what
    off = np.ones(ms[0].size, dtype=bool)
    off[cols] = False
    assert np.isnan(ms.reshape(K, -1)[:, off]).all(), what
    xb = ms.reshape(K, -1)[:, cols]
    dx = bx[:, None] * ref["abar"]
    rx = float(np.max(np.abs(xb - ref["xbar"]) / dx))
    rw = float(np.max(np.abs(out["chain_weight"] - ref["share"]) / bw[None, :]))
    want = br_likelihood_grad(cs["F"], cs["bins"], theory, cs["mask"], ref["xbar"])
    gb = grad_bound(cs["F"], cs["bins"], theory, cs["mask"], cols, dx)
    got = np.zeros_like(want)
    for k, s in enumerate(SPECTRA[cs["F"]]):
        g = out["grad"][s]
        assert g.shape == (K, len(cs["bins"][s]) - 1), (what, s)
        got[:, k, :g.shape[1]] = g
    use = gb > 0
    assert np.array_equal(got[~use], want[~use]) and not got[~use].any(), what
    rg = float(np.max(np.abs(got - want)[use] / gb[use]))
    print(f"  {what}: max |device - reference| / bound: xbar {rx:.4f}, chain_weight {rw:.4f}, grad {rg:.4f} "
          f"(Ju {Ju}, n {T}, C {C}, K {K}, xbar bound / abar {bx.max():.3e})")
    assert rx <= 1.0 and rw <= 1.0 and rg <= 1.0, what
    return ref


# ---- 1. against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("F,K,unbinned,one,lrange", CASES)
def test_grad(F, K, unbinned, one, lrange):
    cs = case(F, K, unbinned, one, lrange=lrange)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    out = bank.loglike_grad(cs["theory"])
    check(out, cs["rows"], cs, f"F {F} K {K} Ju {bank.Ju}")
    a = bank.loglike(cs["theory"])
    assert all(np.array_equal(a[k], out[k]) for k in a)
    assert set(out) == set(a) | {"grad", "mean_scale", "chain_weight"}


def test_cases_cover_tiles():
    gr, tm, ct = grad_info()
    ju = [len(case(F, K, u, o, lrange=lr)["tables"]["cols"]) for F, K, u, o, lr in CASES]
    assert any(j % 4 for j in ju) and any(j % 4 and j > 4 for j in ju), ju
    assert any(j > ct and j % ct for j in ju), (ju, ct)          # several column tiles, the last one partial
    assert any(j < 16 for j in ju) and any(16 < j < ct for j in ju)
    assert tm < 70 < 2 * tm                                      # test_two_model_tiles


def test_two_model_tiles():
    cs = case(3, 70)
    assert len(cs["tables"]["cols"]) == 28
    check(bank_of(cs, cuts=(3, 4), cap=4).loglike_grad(cs["theory"]), cs["rows"], cs, "K 70")


@pytest.fixture(scope="module")
def long_case():
    return case(3, 5, T=2 * grad_info()[0] + 5, C=2)


def test_three_blocks(long_case):
    cs = long_case
    T = cs["rows"].shape[0]
    assert T == 2 * grad_info()[0] + 5 and T % 16 != 0
    bank = bank_of(cs, cap=64)
    check(bank.loglike_grad(cs["theory"]), cs["rows"], cs, f"three blocks n {T}")


def test_bad_rows():
    cs = case(3, 5)
    bad = cs["rows"].copy()
    bad[2, 1, 2, 3] = 0.0                                               # beta = 0 (BB) for chain 1
    bad[5, 2, 3, 6] = 2.0 * np.sqrt(bad[5, 2, 0, 6] * bad[5, 2, 1, 6])  # c^2 = 4 a dd for chain 2
    bad[4, 0, 2, 4] = np.inf                                            # the bank row holds an infinity
    bad[6, 0, 0, 5] = np.nan                                            # and a NaN
    bank = bank_of(cs, rows=bad, cuts=(3, 4), cap=4)
    assert int(torch.isnan(bank.r).sum()) == 4 and not torch.isfinite(bank.X).all()
    out = bank.loglike_grad(cs["theory"])
    assert np.array_equal(out["bad"], [2, 1, 1]) and out["n"] == 7
    assert np.isfinite(out["mean_scale"][:, cs["mask"]]).all()
    check(out, bad, cs, "bad rows")


def test_dominated():
    """One row's t is 800 above every other: xbar is that row's x, the other weights underflow."""
    cs = case(3, 5)
    rows = 3.0 * cs["rows"]
    rows[3, 1] = cs["rows"][3, 1]
    flat = rows.reshape(7, 3, -1)
    t, _ = B.terms(flat, cs["tables"], cs["maxbins"])
    rest = np.delete(t.reshape(21, -1), 1 * 7 + 3, axis=0)
    assert np.all(t[1, 3] - rest.max(axis=0) >= 800.0)
    out = bank_of(cs, rows=rows, cuts=(3, 4), cap=4).loglike_grad(cs["theory"])
    ref = check(out, rows, cs, "dominated")
    x = flat[3, 1][cs["tables"]["cols"]]
    assert np.array_equal(ref["xbar"], np.broadcast_to(x, ref["xbar"].shape))
    xb = out["mean_scale"].reshape(5, -1)[:, cs["tables"]["cols"]]
    assert np.array_equal(xb, ref["xbar"])                              # one weight of exactly 1, the rest 0
    want = np.zeros((3, 5))
    want[1] = 1.0
    assert np.array_equal(out["chain_weight"], want)


def test_empty():
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = case(3, 5)
    bank = BlackwellRaoSamples(4, 3, cs["bins"], cs["mask"], 5)
    out = bank.loglike_grad(cs["theory"])
    assert out["n"] == 0 and np.isnan(out["loglike"]).all() and np.isnan(out["chain_weight"]).all()
    assert out["chain_weight"].shape == (4, 5) and np.isnan(out["mean_scale"]).all()
    used = np.zeros(cs["mask"].size, dtype=bool)
    used[cs["tables"]["cols"]] = True
    for k, s in enumerate(("TT", "EE", "BB", "TE")):
        u = used.reshape(cs["mask"].shape)[k, :out["grad"][s].shape[1]]
        assert np.isnan(out["grad"][s][:, u]).all() and not out["grad"][s][:, ~u].any()
    num = bank.grad_numerators(cs["tables"]["Y"], np.zeros(5))
    torch.cuda.synchronize()
    assert tuple(num.shape) == (4, 5, bank.Jp) and not num.any()


# ---- 2. bit equality -------------------------------------------------------------------------------------
def mref_of(bank, tables):
    f = bank.fields(bank.evaluate(tables["Y"]))
    assert bool((f[1] > 0).all())
    return f[0].amax(dim=0)


@pytest.mark.parametrize("unbinned", [False, True])
def test_bit_equality(unbinned):
    cs = case(3, 5, unbinned)
    tables = cs["tables"]
    ref = bank_of(cs, cuts=(7,), cap=8)
    mref = mref_of(ref, tables)
    num = ref.grad_numerators(tables["Y"], mref)
    assert tuple(num.shape) == (3, 5, ref.Jp) and not num[:, :, ref.Ju:].any() and bool((num[:, :, :ref.Ju] != 0).any())
    # model 4 of K = 5 is the same model run as K = 1 with the same reference
    one = ref.grad_numerators(tables["Y"][4:5].copy(), mref[4:5].clone())
    assert torch.equal(one[:, 0], num[:, 4])
    # chain 2 alone is chain 2 of the three
    solo = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    assert torch.equal(solo.grad_numerators(tables["Y"], mref)[0], num[2])
    # other ring capacities, cuts and a bank with room to spare
    for cuts, cap, capacity in (((3, 4), 4, None), ((1,) * 7, 1, None), ((4, 3), 4, 19)):
        got = bank_of(cs, cuts=cuts, cap=cap, capacity=capacity)
        assert torch.equal(got.grad_numerators(tables["Y"], mref), num), (cuts, cap)
    # twice the same
    assert torch.equal(ref.grad_numerators(tables["Y"], mref), num)
    a, b = ref.loglike_grad(cs["theory"]), ref.loglike_grad(cs["theory"])
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if k != "grad")
    assert all(np.array_equal(a["grad"][s], b["grad"][s]) for s in a["grad"])


def test_bit_equality_blocks(long_case):
    cs = long_case
    tables = cs["tables"]
    ref = bank_of(cs, cap=64)
    mref = mref_of(ref, tables)
    num = ref.grad_numerators(tables["Y"], mref)
    assert torch.equal(ref.grad_numerators(tables["Y"][4:5].copy(), mref[4:5].clone())[:, 0], num[:, 4])
    solo = bank_of(cs, rows=cs["rows"][:, 1:], cap=37)
    assert torch.equal(solo.grad_numerators(tables["Y"], mref)[0], num[1])


# ---- 3. gather -----------------------------------------------------------------------------------------------
def test_gather():
    cs = case(3, 5, C=4)
    tables = cs["tables"]
    whole = bank_of(cs, cuts=(3, 4), cap=4)
    lo = bank_of(cs, rows=cs["rows"][:, :2], cuts=(3, 4), cap=4)
    hi = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    hi_fields = hi.fields(hi.evaluate(tables["Y"]))
    hi_num = hi.grad_numerators(tables["Y"], mref_of(whole, tables))
    calls = []

    def gather(t, dim=0):
        calls.append((tuple(t.shape), dim))
        return torch.cat([t, hi_fields if dim == 1 else hi_num], dim=dim)

    got, want = lo.loglike_grad(cs["theory"], gather), whole.loglike_grad(cs["theory"])
    assert calls == [((3, 2, 5), 1), ((2, 5, lo.Jp), 0)]
    for k in ("loglike", "chain_loglike", "neff", "mean_scale", "chain_weight"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert all(np.array_equal(got["grad"][s], want["grad"][s]) for s in want["grad"])
    assert got["chain_weight"].shape == (4, 5)
    check(got, cs["rows"], cs, "gathered")


# ---- 4. the surface -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["centered", "asis"])
def test_surface(kind, tmp_path):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    model, init, theory = _problem()
    T = 40
    r = L.make_runner(model, kind, 4)
    r.run(init, T, graph_chunk=32, br_samples=S.OPTS, keep_scales=True)
    bank = r.br_samples()
    p = r.plan
    hs = np.full((T, 4, p.nspec, p.maxbins), np.nan)
    for k, s in enumerate(model.spectra):
        hs[:, :, k, :model.nbins(s)] = r.h_scales[s]
    out = bank.loglike_grad(theory)
    tables = bank.tables(theory)
    from gibbssampler_amd.samplers import br_theory
    th = br_theory("test", theory, 3, bank.bins, bank.mask)
    cs = {"F": 3, "bins": bank.bins, "mask": bank.mask, "maxbins": p.maxbins}
    check(out, hs, cs, f"surface {kind}", tables=tables, theory=th)
    a = bank.loglike(theory)
    assert all(np.array_equal(a[k], out[k]) for k in a)
    assert set(out["grad"]) == set(model.spectra) and out["grad"]["TT"].shape == (4, model.nbins("TT"))
    assert np.all(np.isfinite(out["grad"]["TT"])) and out["chain_weight"].shape == (4, 4)
    path = os.path.join(tmp_path, "bank.npz")
    bank.save(path)
    back = BlackwellRaoSamples.load(path).loglike_grad(theory)
    assert all(np.array_equal(back[k], out[k], equal_nan=True) for k in out if k != "grad")
    assert all(np.array_equal(back["grad"][s], out["grad"][s]) for s in out["grad"])
    with pytest.raises(ValueError, match="positive but for TE"):
        bank.loglike_grad({s: -v for s, v in theory.items()})


def _problem():
    from tests import _mh_adapt as A
    model, init = A.small_problem(3)
    fac = (0.5, 1.0, 2.0, 1.0)
    theory = {s: np.stack([f * np.asarray(init[s], dtype=np.float64) for f in fac]) for s in model.spectra}
    theory["TE"][3] *= -1.0
    return model, init, theory


def test_class_surface():
    from gibbssampler_amd import gibbs
    model, init, theory = _problem()
    d = {k: model.d_alm[i] for i, k in enumerate(("TT", "EE", "BB"))}
    fwhm = max(0.5, 180.0 / model.L * 2)
    npix = 12 * model.nside ** 2
    args = (d, model.noise_var[0], model.noise_var[-1], fwhm, model.nside, model.L, npix)
    kw = dict(polarization=True, bins=model.bins, n_iter=20, all_sph=True, nchains=2, seed=S.SEED, fields="TEB",
              br_samples={"lrange": (2, 30)})
    for cls in (gibbs.CenteredGibbs, gibbs.ASIS):
        extra = (model.proposal_variances,) if cls is gibbs.ASIS else ()
        more = {"metropolis_blocks": model.blocks} if cls is gibbs.ASIS else {}
        g = cls(*args, *extra, **more, **kw)
        g.run(init)
        bank = g.blackwell_rao_samples
        got, a = bank.loglike_grad(theory), bank.loglike(theory)
        assert set(got) == {"loglike", "chain_loglike", "neff", "n", "bad", "grad", "mean_scale", "chain_weight"}
        assert all(np.array_equal(a[k], got[k]) for k in a) and got["n"] == 20
        assert got["chain_weight"].shape == (2, 4) and np.allclose(got["chain_weight"].sum(axis=0), 1.0, rtol=1e-12)
        assert all(got["grad"][s].shape == (4, model.nbins(s)) and np.all(np.isfinite(got["grad"][s]))
                   for s in model.spectra)
        assert got["mean_scale"].shape == (4, bank.nspec, bank.maxbins)


# ---- 5. argument checks ------------------------------------------------------------------------------------
def test_argument_checks():
    from gibbssampler_amd import _capi as C
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4, capacity=9)
    lib = bank.lib
    Y = torch.from_numpy(cs["tables"]["Y"]).cuda()
    mref = torch.zeros(5, dtype=torch.float64, device="cuda")
    wb = ctypes.c_longlong()
    assert lib.gs_brs_grad_work_bytes(3, 7, 5, bank.Ju, ctypes.byref(wb)) == 0 and wb.value == 8 * 3 * 5 * bank.Jp
    gr = grad_info()[0]
    assert lib.gs_brs_grad_work_bytes(3, 2 * gr + 1, 5, bank.Ju, ctypes.byref(wb)) == 0
    assert wb.value == 8 * 3 * 3 * 5 * bank.Jp
    assert lib.gs_brs_grad_work_bytes(3, 7, 0, bank.Ju, ctypes.byref(wb)) == -1
    work = torch.zeros(3 * 5 * bank.Jp, dtype=torch.float64, device="cuda")
    num = torch.zeros(3, 5, bank.Jp, dtype=torch.float64, device="cuda")
    gd = lambda X, n, K, Yp, mp, w, nb, o: lib.gs_brs_grad(X, C.ptr(bank.r), 3, 9, n, bank.Ju, K, Yp, mp, w, nb, o, None)  # noqa: E731
    full = work.numel() * 8
    assert gd(None, 7, 5, C.ptr(Y), C.ptr(mref), C.ptr(work), full, C.ptr(num)) == -1
    assert b"null bank" in lib.gs_last_error()
    assert gd(C.ptr(bank.X), 7, 5, C.ptr(Y), C.ptr(mref), C.ptr(work), full, None) == -1
    assert b"null num" in lib.gs_last_error()
    assert gd(C.ptr(bank.X), 7, 5, C.ptr(Y), None, C.ptr(work), full, C.ptr(num)) == -1
    assert b"null Y, mref or workspace" in lib.gs_last_error()
    assert gd(C.ptr(bank.X), 10, 5, C.ptr(Y), C.ptr(mref), C.ptr(work), full, C.ptr(num)) == -1
    assert b"[0, cap]" in lib.gs_last_error()
    assert gd(C.ptr(bank.X), 7, 5, C.ptr(Y), C.ptr(mref), C.ptr(work), full - 8, C.ptr(num)) == -1
    assert b"workspace is smaller" in lib.gs_last_error()
    assert lib.gs_brs_grad_finish(C.ptr(num), None, 3, 5, bank.Ju, C.ptr(num), C.ptr(num), None) == -1
    assert b"null argument" in lib.gs_last_error()
    with pytest.raises(ValueError, match=r"Y must be \[K, Ju\]"):
        bank.grad_numerators(cs["tables"]["Y"][:, :5], mref)
    with pytest.raises(ValueError, match=r"mref \[K\]"):
        bank.grad_numerators(cs["tables"]["Y"], mref[:4])
    torch.cuda.synchronize()
    assert not num.any() and not work.any()
