"""GPU: the Blackwell-Rao sample bank (gs_brs_*, engine.BlackwellRaoSamples) and
BatchedRunner.run(br_samples=) with the class surface.

The bank's loglike, chain_loglike and neff are compared with tests/_br_samples.py
(order-free longdouble sums).  Bound, derived and not tuned: with delta_k = (Ju +
16) 2^-52 T_k the per-sample bound of tests/test_gpu_br_likelihood.py (T_k:
_br_likelihood.term_bound),
    |d loglike|, |d chain_loglike| <= delta_k + n 2^-52
    |d neff|                       <= neff (4 delta_k + 2 n 2^-52)
the second term for the device's re-ordered sum of a chain's n weights (lanes,
lane groups, waves, slices: gs_brs.hip).  Against the streaming estimator both
sides carry delta_k: twice the bound.  Largest |device - numpy| / bound seen on
an MI355X: see DESIGN.md 'Blackwell-Rao sample bank'."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_likelihood as R  # noqa: E402
from tests import _br_samples as B  # noqa: E402
from tests import _mh_adapt as A  # noqa: E402
from tests import test_gpu_br_likelihood as L  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = L.SEED


def slice_rows():
    import ctypes
    from gibbssampler_amd import _capi as C
    sl, tm = ctypes.c_int(), ctypes.c_int()
    assert C.load().gs_brs_info(ctypes.byref(sl), ctypes.byref(tm)) == 0
    assert sl.value >= 16 and sl.value % 16 == 0 and tm.value % 16 == 0
    return sl.value


def case(F, K, unbinned=False, one=False, T=7, C=3, lrange=None):
    """rows [T, C, nspec, maxbins] (NaN off the used set), theory, mask, bins, tables, maxbins."""
    from gibbssampler_amd.engine import br_likelihood_mask, br_likelihood_tables
    bins = L.bins_of(F, unbinned)
    mask = None
    if one:                                                     # Ju = 1: one inverse-Gamma bin
        mask = np.zeros_like(br_likelihood_mask(F, bins))
        mask[-2 if F == 3 else -1, 3] = True
    if lrange is not None:
        mask = br_likelihood_mask(F, bins, None, lrange)
    rows, theory, mask = R.synthetic(F, bins, K, T, C, SEED, mask)
    return {"F": F, "rows": rows, "theory": theory, "mask": mask, "bins": bins, "maxbins": mask.shape[1],
            "tables": br_likelihood_tables(F, bins, theory, mask)}


def bank_of(cs, rows=None, cuts=None, cap=8, capacity=None):
    """rows through a ring of cap slots in launches of `cuts` rows into a new bank."""
    from gibbssampler_amd.engine import BlackwellRaoSamples
    rows = cs["rows"] if rows is None else rows
    T, C = rows.shape[:2]
    bank = BlackwellRaoSamples(C, cs["F"], cs["bins"], cs["mask"], T if capacity is None else capacity)
    x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    ring = torch.full((cap,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    it, row = 1, 0
    for k in (cuts if cuts is not None else [min(cap, T - i) for i in range(0, T, cap)]):
        for i in range(k):
            ring[(it + i - 1) % cap].copy_(x[row + i])
        bank.append(ring, cap, it, k)
        it, row = it + k, row + k
    torch.cuda.synchronize()
    assert bank.n == T
    return bank


def fields(bank, tables):
    return bank.fields(bank.evaluate(tables["Y"]))


def check(out, rows, tables, maxbins, what, factor=1.0, want=None):
    """out against the restatement of rows [T, C, nspec, maxbins] (or against
    `want`, another estimate of the same rows) within factor x the bound."""
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    ref = B.loglike(flat, tables, maxbins)
    if want is None:
        want = ref
        assert out["n"] == ref["n"] == T and np.array_equal(np.asarray(out["bad"]), ref["bad"]), what
    delta, slack = B.bounds(flat, tables, maxbins)
    ne = ref["neff"]
    bound = {"loglike": delta + slack, "chain_loglike": (delta + slack)[None, :], "neff": ne * (4 * delta + 2 * slack)}
    worst = 0.0
    for name in ("loglike", "chain_loglike", "neff"):
        got, w = np.asarray(out[name]), np.asarray(want[name])
        assert got.shape == w.shape and np.array_equal(np.isnan(got), np.isnan(w)), (what, name)
        ok = ~np.isnan(w)
        ratio = float(np.max((np.abs(got - w) / np.broadcast_to(factor * bound[name], w.shape))[ok])) if ok.any() else 0.0
        print(f"  {what} {name}: max |device - reference| / bound = {ratio:.4f} (Ju {len(tables['cols'])}, n {T}, "
              f"max bound {factor * np.max(bound[name]):.3e})")
        worst = max(worst, ratio)
    assert worst <= 1.0, what
    return out


CASES = [(3, 5, False, False, None), (3, 21, False, False, None), (3, 5, False, True, None),
         (3, 5, True, False, None), (1, 5, False, False, None), (2, 5, False, False, None),
         (2, 3, False, True, None), (3, 5, False, False, (2, 5)), (1, 5, True, False, None)]


# ---- 1. evaluation against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("F,K,unbinned,one,lrange", CASES)
def test_eval(F, K, unbinned, one, lrange):
    cs = case(F, K, unbinned, one, lrange=lrange)
    Ju = len(cs["tables"]["cols"])
    if one:
        assert Ju == 1
    if unbinned:
        assert Ju == (252 if F == 3 else 63)                # 63: two stages of 32 columns, the second padded
    if lrange is not None:
        assert Ju == 10                                     # Jp = 12
    if not one and not unbinned and F == 3 and lrange is None:
        assert Ju == 28
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    assert bank.Ju == Ju and bank.Jp == (Ju + 3) // 4 * 4 and tuple(bank.X.shape) == (3, 7, bank.Jp)
    check(bank.loglike(cs["theory"]), cs["rows"], cs["tables"], cs["maxbins"], f"F {F} K {K} Ju {Ju}")


def test_cases_cover_padding():
    ju = [len(case(F, K, u, o, lrange=lr)["tables"]["cols"]) for F, K, u, o, lr in CASES]
    assert any(j % 4 for j in ju) and any(j % 4 and j > 4 for j in ju), ju


@pytest.fixture(scope="module")
def long_case():
    return case(3, 5, T=2 * slice_rows() + 5)


def test_eval_three_slices(long_case):
    cs = long_case
    SL = slice_rows()
    T = cs["rows"].shape[0]
    assert T == 2 * SL + 5 and T % 16 != 0
    bank = bank_of(cs, cap=64)
    check(bank.loglike(cs["theory"]), cs["rows"], cs["tables"], cs["maxbins"], f"three slices n {T}")


# ---- 2. agreement with the streaming estimator ----------------------------------------------------------
@pytest.mark.parametrize("F,K,unbinned", [(3, 5, False), (3, 5, True), (2, 5, False)])
def test_streaming_agreement(F, K, unbinned):
    cs = case(F, K, unbinned)
    st = L.feed(L.new_state(cs["rows"], cs["tables"], cs["maxbins"]), cs["rows"], (3, 4))
    want = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in st.finish().items()}
    out = bank_of(cs, cuts=(3, 4), cap=4).loglike(cs["theory"])
    assert out["n"] == want["n"] == 7 and np.array_equal(out["bad"], st.bad().cpu().numpy())
    check(out, cs["rows"], cs["tables"], cs["maxbins"], f"streaming F {F}", factor=2.0, want=want)


# ---- 3. bit equality ------------------------------------------------------------------------------------
@pytest.mark.parametrize("unbinned", [False, True])
def test_bit_equality(unbinned):
    cs = case(3, 5, unbinned)
    tables = cs["tables"]
    ref = bank_of(cs, cuts=(7,), cap=8)
    # (3, 4) in 4 slots: the second launch starts in slot 3 and wraps; (4, 3): a cut at the wrap
    for cuts, cap in (((3, 4), 8), ((1,) * 7, 8), ((3, 4), 4), ((4, 3), 4), ((1,) * 7, 1)):
        got = bank_of(cs, cuts=cuts, cap=cap)
        assert torch.equal(got.X, ref.X) and torch.equal(got.r, ref.r), (cuts, cap)
    # a bank with room to spare holds the same rows
    big = bank_of(cs, cuts=(3, 4), cap=4, capacity=19)
    assert torch.equal(big.X[:, :7], ref.X) and torch.equal(big.r[:, :7], ref.r)
    f = fields(ref, tables)
    assert torch.equal(fields(big, tables), f)
    # chain 2 alone is chain 2 of the three
    solo = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    assert torch.equal(solo.X[0], ref.X[2]) and torch.equal(solo.r[0], ref.r[2])
    assert torch.equal(fields(solo, tables)[:, 0], f[:, 2])
    # model 4 of K = 5 is the same model run as K = 1
    one = ref.loglike(cs["theory"][4:5])
    assert torch.equal(fields(ref, {"Y": tables["Y"][4:5].copy()})[:, :, 0], f[:, :, 4])
    a = ref.loglike(cs["theory"])
    assert np.array_equal(one["loglike"][0], a["loglike"][4])
    assert np.array_equal(one["chain_loglike"][:, 0], a["chain_loglike"][:, 4])
    # twice the same
    b = ref.loglike(cs["theory"])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert torch.equal(fields(ref, tables), f)


def test_bit_equality_slices_and_padding(long_case):
    # three slices: chain 2 alone, model 4 alone
    cs = long_case
    tables = cs["tables"]
    ref = bank_of(cs, cap=64)
    f = fields(ref, tables)
    solo = bank_of(cs, rows=cs["rows"][:, 2:], cap=37)
    assert torch.equal(solo.X[0], ref.X[2]) and torch.equal(solo.r[0], ref.r[2])
    assert torch.equal(fields(solo, tables)[:, 0], f[:, 2])
    assert torch.equal(fields(ref, {"Y": tables["Y"][4:5].copy()})[:, :, 0], f[:, :, 4])
    # the padding columns are exactly 0 (Ju = 1 -> Jp = 4, Ju = 10 -> Jp = 12)
    for kw in ({"one": True}, {"lrange": (2, 5)}):
        cp = case(3, 5, **kw)
        bank = bank_of(cp, cuts=(3, 4), cap=4)
        assert bank.Jp > bank.Ju and not bank.X[:, :, bank.Ju:].any()
        assert not torch.isnan(bank.X).any()


# ---- 4. bad rows ------------------------------------------------------------------------------------------
def test_bad_rows():
    cs = case(3, 5)
    rows, tables, maxbins = cs["rows"], cs["tables"], cs["maxbins"]
    bad = rows.copy()
    bad[2, 1, 2, 3] = 0.0                                               # beta = 0 (BB) for chain 1
    bad[5, 2, 3, 6] = 2.0 * np.sqrt(bad[5, 2, 0, 6] * bad[5, 2, 1, 6])  # c^2 = 4 a dd for chain 2
    bb = bank_of(cs, rows=bad, cuts=(3, 4), cap=4)
    out = bb.loglike(cs["theory"])
    assert np.array_equal(out["bad"], [0, 1, 1]) and out["n"] == 7
    assert bool(torch.isnan(bb.r[1, 2])) and bool(torch.isnan(bb.r[2, 5])) and int(torch.isnan(bb.r).sum()) == 2
    check(out, bad, tables, maxbins, "bad rows")
    # each is skipped for its chain only: the other chains keep the clean bank's bits
    clean = bank_of(cs, cuts=(3, 4), cap=4)
    fb, fc = fields(bb, tables), fields(clean, tables)
    assert torch.equal(fb[:, 0], fc[:, 0])
    # and a chain with a skipped row gives what its other six rows alone give
    # (the six rows sit in other lanes: the same weights, added in another order)
    lse = lambda f: f[0] + np.log(f[1])          # noqa: E731
    neff = lambda f: f[1] ** 2 / f[2]            # noqa: E731
    for chain, row in ((1, 2), (2, 5)):
        six = np.delete(rows[:, chain:chain + 1], row, axis=0)
        fa = fields(bank_of(cs, rows=six, cuts=(3, 3), cap=4), tables)[:, 0].cpu().numpy()
        fg = fb[:, chain].cpu().numpy()
        delta, slack = B.bounds(six.reshape(6, 1, -1), tables, maxbins)
        assert np.array_equal(fa[0], fg[0]), chain                      # the maximum is order-free
        assert np.all(np.abs(lse(fg) - lse(fa)) <= delta + slack), chain
        assert np.all(np.abs(neff(fg) - neff(fa)) <= neff(fa) * (4 * delta + 2 * slack)), chain
    # a value in an unused column changes nothing (the synthetic rows hold NaN there already)
    other = rows.copy()
    other[:, :, 2, 7:] = 3.0
    other[:, :, :, :2] = -1.0
    o = bank_of(cs, rows=other, cuts=(3, 4), cap=4)
    assert torch.equal(o.X, clean.X) and torch.equal(o.r, clean.r) and torch.equal(fields(o, tables), fc)


# ---- 5. gather and empty -------------------------------------------------------------------------------
def test_gather_and_empty():
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = case(3, 5, C=4)
    tables = cs["tables"]
    whole = bank_of(cs, cuts=(3, 4), cap=4)
    lo = bank_of(cs, rows=cs["rows"][:, :2], cuts=(3, 4), cap=4)
    hi = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    assert torch.equal(torch.cat([fields(lo, tables), fields(hi, tables)], dim=1), fields(whole, tables))
    calls = []

    def gather(t, dim=0):
        calls.append(tuple(t.shape))
        return torch.cat([t, fields(hi, tables)], dim=dim)

    got, want = lo.loglike(cs["theory"], gather), whole.loglike(cs["theory"])
    assert calls == [(3, 2, 5)] and got["n"] == want["n"] == 7
    for k in ("loglike", "chain_loglike", "neff"):
        assert np.array_equal(got[k], want[k]), k
    empty = BlackwellRaoSamples(4, 3, cs["bins"], cs["mask"], 5).loglike(cs["theory"])
    assert empty["n"] == 0 and all(np.isnan(empty[k]).all() for k in ("loglike", "chain_loglike", "neff"))
    assert empty["loglike"].shape == (5,) and empty["chain_loglike"].shape == (4, 5) and not empty["bad"].any()


# ---- 6. save and load ----------------------------------------------------------------------------------
def test_save_load(tmp_path):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4, capacity=11)
    path = os.path.join(tmp_path, "bank.npz")
    bank.save(path)
    with np.load(path, allow_pickle=False) as f:
        assert f["X"].shape == (3, 7, bank.Jp) and f["r"].shape == (3, 7) and int(f["nfields"]) == 3
        assert np.array_equal(f["cols"], cs["tables"]["cols"]) and np.array_equal(f["mask"], cs["mask"])
        assert np.array_equal(f["bins_BB"], L.BINS_B)
    back = BlackwellRaoSamples.load(path)
    assert back.n == 7 and torch.equal(back.X, bank.X[:, :7]) and torch.equal(back.r, bank.r[:, :7])
    a, b = bank.loglike(cs["theory"]), back.loglike(cs["theory"])
    assert set(a) == {"loglike", "chain_loglike", "neff", "n", "bad"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # a checkpoint's state likewise
    again = BlackwellRaoSamples.from_state(bank.state(), 3, cs["bins"], capacity=20)
    assert again.capacity == 20 and all(np.array_equal(a[k], again.loglike(cs["theory"])[k]) for k in a)
    with pytest.raises(ValueError, match=r"\[K, nspec, maxbins\]"):
        back.loglike(cs["theory"][:, :, :5])
    with pytest.raises(ValueError, match=r"theory\[TT\] must be \[K, nbins\]"):
        back.loglike({s: cs["theory"][:, k, :3] for k, s in enumerate(("TT", "EE", "BB", "TE"))})
    t = cs["theory"].copy()
    t[0, 2, 3] = -1.0
    with pytest.raises(ValueError, match="positive but for TE"):
        back.loglike(t)


# ---- 7. the surface ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    model, init = A.small_problem(3)
    fac = (0.5, 1.0, 2.0, 1.0)
    theory = {s: np.stack([f * np.asarray(init[s], dtype=np.float64) for f in fac]) for s in model.spectra}
    theory["TE"][3] *= -1.0
    return model, init, theory


T = 70
OPTS = {"lrange": (2, 12)}


@pytest.fixture(scope="module")
def plain(problem):
    model, init, _ = problem
    return {kind: L.make_runner(model, kind, 4).run(init, T) for kind in ("centered", "asis")}


@pytest.mark.parametrize("kind", ["centered", "asis"])
def test_surface(kind, problem, plain):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    model, init, theory = problem
    h0, a0 = plain[kind]
    banks = []
    for gc in (32, 0):
        r = L.make_runner(model, kind, 4)
        h, a = r.run(init, T, graph_chunk=gc, br_samples=OPTS, keep_scales=True)
        assert L.same(h0, h) and L.same(a0, a), (kind, gc)
        bank = r.br_samples()
        assert isinstance(bank, BlackwellRaoSamples) and bank.n == T and r.plan.scale_trace is None
        banks.append(bank)
    torch.cuda.synchronize()
    assert torch.equal(banks[0].X[:, :T], banks[1].X[:, :T]) and torch.equal(banks[0].r[:, :T], banks[1].r[:, :T])
    # the bank is the kept scale history at the used columns
    p = r.plan
    hs = np.full((T, 4, p.nspec, p.maxbins), np.nan)
    for k, s in enumerate(model.spectra):
        hs[:, :, k, :model.nbins(s)] = r.h_scales[s]
    cols = bank.cols.cpu().numpy()
    assert len(cols) == 11 * 3 + int(np.sum((model.bins["BB"][2:-1] >= 2) & (model.bins["BB"][3:] - 1 <= 12)))
    X = bank.X[:, :T].cpu().numpy()
    assert np.array_equal(X[:, :, :bank.Ju], hs.reshape(T, 4, -1)[:, :, cols].transpose(1, 0, 2))
    assert not X[:, :, bank.Ju:].any()
    # loglike(theory) against the restatement on the kept scales, and against a run
    # that was given the theory beforehand
    res = bank.loglike(theory)
    tables = bank.tables(theory)
    check(res, hs, tables, p.maxbins, f"surface {kind}")
    assert res["loglike"].shape == (4,) and res["chain_loglike"].shape == (4, 4) and np.all(np.isfinite(res["loglike"]))
    fixed = L.make_runner(model, kind, 4)
    fixed.run(init, T, br_likelihood=dict(OPTS, theory=theory))
    check(res, hs, tables, p.maxbins, f"surface {kind} against br_likelihood=", factor=2.0, want=fixed.br_likelihood())
    # together with the other consumers of the scale ring: none moves another
    both = L.make_runner(model, kind, 4)
    hb, _ = both.run(init, T, blackwell_rao=L.BR_OPTS, br_likelihood=dict(OPTS, theory=theory), br_samples=OPTS,
                     summary=True)
    assert L.same(h0, hb) and torch.equal(both._brl.data, fixed._brl.data)
    assert torch.equal(both.br_samples().X[:, :T], bank.X[:, :T]) and torch.equal(both.br_samples().r[:, :T], bank.r[:, :T])
    # 40 + 30 through a state_dict and a new runner
    a1 = L.make_runner(model, kind, 4)
    a1.run(init, 40, br_samples=OPTS)
    st = a1.state_dict()
    assert st["brs_start"] == 0 and tuple(st["brs_X"].shape) == (4, 40, bank.Jp) and tuple(st["brs_r"].shape) == (4, 40)
    b1 = L.make_runner(model, kind, 4)
    b1.run(None, 30, resume=st)
    got = b1.br_samples()
    assert got.n == T and torch.equal(got.X[:, :T], bank.X[:, :T]) and torch.equal(got.r[:, :T], bank.r[:, :T])
    again = got.loglike(theory)
    assert all(np.array_equal(again[k], res[k]) for k in res)
    # a state without the keys is "off"
    b1.run(None, 3, resume={k: v for k, v in st.items() if not k.startswith("brs_")})
    assert b1._brs is None
    with pytest.raises(RuntimeError, match="br_samples"):
        b1.br_samples()
    # no history; start
    c = L.make_runner(model, kind, 4)
    assert c.run(init, T, br_samples=OPTS, keep_history=False) == (None, None)
    assert torch.equal(c.br_samples().X[:, :T], bank.X[:, :T])
    c.run(init, T, br_samples=dict(OPTS, start=10))
    cb = c.br_samples()
    assert cb.n == 60 and c.brs_start == 10 and c.plan.scale_trace is None
    assert torch.equal(cb.X[:, :60], bank.X[:, 10:T]) and torch.equal(cb.r[:, :60], bank.r[:, 10:T])


def test_refusals_and_class_surface(problem):
    from gibbssampler_amd import gibbs
    from gibbssampler_amd.engine import BlackwellRaoSamples
    model, init, theory = problem
    with pytest.raises(NotImplementedError, match="non-centered"):
        L.make_runner(model, "noncentered", 2).run(init, 4, br_samples=OPTS)
    with pytest.raises(ValueError, match="unknown options"):
        L.make_runner(model, "centered", 2).run(init, 4, br_samples=dict(OPTS, theory=theory))
    d = {k: model.d_alm[i] for i, k in enumerate(("TT", "EE", "BB"))}
    fwhm = max(0.5, 180.0 / model.L * 2)
    npix = 12 * model.nside ** 2
    args = (d, model.noise_var[0], model.noise_var[-1], fwhm, model.nside, model.L, npix)
    kw = dict(polarization=True, bins=model.bins, n_iter=20, all_sph=True, nchains=2, seed=SEED, fields="TEB",
              br_samples=OPTS)
    with pytest.raises(NotImplementedError, match="non-centered"):
        gibbs.NonCenteredGibbs(*args, model.proposal_variances, metropolis_blocks=model.blocks, **kw)
    with pytest.raises(NotImplementedError, match="masked"):
        gibbs.CenteredGibbs(*args, mask_path=np.ones(npix), **kw)
    with pytest.raises(ValueError, match="unknown options"):
        gibbs.CenteredGibbs(*args, **dict(kw, br_samples=dict(OPTS, points=3)))
    for cls in (gibbs.CenteredGibbs, gibbs.ASIS):
        extra = (model.proposal_variances,) if cls is gibbs.ASIS else ()
        more = {"metropolis_blocks": model.blocks} if cls is gibbs.ASIS else {}
        g = cls(*args, *extra, **more, **kw)
        with pytest.raises(RuntimeError, match="nothing has run"):
            g.blackwell_rao_samples
        g.run(init)
        bank = g.blackwell_rao_samples
        assert isinstance(bank, BlackwellRaoSamples) and bank is g._runner.br_samples() and bank.n == 20
        got = bank.loglike(theory)
        assert set(got) == {"loglike", "chain_loglike", "neff", "n", "bad"} and got["n"] == 20
        assert got["loglike"].shape == (4,) and got["chain_loglike"].shape == (2, 4) and np.all(np.isfinite(got["loglike"]))


# ---- 8. argument checks -------------------------------------------------------------------------------
def test_argument_checks():
    from gibbssampler_amd import _capi as C
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4, capacity=9)
    X0, r0 = bank.X.clone(), bank.r.clone()
    lib, nsp, mb = bank.lib, bank.nspec, bank.maxbins
    ring = torch.zeros(4, 3, nsp, mb, dtype=torch.float64, device="cuda")
    tab = (C.ptr(bank.cols), C.ptr(bank.kind), C.ptr(bank.coef))
    # append
    assert lib.gs_brs_append(None, C.ptr(bank.r), 3, 9, bank.Ju, nsp, mb, *tab, C.ptr(ring), 4, 1, 1, 7, None) == -1
    assert b"null bank" in lib.gs_last_error()
    assert lib.gs_brs_append(C.ptr(bank.X), C.ptr(bank.r), 3, 9, bank.Ju, nsp, mb, None, None, None, None, 4, 1, 1, 7,
                             None) == -1
    assert b"null table" in lib.gs_last_error()
    assert lib.gs_brs_append(C.ptr(bank.X), C.ptr(bank.r), 3, 9, bank.Ju, nsp, mb, *tab, C.ptr(ring), 4, 1, 3, 7,
                             None) == -1
    assert b"row0 + nsteps <= cap" in lib.gs_last_error()
    assert lib.gs_brs_append(C.ptr(bank.X), C.ptr(bank.r), 3, 9, bank.Ju, nsp, mb, *tab, C.ptr(ring), 4, 1, 5, 0,
                             None) == -1
    assert b"nsteps <= capacity" in lib.gs_last_error()
    with pytest.raises(C.GibbsHipError, match="row0 \\+ nsteps <= cap"):
        bank.append(ring, 4, 8, 3)
    assert bank.n == 7
    with pytest.raises(ValueError, match="smaller than ring_capacity"):
        bank.append(ring, 5, 8, 1)
    # eval
    Y = torch.from_numpy(cs["tables"]["Y"]).cuda()
    state = torch.zeros(8 + 3 * 3 * 5 + 3, dtype=torch.float64, device="cuda")
    work = torch.zeros(3 * 3 * 5, dtype=torch.float64, device="cuda")
    ev = lambda X, r, n, K, Yp, w, wb, s: lib.gs_brs_eval(X, r, 3, 9, n, bank.Ju, K, Yp, w, wb, s, None)  # noqa: E731
    good = (C.ptr(bank.X), C.ptr(bank.r))
    assert ev(None, good[1], 7, 5, C.ptr(Y), C.ptr(work), work.numel() * 8, C.ptr(state)) == -1
    assert b"null bank" in lib.gs_last_error()
    assert ev(*good, 7, 5, C.ptr(Y), C.ptr(work), work.numel() * 8, None) == -1
    assert b"null state" in lib.gs_last_error()
    assert ev(*good, 7, 5, None, C.ptr(work), work.numel() * 8, C.ptr(state)) == -1
    assert b"null Y or workspace" in lib.gs_last_error()
    assert ev(*good, 7, 0, C.ptr(Y), C.ptr(work), work.numel() * 8, C.ptr(state)) == -1
    assert b"K >= 1" in lib.gs_last_error()
    assert ev(*good, 10, 5, C.ptr(Y), C.ptr(work), work.numel() * 8, C.ptr(state)) == -1
    assert b"[0, cap]" in lib.gs_last_error()
    assert ev(*good, 7, 5, C.ptr(Y), C.ptr(work), work.numel() * 8 - 8, C.ptr(state)) == -1
    assert b"workspace is smaller" in lib.gs_last_error()
    with pytest.raises(ValueError, match=r"Y must be \[K, Ju\]"):
        bank.evaluate(cs["tables"]["Y"][:, :5])
    torch.cuda.synchronize()
    assert not state.any() and torch.equal(bank.X, X0) and torch.equal(bank.r, r0)
    # a bank that cannot fit is refused with its size
    need = bank.nbytes(7 * 10 ** 8)                                     # 487 GB
    assert need > torch.cuda.mem_get_info()[0]
    with pytest.raises(RuntimeError, match=f"{need} bytes"):
        bank.reserve(7 * 10 ** 8)
    assert bank.capacity == 9
