"""GPU: the streaming Blackwell-Rao likelihood (gs_brl_*,
engine.BlackwellRaoLikelihood) and BatchedRunner.run(br_likelihood=) with the
class surface.

The device's loglike, chain_loglike and neff are compared with
tests/_br_likelihood.py within |delta| <= (Ju + 16) 2^-52 T_k, T_k the largest
sum over a row's used columns of |coef log arg| + x |Y_k| plus |cst_k|
(term_bound): the recursive-summation bound of the Ju fused terms, plus the
headroom of 16 the marginal test (tests/test_gpu_blackwell_rao.py) grants the
device library's log / exp / lgamma.  The kernel stages the used columns in
chunks of JC = 16 (gs_brl.hip) and owns TK = 128 models per workgroup: the
unbinned case has Ju = 252 = 15 chunks + 12, the K = 134 case a partial tile.
Largest |device - numpy| / bound seen on an MI355X: see DESIGN.md 'Streaming
Blackwell-Rao likelihood'."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_likelihood as R  # noqa: E402
from tests import _mh_adapt as A  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20261021
JC, TK = 16, 128
BINS_A = np.array([0, 1, 2, 3, 4, 6, 8, 9, 18, 52, 65])
BINS_B = np.array([0, 1, 2, 4, 13, 47, 65])
BR_OPTS = {"points": 5, "span": (0.5, 2.0)}


def bins_of(F, unbinned=False):
    from gibbssampler_amd.engine import SPECTRA
    if unbinned:
        return {s: np.arange(0, 66) for s in SPECTRA[F]}
    return {s: (BINS_B if s == "BB" and F > 1 else BINS_A) for s in SPECTRA[F]}


def case(F, K, unbinned=False, one=False, T=7, C=3, seed=SEED):
    """(rows [T, C, nspec, maxbins] with NaN off the used set, tables, maxbins)."""
    from gibbssampler_amd.engine import br_likelihood_mask, br_likelihood_tables
    bins = bins_of(F, unbinned)
    mask = None
    if one:                                                     # Ju = 1: one inverse-Gamma bin
        mask = np.zeros_like(br_likelihood_mask(F, bins))
        mask[-2 if F == 3 else -1, 3] = True
    rows, theory, mask = R.synthetic(F, bins, K, T, C, seed, mask)
    return rows, br_likelihood_tables(F, bins, theory, mask), mask.shape[1]


def new_state(rows, tables, maxbins, nchains=None):
    from gibbssampler_amd.engine import BlackwellRaoLikelihood
    return BlackwellRaoLikelihood(rows.shape[1] if nchains is None else nchains, rows.shape[2], maxbins, tables)


def feed(st, rows, cuts, cap=4):
    """rows [T, C, nspec, maxbins] through a ring of cap slots in launches of `cuts` rows."""
    x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    ring = torch.full((cap,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    it, row = 1, 0
    for k in cuts:
        for i in range(k):
            ring[(it + i - 1) % cap].copy_(x[row + i])
        st.update(ring, cap, it, k)
        it, row = it + k, row + k
    torch.cuda.synchronize()
    return st


def check(st, rows, tables, maxbins, what, out=None):
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    ref = R.update(R.State(C, tables["Y"].shape[0]), flat, tables, maxbins)
    want = R.finish(ref.m, ref.S, ref.Q, ref.n, tables["cst"])
    out = st.finish() if out is None else out
    assert out["n"] == ref.n == T and np.array_equal(st.bad().cpu().numpy(), ref.bad), what
    Ju = len(tables["cols"])
    bound = (Ju + 16) * 2.0 ** -52 * R.term_bound(flat, tables, maxbins)
    worst = 0.0
    for name, w, b in zip(("loglike", "chain_loglike", "neff"), want, (bound, bound[None, :], bound)):
        got = out[name].cpu().numpy()
        assert got.shape == w.shape and np.array_equal(np.isnan(got), np.isnan(w)), (what, name)
        ok = ~np.isnan(w)
        ratio = float(np.max((np.abs(got - w) / np.broadcast_to(b, w.shape))[ok])) if ok.any() else 0.0
        print(f"  {what} {name}: max |device - numpy| / bound = {ratio:.4f} (Ju {Ju}, max bound {bound.max():.3e})")
        worst = max(worst, ratio)
    assert worst <= 1.0, what
    ne = out["neff"].cpu().numpy()
    good = T * C - int(ref.bad.sum())
    assert np.all((ne >= 1.0) & (ne <= good * (1 + 1e-12))), what
    return out


# ---- 1. synthetic rings ------------------------------------------------------------------------------
@pytest.mark.parametrize("F,K,unbinned,one", [(3, 5, False, False), (3, TK + 6, False, False), (3, 5, False, True),
                                              (3, 5, True, False), (1, 5, False, False), (2, 5, False, False),
                                              (2, 3, False, True)])
def test_synthetic_ring(F, K, unbinned, one):
    rows, tables, maxbins = case(F, K, unbinned, one)
    Ju = len(tables["cols"])
    if one:
        assert Ju == 1
    if unbinned:
        assert Ju == 252 and Ju // JC >= 2 and Ju % JC != 0
    if not one and not unbinned and F == 3:
        assert maxbins == 10 and Ju == 8 * 3 + 4 and np.isnan(rows[..., 2, 6:]).all() and np.isnan(rows[..., :2]).all()
    st = feed(new_state(rows, tables, maxbins), rows, (3, 4))           # 7 rows through 4 slots: the ring wraps
    check(st, rows, tables, maxbins, f"F {F} K {K} Ju {Ju}")
    st.reset()
    torch.cuda.synchronize()
    assert not st.data.any()


# ---- 2. bad rows ---------------------------------------------------------------------------------------
def test_bad_rows():
    rows, tables, maxbins = case(3, 5)
    bad = rows.copy()
    bad[2, 1, 2, 3] = 0.0                                               # beta = 0 (BB) for chain 1
    bad[5, 2, 3, 6] = 2.0 * np.sqrt(bad[5, 2, 0, 6] * bad[5, 2, 1, 6])  # c^2 = 4 a dd for chain 2
    st = feed(new_state(bad, tables, maxbins), bad, (3, 4))
    assert np.array_equal(st.bad().cpu().numpy(), [0, 1, 1]) and st.n == 7
    check(st, bad, tables, maxbins, "bad rows")
    # each is skipped for its chain only: the other chains keep the clean run's bits
    clean = feed(new_state(rows, tables, maxbins), rows, (3, 4))
    assert torch.equal(st.fields()[:, 0], clean.fields()[:, 0])
    # and a chain with a skipped row holds what its other six rows alone give
    for chain, row in ((1, 2), (2, 5)):
        six = np.delete(rows[:, chain:chain + 1], row, axis=0)
        alone = feed(new_state(six, tables, maxbins), six, (3, 3))
        assert torch.equal(alone.fields()[:, 0], st.fields()[:, chain]) and alone.n == 6, chain
    # a value in an unused column changes nothing (the synthetic rows hold NaN there already)
    other = rows.copy()
    other[:, :, 2, 7:] = 3.0
    other[:, :, :, :2] = -1.0
    o = feed(new_state(other, tables, maxbins), other, (3, 4))
    assert torch.equal(o.data, clean.data)


# ---- 3. bit equality -----------------------------------------------------------------------------------
@pytest.mark.parametrize("unbinned", [False, True])
def test_bit_equality(unbinned):
    rows, tables, maxbins = case(3, 5, unbinned)
    ref = feed(new_state(rows, tables, maxbins), rows, (7,), cap=8)
    # (3, 4) in 4 slots: the second launch starts in slot 3 and wraps; (4, 3): a cut at the wrap
    for cuts, cap in (((3, 4), 8), ((1,) * 7, 8), ((3, 4), 4), ((4, 3), 4), ((1,) * 7, 1)):
        got = feed(new_state(rows, tables, maxbins), rows, cuts, cap)
        assert torch.equal(got.data, ref.data), (cuts, cap)
    # chain 2 alone is chain 2 of the three
    solo = feed(new_state(rows[:, 2:], tables, maxbins), rows[:, 2:], (3, 4))
    assert torch.equal(solo.fields()[:, 0], ref.fields()[:, 2])
    # model 4 of K = 5 is the same model run as K = 1
    t1 = dict(tables, Y=tables["Y"][4:5].copy(), cst=tables["cst"][4:5].copy())
    one = feed(new_state(rows, t1, maxbins), rows, (3, 4))
    assert torch.equal(one.fields()[:, :, 0], ref.fields()[:, :, 4])
    a, b = one.finish(), ref.finish()
    assert torch.equal(a["loglike"][0], b["loglike"][4]) and torch.equal(a["chain_loglike"][:, 0], b["chain_loglike"][:, 4])


# ---- 4. finish -------------------------------------------------------------------------------------------
def test_finish_gather_and_empty():
    rows, tables, maxbins = case(3, 5, C=4)
    whole = feed(new_state(rows, tables, maxbins), rows, (3, 4))
    lo = feed(new_state(rows[:, :2], tables, maxbins), rows[:, :2], (3, 4))
    hi = feed(new_state(rows[:, 2:], tables, maxbins), rows[:, 2:], (3, 4))
    assert torch.equal(torch.cat([lo.fields(), hi.fields()], dim=1), whole.fields())
    calls = []

    def gather(t, dim=0):
        calls.append(tuple(t.shape))
        return torch.cat([t, hi.fields()], dim=dim)

    got, want = lo.finish(gather), whole.finish()
    assert calls == [(3, 2, 5)] and got["n"] == want["n"] == 7
    for k in ("loglike", "chain_loglike", "neff"):
        assert torch.equal(got[k], want[k]), k
    empty = new_state(rows, tables, maxbins).finish()
    assert empty["n"] == 0 and all(bool(torch.isnan(empty[k]).all()) for k in ("loglike", "chain_loglike", "neff"))


def test_argument_checks():
    from gibbssampler_amd import _capi as C
    rows, tables, maxbins = case(3, 5)
    st = new_state(rows, tables, maxbins)
    ring = torch.zeros(4, 3, 4, maxbins, dtype=torch.float64, device="cuda")
    with pytest.raises(C.GibbsHipError, match="nsteps <= capacity"):
        st.update(ring, 4, 1, 5)
    with pytest.raises(ValueError, match="smaller than capacity"):
        st.update(ring, 5, 1, 1)
    lib = st.lib
    assert lib.gs_brl_update(None, 3, 4, maxbins, 5, st.Ju, None, None, None, None, None, 4, 1, 1, None) == -1
    assert b"null state" in lib.gs_last_error()
    assert lib.gs_brl_update(C.ptr(st.data), 3, 4, maxbins, 0, st.Ju, None, None, None, None, None, 4, 1, 1, None) == -1
    assert b"K >= 1" in lib.gs_last_error()
    assert lib.gs_brl_update(C.ptr(st.data), 3, 4, maxbins, 5, 0, None, None, None, None, None, 4, 1, 1, None) == -1
    assert b"Ju" in lib.gs_last_error()
    assert lib.gs_brl_update(C.ptr(st.data), 3, 4, maxbins, 5, st.Ju, None, None, None, None, None, 4, 1, 1, None) == -1
    assert b"null table" in lib.gs_last_error()
    with pytest.raises(ValueError, match="cols must ascend"):
        new_state(rows, dict(tables, cols=tables["cols"][::-1].copy()), maxbins)
    with pytest.raises(ValueError, match="cols must ascend"):
        new_state(rows, dict(tables, cols=tables["cols"] + 4 * maxbins), maxbins)
    torch.cuda.synchronize()
    assert not st.data.any()


# ---- 5. the surface ----------------------------------------------------------------------------------------
def make_runner(model, kind, nchains, chain0=0):
    from gibbssampler_amd.samplers import BatchedRunner
    return BatchedRunner(kind=kind, lmax=model.L, nside=model.nside, nfields=model.nfields, nchains=nchains,
                         bl=model.bl, noise_var=model.noise_var, bins=model.bins, d_alm=model.d_alm,
                         blocks=model.blocks, proposal_variances=model.proposal_variances, rng="native", seed=SEED,
                         chain0=chain0, store_skymap=False)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return set(a) == set(b) and all(np.array_equal(a[s], b[s]) for s in a)


@pytest.fixture(scope="module")
def problem():
    model, init = A.small_problem(3)
    fac = (0.5, 1.0, 2.0, 1.0)
    theory = {s: np.stack([f * np.asarray(init[s], dtype=np.float64) for f in fac]) for s in model.spectra}
    theory["TE"][3] *= -1.0
    return model, init, {"theory": theory, "lrange": (2, 12)}


T = 70


@pytest.fixture(scope="module")
def plain(problem):
    model, init, _ = problem
    return {kind: make_runner(model, kind, 4).run(init, T) for kind in ("centered", "asis")}


@pytest.mark.parametrize("kind", ["centered", "asis"])
def test_surface(kind, problem, plain):
    from gibbssampler_amd.engine import BlackwellRaoLikelihood
    model, init, opts = problem
    h0, a0 = plain[kind]
    states = []
    for gc in (32, 0):
        r = make_runner(model, kind, 4)
        h, a = r.run(init, T, graph_chunk=gc, br_likelihood=opts, keep_scales=True)
        assert same(h0, h) and same(a0, a), (kind, gc)
        assert r._brl.n == T and r.plan.scale_trace is None and r._brl.K == 4
        states.append(r._brl.data.clone())
    assert torch.equal(states[0], states[1])
    # the restatement on the kept scales
    p = r.plan
    hs = np.full((T, 4, p.nspec, p.maxbins), np.nan)
    for k, s in enumerate(model.spectra):
        hs[:, :, k, :model.nbins(s)] = r.h_scales[s]
    tables = {k: v.numpy() for k, v in r._brl.tables().items()}
    assert len(tables["cols"]) == 11 * 3 + int(np.sum((model.bins["BB"][2:-1] >= 2) & (model.bins["BB"][3:] - 1 <= 12)))
    res = r.br_likelihood()
    out = {k: torch.from_numpy(np.asarray(res[k])) for k in ("loglike", "chain_loglike", "neff")}
    check(r._brl, hs, tables, p.maxbins, f"surface {kind}", dict(out, n=res["n"]))
    assert res["n"] == T and np.array_equal(res["bad"], np.zeros(4)) and res["loglike"].shape == (4,)
    assert res["chain_loglike"].shape == (4, 4) and np.all(np.isfinite(res["loglike"]))
    # together with the marginal posteriors: neither moves the other
    alone = make_runner(model, kind, 4)
    alone.run(init, T, blackwell_rao=BR_OPTS)
    both = make_runner(model, kind, 4)
    hb, _ = both.run(init, T, blackwell_rao=BR_OPTS, br_likelihood=opts)
    assert same(h0, hb) and torch.equal(alone._br.data, both._br.data) and torch.equal(both._brl.data, states[0])
    # 40 + 30 through a state_dict and a new runner
    a1 = make_runner(model, kind, 4)
    a1.run(init, 40, br_likelihood=opts)
    st = a1.state_dict()
    assert st["brl_start"] == 0 and tuple(st["brl_Y"].shape) == (4, len(tables["cols"]))
    b1 = make_runner(model, kind, 4)
    b1.run(None, 30, resume=st)
    assert b1._brl.n == T and torch.equal(b1._brl.data, states[0])
    # a state without the keys is "off"
    b1.run(None, 3, resume={k: v for k, v in st.items() if not k.startswith("brl_")})
    assert b1._brl is None
    with pytest.raises(RuntimeError, match="br_likelihood"):
        b1.br_likelihood()
    # no history; start
    c = make_runner(model, kind, 4)
    assert c.run(init, T, br_likelihood=opts, keep_history=False) == (None, None)
    assert torch.equal(c._brl.data, states[0])
    c.run(init, T, br_likelihood=dict(opts, start=10))
    assert c._brl.n == 60 and c.brl_start == 10 and c.plan.scale_trace is None
    assert isinstance(c._brl, BlackwellRaoLikelihood)


def test_refusals_and_class_surface(problem):
    from gibbssampler_amd import gibbs
    model, init, opts = problem
    with pytest.raises(NotImplementedError, match="non-centered"):
        make_runner(model, "noncentered", 2).run(init, 4, br_likelihood=opts)
    d = {k: model.d_alm[i] for i, k in enumerate(("TT", "EE", "BB"))}
    fwhm = max(0.5, 180.0 / model.L * 2)
    npix = 12 * model.nside ** 2
    args = (d, model.noise_var[0], model.noise_var[-1], fwhm, model.nside, model.L, npix)
    kw = dict(polarization=True, bins=model.bins, n_iter=20, all_sph=True, nchains=2, seed=SEED, fields="TEB",
              br_likelihood=opts)
    with pytest.raises(NotImplementedError, match="non-centered"):
        gibbs.NonCenteredGibbs(*args, model.proposal_variances, metropolis_blocks=model.blocks, **kw)
    with pytest.raises(NotImplementedError, match="masked"):
        gibbs.CenteredGibbs(*args, mask_path=np.ones(npix), **kw)
    with pytest.raises(ValueError, match="unknown options"):
        gibbs.CenteredGibbs(*args, **dict(kw, br_likelihood=dict(opts, points=3)))
    g = gibbs.CenteredGibbs(*args, **kw)
    with pytest.raises(RuntimeError, match="nothing has run"):
        g.blackwell_rao_likelihood
    g.run(init)
    got = g.blackwell_rao_likelihood
    want = g._runner.br_likelihood()
    assert got["n"] == 20 and got["loglike"].shape == (4,) and np.all(np.isfinite(got["loglike"]))
    assert got["n"] == 20 and set(got) == {"loglike", "chain_loglike", "neff", "n", "bad"}
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    from gibbssampler_amd import io as gio
    rec = gio.run_record({}, None, None, model.bins, model.blocks, model.proposal_variances, 0.0, 0.0,
                         br_likelihood=got)
    assert np.array_equal(rec["br_likelihood"]["loglike"], got["loglike"])
