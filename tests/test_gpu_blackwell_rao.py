"""GPU: the scale trace of the C_l draw (gs_cls_scale_trace), the streaming
Blackwell-Rao accumulator (gs_br_*, engine.BlackwellRaoState) and
BatchedRunner.run(blackwell_rao=, keep_scales=) with the class surface.

The device's logpdf is compared with tests/_blackwell_rao.py within, per
element, atol = 16 * 2^-52 * max(alpha |log beta|, beta / D, |lgamma alpha| +
(alpha + 1) |log D|): the terms whose rounding sets the error, 16 the headroom
for the device library's few-ulp log / exp / lgamma.  mass is the trapezoid
rule applied to exp(logpdf); its relative error is the absolute error of
logpdf, so it is compared at rtol 1e-10 with the restated rule applied to the
device's own logpdf (as tests/test_gpu_summary.py checks the summary's finish
on the device's own state)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _blackwell_rao as B  # noqa: E402
from tests import _mh_adapt as A  # noqa: E402
from tests._util import fiducial_dl, make_problem  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20261020
OPTS = {"points": 5, "span": (0.5, 2.0)}


def make_runner(model, kind, nchains, chain0=0, rng="native", seed=SEED):
    from gibbssampler_amd.samplers import BatchedRunner
    return BatchedRunner(kind=kind, lmax=model.L, nside=model.nside, nfields=model.nfields, nchains=nchains,
                         bl=model.bl, noise_var=model.noise_var, bins=model.bins, d_alm=model.d_alm,
                         blocks=model.blocks, proposal_variances=model.proposal_variances, rng=rng, seed=seed,
                         chain0=chain0, store_skymap=False)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return set(a) == set(b) and all(np.array_equal(a[s], b[s]) for s in a)


def check_logpdf(got, rows, alpha, grid, half, what):
    """got [nsb, G] (device) against the restated update + finish of rows [T, C, nsb]."""
    T, C, nsb = rows.shape
    st = B.update(B.State(C, nsb, grid.shape[1]), rows, alpha, grid, half)
    want, _ = B.finish(st.m, st.S, st.n, alpha, grid)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    bound = 16 * 2.0 ** -52 * B.term_bound(rows, alpha, grid, half)
    ok = ~np.isnan(want)
    ratio = float(np.max(np.abs(got - want)[ok] / bound[ok]))
    print(f"  {what}: max |device - numpy| / bound = {ratio:.3f} "
          f"(max error {np.max(np.abs(got - want)[ok]):.3e}, max bound {bound[ok].max():.3e})")
    assert ratio <= 1.0, what
    return want


def check_mass(mass, logpdf, grid, what):
    np.testing.assert_allclose(mass, B.trapezoid_mass(logpdf, grid), rtol=1e-10, atol=0, equal_nan=True,
                               err_msg=what)


# ---- 1. the scale trace ----------------------------------------------------------------------------
BINS_A = np.array([0, 1, 2, 3, 4, 6, 8, 9, 18, 52, 65])      # widths 1, 2, one bin of 9 l, one of 34 l
BINS_B = np.array([0, 1, 2, 4, 13, 47, 65])                   # another bin count: b >= nbins[sp] occurs


@pytest.mark.parametrize("F", [1, 2, 3])
def test_scale_trace(F):
    from gibbssampler_amd.engine import GibbsPlan, SPECTRA
    L, nch, cap = 64, 3, 4
    model, _ = make_problem(L, 32, F)
    spectra = SPECTRA[F]
    bins = {s: (BINS_B if s == "BB" else BINS_A) for s in spectra}
    fid = fiducial_dl(L, F)
    init = {s: np.array([fid[s][bins[s][i]:bins[s][i + 1]].mean() for i in range(len(bins[s]) - 1)]) for s in spectra}
    p = GibbsPlan(L, 32, F, nch, model.bl, model.noise_var, bins)
    d, dl = p.data_tensor(model.d_alm), p.dl_tensor(init)
    params = p.block_params(0, dl)
    ring = torch.full((cap, nch, p.nspec, p.maxbins), -7.0, dtype=torch.float64, device="cuda")
    p.cls_scale_trace(ring, cap)
    ell = np.arange(L + 1, dtype=np.float64)
    ig = [k for k, s in enumerate(spectra) if not (F == 3 and s != "BB")]
    np.random.seed(5)
    kept = {}
    for it in range(1, 7):                                     # 6 steps through 4 slots: the ring wraps
        _, stats = p.cr_sweep(d, params, seed=SEED, iteration=it, store=False)
        X = p.replay_invgamma()
        out = p.cls_draw(stats, variates=X, seed=SEED, iteration=it)
        sc = ring[(it - 1) % cap].clone()
        kept[it] = sc
        for k in ig:
            assert torch.equal(out[:, k], sc[:, k] * X[:, k]), (F, it, spectra[k])
        st, scn = stats.cpu().numpy(), sc.cpu().numpy()
        want = np.zeros_like(scn)
        for k, s in enumerate(spectra):
            b = bins[s]
            for i in range(2, len(b) - 1):
                sl = slice(b[i], b[i + 1])
                if k in ig:
                    chat = st[:, k, sl] / (2 * ell[sl] + 1)
                    want[:, k, i] = np.sum((2 * ell[sl] + 1) * ell[sl] * (ell[sl] + 1) * (chat / (4 * np.pi)), axis=1)
                else:
                    want[:, k, i] = np.sum(ell[sl] * (ell[sl] + 1) / (2 * np.pi) * st[:, k, sl], axis=1)
        np.testing.assert_allclose(scn, want, rtol=1e-13, atol=0, err_msg=f"F {F} it {it}")
        assert np.all(scn[:, :, :2] == 0) and all(np.all(scn[:, k, 2:len(bins[spectra[k]]) - 1] > 0) for k in ig)
        if "BB" in spectra and F > 1:
            assert np.all(scn[:, spectra.index("BB"), len(BINS_B) - 1:] == 0)
    torch.cuda.synchronize()
    for it in (3, 4, 5, 6):                                    # what the ring holds after the wrap
        assert torch.equal(ring[(it - 1) % cap], kept[it])
    # detached: the draw writes nothing more, and its output keeps its bits
    p.cls_scale_trace(None)
    ring.fill_(-7.0)
    again = p.cls_draw(stats, variates=X, seed=SEED, iteration=6)
    torch.cuda.synchronize()
    assert torch.equal(again, out) and bool((ring == -7.0).all())


# ---- 2. nothing else moves ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    return A.small_problem(3)


@pytest.mark.parametrize("kind", ["centered", "asis"])
def test_histories_do_not_move(kind, problem):
    model, init = problem
    T = 70                                                      # two full chunks and a tail
    states = []
    for gc in (32, 0):
        h0, a0 = make_runner(model, kind, 4).run(init, T, graph_chunk=gc)
        r = make_runner(model, kind, 4)
        h, a = r.run(init, T, graph_chunk=gc, blackwell_rao=OPTS, keep_scales=True)
        assert same(h0, h) and same(a0, a), (kind, gc)
        assert r._br.n == T and r.plan.scale_trace is None
        assert r.h_scales["BB"].shape == (T, 4, model.nbins("BB"))
        states.append((r._br.data.clone(), r.h_scales))
    assert torch.equal(states[0][0], states[1][0]) and same(states[0][1], states[1][1])


def test_cached_graph_without_ring_writes_nothing(problem):
    model, init = problem
    r = make_runner(model, "centered", 4)
    h0, _ = r.run(init, 8, graph_chunk=8)
    p = r.plan
    ring = torch.full((8, 4, p.nspec, p.maxbins), -7.0, dtype=torch.float64, device="cuda")
    p.cls_scale_trace(ring, 8)
    p.cls_scale_trace(None)
    ncached = len(r._run_graphs)
    h1, _ = r.run(init, 8, graph_chunk=8)                      # replays the graph captured without the ring
    torch.cuda.synchronize()
    assert len(r._run_graphs) == ncached and same(h0, h1) and bool((ring == -7.0).all())
    # with the ring the run captures graphs of its own and leaves the plain one alone
    h2, _ = r.run(init, 8, graph_chunk=8, blackwell_rao=OPTS)
    h3, _ = r.run(init, 8, graph_chunk=8)
    assert same(h0, h2) and same(h0, h3) and ("scales", 8) in r._run_graphs and 8 in r._run_graphs


# ---- 3. the accumulator on synthetic rings -----------------------------------------------------------
def synthetic(G):
    C, nspec, mb = 3, 4, 7
    rng = np.random.default_rng(SEED)
    n_b = rng.integers(5, 200, size=(nspec, mb)).astype(np.float64)
    alpha = 0.5 * n_b - 1.0
    alpha[0, 3] = 0.5 * (1024.0 ** 2 - 2.0 ** 2) - 1.0          # a whole-range bin: the exponent range
    alpha[:, :2] = np.nan
    alpha[3] = np.nan                                           # TE-like
    alpha[1, 4] = np.nan                                        # a NaN series between live neighbours
    centre = 10.0 ** rng.uniform(-2, 3, size=(nspec, mb))
    width = 1.0 / np.sqrt(np.where(np.isnan(alpha), 1.0, alpha))
    rows = centre * np.where(np.isnan(alpha), 1.0, alpha) * (1.0 + width * rng.normal(size=(9, C, nspec, mb)) * 0.7)
    rows = np.abs(rows) + 1e-3 * centre
    half = np.zeros((nspec, mb), dtype=bool)
    half[:2] = True
    rows = np.where(half, 2.0, 1.0) * rows
    span = np.geomspace(1.0, 2.0, G) / np.sqrt(2.0) if G > 1 else np.ones(1)
    grid = centre[..., None] * (1.0 + 3.0 * width[..., None] * (span - 1.0))
    return rows, alpha, grid, half


def feed(st, x, cuts, cap):
    ring = torch.zeros((cap,) + tuple(x.shape[1:]), dtype=torch.float64, device="cuda")
    it, row = 1, 0
    for k in cuts:
        for i in range(k):
            ring[(it + i - 1) % cap].copy_(x[row + i])
        st.update(ring, cap, it, k)
        it, row = it + k, row + k
    return st


@pytest.mark.parametrize("G", [1, 5, 64])
def test_accumulator_on_synthetic_rings(G):
    from gibbssampler_amd.engine import BlackwellRaoState
    rows, alpha, grid, half = synthetic(G)
    T, C, nspec, mb = rows.shape
    x = torch.from_numpy(rows).cuda()
    new = lambda: BlackwellRaoState(C, grid, alpha, half_mask=0b0011)
    a = feed(new(), x, (5, 4), 8)                               # the second launch wraps the ring
    b = feed(new(), x, (3, 5, 1), 8)
    torch.cuda.synchronize()
    assert torch.equal(a.data, b.data) and a.n == T and not a.bad().any()
    out = a.finish()
    lp, mass = out["logpdf"].cpu().numpy().reshape(-1, G), out["mass"].cpu().numpy().reshape(-1)
    flat = lambda v: v.reshape((-1,) + v.shape[2:])
    check_logpdf(lp, rows.reshape(T, C, -1), flat(alpha), flat(grid), flat(half), f"G {G}")
    check_mass(mass, lp, flat(grid), f"G {G}")
    dead = np.isnan(flat(alpha))
    assert np.all(np.isnan(lp[dead])) and np.all(np.isnan(mass[dead])) and np.all(np.isfinite(lp[~dead]))
    m, S = B.from_device(a.fields().cpu().numpy(), nspec * mb, G)
    assert not m[:, dead].any() and not S[:, dead].any() and np.all(S[:, ~dead] >= 1.0)
    # a skipped row (the sentinel): counted once, and only its own series differs
    bad = rows.copy()
    bad[4, 1, 2, 5] = 0.0
    c = feed(new(), torch.from_numpy(bad).cuda(), (5, 4), 8)
    want = np.zeros((C, nspec), dtype=np.int64)
    want[1, 2] = 1
    assert np.array_equal(c.bad().cpu().numpy(), want) and c.n == T
    diff = (c.fields() != a.fields()).any(dim=0).cpu().numpy().reshape(C, nspec, mb, G)
    only = np.zeros((C, nspec, mb, G), dtype=bool)
    only[1, 2, 5] = True
    assert np.array_equal(diff | only, only) and diff.any()
    a.reset()
    torch.cuda.synchronize()
    assert not a.data.any()


# ---- 4. end to end ---------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
def test_end_to_end(F):
    from gibbssampler_amd import gibbs
    from gibbssampler_amd.engine import br_shapes
    model, init = make_problem(32, 16, F)
    keys = ("EE", "BB") if F == 2 else ("TT", "EE", "BB")
    d = {k: model.d_alm[i] for i, k in enumerate(keys)}
    fwhm = max(0.5, 180.0 / model.L * 2)
    T, nch = 200, 4
    kw = dict(polarization=True, bins=model.bins, n_iter=T, all_sph=True, nchains=nch, seed=SEED,
              fields="EB" if F == 2 else "TEB", blackwell_rao={"points": 9, "span": (0.3, 3.0)})
    args = (d, model.noise_var[0], model.noise_var[-1], fwhm, model.nside, model.L, 12 * model.nside ** 2)
    on = gibbs.CenteredGibbs(*args, keep_scales=True, **kw)
    h = on.run(init)[0]
    post, hs = on.blackwell_rao_posterior, on.h_scales
    alpha, half_mask = br_shapes(F, model.bins)
    for k, s in enumerate(model.spectra):
        nb = model.nbins(s)
        assert hs[s].shape == (T, nch, nb) and h[s].shape == (T + 1, nch, nb)
        assert set(post[s]) >= {"grid", "logpdf", "mass", "alpha", "n"} and post[s]["n"] == T and post[s]["bad"] == 0
        assert np.array_equal(post[s]["alpha"], alpha[k, :nb], equal_nan=True)
        if F == 3 and s == "TE":
            assert np.all(np.isnan(post[s]["logpdf"])) and np.all(np.isnan(post[s]["mass"]))
            continue
        assert np.all(np.isnan(post[s]["logpdf"][:2])) and np.all(np.isfinite(post[s]["logpdf"][2:]))
        half = np.full(nb, bool((half_mask >> k) & 1))
        check_logpdf(post[s]["logpdf"], hs[s], alpha[k, :nb], post[s]["grid"], half, f"F {F} {s}")
        check_mass(post[s]["mass"], post[s]["logpdf"], post[s]["grid"], f"F {F} {s}")
        np.testing.assert_allclose(post[s]["grid"][2:, 0], 0.3 * np.asarray(init[s])[2:], rtol=1e-15)
    off = gibbs.CenteredGibbs(*args, keep_history=False, **kw)
    res = off.run(init)
    assert res[0] is None and off.h_scales is None
    p2 = off.blackwell_rao_posterior
    for s in model.spectra:
        for key in post[s]:
            assert np.array_equal(np.asarray(post[s][key]), np.asarray(p2[s][key]), equal_nan=True), (s, key)


# ---- 5. continuity -----------------------------------------------------------------------------------
def test_continuity(problem):
    model, init = problem
    whole = make_runner(model, "asis", 2)
    hw, _ = whole.run(init, 100, blackwell_rao=OPTS)
    a = make_runner(model, "asis", 2)
    a.run(init, 45, blackwell_rao=OPTS)
    st = a.state_dict()
    assert st["br_start"] == 0 and st["br_half_mask"] == 0b0011 and tuple(st["br_grid"].shape)[2] == 5
    b = make_runner(model, "asis", 2)
    hb, _ = b.run(None, 55, resume=st)
    assert same({s: v[45:] for s, v in hw.items()}, hb)
    assert b._br.n == 100 and torch.equal(whole._br.data, b._br.data)
    pw, pb = whole.blackwell_rao(), b.blackwell_rao()
    for s in model.spectra:
        for k in pw[s]:
            assert np.array_equal(np.asarray(pw[s][k]), np.asarray(pb[s][k]), equal_nan=True), (s, k)
    c = make_runner(model, "asis", 2)
    c.run(init, 100, graph_chunk=8, blackwell_rao=OPTS)
    assert torch.equal(whole._br.data, c._br.data)
    # start: the iterations up to it are not accumulated
    c.run(init, 30, blackwell_rao=dict(OPTS, start=11))
    assert c._br.n == 19 and c.br_start == 11
    # a state without the keys loads as "off"
    old = {k: v for k, v in st.items() if not k.startswith("br_")}
    e = make_runner(model, "asis", 2)
    e.run(init, 3, blackwell_rao=OPTS)
    he, _ = e.run(None, 55, resume=old)
    assert e._br is None and same(he, hb)
    with pytest.raises(RuntimeError, match="blackwell_rao"):
        e.blackwell_rao()


# ---- 6. chains across ranks --------------------------------------------------------------------------
def test_chains_across_ranks(problem):
    model, init = problem
    r4 = make_runner(model, "centered", 4)
    r4.run(init, 21, blackwell_rao=OPTS)
    lo = make_runner(model, "centered", 2)
    lo.run(init, 21, blackwell_rao=OPTS)
    hi = make_runner(model, "centered", 2, chain0=2)
    hi.run(init, 21, blackwell_rao=OPTS)
    assert torch.equal(torch.cat([lo._br.fields(), hi._br.fields()], dim=1), r4._br.fields())
    calls = []

    def gather(t, dim=0):
        calls.append(tuple(t.shape))
        return torch.cat([t, hi._br.fields()], dim=dim)

    got, want = lo.blackwell_rao(gather=gather), r4.blackwell_rao()
    assert len(calls) == 1
    for s in model.spectra:
        for k in want[s]:
            assert np.array_equal(np.asarray(got[s][k]), np.asarray(want[s][k]), equal_nan=True), (s, k)


# ---- 7. refusals ---------------------------------------------------------------------------------------
def test_refusals(problem):
    from gibbssampler_amd import gibbs, _capi as C
    from gibbssampler_amd.samplers import _capture
    model, init = A.small_problem(2)
    d = {"EE": model.d_alm[0], "BB": model.d_alm[1]}
    fwhm = max(0.5, 180.0 / model.L * 2)
    npix = 12 * model.nside ** 2
    args = (d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L, npix)
    kw = dict(polarization=True, bins=model.bins, n_iter=4, all_sph=True, blackwell_rao=OPTS)
    with pytest.raises(NotImplementedError, match="non-centered"):
        gibbs.NonCenteredGibbs(*args, model.proposal_variances, metropolis_blocks=model.blocks, **kw)
    with pytest.raises(NotImplementedError, match="masked"):
        gibbs.CenteredGibbs(*args, mask_path=np.ones(npix), **kw)
    with pytest.raises(NotImplementedError, match="TT-pixel"):
        gibbs.CenteredGibbs(np.zeros(npix), model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L, npix,
                            bins=np.arange(model.L + 2), n_iter=4,
                            blackwell_rao={"grid": np.ones((1, model.L + 1, 3)).cumsum(axis=2)})
    with pytest.raises(NotImplementedError, match="non-centered"):
        make_runner(model, "noncentered", 2).run(init, 4, blackwell_rao=OPTS)
    with pytest.raises(ValueError, match="keep_history=False needs summary="):
        make_runner(model, "centered", 2).run(init, 4, keep_history=False)
    # attach inside a capture: an error, and the plan keeps no ring
    r = make_runner(model, "centered", 2)
    p = r.plan
    ring = p.zeros(4, 2, p.nspec, p.maxbins)
    x = p.zeros(8)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _capture(g):
        x.add_(1.0)
        rc = p.lib.gs_cls_scale_trace(p._h, C.ptr(ring), 4, C.stream_ptr())
        msg = p.lib.gs_last_error()
    assert rc == -1 and b"captured" in msg
    h0, _ = make_runner(model, "centered", 2).run(init, 4)
    h1, _ = r.run(init, 4)
    torch.cuda.synchronize()
    assert same(h0, h1) and not ring.any()
