"""GPU: warm-up adaptation of the NC Metropolis proposal scales (gs_mh_adapt_*,
BatchedRunner.run(n_warmup=...)).

Shapes: tests._util.make_problem at L 40 / N_side 16 (tests/_mh_adapt.small_problem),
TT / EE / TE one whole-range block each, BB one block per bin; the "wide" F = 2
cases have BB blocks of several bins, the last one clipped by nbins, and two
Metropolis attempts per block.

Which case reaches which proposal-drawing site (every launch that calls
mh_propose_at reads the per-chain table through the chain stride):
  k_nc_prologue                       nc2 (graph), nc2-wide-eager: <= 4 chains draw in the prologue
  k_cr_sweep front workgroups         nc5 (raw-moment sweep), nc5-table (GS_NC_RAW=0),
                                      nc5-wide-map (stored map): > 4 chains defer the draws
  k_mh_propose                        asis2-eager, asis2-wide-eager (gs_step_asis -> gs_nc_mh);
                                      the gs_nc_mh side of test_finish_sites
  k_stats_to_nc front (ASIS ProPre)   asis5, asis2-wide (gs_step_asis_fused in the captured graph)
  k_stats_finish_pro                  test_finish_sites[table]: 5 chains, GS_NC_RAW=0, a sweep with
                                      replayed normals cannot take the deferred draws
  k_stats_finish_raw                  test_finish_sites[raw]: 5 chains, a raw sweep of another
                                      iteration leaves the deferred draws to the finish
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _mh_adapt as A  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20261020

# id: (F, kind, nchains, BB blocks, n_iter_metropolis, library options, stored map, graph_chunk)
CASES = {
    "nc2": (3, "noncentered", 2, "per_bin", 1, {}, False, 32),
    "nc5": (3, "noncentered", 5, "per_bin", 1, {}, False, 32),
    "nc5-table": (3, "noncentered", 5, "per_bin", 1, {"GS_NC_RAW": 0}, False, 32),
    "nc5-wide-map": (2, "noncentered", 5, "wide", 2, {}, True, 32),
    "nc2-wide-eager": (2, "noncentered", 2, "wide", 2, {}, False, 0),
    "asis2-eager": (3, "asis", 2, "per_bin", 1, {}, False, 0),
    "asis5": (3, "asis", 5, "per_bin", 1, {}, False, 32),
    "asis2-wide": (2, "asis", 2, "wide", 2, {}, False, 32),
    "asis2-wide-eager": (2, "asis", 2, "wide", 2, {}, False, 0),
}


def make_runner(model, kind, nchains, chain0=0, n_mh=1, store=False, seed=SEED):
    from gibbssampler_amd.samplers import BatchedRunner
    return BatchedRunner(kind=kind, lmax=model.L, nside=model.nside, nfields=model.nfields, nchains=nchains,
                         bl=model.bl, noise_var=model.noise_var, bins=model.bins, d_alm=model.d_alm,
                         blocks=model.blocks, proposal_variances=model.proposal_variances, rng="native", seed=seed,
                         chain0=chain0, n_iter_metropolis=n_mh, store_skymap=store)


def case(name, gsopt, var_scale=1.0):
    F, kind, nch, bb, n_mh, opts, store, gc = CASES[name]
    for k, v in opts.items():
        gsopt.setenv(k, v)
    model, init = A.small_problem(F, bb_blocks=bb, var_scale=var_scale)
    return model, init, make_runner(model, kind, nch, n_mh=n_mh, store=store), n_mh, gc


def flat(model, acc):
    """run()'s accept dict -> [T, nchains, nacc] in the device's flag order."""
    return np.concatenate([acc[s] for s in A.MH_ORDER[model.nfields]], axis=2)


def same(a, b):
    return all(np.array_equal(a[s], b[s]) for s in a) and set(a) == set(b)


def scales(r):
    lam, n = r.plan.mh_scale_get()
    return lam.cpu().numpy(), n.cpu().numpy(), r.plan.mh_proposal_sd().cpu().numpy()


def lam_tol(T, lam):
    # T sequential fp64 updates of a few ulp each
    return 8 * T * 2.0 ** -52 * max(1.0, float(np.max(np.abs(lam))))


# ---- 1. off is invisible -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["nc2", "nc5", "nc2-wide-eager", "asis2-eager", "asis5", "nc5-wide-map"])
def test_enabled_but_never_adapted_is_bit_identical(name, gsopt):
    """Stride 0 (shared table) == per-chain table at log-scale 0: histories and
    accept flags of 20 steps, graph and eager, NC and ASIS."""
    model, init, r0, n_mh, gc = case(name, gsopt)
    h0, a0 = r0.run(init, 20, graph_chunk=gc)
    r1 = make_runner(model, r0.kind, r0.plan.nchains, n_mh=n_mh, store=r0.s is not None)
    r1.plan.mh_adapt_enable()
    h1, a1 = r1.run(init, 20, graph_chunk=gc)
    assert same(h0, h1) and same(a0, a1)
    lam, n, sd = scales(r1)
    assert not lam.any() and not n.any() and r1.n_warmup == 0
    sd0 = r0.plan.mh_proposal_sd().cpu().numpy()
    assert np.array_equal(sd, sd0)
    assert flat(model, a0).sum() > 0


# ---- 2. the recursion --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_recursion_matches_numpy_on_the_device_flags(name, gsopt):
    """T = 200 warm-up steps from variances x 1e4: the numpy recursion fed the
    device's own accept flags gives n == T exactly, the log-scales within
    8 T 2^-52 max(1, max|lam|) and sd within 1e-14 relative of sd0 exp(lam)."""
    T = 200
    model, init, r, n_mh, gc = case(name, gsopt, var_scale=1e4)
    h, acc = r.run(init, T, n_warmup=T, graph_chunk=gc)
    lam, n, sd = scales(r)
    fl = flat(model, acc)
    assert fl.shape == (T, r.plan.nchains, r.plan.nacc) and r.n_warmup == T
    want_lam, want_n = A.recursion(fl, n_mh)
    err = float(np.max(np.abs(lam - want_lam)))
    print(f"{name}: max |lam| {np.max(np.abs(lam)):.3f}, lam range [{lam.min():.3f}, {lam.max():.3f}], "
          f"max |lam - numpy| {err:.3e} (bound {lam_tol(T, lam):.3e})")
    assert np.array_equal(n, want_n) and np.all(n == T)
    assert err <= lam_tol(T, lam)
    assert np.abs(lam).max() > 1.0                          # the scales moved
    for c in range(r.plan.nchains):
        want_sd = A.expand_sd(model, lam[c])
        for k, s in enumerate(r.plan.spectra):
            nb = model.nbins(s)
            np.testing.assert_allclose(sd[c, k, 2:nb], want_sd[s], rtol=1e-14, atol=0)
            assert not sd[c, k, :2].any() and not sd[c, k, nb:].any()
    # chains differ: the table is per chain
    assert not np.array_equal(lam[0], lam[1])


# ---- 3. oracle parity ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_chains():
    """The test-side oracle's adapted chains 0..4 (40 warm-up steps, analytic
    variances), computed once and shared."""
    model, init = A.small_problem(3)
    return model, init, [A.oracle_chain(model, init, SEED, c, 40, 40) for c in range(5)]


@pytest.mark.parametrize("nchains", [2, 5])
def test_adapted_chain_matches_oracle(nchains, oracle_chains):
    """40 adapted steps, device against the oracle chain running its own
    recursion (tolerances of test_gpu_longchain.py): accept flags exactly,
    D_l after steps 1, 20 and 40 within 1e-8 relative; the log-scales within
    the recursion's bound."""
    model, init, ref = oracle_chains
    r = make_runner(model, "noncentered", nchains)
    h, acc = r.run(init, 40, n_warmup=40)
    fl = flat(model, acc)
    lam, n, _ = scales(r)
    for c in range(nchains):
        rh, rf, rl, rn = ref[c]
        np.testing.assert_array_equal(fl[:, c], rf, err_msg=f"flags chain {c}")
        for s in model.spectra:
            for it in (1, 20, 40):
                np.testing.assert_allclose(h[s][it, c], rh[s][it], rtol=1e-8, atol=1e-300,
                                           err_msg=f"{s} chain {c} after step {it}")
        assert np.array_equal(n[c], rn)
        assert np.max(np.abs(lam[c] - rl)) <= lam_tol(40, rl)
    assert fl.sum() > 100 and np.abs(lam).max() > 0.5


# ---- 4. / 5. frozen means frozen; reproducible from the scale alone -------------------------
@pytest.mark.parametrize("name", ["nc2", "nc5", "asis5", "asis2-wide-eager"])
def test_frozen_scales_and_reproducible_from_scale(name, gsopt):
    nw, nf = 25, 15
    model, init, ra, n_mh, gc = case(name, gsopt, var_scale=1e4)
    mk = lambda: make_runner(model, ra.kind, ra.plan.nchains, n_mh=n_mh)  # noqa: E731
    ha, aa = ra.run(init, nw + nf, n_warmup=nw, graph_chunk=gc)
    la, na, sda = scales(ra)
    rb = mk()
    rb.run(init, nw, n_warmup=nw, graph_chunk=gc)
    lb, nb_, sdb = scales(rb)
    # after step n_warmup and after the last step: the same bits
    assert np.array_equal(la, lb) and np.array_equal(na, nb_) and np.array_equal(sda, sdb)
    assert np.all(na == nw) and np.abs(la).max() > 0.5
    # a second runner: the scales through scale_set, the chain state without them
    st = {k: v for k, v in rb.state_dict().items() if not k.startswith("mh_")}
    rc = mk()
    rc.plan.mh_adapt_enable()
    rc.plan.mh_scale_set(lb, nb_)
    assert np.array_equal(scales(rc)[2], sdb)                # the same expansion: bit-identical sd
    hc, ac = rc.run(None, nf, resume=st, graph_chunk=gc)
    assert rc.n_warmup == 0
    off = 0 if ra.kind == "asis" else 1                      # NC histories start with the restored row
    for s in ha:
        assert np.array_equal(hc[s][off:], ha[s][nw + off:]), s
    assert same({s: v[nw:] for s, v in aa.items()}, ac)
    assert np.array_equal(scales(rc)[0], la)


# ---- 6. checkpoint mid warm-up ------------------------------------------------------------------
@pytest.mark.parametrize("name,gc", [("nc2", 4), ("nc2", 0), ("nc5", 4), ("asis5", 4), ("asis2-eager", 0)])
def test_checkpoint_mid_warmup_resumes_bit_for_bit(name, gc, gsopt):
    """state_dict at step 7 of a 20-step warm-up, resumed on a fresh runner
    (graph_chunk 4: the resume lands mid-ring), equals the uninterrupted run."""
    model, init, ra, n_mh, _ = case(name, gsopt, var_scale=1e4)
    ha, aa = ra.run(init, 20, n_warmup=20, graph_chunk=gc)
    rb = make_runner(model, ra.kind, ra.plan.nchains, n_mh=n_mh)
    rb.run(init, 7, n_warmup=20, graph_chunk=gc)
    st = rb.state_dict()
    assert st["mh_n_warmup"] == 20 and int(st["mh_count"].min()) == 7
    rc = make_runner(model, ra.kind, ra.plan.nchains, n_mh=n_mh)
    hc, ac = rc.run(None, 13, resume=st, graph_chunk=gc)
    off = 0 if ra.kind == "asis" else 1
    for s in ha:
        assert np.array_equal(hc[s][off:], ha[s][7 + off:]), s
    assert same({s: v[7:] for s, v in aa.items()}, ac)
    la, na, sda = scales(ra)
    lc, nc_, sdc = scales(rc)
    assert np.array_equal(la, lc) and np.array_equal(na, nc_) and np.array_equal(sda, sdc)
    assert np.all(nc_ == 20) and rc.n_warmup == 20


# ---- 7. sharding invariance ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noncentered", "asis"])
def test_chain_offset_is_invisible(kind):
    """Chains 0-3 of one plan against two plans of 2 chains (chain0 0 and 2)."""
    from gibbssampler_amd.distributed import ShardContext
    model, init = A.small_problem(3, var_scale=1e4)
    r4 = make_runner(model, kind, 4)
    h4, a4 = r4.run(init, 30, n_warmup=20)
    l4 = scales(r4)[0]
    for c0 in (0, 2):
        r2 = make_runner(model, kind, 2, chain0=c0)
        h2, a2 = r2.run(init, 30, n_warmup=20)
        for s in h4:
            assert np.array_equal(h2[s], h4[s][:, c0:c0 + 2]), s
            assert np.array_equal(a2[s], a4[s][:, c0:c0 + 2]), s
        assert np.array_equal(scales(r2)[0], l4[c0:c0 + 2])
    tv = r4.tuned_proposal_variances()
    tg = r4.tuned_proposal_variances(gather=ShardContext(4, backend="gloo").gather)
    assert same(tv, tg)
    lay = r4.plan.mh_block_layout()
    want = A.expand_sd(model, l4.mean(axis=0))
    for s, _, _ in lay:
        np.testing.assert_allclose(tv[s], want[s] ** 2, rtol=1e-13)


# ---- the two statistics-finish sites ------------------------------------------------------------------
@pytest.mark.parametrize("site", ["table", "raw"])
def test_finish_sites(site, gsopt):
    """Deferred draws taken by the statistics finish (k_stats_finish_pro /
    k_stats_finish_raw) read the per-chain table: with distinct scales per
    chain and block the staged step equals gs_nc_mh (k_mh_propose) on the same
    statistics, bit for bit, and differs from the step at the plan's own scales."""
    if site == "table":
        gsopt.setenv("GS_NC_RAW", 0)
    model, init = A.small_problem(3)
    r = make_runner(model, "noncentered", 5)
    p = r.plan
    r.init(init)
    rng = np.random.RandomState(5)
    out = {}
    for tag in ("zero", "scaled"):
        if tag == "scaled":
            p.mh_adapt_enable()
            p.mh_scale_set(rng.uniform(-3.0, 0.5, size=(5, p.nblocks_mh)))
        dl = r.dl.clone()
        acc = p.zeros(5, p.nacc, dtype=torch.int32)
        p.nc_prologue(dl, seed=SEED, iteration=3)
        if site == "table":
            z = torch.from_numpy(np.random.RandomState(1).normal(size=(5, 3, p.NR))).to(p.device)
            p.nc_sweep(r.d, dl, None, z=z, seed=SEED, iteration=3)
        else:
            p.nc_sweep(r.d, dl, None, seed=SEED, iteration=4)
        st = p.nc_stats()
        p.nc_decide(dl, seed=SEED, iteration=3, accept=acc)
        dl2 = r.dl.clone()
        acc2 = p.nc_mh(st, dl2, seed=SEED, iteration=3)
        torch.cuda.synchronize()
        assert torch.equal(dl, dl2) and torch.equal(acc, acc2), tag
        out[tag] = (dl.cpu().numpy(), acc.cpu().numpy())
    assert not np.array_equal(out["zero"][0], out["scaled"][0])
    assert out["scaled"][1].sum() > 0


# ---- 8. it tunes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e2, 1e-8])
def test_it_tunes(scale):
    """F = 3, 5 chains, the analytic variances x 1e2 and x 1e-8, n_warmup = 1000,
    then 300 frozen steps: the acceptance of every block, pooled over the
    chains and the frozen steps, lies in [a*/2.5, 2 a*] = [0.1, 0.5]; the same
    start without warm-up accepts less than a*/10 (x 1e2) or more than 0.9
    (x 1e-8) on the whole-range blocks TT, EE and TE.

    The issue's first choice (x 1e4 / x 1e-6, 300 warm-up steps) does not meet
    the conditions in the test-side oracle chain (tests/_mh_adapt.oracle_chain,
    seed 77, chains 0-4, on the CPU): 300 all-reject steps lower the log-scale
    by at most 0.25 * sum n^-0.6 ~ 6.1, and x 1e4 leaves TT and TE, which need
    about -9, at acceptance 0; untuned x 1e-6 accepts only 0.75 on TT.  So the
    multipliers and the warm-up length were changed, not the band.  The oracle
    with the settings used here:
        x 1e2,  tuned:   EE 0.222  TT 0.207  TE 0.238  BB 0.211 .. 0.291
        x 1e2,  untuned: EE 0      TT 0      TE 0      (BB 0.033 .. 0.775)
        x 1e-8, tuned:   EE 0.246  TT 0.251  TE 0.263  BB 0.214 .. 0.289
        x 1e-8, untuned: EE 0.999  TT 0.927  TE 0.992  (BB 0.990 .. 1)"""
    nw, nf, target = 1000, 300, 0.25
    model, init = A.small_problem(3, var_scale=scale)
    lay = A.block_layout(model)
    r = make_runner(model, "noncentered", 5, seed=77)
    _, acc = r.run(init, nw + nf, n_warmup=nw, target_accept=target)
    pooled = flat(model, acc)[nw:].mean(axis=(0, 1))
    r0 = make_runner(model, "noncentered", 5, seed=77)
    _, acc0 = r0.run(init, nw + nf)
    pooled0 = flat(model, acc0)[nw:].mean(axis=(0, 1))
    for s, off, nb in lay:
        print(f"x{scale:g} {s}: tuned {pooled[off:off + nb].min():.3f} .. {pooled[off:off + nb].max():.3f}, "
              f"untuned {pooled0[off:off + nb].min():.3f} .. {pooled0[off:off + nb].max():.3f}")
    assert pooled.min() >= target / 2.5 and pooled.max() <= 2 * target
    for s, off, nb in lay:
        if nb == 1:                                           # the whole-range blocks
            assert pooled0[off] < target / 10 if scale > 1 else pooled0[off] > 0.9, s


# ---- 9. class surface ------------------------------------------------------------------------------
def test_class_surface():
    from gibbssampler_amd import gibbs
    model, init = A.small_problem(2)
    d = {"EE": model.d_alm[0], "BB": model.d_alm[1]}
    fwhm = max(0.5, 180.0 / model.L * 2)
    kw = dict(metropolis_blocks=model.blocks, polarization=True, bins=model.bins, n_iter=80, all_sph=True,
              nchains=3, seed=SEED)
    nc = gibbs.NonCenteredGibbs(d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L,
                                12 * model.nside ** 2, {s: v * 1e4 for s, v in model.proposal_variances.items()},
                                n_warmup=50, **kw)
    h, acc = nc.run(init)[:2]
    for s in model.spectra:
        assert h[s].shape == (81, 3, model.nbins(s))
    tv = nc.tuned_proposal_variances
    for s in model.spectra:
        assert tv[s].shape == (model.nbins(s) - 2,) and np.all(tv[s] > 0) and np.all(np.isfinite(tv[s]))
        assert np.all(tv[s] < 1e4 * model.proposal_variances[s])
    mab = nc.mean_accept_by_block
    for s in model.spectra:
        assert mab[s].shape == (len(model.blocks[s]) - 1,)
        np.testing.assert_allclose(mab[s], acc[s][50:].mean(axis=(0, 1)))
    # the preliminary -> production loop: a new sampler built with the tuned variances runs
    prod = gibbs.NonCenteredGibbs(d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L,
                                  12 * model.nside ** 2, tv, **dict(kw, n_iter=10))
    h2, acc2 = prod.run({s: h[s][-1, 0] for s in model.spectra})[:2]
    assert h2["EE"].shape == (11, 3, model.nbins("EE")) and prod.n_warmup == 0
    assert sum(int(v.sum()) for v in acc2.values()) > 0
    asis = gibbs.ASIS(d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L, 12 * model.nside ** 2,
                      model.proposal_variances, n_warmup=10, **dict(kw, n_iter=20))
    ha = asis.run(init)[0]
    assert ha["BB"].shape == (20, 3, model.nbins("BB")) and asis._runner.n_warmup == 10
    # masked runs use the pixel-domain MH: no adaptation there
    mask = np.ones(12 * model.nside ** 2)
    with pytest.raises(NotImplementedError, match="pixel-domain"):
        gibbs.NonCenteredGibbs(d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L,
                               12 * model.nside ** 2, model.proposal_variances, mask_path=mask, n_warmup=5,
                               **kw)
    with pytest.raises(ValueError, match="native"):
        gibbs.NonCenteredGibbs(d, model.noise_var[0], model.noise_var[0], fwhm, model.nside, model.L,
                               12 * model.nside ** 2, model.proposal_variances, n_warmup=5, **dict(kw, rng="replay"))
