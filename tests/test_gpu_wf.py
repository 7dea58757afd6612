"""Rao-Blackwellised posterior sky map of the full-sky samplers (gs_wf.hip,
engine.WienerPosterior, BatchedRunner.run(wiener_posterior=), the classes'
posterior_wiener).

Every device result is held to the first-order rounding bounds of DESIGN.md
'Rao-Blackwellised posterior sky map' (tests/_wf_ref.py: they depend on k, C,
the series' magnitudes and the operator's condition only) against a longdouble
restatement computed directly from the stacked D_l samples.  Each test prints
its largest observed / bound ratio."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _wf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = ("alm_mean", "alm_var", "chain_alm_mean", "alm_rhat", "power_of_mean", "mean_power", "op_mean")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def make(P, C):
    from gibbssampler_amd.engine import WienerPosterior
    wp = WienerPosterior(P["F"], P["L"], C, P["bl"], P["bins"], P["kappa"], maxbins=P["maxbins"])
    wp.data_moments(dev(P["d"]))
    return wp


def feed(wp, stack, cuts=None, capacity=None, first=1):
    """rows stack [k, C, nspec, maxbins] as iterations first, first + 1, ...
    through a ring of `capacity` rows, `cuts` rows per launch"""
    k = stack.shape[0]
    cap = k if capacity is None else capacity
    cuts = min(k, cap) if cuts is None else cuts
    ring = torch.zeros((cap,) + stack.shape[1:], dtype=torch.float64, device="cuda")
    done = 0
    while done < k:
        n = min(cuts, k - done)
        for i in range(n):
            ring[(first + done + i - 1) % cap].copy_(dev(stack[done + i]))
        wp.update(ring, cap, first + done, n)
        done += n
    return wp


def results(wp, d, gather=None):
    out = wp.finish(d, gather)
    out.update(wp.power(gather))
    return out


def check_all(tag, got, P, stack):
    ref = R.posterior(P["F"], P["L"], P["bl"], P["kappa"], P["bins"], stack, P["d"])
    b = R.bounds(P["F"], P["L"], ref, P["d"])
    ratios = {}
    for key in OUTPUTS:
        g = host(got[key])
        print(f"{tag} {key}: max |got - ref| {np.nanmax(np.abs(g - np.asarray(ref[key], dtype=float).reshape(g.shape)), initial=0):.3g}")
        want = ref[key]
        if key == "alm_rhat":
            g, want, left_out = R.rhat_mask(g, want, b[key])
            print(f"{tag} alm_rhat: {left_out} elements with an unresolved W left out")
        ratios[key] = R.check(f"{tag} {key}", g, want, b[key])
    print(f"{tag}: observed / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return ratios


# ---- 1. engine against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("L", [5, 16, 70])
@pytest.mark.parametrize("F", [1, 2, 3])
def test_engine_against_restatement(F, L, C):
    worst = {}
    for k in (1, 2, 5):
        P = R.synthetic(F, L, k, C, seed=1000 * F + 10 * L + C + 100 * k)
        wp = feed(make(P, C), P["stack"])
        assert wp.n == k
        got = results(wp, dev(P["d"]))
        assert got["n"] == k
        for key, v in check_all(f"F={F} L={L} C={C} k={k}", got, P, P["stack"]).items():
            worst[key] = max(worst.get(key, 0.0), v)
        var, rhat = host(got["alm_var"]), host(got["alm_rhat"])
        assert np.all(np.isnan(var)) == (C * k < 2) and np.all(np.isfinite(var)) == (C * k >= 2)
        if C == 1 or k < 2:
            assert np.all(np.isnan(rhat))
        else:
            # l = L is unbinned in every spectrum: the same operator in every sample, W == 0 exactly
            assert np.all(np.isnan(rhat[:, R.slot_ell(L) == L])) and np.any(np.isfinite(rhat))
        assert np.all(host(got["mean_power"])[:F] >= 0)
    print(f"F={F} L={L} C={C}: largest observed / bound ratios {worst}")


# ---- 2. one iteration against the existing kernels ----------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3])
def test_one_iteration_against_block_params_and_sweep(F):
    """alm_mean after one row = the CR sweep's s = M d + L z with z = 0 on the
    operator table of gs_block_params(mode 0); alm_var = (L L^T)_ff of that
    table.  Two chains fed the same row, so that the variance exists (C k = 2)
    and its between-chain part is exactly 0."""
    from gibbssampler_amd.engine import GibbsPlan
    L, N = 16, 8
    P = R.synthetic(F, L, 1, 1, seed=77, nside=N)
    stack = np.repeat(P["stack"], 2, axis=1)
    plan = GibbsPlan(L, N, F, 2, P["bl"], P["noise_var"], P["bins"])
    assert plan.maxbins == P["maxbins"]
    dl = dev(stack[0])
    params = plan.block_params(0, dl)
    d = plan.data_tensor(P["d"])
    s, _ = plan.cr_sweep(d, params, z=torch.zeros(2, F, (L + 1) ** 2, dtype=torch.float64, device="cuda"))
    from gibbssampler_amd.engine import WienerPosterior
    wp = WienerPosterior.from_plan(plan)
    wp.data_moments(d)
    wp.update(dl[None], 1, 1, 1)
    got = wp.finish(d)
    ref = R.posterior(F, L, P["bl"], P["kappa"], P["bins"], stack, P["d"])
    b = R.bounds(F, L, ref, P["d"])
    assert torch.equal(s[0], s[1])
    r1 = R.check("alm_mean vs sweep", host(got["alm_mean"]), host(s[0]), b["alm_mean"])
    pr = host(params)[0]                                    # [L+1, NPARAM]
    if F == 3:
        llt = np.stack([pr[:, 5] ** 2, pr[:, 6] ** 2 + pr[:, 7] ** 2, pr[:, 8] ** 2])
    else:
        llt = np.stack([pr[:, F + f] ** 2 for f in range(F)])
    r2 = R.check("alm_var vs L L^T", host(got["alm_var"]), llt[:, R.slot_ell(L)], b["alm_var"])
    print(f"F={F}: observed / bound alm_mean vs sweep {r1:.3g}, alm_var vs L L^T {r2:.3g}")
    check_all(f"one row F={F}", dict(got, **wp.power()), P, stack)


# ---- 3. bit identities -----------------------------------------------------------------------------------------
def test_bit_equality_of_the_state():
    F, L, C, k = 3, 70, 3, 20
    P = R.synthetic(F, L, k, C, seed=5)
    x = P["stack"]
    one = feed(make(P, C), x)                                     # one launch of 20: two tiles and a tail of 4
    assert one.n == k
    for tag, kw in (("chunks of 8", dict(cuts=8, capacity=8)), ("single rows", dict(cuts=1, capacity=1)),
                    ("ring of 4 from iteration 3", dict(cuts=4, capacity=4, first=3)),
                    ("ring of 32, chunks of 7", dict(cuts=7, capacity=32, first=30))):
        other = feed(make(P, C), x, **kw)
        assert torch.equal(other.data, one.data), tag
    for b in range(C):
        solo = feed(make(P, 1), x[:, b:b + 1], cuts=8, capacity=8)
        assert torch.equal(solo.fields()[:, 0], one.fields()[:, b]), f"chain {b}"
    # restore: data= reproduces the state and its count, and continues it
    from gibbssampler_amd.engine import WienerPosterior
    back = WienerPosterior(F, L, C, P["bl"], P["bins"], P["kappa"], maxbins=P["maxbins"], data=one.data)
    back.data_moments(dev(P["d"]))
    more = R.synthetic(F, L, 3, C, seed=6)["stack"]
    feed(one, more, first=k + 1)
    feed(back, more, first=k + 1)
    assert back.n == k + 3 and torch.equal(back.data, one.data)
    # elements past the state's end are untouched
    n = one.data.numel()
    big = torch.full((n + 6,), -3.25, dtype=torch.float64, device="cuda")
    big[:n] = 0.0
    padded = make(P, C)
    padded.data = big[:n]
    feed(padded, x)
    feed(padded, more, first=k + 1)
    torch.cuda.synchronize()
    assert torch.equal(padded.data, one.data) and bool((big[n:] == -3.25).all())
    one.reset()
    assert one.n == 0 and bool((one.data == 0).all())


# ---- 4. gather -------------------------------------------------------------------------------------------------
def test_gather_concatenates_the_chains():
    F, L, k = 3, 16, 5
    P = R.synthetic(F, L, k, 4, seed=9)
    x, d = P["stack"], dev(P["d"])
    whole = feed(make(P, 4), x)
    a, b = feed(make(P, 2), x[:, :2]), feed(make(P, 2), x[:, 2:])
    want = results(whole, d)
    got = results(a, d, gather=lambda t, dim=1: torch.cat([t, b.fields()], dim=dim))
    assert got["chain_alm_mean"].shape == (4, F, (L + 1) ** 2)
    for key in OUTPUTS:
        assert torch.equal(got[key], want[key]) or \
            np.array_equal(host(got[key]), host(want[key]), equal_nan=True), key
    check_all("gathered", got, P, x)


def test_argument_errors():
    from gibbssampler_amd import _capi
    lib = _capi.load()
    P = R.synthetic(2, 5, 1, 2, seed=1)
    wp = make(P, 2)
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    st, q, s = _capi.ptr(wp.data), _capi.ptr(x), _capi.stream_ptr()
    e2b, bl, mom = _capi.ptr(wp.ell2bin), _capi.ptr(wp.bl), _capi.ptr(wp.moments)
    nb = ctypes.c_longlong()
    upd = lambda **kw: lib.gs_wf_update(*[kw.get(n, v) for n, v in (
        ("state", st), ("F", 2), ("C", 2), ("L", 5), ("maxbins", P["maxbins"]), ("bl", bl), ("e2b", e2b), ("k0", 1.0),
        ("k1", 1.0), ("k2", 0.0), ("mom", mom), ("trace", q), ("cap", 1), ("first", 1), ("nsteps", 1), ("count", 1),
        ("stream", s))])
    for call, word in ((lambda: lib.gs_wf_bytes(0, 2, 5, ctypes.byref(nb)), b"nfields"),
                       (lambda: lib.gs_wf_bytes(2, 0, 5, ctypes.byref(nb)), b"nchains"),
                       (lambda: lib.gs_wf_bytes(2, 2, -1, ctypes.byref(nb)), b"lmax"),
                       (lambda: lib.gs_wf_bytes(2, 2, 5, None), b"null bytes"),
                       (lambda: lib.gs_wf_reset(None, 2, 2, 5, s), b"null state"),
                       (lambda: lib.gs_wf_moments(5, 2, None, q, s), b"null d_alm"),
                       (lambda: upd(trace=None), b"null trace"),
                       (lambda: upd(bl=None), b"null bl"),
                       (lambda: upd(nsteps=2), b"nsteps <= capacity"),
                       (lambda: upd(first=0), b"first_iteration"),
                       (lambda: upd(count=0), b"count_after"),
                       (lambda: lib.gs_wf_finish(st, 2, 2, 5, q, q, q, None, q, s), b"null chain_alm_mean"),
                       (lambda: lib.gs_wf_power(st, 2, 2, 5, mom, q, None, q, s), b"null mean_power")):
        assert call() == -1 and word in lib.gs_last_error(), lib.gs_last_error()
    assert upd(nsteps=0) == 0
    torch.cuda.synchronize()
    assert wp.n == 0 and bool((wp.data == 0).all())
    with pytest.raises(ValueError):
        wp.update(torch.zeros(1, 2, 2, P["maxbins"] - 1, dtype=torch.float64, device="cuda"), 1, 1, 1)


# ---- 5. runner -------------------------------------------------------------------------------------------------
N_SIDE, L_MAX, SEED, N_ITER = 8, 16, 20261021, 40


def problem():
    from gibbssampler_amd.problem import synthetic_problem
    return synthetic_problem(L_MAX, N_SIDE, 3, seed=3)


def runner(kind, nchains, P=None):
    from gibbssampler_amd.samplers import BatchedRunner
    P = problem() if P is None else P
    return BatchedRunner(kind=kind, lmax=L_MAX, nside=N_SIDE, nfields=3, nchains=nchains, bl=P["bl"],
                         noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                         proposal_variances=P["proposal_variances"], rng="native", seed=SEED, store_skymap=False)


def stack_of(hist, r, rows):
    """history {spectrum: [rows, chains, nbins]} -> [k, C, nspec, maxbins] of the given rows"""
    p = r.plan
    out = np.zeros((len(rows), p.nchains, p.nspec, p.maxbins))
    for q, s in enumerate(p.spectra):
        out[:, :, q, :hist[s].shape[2]] = hist[s][rows]
    return out


@pytest.mark.parametrize("chunk", [8, 0])
@pytest.mark.parametrize("kind,nchains", [("centered", 1), ("asis", 3), ("noncentered", 3)])
def test_runner(kind, nchains, chunk):
    """posterior of the run = the restatement on the run's own D_l history; the
    histories do not change with the option."""
    P = problem()
    plain = runner(kind, nchains, P)
    h0, a0 = plain.run(P["dls_init"], N_ITER, graph_chunk=chunk)
    with pytest.raises(RuntimeError):
        plain.wiener_posterior()
    start = 5
    r = runner(kind, nchains, P)
    h, a = r.run(P["dls_init"], N_ITER, graph_chunk=chunk, wiener_posterior={"start": start})
    for s in h:
        assert np.array_equal(h[s], h0[s]), s
    if a0 is not None:
        for s in a:
            assert np.array_equal(a[s], a0[s]), s
    out = r.wiener_posterior()
    assert out["n"] == N_ITER - start
    off = 0 if kind == "asis" else 1                    # history row of iteration 1
    rows = np.arange(start + 1, N_ITER + 1) - 1 + off
    Q = dict(F=3, L=L_MAX, bl=P["bl"], bins=P["bins"], kappa=R.noise_weights(12 * N_SIDE ** 2, P["noise_var"]),
             d=np.asarray(P["d_alm"]))
    check_all(f"{kind} chunk={chunk}", out, Q, stack_of(h, r, rows))
    # default start: every iteration
    r.run(P["dls_init"], 12, graph_chunk=chunk, wiener_posterior=True)
    assert r.wiener_posterior()["n"] == 12


def test_runner_without_history_and_resume():
    P = problem()
    whole = runner("asis", 3, P)
    assert whole.run(P["dls_init"], N_ITER, graph_chunk=8, wiener_posterior=True, keep_history=False) == (None, None)
    assert whole.wiener_posterior()["n"] == N_ITER
    with pytest.raises(ValueError):
        runner("asis", 3, P).run(P["dls_init"], 4, keep_history=False)
    first = runner("asis", 3, P)
    first.run(P["dls_init"], 24, graph_chunk=8, wiener_posterior=True)
    st = first.state_dict()
    assert "wf_state" in st and st["wf_start"] == 0
    second = runner("asis", 3, P)
    second.run(None, 16, graph_chunk=8, resume=st)              # the restored state continues without the option
    assert torch.equal(second._wf.data, whole._wf.data)
    # an old checkpoint without the keys means "none"
    old = {k: v for k, v in st.items() if not k.startswith("wf_")}
    third = runner("asis", 3, P)
    third.run(None, 2, graph_chunk=8, resume=old)
    with pytest.raises(RuntimeError):
        third.wiener_posterior()


# ---- 6. class surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
def test_class_surface(F):
    from gibbssampler_amd.gibbs import ASIS, CenteredGibbs
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.sht import HealpixSHT
    N, L = N_SIDE, L_MAX
    P = synthetic_problem(L, N, F, seed=4)
    NR, npix = (L + 1) ** 2, 12 * N * N
    nspec, nop, C = (4, 5, 2) if F == 3 else (2, 2, 2)
    fields = ("TT", "EE", "BB")[3 - F:]
    alm = {f: P["d_alm"][i] for i, f in enumerate(fields)}
    nt, npol = (P["noise_var"][0], P["noise_var"][1]) if F == 3 else (P["noise_var"][0], P["noise_var"][0])
    kw = dict(polarization=True, all_sph=True, n_iter=6, rng="native", seed=9, nchains=C, bins=P["bins"],
              fields="TEB" if F == 3 else "EB")
    shapes = {"alm_mean": (F, NR), "alm_var": (F, NR), "alm_rhat": (F, NR), "chain_alm_mean": (C, F, NR),
              "power_of_mean": (nspec, L + 1), "mean_power": (nspec, L + 1), "map_mean": (F, npix),
              "op_mean": (nop, L + 1)}
    cg = CenteredGibbs(alm, nt, npol, 0.5, N, L, npix, wiener_posterior=True, **kw)
    with pytest.raises(RuntimeError):
        cg.posterior_wiener
    plain = CenteredGibbs(alm, nt, npol, 0.5, N, L, npix, **kw)
    h, h0 = cg.run(P["dls_init"])[0], plain.run(P["dls_init"])[0]
    for sp in h:
        np.testing.assert_array_equal(h[sp], h0[sp])
    with pytest.raises(RuntimeError):
        plain.posterior_wiener
    out = cg.posterior_wiener
    assert set(out) == set(shapes) | {"n"} and out["n"] == 6
    for key, shape in shapes.items():
        assert out[key].shape == shape and out[key].dtype == np.float64, key
    assert np.all(np.isfinite(out["alm_mean"])) and np.all(out["alm_var"] > 0)
    want = HealpixSHT(N, L).alm2map_batch(dev(out["alm_mean"])[None], F)[0]
    assert np.array_equal(out["map_mean"], host(want))
    asis = ASIS(alm, nt, npol, 0.5, N, L, npix, P["proposal_variances"], metropolis_blocks=P["blocks"],
                wiener_posterior={"start": 2}, keep_history=False, **kw)
    assert asis.run(P["dls_init"])[0] is None
    out = asis.posterior_wiener
    assert set(out) == set(shapes) | {"n"} and out["n"] == 4
