"""Streaming posterior mean and variance of the sky map (gs_smap.hip,
engine.SkymapMoments, the masked drivers' run(skymap_summary=)).

Every device result is held to the first-order rounding bounds of DESIGN.md
'Posterior sky map' (tests/_smap_ref.py: they depend on k, C and the data's
magnitude only) against a longdouble restatement that computes the moments
directly from the stacked samples.  Each test prints its largest observed /
bound ratio."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import sht as O  # noqa: E402
from tests import _smap_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def data(k, C, n, seed=0):
    """the large common offset is what separates Welford from raw sums: a raw
    sum of squares rounds at u k 1e12 ~ 1e-4, far outside the bounds"""
    return 1e6 + np.random.default_rng(seed).standard_normal((k, C, n))


def feed(st, x):
    for row in x:
        st.update(dev(row))
    return st


def check_finish(tag, fin, x):
    ref = R.moments(x)
    b = R.bounds(x, ref)
    ratios = {key: R.check(f"{tag} {key}", host(fin[key]), ref[key], b[key])
              for key in ("mean", "var", "chain_mean", "rhat")}
    print(f"{tag}: observed / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    return max(ratios.values())


# ---- 1. engine against longdouble --------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [9, 289, 578, 768])
def test_engine_against_longdouble(C, n):
    from gibbssampler_amd.engine import SkymapMoments
    worst = 0.0
    for k in (1, 2, 5):
        x = data(k, C, n, seed=100 * n + 10 * C + k)
        st = feed(SkymapMoments(C, n), x)
        assert st.n == k
        fin = st.finish()
        assert fin["n"] == k
        worst = max(worst, check_finish(f"C={C} n={n} k={k}", fin, x))
        var = host(fin["var"])
        if k == 1:
            assert np.all(np.isnan(var)) if C == 1 else np.all(np.isfinite(var))
            assert np.all(np.isnan(host(fin["rhat"])))
    print(f"C={C} n={n}: largest observed / bound ratio {worst:.3g}")


# ---- 2. bit identities ---------------------------------------------------------------------------------------
def test_bit_identities():
    from gibbssampler_amd.engine import SkymapMoments
    C, n, k = 3, 289, 4                      # odd n: chain 1's rows are only 8-byte aligned
    x = data(k, C, n, seed=7)
    st = feed(SkymapMoments(C, n), x)
    again = feed(SkymapMoments(C, n), x)
    assert torch.equal(st.data, again.data)                                   # two runs, identical states
    f = st.fields()
    for b in range(C):
        one = feed(SkymapMoments(1, n), x[:, b:b + 1])
        assert torch.equal(one.fields()[:, 0], f[:, b]), f"chain {b}"
    # a non-contiguous chain stride ([C, 2n] viewed as [:, :n]), also shifted by one
    # element so that x's rows change their 16-byte phase
    for shift in (0, 1):
        wide = SkymapMoments(C, n)
        for row in x:
            buf = torch.full((C, 2 * n + 1), 7.0, dtype=torch.float64, device="cuda")
            view = buf[:, shift:shift + n]
            view.copy_(dev(row))
            assert view.stride(0) == 2 * n + 1 and not view.is_contiguous()
            wide.update(view)
        assert torch.equal(wide.data, st.data), f"shift {shift}"
    # elements past the state's end are untouched
    pad = 6
    big = torch.full((st.data.numel() + pad,), -3.25, dtype=torch.float64, device="cuda")
    big[:st.data.numel()] = 0.0
    padded = SkymapMoments(C, n)
    padded.data = big[:st.data.numel()]
    feed(padded, x)
    torch.cuda.synchronize()
    assert torch.equal(padded.data, st.data)
    assert bool((big[st.data.numel():] == -3.25).all())
    # restore: data= / fields() reproduce the state and its count
    back = SkymapMoments(C, n, data=st.data)
    assert back.n == k and torch.equal(back.fields(), st.fields())
    x5 = data(1, C, n, seed=8)[0]
    st.update(dev(x5))
    back.update(dev(x5))
    assert torch.equal(back.data, st.data)
    st.reset()
    assert st.n == 0 and bool((st.data == 0).all())


def test_grid_stride_rows():
    """a row of more pairs than the launch has threads for (C = 3 caps grid.x at
    8192 // 3 workgroups of 256 pairs): the grid-stride path, with an odd n so
    that heads and tails exist.  Chain b equals a one-chain state, whose launch
    covers the row without striding, bit for bit; moments within the bound."""
    from gibbssampler_amd.engine import SkymapMoments
    C, k = 3, 2
    n = 2 * (8192 // C) * 256 + 2 * 256 * 5 + 1
    x = data(k, C, n, seed=31)
    st = feed(SkymapMoments(C, n), x)
    for b in (0, 1, 2):
        one = feed(SkymapMoments(1, n), x[:, b:b + 1])
        assert torch.equal(one.fields()[:, 0], st.fields()[:, b]), f"chain {b}"
    check_finish(f"grid-stride n={n}", st.finish(), x)


def test_argument_errors():
    from gibbssampler_amd import _capi
    from gibbssampler_amd.engine import SkymapMoments
    lib = _capi.load()
    st = SkymapMoments(2, 9)
    x = torch.zeros(2, 9, dtype=torch.float64, device="cuda")
    p, q, s = _capi.ptr(st.data), _capi.ptr(x), _capi.stream_ptr()
    nb = ctypes.c_longlong()
    for call, word in ((lambda: lib.gs_smap_bytes(0, 9, ctypes.byref(nb)), b": C "),
                       (lambda: lib.gs_smap_bytes(2, 0, ctypes.byref(nb)), b": n "),
                       (lambda: lib.gs_smap_bytes(2, 9, None), b"null bytes"),
                       (lambda: lib.gs_smap_reset(None, 2, 9, s), b"null state"),
                       (lambda: lib.gs_smap_update(p, 2, 9, None, 9, 1, s), b"null x"),
                       (lambda: lib.gs_smap_update(p, 2, 9, q, 9, 0, s), b"count_after"),
                       (lambda: lib.gs_smap_update(p, 0, 9, q, 9, 1, s), b": C "),
                       (lambda: lib.gs_smap_finish(p, 2, 9, q, q, None, q, s), b"null chain_mean"),
                       (lambda: lib.gs_smap_power(2, 2, q, None, q, q, s), b"null var")):
        assert call() == -1 and word in lib.gs_last_error(), lib.gs_last_error()
    with pytest.raises(ValueError):
        st.update(torch.zeros(2, 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        st.update(torch.zeros(9, 2, dtype=torch.float64, device="cuda").t())
    torch.cuda.synchronize()
    assert st.n == 0


# ---- 3. capture ----------------------------------------------------------------------------------------------
def test_update_is_capturable():
    """in-process, like the project's other graph tests (tests/test_gpu_br_device.py)"""
    from gibbssampler_amd.engine import SkymapMoments
    C, n = 3, 289
    x = data(3, C, n, seed=11)
    eager = feed(SkymapMoments(C, n), x)
    st = feed(SkymapMoments(C, n), x[:1])
    static = dev(x[1])
    torch.cuda.synchronize()
    graphs = []
    side = torch.cuda.Stream()
    for count in (2, 3):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                st.update(static, count_after=count)
        torch.cuda.current_stream().wait_stream(side)
        graphs.append(g)
    assert st.n == 1                                 # a capture runs nothing
    for g, row in zip(graphs, x[1:]):
        static.copy_(dev(row))
        g.replay()
    torch.cuda.synchronize()
    assert st.n == 3 and torch.equal(st.data, eager.data)


# ---- 4. power ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 16])
@pytest.mark.parametrize("F", [2, 3])
def test_power(L, F):
    from gibbssampler_amd.engine import SkymapMoments
    C, k, n = 2, 3, F * (L + 1) ** 2
    x = np.random.default_rng(L + F).standard_normal((k, C, n)) * 3.0 + 0.5
    st = feed(SkymapMoments(C, n), x)
    fin = st.finish()
    pw = st.power(L, F, finished=fin)
    pom, mp = R.power(host(fin["mean"]).reshape(F, -1), host(fin["var"]).reshape(F, -1), L)
    bp, bm = R.power_bounds(pom, mp, L)
    r1 = R.check("power_of_mean", host(pw["power_of_mean"]), pom, np.broadcast_to(bp, pom.shape))
    r2 = R.check("mean_power", host(pw["mean_power"]), mp, np.broadcast_to(bm, mp.shape))
    print(f"L={L} F={F}: observed / bound power_of_mean {r1:.3g}, mean_power {r2:.3g}")
    assert np.all(host(pw["mean_power"]) >= host(pw["power_of_mean"]))
    with pytest.raises(ValueError):
        st.power(L + 1, F)


# ---- 8. gather -----------------------------------------------------------------------------------------------
def test_gather_doubles_the_chains():
    from gibbssampler_amd.engine import SkymapMoments
    C, n, k = 3, 289, 4
    x = data(k, C, n, seed=21)
    st = feed(SkymapMoments(C, n), x)
    fin = st.finish()
    twice = st.finish(gather=lambda t, dim=1: torch.cat([t, t], dim=dim))
    assert twice["chain_mean"].shape == (2 * C, n)
    x2 = np.concatenate([x, x], axis=1)
    check_finish("gathered", twice, x2)
    b = R.bounds(x2)
    assert np.all(np.abs(host(twice["mean"]) - host(fin["mean"])) <= 2 * b["mean"])
    ref = R.moments(x2)
    assert np.all(host(twice["var"]) < host(fin["var"]))           # (N - 1) -> (2N - 1) under the same spread
    np.testing.assert_allclose(host(twice["var"]), ref["var"].astype(float), rtol=1e-6)


# ---- the masked problem of tests/test_gpu_batched.py, rebuilt locally ------------------------------------------
N_SIDE, L_MAX, SEED = 8, 16, 4242


def problem(seed=3):
    rng = np.random.default_rng(seed)
    N, L = N_SIDE, L_MAX
    npix = 12 * N * N
    th, _ = O.pixel_angles(N)
    mask = (np.abs(np.cos(th)) > 0.2).astype(float)
    maps = rng.standard_normal((3, npix)) * np.array([[30.0], [0.3], [0.3]])
    ntemp = np.full(npix, 40.0 ** 2) * np.linspace(0.9, 1.1, npix)
    npol = np.full(npix, 0.2 ** 2) * np.linspace(1.2, 0.8, npix)
    ell = np.arange(L + 1)
    bl = np.exp(-0.5 * ell * (ell + 1) * (0.07 / np.sqrt(8 * np.log(2))) ** 2)
    dl = {"EE": np.where(ell >= 2, 10.0 * (np.maximum(ell, 1) / 100) ** 0.5, 0), "BB": np.where(ell >= 2, 0.01, 0.0)}
    s0 = rng.standard_normal((4, 3, (L + 1) ** 2)) * np.array([[3.0], [0.05], [0.005]])
    return dict(mask=mask, maps=maps, ntemp=ntemp, npol=npol, bl=bl, dl=dl, s0=s0[:, 1:])


def make_cr(P, B, **kw):
    from gibbssampler_amd.masked import MaskedCR
    pix = {"Q": P["maps"][1], "U": P["maps"][2]}
    return MaskedCR(pix, P["ntemp"], P["npol"], P["bl"], L_MAX, N_SIDE, mask=P["mask"], nfields=2, rng="native",
                    seed=SEED, sht_mode="recurrence", chain=2, nchains=B, **kw)


def stack_of(maps, B):
    """list of k device maps [B?, F, NR] -> [k, B, F NR] numpy"""
    return np.stack([host(m).reshape(B, -1) for m in maps])


def check_summary(tag, out, maps, B):
    x = stack_of(maps, B)
    ref = R.moments(x)
    b = R.bounds(x, ref)
    F, NR = 2, (L_MAX + 1) ** 2
    assert out["n"] == len(maps)
    assert out["alm_mean"].shape == (F, NR) and out["chain_alm_mean"].shape == (B, F, NR)
    ratios = [R.check(f"{tag} alm_mean", out["alm_mean"].reshape(-1), ref["mean"], b["mean"]),
              R.check(f"{tag} alm_var", out["alm_var"].reshape(-1), ref["var"], b["var"]),
              R.check(f"{tag} chain_alm_mean", out["chain_alm_mean"].reshape(B, -1), ref["chain_mean"],
                      b["chain_mean"]),
              R.check(f"{tag} alm_rhat", out["alm_rhat"].reshape(-1), ref["rhat"], b["rhat"])]
    pom, mp = R.power(out["alm_mean"], out["alm_var"] if len(maps) * B >= 2 else np.zeros_like(out["alm_mean"]),
                      L_MAX)
    bp, bm = R.power_bounds(pom, mp, L_MAX)
    ratios.append(R.check(f"{tag} power_of_mean", out["power_of_mean"], pom, np.broadcast_to(bp, pom.shape)))
    if len(maps) * B >= 2:
        ratios.append(R.check(f"{tag} mean_power", out["mean_power"], mp, np.broadcast_to(bm, mp.shape)))
    print(f"{tag}: largest observed / bound ratio {max(ratios):.3g}")


# ---- 5. runners ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_masked_runner(B):
    """MaskedRunner (aux + MALA composition of the a12 ladder): runner.s after runs
    of 1, 2 and 3 iterations with the same seed are the post-CR maps s_1, s_2,
    s_3 (the runs share their prefixes: histories compared)."""
    from gibbssampler_amd.masked import MaskedRunner
    P = problem()
    bins = {"EE": np.arange(L_MAX + 2), "BB": np.arange(L_MAX + 2)}
    init = {"EE": P["dl"]["EE"], "BB": P["dl"]["BB"]}
    s0 = P["s0"][:B] if B > 1 else P["s0"][0]

    def run(n_iter, **kw):
        r = MaskedRunner(make_cr(P, B, gibbs_cr=True, ula=True, n_gibbs=1), bins)
        h, a, _, _ = r.run(init, n_iter, s0, **kw)
        return r, h, a

    plain = [run(i) for i in (1, 2, 3)]
    h3, a3 = plain[2][1], plain[2][2]
    for i, (_, h, a) in enumerate(plain[:2]):
        for sp in h:
            np.testing.assert_array_equal(h[sp], h3[sp][:i + 2], err_msg=f"prefix {i + 1} {sp}")
        np.testing.assert_array_equal(a, a3[:i + 1])
    s = [r.s.clone() for r, _, _ in plain]
    with pytest.raises(RuntimeError):
        plain[2][0].skymap_summary()
    for tag, opt, pick in (("all", True, (0, 1, 2)), ("start=1", {"start": 1}, (1, 2)),
                           ("every=2", {"every": 2}, (0, 2))):
        r, h, a = run(3, skymap_summary=opt)
        for sp in h:
            np.testing.assert_array_equal(h[sp], h3[sp], err_msg=f"{tag} {sp}")
        np.testing.assert_array_equal(a, a3)
        assert torch.equal(r.s, s[2])
        check_summary(f"MaskedRunner B={B} {tag}", r.skymap_summary(), [s[i] for i in pick], B)


@pytest.mark.parametrize("B", [1, 3])
def test_masked_asis_runner(B):
    """MaskedMHRunner("asis") with the PCG CR kind.  runner.s is the RE-CENTRED map
    (ASIS.py:203), not the one the CR step produced, so the post-CR maps s_i are
    captured through a one-iteration replay of the CR step with the same seed
    and iteration: s_i = PCG(D_{i-1}, iteration i), D_{i-1} the history row
    i - 1 of the run without the option (the PCG takes no start map)."""
    from gibbssampler_amd.masked import MaskedMHRunner, KIND_PCG
    P = problem()
    L = L_MAX
    bins = {"EE": np.arange(L + 2), "BB": np.array([0, 2, 5, 9, 13, L + 1])}
    blocks = {"EE": np.array([2, 6, L + 1]), "BB": np.array([2, 3, 4, 5])}
    ell = np.arange(2, L + 1)
    pv = {"EE": (0.05 * 10.0 * (ell / 100.0) ** 0.5) ** 2, "BB": np.full(len(bins["BB"]) - 3, (0.2 * 0.01) ** 2)}
    start = {"EE": P["dl"]["EE"].copy(), "BB": np.array([np.mean(P["dl"]["BB"][bins["BB"][i]:bins["BB"][i + 1]])
                                                         for i in range(len(bins["BB"]) - 1)])}

    def make():
        return MaskedMHRunner("asis", make_cr(P, B, gibbs_cr=False, ula=False, pcg_accuracy=1e-6), bins, blocks, pv,
                              cr_kind_=KIND_PCG)

    r0 = make()
    h3, acc3 = r0.run(start, 3)[:2]
    h2 = make().run(start, 2)[0]
    for sp in h3:
        np.testing.assert_array_equal(h2[sp], h3[sp][:3], err_msg=f"prefix {sp}")
    rep = make()
    s = []
    for i in (1, 2, 3):
        rows = [{sp: (h3[sp][i - 1] if B == 1 else h3[sp][i - 1, b]) for sp in h3} for b in range(B)]
        dl = rep.mh.unfold(rep.plan.dl_tensor(rows))
        dl = dl.reshape(rep.cr._shape(*dl.shape[1:])) if B == 1 else dl
        s.append(rep.cr.pcg_solve(dl, rep.cr.pcg_rhs(dl, iteration=i)).clone())
    for tag, opt, pick in (("all", True, (0, 1, 2)), ("start=1", {"start": 1}, (1, 2)),
                           ("every=2", {"every": 2}, (0, 2))):
        r = make()
        h, acc = r.run(start, 3, skymap_summary=opt)[:2]
        for sp in h:
            np.testing.assert_array_equal(h[sp], h3[sp], err_msg=f"{tag} {sp}")
            np.testing.assert_array_equal(acc[sp], acc3[sp], err_msg=f"{tag} {sp} accepts")
        assert torch.equal(r.s, r0.s)
        check_summary(f"MaskedMHRunner asis B={B} {tag}", r.skymap_summary(), [s[i] for i in pick], B)


# ---- 6. pixels -----------------------------------------------------------------------------------------------
def test_pixels():
    """map_mean = alm2map(alm_mean) against the mean of the three synthesised maps:
    equal by linearity up to the transform's rounding.  Each transform is held to
    atol = 1e-11 max|map| at this size by tests/test_gpu_sht.py (its comparisons
    with the oracle), so the two sides differ by at most twice that."""
    from gibbssampler_amd.masked import MaskedRunner
    from gibbssampler_amd.sht import HealpixSHT
    P, B = problem(), 3
    bins = {"EE": np.arange(L_MAX + 2), "BB": np.arange(L_MAX + 2)}
    init = {"EE": P["dl"]["EE"], "BB": P["dl"]["BB"]}

    def run(n_iter, **kw):
        r = MaskedRunner(make_cr(P, B, gibbs_cr=True, ula=True, n_gibbs=1), bins)
        r.run(init, n_iter, P["s0"][:B], **kw)
        return r

    s = [run(i).s.clone() for i in (1, 2, 3)]
    r = run(3, skymap_summary={"pixels": True})
    out = r.skymap_summary()
    npix = 12 * N_SIDE ** 2
    assert out["map_mean"].shape == (2, npix) and out["map_var"].shape == (2, npix) and out["n"] == 3
    sht = HealpixSHT(N_SIDE, L_MAX)
    maps = [sht.alm2map_batch(m.reshape(B, 2, -1), 2) for m in s]
    assert np.array_equal(out["map_mean"], host(sht.alm2map_batch(dev(out["alm_mean"])[None], 2))[0])
    x = stack_of(maps, B)
    ref = R.moments(x)
    scale = np.abs(x).max()
    err = np.abs(out["map_mean"].reshape(-1) - ref["mean"].astype(float)).max()
    print(f"map_mean vs mean of maps: {err / scale:.3g} of max|map| (bound 2e-11)")
    assert err <= 2e-11 * scale
    b = R.bounds(x, ref)
    r1 = R.check("map_var", out["map_var"].reshape(-1), ref["var"], b["var"])
    r2 = R.check("map_rhat", out["map_rhat"].reshape(-1), ref["rhat"], b["rhat"])
    print(f"pixels: observed / bound map_var {r1:.3g}, map_rhat {r2:.3g}")
    assert "map_var" not in run(1, skymap_summary=True).skymap_summary()


# ---- 7. class surface ----------------------------------------------------------------------------------------
def test_class_surface():
    from gibbssampler_amd.gibbs import CenteredGibbs, ASIS
    P = problem()
    N, L = N_SIDE, L_MAX
    NR, npix = (L + 1) ** 2, 12 * N * N
    pix = {"Q": P["maps"][1], "U": P["maps"][2]}
    init = {"EE": P["dl"]["EE"], "BB": P["dl"]["BB"]}
    kw = dict(mask_path=P["mask"], polarization=True, n_iter=2, rng="native", seed=9, nchains=2)
    shapes = {"alm_mean": (2, NR), "alm_var": (2, NR), "alm_rhat": (2, NR), "chain_alm_mean": (2, 2, NR),
              "power_of_mean": (2, L + 1), "mean_power": (2, L + 1), "map_mean": (2, npix)}
    cg = CenteredGibbs(pix, P["ntemp"], P["npol"], 4.0, N, L, npix, gibbs_cr=True, skymap_summary=True, **kw)
    with pytest.raises(RuntimeError):
        cg.posterior_skymap
    plain = CenteredGibbs(pix, P["ntemp"], P["npol"], 4.0, N, L, npix, gibbs_cr=True, **kw)
    h, h0 = cg.run(init)[0], plain.run(init)[0]
    for sp in h:
        np.testing.assert_array_equal(h[sp], h0[sp])
    with pytest.raises(RuntimeError):
        plain.posterior_skymap
    out = cg.posterior_skymap
    assert set(out) == set(shapes) | {"n"} and out["n"] == 2
    for key, shape in shapes.items():
        assert out[key].shape == shape and out[key].dtype == np.float64, key
    assert np.all(np.isfinite(out["alm_mean"])) and np.all(out["alm_var"] >= 0)
    ell = np.arange(2, L + 1)
    pv = {"EE": (0.05 * 10.0 * (ell / 100.0) ** 0.5) ** 2, "BB": np.full(L - 1, (0.2 * 0.01) ** 2)}
    asis = ASIS(pix, P["ntemp"], P["npol"], 4.0, N, L, npix, pv, skymap_summary={"pixels": True, "start": 1}, **kw)
    with pytest.raises(RuntimeError):
        asis.posterior_skymap
    asis.run(init)
    out = asis.posterior_skymap
    shapes.update(map_var=(2, npix), map_rhat=(2, npix))
    assert set(out) == set(shapes) | {"n"} and out["n"] == 1
    for key, shape in shapes.items():
        assert out[key].shape == shape, key
    # the drivers this pull request does not open: full-sky harmonic and TT pixel runs
    alm = {"EE": np.zeros(NR), "BB": np.zeros(NR)}
    with pytest.raises(NotImplementedError, match="skymap_summary"):
        CenteredGibbs(alm, 1.0, 1.0, 4.0, N, L, npix, polarization=True, all_sph=True, skymap_summary=True)
    with pytest.raises(NotImplementedError, match="skymap_summary"):
        CenteredGibbs(np.zeros(npix), np.ones(npix), None, 4.0, N, L, npix, skymap_summary=True)
    with pytest.raises(ValueError):
        CenteredGibbs(pix, P["ntemp"], P["npol"], 4.0, N, L, npix, skymap_summary={"every": 0}, **kw)
