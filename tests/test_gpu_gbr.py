"""GPU: the Gaussianised Blackwell-Rao likelihood (gs_gbr_*, BlackwellRaoSamples.
gaussianize, engine.GaussianizedBlackwellRao) and the D_l draws of the bank.

Every stage is compared with tests/_gbr.py (order-free longdouble sums) fed with
the device's output of the stage before it, within bounds that are derived and
not tuned (units of 2^-52 times the magnitudes of the terms):
  logp     _gbr.logp_bound: 16 units of |alpha log beta| + beta / D, |lgamma(alpha)|,
           (alpha + 1) |log D| and log N, and n 2^-52 for the re-ordered sums
  x, sx    from the device's logp: the two cumulative sums carry (G + 8) (2^-52 +
           2^-1074 / F) relative each, F the scaled one-sided cumulative (its terms
           round absolutely once they are denormal) (G rounded additions of positive terms, exp and the
           product), x moves by F / phi(x) <= 1.26 per unit of relative error of
           its cumulative, plus 8 2^-52 |x| for the quantile itself:
           |dx| <= 2^-52 (2.52 (G + 8) + 8 |x|); sx, an exponential of a sum, relative
           2^-52 (2 (G + 8) + 16) + 2 |x| |dx|  [d(x^2 / 2) = |x| |dx|, with room]
  S1, S2   from the device's tables: sum_i xerr_ij (+ n 2^-52 sum_i |x_ij|) and
           sum_i (xerr_ij |x_ik| + |x_ij| xerr_ik) + (n + 8) 2^-52 sum_i |x_ij x_ik|,
           xerr of _gbr.transform (the matrix cores add the rows in their own order)
  mu, cov  from the device's sums, host fp64: 8 2^-52 (|S2| / N + mu^2) N / (N - 1)
  loglike  _gbr.loglike_bound, from the device's tables, mu and covariance
Largest |device - restatement| / bound seen on an MI355X: DESIGN.md 'Gaussianised
Blackwell-Rao likelihood'."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_likelihood as R  # noqa: E402
from tests import _gbr as GB  # noqa: E402
from tests import _mh_adapt as A  # noqa: E402
from tests import test_gpu_br_likelihood as L  # noqa: E402
from tests import test_gpu_br_samples as S  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = L.SEED
EPS = 2.0 ** -52
G = 64


def make_case(F, T, C=3, unbinned=False, lrange=None, nan_row=None):
    """A synthetic scale history and D_l draws beside it: rows, dls [T, C, nspec, maxbins]."""
    from gibbssampler_amd.engine import br_shapes
    cs = S.case(F, 2, unbinned, T=T, C=C, lrange=lrange)
    rows = cs["rows"].copy()
    alpha, half = br_shapes(F, cs["bins"], cs["maxbins"])
    rng = np.random.default_rng(SEED + T)
    fac = np.array([0.5 if (half >> k) & 1 else 1.0 for k in range(rows.shape[2])])[None, None, :, None]
    with np.errstate(all="ignore"):
        g = rng.gamma(np.where(np.isfinite(alpha), alpha, 1.0), 1.0, size=rows.shape)
        dls = np.where(np.isfinite(alpha)[None, None], rows * fac / g, rows)
    if nan_row is not None:
        i, c = nan_row
        k, b = np.argwhere(cs["mask"] & np.isfinite(alpha))[0]
        rows[i, c, k, b] = -1.0                                  # a skipped row: r is NaN
    cs.update(rows=rows, dls=dls)
    return cs


def bank_of(cs, rows=None, dls=None, cuts=None, cap=8, draws=True):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    rows = cs["rows"] if rows is None else rows
    dls = cs["dls"] if dls is None else dls
    T, C = rows.shape[:2]
    bank = BlackwellRaoSamples(C, cs["F"], cs["bins"], cs["mask"], T, draws=draws)
    x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(dls)).cuda()
    ring = torch.full((cap,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    tring = torch.full_like(ring, float("nan"))
    it, row = 1, 0
    for k in (cuts if cuts is not None else [min(cap, T - i) for i in range(0, T, cap)]):
        for i in range(k):
            ring[(it + i - 1) % cap].copy_(x[row + i])
            tring[(it + i - 1) % cap].copy_(d[row + i])
        bank.append(ring, cap, it, k, tring if draws else None)
        it, row = it + k, row + k
    torch.cuda.synchronize()
    assert bank.n == T
    return bank


def ratio(what, got, want, bound):
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    r = float(np.max(np.abs(got - want) / np.broadcast_to(bound, want.shape)))
    print(f"  {what}: max |device - restatement| / bound = {r:.4f} (max bound {np.max(bound):.3e})")
    return r


# ---- 1. draw packing -------------------------------------------------------------------------------------
def test_draw_packing():
    cs = make_case(3, 12)
    ref = bank_of(cs, cuts=(12,), cap=32)
    plain = bank_of(cs, cuts=(12,), cap=32, draws=False)
    assert plain.Dl is None and ref.nbytes(5) == 8 * 3 * 5 * (2 * ref.Jp + 1) and plain.nbytes(5) == 8 * 3 * 5 * (ref.Jp + 1)
    assert torch.equal(ref.X, plain.X) and torch.equal(ref.r, plain.r)
    cols = ref.cols.cpu().numpy()
    want = cs["dls"].reshape(12, 3, -1)[:, :, cols].transpose(1, 0, 2)
    assert np.array_equal(ref.Dl[:, :, :ref.Ju].cpu().numpy(), want) and not ref.Dl[:, :, ref.Ju:].any()
    for cuts, cap in (((3, 8, 1), 32), ((3, 8, 1), 8), ((1,) * 12, 1), ((5, 7), 8)):      # (5, 7) in 8 slots wraps
        got = bank_of(cs, cuts=cuts, cap=cap)
        assert torch.equal(got.Dl, ref.Dl) and torch.equal(got.X, ref.X) and torch.equal(got.r, ref.r), (cuts, cap)


# ---- 2, 3, 4. the fit and the evaluator ------------------------------------------------------------------
SHAPES = {"eb": dict(F=2, T=70, lrange=(2, 10), nan_row=(9, 1)), "unbinned": dict(F=2, T=70, unbinned=True, lrange=(2, 40)),
          "teb": dict(F=3, T=517)}


@pytest.fixture(scope="module", params=list(SHAPES))
def fitted(request):
    cs = make_case(**SHAPES[request.param])
    bank = bank_of(cs, cap=64)
    return request.param, cs, bank, bank.gaussianize(points=G)


def test_shapes_cross_the_boundaries(fitted):
    import ctypes
    from gibbssampler_amd import _capi as C
    name, cs, bank, gbr = fitted
    nb, br, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert C.load().gs_gbr_info(bank.n, gbr.Jg, ctypes.byref(nb), ctypes.byref(br), ctypes.byref(ct)) == 0
    assert ct.value == 64 and br.value % 64 == 0 and nb.value * br.value >= bank.n
    if name == "eb":
        assert bank.n % 64 and bank.n > 64 and bank.n % 4 and gbr.Jg % 4 and nb.value == 1
        assert int(torch.isnan(bank.r).sum()) == 1
    if name == "unbinned":
        assert gbr.Jg == 78
    if name == "teb":
        assert nb.value == 3 and gbr.Jg < bank.Ju and bool((bank.kind == 2).any())


def test_fit_accuracy(fitted):
    from gibbssampler_amd.engine import gbr_columns
    name, cs, bank, gbr = fitted
    n, Jg = bank.n, gbr.Jg
    col = gbr_columns(cs["F"], cs["bins"], cs["mask"])
    good = ~np.isnan(bank.r.cpu().numpy())
    beta = bank.X.cpu().numpy()[:, :, col["gcol"]] * col["half"]
    D = bank.Dl.cpu().numpy()[:, :, col["gcol"]]
    glo, gh = gbr.glo.cpu().numpy(), gbr.gh.cpu().numpy()
    worst = {}
    # logp
    want, tmax, N = GB.marginals(beta, good, col["alpha"], glo, gh, G)
    assert N == gbr.n == good.sum()
    logp = gbr.logp.cpu().numpy()
    worst["logp"] = ratio(f"{name} logp", logp, want, GB.logp_bound(tmax, N, col["alpha"], glo, gh, G, N))
    # tables from the device's logp
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    tx, tp = gbr.tx.cpu().numpy(), gbr.tp.cpu().numpy()
    # the same nodes are lost to underflow (far tails of a narrow marginal on a wide grid), never node 1
    assert np.array_equal(np.isinf(tx[:, :, 0]), np.isinf(x)) and np.isfinite(tx[:, 1, 0]).all()
    fin = np.isfinite(x)
    # the one-sided cumulative each x comes from, in the kernel's scaled units: where it nears the
    # smallest double its terms are denormal and round absolutely (2^-1074 each), not relatively
    lq = logp + GB.nodes(glo, gh, G).astype(np.float64)
    q = np.exp(lq - lq.max(axis=1, keepdims=True))
    cell = 0.5 * (q[:, :-1] + q[:, 1:]) * gh[:, None]
    FL = np.concatenate([np.zeros((Jg, 1)), np.cumsum(cell, axis=1)], axis=1)
    FR = np.concatenate([np.cumsum(cell[:, ::-1], axis=1)[:, ::-1], np.zeros((Jg, 1))], axis=1)
    Fs = np.where(FL / FL[:, -1:] <= 0.5, FL, FR)[fin]
    bx = 2.52 * (G + 8) * (EPS + 2.0 ** -1074 / Fs) + EPS * 8 * np.abs(x[fin])
    worst["x"] = ratio(f"{name} x", tx[:, :, 0][fin], x[fin], bx)
    bs = sx[fin] * EPS * (2 * (G + 8) + 16) + sx[fin] * 2 * np.abs(x[fin]) * bx
    worst["sx"] = ratio(f"{name} sx", tx[:, :, 1][fin], sx[fin], bs)
    assert np.array_equal(tp[:, :, 0], logp)
    worst["sp"] = ratio(f"{name} sp", tp[:, :, 1], sp, 4 * EPS * np.abs(logp).max(axis=1, keepdims=True))
    worst["mass"] = ratio(f"{name} mass", gbr.mass, mass, EPS * (G + 16) * mass)
    # moments from the device's tables
    xs, inside, xerr = GB.transform(D, glo, gh, tx)
    assert inside[good].all()
    xs, xerr = np.where(good[:, :, None], xs, 0), np.where(good[:, :, None], xerr, 0.0)
    cnt, S1, S2 = GB.moments(xs, good)
    ax = np.abs(xs.astype(np.float64))
    part = gbr.chain_sums
    assert np.array_equal(part["cnt"].cpu().numpy(), cnt)
    worst["S1"] = ratio(f"{name} S1", part["S1"].cpu().numpy(), S1, xerr.sum(axis=1) + n * EPS * ax.sum(axis=1) + 1e-300)
    b2 = np.einsum("cij,cik->cjk", xerr, ax)
    b2 = b2 + b2.transpose(0, 2, 1) + (n + 8) * EPS * np.einsum("cij,cik->cjk", ax, ax)
    S2d = part["S2"].cpu().numpy()
    worst["S2"] = ratio(f"{name} S2", S2d, S2, b2 + 1e-300)
    assert np.array_equal(S2d, S2d.transpose(0, 2, 1))
    # the finish from the device's sums
    N, mu, cov = GB.finish(cnt, part["S1"].cpu().numpy(), S2d)
    s2 = np.abs(S2d).sum(axis=0)
    worst["mu"] = ratio(f"{name} mu", gbr.mu.cpu().numpy(), mu, 8 * EPS * np.abs(part["S1"].cpu().numpy()).sum(axis=0) / N + 1e-300)
    bc = 8 * EPS * (s2 / N + np.abs(np.outer(mu, mu)).astype(np.float64)) * N / (N - 1)
    worst["cov"] = ratio(f"{name} cov", gbr.cov, cov, bc)
    # loglike from the device's tables, mu and covariance
    med = np.median(D.reshape(-1, Jg), axis=0)
    theory = np.ones((3,) + cs["mask"].shape)
    flat = theory.reshape(3, -1)
    flat[:, col["tcol"]] = med[None, :] * np.array([1.0, 0.9, 1.15])[:, None]
    res = gbr.loglike(theory)
    ref = GB.loglike(flat[:, col["tcol"]], glo, gh, tx, tp, gbr.mu.cpu().numpy(), gbr.cov)
    assert not res["outside"].any() and res["n"] == N
    worst["marginal"] = ratio(f"{name} marginal", res["marginal"], ref["marginal"],
                              ref["lperr"].sum(axis=1) + (Jg + 8) * EPS * np.abs(ref["marginal"]))
    worst["loglike"] = ratio(f"{name} loglike", res["loglike"], ref["loglike"], GB.loglike_bound(ref, gbr.cov))
    assert max(worst.values()) <= 1.0, worst


def test_determinism_and_evaluator(fitted, tmp_path):
    from gibbssampler_amd.engine import GaussianizedBlackwellRao, gbr_columns
    name, cs, bank, gbr = fitted
    again = bank.gaussianize(points=G)                          # twice the same
    for k in ("tx", "tp", "mu", "chol"):
        assert torch.equal(getattr(again, k), getattr(gbr, k)), k
    # evaluator: device tensor against numpy, save / load, outside
    col = gbr_columns(cs["F"], cs["bins"], cs["mask"])
    med = np.median(bank.Dl.cpu().numpy()[:, :, col["gcol"]].reshape(-1, gbr.Jg), axis=0)
    theory = np.ones((3,) + cs["mask"].shape)
    flat = theory.reshape(3, -1)
    flat[:, col["tcol"]] = med[None, :] * np.array([1.0, 0.9, 1.15])[:, None]
    flat[2, col["tcol"][1]] = 0.5 * float(torch.exp(gbr.glo[1] + gbr.gh[1]))     # below node 1: off the interval
    res = gbr.loglike(theory)
    rt = gbr.loglike_t(torch.from_numpy(theory).cuda())
    for k in ("loglike", "marginal", "outside"):
        assert np.array_equal(rt[k].cpu().numpy(), res[k]), k
    assert list(res["outside"]) == [0, 0, 1] and np.isneginf(res["loglike"][2]) and np.isfinite(res["loglike"][:2]).all()
    assert set(res) == {"loglike", "marginal", "outside", "n", "mass"} and res["mass"].shape == (gbr.Jg,)
    path = str(tmp_path / "gbr.npz")
    gbr.save(path)
    back = GaussianizedBlackwellRao.load(path)
    r2 = back.loglike(theory)
    assert all(np.array_equal(r2[k], res[k]) for k in res)


def test_chain_alone(fitted):
    """(m, S), S1 and S2 of chain 2 alone, on the full fit's grid and tables, are chain
    2's of the three, bit for bit."""
    import ctypes
    from gibbssampler_amd import _capi as C
    from gibbssampler_amd.engine import gbr_columns
    name, cs, bank, gbr = fitted
    solo = bank_of(cs, rows=cs["rows"][:, 2:], dls=cs["dls"][:, 2:], cap=37)
    col = gbr_columns(cs["F"], cs["bins"], cs["mask"])
    gcol, alpha, half = (torch.from_numpy(col[k]).cuda() for k in ("gcol", "alpha", "half"))
    lib = C.load()
    f64 = torch.float64
    m = torch.zeros(1, gbr.Jg, G, dtype=f64, device="cuda")
    Sx = torch.zeros(1, gbr.Jg, G, dtype=f64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    C.check(lib.gs_gbr_marginals(C.ptr(solo.X), C.ptr(solo.r), 1, solo.capacity, solo.n, solo.Ju, gbr.Jg, C.ptr(gcol),
                                 C.ptr(alpha), C.ptr(half), C.ptr(gbr.glo), C.ptr(gbr.gh), G, C.ptr(m), C.ptr(Sx),
                                 C.ptr(cnt), C.stream_ptr()), "gs_gbr_marginals")
    wb = ctypes.c_longlong()
    assert lib.gs_gbr_moments_work_bytes(1, solo.n, gbr.Jg, ctypes.byref(wb)) == 0
    work = torch.empty(wb.value // 8, dtype=f64, device="cuda")
    S1 = torch.zeros(1, gbr.Jg, dtype=f64, device="cuda")
    S2 = torch.zeros(1, gbr.Jg, gbr.Jg, dtype=f64, device="cuda")
    C.check(lib.gs_gbr_moments(C.ptr(solo.Dl), C.ptr(solo.r), 1, solo.capacity, solo.n, solo.Ju, gbr.Jg, C.ptr(gcol),
                               C.ptr(gbr.tx), C.ptr(gbr.glo), C.ptr(gbr.gh), G, C.ptr(work), wb.value, C.ptr(S1),
                               C.ptr(S2), C.stream_ptr()), "gs_gbr_moments")
    torch.cuda.synchronize()
    part = gbr.chain_sums
    assert torch.equal(m[0], part["m"][2]) and torch.equal(Sx[0], part["S"][2]) and int(cnt[0]) == int(part["cnt"][2])
    assert torch.equal(S1[0], part["S1"][2]) and torch.equal(S2[0], part["S2"][2])


def test_two_banks_gathered():
    """Two 2-chain banks gathered with a concatenating stub give the 4-chain fit's bits."""
    from gibbssampler_amd.engine import gbr_columns
    cs = make_case(2, 70, C=4)
    full = bank_of(cs, cap=64).gaussianize(points=G)
    a = bank_of(cs, rows=cs["rows"][:, :2], dls=cs["dls"][:, :2], cap=64)
    b = bank_of(cs, rows=cs["rows"][:, 2:], dls=cs["dls"][:, 2:], cap=64)
    gl = torch.from_numpy(gbr_columns(2, cs["bins"], cs["mask"])["gcol"]).cuda().long()
    ext = {k: (bk.Dl[:, :, gl].amin(dim=(0, 1))[None], bk.Dl[:, :, gl].amax(dim=(0, 1))[None]) for k, bk in (("a", a), ("b", b))}
    a_part, sent, calls = [], [], [0]

    def first_a(t, dim):
        # rank a's marginal partials on the shared grid (calls 3 .. 5); the rest is not used
        calls[0] += 1
        if calls[0] <= 2:
            return torch.cat([t, ext["b"][calls[0] - 1]], dim=0)
        if calls[0] <= 5:
            a_part.append(t.clone())
        return t

    a.gaussianize(points=G, gather=first_a)
    calls[0] = 0

    def rank_b(t, dim):
        # rank b's view: a's extremes and marginal partials before its own, so that it builds the
        # shared tables; what it sends is recorded (its own finish is not used)
        calls[0] += 1
        if calls[0] <= 2:
            return torch.cat([ext["a"][calls[0] - 1], t], dim=0)
        sent.append(t.clone())
        return torch.cat([a_part[calls[0] - 3], t], dim=dim) if calls[0] <= 5 else t

    try:                                                        # its finish mixes N of four chains with sums of two
        b.gaussianize(points=G, gather=rank_b)
    except ValueError as e:
        assert "more kept samples than columns" in str(e)
    calls[0] = 0

    def rank_a(t, dim):
        calls[0] += 1
        if calls[0] <= 2:
            return torch.cat([t, ext["b"][calls[0] - 1]], dim=0)
        return torch.cat([t, sent[calls[0] - 3]], dim=dim)

    got = a.gaussianize(points=G, gather=rank_a)
    for k in ("glo", "gh", "tx", "tp", "mu", "chol"):
        assert torch.equal(getattr(got, k), getattr(full, k)), k
    assert got.n == full.n and got.logdet == full.logdet


# ---- 6. option off ---------------------------------------------------------------------------------------
def test_option_off(tmp_path):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = make_case(3, 12)
    plain = bank_of(cs, cuts=(12,), cap=32, draws=False)
    with pytest.raises(ValueError, match="draws"):
        plain.gaussianize()
    p0, p1 = str(tmp_path / "plain.npz"), str(tmp_path / "draws.npz")
    plain.save(p0)
    with np.load(p0) as f:
        assert "Dl" not in f.files
    back = BlackwellRaoSamples.load(p0)
    assert back.Dl is None and not back.draws and torch.equal(back.X[:, :12], plain.X)
    with pytest.raises(ValueError, match="draws"):
        back.gaussianize()
    full = bank_of(cs, cuts=(12,), cap=32)
    full.save(p1)
    again = BlackwellRaoSamples.load(p1)
    assert again.draws and torch.equal(again.Dl[:, :12], full.Dl) and torch.equal(again.X[:, :12], full.X)
    few = bank_of(make_case(2, 12, unbinned=True, lrange=(2, 40)), cuts=(12,), cap=32)
    with pytest.raises(ValueError, match="more kept samples than columns"):
        few.gaussianize(points=G)                               # N = 36 kept samples, Jg = 78 columns


# ---- 5. surface ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["centered", "asis"])
def test_surface(kind):
    """CenteredGibbs / ASIS, EB, N_side 8, l_max 16 (the reference golden problem), 4
    chains x 200 iterations: the bank's draws are the history, and gaussianize().loglike
    matches the restatement of the whole fit (marginals, tables, moments, finish) on the
    downloaded X, r and Dl.  The sanity condition holds on the oracle's CPU chain of the
    same problem with room (tools/gbr_cpu_check.py: |mu| <= 0.08, C_jj in [0.90, 1.09]).
    Bound of the end-to-end loglike, first order: the evaluator's own bound
    (_gbr.loglike_bound) plus the tables' errors carried through the form -- with dx_j =
    2.52 max_g logp_bound + 2^-52 (2.52 (G + 8) + 8 |x|_max) the error of column j's x
    table and of each transformed draw, every x (of the theory and, through mu and C, of
    the draws) moves loglike by at most (1 + 4 Jg cond(C)) (|x_j - (C^-1 (x - mu))_j| + |x_j|
    + 1) dx_j, and log p by max_g logp_bound."""
    from gibbssampler_amd import gibbs
    from gibbssampler_amd.engine import GBR_POINTS, BlackwellRaoSamples, gbr_columns
    from tests._golden import init_of, load
    g = load(16)
    Npix, T = int(g["Npix"]), 200
    pix = {"EE": g["d_E"], "BB": g["d_B"], "Q": np.zeros(Npix), "U": np.zeros(Npix)}
    args = (pix, np.ones(Npix) * float(g["noise_temp"]), np.ones(Npix) * float(g["noise_pol"]), float(g["fwhm_deg"]),
            int(g["nside"]), int(g["L"]), Npix)
    bins = {"EE": g["bins_EE"], "BB": g["bins_BB"]}
    kw = dict(polarization=True, bins=bins, n_iter=T, nchains=4, seed=SEED, keep_history=True,
              br_samples={"lrange": (2, 12), "draws": True})
    if kind == "centered":
        smp = gibbs.CenteredGibbs(*args, **kw)
    else:
        smp = gibbs.ASIS(*args, {"EE": g["pv_EE"], "BB": g["pv_BB"]},
                         metropolis_blocks={"EE": g["blocks_EE"], "BB": g["blocks_BB"]}, all_sph=True, **kw)
    h = smp.run(init_of(g))[0]
    bank = smp.blackwell_rao_samples
    assert isinstance(bank, BlackwellRaoSamples) and bank.draws and bank.n == T
    col = gbr_columns(2, bank.bins, bank.mask)
    Jg = len(col["gcol"])
    Dl = bank.Dl.cpu().numpy()[:, :T]
    hist = {s: np.asarray(h[s]) for s in ("EE", "BB")}
    hist = {s: (v if v.ndim == 3 else v[:, None, :])[-T:] for s, v in hist.items()}        # [T, chains, nbins]
    maxbins = bank.maxbins
    for j, c in enumerate(bank.cols.cpu().numpy()):
        s = ("EE", "BB")[c // maxbins]
        assert np.array_equal(Dl[:, :, j], hist[s][:, :, c % maxbins].T), (s, c % maxbins)
    gbr = bank.gaussianize()
    G = GBR_POINTS
    assert gbr.G == G and gbr.n == 4 * T and gbr.Jg == Jg
    mu, cov = gbr.mu.cpu().numpy(), gbr.cov
    dg = np.diag(cov)
    print(f"  surface {kind}: |mu| max {np.abs(mu).max():.3f}, diag cov in [{dg.min():.3f}, {dg.max():.3f}]")
    assert np.all(np.abs(mu) < 0.5) and np.all(dg > 0.5) and np.all(dg < 2.0)
    # the whole fit restated from the downloaded bank
    good = ~np.isnan(bank.r.cpu().numpy()[:, :T])
    beta = bank.X.cpu().numpy()[:, :T][:, :, col["gcol"]] * col["half"]
    D = Dl[:, :, col["gcol"]]
    glo, gh = gbr.glo.cpu().numpy(), gbr.gh.cpu().numpy()
    logp, tmax, N = GB.marginals(beta, good, col["alpha"], glo, gh, G)
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    tx, tp = np.stack([x, sx], axis=-1), np.stack([logp.astype(np.float64), sp], axis=-1)
    xd, inside, _ = GB.transform(D, glo, gh, tx)
    assert inside[good].all()
    cnt, S1, S2 = GB.moments(np.where(good[:, :, None], xd, 0), good)
    N, rmu, rcov = GB.finish(cnt, S1, S2)
    med = np.median(D.reshape(-1, Jg), axis=0)
    th = med[None, :] * np.array([1.0, 1.1])[:, None]
    theory = {s: np.ones((2, len(bins[s]) - 1)) for s in ("EE", "BB")}
    for j, c in enumerate(col["tcol"]):
        theory[("EE", "BB")[c // maxbins]][:, c % maxbins] = th[:, j]
    res = gbr.loglike(theory)
    ref = GB.loglike(th, glo, gh, tx, tp, rmu.astype(np.float64), rcov.astype(np.float64))
    assert not res["outside"].any() and res["n"] == N
    lpb = GB.logp_bound(tmax, N, col["alpha"], glo, gh, G, N).max(axis=1)
    dx = 2.52 * lpb + EPS * (2.52 * (G + 8) + 8 * np.abs(x[np.isfinite(x)]).max())
    rc = rcov.astype(np.float64)
    amp = 1 + 4 * Jg * np.linalg.cond(rc)
    bound = GB.loglike_bound(ref, rc) + lpb.sum() + amp * ((np.abs(ref["grad_x"]) + np.abs(ref["x"]) + 1) * dx[None, :]).sum(axis=1)
    assert ratio(f"surface {kind} loglike", res["loglike"], ref["loglike"], bound) <= 1.0
