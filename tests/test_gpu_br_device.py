"""GPU: the Blackwell-Rao sample bank's likelihood of theories that live on the
device (gs_brt.hip, engine.BlackwellRaoSamples.loglike_t / loglike_grad_t /
loglike_torch).

Bounds, derived (DESIGN.md 'Blackwell-Rao likelihood of device theories') and not
tuned.  With delta_k = (Ju + 16) 2^-52 T_k the evaluator's per-sample bound:
    tables   |d Y| <= 8 2^-52 |Y| entrywise (the kernel mirrors the host's rounded
             operations: 3 per entry at most, observed 0);  |d cst| <= (Ju + 16)
             2^-52 sum |terms| (the kernel adds in column order, the host with
             fsum; the device's log is within 1 ulp)
    loglike  |d loglike|, |d chain_loglike| <= 2 delta_k + n 2^-52 (r13's bound with
             the table rounding added);  |d neff| <= neff (8 delta_k + 2 n 2^-52)
    grad     r14's bound with 2 delta_k in place of delta_k:
             |d xbar_kj| <= (4 delta_k + (2 C n + 16) 2^-52) abar_kj,
             |d chain_weight| <= 4 delta_k + 2 C n 2^-52, grad through the chain rule
Largest |device - reference| / bound seen on an MI355X: see DESIGN.md."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _br_grad as G  # noqa: E402
from tests import _br_likelihood as R  # noqa: E402
from tests import _br_samples as B  # noqa: E402
from tests import test_gpu_br_grad as TG  # noqa: E402
from tests import test_gpu_br_samples as S  # noqa: E402
from tests.test_gpu_br_samples import bank_of  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def case(F, K, unbinned=False, one=False, T=7, C=3, lrange=None):
    return S.case(F, K, unbinned, one, T=T, C=C, lrange=lrange)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def keep(out):
    """A copy of a result that outlives the next call (the tensors are the bank's workspace)."""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def eqn(a, b):
    """torch.equal with NaN equal to NaN (mean_scale is NaN off the used set)."""
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


def same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in (keys or a)
               if not (torch.is_tensor(a[k]) and a[k].dtype.is_floating_point)) and \
        all(torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)) for k in (keys or a)
            if torch.is_tensor(a[k]) and a[k].dtype.is_floating_point)


# ---- 1. tables ---------------------------------------------------------------------------------------------
def device_tables(bank, theory):
    """(Y [K, Ju], cst [K], bad [K], guard) of gs_brt_tables on theory [K, nspec, maxbins] (numpy)."""
    from gibbssampler_amd import _capi as C
    tb = bank._brt_tables()
    K = theory.shape[0]
    D = dev(theory)
    buf = torch.full((K * bank.Jp + 8,), -3.0, dtype=torch.float64, device="cuda")   # Y and a guard behind it
    cst = torch.full((K,), -3.0, dtype=torch.float64, device="cuda")
    bad = torch.full((K,), 7, dtype=torch.int32, device="cuda")
    C.check(bank.lib.gs_brt_tables(C.ptr(D), K, bank.nspec, bank.maxbins, bank.Ju, C.ptr(bank.cols), C.ptr(bank.kind),
                                   C.ptr(tb["part"]), C.ptr(tb["cons"]), C.ptr(buf), C.ptr(cst), C.ptr(bad),
                                   C.stream_ptr()), "gs_brt_tables")
    torch.cuda.synchronize()
    return buf[:K * bank.Ju].view(K, bank.Ju).cpu().numpy(), cst.cpu().numpy(), bad.cpu().numpy(), buf[K * bank.Ju:]


def cst_terms(cs):
    """sum |terms| [K] of the tables' cst (the terms of engine.br_likelihood_tables)."""
    from tests.test_br_device_cpu import column_tables, tables_np
    return np.abs(tables_np(cs["theory"], column_tables(cs["F"], cs["bins"], cs["mask"]))[3]).sum(axis=1)


TABLE_CASES = [(2, 5, False, True, None), (2, 5, True, False, (2, 15)), (3, 5, False, False, None),
               (3, 70, False, False, None), (1, 5, True, False, None), (3, 5, True, False, None),
               (3, 5, False, False, (2, 5))]


@pytest.mark.parametrize("F,K,unbinned,one,lrange", TABLE_CASES)
def test_tables(F, K, unbinned, one, lrange):
    from gibbssampler_amd.engine import BlackwellRaoSamples
    cs = case(F, K, unbinned, one, lrange=lrange)
    tabs = cs["tables"]
    Ju = len(tabs["cols"])
    want_ju = {(2, True, None): 1, (2, False, (2, 15)): 28, (3, False, None): 28, (1, False, None): 63,
               (3, False, (2, 5)): 10}
    if (F, one, lrange) in want_ju and not (F == 3 and unbinned):
        assert Ju == want_ju[(F, one, lrange)]
    if F == 3 and unbinned:
        assert Ju == 252
    if F == 3:
        assert np.any(cs["theory"][1, 3] * cs["theory"][0, 3] < 0)          # a model of the opposite TE sign
        assert set(tabs["kind"]) == {0, 1, 2}
    bank = BlackwellRaoSamples(2, F, cs["bins"], cs["mask"], 4)
    Y, cst, bad, guard = device_tables(bank, cs["theory"])
    assert not bad.any()
    ry = float(np.max(np.abs(Y - tabs["Y"]) / (8 * EPS * np.abs(tabs["Y"]))))
    rc = float(np.max(np.abs(cst - tabs["cst"]) / ((Ju + 16) * EPS * cst_terms(cs))))
    print(f"  tables F {F} K {K} Ju {Ju}: max |device - host| / bound: Y {ry:.4f}, cst {rc:.4f}; "
          f"Y bit-equal {np.array_equal(Y, tabs['Y'])}")
    assert ry <= 1.0 and rc <= 1.0
    # Y is [K][Ju], the layout gs_brs_eval reads: nothing is written behind it (the bank's
    # padding columns Ju .. Jp - 1 are X's, and exactly 0 there)
    assert bool((guard == -3.0).all())
    if bank.Jp > bank.Ju:
        assert not bank_of(case(F, K, unbinned, one, lrange=lrange), cuts=(3, 4), cap=4).X[:, :, bank.Ju:].any()


def test_table_cases_cover_tiles():
    assert S.slice_rows() and 64 < 70 < 128                     # K = 70: two 64-model tiles, the second ragged
    ju = [len(case(F, K, u, o, lrange=lr)["tables"]["cols"]) for F, K, u, o, lr in TABLE_CASES]
    assert sorted(set(ju)) == [1, 10, 28, 63, 252]


# ---- 2. likelihood -----------------------------------------------------------------------------------------
def check_loglike(out, rows, cs, what, want=None, factor=1.0):
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    tables, maxbins = cs["tables"], cs["maxbins"]
    ref = B.loglike(flat, tables, maxbins)
    if want is None:
        want = ref
        assert out["n"] == T and np.array_equal(np.asarray(out["bad"]), ref["bad"]), what
    delta, slack = B.bounds(flat, tables, maxbins)
    bound = {"loglike": 2 * delta + slack, "chain_loglike": (2 * delta + slack)[None, :],
             "neff": ref["neff"] * (8 * delta + 2 * slack)}
    worst = 0.0
    for name in ("loglike", "chain_loglike", "neff"):
        got, w = np.asarray(out[name]), np.asarray(want[name])
        assert got.shape == w.shape and np.array_equal(np.isnan(got), np.isnan(w)), (what, name)
        ok = ~np.isnan(w)
        ratio = float(np.max((np.abs(got - w) / np.broadcast_to(factor * bound[name], w.shape))[ok])) if ok.any() else 0.0
        print(f"  {what} {name}: max |device - reference| / bound = {ratio:.4f} (Ju {len(tables['cols'])}, n {T})")
        worst = max(worst, ratio)
    assert worst <= 1.0, what


@pytest.mark.parametrize("F,K,unbinned,one,lrange", S.CASES)
def test_loglike(F, K, unbinned, one, lrange):
    cs = case(F, K, unbinned, one, lrange=lrange)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    out = bank.loglike_t(dev(cs["theory"]))
    assert set(out) == {"loglike", "chain_loglike", "neff", "n", "bad", "bad_model"}
    assert all(torch.is_tensor(out[k]) and out[k].is_cuda for k in out if k != "n")
    assert not out["bad_model"].any()
    check_loglike(host(out), cs["rows"], cs, f"F {F} K {K} Ju {bank.Ju}")


@functools.lru_cache(maxsize=None)
def long_case():
    return S.case(3, 5, T=2 * S.slice_rows() + 5)


def test_loglike_three_slices():
    cs = long_case()
    assert cs["rows"].shape[0] == 517
    bank = bank_of(cs, cap=64)
    check_loglike(host(bank.loglike_t(dev(cs["theory"]))), cs["rows"], cs, "three slices n 517")


def bad_rows(cs):
    bad = cs["rows"].copy()
    bad[2, 1, 2, 3] = 0.0
    bad[5, 2, 3, 6] = 2.0 * np.sqrt(bad[5, 2, 0, 6] * bad[5, 2, 1, 6])
    return bad


def test_loglike_bad_rows():
    cs = case(3, 5)
    bad = bad_rows(cs)
    bank = bank_of(cs, rows=bad, cuts=(3, 4), cap=4)
    out = host(bank.loglike_t(dev(cs["theory"])))
    assert np.array_equal(out["bad"], [0, 1, 1])
    check_loglike(out, bad, cs, "bad rows")


# ---- 3. gradient -------------------------------------------------------------------------------------------
def check_grad(out, rows, cs, what):
    """loglike_grad_t (host copies) against tests/_br_grad.py, r14's bound with 2 delta_k for delta_k."""
    from gibbssampler_amd.engine import br_likelihood_grad
    tables, theory, maxbins = cs["tables"], cs["theory"], cs["maxbins"]
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    ref = G.weights(flat, tables, maxbins)
    delta, _ = B.bounds(flat, tables, maxbins)
    bx, bw = G.xbar_bound(flat, tables, maxbins)
    bx, bw = bx + 2 * delta, bw + 2 * delta
    cols = np.asarray(tables["cols"], dtype=np.int64)
    K, Ju = ref["xbar"].shape
    ms = out["mean_scale"]
    assert ms.shape == theory.shape and out["chain_weight"].shape == (C, K) and out["grad"].shape == theory.shape, what
    off = np.ones(ms[0].size, dtype=bool)
    off[cols] = False
    assert np.isnan(ms.reshape(K, -1)[:, off]).all(), what
    dx = bx[:, None] * ref["abar"]
    rx = float(np.max(np.abs(ms.reshape(K, -1)[:, cols] - ref["xbar"]) / dx))
    rw = float(np.max(np.abs(out["chain_weight"] - ref["share"]) / bw[None, :]))
    want = br_likelihood_grad(cs["F"], cs["bins"], theory, cs["mask"], ref["xbar"])
    gb = TG.grad_bound(cs["F"], cs["bins"], theory, cs["mask"], cols, dx)
    use = gb > 0
    got = out["grad"]
    assert np.array_equal(got[~use], want[~use]) and not got[~use].any(), what     # exactly 0 off the used set
    rg = float(np.max(np.abs(got - want)[use] / gb[use]))
    print(f"  {what}: max |device - reference| / bound: xbar {rx:.4f}, chain_weight {rw:.4f}, grad {rg:.4f} "
          f"(Ju {Ju}, n {T}, C {C}, K {K})")
    assert rx <= 1.0 and rw <= 1.0 and rg <= 1.0, what
    return gb, bx, ref


def check_routes(bank, cs, rows, out, what):
    """The device route and the host route on the same inputs: within the sum of their two bounds."""
    T, C = rows.shape[:2]
    flat = rows.reshape(T, C, -1)
    h = bank.loglike_grad(cs["theory"])
    delta, slack = B.bounds(flat, cs["tables"], cs["maxbins"])
    assert np.all(np.abs(out["loglike"] - h["loglike"]) <= (delta + slack) + (2 * delta + slack))
    bx, _ = G.xbar_bound(flat, cs["tables"], cs["maxbins"])
    ref = G.weights(flat, cs["tables"], cs["maxbins"])
    cols = np.asarray(cs["tables"]["cols"], dtype=np.int64)
    gb = TG.grad_bound(cs["F"], cs["bins"], cs["theory"], cs["mask"], cols, ((bx + 2 * delta) + bx)[:, None] * ref["abar"])
    from gibbssampler_amd.engine import SPECTRA
    hg = np.zeros_like(out["grad"])
    for k, s in enumerate(SPECTRA[cs["F"]]):
        hg[:, k, :h["grad"][s].shape[1]] = h["grad"][s]
    d = np.abs(out["grad"] - hg)
    assert np.all(d <= gb), what
    print(f"  {what}: device route against host route: max |d grad| / bound = "
          f"{float(np.max(d[gb > 0] / gb[gb > 0])):.4f}, grad bit-equal {np.array_equal(out['grad'], hg)}, "
          f"loglike bit-equal {np.array_equal(out['loglike'], h['loglike'])}")


@pytest.mark.parametrize("F,K,unbinned,one,lrange", S.CASES)
def test_grad(F, K, unbinned, one, lrange):
    cs = case(F, K, unbinned, one, lrange=lrange)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th = dev(cs["theory"])
    a = keep(bank.loglike_t(th))
    res = bank.loglike_grad_t(th)
    assert set(res) == set(a) | {"grad", "mean_scale", "chain_weight"} and same(a, res, list(a))
    out = host(res)
    check_loglike(out, cs["rows"], cs, f"F {F} K {K} Ju {bank.Ju}")
    check_grad(out, cs["rows"], cs, f"F {F} K {K} Ju {bank.Ju}")
    check_routes(bank, cs, cs["rows"], out, f"F {F} K {K} Ju {bank.Ju}")


def test_grad_two_model_tiles():
    cs = case(3, 70)
    out = host(bank_of(cs, cuts=(3, 4), cap=4).loglike_grad_t(dev(cs["theory"])))
    check_grad(out, cs["rows"], cs, "K 70")


def test_grad_two_column_tiles_and_three_blocks():
    gr, _, ct = TG.grad_info()
    cs = case(3, 5, True)
    assert len(cs["tables"]["cols"]) > ct                       # two column tiles
    check_grad(host(bank_of(cs, cuts=(3, 4), cap=4).loglike_grad_t(dev(cs["theory"]))), cs["rows"], cs, "Ju 252")
    cl = case(3, 5, T=2 * gr + 5, C=2)
    assert cl["rows"].shape[0] == 2053
    bank = bank_of(cl, cap=64)
    out = host(bank.loglike_grad_t(dev(cl["theory"])))
    check_grad(out, cl["rows"], cl, "three blocks n 2053")
    check_routes(bank, cl, cl["rows"], out, "three blocks n 2053")


def test_grad_bad_rows():
    cs = case(3, 5)
    bad = bad_rows(cs)
    out = host(bank_of(cs, rows=bad, cuts=(3, 4), cap=4).loglike_grad_t(dev(cs["theory"])))
    check_grad(out, bad, cs, "bad rows")


# ---- 4. independence ---------------------------------------------------------------------------------------
def test_independence():
    from gibbssampler_amd.engine import SPECTRA
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th = dev(cs["theory"])
    five = keep(bank.loglike_grad_t(th))
    one = keep(bank.loglike_grad_t(th[4:5].clone()))
    for k in ("loglike", "neff", "grad", "mean_scale"):
        assert eqn(one[k][0], five[k][4]), k
    for k in ("chain_loglike", "chain_weight"):
        assert torch.equal(one[k][:, 0], five[k][:, 4]), k
    # a dict theory and its packed tensor
    d = {s: th[:, k, :len(cs["bins"][s]) - 1].clone() for k, s in enumerate(SPECTRA[3])}
    packed = bank.fiducial.unsqueeze(0).repeat(5, 1, 1)
    for k, s in enumerate(SPECTRA[3]):
        packed[:, k, :d[s].shape[1]] = d[s]
    a, b = keep(bank.loglike_grad_t(d)), keep(bank.loglike_grad_t(packed))
    assert same(a, b) and same(a, five)
    # a spectrum left out takes the fiducial: filled in by hand it is the same
    bank.fiducial[2].copy_(th[2, 2])                            # model 2's BB as the fiducial BB
    part = {s: v for s, v in d.items() if s != "BB"}
    full = dict(part, BB=bank.fiducial[2, :d["BB"].shape[1]].unsqueeze(0).repeat(5, 1))
    a, b = keep(bank.loglike_grad_t(part)), keep(bank.loglike_grad_t(full))
    assert same(a, b) and torch.equal(a["loglike"][2], five["loglike"][2]) and not torch.equal(a["loglike"], five["loglike"])
    la, lb = keep(bank.loglike_t(part)), keep(bank.loglike_t(full))
    assert same(la, lb) and same(la, a, list(la))


# ---- 5. bad models -----------------------------------------------------------------------------------------
def test_bad_models():
    cs = case(3, 3)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th = cs["theory"].copy()
    th[0, 2, 3] = 0.0                                            # a BB bin that is not positive
    th[1, 3, 4] = 1.01 * np.sqrt(th[1, 0, 4] * th[1, 1, 4])      # TE^2 > TT EE
    with pytest.raises(ValueError):
        bank.loglike(th)                                         # the host route raises
    t = dev(th)
    out = keep(bank.loglike_grad_t(t))
    torch.cuda.synchronize()
    assert out["bad_model"].tolist() == [1, 1, 0]
    used = torch.from_numpy(cs["mask"]).cuda()
    for k in (0, 1):
        assert bool(torch.isnan(out["loglike"][k])) and bool(torch.isnan(out["chain_loglike"][:, k]).all())
        assert bool(torch.isnan(out["grad"][k][used]).all()) and not out["grad"][k][~used].any()
    solo = keep(bank.loglike_grad_t(t[2:3].clone()))
    assert solo["bad_model"].tolist() == [0] and bool(torch.isfinite(solo["loglike"]).all())
    for k in ("loglike", "neff", "grad", "mean_scale"):
        assert eqn(solo[k][0], out[k][2]), k
    for k in ("chain_loglike", "chain_weight"):
        assert torch.equal(solo[k][:, 0], out[k][:, 2]), k
    ll = keep(bank.loglike_t(t))
    assert ll["bad_model"].tolist() == [1, 1, 0] and same(ll, out, list(ll))


# ---- 6. no host round trip ---------------------------------------------------------------------------------
def test_graph_capture():
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th5 = dev(cs["theory"])
    graphs = {}
    for K in (1, 5):
        static = th5[:K].clone()
        bank.loglike_grad_t(static)                              # the warm-up call: the workspace of this K
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                res = bank.loglike_grad_t(static)
        torch.cuda.current_stream().wait_stream(side)
        graphs[K] = (g, static, res)
    for rep in range(3):
        for K in (1, 5):
            g, static, res = graphs[K]
            new = th5[(rep + 1) % 5:(rep + 1) % 5 + 1] if K == 1 else th5 * (1.0 + 0.01 * (rep + 1))
            static.copy_(new)
            g.replay()
            torch.cuda.synchronize()
            got = keep(res)
            for k in ("loglike", "grad"):                        # poison the workspace: the eager call rewrites it
                res[k].fill_(-1.0)
            want = keep(bank.loglike_grad_t(new.clone()))
            assert same(got, want), (K, rep)
            assert bool(torch.isfinite(got["loglike"]).all()) and bool((got["grad"] != 0).any())


# ---- 7. autograd -------------------------------------------------------------------------------------------
def test_autograd_is_the_gradient_pass():
    cs = case(3, 5)
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th = dev(cs["theory"]).requires_grad_(True)
    want = keep(bank.loglike_grad_t(th))
    ll = bank.loglike_torch(th)
    assert ll.requires_grad and torch.equal(ll.detach(), want["loglike"])
    g, = torch.autograd.grad(ll.sum(), th)
    assert torch.equal(g, want["grad"])
    w = torch.tensor([2.0, -0.5, 0.0, 3.0, 1.0], dtype=torch.float64, device="cuda")
    g2, = torch.autograd.grad((bank.loglike_torch(th) * w).sum(), th)
    assert torch.equal(g2, w[:, None, None] * want["grad"])
    # no gradient asked: the loglike_t route, a plain tensor
    plain = bank.loglike_torch(th.detach())
    assert not plain.requires_grad and torch.equal(plain, want["loglike"])
    assert "grad" not in bank._brt_tables()["ws"].get(3, {}) and "grad" in bank._brt_tables()["ws"][5]
    bank.loglike_torch(th.detach()[:3].clone())
    assert "grad" not in bank._brt_tables()["ws"][3]             # K = 3 has only ever run loglike_t
    # a double backward raises and names loglike_hess
    g3, = torch.autograd.grad(bank.loglike_torch(th).sum(), th, create_graph=False)
    with pytest.raises(RuntimeError, match="loglike_hess"):
        torch.autograd.grad(bank.loglike_torch(th).sum(), th, create_graph=True)


def test_autograd_central_differences():
    """r14's rule: grad D against central differences of the longdouble restatement in
    log D, h = (2^-52 T_k)^(1/3), within 10 (h^2 + 2^-52 T_k / h) of the terms' magnitudes."""
    from tests.test_br_grad_cpu import magnitudes
    cs = case(3, 3, lrange=(2, 5))
    rows, theory, mask, bins = cs["rows"], cs["theory"], cs["mask"], cs["bins"]
    from gibbssampler_amd.engine import br_likelihood_tables
    bank = bank_of(cs, cuts=(3, 4), cap=4)
    th = dev(theory).requires_grad_(True)
    g, = torch.autograd.grad(bank.loglike_torch(th).sum(), th)
    g = g.cpu().numpy()
    flat = rows.reshape(7, 3, -1)
    ref = G.weights(flat, cs["tables"], cs["maxbins"])
    Tk = R.term_bound(flat, cs["tables"], cs["maxbins"])
    h = (EPS * Tk) ** (1.0 / 3.0)
    A = magnitudes(3, bins, theory, mask, ref["abar"])
    used = np.zeros(mask.size, dtype=bool)
    used[cs["tables"]["cols"]] = True
    worst = 0.0
    for sp, b in zip(*np.nonzero(used.reshape(mask.shape))):
        for k in range(3):
            f = []
            for sgn in (1.0, -1.0):
                t1 = theory[k:k + 1].copy()
                t1[0, sp, b] *= 1.0 + sgn * h[k]
                f.append(G.weights(flat, br_likelihood_tables(3, bins, t1, mask), cs["maxbins"])["loglike_ld"][0])
            quot = float((f[0] - f[1]) / (2 * np.longdouble(h[k])))
            bound = 10.0 * (h[k] ** 2 + EPS * Tk[k] / h[k]) * A[k, sp, b]
            worst = max(worst, abs(g[k, sp, b] * theory[k, sp, b] - quot) / bound)
    print(f"  autograd against central differences: max / bound = {worst:.4f}")
    assert worst <= 1.0


def lbfgs_problem():
    """F = 2, Ju = 10 (l = 2 .. 6 unbinned), 4 chains x 64 rows; the start 0.8 x the
    fiducial (the mean scale over n_b / 2 of each bin); the CPU restatement's optimum."""
    cs = case(2, 1, True, T=64, C=4, lrange=(2, 6))
    rows, mask, bins = cs["rows"], cs["mask"], cs["bins"]
    assert len(cs["tables"]["cols"]) == 10
    from gibbssampler_amd.engine import br_likelihood_tables
    from tests.test_br_device_cpu import column_tables
    ct = column_tables(2, bins, mask)
    cols, hb = ct["cols"], ct["cons"][0]
    flat = rows.reshape(64, 4, -1)
    fid = flat.reshape(256, -1)[:, cols].mean(axis=0) / hb
    def theory_of(v):
        t = np.ones((1, mask.size))
        t[0, cols] = v
        return t.reshape((1,) + mask.shape)

    # CPU beforehand: the fixed point D = xbar(D) / (n_b / 2) (an EM step: monotone) from the start
    # (all bins inverse-Gamma: Y = 1 / D, t = r - x . Y, the restatement's weights in longdouble)
    LD = np.longdouble
    parts = [R.row_parts(flat[i, c], cs["tables"], cs["maxbins"]) for i in range(64) for c in range(4)]
    assert all(p[0] for p in parts)
    x = np.stack([p[1] for p in parts]).astype(LD)
    r = np.stack([np.sum(np.asarray(cs["tables"]["coef"]).astype(LD) * p[2].astype(LD)) for p in parts])
    v = (0.8 * fid).astype(LD)
    done = False
    for _ in range(5000):
        t = r - x @ (1.0 / v)
        w = np.exp(t - t.max())
        new = (w @ x) / w.sum() / hb
        done = float(np.max(np.abs(new / v - 1.0))) < 1e-15
        v = new
        if done:
            break
    assert done, "the CPU restatement does not converge from this start"
    v = v.astype(np.float64)
    tb = br_likelihood_tables(2, bins, theory_of(v), mask)
    end = B.loglike(flat, tb, cs["maxbins"])
    assert end["neff"][0] >= 4.0
    delta, slack = B.bounds(flat, tb, cs["maxbins"])
    bx, _ = G.xbar_bound(flat, tb, cs["maxbins"])
    w = G.weights(flat, tb, cs["maxbins"])
    gd_bound = (bx + 2 * delta)[0] * w["abar"][0] / v            # the error bound of grad D at the optimum
    return cs, cols, fid, v, float(end["loglike"][0]), gd_bound, float(2 * delta[0] + slack)


def test_lbfgs_finds_the_maximum():
    """Twenty torch.optim.LBFGS steps (torch's default: no line search, 20 iterations
    each, stopping at max |grad D| <= 10 x the gradient's error bound) in u = log D.
    A line search on the computed loglike cannot go below |d u| ~ sqrt(2^-52 |loglike|)
    ~ 3e-8 (seen: strong_wolfe stalls at max |grad D| = 3.2e-8), so the steps are
    judged by their gradients.  A step that moved u must raise the loglike strictly
    wherever the computed values can tell: when its first-order gain |g . du| / 2
    exceeds the loglike's own bound 2 delta_k + n 2^-52; below that the two values
    agree within that bound."""
    cs, cols, fid, vopt, llopt, gd_bound, ll_bound = lbfgs_problem()
    bank = bank_of(cs, cap=64)
    nsb = cs["mask"].size
    idx = torch.from_numpy(cols).cuda()
    u = torch.log(dev(0.8 * fid)).requires_grad_(True)
    base = torch.ones(nsb, dtype=torch.float64, device="cuda")

    def theory_of(u):
        return base.index_put((idx,), torch.exp(u)).reshape((1,) + cs["mask"].shape)

    tol = 10.0 * float(gd_bound.min())
    opt = torch.optim.LBFGS([u], lr=1.0, max_iter=20, history_size=10, tolerance_grad=tol, tolerance_change=0.0)

    def closure():
        opt.zero_grad()
        loss = -bank.loglike_torch(theory_of(u)).sum()
        loss.backward()
        return loss

    trail = [float(bank.loglike_t(theory_of(u.detach()))["loglike"][0])]
    moved = 0
    for step in range(20):
        before = u.detach().clone()
        g0 = bank.loglike_grad_t(theory_of(before))["grad"].reshape(-1)[idx] * torch.exp(before)
        opt.step(closure)
        ll = float(bank.loglike_t(theory_of(u.detach()))["loglike"][0])
        if not torch.equal(before, u.detach()):                  # an accepted step
            moved += 1
            gain = 0.5 * abs(float((g0 * (u.detach() - before)).sum()))
            print(f"  L-BFGS step {step}: loglike {trail[-1]!r} -> {ll!r}, first-order gain {gain:.3e}, bound {ll_bound:.3e}")
            if gain > ll_bound:
                assert ll > trail[-1], (step, ll, trail[-1])
            else:
                assert abs(ll - trail[-1]) <= ll_bound, (step, ll, trail[-1])
        trail.append(ll)
    assert moved >= 1
    out = bank.loglike_grad_t(theory_of(u.detach()))
    gd = (out["grad"].reshape(-1)[idx] * torch.exp(u.detach())).cpu().numpy()
    ratio = float(np.max(np.abs(gd) / gd_bound))
    print(f"  L-BFGS: loglike {trail[0]:.6f} -> {trail[-1]:.6f} (CPU optimum {llopt:.6f}); max |grad D| = "
          f"{np.max(np.abs(gd)):.3e}, / error bound = {ratio:.2f}; max |D / D_cpu - 1| = "
          f"{float(np.max(np.abs(np.exp(u.detach().cpu().numpy()) / vopt - 1.0))):.2e}")
    assert ratio <= 100.0, f"max |grad D| / bound = {ratio}"
    assert float(out["neff"][0]) >= 4.0


# ---- 8. the run surface ------------------------------------------------------------------------------------
def test_run_surface(tmp_path):
    from gibbssampler_amd import gibbs
    from gibbssampler_amd.engine import SPECTRA, BlackwellRaoSamples
    from gibbssampler_amd.samplers import br_theory
    model, init, theory = TG._problem()
    d = {k: model.d_alm[i] for i, k in enumerate(("TT", "EE", "BB"))}
    fwhm = max(0.5, 180.0 / model.L * 2)
    args = (d, model.noise_var[0], model.noise_var[-1], fwhm, model.nside, model.L, 12 * model.nside ** 2)
    smp = gibbs.CenteredGibbs(*args, polarization=True, bins=model.bins, n_iter=40, all_sph=True, nchains=2,
                              seed=S.SEED, fields="TEB", br_samples={"lrange": (2, 12)}, keep_scales=True)
    smp.run(init)
    bank = smp.blackwell_rao_samples
    th = br_theory("test", theory, 3, bank.bins, bank.mask)
    t = dev(th)
    a = keep(bank.loglike_t(t))
    assert torch.equal(smp.blackwell_rao_samples.loglike_torch(t), a["loglike"]) and a["n"] == 40
    # against the restatement of the kept scale history, and against loglike (the sum of the two routes' bounds)
    hs = np.full((40, 2, bank.nspec, bank.maxbins), np.nan)
    for k, s in enumerate(model.spectra):
        hs[:, :, k, :model.nbins(s)] = smp.h_scales[s]
    cs = {"tables": bank.tables(theory), "maxbins": bank.maxbins}
    check_loglike(host(a), hs, cs, "run surface")
    h = bank.loglike(theory)
    delta, slack = B.bounds(hs.reshape(40, 2, -1), cs["tables"], bank.maxbins)
    for k in ("loglike", "chain_loglike"):
        assert np.all(np.abs(a[k].cpu().numpy() - h[k]) <= (delta + slack) + (2 * delta + slack)), k
    assert np.array_equal(a["bad"].cpu().numpy(), h["bad"])
    # the dict of device tensors is the packed tensor
    dd = {s: dev(np.atleast_2d(theory[s])) for s in SPECTRA[3]}
    assert same(keep(bank.loglike_t(dd)), a)
    g = keep(bank.loglike_grad_t(t))
    path = os.path.join(tmp_path, "bank.npz")
    bank.save(path)
    back = BlackwellRaoSamples.load(path)
    assert same(keep(back.loglike_grad_t(t)), g) and torch.equal(back.loglike_torch(t), a["loglike"])


def test_gather():
    cs = case(3, 5, C=4)
    tables = cs["tables"]
    th = dev(cs["theory"])
    whole = bank_of(cs, cuts=(3, 4), cap=4)
    lo = bank_of(cs, rows=cs["rows"][:, :2], cuts=(3, 4), cap=4)
    hi = bank_of(cs, rows=cs["rows"][:, 2:], cuts=(3, 4), cap=4)
    hi_fields = hi.fields(hi.evaluate(tables["Y"]))
    hi_num = hi.grad_numerators(tables["Y"], TG.mref_of(whole, tables))
    calls = []

    def gather(t, dim=0):
        calls.append((tuple(t.shape), dim))
        return torch.cat([t, hi_fields if dim == 1 else hi_num], dim=dim)

    want = keep(whole.loglike_grad_t(th))
    got = keep(lo.loglike_grad_t(th, gather))
    assert calls == [((3, 2, 5), 1), ((2, 5, lo.Jp), 0)]
    for k in ("loglike", "chain_loglike", "neff", "grad", "mean_scale", "chain_weight"):
        assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(want[k], nan=-7.0)), k
    assert tuple(got["chain_weight"].shape) == (4, 5)
    calls.clear()
    ll = keep(lo.loglike_t(th, gather))
    assert calls == [((3, 2, 5), 1)] and torch.equal(ll["loglike"], want["loglike"])
    assert torch.equal(ll["chain_loglike"], want["chain_loglike"])
