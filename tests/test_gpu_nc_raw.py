"""Raw-moment statistics of native-draw NC steps (include/gibbs_capi.h
gs_data_moments): the sweep accumulates sum z z^T and sum d z^T, the statistics
finish applies the operator of the chain's D_l to them and to sum d d^T.

Shapes: L 70 with 5 chains (two l tiles, a partial tile with l < 0 lanes,
diagonal and off-diagonal blocks, the throughput form without a parameter
table); L 300 / N_side 128 with 2 chains (the latency form, and the throughput
form under GS_SWEEP_THROUGHPUT=1).

Tolerance of the statistic rows against the oracle: that of
tests/test_gpu_parity.py::test_native_cr_sweep_matches_oracle (rtol 1e-10,
atol 1e-12 of the largest row entry).

Zero bins.  The NC operator of a zero D_l is P = 0, Q = I (the draw is z
itself), so the statistics there are sum z z^T and sum d z^T, not zero.  What
must hold exactly is that the P terms vanish: at those l the raw-moment rows
equal, bit for bit, the rows of the direct accumulation of s = 0 d + 1 z
(GS_NC_RAW=0), which adds the same products in the same order.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import harmonic as H  # noqa: E402
from tests._util import stats_rows, make_problem  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x0BAD_5EED_1234
IT = 6
CHAIN0 = 3
ZERO_BB = slice(5, 9)          # BB bins set to zero in the F >= 2 starts


def _plan(m, nchains, chain0=CHAIN0):
    from gibbssampler_amd.engine import GibbsPlan
    return GibbsPlan(m.L, m.nside, m.nfields, nchains, m.bl, m.noise_var, m.bins, blocks=m.blocks,
                     proposal_variances=m.proposal_variances, chain0=chain0)


def _starts(m, init, nch):
    """One start per chain (the operator is per chain), BB zero in a few bins."""
    out = []
    for c in range(nch):
        d = {s: np.array(v, dtype=np.float64) * (1.0 + 0.05 * c) for s, v in init.items()}
        if "BB" in d:
            d["BB"][ZERO_BB] = 0.0
        out.append(d)
    return out


def _oracle_rows(m, starts, d, nch, chain0=CHAIN0, seed=SEED, it=IT):
    rows = []
    for c in range(nch):
        M, Lc = H.noncentered_params(m, m.unfold(starts[c]))
        z = np.stack([H.cr_normals(seed, chain0 + c, it, 0, f, m.L) for f in range(m.nfields)])
        rows.append(stats_rows(m.nfields, H.sweep_stats(m, H.cr_apply(m, M, Lc, d, z), d)))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _case(F, L, nside, nch):
    m, init = make_problem(L, nside, F, seed=21)
    starts = _starts(m, init, nch)
    ref = _oracle_rows(m, starts, m.d_alm, nch)
    ref.setflags(write=False)
    return m, starts, ref


def _device_rows(m, starts, nch, d_host=None, store=False):
    p = _plan(m, nch)
    d = p.data_tensor(m.d_alm if d_host is None else d_host)
    dl = p.dl_tensor(starts)
    s = p.zeros(nch, p.F, p.NR) if store else None
    p.nc_prologue(dl, seed=SEED, iteration=IT)
    p.nc_sweep(d, dl, s, seed=SEED, iteration=IT)
    rows = p.nc_stats().cpu().numpy()
    return rows, (None if s is None else s.cpu().numpy())


def _zero_columns(m, F):
    """(row indices, l) pairs where the start D_l is zero."""
    out = [(list(range(2 * F if F != 3 else 8)), np.array([0, 1]))]
    if F >= 2:
        b = m.bins["BB"]
        ls = np.arange(b[ZERO_BB.start], b[ZERO_BB.stop])
        out.append(([1, 3] if F == 2 else [2, 7], ls))
    return out


@pytest.mark.parametrize("F", [1, 2, 3])
@pytest.mark.parametrize("L,nside,nch,throughput", [(70, 32, 5, False), (300, 128, 2, False), (300, 128, 2, True)])
def test_raw_stats_match_oracle(gsopt, F, L, nside, nch, throughput):
    m, starts, ref = _case(F, L, nside, nch)
    if throughput:
        gsopt.setenv("GS_SWEEP_THROUGHPUT", "1")
    got, _ = _device_rows(m, starts, nch)
    for c in range(nch):
        np.testing.assert_allclose(got[c], ref[c], rtol=1e-10, atol=1e-12 * np.abs(ref[c]).max(), err_msg=f"chain {c}")
    # the stored-map variant accumulates the same raw sums: the same bits, and the map is the oracle's
    got_s, s = _device_rows(m, starts, nch, store=True)
    np.testing.assert_array_equal(got_s, got)
    M, Lc = H.noncentered_params(m, m.unfold(starts[0]))
    z = np.stack([H.cr_normals(SEED, CHAIN0, IT, 0, f, L) for f in range(F)])
    s_ref = H.cr_apply(m, M, Lc, m.d_alm, z)
    np.testing.assert_allclose(s[0], s_ref, rtol=1e-10, atol=1e-12 * np.abs(s_ref).max())
    # zero D_l: P = 0, Q = I -- exactly the direct accumulation of s = z
    gsopt.setenv("GS_NC_RAW", "0")
    legacy, _ = _device_rows(m, starts, nch)
    for c in range(nch):
        np.testing.assert_allclose(legacy[c], ref[c], rtol=1e-10, atol=1e-12 * np.abs(ref[c]).max())
    for rows, ls in _zero_columns(m, F):
        np.testing.assert_array_equal(got[:, rows][:, :, ls], legacy[:, rows][:, :, ls])
        assert np.all(np.isfinite(got[:, rows][:, :, ls]))


def test_moments_follow_the_data_tensor():
    """Two data tensors on one plan: each sweep's statistics belong to its own
    tensor (a new pointer recomputes the moments; an in-place change needs
    data_moments again)."""
    F, L, nside, nch = 3, 70, 32, 2
    m, starts, _ = _case(F, L, nside, 5)
    starts = starts[:nch]
    rng = np.random.RandomState(4)
    d1 = np.array(m.d_alm)
    d2 = 1.5 * d1 + rng.normal(size=d1.shape) * np.abs(d1).mean()
    d3 = 0.5 * d1 - rng.normal(size=d1.shape) * np.abs(d1).mean()
    p = _plan(m, nch)
    dl = p.dl_tensor(starts)
    t1, t2 = p.data_tensor(d1), p.data_tensor(d2)

    def rows(t):
        p.nc_prologue(dl, seed=SEED, iteration=IT)
        p.nc_sweep(t, dl, None, seed=SEED, iteration=IT)
        return p.nc_stats().cpu().numpy()

    def check(got, d):
        ref = _oracle_rows(m, starts, d, nch)
        for c in range(nch):
            np.testing.assert_allclose(got[c], ref[c], rtol=1e-10, atol=1e-12 * np.abs(ref[c]).max())

    p.data_moments(t1)
    check(rows(t1), d1)
    check(rows(t2), d2)                 # another tensor: the sweep recomputes the moments
    check(rows(t1), d1)
    t1.copy_(torch.from_numpy(d3))      # the same buffer, new values: the explicit call
    p.data_moments(t1)
    check(rows(t1), d3)


def _runner(P, F, nch, store):
    from gibbssampler_amd.samplers import BatchedRunner
    return BatchedRunner("noncentered", P["lmax"], P["nside"], F, nch, P["bl"], P["noise_var"], P["bins"], P["d_alm"],
                         blocks=P["blocks"], proposal_variances=P["proposal_variances"], rng="native", seed=23,
                         store_skymap=store)


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("L,nside,nch", [(70, 32, 5), (300, 128, 2)])
def test_captured_steps_equal_eager(F, L, nside, nch):
    """A captured 5-step graph replayed twice == 10 eager steps, bit for bit: the
    D_l trace, the per-step accept flags and the final D_l; with and without
    the stored map (which must not change the chain)."""
    from gibbssampler_amd.problem import synthetic_problem
    P = synthetic_problem(L, nside, F, seed=9)
    K, R = 5, 2
    out = {}
    for store in (False, True):
        e = _runner(P, F, nch, store)
        e.init(P["dls_init"])
        tr, ac = [], []
        for _ in range(K * R):
            e.step()
            tr.append(e.dl.clone())
            ac.append(e.accept.clone())
        eager = (torch.stack(tr).cpu().numpy(), torch.stack(ac).cpu().numpy())
        g = _runner(P, F, nch, store)
        g.init(P["dls_init"])
        p = g.plan
        trace = p.zeros(K, nch, p.nspec, p.maxbins)
        acc = p.zeros(K, nch, max(p.nacc, 1), dtype=torch.int32)
        g.capture_steps(K, trace=trace, trace_capacity=K, accept_trace=acc)
        tr, ac = [], []
        for _ in range(R):
            g.step()
            tr.append(trace.clone())
            ac.append(acc.clone())
        graph = (torch.cat(tr).cpu().numpy(), torch.cat(ac).cpu().numpy())
        np.testing.assert_array_equal(graph[0], eager[0])
        np.testing.assert_array_equal(graph[1], eager[1])
        np.testing.assert_array_equal(g.dl.cpu().numpy(), eager[0][-1])
        assert g.iteration == K * R
        out[store] = eager
    np.testing.assert_array_equal(out[True][0], out[False][0])
    np.testing.assert_array_equal(out[True][1], out[False][1])


def test_sweep_timing_in_captured_steps():
    """time_every = 1: every captured step's sweep is bracketed once."""
    from gibbssampler_amd.problem import synthetic_problem
    P = synthetic_problem(70, 32, 3, seed=9)
    r = _runner(P, 3, 5, False)
    r.init(P["dls_init"])
    steps = 4
    r.capture_steps(steps, time_sweeps=True, time_every=1)
    r.step()
    torch.cuda.synchronize()
    total, count = r.plan.sweep_timing(False)
    assert count == steps
    assert total > 0.0
