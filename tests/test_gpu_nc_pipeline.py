"""The pipelined schedule of multi-step native NC graphs (include/gibbs_capi.h
gs_nc_steps; option GS_NC_PIPE): sweep i + 1 on a side stream beside the
statistics finish and the MH of step i, two buffers of partials, the MH draws in
front of the finish (<= 4 chains: in a prologue launch).  No arithmetic
changes, so every comparison is bit for bit against the serial schedule
(GS_NC_PIPE=0, a fresh plan).

Shapes (those of tests/test_gpu_nc_raw.py): L 70 with 5 chains (two l tiles, a
partial tile, the throughput form, draws in the finish front); L 300 / N_side
128 with 2 chains (the latency form, draws in the prologue launch).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAPES = {"L70": (70, 32, 5), "L300": (300, 128, 2)}
NREF = 10                          # serial steps every case compares with


@functools.lru_cache(maxsize=None)
def _problem(F, shape):
    from gibbssampler_amd.problem import synthetic_problem
    L, nside, _ = SHAPES[shape]
    return synthetic_problem(L, nside, F, seed=9)


def _runner(F, shape, pipe, kind="noncentered", store=False):
    """A fresh, initialised runner whose plan is created with GS_NC_PIPE = pipe."""
    from gibbssampler_amd import _capi
    from gibbssampler_amd.samplers import BatchedRunner
    P = _problem(F, shape)
    with _capi.options(GS_NC_PIPE="1" if pipe else "0"):
        r = BatchedRunner(kind, P["lmax"], P["nside"], F, SHAPES[shape][2], P["bl"], P["noise_var"], P["bins"],
                          P["d_alm"], blocks=P["blocks"], proposal_variances=P["proposal_variances"], rng="native",
                          seed=23, store_skymap=store)
    r.init(P["dls_init"])
    return r


def _replays(r, K, R, adapt=False, **kw):
    """capture_steps(K) replayed R times: (D_l trace [K R, nchains, ...], accept trace)."""
    p = r.plan
    trace = p.zeros(K, p.nchains, p.nspec, p.maxbins)
    acc = p.zeros(K, p.nchains, max(p.nacc, 1), dtype=torch.int32)
    r.capture_steps(K, trace=trace, trace_capacity=K, accept_trace=acc, adapt=adapt, **kw)
    tr, ac = [], []
    for _ in range(R):
        r.step()
        tr.append(trace.clone())
        ac.append(acc.clone())
    torch.cuda.synchronize()
    return torch.cat(tr).cpu().numpy(), torch.cat(ac).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _serial(F, shape, kind="noncentered", store=False):
    """NREF steps of the serial schedule (5-step graph replayed twice), read-only."""
    r = _runner(F, shape, False, kind, store)
    out = _replays(r, 5, NREF // 5)
    assert not r.graph_pipelined
    for a in out:
        a.setflags(write=False)
    return out


CASES = [(3, "L70", 5), (3, "L70", 1), (3, "L70", 2), (3, "L300", 5), (3, "L300", 1), (3, "L300", 2),
         (2, "L70", 5)]


@pytest.mark.parametrize("F,shape,K", CASES)
def test_pipelined_replays_equal_serial(F, shape, K):
    """K = 5 replayed twice (odd: the second replay begins on the slot the first
    ended on; the replay boundary and the counter advance), K = 1 (nothing
    overlaps) and K = 2, against the first steps of the serial chain."""
    ref_tr, ref_ac = _serial(F, shape)
    r = _runner(F, shape, True)
    R = 2 if K == 5 else 3
    tr, ac = _replays(r, K, R)
    assert r.graph_pipelined
    np.testing.assert_array_equal(tr, ref_tr[:K * R])
    np.testing.assert_array_equal(ac, ref_ac[:K * R])
    np.testing.assert_array_equal(r.dl.cpu().numpy(), ref_tr[K * R - 1])
    assert r.iteration == K * R


@pytest.mark.parametrize("shape", ["L70", "L300"])
def test_adaptation_between_decide_and_next_draws(shape):
    """adapt=True: the scales written after step i's decide are the ones step
    i + 1's proposals (finish front / prologue launch) read."""
    out = []
    for pipe in (False, True):
        r = _runner(3, shape, pipe)
        r._adapt_enable(0.25)
        tr, ac = _replays(r, 6, 1, adapt=True)
        lam, n = r.plan.mh_scale_get()
        out.append((tr, ac, lam.cpu().numpy(), n.cpu().numpy()))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    assert np.all(out[1][3] == 6) and np.abs(out[1][2]).max() > 0.0


@pytest.mark.parametrize("shape", ["L70", "L300"])
def test_sweep_timing_on_the_sweeps_branch(shape):
    ref_tr, ref_ac = _serial(3, shape)
    r = _runner(3, shape, True)
    tr, ac = _replays(r, 5, 1, time_sweeps=True, time_every=2)
    total, count = r.plan.sweep_timing(False)
    assert count == 3 and total > 0.0
    np.testing.assert_array_equal(tr, ref_tr[:5])
    np.testing.assert_array_equal(ac, ref_ac[:5])


def test_two_captures_before_either_replays():
    """The benchmark's order: the warm-up graph and the timed graph are both
    captured on one plan (its side stream and events) before either replays."""
    ref_tr, _ = _serial(3, "L70")
    r = _runner(3, "L70", True)
    p = r.plan
    warm = r.capture_steps(3)
    trace = p.zeros(5, p.nchains, p.nspec, p.maxbins)
    r.capture_steps(5, trace=trace, trace_capacity=5, time_sweeps=True, time_every=2)
    warm.replay()
    r.iteration += 3
    r.step()
    torch.cuda.synchronize()
    total, count = p.sweep_timing(False)
    assert count == 3 and total > 0.0
    # the trace slot of iteration it is (it - 1) % 5
    got = trace.cpu().numpy()
    for it in range(4, 9):
        np.testing.assert_array_equal(got[(it - 1) % 5], ref_tr[it - 1])


def test_state_after_pipelined_replay_continues_serially():
    ref_tr, ref_ac = _serial(3, "L70")
    r = _runner(3, "L70", True)
    _replays(r, 5, 1)
    st = r.state_dict()
    s = _runner(3, "L70", False)
    s.load_state_dict(st)
    tr, ac = _replays(s, 5, 1)
    np.testing.assert_array_equal(tr, ref_tr[5:])
    np.testing.assert_array_equal(ac, ref_ac[5:])


@pytest.mark.parametrize("kind,store", [("noncentered", True), ("asis", False)])
def test_state_dependent_runners_keep_the_serial_schedule(kind, store):
    """A stored map and ASIS: the sweep or the operator depends on the state.
    Under GS_NC_PIPE=1 they capture without the pipeline and give their
    GS_NC_PIPE=0 results."""
    ref_tr, ref_ac = _serial(3, "L70", kind, store)
    r = _runner(3, "L70", True, kind, store)
    tr, ac = _replays(r, 5, 2)
    assert not r.graph_pipelined
    np.testing.assert_array_equal(tr, ref_tr)
    np.testing.assert_array_equal(ac, ref_ac)
    if store:
        # the stored map does not change the chain
        np.testing.assert_array_equal(tr, _serial(3, "L70")[0])
