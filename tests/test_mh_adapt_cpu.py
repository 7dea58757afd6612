"""Warm-up adaptation of the NC Metropolis proposal scales: what needs no GPU.

  * the test-side recursion (tests/_mh_adapt.py) on hand-made flag sequences;
  * argument validation of run(n_warmup=...) for the centered sampler and
    replayed runs;
  * states written before the adaptation existed load as "not adapting";
  * the variances handed back (tuned_variances) and the config helper.
"""
import numpy as np
import pytest

from tests import _mh_adapt as A


def test_all_accept_rises_all_reject_falls_and_n_counts():
    T, n_mh = 30, 2
    up = np.ones((T, 3 * n_mh), dtype=np.int64)
    lam, n = A.recursion(up, n_mh)
    assert np.all(n == T)
    want = sum(k ** -0.6 * 0.75 for k in range(1, T + 1))
    np.testing.assert_allclose(lam, want, rtol=1e-13)
    lam_prev = 0.0
    for t in range(1, 6):                                   # monotone from the first step
        lam_t, _ = A.recursion(up[:t], n_mh)
        assert np.all(lam_t > lam_prev)
        lam_prev = lam_t.max()
    down, n2 = A.recursion(np.zeros((T, 3 * n_mh), dtype=np.int64), n_mh)
    assert np.all(n2 == T)
    np.testing.assert_allclose(down, -sum(k ** -0.6 * 0.25 for k in range(1, T + 1)), rtol=1e-13)


def test_block_mean_of_attempts_and_fixed_point():
    # one of four attempts accepted: abar = a* = 0.25, the scale does not move
    fl = np.tile(np.array([1, 0, 0, 0, 0, 0, 1, 1]), (10, 1))
    np.testing.assert_array_equal(A.block_means(fl, 4), np.tile([0.25, 0.5], (10, 1)))
    lam, n = A.recursion(fl, 4)
    assert lam[0] == 0.0 and lam[1] > 0.0 and np.all(n == 10)


def test_clamp_is_hit_and_holds():
    lam, n = A.recursion(np.ones((200, 1), dtype=np.int64), 1, lam_max=3.0)
    assert lam[0] == 3.0 and n[0] == 200
    lam, _ = A.recursion(np.zeros((2000, 1), dtype=np.int64), 1, lam_max=3.0)
    assert lam[0] == -3.0
    lam, n = A.rm_update(np.array([19.9]), np.array([0]), np.array([1.0]))
    assert lam[0] == 20.0 and n[0] == 1


def test_expand_sd_blocks_clipped_and_per_chain_shape():
    m, _ = A.small_problem(2, bb_blocks="wide")
    lay = A.block_layout(m)
    assert [s for s, _, _ in lay] == ["EE", "BB"] and lay[1][1:] == (1, 4)
    nblk = 5
    lam = np.arange(1, nblk + 1) * 0.1
    sd = A.expand_sd(m, lam)
    sd0 = {s: np.sqrt(m.proposal_variances[s]) for s in m.spectra}
    np.testing.assert_array_equal(sd["EE"], sd0["EE"] * np.exp(0.1))
    nb = m.nbins("BB")
    edges = [2, 7, 12, 20, nb]                              # the last edge clipped by nbins
    for k in range(4):
        lo, hi = edges[k] - 2, edges[k + 1] - 2
        np.testing.assert_array_equal(sd["BB"][lo:hi], sd0["BB"][lo:hi] * np.exp(lam[1 + k]))
    assert len(sd["BB"]) == nb - 2
    z = A.expand_sd(m, np.zeros(nblk))
    for s in m.spectra:
        np.testing.assert_array_equal(z[s], sd0[s])         # exp(0) = 1: the plan's own table


def test_run_rejects_warmup_for_centered_and_replay():
    from gibbssampler_amd.samplers import check_warmup
    assert check_warmup("centered", "native", 0) == 0
    assert check_warmup("noncentered", "replay", 0) == 0
    assert check_warmup("asis", "native", 12) == 12
    with pytest.raises(ValueError, match="centered"):
        check_warmup("centered", "native", 5)
    with pytest.raises(ValueError, match="native"):
        check_warmup("noncentered", "replay", 5)
    with pytest.raises(ValueError, match="native"):
        check_warmup("asis", "replay", 1)
    with pytest.raises(ValueError):
        check_warmup("noncentered", "native", -1)
    with pytest.raises(ValueError, match="target_accept"):
        check_warmup("noncentered", "native", 5, target_accept=1.5)


def test_state_without_adaptation_keys_is_not_adapting():
    torch = pytest.importorskip("torch")
    from gibbssampler_amd.samplers import warmup_of_state
    old = {"kind": "noncentered", "rng": "native", "seed": 1, "iteration": 9, "dl": torch.zeros(1, 2, 4)}
    assert warmup_of_state(old) == (0, 0.25, None, None)
    lam, cnt = torch.full((2, 3), 0.5, dtype=torch.float64), torch.full((2, 3), 7, dtype=torch.int32)
    new = dict(old, mh_log_scale=lam, mh_count=cnt, mh_n_warmup=20, mh_target_accept=0.3)
    nw, tgt, l2, c2 = warmup_of_state(new)
    assert (nw, tgt) == (20, 0.3) and l2 is lam and c2 is cnt


def test_tuned_variances_form():
    from gibbssampler_amd.samplers import tuned_variances
    m, _ = A.small_problem(2, bb_blocks="wide")
    lay = A.block_layout(m)
    lam = np.array([0.3, -1.0, 0.0, 2.0, 0.5])
    tv = tuned_variances(m.proposal_variances, m.blocks, m.bins, lay, lam)
    sd = A.expand_sd(m, lam)
    for s in m.spectra:
        assert tv[s].shape == (m.nbins(s) - 2,)
        np.testing.assert_allclose(tv[s], sd[s] ** 2, rtol=1e-14)


def test_config_helper_fills_production_run():
    from gibbssampler_amd.config import make_config
    cfg = make_config(16)
    assert cfg.preliminary_run and cfg.starting_point is None
    tv = {s: np.full(len(b) - 3, 2.0) for s, b in cfg.bins.items()}
    sp = {s: np.arange(len(b) - 1, dtype=float) for s, b in cfg.bins.items()}
    out = cfg.use_preliminary(tv, sp)
    assert out is cfg and cfg.preliminary_run is False
    for s in cfg.bins:
        np.testing.assert_array_equal(cfg.proposal_variances_nc_polarized[s], tv[s])
        np.testing.assert_array_equal(cfg.starting_point[s], sp[s])
    with pytest.raises(ValueError, match="nbins-2"):
        cfg.use_preliminary({s: v[:-1] for s, v in tv.items()}, sp)
    with pytest.raises(ValueError, match="starting_point"):
        cfg.use_preliminary(tv, {s: v[:-1] for s, v in sp.items()})
    with pytest.raises(ValueError, match="positive"):
        cfg.use_preliminary({s: -v for s, v in tv.items()}, sp)


def test_run_record_stores_tuned_variances_under_new_keys():
    from gibbssampler_amd.io import run_record
    bins = {"EE": np.arange(6), "BB": np.arange(6)}
    pv = {"EE": np.ones(3), "BB": np.ones(3)}
    base = run_record(None, None, None, bins, bins, pv, 1.0, 1.0)
    rec = run_record(None, None, None, bins, bins, pv, 1.0, 1.0,
                     tuned_proposal_variances={"EE": 2 * np.ones(3), "BB": 3 * np.ones(3)}, n_warmup=50)
    assert set(rec) - set(base) == {"tuned_proposal_variances_EE", "tuned_proposal_variances_BB", "n_warmup"}
    for k in base:
        assert np.all(np.asarray(rec[k] == base[k])) or rec[k] is base[k]
    np.testing.assert_array_equal(rec["tuned_proposal_variances_BB"], 3 * np.ones(3))
    assert rec["n_warmup"] == 50
