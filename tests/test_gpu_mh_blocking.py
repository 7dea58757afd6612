"""GPU: the NC Metropolis kernels under multi-block TT / EE / TE layouts against
the oracle.

The reference's blocking gives TT, EE and TE one whole-range block each, so the
other GPU tests decide one block per T / E phase.  Here every spectrum has
several blocks (tests/_mh_layouts.py), at l_max 130 / N_side 64 (three l tiles,
the last partial), 2 chains from chain id 3, native Philox streams, 3
iterations through BatchedRunner, against the live oracle loop
noncentered_params -> cr_normals -> cr_apply -> sweep_stats -> nc_mh (ASIS: the
loop of test_configs3_asis_fullsize_matches_oracle):

  per_bin        T / E unbinned, one block per bin (129 narrow blocks and one
                 that is empty after clipping, per T / E phase); BB binned,
                 [2, 30) then per bin
  binned_mixed   every spectrum binned (unbinned to l 40, then 3 wide; BB to
                 l 60, then 7; F < 3: EE to l 50, then 4), one wide block, then
                 per-bin blocks, [nb - 5, nb - 1) and [nb - 1, nb + 7) clipped;
                 bins 2-3 of TT and TE and the last two bins of EE in no block
  many_wide      T / E unbinned, six blocks of 21-22 multipoles per spectrum
                 (more than the four wide blocks the LDS-phase kernel decides
                 under one pair of barriers; one wave each in the register form)
  near_singular  per_bin from TE = 0.98 sqrt(TT EE) in every third bin: the
                 per-l positive-definiteness test rejects some TT blocks of an
                 iteration while others accept

D_l after every iteration: 1e-10 relative (native vs oracle: libm ulps only);
accept flags: exactly.  Both MH forms (two workgroups per chain, the default
when the proposal launch left a snapshot, and GS_MH_SPLIT=0), 1 and 2
Metropolis attempts per block, F = 1, 2, 3, noncentered and ASIS.

The plan refuses a TEB model whose TT, EE and TE bins differ, and blocks are an
edge array (consecutive blocks touch), so at F = 3 the T / E spectra share the TT
bins and the bins of no block lie at the ends of the range
(test_plan_refuses_unshared_te_bins).

k_mh_fused (the LDS-phase kernel) runs when the l range exceeds one l per
thread: one case at l_max 1100 / N_side 512 (binned_mixed, unbinned to l 300,
wide blocks [4, 152) / [2, 150)), 1 chain, 2 iterations.  The live oracle took 12 s for it
on one CPU core (over 10 s), so its D_l and flags are the fixture
tests/golden/mh_fused_teb_L1100.npz (tools/gen_golden_longchain_small.py).

Checked by mutation on scratch builds (MI355X):
  * the [TT] and [TE] phases swapped in gs_plan_create: every F = 3 case of
    test_blocked_layouts_match_oracle, the l_max 1100 case and the noncentered
    and ASIS long chains fail; the suite without these two files stays green;
  * block edges clipped to nbins - 1: every case of
    test_blocked_layouts_match_oracle, the l_max 1100 case and both long chains;
  * k_mh_reg's narrow-block loop starting at nwide + tid + 1: every case of
    test_blocked_layouts_match_oracle, test_forms_bit_identical and both long
    chains (this one the older tests catch too, through the per-bin BB blocks).

"""
import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _mh_layouts as ML  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
NCH, CHAIN0, NITER = 2, 3, 3
RTOL = 1e-10
FUSED_FIX = os.path.join(ROOT, "tests", "golden", "mh_fused_teb_L1100.npz")

# (layout, F, kind, Metropolis attempts per block)
CASES = [(lay, 3, "noncentered", 1) for lay in ML.LAYOUTS] + \
        [(lay, 3, "asis", 1) for lay in ("per_bin", "binned_mixed")] + \
        [("binned_mixed", 3, "noncentered", 2)] + \
        [(lay, F, "noncentered", 1) for F in (2, 1) for lay in ("per_bin", "binned_mixed")]


@functools.lru_cache(maxsize=None)
def _case(layout, F):
    P, start = ML.build(layout, F)
    return P, start, ML.model_of(P)


@functools.lru_cache(maxsize=None)
def _oracle(layout, F, kind, n_mh):
    """Per chain (D_l history, flags) of the oracle; computed once, never modified."""
    P, start, m = _case(layout, F)
    return [ML.oracle_chain(m, kind, start, SEED, CHAIN0 + c, NITER, n_mh) for c in range(NCH)]


def _runner(P, start, kind, n_mh=1, nch=NCH, chain0=CHAIN0):
    from gibbssampler_amd.samplers import BatchedRunner
    r = BatchedRunner(kind, P["lmax"], P["nside"], P["nfields"], nch, P["bl"], P["noise_var"], P["bins"], P["d_alm"],
                      blocks=P["blocks"], proposal_variances=P["proposal_variances"], rng="native", seed=SEED,
                      chain0=chain0, n_iter_metropolis=n_mh, store_skymap=False)
    r.init(start)
    return r


def _eager(r, n):
    dl, acc = [], []
    for _ in range(n):
        r.step()
        dl.append(r.dl.cpu().numpy().copy())
        acc.append(r.accept.cpu().numpy().copy())
    return np.stack(dl), np.stack(acc)


def _graph(r, n):
    p = r.plan
    trace = p.zeros(n, p.nchains, p.nspec, p.maxbins)
    acc = p.zeros(n, p.nchains, max(p.nacc, 1), dtype=torch.int32)
    r.capture_steps(n, trace=trace, trace_capacity=n, accept_trace=acc)
    r.step()
    torch.cuda.synchronize()
    return trace.cpu().numpy(), acc.cpu().numpy()


def _compare(p, dl, acc, want, label):
    """dl [n, chains, nspec, maxbins], acc [n, chains, nacc] against the oracle's per-chain (history, flags)."""
    worst = 0.0
    for it in range(dl.shape[0]):
        flags = p.split_accept(torch.from_numpy(acc[it]))
        for c, (hist, wfl) in enumerate(want):
            for k, sp in enumerate(p.spectra):
                ref = hist[sp][it]
                got = dl[it, c, k, :len(ref)]
                nz = ref != 0
                if nz.any():
                    worst = max(worst, float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))))
                np.testing.assert_array_equal(flags[sp][c], wfl[sp][it],
                                              err_msg=f"{label}: flags {sp} chain {c} iteration {it + 1}")
                np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0,
                                           err_msg=f"{label}: D_l {sp} chain {c} iteration {it + 1}")
    print(f"{label}: max |device - oracle| / |oracle| = {worst:.3e} ({worst / RTOL:.3e} of the tolerance)")


@pytest.mark.parametrize("split", [None, "0"], ids=["split_default", "split_off"])
@pytest.mark.parametrize("layout,F,kind,n_mh", CASES, ids=lambda v: str(v))
def test_blocked_layouts_match_oracle(gsopt, layout, F, kind, n_mh, split):
    P, start, _ = _case(layout, F)
    want = _oracle(layout, F, kind, n_mh)
    if split is not None:
        gsopt.setenv("GS_MH_SPLIT", split)
    r = _runner(P, start, kind, n_mh)
    assert r.plan.mh_reg_form
    dl, acc = _eager(r, NITER)
    _compare(r.plan, dl, acc, want, f"{layout} F={F} {kind} n_mh={n_mh} split={split}")


@pytest.mark.parametrize("layout,F,kind,n_mh", [c for c in CASES if c[1] == 3], ids=lambda v: str(v))
def test_both_branches_in_every_spectrum(layout, F, kind, n_mh):
    """The layouts' conditions, on the oracle's flags: every spectrum of every
    chain accepts some and rejects some of its decisions over the 3 iterations."""
    for c, (_, fl) in enumerate(_oracle(layout, F, kind, n_mh)):
        for sp, f in fl.items():
            assert 0 < int(f.sum()) < f.size, (layout, kind, sp, c, int(f.sum()), f.size)


def test_near_singular_rejects_some_blocks_only():
    """near_singular: at least 10 proposals fail the per-l positive-definiteness
    test (oracle H._psd_ok), and in some iteration of some T / E spectrum blocks
    fail it while other blocks of the same spectrum accept."""
    P, start, m = _case("near_singular", 3)
    for c in range(NCH):
        cnt = ML.count_psd_failures(m, start, SEED, CHAIN0 + c, NITER)
        failed = sum(int(cnt[sp][:, 0].sum()) for sp in ("TT", "EE", "TE"))
        print(f"near_singular chain {CHAIN0 + c}: {failed} failed positive-definiteness tests",
              {sp: cnt[sp].tolist() for sp in ("TT", "EE", "TE")})
        assert failed >= 10
        assert any(f > 0 and a > 0 for sp in ("TT", "EE", "TE") for f, a in cnt[sp])


def test_many_wide_has_more_wide_blocks_than_one_group():
    src = open(os.path.join(ROOT, "gibbssampler_amd", "csrc", "gs_kernels.hip")).read()
    small = int(re.search(r"constexpr int MH_SMALL = (\d+);", src).group(1))
    maxw = int(re.search(r"constexpr int MAXW = (\d+);", src).group(1))
    P, _, _ = _case("many_wide", 3)
    for sp in ("TT", "EE", "TE"):
        n = ML.wide_blocks(P["bins"][sp], P["blocks"][sp], small)
        assert n >= 5 and n > maxw, (sp, n)
        assert n == len(P["blocks"][sp]) - 1          # and none narrow
    # the other layouts put narrow blocks beside wide ones in a T / E phase
    P, _, _ = _case("binned_mixed", 3)
    for sp in ("TT", "EE", "TE"):
        n = ML.wide_blocks(P["bins"][sp], P["blocks"][sp], small)
        assert 1 <= n < len(P["blocks"][sp]) - 1
        assert P["blocks"][sp][-1] > len(P["bins"][sp]) - 1 or sp == "EE"      # a clipped last edge


def test_plan_refuses_unshared_te_bins():
    """binned_mixed with each spectrum's own bins (TT to l 40 then 3 wide, EE to
    50 then 4, TE to 30 then 5) is not a model the plan takes at F = 3."""
    from gibbssampler_amd import _capi
    from gibbssampler_amd.engine import GibbsPlan
    from gibbssampler_amd.problem import synthetic_problem
    bins = ML.mixed_bins(ML.L_SMALL, 3, shared=False)
    P = synthetic_problem(ML.L_SMALL, ML.NSIDE_SMALL, 3, seed=0, bins=bins, blocks=ML.mixed_blocks(bins))
    with pytest.raises(_capi.GibbsHipError, match="TT, EE and TE must share bins"):
        GibbsPlan(P["lmax"], P["nside"], 3, 1, P["bl"], P["noise_var"], P["bins"], blocks=P["blocks"],
                  proposal_variances=P["proposal_variances"])


@pytest.mark.parametrize("layout", ["per_bin", "binned_mixed"])
def test_forms_bit_identical(gsopt, layout):
    """F = 3: the split and the one-workgroup MH, eager steps and one captured
    3-step graph, the pipelined and the serial multi-step graph (GS_NC_PIPE, read
    at plan creation) give the same bits: D_l after every iteration and flags."""
    P, start, _ = _case(layout, 3)

    def run(split, graph, pipe="1"):
        gsopt.setenv("GS_MH_SPLIT", split)
        gsopt.setenv("GS_NC_PIPE", pipe)
        r = _runner(P, start, "noncentered")
        return _graph(r, NITER) if graph else _eager(r, NITER)

    base = run("1", False)
    assert base[1].any() and not base[1].all()
    for split, graph, pipe in (("0", False, "1"), ("1", True, "1"), ("0", True, "1"), ("1", True, "0"),
                               ("0", True, "0")):
        got = run(split, graph, pipe)
        for x, y in zip(base, got):
            np.testing.assert_array_equal(x, y, err_msg=f"{layout}: split={split} graph={graph} pipe={pipe}")


def test_lds_phase_kernel_matches_oracle_fixture():
    """l_max 1100 / N_side 512: the plan does not take the register form, so
    k_mh_fused decides; D_l and flags of 2 iterations of chain 0 against the
    oracle's (fixture; the live oracle measured 12 s on one core)."""
    ref = np.load(FUSED_FIX)
    lmax, nside, niter = int(ref["lmax"]), int(ref["nside"]), int(ref["niter"])
    P, start = ML.build("binned_mixed", 3, lmax=lmax, nside=nside, upto=int(ref["upto"]), wide=int(ref["wide"]),
                        wide_bb=int(ref["wide"]))
    for sp in P["bins"]:
        np.testing.assert_array_equal(P["blocks"][sp], ref[f"blocks_{sp}"])       # the layout the fixture ran
    from gibbssampler_amd.samplers import BatchedRunner
    r = BatchedRunner("noncentered", lmax, nside, 3, 1, P["bl"], P["noise_var"], P["bins"], P["d_alm"],
                      blocks=P["blocks"], proposal_variances=P["proposal_variances"], rng="native",
                      seed=int(ref["seed"]), chain0=0, store_skymap=False)
    r.init(start)
    assert not r.plan.mh_reg_form
    dl, acc = _eager(r, niter)
    want = [({sp: ref[f"dl_{sp}"] for sp in r.plan.spectra}, {sp: ref[f"flags_{sp}"] for sp in r.plan.spectra})]
    for sp in r.plan.spectra:
        f = ref[f"flags_{sp}"]
        assert 0 < int(f.sum()) < f.size, sp
    _compare(r.plan, dl, acc, want, "binned_mixed L1100 (k_mh_fused)")
