"""GPU: 100-iteration chains in which every spectrum moves, against the oracle's
same-stream chains.

tests/test_gpu_longchain.py runs the reference's blocking, under which TT, EE
and TE stay at their start.  Here TEB at l_max 130 / N_side 64 runs the
multi-block layouts of tests/_mh_layouts.py, chains 0-3, seed 20261015, 100
native iterations as ONE captured hipGraph through BatchedRunner, against the
fixtures tools/gen_golden_longchain_small.py wrote with the oracle alone:

  longchain_nc_teb_L130_blocks.npz   noncentered, layout binned_mixed
  longchain_centered_teb_L130.npz    centered, the bins of binned_mixed
  longchain_asis_teb_L130.npz        ASIS, layout per_bin

with test_gpu_longchain.py's tolerances: the per-bin means of the D_l over the
iterations 1e-6 relative, the D_l after iterations 1, 50 and 100 1e-8 relative,
the accept counts per chain and spectrum exactly.  The noncentered chains also
run as eager steps and must give the graph's trace bit for bit.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _mh_layouts as ML  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _runner(ref):
    from gibbssampler_amd.samplers import BatchedRunner
    kind, layout = str(ref["kind"]), str(ref["layout"])
    P, start = ML.build(layout, 3)
    r = BatchedRunner(kind=kind, lmax=P["lmax"], nside=P["nside"], nfields=3, nchains=int(ref["nchains"]),
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=int(ref["seed"]), chain0=0,
                      store_skymap=kind != "noncentered")
    r.init(start)
    return r, P


def _graph_run(r, niter):
    p = r.plan
    trace = p.zeros(niter, p.nchains, p.nspec, p.maxbins)
    acc = p.zeros(niter, p.nchains, max(p.nacc, 1), dtype=torch.int32)
    r.capture_steps(niter, trace=trace, trace_capacity=niter, accept_trace=acc)
    r.step()
    torch.cuda.synchronize()
    return trace.cpu().numpy(), acc.cpu().numpy()


def _check(name):
    ref = np.load(os.path.join(GOLDEN, name))
    niter, nch = int(ref["niter"]), int(ref["nchains"])
    r, P = _runner(ref)
    p = r.plan
    tr, ac = _graph_run(r, niter)
    snaps = [int(i) for i in ref["snapshot_iterations"]]
    worst_mean = worst_snap = 0.0

    def rel(got, want):
        nz = want != 0
        return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0

    flags = None
    if str(ref["kind"]) != "centered":
        flags = [p.split_accept(torch.from_numpy(ac[i])) for i in range(niter)]
    for k, sp in enumerate(p.spectra):
        nb = len(P["bins"][sp]) - 1
        got_mean = tr[:, :, k, :nb].mean(axis=0)
        worst_mean = max(worst_mean, rel(got_mean, ref[f"mean_{sp}"]))
        for j, it in enumerate(snaps):
            worst_snap = max(worst_snap, rel(tr[it - 1, :, k, :nb], ref[f"snap_{sp}"][:, j]))
    print(f"{name}: means {worst_mean:.3e} ({worst_mean / 1e-6:.3e} of 1e-6), "
          f"snapshots {worst_snap:.3e} ({worst_snap / 1e-8:.3e} of 1e-8)")
    for k, sp in enumerate(p.spectra):
        nb = len(P["bins"][sp]) - 1
        np.testing.assert_allclose(tr[:, :, k, :nb].mean(axis=0), ref[f"mean_{sp}"], rtol=1e-6, atol=1e-300,
                                   err_msg=f"mean {sp}")
        for j, it in enumerate(snaps):
            np.testing.assert_allclose(tr[it - 1, :, k, :nb], ref[f"snap_{sp}"][:, j], rtol=1e-8, atol=1e-300,
                                       err_msg=f"{sp} after iteration {it}")
        if flags is not None:
            got_acc = np.array([sum(int(flags[i][sp][c].sum()) for i in range(niter)) for c in range(nch)])
            np.testing.assert_array_equal(got_acc, ref[f"accepts_{sp}"], err_msg=f"accepts {sp}")
            assert np.all((0 < ref[f"accepts_{sp}"]) & (ref[f"accepts_{sp}"] < ref[f"decisions_{sp}"])), sp
    return ref, tr, ac


def test_longchain_noncentered_blocks_vs_oracle():
    ref, tr, ac = _check("longchain_nc_teb_L130_blocks.npz")
    # the same chains as eager steps: the graph's trace and flags bit for bit
    r, _ = _runner(ref)
    for i in range(int(ref["niter"])):
        r.step()
        np.testing.assert_array_equal(r.dl.cpu().numpy(), tr[i], err_msg=f"eager D_l, iteration {i + 1}")
        np.testing.assert_array_equal(r.accept.cpu().numpy(), ac[i], err_msg=f"eager flags, iteration {i + 1}")


def test_longchain_centered_vs_oracle():
    ref, _, _ = _check("longchain_centered_teb_L130.npz")
    for sp in ("TT", "EE", "BB", "TE"):
        s = ref[f"snap_{sp}"]                   # [chain, snapshot, bin]: every used bin moved between 50 and 100
        assert np.all(s[:, 1, 2:] != s[:, 2, 2:]), sp


def test_longchain_asis_vs_oracle():
    _check("longchain_asis_teb_L130.npz")
