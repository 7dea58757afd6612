"""The small long-chain fixtures (tools/gen_golden_longchain_small.py) stay in
step with the layouts of tests/_mh_layouts.py and the oracle: they load, every
spectrum moves in them, and chain 0's first iteration recomputed by the oracle
equals each fixture's iteration-1 snapshot exactly.  The l_max 1100 fixture of
the LDS-phase MH kernel is checked for its layout and both decision branches.
"""
import os

import numpy as np
import pytest

from tests import _mh_layouts as ML

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPECTRA = ("TT", "EE", "BB", "TE")
FIXTURES = {"longchain_nc_teb_L130_blocks.npz": ("noncentered", "binned_mixed"),
            "longchain_centered_teb_L130.npz": ("centered", "binned_mixed"),
            "longchain_asis_teb_L130.npz": ("asis", "per_bin")}
L1024 = os.path.join(GOLDEN, "longchain_nc_teb_L1024_c4.npz")


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_matches_layout_and_oracle(name):
    path = os.path.join(GOLDEN, name)
    ref = np.load(path)
    kind, layout = FIXTURES[name]
    assert (str(ref["kind"]), str(ref["layout"])) == (kind, layout)
    assert (int(ref["seed"]), int(ref["niter"]), int(ref["nchains"])) == (20261015, 100, 4)
    assert list(ref["snapshot_iterations"]) == [1, 50, 100]
    assert os.path.getsize(path) < os.path.getsize(L1024)
    P, start = ML.build(layout, 3)
    m = ML.model_of(P)
    first, _ = ML.oracle_step(m, kind, start, int(ref["seed"]), 0, 1)
    for sp in SPECTRA:
        nb = len(P["bins"][sp]) - 1
        assert ref[f"mean_{sp}"].shape == (4, nb) and ref[f"snap_{sp}"].shape == (4, 3, nb)
        np.testing.assert_array_equal(ref[f"snap_{sp}"][0, 0], first[sp], err_msg=sp)
        if kind == "centered":
            s = ref[f"snap_{sp}"]
            assert np.all(s[:, 1, 2:] != s[:, 2, 2:]), sp        # every used bin moves between iterations 50 and 100
        else:
            acc, dec = ref[f"accepts_{sp}"], ref[f"decisions_{sp}"]
            assert np.all(dec == 100 * (len(P["blocks"][sp]) - 1))
            assert np.all((0 < acc) & (acc < dec)), (sp, acc, dec)
            # the chain left its start in blocked bins (bins of no block keep it)
            assert np.any(ref[f"snap_{sp}"][:, 2] != np.asarray(start[sp])[None], axis=1).all(), sp


def test_lds_phase_fixture_layout():
    ref = np.load(os.path.join(GOLDEN, "mh_fused_teb_L1100.npz"))
    lmax = int(ref["lmax"])
    assert lmax + 1 - 2 > 1024                     # more multipoles than threads of the register MH form
    P, _ = ML.build("binned_mixed", 3, lmax=lmax, nside=int(ref["nside"]), upto=int(ref["upto"]),
                    wide=int(ref["wide"]), wide_bb=int(ref["wide"]))
    for sp in SPECTRA:
        np.testing.assert_array_equal(P["blocks"][sp], ref[f"blocks_{sp}"])
        f = ref[f"flags_{sp}"]
        assert f.shape == (int(ref["niter"]), len(P["blocks"][sp]) - 1)
        assert ref[f"dl_{sp}"].shape == (int(ref["niter"]), len(P["bins"][sp]) - 1)
        assert 0 < int(f.sum()) < f.size, sp


def test_layout_shapes():
    """What the layouts are for: bins of no block, a clipped last edge, an empty
    block, wide beside narrow blocks (MH_SMALL = 16 multipoles)."""
    P, _ = ML.build("binned_mixed", 3)
    for sp in ("TT", "EE", "TE"):
        np.testing.assert_array_equal(P["bins"][sp], P["bins"]["TT"])
        nb = len(P["bins"][sp]) - 1
        e = np.clip(P["blocks"][sp], 0, nb)
        covered = np.zeros(nb, dtype=bool)
        for k in range(len(e) - 1):
            covered[e[k]:e[k + 1]] = True
        assert int((~covered[2:]).sum()) == 2, sp
        assert 1 <= ML.wide_blocks(P["bins"][sp], P["blocks"][sp], 16) < len(e) - 1
    assert P["blocks"]["TT"][-1] > len(P["bins"]["TT"]) - 1
    P, _ = ML.build("per_bin", 3)
    nb = len(P["bins"]["TT"]) - 1
    assert P["blocks"]["TT"][-2] == nb and P["blocks"]["TT"][-1] == nb + 1       # the last block clips to empty
    P, _ = ML.build("many_wide", 3)
    for sp in ("TT", "EE", "TE"):
        w = np.diff(P["blocks"][sp])
        assert len(w) == 6 and set(w) <= {21, 22}
