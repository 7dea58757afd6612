"""The packed diagonal workgroups of the CR sweep (gs_kernels.hip
cr_sweep_packed, csrc/gs_sweep_pack.h; option GS_SWEEP_PACK): the native-draw
throughput sweep without the map deals the column segments of a diagonal
workgroup over its threads by length.  No sum changes its terms or their
order, so every comparison is bit for bit between a fresh plan made with
GS_SWEEP_PACK=1 and a fresh plan made with GS_SWEEP_PACK=0.

Shapes (chains > 4: the throughput form; <= 4 chains with 4-row chunks would
take the latency form, which the option does not touch).  Which workgroups the
table builder packs is counted on the CPU by tests/sweep_pack_check.cpp, and
tests/test_sweep_pack_cpu.py (GPU_SHAPES) asserts per shape what is said here;
the plan reports its packed and absorbed counts, asserted below.
  L70   N_side 32, 5 chains: 8-row chunks, two l tiles.  One packed workgroup,
        interior (tile 0, chunk group 1: all l >= 7, no row m = 0, no absorb);
        the partial tile and the groups at the ends issue 7 rows either way and
        stay plain
  L96   N_side 64, 5 chains: 8-row chunks.  Three packed workgroups: two absorb
        the next chunk group's single entry, one holds row m = 0 (taken before
        the loop, one slot), one is of the partial tile (lanes l < 0).  The
        shape the F = 1, F = 2, GS_NC_RAW=0 and ASIS variants run on
  L127 / L128 / L130  N_side 64, 5 chains: a tile edge just below, on and just
        off a multiple of 64: L127 packs the workgroup with row m = 0, L128
        absorbs two single entries
  L300 / L320  N_side 128, 6 chains: 4-row chunks; L300 packs three workgroups of
        the partial tile and row m = 0, L320 absorbs five single entries
  L520 / L576  N_side 256, 5 chains: 16-row chunks, the flagship's chunking; at
        L520 a tile's last chunk group holds 9 rows, not one entry (no absorb:
        that needs L a multiple of 64 there); L576 absorbs nine, as the
        flagship's tiles do
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAPES = {"L70": (70, 32, 5), "L96": (96, 64, 5), "L127": (127, 64, 5), "L128": (128, 64, 5), "L130": (130, 64, 5),
          "L300": (300, 128, 6), "L320": (320, 128, 6), "L520": (520, 256, 5), "L576": (576, 256, 5)}
# per shape: packed workgroups, absorbed one-entry chunk groups (per chain; the
# counts of tests/sweep_pack_check.cpp)
PACKED = {"L70": (1, 0), "L96": (3, 2), "L127": (4, 0), "L128": (3, 2), "L130": (3, 0), "L300": (15, 0),
          "L320": (15, 5), "L520": (8, 0), "L576": (9, 9)}
SEED, IT = 23, 4


@functools.lru_cache(maxsize=None)
def _problem(F, shape):
    from gibbssampler_amd.problem import synthetic_problem
    L, nside, _ = SHAPES[shape]
    return synthetic_problem(L, nside, F, seed=9)


def _runner(F, shape, pack, kind="noncentered", **opts):
    """A fresh, initialised runner whose plan is created with GS_SWEEP_PACK = pack."""
    from gibbssampler_amd import _capi
    from gibbssampler_amd.samplers import BatchedRunner
    P = _problem(F, shape)
    with _capi.options(GS_SWEEP_PACK="1" if pack else "0", **opts):
        r = BatchedRunner(kind, P["lmax"], P["nside"], F, SHAPES[shape][2], P["bl"], P["noise_var"], P["bins"],
                          P["d_alm"], blocks=P["blocks"], proposal_variances=P["proposal_variances"], rng="native",
                          seed=SEED, store_skymap=False)
    r.init(P["dls_init"])
    # the grid the plan built: packed with the option on at tw = 1, plain otherwise
    want = PACKED[shape] if pack and opts.get("GS_SWEEP_TW", "1") == "1" else (0, 0)
    assert (r.plan.sweep_packed, r.plan.sweep_absorbed) == want
    return r


def _eager_stats(r):
    """The statistic rows of one eager native NC sweep + finish (no map) at the runner's state."""
    p = r.plan
    p.nc_prologue(r.dl, seed=SEED, iteration=IT)
    p.nc_sweep(r.d, r.dl, None, seed=SEED, iteration=IT)
    out = p.nc_stats().cpu().numpy()
    torch.cuda.synchronize()
    return out


def _replays(r, K=3, R=2):
    """capture_steps(K) replayed R times: the D_l trace and the accept trace of K R steps."""
    p = r.plan
    trace = p.zeros(K, p.nchains, p.nspec, p.maxbins)
    acc = p.zeros(K, p.nchains, max(p.nacc, 1), dtype=torch.int32)
    r.capture_steps(K, trace=trace, trace_capacity=K, accept_trace=acc)
    tr, ac = [], []
    for _ in range(R):
        r.step()
        tr.append(trace.clone())
        ac.append(acc.clone())
    torch.cuda.synchronize()
    return torch.cat(tr).cpu().numpy(), torch.cat(ac).cpu().numpy()


def _run(F, shape, pack, kind="noncentered", stats=True, **opts):
    st = _eager_stats(_runner(F, shape, pack, kind, **opts)) if stats else None
    r = _runner(F, shape, pack, kind, **opts)
    tr, ac = _replays(r)
    return st, tr, ac, r.dl.cpu().numpy(), r.graph_pipelined


def _assert_same(on, off):
    for a, b in zip(on[:4], off[:4]):
        if a is not None:
            np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(on[1])) and on[1].shape[0] == 6


@pytest.mark.parametrize("F,shape", [(1, "L70"), (2, "L70"), (3, "L70"), (1, "L96"), (2, "L96"), (3, "L96"),
                                     (3, "L127"), (1, "L128"), (2, "L128"), (3, "L128"), (3, "L130"), (3, "L300"),
                                     (3, "L320"), (3, "L520"), (3, "L576")])
def test_packed_equals_plain(F, shape):
    """Raw-moment NC steps: the statistics of one eager sweep + finish, then a
    3-step graph replayed twice (the pipelined schedule, both partial slots)."""
    on, off = _run(F, shape, True), _run(F, shape, False)
    assert on[4] and off[4]                     # both pipelined: the sweeps ahead fill both slots
    _assert_same(on, off)
    assert np.abs(on[0]).max() > 0.0


@pytest.mark.parametrize("F,shape", [(3, "L70"), (1, "L96"), (2, "L96"), (3, "L96"), (3, "L127"), (3, "L128")])
def test_packed_equals_plain_direct_statistics(F, shape):
    """GS_NC_RAW=0: the sweep accumulates the statistics of s (the operator per
    lane), the same row code path of the packed form; L96: with the absorbed
    entry, row m = 0 and the partial tile."""
    on, off = _run(F, shape, True, GS_NC_RAW="0"), _run(F, shape, False, GS_NC_RAW="0")
    _assert_same(on, off)


@pytest.mark.parametrize("F,shape", [(3, "L70"), (1, "L96"), (2, "L96"), (3, "L96"), (3, "L128")])
def test_packed_equals_plain_asis(F, shape):
    """ASIS steps without the map: both of a step's sweeps draw natively through
    the same no-map throughput sweep (the operator from the table)."""
    on, off = _run(F, shape, True, "asis", stats=False), _run(F, shape, False, "asis", stats=False)
    assert not on[4]
    _assert_same(on, off)


def test_option_ignored_for_other_workgroup_shapes():
    """GS_SWEEP_TW=2 keeps the plain grid (the plan reports no packed workgroup,
    _runner): the option changes nothing there."""
    on, off = _run(3, "L96", True, GS_SWEEP_TW="2"), _run(3, "L96", False, GS_SWEEP_TW="2")
    _assert_same(on, off)
