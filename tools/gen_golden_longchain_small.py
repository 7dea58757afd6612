"""Long-chain oracle fixtures in which every spectrum moves.

tools/gen_golden_longchain.py's fixture runs the reference's blocking, where TT,
EE and TE are one whole-range Metropolis block each and never leave their start
in 100 iterations.  These run TEB at l_max 130 / N_side 64 with the multi-block
layouts of tests/_mh_layouts.py (synthetic_problem seed 0, native Philox
streams, seed 20261015, chains 0-3, 100 iterations), with the oracle alone
(oracle/harmonic.py):

  longchain_nc_teb_L130_blocks.npz   noncentered, layout binned_mixed
  longchain_centered_teb_L130.npz    centered, the bins of binned_mixed
  longchain_asis_teb_L130.npz        ASIS, layout per_bin (ASIS.py:134-226; the
                                     re-centring quirk of ASIS.py:203 acts on
                                     the map, which the next CR replaces)

Each keeps what the L 1024 fixture keeps: per chain / spectrum / bin the mean
of the binned D_l over the iterations, the D_l after iterations 1, 50 and 100,
the accept counts per chain and spectrum and the decisions per chain.  The
archive members carry a fixed date, so a rerun reproduces the files byte for
byte.  tests/test_gpu_longchain_small.py compares the device with them;
tests/test_longchain_fixtures_cpu.py keeps them in step with the layouts.

usage: python tools/gen_golden_longchain_small.py [--niter 100] [--procs 4] [--out DIR]
(~1 min on 4 cores)
"""
import argparse
import multiprocessing as mp
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20261015
NCHAINS = 4
GOLDEN = os.path.join(ROOT, "tests", "golden")
# file -> (sampler, layout)
FIXTURES = {
    "longchain_nc_teb_L130_blocks.npz": ("noncentered", "binned_mixed"),
    "longchain_centered_teb_L130.npz": ("centered", "binned_mixed"),
    "longchain_asis_teb_L130.npz": ("asis", "per_bin"),
}


def run_chain(args):
    name, chain, niter = args
    from tests import _mh_layouts as ML
    kind, layout = FIXTURES[name]
    P, start = ML.build(layout, 3)
    m = ML.model_of(P)
    hist, flags = ML.oracle_chain(m, kind, start, SEED, chain, niter)
    snaps = [it for it in (1, niter // 2, niter)]
    out = {"snaps": snaps}
    for sp in m.spectra:
        out[f"mean_{sp}"] = hist[sp].mean(axis=0)
        out[f"snap_{sp}"] = np.stack([hist[sp][it - 1] for it in snaps])
        if flags is not None:
            out[f"accepts_{sp}"] = int(flags[sp].sum())
            out[f"decisions_{sp}"] = int(flags[sp].size)
    return name, chain, out


FUSED_NAME = "mh_fused_teb_L1100.npz"
FUSED = dict(lmax=1100, nside=512, upto=300, wide=150, niter=2)


def run_fused(_):
    """binned_mixed scaled to l_max 1100 (beyond one l per thread of the register
    MH form): D_l and accept flags of chain 0's first iterations, for
    tests/test_gpu_mh_blocking.py::test_lds_phase_kernel_matches_oracle_fixture."""
    import time
    from tests import _mh_layouts as ML
    q = FUSED
    P, start = ML.build("binned_mixed", 3, lmax=q["lmax"], nside=q["nside"], upto=q["upto"], wide=q["wide"],
                        wide_bb=q["wide"])
    m = ML.model_of(P)
    t0 = time.time()
    hist, flags = ML.oracle_chain(m, "noncentered", start, SEED, 0, q["niter"])
    print(f"{FUSED_NAME}: oracle {time.time() - t0:.0f} s", flush=True)
    out = {k: np.int64(v) for k, v in q.items()}
    out["seed"] = np.int64(SEED)
    for sp in m.spectra:
        out[f"dl_{sp}"] = hist[sp]
        out[f"flags_{sp}"] = flags[sp].astype(np.int8)
        out[f"blocks_{sp}"] = np.asarray(P["blocks"][sp], dtype=np.int64)
    return out


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member date (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--niter", type=int, default=100)
    ap.add_argument("--procs", type=int, default=4)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    jobs = [(name, c, a.niter) for name in FIXTURES for c in range(NCHAINS)]
    with mp.get_context("spawn").Pool(a.procs) as pool:
        fused = pool.map_async(run_fused, [0])
        res = pool.map(run_chain, jobs)
        save_npz(os.path.join(a.out, FUSED_NAME), fused.get()[0])
        print(f"wrote {os.path.join(a.out, FUSED_NAME)}")
    for name, (kind, layout) in FIXTURES.items():
        rs = [r[2] for r in sorted((r for r in res if r[0] == name), key=lambda r: r[1])]
        out = {"seed": np.int64(SEED), "niter": np.int64(a.niter), "nchains": np.int64(NCHAINS),
               "kind": np.array(kind), "layout": np.array(layout),
               "config": np.array(f"{kind} TEB all_sph, N_side 64, l_max 130, synthetic_problem(seed=0), "
                                  f"tests._mh_layouts.build('{layout}', 3)"),
               "snapshot_iterations": np.array(rs[0]["snaps"], dtype=np.int64)}
        for sp in ("TT", "EE", "BB", "TE"):
            out[f"mean_{sp}"] = np.stack([r[f"mean_{sp}"] for r in rs])
            out[f"snap_{sp}"] = np.stack([r[f"snap_{sp}"] for r in rs])
            if kind != "centered":
                out[f"accepts_{sp}"] = np.array([r[f"accepts_{sp}"] for r in rs], dtype=np.int64)
                out[f"decisions_{sp}"] = np.array([r[f"decisions_{sp}"] for r in rs], dtype=np.int64)
        path = os.path.join(a.out, name)
        save_npz(path, out)
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
