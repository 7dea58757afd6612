"""Cost of keeping the D_l draws in the Blackwell-Rao sample bank (DESIGN.md
'Gaussianised Blackwell-Rao likelihood'): BatchedRunner.run() per step with
br_samples draws off and on over a low-l range, interleaved, three runs each
after one discarded run, cases as tools/brs_overhead.py.  One JSON line per
measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"centered": dict(kind="centered", lmax=512, nside=256, nchains=1),
         "asis": dict(kind="asis", lmax=1024, nside=512, nchains=32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default="asis")
    ap.add_argument("--nfields", type=int, default=3)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--low-l", type=int, default=30, help="l_max of the low-l range")
    args = ap.parse_args()
    import torch
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.samplers import BatchedRunner

    c = CASES[args.case]
    P = synthetic_problem(c["lmax"], c["nside"], args.nfields, seed=0)
    r = BatchedRunner(kind=c["kind"], lmax=P["lmax"], nside=P["nside"], nfields=args.nfields, nchains=c["nchains"],
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=20261021, store_skymap=False)
    modes = {"draws_off": {"br_samples": {"lrange": (2, args.low_l)}},
             "draws_on": {"br_samples": {"lrange": (2, args.low_l), "draws": True}}}

    def timed(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(P["dls_init"], n, graph_chunk=args.chunk, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    info = {}
    for mode in modes:                                      # captures, first launches
        r.run(P["dls_init"], 2 * args.chunk, graph_chunk=args.chunk, **modes[mode])
        if r._brs is not None:
            info[mode] = {"Ju": r._brs.Ju, "bank_bytes_per_step": r._brs.nbytes(1)}
    timed("draws_off", args.steps)                                # the first off run is left out
    for rep in range(3):
        for mode in modes:
            print(json.dumps({"case": args.case, "mode": mode, "rep": rep, "steps": args.steps,
                              "nchains": c["nchains"], "ms_per_step": timed(mode, args.steps) * 1e3,
                              **info.get(mode, {})}), flush=True)


if __name__ == "__main__":
    main()
