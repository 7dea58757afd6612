"""Cost of the streaming Blackwell-Rao likelihood (DESIGN.md 'Streaming
Blackwell-Rao likelihood'): BatchedRunner.run() per step with br_likelihood off
and on for K theory spectra over a low-l range and over every drawn bin,
interleaved, three runs each, for
  --case centered   configs[1] shape: centered, l_max 512, N_side 256, 1 chain
  --case asis       configs[3] shape: ASIS, l_max 1024, N_side 512, 32 chains
With --profile only a short run with it on (for a kernel trace).  One JSON
line per measurement."""
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
    ap.add_argument("--models", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--low-l", type=int, default=30, help="l_max of the low-l range")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.samplers import BatchedRunner

    c = CASES[args.case]
    P = synthetic_problem(c["lmax"], c["nside"], args.nfields, seed=0)
    r = BatchedRunner(kind=c["kind"], lmax=P["lmax"], nside=P["nside"], nfields=args.nfields, nchains=c["nchains"],
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=20261021, store_skymap=False)
    rng = np.random.default_rng(0)
    modes = {"off": {}}
    for K in args.models:
        # the fiducial scaled by one amplitude per model, within +-10 %
        amp = 1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=K)
        theory = {s: amp[:, None] * np.asarray(v, dtype=np.float64)[None] for s, v in P["dls_init"].items()}
        modes[f"on_K{K}_low"] = {"br_likelihood": {"theory": theory, "lrange": (2, args.low_l)}}
        modes[f"on_K{K}_full"] = {"br_likelihood": {"theory": theory}}

    def timed(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(P["dls_init"], n, graph_chunk=args.chunk, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    info = {}
    for mode in modes:                                      # captures, first launches
        r.run(P["dls_init"], 2 * args.chunk, graph_chunk=args.chunk, **modes[mode])
        if r._brl is not None:
            info[mode] = {"Ju": r._brl.Ju, "K": r._brl.K, "state_bytes": r._brl.data.numel() * 8}
    if args.profile:
        timed(list(modes)[-1], 8 * args.chunk)
        return
    for rep in range(3):
        for mode in modes:
            print(json.dumps({"case": args.case, "mode": mode, "rep": rep, "steps": args.steps,
                              "nchains": c["nchains"], "ms_per_step": timed(mode, args.steps) * 1e3,
                              **info.get(mode, {})}), flush=True)
    res = r.br_likelihood()
    print(json.dumps({"case": args.case, "n": res["n"], "bad": int(res["bad"].sum()),
                      "neff_min": float(res["neff"].min()), "neff_max": float(res["neff"].max()),
                      "loglike_max": float(res["loglike"].max())}))


if __name__ == "__main__":
    main()
