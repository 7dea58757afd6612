"""Cost of the Rao-Blackwellised posterior sky map at the flagship shape
(DESIGN.md 'Rao-Blackwellised posterior sky map'): BatchedRunner.run() per step
of the NC sampler (32 chains, L 1024, TEB, 1024 steps, graph_chunk 32) with
wiener_posterior off and on, interleaved, three runs each after one discarded
off run; with --summary also with the streaming summary alone, the launch the
update is measured against.  One JSON line per measurement, appended to
profiles/wf_overhead.jsonl."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lmax", type=int, default=1024)
    ap.add_argument("--nside", type=int, default=512)
    ap.add_argument("--nchains", type=int, default=32)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wf_overhead.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.samplers import BatchedRunner

    P = synthetic_problem(args.lmax, args.nside, 3, seed=0)
    r = BatchedRunner(kind="noncentered", lmax=P["lmax"], nside=P["nside"], nfields=3, nchains=args.nchains,
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=20261015, store_skymap=False)
    modes = {"off": {}, "on": {"wiener_posterior": True}}
    if args.summary:
        modes["summary"] = {"summary": {"max_lag": 32}}

    def timed(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(P["dls_init"], n, graph_chunk=args.chunk, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    r.run(P["dls_init"], 2 * args.chunk, graph_chunk=args.chunk, wiener_posterior=True)     # captures, first launches
    timed("off", args.steps)                                                                # discarded
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rep in range(args.reps):
            for mode in modes:
                line = json.dumps({"mode": mode, "rep": rep, "steps": args.steps, "nchains": args.nchains,
                                   "lmax": args.lmax, "chunk": args.chunk,
                                   "ms_per_step": timed(mode, args.steps) * 1e3})
                print(line, flush=True)
                f.write(line + "\n")
    out = r.run(P["dls_init"], 4 * args.chunk, graph_chunk=args.chunk, wiener_posterior=True, keep_history=False)
    res = r.wiener_posterior()
    print(json.dumps({"check": "finite", "n": res["n"], "returned": [o is None for o in out],
                      "alm_mean_finite": bool(np.isfinite(res["alm_mean"]).all())}), flush=True)


if __name__ == "__main__":
    main()
