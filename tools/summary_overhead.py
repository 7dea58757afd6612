"""Cost of the streaming posterior summary at the flagship shape (DESIGN.md
'Streaming posterior summaries'): BatchedRunner.run() per step with summary
off, on, and on with keep_history=False, interleaved, three runs each; with
--long N one N-iteration run with keep_history=False that prints the device
memory before and after and the ESS / R-hat ranges; with --profile only a
short summary-on run (for a kernel trace).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lmax", type=int, default=1024)
    ap.add_argument("--nside", type=int, default=512)
    ap.add_argument("--nchains", type=int, default=32)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--max-lag", type=int, default=32)
    ap.add_argument("--long", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.samplers import BatchedRunner

    P = synthetic_problem(args.lmax, args.nside, 3, seed=0)
    r = BatchedRunner(kind="noncentered", lmax=P["lmax"], nside=P["nside"], nfields=3, nchains=args.nchains,
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=20261015, store_skymap=False)
    sm = {"max_lag": args.max_lag}
    modes = {"off": {}, "on": {"summary": sm}, "no_history": {"summary": sm, "keep_history": False}}

    def timed(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(P["dls_init"], n, graph_chunk=args.chunk, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    r.run(P["dls_init"], 2 * args.chunk, graph_chunk=args.chunk, summary=sm)      # captures, first launches
    if args.profile:
        timed("on", 8 * args.chunk)
        return
    if args.long:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        per_step = timed("no_history", args.long)
        after, peak = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
        out = r.summary()
        rng = {s: {k: [float(np.nanmin(v[k][2:])), float(np.nanmax(v[k][2:]))] for k in ("ess", "rhat")}
               for s, v in out.items()}
        print(json.dumps({"long": args.long, "ms_per_step": per_step * 1e3, "n": out["BB"]["n"],
                          "allocated_before": before, "allocated_after": after, "peak": peak,
                          "ess_truncated": {s: int(v["ess_truncated"].sum()) for s, v in out.items()}, **rng}))
        return
    for rep in range(3):
        for mode in modes:
            print(json.dumps({"mode": mode, "rep": rep, "steps": args.steps, "nchains": args.nchains,
                              "max_lag": args.max_lag, "ms_per_step": timed(mode, args.steps) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
