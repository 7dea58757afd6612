"""Cost of the streaming Blackwell-Rao posteriors (DESIGN.md 'Streaming
Blackwell-Rao posteriors'): BatchedRunner.run() per step with blackwell_rao
off and on at G grid points, interleaved, three runs each, for
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
    ap.add_argument("--points", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    from gibbssampler_amd.problem import synthetic_problem
    from gibbssampler_amd.samplers import BatchedRunner

    c = CASES[args.case]
    P = synthetic_problem(c["lmax"], c["nside"], args.nfields, seed=0)
    r = BatchedRunner(kind=c["kind"], lmax=P["lmax"], nside=P["nside"], nfields=args.nfields, nchains=c["nchains"],
                      bl=P["bl"], noise_var=P["noise_var"], bins=P["bins"], d_alm=P["d_alm"], blocks=P["blocks"],
                      proposal_variances=P["proposal_variances"], rng="native", seed=20261020, store_skymap=False)
    modes = {"off": {}}
    for G in args.points:
        modes[f"on_G{G}"] = {"blackwell_rao": {"points": G, "span": (0.5, 2.0)}}

    def timed(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(P["dls_init"], n, graph_chunk=args.chunk, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for mode in modes:                                      # captures, first launches
        r.run(P["dls_init"], 2 * args.chunk, graph_chunk=args.chunk, **modes[mode])
    if args.profile:
        timed(f"on_G{args.points[-1]}", 8 * args.chunk)
        return
    for rep in range(3):
        for mode in modes:
            print(json.dumps({"case": args.case, "mode": mode, "rep": rep, "steps": args.steps,
                              "nchains": c["nchains"], "ms_per_step": timed(mode, args.steps) * 1e3}), flush=True)
    post = r.blackwell_rao()
    print(json.dumps({"case": args.case, "n": post["BB"]["n"], "state_bytes": r._br.data.numel() * 8,
                      "mass_BB_min": float(post["BB"]["mass"][2:].min()),
                      "mass_BB_max": float(post["BB"]["mass"][2:].max())}))


if __name__ == "__main__":
    main()
