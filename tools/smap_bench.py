"""Cost of the streaming sky-map posterior (gs_smap.hip, run(skymap_summary=)).

1. engine.SkymapMoments.update (k_smap_update) against the torch expression of
   the same Welford step on the same tensors, at [32, 2 * 1025^2] (N_side 512,
   32 chains, EB) and [16, 2 * 513^2]: interleaved, three runs each, device
   events around a window of back-to-back calls after a warm-up.  The kernel
   moves 40 B per element (3 loads + 2 stores of 8 B); bytes/s is that count
   over the time per call, for both variants (the torch expression moves more:
   its temporaries are its cost).
2. bench.py's masked_asis workload (its own set-up and warm-up) timed with and
   without skymap_summary=True set through the runner, interleaved.

  python tools/smap_bench.py [--out profiles/smap_bench.json] [--nchains 16] [--steps 10]

One JSON line per measurement is appended to --out and printed."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12          # MI355X HBM3E peak, bytes/s
HBM_COPY = 6.29e12         # measured float4 copy on the same chip
SHAPES = ((32, 2 * 1025 ** 2), (16, 2 * 513 ** 2))


def torch_step(mean, M2, x, k):
    d = x - mean
    mean += d / k
    M2 += d * (x - mean)


def time_calls(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def bench_update(emit):
    import torch
    from gibbssampler_amd.engine import SkymapMoments
    for C, n in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(C)
        x = torch.randn((C, n), dtype=torch.float64, device="cuda", generator=g)
        st = SkymapMoments(C, n)
        mean, M2 = torch.zeros_like(x), torch.zeros_like(x)
        # same results first (same seeded input, one step each)
        st.update(x)
        torch_step(mean, M2, x, 1.0)
        same = bool(torch.equal(st.fields()[0], mean)) and bool(torch.equal(st.fields()[1], M2))
        variants = {"kernel": (lambda i: st.update(x, count_after=i + 2), 300),
                    "torch": (lambda i: torch_step(mean, M2, x, float(i + 2)), 60)}
        for fn, _ in variants.values():                 # warm-up of both
            for i in range(5):
                fn(i)
        sec = {k: [] for k in variants}
        for run in range(3):
            for name, (fn, reps) in variants.items():
                t = time_calls(fn, reps)
                sec[name].append(t)
                byts = 40.0 * C * n
                emit({"what": "update", "variant": name, "shape": [C, n], "run": run, "calls": reps,
                      "ms_per_call": round(t * 1e3, 4), "algorithmic_bytes_per_call": byts,
                      "bytes_per_s": round(byts / t, 1), "frac_of_hbm_spec_peak": round(byts / t / HBM_SPEC, 4),
                      "frac_of_hbm_measured_copy": round(byts / t / HBM_COPY, 4), "bound": "HBM bandwidth",
                      "first_step_bits_equal_torch": same})
        emit({"what": "update_summary", "shape": [C, n], "kernel_ms_median": round(sorted(sec["kernel"])[1] * 1e3, 4),
              "torch_ms_median": round(sorted(sec["torch"])[1] * 1e3, 4),
              "torch_over_kernel": round(sorted(sec["torch"])[1] / sorted(sec["kernel"])[1], 3)})
        del st, mean, M2, x
        torch.cuda.empty_cache()


def bench_masked_asis(emit, nchains, steps):
    import numpy as np
    import torch
    import bench
    from gibbssampler_amd.distributed import ShardContext
    sys.argv = ["bench.py", "--no-cpu-baseline", "--workload", "masked_asis", "--nchains", str(nchains),
                "--steps", str(steps), "--warmup", "1"]
    args = bench.parse()
    ctx = ShardContext(args.nchains, backend="nccl")
    try:
        runner, go, _, what, _ = bench.masked_head_setup(args, ctx)
        B = args.nchains
        h = go()[0]                                      # bench.py's timed call, here the warm-up of both variants
        last_of = lambda h: ({s: h[s][-1] for s in h} if B == 1 else
                             [{s: h[s][-1][b] for s in h} for b in range(B)])
        last = last_of(h)
        runner.run(last, 1, s_init=runner.s, skymap_summary=True)
        for run in range(3):
            for name, kw in (("without", {}), ("with", {"skymap_summary": True})):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = runner.run(last, args.steps, s_init=runner.s, **kw)[0]
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                last = last_of(h)
                emit({"what": "bench masked_asis", "skymap_summary": name, "run": run, "nside": args.nside,
                      "lmax": args.lmax, "chains": B, "steps": args.steps, "ms_per_step": round(el / args.steps * 1e3, 3),
                      "chain_iterations_per_s": round(args.steps * B / el, 4), "workload": what})
        out = runner.skymap_summary()
        # this workload keeps the reference's re-centring (ASIS.py:203) in front of an
        # over-relaxed CR that starts from the re-centred map, so its maps drift: the
        # figures wanted from it are the times; whether the moments stayed finite is recorded
        rh = out["alm_rhat"][np.isfinite(out["alm_rhat"])]
        emit({"what": "bench masked_asis result", "n": out["n"], "map_finite": bool(torch.isfinite(runner.s).all()),
              "alm_var_finite": bool(np.all(np.isfinite(out["alm_var"]))),
              "max_rhat": float(rh.max()) if rh.size else None})
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smap_bench.json"))
    ap.add_argument("--nchains", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-bench", action="store_true", help="only the update timing")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("smap_bench: needs the GPU (no time is reported without one)")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        bench_update(emit)
        if not a.skip_bench:
            bench_masked_asis(emit, a.nchains, a.steps)


if __name__ == "__main__":
    main()
