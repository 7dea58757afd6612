"""Time of one BlackwellRaoSamples.loglike call (DESIGN.md 'Blackwell-Rao sample
bank') at 32 chains x 8192 rows over the Planck-like low-l set (l <= 30
unbinned TEB, Ju = 116) for K = 1, 64, 1024 theory spectra, against the route
that exists without the bank: the same rows re-fed through a 32-slot scale ring
into BlackwellRaoLikelihood.update + finish.  Event-timed, warmed, three runs
each, interleaved in one process.  The timed region of both routes starts with
the tables on the device (evaluate / update ... finish); the host's table
construction (br_likelihood_tables) is reported apart.  One JSON line per
measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--lmax", type=int, default=30)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--ring", type=int, default=32)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd import _capi as CA
    from gibbssampler_amd.engine import SPECTRA, BlackwellRaoLikelihood, BlackwellRaoSamples, br_likelihood_mask

    F, C, N = 3, args.chains, args.rows
    bins = {s: np.arange(0, args.lmax + 2) for s in SPECTRA[F]}
    mask = br_likelihood_mask(F, bins)
    nspec, maxbins = mask.shape
    rng = np.random.default_rng(0)
    # scales near n_b D / 2 of a smooth fiducial, blocks with a correlation of 0.3
    l0 = np.arange(maxbins, dtype=np.float64)
    nb = (l0 + 1) ** 2 - l0 ** 2
    fid = np.stack([1e3 / (l0 + 1), 1.0 / (l0 + 1), 0.1 / (l0 + 1), np.zeros(maxbins)])
    fid[3] = 0.3 * np.sqrt(fid[0] * fid[1])
    hist = torch.empty(N, C, nspec, maxbins, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    jit = 1.0 + torch.randn(N, C, nspec, maxbins, dtype=torch.float64, device="cuda", generator=g) / \
        torch.from_numpy(np.sqrt(np.maximum(nb, 1.0))).cuda()
    hist.copy_(torch.from_numpy(nb * fid).cuda() * jit.abs())
    hist[:, :, 3] = 0.3 * torch.sqrt(hist[:, :, 0] * hist[:, :, 1])
    bank = BlackwellRaoSamples(C, F, bins, mask, N)
    for i in range(0, N, args.ring):
        bank.append(hist[i:i + args.ring], args.ring, i + 1, min(args.ring, N - i))
    torch.cuda.synchronize()
    assert bank.n == N and bank.Ju == int(mask.sum())
    ring = torch.empty(args.ring, C, nspec, maxbins, dtype=torch.float64, device="cuda")

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for K in args.models:
        amp = 1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=K)
        theory = amp[:, None, None] * fid[None]
        t0 = time.perf_counter()
        tab = bank.tables(theory)
        host_ms = (time.perf_counter() - t0) * 1e3
        Y = torch.from_numpy(tab["Y"]).cuda()
        cst = torch.from_numpy(tab["cst"]).cuda()
        st = BlackwellRaoLikelihood(C, nspec, maxbins, tab)
        lib = bank.lib
        ll = torch.zeros(K, dtype=torch.float64, device="cuda")
        cl = torch.zeros(C, K, dtype=torch.float64, device="cuda")
        ne = torch.zeros(K, dtype=torch.float64, device="cuda")

        def bank_route():
            state = bank.evaluate(Y)
            CA.check(lib.gs_brl_finish(CA.ptr(state), C, K, CA.ptr(cst), CA.ptr(ll), CA.ptr(cl), CA.ptr(ne),
                                       CA.stream_ptr()), "gs_brl_finish")
            return ll.clone()

        def refeed_route():
            st.reset()
            for i in range(0, N, args.ring):
                k = min(args.ring, N - i)
                ring[:k].copy_(hist[i:i + k])
                st.update(ring, args.ring, 1, k)                # the chunk sits in slots 0 .. k - 1
            return st.finish()["loglike"].clone()

        bank_route(), refeed_route()                            # warm
        torch.cuda.synchronize()
        for rep in range(3):
            tb, a = ev_time(bank_route)
            tr, b = ev_time(refeed_route)
            rec = {"K": K, "rep": rep, "chains": C, "rows": N, "Ju": bank.Ju, "bank_ms": tb, "refeed_ms": tr,
                   "host_tables_ms": host_ms, "max_abs_diff": float((a - b).abs().max()),
                   "bank_GBps": bank.nbytes(N) / tb * 1e-6,
                   "bank_TFLOPs": 2.0 * C * N * bank.Jp * K / tb * 1e-9, "bank_Gexp_per_s": C * N * K / tb * 1e-6}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
