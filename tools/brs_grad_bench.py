"""Time of one BlackwellRaoSamples.loglike_grad call (DESIGN.md 'Blackwell-Rao
likelihood gradient') at 32 chains x 8192 rows over the Planck-like low-l set (l
<= 30 unbinned TEB, Ju = 116) for K = 1, 64, 1024 theory spectra, against the
only route to the derivative without it: central differences through loglike on
2 Ju perturbed theories per model (K = 1 and 64; at K = 1024 that is 237,568
models, whose per-slice workspace alone is 5.8 GB and whose host tables take
minutes -- left out).  Event-timed, warmed, three runs each, interleaved in one
process.  call_ms and cd_ms span the whole call, host tables and chain rule
included; device_ms is the device part of loglike_grad with the tables on the
device (evaluate + finish, the second pass, its finish), num_ms the second pass
alone (k_brs_grad + combine).  One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--lmax", type=int, default=30)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--cd-models", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--step", type=float, default=1e-4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd import _capi as CA
    from gibbssampler_amd.engine import SPECTRA, BlackwellRaoSamples, br_likelihood_mask

    F, C, N = 3, args.chains, args.rows
    bins = {s: np.arange(0, args.lmax + 2) for s in SPECTRA[F]}
    mask = br_likelihood_mask(F, bins)
    nspec, maxbins = mask.shape
    rng = np.random.default_rng(0)
    # the bank of tools/brs_eval_bench.py
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
    del hist, jit
    assert bank.n == N and bank.Ju == int(mask.sum())
    used = [(int(c) // maxbins, int(c) % maxbins) for c in bank.cols.cpu().numpy()]
    lib = bank.lib

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
        tab = bank.tables(theory)
        Y = torch.from_numpy(tab["Y"]).cuda()
        cst = torch.from_numpy(tab["cst"]).cuda()
        ll = torch.zeros(K, dtype=torch.float64, device="cuda")
        cl = torch.zeros(C, K, dtype=torch.float64, device="cuda")
        ne = torch.zeros(K, dtype=torch.float64, device="cuda")
        xbar = torch.zeros(K, bank.Ju, dtype=torch.float64, device="cuda")
        cw = torch.zeros(C, K, dtype=torch.float64, device="cuda")
        keep = {}

        def pass1():
            state = bank.evaluate(Y)
            CA.check(lib.gs_brl_finish(CA.ptr(state), C, K, CA.ptr(cst), CA.ptr(ll), CA.ptr(cl), CA.ptr(ne),
                                       CA.stream_ptr()), "gs_brl_finish")
            keep["state"] = state
            keep["mref"] = bank.fields(state)[0].amax(dim=0)    # every chain holds samples here
            return state

        def pass2():
            keep["num"] = bank.grad_numerators(Y, keep["mref"])
            return keep["num"]

        def device():
            pass1()
            pass2()
            CA.check(lib.gs_brs_grad_finish(CA.ptr(keep["num"]), CA.ptr(keep["state"]), C, K, bank.Ju, CA.ptr(xbar),
                                            CA.ptr(cw), CA.stream_ptr()), "gs_brs_grad_finish")
            return xbar

        def call():
            return bank.loglike_grad(theory)

        def central():
            h = args.step
            th = np.repeat(theory, 2 * bank.Ju, axis=0).reshape(K, bank.Ju, 2, nspec, maxbins)
            for j, (sp, b) in enumerate(used):
                th[:, j, 0, sp, b] *= 1.0 + h
                th[:, j, 1, sp, b] *= 1.0 - h
            f = bank.loglike(th.reshape(-1, nspec, maxbins))["loglike"].reshape(K, bank.Ju, 2)
            out = np.zeros((K, nspec, maxbins))
            for j, (sp, b) in enumerate(used):
                out[:, sp, b] = (f[:, j, 0] - f[:, j, 1]) / (2.0 * h * theory[:, sp, b])
            return out

        cd = K in args.cd_models
        device(), call()                                        # warm
        if cd:
            central()
        torch.cuda.synchronize()
        for rep in range(3):
            t1, _ = ev_time(pass1)
            t2, _ = ev_time(pass2)
            td, _ = ev_time(device)
            tc, out = ev_time(call)
            flop = 2.0 * C * N * bank.Jp * K
            rec = {"K": K, "rep": rep, "chains": C, "rows": N, "Ju": bank.Ju, "eval_ms": t1, "num_ms": t2,
                   "device_ms": td, "call_ms": tc, "num_TFLOPs_two_contractions": 2.0 * flop / t2 * 1e-9,
                   "num_Gexp_per_s": C * N * K / t2 * 1e-6, "eval_TFLOPs": flop / t1 * 1e-9}
            if cd:
                tcd, want = ev_time(central)
                got = np.zeros_like(want)
                for k, s in enumerate(SPECTRA[F]):
                    got[:, k, :out["grad"][s].shape[1]] = out["grad"][s]
                scale = np.abs(want).max(axis=(1, 2), keepdims=True)
                rec.update(cd_ms=tcd, cd_models=2 * bank.Ju * K, cd_over_call=tcd / tc,
                           max_rel_diff=float(np.max(np.abs(got - want) / scale)))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
