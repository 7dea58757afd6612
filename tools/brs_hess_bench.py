"""Time of one BlackwellRaoSamples.loglike_hess call (DESIGN.md 'Blackwell-Rao
likelihood Hessian') at 32 chains x 8192 rows over the Planck-like low-l set (l
<= 30 unbinned TEB, Ju = 116) for K = 1 and 16 theory spectra, against the only
route to the curvature without it: central differences through loglike_grad on
2 Ju perturbed theories per model.  Event-timed, warmed, three runs each,
interleaved in one process.  call_ms and cd_ms span the whole call, host tables
and chain rule included; hess_ms is the Hessian pass alone (k_brh_gram + combine),
its rate counted over the 2 n Ju^2 C K flop of the weighted Gram.  One JSON line
per measurement."""
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
    ap.add_argument("--models", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--ring", type=int, default=32)
    ap.add_argument("--step", type=float, default=1e-4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gibbssampler_amd.engine import SPECTRA, BlackwellRaoSamples, br_likelihood_mask

    F, C, N = 3, args.chains, args.rows
    bins = {s: np.arange(0, args.lmax + 2) for s in SPECTRA[F]}
    mask = br_likelihood_mask(F, bins)
    nspec, maxbins = mask.shape
    rng = np.random.default_rng(0)
    # the bank of tools/brs_grad_bench.py
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
    Ju = bank.Ju

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
        keep = {}

        def call():
            return bank.loglike_hess(theory)

        def grad_call():
            out, g = bank._grad_pass(theory, None)
            keep.update(g)
            return out

        def hess_pass():
            return bank.hess_numerators(keep["Y"], keep["mref"], keep["xbar"])

        def central():
            h = args.step
            th = np.repeat(theory, 2 * Ju, axis=0).reshape(K, Ju, 2, nspec, maxbins)
            for j, (sp, b) in enumerate(used):
                th[:, j, 0, sp, b] *= 1.0 + h
                th[:, j, 1, sp, b] *= 1.0 - h
            gr = bank.loglike_grad(th.reshape(-1, nspec, maxbins))["grad"]
            full = np.zeros((K * Ju * 2, nspec, maxbins))
            for k, s in enumerate(SPECTRA[F]):
                full[:, k, :gr[s].shape[1]] = gr[s]
            ga = full.reshape(K, Ju, 2, -1)[:, :, :, bank.cols.cpu().numpy().astype(np.int64)]   # [K, b, +-, a]
            out = np.zeros((K, Ju, Ju))
            for j, (sp, b) in enumerate(used):
                out[:, :, j] = (ga[:, j, 0] - ga[:, j, 1]) / (2.0 * h * theory[:, sp, b])[:, None]
            return out

        call(), grad_call(), hess_pass(), central()               # warm
        torch.cuda.synchronize()
        for rep in range(3):
            tg, _ = ev_time(grad_call)
            th_, _ = ev_time(hess_pass)
            tc, out = ev_time(call)
            tcd, want = ev_time(central)
            flop = 2.0 * C * N * Ju * Ju * K
            scale = np.abs(want).max(axis=(1, 2), keepdims=True)
            rec = {"K": K, "rep": rep, "chains": C, "rows": N, "Ju": Ju, "grad_call_ms": tg, "hess_ms": th_,
                   "call_ms": tc, "hess_TFLOPs": flop / th_ * 1e-9, "cd_ms": tcd, "cd_models": 2 * Ju * K,
                   "cd_over_call": tcd / tc, "max_rel_diff": float(np.max(np.abs(out["hess"] - want) / scale))}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
