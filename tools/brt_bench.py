"""Time of BlackwellRaoSamples.loglike_t / loglike_grad_t (DESIGN.md 'Blackwell-Rao
likelihood of device theories') against the host routes loglike / loglike_grad of
the same build, fed the same theories: 32 chains x 8192 rows over the Planck-like
low-l set (l <= 30 unbinned TEB, Ju = 116) for K = 1, 64, 1024 theory spectra.
Whole-call times, event-timed, warmed, three runs, the four routes interleaved in
one process; at K = 1 also the replay of a captured graph of each device route.
The host routes take the theory as numpy and return numpy; the device routes take
and return device tensors (what a sampler that keeps its spectra on the device
holds).  One JSON line per measurement."""
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
    ap.add_argument("--ring", type=int, default=32)
    args = ap.parse_args()
    import numpy as np
    import torch
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
        th = torch.from_numpy(theory).cuda()
        routes = {"loglike_ms": lambda: bank.loglike(theory), "loglike_t_ms": lambda: bank.loglike_t(th),
                  "loglike_grad_ms": lambda: bank.loglike_grad(theory), "loglike_grad_t_ms": lambda: bank.loglike_grad_t(th)}
        for fn in routes.values():                              # warm
            fn()
        torch.cuda.synchronize()
        graphs = {}
        if K == 1:
            side = torch.cuda.Stream()
            for name in ("loglike_t", "loglike_grad_t"):
                gr = torch.cuda.CUDAGraph()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    with torch.cuda.graph(gr, stream=side):
                        getattr(bank, name)(th)
                torch.cuda.current_stream().wait_stream(side)
                gr.replay()
                graphs[name + "_graph_ms"] = gr.replay
            torch.cuda.synchronize()
        for rep in range(3):
            rec = {"K": K, "rep": rep, "chains": C, "rows": N, "Ju": bank.Ju}
            outs = {}
            for name, fn in list(routes.items()) + list(graphs.items()):
                rec[name], outs[name] = ev_time(fn)
            hg, dg = outs["loglike_grad_ms"], outs["loglike_grad_t_ms"]
            got = dg["grad"].cpu().numpy()
            want = np.zeros_like(got)
            for k, s in enumerate(SPECTRA[F]):
                want[:, k, :hg["grad"][s].shape[1]] = hg["grad"][s]
            rec.update(loglike_speedup=rec["loglike_ms"] / rec["loglike_t_ms"],
                       grad_speedup=rec["loglike_grad_ms"] / rec["loglike_grad_t_ms"],
                       grad_bit_equal=bool(np.array_equal(got, want)),
                       max_abs_dloglike=float(np.max(np.abs(dg["loglike"].cpu().numpy() - hg["loglike"]))))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
