"""Gaussianised Blackwell-Rao likelihood: the fit and the evaluator on one GPU
(DESIGN.md 'Gaussianised Blackwell-Rao likelihood').  A synthetic EB bank of
--chains x --rows rows (unbinned, lrange (2, --lmax)), event-timed after one
warm-up, three runs, each interleaved with the route a user would otherwise
write: the same Hermite transform in torch ops and x^T x per chain through
torch's fp64 batched GEMM.  With --agree the exact bank estimator and the
Gaussianised one are compared on loglike differences between a few theories.
One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_bank(torch, chains, rows, lmax, seed=20261021):
    from gibbssampler_amd.engine import BlackwellRaoSamples, br_likelihood_mask, gbr_columns
    bins = {s: np.arange(0, lmax + 3) for s in ("EE", "BB")}
    mask = br_likelihood_mask(2, bins, None, (2, lmax))
    bank = BlackwellRaoSamples(chains, 2, bins, mask, rows, draws=True)
    col = gbr_columns(2, bins, mask)
    g = torch.Generator(device="cuda").manual_seed(seed)
    alpha = torch.from_numpy(col["alpha"]).cuda()
    shape = (chains, rows, bank.Ju)
    # beta ~ Gamma(alpha + 3) (a posterior-like spread of the scales), D = beta / Gamma(alpha)
    beta = torch._standard_gamma((alpha + 3.0).expand(shape).contiguous(), generator=g)
    draw = beta / torch._standard_gamma(alpha.expand(shape).contiguous(), generator=g)
    bank.X[:, :, :bank.Ju] = beta
    bank.Dl[:, :, :bank.Ju] = draw
    bank.r.copy_((bank.coef * torch.log(beta)).sum(dim=2))
    bank._n = rows
    return bank, col


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def torch_route(torch, bank, gbr, gl):
    """x = T(Dl) with torch ops, then S1 and S2 per chain with torch's fp64 GEMM."""
    n, G = bank.n, gbr.G
    D = bank.Dl[:, :n][:, :, gl]
    u = (torch.log(D) - gbr.glo) / gbr.gh
    k = u.floor().clamp(1, G - 3).long()
    t = u - k
    j = torch.arange(gbr.Jg, device=D.device).expand_as(k)
    y0, s0, y1, s1 = gbr.tx[j, k, 0], gbr.tx[j, k, 1], gbr.tx[j, k + 1, 0], gbr.tx[j, k + 1, 1]
    omt = 1 - t
    x = (1 + 2 * t) * omt * omt * y0 + t * omt * omt * s0 + t * t * (3 - 2 * t) * y1 + t * t * (t - 1) * s1
    return x.sum(dim=1), torch.bmm(x.transpose(1, 2), x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--lmax", type=int, default=30)
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--agree", action="store_true")
    args = ap.parse_args()
    import torch
    from gibbssampler_amd import _capi as C
    bank, col = make_bank(torch, args.chains, args.rows, args.lmax)
    lib = C.load()
    gl = torch.from_numpy(col["gcol"]).cuda().long()
    gcol = torch.from_numpy(col["gcol"]).cuda()
    base = {"chains": args.chains, "rows": args.rows, "lrange": [2, args.lmax]}
    gbr = bank.gaussianize()                                   # warm-up
    Jg, G, n = gbr.Jg, gbr.G, bank.n
    nb, br, ct = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    C.check(lib.gs_gbr_info(n, Jg, ctypes.byref(nb), ctypes.byref(br), ctypes.byref(ct)), "gs_gbr_info")
    base.update(Jg=Jg, G=G, row_blocks=nb.value, block_rows=br.value)
    f64 = torch.float64
    alpha, half = torch.from_numpy(col["alpha"]).cuda(), torch.from_numpy(col["half"]).cuda()
    m = torch.zeros(args.chains, Jg, G, dtype=f64, device="cuda")
    S = torch.zeros_like(m)
    cnt = torch.zeros(args.chains, dtype=torch.int64, device="cuda")
    wb = ctypes.c_longlong()
    C.check(lib.gs_gbr_moments_work_bytes(args.chains, n, Jg, ctypes.byref(wb)), "gs_gbr_moments_work_bytes")
    work = torch.empty(wb.value // 8, dtype=f64, device="cuda")
    S1 = torch.zeros(args.chains, Jg, dtype=f64, device="cuda")
    S2 = torch.zeros(args.chains, Jg, Jg, dtype=f64, device="cuda")
    st = C.stream_ptr()

    def marg():
        C.check(lib.gs_gbr_marginals(C.ptr(bank.X), C.ptr(bank.r), args.chains, bank.capacity, n, bank.Ju, Jg, C.ptr(gcol),
                                     C.ptr(alpha), C.ptr(half), C.ptr(gbr.glo), C.ptr(gbr.gh), G, C.ptr(m), C.ptr(S),
                                     C.ptr(cnt), st), "gs_gbr_marginals")

    def moments():
        C.check(lib.gs_gbr_moments(C.ptr(bank.Dl), C.ptr(bank.r), args.chains, bank.capacity, n, bank.Ju, Jg, C.ptr(gcol),
                                   C.ptr(gbr.tx), C.ptr(gbr.glo), C.ptr(gbr.gh), G, C.ptr(work), wb.value, C.ptr(S1),
                                   C.ptr(S2), st), "gs_gbr_moments")

    med = bank.Dl[:, :n][:, :, gl].reshape(-1, Jg).median(dim=0).values
    theory = torch.ones(args.models, bank.nspec, bank.maxbins, dtype=f64, device="cuda")
    fac = torch.linspace(0.9, 1.1, args.models, dtype=f64, device="cuda")
    theory.view(args.models, -1)[:, torch.from_numpy(col["tcol"]).cuda().long()] = med[None, :] * fac[:, None]
    marg(), moments(), torch_route(torch, bank, gbr, gl), gbr.loglike_t(theory)      # warm-up
    torch.cuda.synchronize()
    for rep in range(3):
        for name, fn in (("gaussianize", lambda: bank.gaussianize()), ("k_gbr_marg", marg),
                         ("k_gbr_moments+combine", moments), ("torch_transform+bmm", lambda: torch_route(torch, bank, gbr, gl)),
                         ("loglike_t", lambda: gbr.loglike_t(theory))):
            ms, _ = timed(torch, fn)
            extra = {}
            if name == "k_gbr_marg":
                extra = {"exp_per_s": args.chains * n * Jg * G / (ms * 1e-3)}
            if name in ("k_gbr_moments+combine", "torch_transform+bmm"):
                extra = {"tflops_full_gemm": 2.0 * args.chains * n * Jg * Jg / (ms * 1e-3) * 1e-12}
            if name == "loglike_t":
                extra = {"models": args.models}
            print(json.dumps(dict(base, what=name, rep=rep, ms=ms, **extra)), flush=True)
    s1t, s2t = torch_route(torch, bank, gbr, gl)
    moments()
    torch.cuda.synchronize()
    print(json.dumps(dict(base, what="fused against torch", max_rel_S2=float(((S2 - s2t).abs().max() / s2t.abs().max())),
                          max_abs_S1=float((S1 - s1t).abs().max()))), flush=True)
    if args.agree:
        K = 5
        th = theory[:: args.models // K][:K].contiguous()
        exact = bank.loglike_t(th)
        gau = gbr.loglike_t(th)
        ex, ga = exact["loglike"].cpu().numpy(), gau["loglike"].cpu().numpy()
        print(json.dumps(dict(base, what="estimator agreement", factors=[float(v) for v in fac[:: args.models // K][:K].cpu()],
                              exact_dloglike=[float(v) for v in ex - ex[K // 2]],
                              gaussianised_dloglike=[float(v) for v in ga - ga[K // 2]],
                              exact_neff=[float(v) for v in exact["neff"].cpu()])), flush=True)


if __name__ == "__main__":
    main()
