"""CPU: the sanity condition of the Gaussianised Blackwell-Rao surface test on the
oracle's centered chain (oracle/reference_eb.py), numpy only.

The l_max 16 / N_side 8 EB golden problem, 4 chains x 200 iterations, lrange (2,
12): the restatement (tests/_gbr.py) fits mu and cov of the transformed draws
from the chain's D_l and inverse-Gamma scales, and the condition 0.5 < C_jj < 2,
|mu_j| < 0.5 is printed with its margins.  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import harmonic as H  # noqa: E402
from oracle import reference_eb as RE  # noqa: E402
from tests import _gbr as GB  # noqa: E402
from tests._golden import init_of, load, model_from  # noqa: E402


def chain(model, init, n_iter, seed):
    """(D [n_iter, Jg], beta [n_iter, Jg], alpha [Jg]) over the bins wholly in l = 2 .. 12."""
    np.random.seed(seed)
    binned = {s: np.asarray(init[s], dtype=np.float64) for s in model.spectra}
    RE.cr_centered(model, model.unfold(binned))
    use = {s: np.flatnonzero((model.bins[s][:-1] >= 2) & (model.bins[s][1:] - 1 <= 12)) for s in model.spectra}
    Ds, Bs, alpha = [], [], None
    for _ in range(n_iter):
        skymap = RE.cr_centered(model, model.unfold(binned))
        stats = H.sweep_stats(model, skymap, model.d_alm)
        chat = H.centered_betas(model, stats["ss"])
        ab = {s: H.invgamma_params(model, s, chat[s]) for s in model.spectra}
        var = {s: RE.draw_invgamma(model, s) for s in model.spectra}
        binned = H.centered_cls_draw(model, stats, variates=var)
        Ds.append(np.concatenate([binned[s][use[s]] for s in model.spectra]))
        Bs.append(np.concatenate([ab[s][1][use[s]] for s in model.spectra]))
        alpha = np.concatenate([ab[s][0][use[s]] for s in model.spectra])
    return np.array(Ds), np.array(Bs), alpha


def main():
    from gibbssampler_amd.engine import GBR_POINTS, GBR_SPAN, gbr_grid
    g = load(16)
    model, init = model_from(g), init_of(g)
    runs = [chain(model, init, 200, 100 + c) for c in range(4)]
    D, beta, alpha = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), runs[0][2]
    good = np.ones(D.shape[:2], dtype=bool)
    glo, gh = gbr_grid(D.min(axis=(0, 1)), D.max(axis=(0, 1)), GBR_POINTS, *GBR_SPAN)
    logp, _, N = GB.marginals(beta, good, alpha, glo, gh, GBR_POINTS)
    x, sx, sp, mass = GB.tables(logp, glo, gh)
    xd, inside, _ = GB.transform(D, glo, gh, np.stack([x, sx], axis=-1))
    cnt, S1, S2 = GB.moments(xd, good)
    N, mu, cov = GB.finish(cnt, S1, S2)
    mu, dg = mu.astype(np.float64), np.diag(cov).astype(np.float64)
    print(json.dumps({"what": "gbr surface sanity on the oracle's centered chain", "nside": model.nside, "lmax": model.L,
                      "chains": 4, "iterations": 200, "Jg": int(len(alpha)), "N": int(N), "inside": bool(inside.all()),
                      "max_abs_mu": float(np.abs(mu).max()), "min_diag_cov": float(dg.min()),
                      "max_diag_cov": float(dg.max()), "max_abs_mass_minus_1": float(np.abs(mass - 1).max()),
                      "holds": bool(np.abs(mu).max() < 0.5 and dg.min() > 0.5 and dg.max() < 2.0)}))


if __name__ == "__main__":
    main()
