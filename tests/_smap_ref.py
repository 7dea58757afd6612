"""numpy longdouble restatement of the sky-map moments (gs_smap.hip): the pooled
mean and variance, the per-chain means, R-hat and the per-l powers, computed
DIRECTLY from a stacked [k, C, n] array of samples (two-pass sums, no Welford
step and no chain merge), and the first-order rounding bounds of DESIGN.md
'Posterior sky map' that the device results are held to."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def moments(stack):
    """stack [k, C, n] -> {mean, var, rhat [n], chain_mean [C, n]} (longdouble).
    var is NaN when C k < 2; rhat is NaN for C = 1, k < 2 or W == 0."""
    x = np.asarray(stack, dtype=LD)
    k, C, n = x.shape
    N = k * C
    flat = x.reshape(N, n)
    mean = flat.sum(axis=0) / N
    var = ((flat - mean) ** 2).sum(axis=0) / (N - 1) if N >= 2 else np.full(n, np.nan, dtype=LD)
    cm = x.sum(axis=0) / k
    rhat = np.full(n, np.nan, dtype=LD)
    aux = {}
    if C > 1 and k >= 2:
        M2c = ((x - cm[None]) ** 2).sum(axis=0)
        W = (M2c / (k - 1)).sum(axis=0) / C
        g0 = (M2c / k).sum(axis=0) / C
        m = cm.sum(axis=0) / C
        Bn = ((cm - m) ** 2).sum(axis=0) / (C - 1)
        varp = g0 + Bn
        ok = W > 0
        rhat[ok] = np.sqrt(varp[ok] / W[ok])
        aux = dict(W=W, g0=g0, Bn=Bn, varp=varp)
    return dict(mean=mean, var=var, chain_mean=cm, rhat=rhat, **aux)


def bounds(stack, ref=None):
    """Per-element first-order bounds (DESIGN.md 'Posterior sky map'): they depend
    on k, C and the data's magnitude only -- X = max |x| and D = max |x - pooled
    mean| of the element over all samples -- never on the code under test."""
    x = np.asarray(stack, dtype=LD)
    k, C, n = x.shape
    N = k * C
    ref = moments(stack) if ref is None else ref
    X = np.abs(x).max(axis=(0, 1)).astype(np.float64)
    D = np.abs(x - ref["mean"]).max(axis=(0, 1)).astype(np.float64)
    e_cm = k * U * (X + 4 * D)
    e_M2 = U * (4 * k * k * D * (X + 4 * D) + 8 * k * D * D + 2 * k * (k + 1) * D * D)
    e_m = e_cm + (C - 1) * U * (X + 6 * D)
    e_Mtot = C * e_M2 + (C - 1) * (8 * D * k * e_m + 24 * U * D * D * k + 2 * U * N * D * D)
    out = dict(mean=e_m, chain_mean=np.broadcast_to(e_cm, (C, n)).copy(), X=X, D=D)
    out["var"] = e_Mtot / (N - 1) + 4 * U * D * D if N >= 2 else np.full(n, np.nan)
    e_rhat = np.full(n, np.nan)
    if C > 1 and k >= 2:
        f = lambda a: np.asarray(a, dtype=np.float64)
        W, g0, Bn, varp, rhat = f(ref["W"]), f(ref["g0"]), f(ref["Bn"]), f(ref["varp"]), f(ref["rhat"])
        e_W = e_M2 / (k - 1) + (C + 2) * U * W
        e_g0 = e_M2 / k + (C + 2) * U * g0
        e_d = 2 * e_cm + C * U * X + 2 * U * D
        e_sb2 = C * 4 * D * e_d + (C + 1) * U * C * 4 * D * D
        e_varp = e_g0 + e_sb2 / (C - 1) + U * Bn + U * varp
        ok = W > 0
        e_rhat[ok] = rhat[ok] * (0.5 * (e_varp[ok] / varp[ok] + e_W[ok] / W[ok]) + 2 * U)
    out["rhat"] = e_rhat
    return out


def slot_ell(L):
    """multipole of every slot of the real m-major layout."""
    out = np.empty((L + 1) ** 2, dtype=np.int64)
    out[:L + 1] = np.arange(L + 1)
    for m in range(1, L + 1):
        for ell in range(m, L + 1):
            r = 2 * (m * (2 * L + 1 - m) // 2 + ell) - (L + 1)
            out[r] = out[r + 1] = ell
    return out


def power(mean, var, L):
    """mean, var [F, (L+1)^2] -> (power_of_mean, mean_power) [F, L+1], longdouble."""
    mean, var = np.asarray(mean, dtype=LD), np.asarray(var, dtype=LD)
    ell = slot_ell(L)
    F = mean.shape[0]
    pom, vs = np.zeros((F, L + 1), dtype=LD), np.zeros((F, L + 1), dtype=LD)
    for f in range(F):
        np.add.at(pom[f], ell, mean[f] ** 2)
        np.add.at(vs[f], ell, var[f])
    w = (2 * np.arange(L + 1) + 1).astype(LD)
    return pom / w, (pom + vs) / w


def power_bounds(pom, mp, L):
    """(2l+1) non-negative terms per sum, one division, one more add:
    (2l + 4) u |power_of_mean| and (2l + 6) u |mean_power|."""
    ell = np.arange(L + 1)
    return (2 * ell + 4) * U * np.abs(np.asarray(pom, dtype=np.float64)), \
        (2 * ell + 6) * U * np.abs(np.asarray(mp, dtype=np.float64))


def check(name, got, ref, bound):
    """|got - ref| <= bound elementwise (exact where the bound is 0; NaN where
    the reference is NaN); returns the largest observed / bound ratio."""
    got = np.asarray(got, dtype=LD)
    ref = np.asarray(ref, dtype=LD).reshape(got.shape)
    bound = np.asarray(bound, dtype=np.float64).reshape(got.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN pattern"
    err = np.abs(got - ref)[~nan].astype(np.float64)
    b = bound[~nan]
    assert np.all(err[b == 0] == 0), f"{name}: inexact where the bound is 0"
    ratio = float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0
    assert ratio <= 1.0, f"{name}: observed / bound = {ratio}"
    return ratio
