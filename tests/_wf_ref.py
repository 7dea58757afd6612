"""numpy longdouble restatement of the Rao-Blackwellised posterior sky map
(gs_wf.hip), computed DIRECTLY from stacked D_l samples [k, C, nspec, maxbins]
and the data d [F, (L+1)^2]: the centered operator of DESIGN.md section 5 per
(sample, chain, l), then two-pass means and covariances (no Welford step, no
chain merge), and the first-order rounding bounds of DESIGN.md
'Rao-Blackwellised posterior sky map' that the device results are held to.
The bounds depend on k, C, the magnitudes X = max |x| and D = max |x - pooled
mean| of the series involved and on the operator's own rounding (a fixed count
of operations times its condition) -- never on the code under test."""
import numpy as np

from tests._smap_ref import check, slot_ell  # noqa: F401  (check: the tests' comparison)

LD = np.longdouble
U = 2.0 ** -53
PI = LD(3.14159265358979323846264338327950288)
SPECTRA = {1: ("TT",), 2: ("EE", "BB"), 3: ("TT", "EE", "BB", "TE")}
# operations between the D_l and an operator entry / a Sigma entry rebuilt from its
# Cholesky factor, each a relative rounding of at most u amplified by the condition
# of the 2x2 steps (DESIGN.md derives the counts)
N_OP_BLOCK = 140
N_OP_DIAG = 16
# F = 3: the operator planes (M00, M01, M10, M11, M22), the entries and data rows of a field's series
OPS3 = {0: ((0, 0), (1, 1)), 1: ((2, 0), (3, 1)), 2: ((4, 2),)}


def ell2bin(F, L, bins):
    out = np.full((len(SPECTRA[F]), L + 1), -1, dtype=np.int64)
    for q, s in enumerate(SPECTRA[F]):
        e = np.asarray(bins[s])
        for i in range(len(e) - 1):
            out[q, e[i]:e[i + 1]] = i
    return out


def noise_weights(npix, noise_var):
    return npix / (4.0 * np.pi * np.asarray(noise_var, dtype=np.float64))


def unbinned_var(F, L, bins, stack):
    """stack [k, C, nspec, maxbins] -> the per-l variances [nspec, k, C, L+1]
    (longdouble): D 2 pi / (l (l+1)), l = 0 keeps D_0, an unbinned l reads 0."""
    x = np.asarray(stack, dtype=LD)
    e2b = ell2bin(F, L, bins)
    ell = np.arange(L + 1)
    fac = np.where(ell == 0, LD(1), 2 * PI / np.maximum(ell * (ell + 1), 1).astype(LD))
    out = []
    for q in range(e2b.shape[0]):
        v = x[:, :, q, np.maximum(e2b[q], 0)]
        out.append(np.where(e2b[q] < 0, LD(0), v) * fac)
    return np.stack(out)


def _pinv(v):
    return np.where(v != 0, LD(1) / np.where(v != 0, v, LD(1)), LD(0))


def operator(F, L, bl, kappa, bins, stack):
    """The centered operator per (sample, chain, l): M [nop, k, C, L+1], Sigma
    [nspec, k, C, L+1] in spectrum order (s00, s11, s22, s01 for F = 3) and cond
    [k, C, L+1], the product of the conditions of the 2x2 steps (1 elsewhere).
    Sigma = (C^+ + diag(b^2 kappa))^-1, M = Sigma diag(b kappa); zero-variance rule:
    a zero TT or EE drops the TE coupling and takes zero prior precision."""
    v = unbinned_var(F, L, bins, stack)
    b = np.asarray(bl, dtype=LD)
    kap = [LD(x) for x in kappa]
    if F != 3:
        sig = [LD(1) / (kap[f] * b * b + _pinv(v[f])) for f in range(F)]
        M = [sig[f] * (kap[f] * b) for f in range(F)]
        return np.stack(M), np.stack(sig), np.ones(v.shape[1:])
    tt, ee, bb, te = v
    full = (tt != 0) & (ee != 0)
    det = np.where(full, tt * ee - te * te, LD(1))
    it = np.where(full, ee / det, _pinv(tt))
    ie = np.where(full, tt / det, _pinv(ee))
    ite = np.where(full, -te / det, LD(0))
    q00, q11, q01 = it + b * b * kap[0], ie + b * b * kap[1], ite
    det2 = q00 * q11 - q01 * q01
    s00, s11, s01 = q11 / det2, q00 / det2, -q01 / det2
    s22 = LD(1) / (_pinv(bb) + b * b * kap[2])
    M = np.stack([s00 * (b * kap[0]), s01 * (b * kap[1]), s01 * (b * kap[0]), s11 * (b * kap[1]), s22 * (b * kap[2])])
    k1 = np.where(full, (tt * ee + te * te) / det, LD(1))
    k2 = (q00 * q11 + q01 * q01) / det2
    return M, np.stack([s00, s11, s22, s01]), (k1 * k2 * k2).astype(np.float64)


def data_moments(F, L, d):
    """S_l [nspec, L+1] in spectrum order and the sums of |d_g d_h| (longdouble)."""
    d = np.asarray(d, dtype=LD).reshape(F, -1)
    ell = slot_ell(L)
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1)] if F == 3 else [(f, f) for f in range(F)]
    S, Sabs = np.zeros((len(pairs), L + 1), dtype=LD), np.zeros((len(pairs), L + 1), dtype=LD)
    for q, (g, h) in enumerate(pairs):
        np.add.at(S[q], ell, d[g] * d[h])
        np.add.at(Sabs[q], ell, np.abs(d[g] * d[h]))
    return S, Sabs


def _power_terms(F, M, S):
    """(M S M^T) per spectrum, unnormalised: M [nop, ...], S [nspec, L+1]."""
    if F != 3:
        return np.stack([M[f] * M[f] * S[f] for f in range(F)])
    att, aee, abb, ate = S
    return np.stack([M[0] * M[0] * att + 2 * M[0] * M[1] * ate + M[1] * M[1] * aee,
                     M[2] * M[2] * att + 2 * M[2] * M[3] * ate + M[3] * M[3] * aee,
                     M[4] * M[4] * abb,
                     M[0] * M[2] * att + (M[0] * M[3] + M[1] * M[2]) * ate + M[1] * M[3] * aee])


def _mean(x, axes):
    """Two-pass mean about the first sample: a constant series (the operator of a
    zero-variance l) has exactly zero deviations, as it has on the device."""
    x0 = x[(slice(None),) * min(axes) + (slice(0, 1),) * len(axes)]
    n = np.prod([x.shape[a] for a in axes])
    return (x0 + (x - x0).sum(axis=axes, keepdims=True) / n)


def _series_terms(F, f):
    return OPS3[f] if F == 3 else ((f, f),)


def posterior(F, L, bl, kappa, bins, stack, d):
    """Everything the device returns, in longdouble, plus what the bounds need."""
    M, Sg, cond = operator(F, L, bl, kappa, bins, stack)
    k, C = M.shape[1], M.shape[2]
    N = k * C
    d = np.asarray(d, dtype=LD).reshape(F, -1)
    ell = slot_ell(L)
    S, Sabs = data_moments(F, L, d)
    w2 = (2 * np.arange(L + 1) + 1).astype(LD)
    nan = lambda *shape: np.full(shape, np.nan, dtype=LD)
    # the series of every slot: m [k, C, F, NR]
    m = np.zeros((k, C, F, d.shape[1]), dtype=LD)
    for f in range(F):
        for op, g in _series_terms(F, f):
            m[:, :, f] += M[op][:, :, ell] * d[g]
    mean = _mean(m, (0, 1))[0, 0]
    sig_ff = _mean(Sg[:F], (1, 2))[:, 0, 0][:, ell]
    var = sig_ff + ((m - mean) ** 2).sum(axis=(0, 1)) / (N - 1) if N >= 2 else nan(F, d.shape[1])
    cm = _mean(m, (0,))[0]
    rhat, aux = nan(F, d.shape[1]), {}
    if C > 1 and k >= 2:
        M2c = ((m - cm[None]) ** 2).sum(axis=0)
        W = (M2c / (k - 1)).sum(axis=0) / C
        g0 = (M2c / k).sum(axis=0) / C
        Bn = ((cm - _mean(cm, (0,))[0]) ** 2).sum(axis=0) / (C - 1)
        varp = g0 + Bn
        ok = W > 0
        rhat[ok] = np.sqrt(varp[ok] / W[ok])
        aux = dict(W=W, g0=g0, Bn=Bn, varp=varp)
    op_mean = _mean(M, (1, 2))[:, 0, 0]
    P = Sg + _power_terms(F, M, S) / w2                         # [nspec, k, C, L+1]
    return dict(alm_mean=mean, alm_var=var, chain_alm_mean=cm, alm_rhat=rhat, op_mean=op_mean,
                power_of_mean=_power_terms(F, op_mean, S) / w2, mean_power=_mean(P, (1, 2))[:, 0, 0],
                M=M, Sg=Sg, cond=cond, series=m, S=S, Sabs=Sabs, P=P, **aux)


def _xd(x):
    """X = max |x| and D = max |x - pooled mean| over the samples: x [..., k, C, n] -> [..., n]."""
    mean = _mean(x, (x.ndim - 3, x.ndim - 2))
    return np.abs(x).max(axis=(-3, -2)).astype(np.float64), np.abs(x - mean).max(axis=(-3, -2)).astype(np.float64)


def bounds(F, L, ref, d):
    """Per-element first-order bounds of every output (DESIGN.md derives them).
    eta = N_OP u max cond is the operator's relative rounding; a series x of a
    chain with magnitudes X, D and input perturbation eta X has
      chain mean    E = eta X + k u (X + 6 D)       (Welford with a reciprocal)
      pooled mean   E + (C - 1) u (X + 6 D)         (Chan)
      co-moment (a, b) of a chain
                    2 k (D_a E_b + D_b E_a) + u (12 k + 2 k (k + 1)) D_a D_b + 4 k eta^2 X_a X_b
      pooled        C times that + (C - 1) (4 k (D_a Em_b + D_b Em_a) + (24 k + 2 N) u D_a D_b)"""
    M, Sg, series = ref["M"], ref["Sg"], ref["series"]
    k, C = M.shape[1], M.shape[2]
    N = k * C
    d = np.abs(np.asarray(d, dtype=np.float64).reshape(F, -1))
    ell = slot_ell(L)
    eta = (N_OP_BLOCK if F == 3 else N_OP_DIAG) * U * ref["cond"].max(axis=(0, 1))          # [L+1]
    XM, DM = _xd(M)
    XS, DS = _xd(Sg)
    E = lambda X, D: eta * X + k * U * (X + 6 * D)
    Em = lambda X, D: E(X, D) + (C - 1) * U * (X + 6 * D)
    out = {"op_mean": Em(XM, DM)}
    nr = d.shape[1]
    b_mean, b_cm, b_var, b_rhat = (np.zeros((F, nr)) for _ in range(4))
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    Mbar = np.abs(f64(ref["op_mean"]))
    for f in range(F):
        terms = _series_terms(F, f)
        absmd = sum(Mbar[op][ell] * d[g] for op, g in terms)
        b_mean[f] = sum(Em(XM[op], DM[op])[ell] * d[g] for op, g in terms) + 3 * U * absmd
        absmd_c = sum(XM[op][ell] * d[g] for op, g in terms)
        b_cm[f] = sum(E(XM[op], DM[op])[ell] * d[g] for op, g in terms) + 3 * U * absmd_c
        T = sum(DM[op][ell] * d[g] for op, g in terms)
        e_q = np.zeros(nr)             # a chain's quadratic form of co-moments
        e_Q = np.zeros(nr)             # the pooled one
        for oa, ga in terms:
            for ob, gb in terms:
                Da, Db, Xa, Xb = DM[oa], DM[ob], XM[oa], XM[ob]
                # the last term is second order in the operator's rounding: it is what is left
                # where an operator is constant up to its last bits (deviations below eta X)
                eC = 2 * k * (Da * E(Xb, Db) + Db * E(Xa, Da)) + U * (12 * k + 2 * k * (k + 1)) * Da * Db + \
                    4 * k * (eta * Xa) * (eta * Xb)
                eT = C * eC + (C - 1) * (4 * k * (Da * Em(Xb, Db) + Db * Em(Xa, Da)) + (24 * k + 2 * N) * U * Da * Db)
                e_q += eC[ell] * d[ga] * d[gb]
                e_Q += eT[ell] * d[ga] * d[gb]
        sf = f if F != 3 else (0, 1, 2)[f]
        e_sig = Em(XS[sf], DS[sf])[ell]
        if N >= 2:
            b_var[f] = e_sig + e_Q / (N - 1) + 8 * U * T * T + 2 * U * np.abs(f64(ref["alm_var"][f]))
        else:
            b_var[f] = np.nan
        if C > 1 and k >= 2:
            W, g0, Bn, varp, rh = (f64(ref[key][f]) for key in ("W", "g0", "Bn", "varp", "alm_rhat"))
            Xs, Ds = _xd(series[:, :, f])
            e_qc = e_q + 4 * U * k * T * T
            e_W = e_qc / (k - 1) + (C + 2) * U * W
            e_g0 = e_qc / k + (C + 2) * U * g0
            e_d = 2 * b_cm[f] + C * U * Xs + 2 * U * Ds
            e_sb2 = C * 4 * Ds * e_d + (C + 1) * U * C * 4 * Ds * Ds
            e_varp = e_g0 + e_sb2 / (C - 1) + U * Bn + U * varp
            ok = W > 0
            b_rhat[f] = np.nan
            b_rhat[f][ok] = rh[ok] * (0.5 * (e_varp[ok] / varp[ok] + e_W[ok] / W[ok]) + 2 * U)
            # W not above twice its own rounding bound: the ratio var+ / W is not determined
            # by the data there (an operator that is constant up to its last bits); NaN, the
            # W == 0 outcome, is as valid as any value: marked inf, left out by rhat_mask
            b_rhat[f][(W <= 2 * e_W) & (e_W > 0)] = np.inf
        else:
            b_rhat[f] = np.nan
    out.update(alm_mean=b_mean, chain_alm_mean=np.broadcast_to(b_cm, (C, F, nr)).copy(), alm_var=b_var,
               alm_rhat=b_rhat)
    # powers: the data moments carry (2l + 3) u of their absolute sums
    lw = np.arange(L + 1)
    w2 = 2.0 * lw + 1.0
    Sabs = f64(ref["Sabs"])
    absM = np.abs(f64(M))
    qabs = f64(_power_terms(F, absM.astype(LD), Sabs.astype(LD))) / w2                       # [nspec, k, C, L+1]
    P = ref["P"]
    XP, DP = _xd(P)
    dP = (eta * (np.abs(f64(Sg)) + 2 * qabs) + (2 * lw + 9) * U * qabs + U * np.abs(f64(P))).max(axis=(1, 2))
    out["mean_power"] = dP + k * U * (XP + 6 * DP) + (C - 1) * U * (XP + 6 * DP)
    eM = out["op_mean"]
    # d(M S M^T) <= sum |dM_a| |M_b| |S| + ...: bounded with (|Mbar| + eM) in place of one factor
    grow = f64(_power_terms(F, (Mbar + eM).astype(LD), Sabs.astype(LD))) - f64(_power_terms(F, Mbar.astype(LD), Sabs.astype(LD)))
    pabs = f64(_power_terms(F, Mbar.astype(LD), Sabs.astype(LD)))
    out["power_of_mean"] = (grow + (2 * lw + 9) * U * pabs) / w2
    return out


def synthetic(F, L, k, C, seed=0, nside=8):
    """A synthetic ring and data for the engine tests: bins wider than one l with
    irregular edges (TT, EE and TE share theirs; BB has its own), the top of the
    l range left unbinned, D_l = 0 bins that take both zero-variance branches
    of the TEB block (TT = 0 with EE != 0 in bin 1, EE = 0 with TT != 0 in bin
    2), |TE| <= 0.5 sqrt(TT EE), and data 1e3 + N(0, 1)."""
    rng = np.random.default_rng(seed)
    spectra = SPECTRA[F]
    shared = np.array([e for e in (0, 2, 3, 7, 12, 19, 29, 31, 47, 64) if e < L - 1] + [L - 1])
    own = np.array([e for e in (0, 1, 4, 9, 23, 50) if e < L] + [L])
    bins = {s: (own if s == "BB" else shared) for s in spectra}
    if F == 1:
        bins = {"TT": shared}
    nb = {s: len(bins[s]) - 1 for s in spectra}
    maxbins = max(nb.values())
    stack = np.zeros((k, C, len(spectra), maxbins))
    for q, s in enumerate(spectra):
        if s != "TE":
            stack[:, :, q, :nb[s]] = (0.5 + q) * np.exp(0.3 * rng.standard_normal((k, C, nb[s])))
    if F == 3:
        rho = rng.uniform(-0.5, 0.5, size=(k, C, nb["TE"]))
        stack[:, :, 3, :nb["TE"]] = rho * np.sqrt(stack[:, :, 0, :nb["TE"]] * stack[:, :, 1, :nb["TE"]])
        stack[:, :, 0, 1] = 0.0           # TT = 0, EE != 0 (TE left as drawn: the rule drops it)
        stack[:, :, 1, 2] = 0.0           # EE = 0, TT != 0
        stack[:, :, 2, 1] = 0.0
    else:
        stack[:, :, 0, 1] = 0.0
    ell = np.arange(L + 1)
    bl = np.exp(-0.5 * ell * (ell + 1) * 0.01 ** 2)
    noise_var = {1: [30.0], 2: [20.0, 10.0], 3: [30.0, 20.0, 10.0]}[F]
    d = 1e3 + rng.standard_normal((F, (L + 1) ** 2))
    return dict(F=F, L=L, bins=bins, maxbins=maxbins, stack=stack, bl=bl, noise_var=np.array(noise_var),
                kappa=noise_weights(12 * nside ** 2, noise_var), d=d, nside=nside)


def rhat_mask(got, ref, bound):
    """(got, ref) of an R-hat comparison with the unresolved elements (bound inf)
    set to NaN on both sides, and their number."""
    got, ref = np.array(got, dtype=LD), np.array(ref, dtype=LD).reshape(np.shape(got))
    out = np.isinf(np.asarray(bound, dtype=np.float64).reshape(got.shape))
    got[out] = np.nan
    ref[out] = np.nan
    return got, ref, int(out.sum())
