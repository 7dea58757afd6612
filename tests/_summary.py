"""Test-side restatement of the streaming posterior summaries (numpy, fp64):
the update recursion and the finish of gibbssampler_amd/csrc/gs_summary.hip,
in the same algebraic form and operation order as its header comment.

State of C chains x nsb (spectrum, bin) pairs after n samples, per series:
    r      the first sample             y_t = x_t - r
    mean, M2   Welford:  d = x_t - mean; mean += d / t; M2 += d (x_t - mean)
    mn, mx     min / max
    S      sum y_t
    P[j-1] sum_{t > j} y_t y_{t-j},  j = 1..K
    head[i] = y_{i+1}  (the first K values),  ring[i] = y_{n-i}  (the last K, 0 newest)

Finish, over the chains c of one (spectrum, bin):
    s_c^2 = M2_c / (n - 1);  g_0,c = M2_c / n;  delta_c = mean_c - r_c
    g_j,c = (P_j - delta_c ((S - sum head[0..j)) + (S - sum ring[0..j))) + (n - j) delta_c^2) / n
    mean = mean_c mean_c;  var = (sum_c M2_c + n sum_c (mean_c - mean)^2) / (C n - 1)
    W = mean_c s_c^2;  B/n = sum_c (mean_c - mean)^2 / (C - 1)  (0 in var+ when C = 1)
    var+ = mean_c g_0,c + B/n;  rhat = sqrt(var+ / W)  (NaN when C = 1)
    rho_j = 1 - (mean_c g_0,c - mean_c g_j,c) / var+
    Geyer: G_k = rho_2k + rho_2k+1, 2k + 1 <= min(K, n - 1); stop at the first
    G_k < 0; G_k <- min(G_k, G_k-1); tau = -1 + 2 sum G_k; ess = C n / tau;
    ess_truncated: no negative pair was met.  W == 0: rhat, ess, rho NaN.
The device accumulates P_j with a fused multiply-add, numpy with a rounded
product: the update is compared within a tolerance, the finish (single rounded
operations on both sides) almost to the bit.
"""
import numpy as np

FIXED = ("r", "mean", "M2", "mn", "mx", "S")


class State:
    def __init__(self, shape, K):
        self.K, self.n = int(K), 0
        for k in FIXED:
            setattr(self, k, np.zeros(shape))
        self.P = np.zeros((self.K,) + tuple(shape))
        self.head = np.zeros((self.K,) + tuple(shape))
        self.ring = np.zeros((self.K,) + tuple(shape))


def update(st, rows):
    """Add the rows [T, ...shape] (iteration order) to the state, one at a time."""
    K = st.K
    for x in np.asarray(rows, dtype=np.float64):
        t = st.n
        if t == 0:
            st.r, st.mn, st.mx = x.copy(), x.copy(), x.copy()
        y = x - st.r
        d = x - st.mean
        st.mean = st.mean + d / float(t + 1)
        st.M2 = st.M2 + d * (x - st.mean)
        st.mn, st.mx = np.minimum(st.mn, x), np.maximum(st.mx, x)
        st.S = st.S + y
        m = min(K, t)                        # y_{t+1-j} exists for j <= t
        if m:
            st.P[:m] += y * st.ring[:m]
        if t < K:
            st.head[t] = y
        if K:
            st.ring[1:] = st.ring[:-1].copy()
            st.ring[0] = y
        st.n = t + 1
    return st


def from_device(fields, n, K):
    """State from the device fields [6 + 3K, C, nsb] (numpy) and the count n."""
    f = np.asarray(fields)
    st = State(f.shape[1:], K)
    st.n = int(n)
    for i, k in enumerate(FIXED):
        setattr(st, k, f[i].copy())
    st.P, st.head, st.ring = f[6:6 + K].copy(), f[6 + K:6 + 2 * K].copy(), f[6 + 2 * K:6 + 3 * K].copy()
    return st


def gammas(st):
    """Per-chain autocovariances [C, K + 1, nsb] from a state with arrays [C, nsb]."""
    n, K = st.n, st.K
    nd = float(n)
    C, nsb = st.mean.shape
    g = np.full((C, K + 1, nsb), np.nan)
    with np.errstate(all="ignore"):
        if n >= 1:
            g[:, 0] = st.M2 / nd
        delta = st.mean - st.r
        d2 = delta * delta
        hs, ts = np.zeros((C, nsb)), np.zeros((C, nsb))
        for j in range(1, K + 1):
            if n > j:
                hs = hs + st.head[j - 1]
                ts = ts + st.ring[j - 1]
                cross = delta * ((st.S - hs) + (st.S - ts))
                g[:, j] = ((st.P[j - 1] - cross) + (nd - float(j)) * d2) / nd
    return g


def finish(st):
    """The finish over the chain axis of a state with arrays [C, nsb]; dict of
    arrays: mean, var, min, max, ess, ess_truncated, rhat [nsb], chain_mean,
    chain_var [C, nsb], acf [K + 1, nsb], gamma [C, K + 1, nsb], n."""
    n, K = st.n, st.K
    nd = float(n)
    C, nsb = st.mean.shape
    Cd = float(C)
    nan = np.full(nsb, np.nan)
    with np.errstate(all="ignore"):
        chain_var = st.M2 / (nd - 1.0) if n >= 2 else np.full((C, nsb), np.nan)
        sum_mean, sum_M2, sum_var, sum_g0 = (np.zeros(nsb) for _ in range(4))
        for c in range(C):
            sum_mean = sum_mean + st.mean[c]
            sum_M2 = sum_M2 + st.M2[c]
            sum_var = sum_var + chain_var[c]
            sum_g0 = sum_g0 + st.M2[c] / nd
        mean = sum_mean / Cd
        sb2 = np.zeros(nsb)
        for c in range(C):
            d = st.mean[c] - mean
            sb2 = sb2 + d * d
        W, g0 = sum_var / Cd, sum_g0 / Cd
        var = (sum_M2 + nd * sb2) / (Cd * nd - 1.0) if n >= 1 and C * n >= 2 else nan.copy()
        Bn = sb2 / (Cd - 1.0) if C > 1 else np.zeros(nsb)
        varp = g0 + Bn
        degenerate = ~(W > 0.0)
        rhat = np.where(degenerate, np.nan, np.sqrt(varp / W)) if C > 1 else nan.copy()
        g = gammas(st)
        acf = np.empty((K + 1, nsb))
        for j in range(K + 1):
            acc = g[0, j].copy()
            for c in range(1, C):
                acc = acc + g[c, j]
            acf[j] = np.where(degenerate, np.nan, 1.0 - (g0 - acc / Cd) / varp)
        ess, trunc = nan.copy(), np.zeros(nsb, dtype=bool)
        jmax = min(K, n - 1)
        for i in np.nonzero(~degenerate)[0]:
            total, last, npairs, tr = 0.0, 0.0, 0, True
            k = 0
            while 2 * k + 1 <= jmax:
                G = acf[2 * k, i] + acf[2 * k + 1, i]
                if not G >= 0.0:
                    tr = False
                    break
                if npairs > 0:
                    G = min(G, last)
                last = G
                total = total + G
                npairs += 1
                k += 1
            trunc[i] = tr
            if npairs > 0:
                ess[i] = (Cd * nd) / (-1.0 + 2.0 * total)
    return {"mean": mean, "var": var, "min": st.mn.min(axis=0), "max": st.mx.max(axis=0), "ess": ess,
            "ess_truncated": trunc, "rhat": rhat, "chain_mean": st.mean.copy(), "chain_var": chain_var, "acf": acf,
            "gamma": g, "n": n}


def summarise(rows, K):
    """update + finish of rows [T, C, nsb]."""
    rows = np.asarray(rows, dtype=np.float64)
    return finish(update(State(rows.shape[1:], K), rows))


def direct_gamma(rows, K):
    """Two-pass centred autocovariances (divisor n) of rows [T, ...]: [K + 1, ...]."""
    x = np.asarray(rows, dtype=np.float64)
    T = x.shape[0]
    c = x - x.mean(axis=0)
    out = np.full((K + 1,) + x.shape[1:], np.nan)
    for j in range(min(K, T - 1) + 1):
        out[j] = (c[j:] * c[:T - j]).sum(axis=0) / T
    return out


def ar1(rng, T, shape, phi=0.5, offset=0.0):
    """x_t = phi x_{t-1} + e_t from the stationary law, plus offset: [T, ...shape]."""
    x = np.empty((T,) + tuple(shape))
    x[0] = rng.standard_normal(shape) / np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + rng.standard_normal(shape)
    return x + offset
