"""The table-driven Box-Muller radius of the CR sweep (csrc/gs_rng.h
bm_m2log_tab, bm_sqrt_radius), restated operation for operation with exact
rationals: every fp64 operation of the device code is one correctly rounded
operation here (an fma is the exact rational a b + c rounded once), so the
values are the device's bit for bit, except the rsq seed (below).

Checked, over both edges of every log cell at every exponent a uniform can
have and over 10^5 seeded uniforms u1 = (K + 1/2) 2^-53:
  * -2 ln u1, with the one-word ln 2 (the low word's term is at most
    53 x 4.64e-17 = 2.5e-15 where the result is at least 1.386 |e|: under a
    third of an ulp), stays within the 3 ulp the comments state;
  * the square root whose last correction uses the first-step half-reciprocal
    h0 stays within 1 ulp of the exact root of its argument.  The hardware's
    rsq seed is modelled by the extremes of the error the comment allows it
    (the correctly rounded 1 / sqrt(x) times 1 - 2^-22, 1, 1 + 2^-22): the
    result's error is 3/2 e^3 + O(e^4) in the seed's error e, largest at the
    extremes.
Errors are measured in ulps of the exact value (decimal, 60 digits).
"""
import math
import os
import random
import re
from decimal import Decimal, getcontext
from fractions import Fraction

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gibbssampler_amd", "csrc")
getcontext().prec = 60

NU = 100_000
LOG_BOUND_ULP = 3.0
SQRT_BOUND_ULP = 1.0


def fma(a, b, c):
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:      # IEEE: a zero sum is -0 only when the product and c are both -0
        neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
        return -0.0 if neg and Fraction(a) * Fraction(b) == 0 else 0.0
    return float(v)


@pytest.fixture(scope="module")
def log_tab():
    src = open(os.path.join(CSRC, "gs_bm_tables.h")).read()
    body = re.search(r"BM_LOG_TAB\[(\d+)\]\s*=\s*\{(.*?)\};", src, re.S)
    v = [float(x) for x in body.group(2).replace("\n", " ").split(",") if x.strip()]
    assert len(v) == int(body.group(1)) == 1024
    return v


def m2log(x, tab):
    """bm_m2log_tab: -2 ln(x 2^-53)."""
    m, e = math.frexp(x)
    e -= 53
    k = int((m - 0.5) * 1024)                       # the top 9 mantissa bits
    c, l2c = tab[2 * k], tab[2 * k + 1]
    r = fma(m, c, -1.0)
    q = fma(r, -0.4, 0.5)
    q = fma(q, r, -0.6666666666666666)
    q = fma(q, r, 1.0)
    q = fma(q, r, -2.0)
    return fma(float(e), -1.3862943611198906, fma(q, r, l2c))


def sqrt_radius(x, y0):
    """bm_sqrt_radius from the seed y0 ~ 1 / sqrt(x)."""
    y0 = min(abs(y0), 1073741824.0)
    g0 = x * y0
    h0 = y0 * 0.5
    r0 = fma(-h0, g0, 0.5)
    g1 = fma(g0, r0, g0)
    d0 = fma(-g1, g1, x)
    return fma(d0, h0, g1)


def dec(x):
    f = Fraction(x)
    return Decimal(f.numerator) / Decimal(f.denominator)


def ulps(got, exact):
    return float(abs(dec(got) - exact) / dec(math.ulp(float(exact))))


def _points():
    """x = K + 1/2 (as a double) at both edges of every log cell for every binade
    of x that holds such values with 10 mantissa bits to spare, then the seeded
    uniforms formed as u53 forms them."""
    xs = []
    for e in range(11, 54):                          # x in [2^(e-1), 2^e)
        for k in range(512):
            # the cell's edges are integers here; in the last binade K + 1/2
            # has rounded to an integer (to even), below it it is exact
            lo = math.ldexp(0.5 + k / 1024.0, e)
            hi = math.ldexp(0.5 + (k + 1) / 1024.0, e)
            xs += [lo, hi - 1.0] if e == 53 else [lo + 0.5, hi - 0.5]
    rng = random.Random(20261)
    for _ in range(NU):
        a, b = rng.getrandbits(32), rng.getrandbits(32)
        xs.append(float(a >> 5) * 67108864.0 + float(b >> 6) + 0.5)
    # small K: the far tail of the radius
    xs += [K + 0.5 for K in range(0, 64)]
    return [x for x in xs if 0.5 <= x < 9007199254740992.0]


@pytest.fixture(scope="module")
def evaluated(log_tab):
    out = []
    for x in _points():
        v = m2log(x, log_tab)
        exact = -2 * (dec(x) / Decimal(2 ** 53)).ln()
        out.append((x, v, ulps(v, exact)))
    return out


def test_m2log_one_word_ln2_within_3_ulp(evaluated):
    worst = max(evaluated, key=lambda t: t[2])
    print(f"-2 ln u: {len(evaluated)} points, worst {worst[2]:.3f} ulp at x = {worst[0]!r}")
    assert all(v > 0.0 for _, v, _ in evaluated)
    assert worst[2] <= LOG_BOUND_ULP


def test_sqrt_radius_h0_correction_within_1_ulp(evaluated):
    worst = (0.0, None, None)
    for x, v, _ in evaluated[::7] + evaluated[-64:]:
        exact = dec(v).sqrt()
        seed = float(1 / exact)
        for s in (-1, 0, 1):
            got = sqrt_radius(v, seed * (1.0 + s * 2.0 ** -22))
            err = ulps(got, exact)
            if err > worst[0]:
                worst = (err, v, s)
    print(f"sqrt: worst {worst[0]:.4f} ulp at x = {worst[1]!r}, seed error {worst[2]} x 2^-22")
    assert worst[0] <= SQRT_BOUND_ULP


def test_sqrt_radius_signed_zero():
    """x = +-0: the clamped seed 2^30 carries the signed zero through (h0 = 2^29 is finite)."""
    for z in (0.0, -0.0):
        got = sqrt_radius(z, math.inf)
        assert got == 0.0 and math.copysign(1.0, got) == math.copysign(1.0, z)


def test_rounded_up_uniform_is_finite_and_tiny(log_tab):
    """K = 2^53 - 1: K + 1/2 rounds to 2^53 (u1 rounds to 1, once in 2^53 draws).
    The exact value is 0; the terms cancel to rounding level, nothing more."""
    v = m2log(9007199254740992.0, log_tab)
    assert math.isfinite(v) and abs(v) <= 2.0 ** -50
