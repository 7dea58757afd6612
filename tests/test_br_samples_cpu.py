"""CPU: the options of run(br_samples=) (samplers.check_br_samples) and the numpy
restatement of the sample bank's evaluator (tests/_br_samples.py) against the
streaming estimator's restatement (tests/_br_likelihood.py)."""
import numpy as np
import pytest

pytest.importorskip("torch")

from tests import _br_likelihood as R  # noqa: E402
from tests import _br_samples as B  # noqa: E402

SEED = 20261021
BINS_A = np.array([0, 1, 2, 3, 4, 6, 8, 9, 18, 52, 65])
BINS_B = np.array([0, 1, 2, 4, 13, 47, 65])


def bins_of(F):
    from gibbssampler_amd.engine import SPECTRA
    return {s: (BINS_B if s == "BB" and F > 1 else BINS_A) for s in SPECTRA[F]}


def test_check_br_samples():
    from gibbssampler_amd.engine import br_likelihood_mask
    from gibbssampler_amd.samplers import check_br_samples
    bins = bins_of(3)
    assert check_br_samples(None, 3, bins) is None and check_br_samples(False, 3, bins) is None
    drawn = br_likelihood_mask(3, bins)
    got = check_br_samples(True, 3, bins)
    assert np.array_equal(got["mask"], drawn) and got["start"] is None
    got = check_br_samples({"lrange": (2, 8), "start": 5}, 3, bins)
    assert got["start"] == 5 and np.array_equal(got["mask"], br_likelihood_mask(3, bins, None, (2, 8)))
    assert got["mask"].sum() == 5 * 3 + 1                              # bins 2 .. 6 of TT, EE, TE; [2, 4) of BB
    with pytest.raises(ValueError, match="unknown options"):
        check_br_samples({"lrange": (2, 8), "theory": 1}, 3, bins)
    with pytest.raises(ValueError, match="either lrange or mask"):
        check_br_samples({"lrange": (2, 8), "mask": drawn}, 3, bins)
    with pytest.raises(ValueError, match="empty used set"):
        check_br_samples({"lrange": (0, 1)}, 3, bins)
    with pytest.raises(ValueError, match="empty used set"):
        check_br_samples({"mask": np.zeros_like(drawn)}, 3, bins)
    split = drawn.copy()
    split[1, 4] = False                                                # EE without its TT and TE
    with pytest.raises(ValueError, match="TEB block is used as a whole"):
        check_br_samples({"mask": split}, 3, bins)
    with pytest.raises(ValueError, match="start must be >= 0"):
        check_br_samples({"start": -1}, 3, bins)
    with pytest.raises(ValueError, match="lrange must be"):
        check_br_samples({"lrange": (8, 2)}, 3, bins)
    with pytest.raises(ValueError, match="mask must be"):
        check_br_samples({"mask": drawn[:, :4]}, 3, bins)
    with pytest.raises(ValueError, match="dict"):
        check_br_samples(3, 3, bins)


def test_br_theory_rules():
    from gibbssampler_amd.engine import br_likelihood_mask
    from gibbssampler_amd.samplers import br_theory
    bins = bins_of(3)
    mask = br_likelihood_mask(3, bins)
    _, theory, _ = R.synthetic(3, bins, 2, 1, 1, SEED)
    assert np.array_equal(br_theory("x", theory, 3, bins, mask), theory)
    with pytest.raises(ValueError, match=r"\[K, nspec, maxbins\]"):
        br_theory("x", theory[:, :, :5], 3, bins, mask)
    t = theory.copy()
    t[0, 2, 3] = -1.0
    with pytest.raises(ValueError, match="positive but for TE"):
        br_theory("x", t, 3, bins, mask)
    t = theory.copy()
    t[1, 3, 4] = 2.0 * np.sqrt(t[1, 0, 4] * t[1, 1, 4])
    with pytest.raises(ValueError, match="positive definite"):
        br_theory("x", t, 3, bins, mask)


@pytest.mark.parametrize("F", [1, 2, 3])
def test_restatement_agrees_with_streaming(F):
    from gibbssampler_amd.engine import br_likelihood_tables
    bins = bins_of(F)
    rows, theory, mask = R.synthetic(F, bins, 5, 7, 3, SEED)
    tables = br_likelihood_tables(F, bins, theory, mask)
    maxbins = mask.shape[1]
    flat = rows.reshape(7, 3, -1)
    if F == 3:
        flat = flat.copy()
        flat[2, 1, 2 * maxbins + 3] = 0.0                              # one bad row (beta = 0, BB) for chain 1
    ref = R.update(R.State(3, 5), flat, tables, maxbins)
    want = R.finish(ref.m, ref.S, ref.Q, ref.n, tables["cst"])
    got = B.loglike(flat, tables, maxbins)
    assert got["n"] == ref.n == 7 and np.array_equal(got["bad"], ref.bad)
    for name, w in zip(("loglike", "chain_loglike", "neff"), want):
        assert np.all(np.isfinite(w))
        np.testing.assert_allclose(got[name], w, rtol=1e-12, atol=0.0, err_msg=name)
