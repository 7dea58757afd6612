"""The unchanged-caller drop-in: with ``dropin/`` on
sys.path in place of the reference checkout, the reference-module imports of
main_polarization.py (lines 1-2, 7-9) resolve to this package, its constructor
calls (main_polarization.py:109-126) bind to the classes' signatures, and every
``config.<name>`` / ``<sampler>.constrained_sampler.<name>`` it reads exists.

The caller's side is stored as names only (tests/golden/main_polarization_names.json:
the names it imports, the positional count and keyword names of its constructor
calls, the config attributes it reads); nothing of the caller is executed or
copied.  CPU only: binding checks signatures, nothing is constructed on a device."""
import importlib
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
NAMES = os.path.join(ROOT, "tests", "golden", "main_polarization_names.json")
REF_MODULES = ("utils", "config", "NonCenteredGibbs", "ASIS", "CenteredGibbs")


def _caller_names():
    with open(NAMES) as f:
        return json.load(f)


@pytest.fixture
def dropin_modules():
    saved = {k: sys.modules.pop(k) for k in REF_MODULES + ("_gs_path",) if k in sys.modules}
    sys.path.insert(0, DROPIN)
    try:
        yield {m: importlib.import_module(m) for m in REF_MODULES}
    finally:
        sys.path.remove(DROPIN)
        for k in REF_MODULES + ("_gs_path",):
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_reference_imports_resolve_to_this_package(dropin_modules):
    import gibbssampler_amd.config as gcfg
    import gibbssampler_amd.gibbs as gg
    import gibbssampler_amd.utils as gutils
    m = dropin_modules
    assert m["config"] is gcfg and m["utils"] is gutils
    assert m["CenteredGibbs"].CenteredGibbs is gg.CenteredGibbs
    assert m["NonCenteredGibbs"].NonCenteredGibbs is gg.NonCenteredGibbs
    assert m["ASIS"].ASIS is gg.ASIS
    names = _caller_names()
    for module, attrs in names["imports_from"].items():
        assert module in REF_MODULES
        for a in attrs:
            assert hasattr(m[module], a), (module, a)
    for module in names["imports"]:
        assert module in m


def test_constructor_calls_bind(dropin_modules):
    m = dropin_modules
    calls = _caller_names()["constructor_calls"]
    assert {c[0] for c in calls} == {"CenteredGibbs", "NonCenteredGibbs", "ASIS"}
    for name, npos, kws in calls:
        cls = getattr(m[name], name)
        sig = inspect.signature(cls.__init__)
        sig.bind(None, *([0] * npos), **{k: 0 for k in kws})


def test_config_and_attribute_reads_exist(dropin_modules):
    cfg = dropin_modules["config"]
    names = set(_caller_names()["config_attributes"])
    assert len(names) >= 19
    missing = sorted(n for n in names if not hasattr(cfg, n))
    assert not missing, missing
    assert cfg.NSIDE == 256 and cfg.L_MAX_SCALARS == 512 and len(cfg.bins["BB"]) == 413
    # main_polarization.py:180-182 reads these off the ASIS sampler and its step object
    import types
    import gibbssampler_amd.gibbs as gg
    owner = types.SimpleNamespace(lmax=16, nside=8, Npix=768, bl_map=None, bl_gauss=None, pix_map=None,
                                  gibbs_cr=True)
    step = gg._StepBase(owner)
    assert step.pcg_accuracy == 1.0e-5 and step.gibbs_cr is True and step.n_gibbs == 1
    assert "rj_step" in inspect.signature(dropin_modules["ASIS"].ASIS.__init__).parameters
