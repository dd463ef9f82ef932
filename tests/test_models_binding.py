"""CPU checks of the bulk model export's bindings: the Julia drop-in calls partls_opt_models, and that ccall agrees
with include/partls.h (tools/check_julia_binding.py)."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_julia_binding as CJ  # noqa: E402


def test_julia_dropin_calls_partls_opt_models():
    calls = CJ.parse_ccalls()
    models = [c for c in calls if c[0] == "partls_opt_models"]
    assert len(models) == 1
    sym, ret, types, nactual, _ = models[0]
    protos = CJ.parse_header()
    assert sym in protos and len(types) == len(protos[sym][1]) == nactual == 14
    checked = CJ.check()
    assert any(s == "partls_opt_models" for s, _ in checked)
    # the per-pattern fallback stays, with its status-9 reroute
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "for b in redo" in text and "stb == 9 && return _fit_opt_julia" in text


def test_python_binding_declares_partls_opt_models(partls):
    names = {name: args for name, _, args in partls.lowlevel.SYMBOLS}
    assert len(names["partls_opt_models"]) == 14
