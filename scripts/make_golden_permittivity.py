#!/usr/bin/env python3
"""
Generate tests/golden/permittivity_ref.npz: inputs and outputs of the reference's
``calculate_relative_permittivity`` (``src/mdhelper/analysis/electrostatics.py``), inputs and outputs only.

    python scripts/make_golden_permittivity.py <root of a checkout of the reference>

The reference module imports MDAnalysis, pint (through the package root) and its own ``analysis.base`` /
``algorithm`` modules at the top; none of them is needed by the function, so the file is loaded by path behind
inert stand-in modules, the way ``scripts/make_golden_profile.py`` loads ``profile.py``.  Every case uses
``reduced=True``: the unit registry is then never touched.  The non-reduced branch multiplies its arguments by
pint units, and pint is not a dependency here, so that branch stays unpinned by the reference (the test compares
it with the closed form instead).
"""

import importlib.util
import pathlib
import sys
import types

import numpy as np

OUT = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "permittivity_ref.npz"


def load_reference(root):
    path = pathlib.Path(root) / "src" / "mdhelper" / "analysis" / "electrostatics.py"

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Anything:
        """Stands for a class in annotations and for a registry whose attributes are never used."""
        def __getattr__(self, name):
            return Anything()

    mda = module("MDAnalysis", __path__=[], AtomGroup=type("AtomGroup", (), {}))
    module("MDAnalysis.lib", __path__=[])
    mda.lib = sys.modules["MDAnalysis.lib"]
    module("MDAnalysis.lib.mdamath", make_whole=None)
    module("mdhelper", __path__=[], FOUND_OPENMM=False, Q_=type("Q_", (), {}), ureg=Anything())
    module("mdhelper.analysis", __path__=[])
    module("mdhelper.analysis.base", DynamicAnalysisBase=type("DynamicAnalysisBase", (), {}))
    module("mdhelper.algorithm", __path__=[])
    module("mdhelper.algorithm.topology", unwrap=None)
    module("mdhelper.algorithm.unit", strip_unit=None)
    spec = importlib.util.spec_from_file_location("mdhelper.analysis.electrostatics", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261017)
    # (frames, temperature, volumes): a single frame (no fluctuation: exactly 1), a short and a long series with a
    # mean dipole that is not zero, a constant volume and one that fluctuates
    cases = {
        "one_frame": (1, 1.0, np.array([1000.0])),
        "short": (5, 1.0, np.full(5, 27000.0)),
        "long": (400, 0.8, 64000.0 * (1 + 0.01 * rng.normal(size=400))),
        "hot": (64, 2.5, np.array([8000.0])),
    }
    out = {"cases": np.array(list(cases))}
    for name, (n, T, V) in cases.items():
        M = rng.normal(size=(n, 3)) * np.array([30.0, 5.0, 80.0]) + np.array([12.0, -40.0, 0.5])
        eps = ref.calculate_relative_permittivity(M.copy(), T, V.copy(), reduced=True)
        assert np.isfinite(eps), name
        out[f"M_{name}"], out[f"T_{name}"], out[f"V_{name}"] = M, np.float64(T), V
        out[f"out_{name}"] = np.float64(eps)
    assert out["out_one_frame"] == 1.0
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
