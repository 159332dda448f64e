#!/usr/bin/env python3
"""
Generate tests/golden/profile_ref.npz: inputs and outputs of the reference's
``calculate_potential_profile`` (``src/mdhelper/analysis/profile.py``), inputs and outputs only.

    python scripts/make_golden_profile.py <root of a checkout of the reference>

The reference module imports MDAnalysis, pint (through the package root) and its own ``analysis.base`` /
``algorithm`` modules at the top; none of them is needed by the function, so the file is loaded by path
behind inert stand-in modules, the way ``scripts/make_golden.py`` loads ``algorithm/accelerated.py``
without numba.  Every case uses ``reduced=True``: the unit registry is then never touched.  A case in which
the reference raises is recorded with its error message (``error_<case>``) instead of an output.
"""

import importlib.util
import json
import pathlib
import sys
import types
import warnings

import numpy as np

OUT = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "profile_ref.npz"


def load_reference(root):
    path = pathlib.Path(root) / "src" / "mdhelper" / "analysis" / "profile.py"

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Anything:
        """Stands for a class in annotations and for a registry whose attributes are never used."""
        def __getattr__(self, name):
            return Anything()

    module("MDAnalysis", AtomGroup=type("AtomGroup", (), {}))
    module("mdhelper", __path__=[], FOUND_OPENMM=False, Q_=type("Q_", (), {}), ureg=Anything())
    module("mdhelper.analysis", __path__=[])
    module("mdhelper.analysis.base", DynamicAnalysisBase=type("DynamicAnalysisBase", (), {}))
    module("mdhelper.algorithm", __path__=[])
    module("mdhelper.algorithm.molecule", center_of_mass=None)
    module("mdhelper.algorithm.topology", unwrap=None, wrap=None)
    module("mdhelper.algorithm.unit", strip_unit=None)
    spec = importlib.util.spec_from_file_location("mdhelper.analysis.profile", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    L, n = 60.0, 201
    bins = np.linspace(L / (2 * n), L - L / (2 * n), n)
    rng = np.random.default_rng(20261017)
    # a slab: a positive layer at the left wall, a negative one at the right wall and a field-free bulk between
    # them (the plateau the sigma_q-free integral case looks for around the middle bin) ...
    layers = 0.02 * (np.exp(-((bins - 6.0) / 1.5) ** 2) - np.exp(-((bins - 54.0) / 1.5) ** 2))
    layers[np.abs(bins - L / 2) < 12.0] = 0.0
    # ... and a noisy, neutral profile for the cases that are told sigma_q or dV
    noisy = layers + 1e-3 * rng.normal(size=n)
    noisy -= noisy.mean()
    cases = {
        "integral_sigma": ("noisy", {"sigma_q": -0.013}),
        "integral_sigma_dielectric": ("noisy", {"sigma_q": 0.004, "dielectric": 78.4}),
        "integral_dV": ("noisy", {"dV": 1.5, "dielectric": 2.5}),
        "integral_V0": ("noisy", {"sigma_q": -0.013, "V0": 0.35}),
        "integral_plateau": ("layers", {}),
        "matrix_slab": ("noisy", {"sigma_q": -0.013, "method": "matrix"}),
        "matrix_slab_dV": ("noisy", {"dV": -0.7, "dielectric": 4.0, "method": "matrix"}),
        "matrix_pbc": ("noisy", {"sigma_q": 0.0, "method": "matrix", "pbc": True}),
    }
    out = {"bins": bins, "L": np.float64(L), "layers": layers, "noisy": noisy,
           "cases": np.array(json.dumps(cases))}
    profiles = {"layers": layers, "noisy": noisy}
    for name, (which, kw) in cases.items():
        kw = dict(kw)
        dielectric = kw.pop("dielectric", 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                psi = ref.calculate_potential_profile(bins.copy(), profiles[which].copy(), L, dielectric,
                                                      reduced=True, **kw)
            except ValueError as exc:
                # V0 != 0 with method="integral": the reference hands V0 to cumulative_trapezoid(initial=...),
                # which SciPy >= 1.12 refuses (and which older SciPy only wrote into the first element); what
                # the reference did here is recorded, the test holds the port to the documented "add V0"
                assert "V0" in kw, name
                out["error_" + name] = np.array(f"{type(exc).__name__}: {exc}")
                continue
        assert np.all(np.isfinite(psi)), name
        out["out_" + name] = np.asarray(psi, dtype=np.float64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
