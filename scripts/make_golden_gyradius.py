#!/usr/bin/env python3
"""
Generate tests/golden/gyradius_ref.npz: inputs and outputs of the reference's ``radius_of_gyration``
(``src/mdhelper/algorithm/molecule.py``), inputs and outputs only.

    python scripts/make_golden_gyradius.py <root of a checkout of the reference>

The reference module imports MDAnalysis at the top for its annotations; the function needs none of it for
array input, so the file is loaded by path behind an inert stand-in module, the way
``scripts/make_golden_profile.py`` loads ``analysis/profile.py``.

Cases ``(M, N_p)``: random-walk chains with ~1.5 Å bonds, float32 positions (stored as float32, handed to the
reference as they are) and non-uniform float64 masses, called as ``Gyradius._single_frame`` calls it
(``grouping="segments"``, positions ``[M, N_p, 3]``, masses ``[M, N_p]``) with ``components`` False and True; the
first case also in the ungrouped form (one chain as ``[N_p, 3]``) and the ragged-list form (chains of different
lengths).  ``far`` is the (3, 130) case 9 000 Å from the origin, where a one-pass second moment cancels.
"""

import importlib.util
import pathlib
import sys
import types

import numpy as np

OUT = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "gyradius_ref.npz"

CASES = {"m5_n2": (5, 2, 0.0), "m7_n63": (7, 63, 0.0), "m4_n64": (4, 64, 0.0), "m4_n65": (4, 65, 0.0),
         "m3_n130": (3, 130, 0.0), "far": (3, 130, 9000.0)}


def load_reference(root):
    path = pathlib.Path(root) / "src" / "mdhelper" / "algorithm" / "molecule.py"
    stand_in = types.ModuleType("MDAnalysis")
    stand_in.AtomGroup = type("AtomGroup", (), {})
    sys.modules["MDAnalysis"] = stand_in
    spec = importlib.util.spec_from_file_location("reference_molecule", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def chains(rng, M, N_p, offset):
    """float32[M, N_p, 3] random walks, float64[M, N_p] masses."""
    steps = rng.normal(size=(M, N_p, 3))
    steps *= 1.5 / np.linalg.norm(steps, axis=-1, keepdims=True)
    pos = rng.uniform(0.0, 40.0, (M, 1, 3)) + np.cumsum(steps, axis=1) + offset
    return pos.astype(np.float32), rng.uniform(1.0, 20.0, (M, N_p))


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261017)
    out = {"cases": np.array(sorted(CASES))}
    for name, (M, N_p, offset) in CASES.items():
        pos, masses = chains(rng, M, N_p, offset)
        out[f"pos_{name}"], out[f"masses_{name}"] = pos, masses
        for components in (False, True):
            r = ref.radius_of_gyration(grouping="segments", positions=pos, masses=masses, components=components)
            assert r.shape == ((M, 3) if components else (M,)) and np.all(np.isfinite(r)), name
            out[f"out_{name}_{'xyz' if components else 'rg'}"] = np.asarray(r, dtype=np.float64)
    # ungrouped: one chain as [N_p, 3] / [N_p]
    pos, masses = out["pos_m7_n63"][2], out["masses_m7_n63"][2]
    out["out_single_rg"] = np.float64(ref.radius_of_gyration(positions=pos, masses=masses))
    out["out_single_xyz"] = np.asarray(ref.radius_of_gyration(positions=pos, masses=masses, components=True))
    # ragged lists: the chains of m4_n65 cut to different lengths
    lengths = np.array([65, 17, 1, 40])
    out["ragged_lengths"] = lengths
    pos = [p[:n] for p, n in zip(out["pos_m4_n65"], lengths)]
    masses = [m[:n] for m, n in zip(out["masses_m4_n65"], lengths)]
    out["out_ragged_rg"] = np.asarray(ref.radius_of_gyration(positions=pos, masses=masses), dtype=np.float64)
    out["out_ragged_xyz"] = np.asarray(ref.radius_of_gyration(positions=pos, masses=masses, components=True),
                                       dtype=np.float64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(CASES)} cases)")


if __name__ == "__main__":
    main()
