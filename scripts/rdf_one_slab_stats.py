"""Statistics of one RDF call of one slab, twice over in one process (16 frames of 8 192 atoms, three ranges):
pairs_exact, pairs_computed, cell_units.  The sort scatters through LDS atomics, so the tiling — and with it these
figures, not the counts — differs from run to run of one build.  Run on the GPU box; MDX_LIBRARY selects the library."""
import json
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

rng = np.random.default_rng(5)
L = np.float32(43.43)
pos = (rng.random((16, 8192, 3)) * L).astype(np.float32)
dims = np.array([L, L, L, 90, 90, 90], dtype=np.float32)
for rep in range(2):
    out = {}
    for name, excl, rr in (("self_excl_r15", (1, 1), (0.0, 15.0)), ("self_lower", None, (3.0, 12.0)),
                           ("self_excl_r8", (1, 1), (0.0, 8.0))):
        eng = _core.RdfEngine(np.linspace(rr[0], rr[1], 202), excl, algo="cell")
        eng.accumulate(pos, None, dims)
        st = eng.stats()
        out[name] = {k: int(st[k]) for k in ("pairs_exact", "pairs_computed", "cell_units", "cell_units_general")}
        out[name]["counts_sum"] = int(eng.counts().sum())
        eng.close()
    print(json.dumps(out, sort_keys=True))
