"""Time of one RDF call on 1, 2, 4 and 7 resident frames (the `spread` mapping of the pair kernel: fewer than eight
frames, items dealt to the XCDs one by one) and on 8 to 1 024: what a launch costs beside its frames.  C2(i) shapes:
32 768 atoms, L = 68.94 A,
201 bins over (0, 15), exclusion (1, 1).  Run on the GPU box; MDX_LIBRARY selects the library:
    python scripts/rdf_one_frame_time.py [calls]
Prints one JSON line: median and minimum wall time per call in ms (a call ends in synchronize())."""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(9)
N, L = 32768, np.float32(68.94)
pos = np.tile((rng.random((64, N, 3)) * L).astype(np.float32), (16, 1, 1))      # 1 024 frames, 64 distinct
boxes = np.tile(np.array([L, L, L, 90, 90, 90], dtype=np.float32), (1024, 1))
d_pos, d_box = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(boxes)
out = {}
for frames in (1, 2, 4, 7, 8, 64, 256, 1024):
    eng = _core.RdfEngine(np.linspace(0.0, 15.0, 202), (1, 1), algo="cell")
    t = []
    n_calls = max(20, min(calls, 12800 // frames))
    for k in range(n_calls + 10):
        t0 = time.perf_counter()
        eng.accumulate_device(d_pos.ptr, N, None, N, d_box.ptr, frames)
        eng.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    eng.close()
    t = t[10:]
    out[str(frames)] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4)}
print(json.dumps(out, sort_keys=True))
