"""Record tests/golden/solve_routes/*.npz: what tests/test_gpu_solve_routes.py's batches return on the GPU (next state, gradients, status,
the record's x, cls, pflag and pinv rows) with the library that is loaded - NBL_LIB_PATH names another build.  The test compares later
builds with these files byte for byte, so they are recorded once, from the build whose results are to be kept.
The output directory has to be named: a run without it must not re-baseline the test by accident.
usage (GPU box): python tools/record_solve_routes_golden.py <output directory>     (tests/golden/solve_routes to replace the fixtures)"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_solve_routes as t

if len(sys.argv) != 2:
    sys.exit(__doc__)
out = sys.argv[1]
os.makedirs(out, exist_ok=True)
for name in t.CASES:
    arrays, info = t.device_results(name)
    print(name, info["routes"], flush=True)
    for path, keys in t.golden_files(name):
        path = os.path.join(out, os.path.basename(path))
        np.savez_compressed(path, **{k: arrays[k] for k in keys})
        print("  ", path, os.path.getsize(path), "bytes")
