#!/usr/bin/env python3
"""Record tests/golden/noise_and_lookup_bits.npz: what the library computes, bit for bit, for the cases of
tests/noise_bits_cases.py (exported noise, costs, action_seq, state_seq of two consecutive solves each), on an MI355X.

The fixture holds the outputs of the commit BEFORE a change that must not move a bit of the noise chain or of the map
lookup: run this on a checkout of that commit, or with MPPI_HIP_LIB pointing at a library built from it
(scripts/build_variant.sh), and name it with --label.
    python scripts/record_noise_bits.py --label "parent c5a1bd6" [--out tests/golden/noise_and_lookup_bits.npz]
A second run against the same build must reproduce the file's arrays (--check compares instead of writing)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mppi_playground_amd  # noqa: E402,F401
import noise_bits_cases as nb  # noqa: E402
from test_gpu_covariance import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True, help="which build the outputs are of")
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "noise_and_lookup_bits.npz"))
ap.add_argument("--check", action="store_true", help="compare with the file instead of writing it")
args = ap.parse_args()

arrays = {}
for c in nb.CASES:
    for key, v in nb.run(c, make).items():
        arrays[f"{c['name']}/{key}"] = v
    print(c["name"], "costs", arrays[f"{c['name']}/costs_0"][:3], flush=True)
for g in nb.GENERIC:
    for key, v in nb.run_generic(g).items():
        arrays[f"{g['name']}/{key}"] = v
    print(g["name"], flush=True)

if args.check:
    z = np.load(args.out)
    bad = [k for k in arrays if not np.array_equal(arrays[k].view(np.uint32), z[k].view(np.uint32))]
    missing = sorted(set(z.files) - set(arrays) - {"label"})
    print(f"checked {len(arrays)} arrays against {args.out} ({z['label']}): {len(bad)} differ, {len(missing)} not produced")
    for k in bad + missing:
        print("  ", k)
    sys.exit(1 if bad or missing else 0)
np.savez_compressed(args.out, label=np.array(args.label), **arrays)
print(f"wrote {args.out}: {len(arrays)} arrays, {os.path.getsize(args.out)} bytes, lib {mppi_playground_amd._capi.LIB_PATH}")
