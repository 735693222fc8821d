#!/usr/bin/env python3
"""The per-tick hand-over of a disc table (mppi_set_discs) on two BUILDS of the library, for nav2d_discs and racing_discs at
T = 50, n = 8, from a device table and from a host table: four figures per build.

A figure is the median time of one call from enqueue to stream-idle (host clock around the call and a device synchronise)
over --calls calls after --warm warm-up calls.  Every run is a process of its own (MPPI_HIP_LIB selects the library); the
other build and the shipped one take turns, the other build first, --reps runs each.  Printed: every run's figures, each
build's minimum, maximum and run-to-run spread (max - min) over its runs, and whether every run of the shipped build lies
inside the other build's range (below its minimum counts as inside: faster is no regression).
Usage (GPU box): python scripts/step_table_timing.py other_build.so [--reps 3] [--calls 2000] [--warm 300]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIGURES = [(m, src) for m in ("nav2d_discs", "racing_discs") for src in ("device", "host")]
T, N = 50, 4096


def child(calls, warm):
    sys.path[:0] = [ROOT, HERE]
    import numpy as np
    import torch

    import moving_discs_timing as nav
    import racing_opponents_timing as rac

    out = {}
    for model, build in (("nav2d_discs", nav.build), ("racing_discs", rac.build)):
        solver, x0 = build(N, T, 8)
        solver.forward(x0)  # (parameters, maps, the window and the first table: the buffer has its size from here on)
        tab = np.zeros((T, 8, 4), np.float32)
        tab[:, :, 2], tab[:, :, 3] = 0.1, 10.0
        dev = torch.from_numpy(tab).cuda()
        st = solver._stream()
        for src in ("device", "host"):
            ptr, on_device = (dev.data_ptr(), 1) if src == "device" else (tab.ctypes.data_as(C.c_void_p), 0)
            times = []
            for i in range(warm + calls):
                t0 = time.perf_counter()
                solver._h.call("mppi_set_discs", ptr, T, 8, on_device, st)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e6)
            out[f"{model} {src}"] = statistics.median(times[warm:])
        solver.forward(x0)  # (the handle still solves)
        torch.cuda.synchronize()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.calls, args.warm)
    builds = ([("other", os.path.abspath(args.other))] if args.other else []) + [("shipped", "")]
    runs = {name: [] for name, _ in builds}
    for rep in range(args.reps):
        for name, lib in builds:
            env = dict(os.environ)
            env.pop("MPPI_HIP_LIB", None)
            if lib:
                env["MPPI_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warm", str(args.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:  # (nothing more is started on the device after a run that failed)
                sys.exit(f"{name}, run {rep}: exit status {r.returncode}\n{r.stderr[-2000:]}")
            runs[name].append(json.loads(line[0][7:]))
            print(f"{name:8s} run {rep}: " + "  ".join(f"{m} {src} {runs[name][-1][f'{m} {src}']:.2f}" for m, src in FIGURES) + "  us", flush=True)
    for m, src in FIGURES:
        key, rng = f"{m} {src}", {}
        for name, _ in builds:
            v = [r[key] for r in runs[name]]
            rng[name] = (min(v), max(v))
            print(f"{key:20s} {name:8s} min {min(v):.2f}  max {max(v):.2f}  spread {max(v) - min(v):.2f} us")
        if "other" in rng:
            print(f"{key:20s} shipped inside the other build's range: {rng['shipped'][1] <= rng['other'][1]}")


if __name__ == "__main__":
    main()
