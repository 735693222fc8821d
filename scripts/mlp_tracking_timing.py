#!/usr/bin/env python3
"""What the tracking cost of the learned-dynamics models costs (envs.MLPModel.set_reference, angular=), and that a solver
WITHOUT it costs what it did: this library against a build of the parent commit.  The numbers of profiles/r26_mlp_tracking.md.

Solves measured: mlp41 and mlp82 (two tanh layers of 32 units, residual) at N = 2^20, T = 50 and N = 4096, T = 25,
  none     no reference, no angular component (the default solver: what the parent build can run too),
  ref      a reference of T rows,
  ref+ang  a reference and two angular components.
Per solve: the rollout stage (mppi_get_timing) and the whole solve (open-loop wall clock), each the median over the solves of a
round.  Every round is a process of its own; the two libraries take turns (MPPI_HIP_LIB selects the parent's, the
scripts/lib_ab.py way) over --rounds rounds in one session.  Printed per figure: the rounds' median and range.

The condition: every `none` median of this library lies inside the parent's own min-max range of the session (nothing on that
path should add vector work, so the parent's spread is the whole margin).  The two tracking columns are reported, not bounded.
Exit status 1 when the condition fails.
Usage: python scripts/mlp_tracking_timing.py --parent path/to/libmppi_hip_parent.so [--rounds 4]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1 << 20, 50, 8), (4096, 25, 40))  # (N, T, solves per figure)
MODELS = ("mlp41", "mlp82")
VARIANTS = ("none", "ref", "ref+ang")


NEW_ENTRY_POINTS = ("mppi_set_mlp_reference", "mppi_get_mlp_reference", "mppi_set_mlp_angular", "mppi_get_mlp_angular")


def child(variants):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
    import numpy as np
    import torch  # (before the library: it brings the HIP runtime the library binds to)

    if os.environ.get("MPPI_HIP_LIB"):  # the parent's build lacks this feature's entry points; its rounds never call them
        from mppi_playground_amd import _capi

        _capi.load(allow_missing=NEW_ENTRY_POINTS)

    import mlp8_timing as base  # (the networks, limits and timers of the 8-state note)
    from pi_mpc.mppi import MPPI

    limits = dict(base.LIMITS)
    limits[1] = ([-1.5], [1.5], [0.8])
    out = {}
    for N, T, n in SIZES:
        for name in MODELS:
            ds, dc = int(name[3]), int(name[4])
            for variant in variants:
                m = base.network(name)
                if variant == "ref+ang":
                    m.set_angular((0, ds - 1))
                if variant != "none":
                    rng = np.random.default_rng(T)
                    goals = rng.uniform(-0.5, 0.5, (T, ds)).astype(np.float32)
                    if variant == "ref+ang":
                        goals[:, [0, ds - 1]] = rng.uniform(3.0, 9.0, (T, 2)) * np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None]
                    m.set_reference(torch.from_numpy(goals).cuda(), torch.from_numpy(rng.uniform(0.5, 2.0, (T, ds)).astype(np.float32)).cuda())
                lo, hi, sig = limits[dc]
                solver = MPPI(horizon=T, num_samples=N, dim_state=ds, dim_control=dc, dynamics=m.dynamics, cost_func=m.cost,
                              u_min=torch.tensor(lo), u_max=torch.tensor(hi), sigmas=torch.tensor(sig), lambda_=1.0)
                assert solver._model == name
                x0 = torch.tensor(base.X0[:ds], device="cuda")
                base.loop(solver, x0, 10 if N < 100000 else 3)
                key = f"N={N} T={T} {name} {variant}"
                out[key + " rollout"] = base.stage_us(solver, x0, n)
                vals = []
                for _ in range(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    solver.forward(x0)
                    torch.cuda.synchronize()
                    vals.append((time.perf_counter() - t0) * 1e6)
                out[key + " solve"] = statistics.median(vals)
                del solver
                torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmppi_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child.split(","))
        return 0
    if args.rounds < 4:
        ap.error("at least four rounds")
    runs = {"this": ("", ",".join(VARIANTS)), "parent": (os.path.abspath(args.parent), "none")}
    res = {who: {} for who in runs}
    for rnd in range(args.rounds):
        for who in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):
            lib, variants = runs[who]
            env = dict(os.environ)
            env.pop("MPPI_HIP_LIB", None)
            if lib:
                env["MPPI_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent", args.parent, "--child", variants], env=env,
                               capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"round {rnd} {who} failed (exit {r.returncode}): {r.stderr[-600:]}", flush=True)
                return 2
            for k, v in json.loads(line[0][7:]).items():
                res[who].setdefault(k, []).append(v)
            print(f"round {rnd} {who}: done", flush=True)
    ok = True
    print(f"{'figure (us)':44s} {'this: median [min, max]':34s} parent: median [min, max]")
    for k in res["this"]:
        v = res["this"][k]
        cell = f"{statistics.median(v):10.2f} [{min(v):10.2f}, {max(v):10.2f}]"
        p = res["parent"].get(k)
        if p is None:
            print(f"{k:44s} {cell}")
            continue
        inside = min(p) <= statistics.median(v) <= max(p)
        ok = ok and inside
        print(f"{k:44s} {cell}   {statistics.median(p):10.2f} [{min(p):10.2f}, {max(p):10.2f}]  {'inside' if inside else 'OUTSIDE'}")
    print("no-reference medians inside the parent's range: " + ("yes" if ok else "NO"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
