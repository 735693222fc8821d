#!/usr/bin/env python3
"""What the learned terminal value of the learned-dynamics models costs (envs.MLPModel.set_value, MPPI(terminal_cost=)), and
that a solver WITHOUT it costs what it did: this library against a build of the parent commit.  The numbers of
profiles/r27_mlp_value.md.

Solves measured: mlp41 and mlp82 (two tanh layers of 32 units, residual) at N = 2^20, T = 50 and N = 4096, T = 25,
  none       the default solver (the kernels without reference, mask or value),
  ref        a reference of T rows, no value (the kernels that carry the value's branch, not taken): both libraries,
  value      a two-layer tanh value network on the handle of `none`,
  ref+value  the same on the handle of `ref`,
and what the feature is for: mlp41, N = 4096, the whole solve at T = 8 with the value against T = 25 without.
Per solve: the rollout stage (mppi_get_timing) and the whole solve (open-loop wall clock), each the median over the solves of a
round.  Every round is a process of its own; the two libraries take turns (MPPI_HIP_LIB selects the parent's, the
scripts/lib_ab.py way) over --rounds rounds in one session.  Printed per figure: the rounds' median and range, and for the
figures both libraries have, whether this library's median lies inside the parent's own min-max range.  Nothing is bounded:
the exit status is 0 when every round ran.
Usage: python scripts/mlp_value_timing.py --parent path/to/libmppi_hip_parent.so [--rounds 4]"""
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
VARIANTS = ("none", "ref", "value", "ref+value")
NEW_ENTRY_POINTS = ("mppi_set_mlp_value", "mppi_get_mlp_value")


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

    def value_net(ds, seed=3):
        rng = np.random.default_rng(seed)
        dims = [ds, 32, 32, 1]
        Ws = [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
        return Ws, [(0.1 * rng.standard_normal(o)).astype(np.float32) for o in dims[1:]]

    def timed(name, N, T, n, variant):
        ds, dc = int(name[3]), int(name[4])
        m = base.network(name)
        if variant.startswith("ref"):
            rng = np.random.default_rng(T)
            m.set_reference(torch.from_numpy(rng.uniform(-0.5, 0.5, (T, ds)).astype(np.float32)).cuda(),
                            torch.from_numpy(rng.uniform(0.5, 2.0, (T, ds)).astype(np.float32)).cuda())
        use = variant.endswith("value")
        if use:
            m.set_value(*value_net(ds), activation="tanh", weight=1.0)
        lo, hi, sig = limits[dc]
        solver = MPPI(horizon=T, num_samples=N, dim_state=ds, dim_control=dc, dynamics=m.dynamics, cost_func=m.cost,
                      terminal_cost=m.terminal_cost if use else None, u_min=torch.tensor(lo), u_max=torch.tensor(hi),
                      sigmas=torch.tensor(sig), lambda_=1.0)
        assert solver._model == name
        x0 = torch.tensor(base.X0[:ds], device="cuda")
        base.loop(solver, x0, 10 if N < 100000 else 3)
        rollout = base.stage_us(solver, x0, n)
        vals = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solver.forward(x0)
            torch.cuda.synchronize()
            vals.append((time.perf_counter() - t0) * 1e6)
        del solver
        torch.cuda.empty_cache()
        return rollout, statistics.median(vals)

    out = {}
    for N, T, n in SIZES:
        for name in MODELS:
            for variant in variants:
                key = f"N={N} T={T} {name} {variant}"
                out[key + " rollout"], out[key + " solve"] = timed(name, N, T, n, variant)
    if "value" in variants:  # what the feature is for: a short horizon with the value against the long one without
        key = "N=4096 T=8 mlp41 value"
        out[key + " rollout"], out[key + " solve"] = timed("mlp41", 4096, 8, 40, "value")
    key = "N=4096 T=8 mlp41 none"
    out[key + " rollout"], out[key + " solve"] = timed("mlp41", 4096, 8, 40, "none")
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
    runs = {"this": ("", ",".join(VARIANTS)), "parent": (os.path.abspath(args.parent), "none,ref")}
    res = {who: {} for who in runs}
    for rnd in range(args.rounds):
        for who in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):
            lib, variants = runs[who]
            env = dict(os.environ)
            env.pop("MPPI_HIP_LIB", None)
            if lib:
                env["MPPI_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent", args.parent, "--child", variants], env=env,
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"round {rnd} {who} failed (exit {r.returncode}): {r.stderr[-600:]}", flush=True)
                return 2
            for k, v in json.loads(line[0][7:]).items():
                res[who].setdefault(k, []).append(v)
            print(f"round {rnd} {who}: done", flush=True)
    print(f"{'figure (us)':44s} {'this: median [min, max]':34s} parent: median [min, max]")
    for k in res["this"]:
        v = res["this"][k]
        cell = f"{statistics.median(v):10.2f} [{min(v):10.2f}, {max(v):10.2f}]"
        p = res["parent"].get(k)
        if p is None:
            print(f"{k:44s} {cell}")
            continue
        inside = min(p) <= statistics.median(v) <= max(p)
        print(f"{k:44s} {cell}   {statistics.median(p):10.2f} [{min(p):10.2f}, {max(p):10.2f}]  {'inside' if inside else 'OUTSIDE'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
