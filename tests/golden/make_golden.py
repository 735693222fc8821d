#!/usr/bin/env python3
"""Golden-vector generator (TEST INFRASTRUCTURE — runs only in the build container).

Imports the *real* reference (``/root/reference``, read-only, CPU) and records the
inputs/outputs of ``pi_mpc.mppi.MPPI.forward`` for the five shipped models into small
``.npz`` fixtures under ``tests/golden/``.  Nothing from the reference (source,
bytecode) is written into the fixtures: they hold arrays only.

Usage (container only; the GPU box has no /root/reference):
    python tests/golden/make_golden.py            # every small case (N <= 4096) + env artefacts + RNG stream + model pins
    python tests/golden/make_golden.py round2     # only the cases added in round 2 (dense softmax at N = 4096,
                                                  # racing / nav2d with SG, exploration, LBPS, MPO, ESSPS end point,
                                                  # get_samples_from_posterior between two solves)
    python tests/golden/make_golden.py round5     # only the cases added in round 5 (LBPS / MPO at N = 4096 on nav2d and
                                                  # racing, ESSPS clamped at lambda_min and at lambda_max; noise by seed)
    python tests/golden/make_golden.py fullsize [c2|c5|c3|c4 ...]
                                                  # BASELINE.json's configs at FULL size through the real reference,
                                                  # seed 42, two closed-loop solves; outputs and summaries only (< 100 KB)
    python tests/golden/make_golden.py only <substring> [...]   # the small cases whose name contains a substring
    python tests/golden/make_golden.py closures   # the classic-control examples' own closures as pi_mpc.recognize sees them:
                                                  # their fingerprints (sha256) and their values on its probe batches

Recipe follows SURVEY.md Appendix C: stub the UI-only imports (moviepy, fire,
gymnasium), run with cwd=/root/reference (racing_env.py:47-49 opens a relative CSV),
extract the nested model closures of example/{pendulum,cartpole,mountaincar}.py with
``ast`` and run them eagerly.
"""
from __future__ import annotations

import ast
import os
import sys
import textwrap
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    sys.path[:0] = [f"{REF}/src", f"{REF}/example"]
    for n in [
        "moviepy",
        "moviepy.video",
        "moviepy.video.io",
        "moviepy.video.io.ImageSequenceClip",
        "fire",
        "gymnasium",
    ]:
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["moviepy.video.io.ImageSequenceClip"].ImageSequenceClip = object
    sys.modules["fire"].Fire = lambda f: None
    gym = sys.modules["gymnasium"]  # GoalInDangerZoneEnv subclasses gym.Env and builds spaces.Box in __init__
    gym.Env = object
    gym.spaces = types.ModuleType("gymnasium.spaces")
    gym.spaces.Box = lambda *a, **k: None
    sys.modules["gymnasium.spaces"] = gym.spaces
    import matplotlib

    matplotlib.use("Agg")
    os.chdir(REF)


def _extract_closures(path: str, names):
    """Pull nested FunctionDefs out of ``main()`` of an example script (eager, no jit)."""
    import torch

    src = open(path).read()
    tree = ast.parse(src)
    ns = {"torch": torch}
    # module-level angle_normalize (drop the jit decorator)
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "angle_normalize":
            node.decorator_list = []
            seg = ast.unparse(node)
            exec(seg, ns)
    main = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    out = {}
    for node in main.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.decorator_list = []
            seg = textwrap.dedent(ast.unparse(node))
            exec(seg, ns)
            out[node.name] = ns[node.name]
    return out


def pack_bits(m: np.ndarray) -> np.ndarray:
    return np.packbits((m != 0).astype(np.uint8).ravel())


class Recorder:
    """Wraps cost_func to capture the per-call costs the solver sums (mppi.py:307-336).

    `feed`: when set to a tensor [N], the wrapped cost is NOT evaluated: the first call of the solve returns `feed` and
    the other T calls return zeros, so that `torch.sum(costs, dim=1) + terminal` (mppi.py:333-334) is exactly `feed` and
    the REFERENCE's own steps 4-8 (temperature rule, softmax, weighted mean, SG filter, batch-1 rollout, warm start:
    mppi.py:341-460) run on prescribed total costs — the sensitivity probes below."""

    def __init__(self, fn):
        self.fn = fn
        self.calls = []
        self.feed = None

    def __call__(self, state, action, info):
        if self.feed is not None:
            first = not self.calls
            self.calls.append(None)
            return self.feed.clone() if first else torch_zeros_like(self.feed)
        c = self.fn(state, action, info)
        self.calls.append(c.detach().clone())
        return c


def torch_zeros_like(t):
    import torch

    return torch.zeros_like(t)


# ---------------------------------------------------------------------------------------------------------------------
# The reference's OWN sensitivity to fp32 rounding of its costs ("bands").  forward() turns the N total costs into the
# action sequence through softmax(-c / lambda): a cost change dc moves a weight by w * dc / lambda, so the 1e-5 the
# north star asks of action_seq / state_seq is a statement about the costs to ~1e-5 * lambda — below one fp32 ulp of the
# cost for nav2d / goal zone at lambda = 1.  Instead of deriving a tolerance analytically, every fixture records how far
# the reference's own outputs move when its total costs are replaced by equally valid fp32 evaluations of the same
# sums.
# VARIANTS (index = row of every band array; round 5: 256 probes instead of 24, so that a band is a measurement — the tests
# hold the HIP path to 1.0 x the sample maximum and the report also gives the 99th percentile):
#   ulp_0..159        every total cost moved to the next fp32 value up or down (seeded random signs): a 1-ulp change
#   f64sum            the T stage costs + terminal re-summed in float64, rounded once to fp32 (the exactly rounded sum —
#                     what the HIP kernels compute for every model but racing, mppi_models.hpp: CostSum)
#   seqsum / revsum   the same terms summed sequentially in fp32, t = 0..T-1 then the terminal (the racing kernel's
#                     order) / terminal first, then t = T-1..0
#   pairsum           the same terms summed as a balanced pairwise tree in fp32 (torch.sum's own order is a vectorised
#                     cascade that depends on the CPU's ISA: all of these are valid fp32 evaluations of the same sum)
#   stage_ulp_0..91   every stage cost and the terminal moved by one fp32 ulp (seeded signs), then summed by the
#                     reference's own torch.sum(dim=1) + terminal: a different-but-valid fp32 evaluation of each term
# A band is the maximum over the variants: a sample of the reference's spread under rounding-level changes of its costs,
# against which the tests hold the HIP path's distance to the reference: err <= max(1e-5, band).
N_ULP, N_STAGE_ULP = 160, 92
BAND_VARIANTS = (tuple(f"ulp_{i}" for i in range(N_ULP)) + ("f64sum", "seqsum", "revsum", "pairsum")
                 + tuple(f"stage_ulp_{i}" for i in range(N_STAGE_ULP)))
assert len(BAND_VARIANTS) == 256


def _variant_costs(v: int, costs, stage, terminal):
    import torch

    name = BAND_VARIANTS[v]
    rng = np.random.default_rng(9000 + v)
    if name.startswith("ulp_"):
        sign = torch.from_numpy(rng.choice(np.float32([-1.0, 1.0]), size=costs.shape[0]))
        return torch.nextafter(costs, costs + sign * float("inf"))
    if name == "f64sum":
        return (stage.double().sum(dim=1) + terminal.double()).float()
    if name == "seqsum":
        acc = torch.zeros_like(terminal)
        for t in range(stage.shape[1]):
            acc = acc + stage[:, t]
        return acc + terminal
    if name == "revsum":
        acc = terminal.clone()
        for t in reversed(range(stage.shape[1])):
            acc = acc + stage[:, t]
        return acc
    if name == "pairsum":
        terms = [stage[:, t] for t in range(stage.shape[1])] + [terminal]
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    sign = torch.from_numpy(rng.choice(np.float32([-1.0, 1.0]), size=tuple(stage.shape)))
    st = torch.nextafter(stage, stage + sign * float("inf"))
    sign_t = torch.from_numpy(rng.choice(np.float32([-1.0, 1.0]), size=terminal.shape[0]))
    return torch.sum(st, dim=1) + torch.nextafter(terminal, terminal + sign_t * float("inf"))


class FeedDynamics:
    """Wraps the dynamics callable of a recorded solver.  While the Recorder feeds prescribed total costs, the N-sample
    rollout (mppi.py:280-336) cannot influence anything the probes measure — steps 4-8 read the costs, the clamped
    actions and, for state_seq, the batch-1 rollout only — so the N-row calls return their input untouched and the 256
    probes per solve cost a softmax each instead of a rollout each.  Batch-1 calls (the solution's rollout,
    mppi.py:448-449,508-524) always run the real dynamics.  run_case() asserts that a fed solve with the recorded costs
    reproduces the recorded solve bit for bit THROUGH this wrapper."""

    def __init__(self, fn, rec, num_samples):
        self.fn, self.rec, self.n = fn, rec, num_samples

    def __call__(self, state, action):
        if self.rec.feed is not None and self.n > 1 and state.shape[0] == self.n:
            return state
        return self.fn(state, action)


def _snapshot(solver):
    import copy

    import torch

    s = dict(prev=solver._previous_action_seq.detach().clone(), hist=solver._actions_history_for_sg.detach().clone(),
             lam=solver._lambda, auto=solver._auto_lambda, rng=torch.get_rng_state())
    if hasattr(solver, "optimizer"):  # MPO: the dual and its Adam moments (mppi.py:191-200)
        s["logT"] = solver.log_temperature.data.clone()
        s["opt"] = copy.deepcopy(solver.optimizer.state_dict())
    return s


def _restore(solver, s):
    import copy

    import torch

    solver._previous_action_seq = s["prev"].clone()
    solver._actions_history_for_sg = s["hist"].clone()
    solver._lambda, solver._auto_lambda = s["lam"], s["auto"]
    torch.set_rng_state(s["rng"])
    if "opt" in s:
        solver.log_temperature.data.copy_(s["logT"])
        solver.optimizer.load_state_dict(copy.deepcopy(s["opt"]))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _feed_solve(solver, rec, state, costs):
    rec.calls.clear()
    rec.feed = costs
    try:
        a, s = solver.forward(state=state.clone())
    finally:
        rec.feed = None
        rec.calls.clear()
    return a.detach().numpy().copy(), s.detach().numpy().copy()


MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
assert MODE in ("all", "round2", "round5", "fullsize", "only", "closures"), MODE
ONLY_ROUND2 = MODE == "round2"
PARTIAL = MODE != "all"  # env artefacts, RNG stream and model pins are rewritten by the full run only
ROUND2 = set()  # names registered with round2=True


def _selected(name, round2=False, round5=False):
    if MODE == "all":
        return True
    if MODE == "round2":
        return round2
    if MODE == "round5":
        return round5
    if MODE == "only":
        return any(sub in name for sub in sys.argv[2:])
    return False  # fullsize: handled by run_case_full


def run_case(name, make_solver, x0, K, next_state, keep_S, before_solve=None, round2=False, posterior_after=None,
             round5=False, eps_by_seed=False):
    """Run K closed-loop solves and dump everything the parity tests need.  posterior_after = (k, n): call
    get_samples_from_posterior(action_seq_k, state, n) right after solve k (mppi.py:489-506) and record it — the draw
    comes from the same global generator, so the noise of solve k+1 pins the stream position.
    eps_by_seed: the [N,T,dc] noise blocks are NOT stored (they are torch's CPU stream from seed 42, which
    oracle/mppi_oracle.c restates and torch_cpu_randn.npz pins: tests/helpers.py regenerates them); a float64 checksum and
    the first / last rows are kept to verify the regenerated blocks."""
    import torch

    if round2:
        ROUND2.add(name)
    if not _selected(name, round2, round5):
        return

    solver, rec, extra = make_solver()
    N, T = solver._num_samples, solver._horizon
    d = dict(extra)
    if eps_by_seed:
        d["eps_by_seed"] = np.int64(42)
        d["sigmas"] = solver._sigmas.numpy().copy() if hasattr(solver, "_sigmas") else np.zeros(0, np.float32)
    else:
        d["ctor_eps"] = solver._action_noises.numpy().copy()  # Q2: ctor consumes one draw
    state = torch.as_tensor(np.asarray(x0), dtype=torch.float32)
    auto = solver._auto_lambda
    for k in range(K):
        if before_solve is not None:
            for kk, vv in before_solve(state, k).items():
                d[f"{kk}_{k}"] = vv
        rec.calls.clear()
        mean_in = solver._previous_action_seq.detach().clone().numpy()
        hist_in = solver._actions_history_for_sg.detach().clone().numpy()
        pre = _snapshot(solver)
        a, s = solver.forward(state=state.clone())
        calls = list(rec.calls)
        # first T+1 calls belong to the N-sample pass; (no cost calls in the B=1 rollout)
        stage = torch.stack(calls[:T], dim=1)
        terminal = calls[T]
        costs = torch.sum(stage, dim=1) + terminal  # exactly mppi.py:333-334
        d[f"x0_{k}"] = state.numpy().copy()
        d[f"mean_in_{k}"] = mean_in
        d[f"sg_hist_in_{k}"] = hist_in
        if eps_by_seed:
            e = solver._action_noises.numpy()
            d[f"eps_sum64_{k}"] = np.float64(e.astype(np.float64).sum())
            d[f"eps_head_{k}"], d[f"eps_tail_{k}"] = e[:2].copy(), e[-1:].copy()
        else:
            d[f"eps_{k}"] = solver._action_noises.numpy().copy()
        d[f"costs_{k}"] = costs.numpy().copy()
        d[f"stage_costs_{k}"] = stage.numpy().copy() if keep_S else np.zeros(0, np.float32)
        d[f"lambda_{k}"] = np.float64(solver._lambda)
        d[f"weights_{k}"] = solver._weights.detach().numpy().copy()
        d[f"action_seq_{k}"] = a.detach().numpy().copy()
        d[f"state_seq_{k}"] = s.detach().numpy().copy()
        if keep_S:
            d[f"U_{k}"] = solver._perturbed_action_seqs.numpy().copy()
            d[f"S_{k}"] = solver._state_seq_batch.numpy().copy()
        if k == 0 and N >= 8:
            ts, tw = solver.get_top_samples(8)
            d["top8_states_0"] = ts.numpy().copy()
            d["top8_weights_0"] = tw.detach().numpy().copy()
        if posterior_after is not None and posterior_after[0] == k:
            ps, pst = solver.get_samples_from_posterior(a, state.clone(), posterior_after[1])
            d["posterior_after"] = np.int64(k)
            d["posterior_samples"] = ps.detach().numpy().copy()
            d["posterior_states"] = pst.detach().numpy().copy()
        # ---- per-solve bands: the reference's steps 4-8 re-run on the SAME inputs with perturbed total costs
        post = _snapshot(solver)
        lam_used = pre["lam"] if auto == "MPO" else solver._lambda  # the temperature of this solve's weights
        a_np, s_np = a.detach().numpy(), s.detach().numpy()
        _restore(solver, pre)  # (sanity: feeding the recorded costs back reproduces the solve bit for bit)
        a_chk, s_chk = _feed_solve(solver, rec, state, costs)
        assert np.array_equal(a_chk, a_np) and np.array_equal(s_chk, s_np) and solver._lambda == post["lam"], name
        nv = len(BAND_VARIANTS)
        fixed = np.zeros((nv, 2))   # [variant] (action, state) at the temperature the reference used
        ruled = np.zeros((nv, 3))   # [variant] (action, state, lambda) with the temperature rule re-run
        for v in range(nv):
            cv = _variant_costs(v, costs, stage, terminal)
            _restore(solver, pre)
            solver._auto_lambda, solver._lambda = None, float(lam_used)
            av, sv = _feed_solve(solver, rec, state, cv)
            fixed[v] = _rel(av, a_np), _rel(sv, s_np)
            if auto is not None:
                _restore(solver, pre)
                av, sv = _feed_solve(solver, rec, state, cv)
                ruled[v] = _rel(av, a_np), _rel(sv, s_np), abs(solver._lambda - post["lam"]) / post["lam"]
        _restore(solver, post)
        d[f"band_fixed_{k}"] = fixed
        if auto is not None:
            d[f"band_rule_{k}"] = ruled
        state = next_state(state, a, s)
    d["K"] = np.int64(K)
    # ---- closed-loop bands: the whole K-solve loop re-run per variant (same seed -> same noise; every solve's total
    # costs replaced by the variant's evaluation of the SAME terms; states, warm start, SG history and the temperature
    # rule's memory all evolve on their own), compared with the unperturbed loop above
    cl = np.zeros((K, len(BAND_VARIANTS), 4))  # [solve][variant] (x0, action, state, lambda)
    for v in range(len(BAND_VARIANTS)):
        solver2, rec2, _ = make_solver()
        st2 = torch.as_tensor(np.asarray(x0), dtype=torch.float32)
        for k in range(K):
            if before_solve is not None:
                before_solve(st2, k)
            rec2.calls.clear()
            pre = _snapshot(solver2)
            solver2.forward(state=st2.clone())
            calls = list(rec2.calls)
            stage2, term2 = torch.stack(calls[:T], dim=1), calls[T]
            costs2 = torch.sum(stage2, dim=1) + term2
            _restore(solver2, pre)
            av, sv = _feed_solve(solver2, rec2, st2, _variant_costs(v, costs2, stage2, term2))
            lam_ref = float(d[f"lambda_{k}"])
            cl[k, v] = (_rel(st2.numpy(), d[f"x0_{k}"]), _rel(av, d[f"action_seq_{k}"]), _rel(sv, d[f"state_seq_{k}"]),
                        abs(float(solver2._lambda) - lam_ref) / lam_ref)
            a2, s2 = torch.from_numpy(av), torch.from_numpy(sv)
            if posterior_after is not None and posterior_after[0] == k:  # keeps the noise stream aligned
                solver2.get_samples_from_posterior(a2, st2.clone(), posterior_after[1])
            st2 = next_state(st2, a2, s2)
    d["band_closed_loop"] = cl
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB)")


def run_case_full(name, make_solver, x0, K, next_state, before_solve=None, nv_fixed=256, nv_closed=32):
    """BASELINE.json's configurations at FULL size through the real reference, seed 42 (its constructor default,
    mppi.py:46,93), K closed-loop solves.  Only outputs and summaries are kept (the noise is torch's CPU stream from the
    seed; the product draws the same stream with noise_source="torch_cpu" and the oracle restates it): per solve the start
    state, temperature, action_seq, state_seq, warm start / SG history going in, min / max / float64 sum / ESS / a 64-bin
    histogram of the N total costs, the 32 smallest (index, cost, weight) triples with their noise rows (pins the stream
    position and the arg-min), checksums of the whole noise block, and the bands (nv_fixed probes per solve, nv_closed
    whole-loop probes: a full-size closed-loop probe is a full rollout per solve)."""
    import time

    import torch

    t0 = time.time()
    solver, rec, extra = make_solver()
    N, T = solver._num_samples, solver._horizon
    d = dict(extra)
    d["N"], d["T"], d["K"], d["seed"] = np.int64(N), np.int64(T), np.int64(K), np.int64(42)
    e0 = solver._action_noises.numpy()
    d["ctor_eps_sum64"] = np.float64(e0.astype(np.float64).sum())
    state = torch.as_tensor(np.asarray(x0), dtype=torch.float32)
    auto = solver._auto_lambda
    vsel_fixed = _spread(nv_fixed)
    vsel_closed = _spread(nv_closed)
    d["band_variants_fixed"], d["band_variants_closed"] = np.int64(vsel_fixed), np.int64(vsel_closed)
    for k in range(K):
        if before_solve is not None:
            for kk, vv in before_solve(state, k).items():
                d[f"{kk}_{k}"] = vv
        rec.calls.clear()
        d[f"mean_in_{k}"] = solver._previous_action_seq.detach().clone().numpy()
        d[f"sg_hist_in_{k}"] = solver._actions_history_for_sg.detach().clone().numpy()
        pre = _snapshot(solver)
        a, s = solver.forward(state=state.clone())
        calls = list(rec.calls)
        rec.calls.clear()
        stage = torch.stack(calls[:T], dim=1)
        terminal = calls[T]
        del calls
        costs = torch.sum(stage, dim=1) + terminal  # exactly mppi.py:333-334
        c = costs.numpy()
        w = solver._weights.detach().numpy()
        eps = solver._action_noises.numpy()
        order = np.lexsort((np.arange(N), c))[:32]  # ascending cost, then index
        d[f"x0_{k}"] = state.numpy().copy()
        d[f"lambda_{k}"] = np.float64(solver._lambda)
        d[f"action_seq_{k}"] = a.detach().numpy().copy()
        d[f"state_seq_{k}"] = s.detach().numpy().copy()
        d[f"cmin_{k}"], d[f"cmax_{k}"] = np.float32(c.min()), np.float32(c.max())
        d[f"costs_sum64_{k}"] = np.float64(c.astype(np.float64).sum())
        w64 = w.astype(np.float64)
        d[f"ess_{k}"] = np.float64(1.0 / np.sum(w64 * w64))
        d[f"wsum64_{k}"] = np.float64(w64.sum())
        d[f"wmax_{k}"] = np.float32(w.max())
        edges = np.linspace(float(c.min()), float(c.max()), 65)
        d[f"hist_edges_{k}"] = edges
        d[f"hist_{k}"] = np.histogram(c.astype(np.float64), bins=edges)[0].astype(np.int64)
        # quantiles of the cost distribution at sample ranks (robust against single bin-edge flips)
        qs = np.array([0.001, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
        d[f"quantile_ranks_{k}"] = (qs * (N - 1)).astype(np.int64)
        d[f"quantiles_{k}"] = np.sort(c)[d[f"quantile_ranks_{k}"]]
        d[f"top32_idx_{k}"] = order.astype(np.int64)
        d[f"top32_cost_{k}"] = c[order].copy()
        d[f"top32_weight_{k}"] = w[order].copy()
        d[f"top32_eps_{k}"] = eps[order].copy()
        d[f"top32_stage_{k}"] = stage.numpy()[order].copy()
        d[f"top32_terminal_{k}"] = terminal.numpy()[order].copy()
        e64 = eps.astype(np.float64)
        d[f"eps_sum64_{k}"], d[f"eps_sumsq64_{k}"] = np.float64(e64.sum()), np.float64((e64 * e64).sum())
        d[f"eps_head_{k}"], d[f"eps_tail_{k}"] = eps[:2].copy(), eps[-1:].copy()
        del e64, eps, w, w64, c
        # ---- per-solve bands (the reference's steps 4-8 on prescribed costs; see run_case)
        post = _snapshot(solver)
        lam_used = pre["lam"] if auto == "MPO" else solver._lambda
        a_np, s_np = a.detach().numpy(), s.detach().numpy()
        _restore(solver, pre)
        a_chk, s_chk = _feed_solve(solver, rec, state, costs)
        assert np.array_equal(a_chk, a_np) and np.array_equal(s_chk, s_np) and solver._lambda == post["lam"], name
        if k == 0:  # the dim-0 reductions of steps 4-6 under another thread count: same bits?
            nt = torch.get_num_threads()
            torch.set_num_threads(1)
            _restore(solver, pre)
            a1, s1 = _feed_solve(solver, rec, state, costs)
            d["one_thread_same_bits"] = np.bool_(np.array_equal(a1, a_np) and np.array_equal(s1, s_np)
                                                 and solver._lambda == post["lam"])
            d["one_thread_action_rel"] = np.float64(_rel(a1, a_np))
            torch.set_num_threads(nt)
        fixed = np.zeros((len(vsel_fixed), 2))
        ruled = np.zeros((len(vsel_fixed), 3))
        for j, v in enumerate(vsel_fixed):
            cv = _variant_costs(v, costs, stage, terminal)
            _restore(solver, pre)
            solver._auto_lambda, solver._lambda = None, float(lam_used)
            av, sv = _feed_solve(solver, rec, state, cv)
            fixed[j] = _rel(av, a_np), _rel(sv, s_np)
            if auto is not None:
                _restore(solver, pre)
                av, sv = _feed_solve(solver, rec, state, cv)
                ruled[j] = _rel(av, a_np), _rel(sv, s_np), abs(solver._lambda - post["lam"]) / post["lam"]
        _restore(solver, post)
        d[f"band_fixed_{k}"] = fixed
        if auto is not None:
            d[f"band_rule_{k}"] = ruled
        print(f"  {name}: solve {k} done at {time.time() - t0:.0f} s, lambda {solver._lambda:.6g}, ess {d[f'ess_{k}']:.4g}, "
              f"band action {fixed[:, 0].max():.2e}", flush=True)
        del stage, terminal, costs
        state = next_state(state, a, s)
    # ---- closed-loop bands (the first solver is released first: at C4 one solver is 30 GB of the reference's buffers)
    import gc

    del solver, rec, pre, post
    gc.collect()
    cl = np.zeros((K, len(vsel_closed), 4))
    for j, v in enumerate(vsel_closed):
        solver2, rec2, _ = make_solver()
        st2 = torch.as_tensor(np.asarray(x0), dtype=torch.float32)
        for k in range(K):
            if before_solve is not None:
                before_solve(st2, k)
            rec2.calls.clear()
            pre = _snapshot(solver2)
            solver2.forward(state=st2.clone())
            calls = list(rec2.calls)
            rec2.calls.clear()
            stage2, term2 = torch.stack(calls[:T], dim=1), calls[T]
            del calls
            costs2 = torch.sum(stage2, dim=1) + term2
            _restore(solver2, pre)
            av, sv = _feed_solve(solver2, rec2, st2, _variant_costs(v, costs2, stage2, term2))
            lam_ref = float(d[f"lambda_{k}"])
            cl[k, j] = (_rel(st2.numpy(), d[f"x0_{k}"]), _rel(av, d[f"action_seq_{k}"]), _rel(sv, d[f"state_seq_{k}"]),
                        abs(float(solver2._lambda) - lam_ref) / lam_ref)
            a2, s2 = torch.from_numpy(av), torch.from_numpy(sv)
            st2 = next_state(st2, a2, s2)
        del solver2, rec2, stage2, term2, costs2
        print(f"  {name}: closed-loop probe {j + 1}/{len(vsel_closed)} at {time.time() - t0:.0f} s", flush=True)
    d["band_closed_loop"] = cl
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.0f} KiB) in {time.time() - t0:.0f} s")


def _spread(n):
    """n of the 256 variant indices, every class represented: the four re-summations always, the rest evenly."""
    n = min(n, len(BAND_VARIANTS))
    special = [N_ULP, N_ULP + 1, N_ULP + 2, N_ULP + 3][:max(n, 1)]
    rest = [v for v in range(len(BAND_VARIANTS)) if v not in special]
    take = max(n - len(special), 0)
    idx = sorted(set(special + [rest[int(i * len(rest) / max(take, 1))] for i in range(take)]))
    return idx


def main():
    _import_reference()
    import torch

    torch.set_num_threads(1)
    from pi_mpc.mppi import MPPI

    cpu = torch.device("cpu")

    def pred_next(state, a, s):
        # closed loop without a simulator: apply the predicted next state.
        return s[0, 1].detach().clone()

    # ------------------------------------------------------------ classic control
    def classic(example, dyn_name, cost_name, **kw):
        fns = _extract_closures(f"{REF}/example/{example}.py", [dyn_name, cost_name])

        def make():
            rec = Recorder(fns[cost_name])
            solver = MPPI(dynamics=FeedDynamics(fns[dyn_name], rec, kw["num_samples"]), cost_func=rec, device=cpu, **kw)
            return solver, rec, {}

        return make

    pend = dict(dim_state=2, dim_control=1, u_min=torch.tensor([-2.0]), u_max=torch.tensor([2.0]),
                sigmas=torch.tensor([1.0]))
    x0_pend = [np.pi, 0.0]
    run_case("pendulum_T50_N1000_essps",
             classic("pendulum", "dynamics", "cost_function", horizon=50, num_samples=1000,
                     lambda_="ESSPS", **pend), x0_pend, 3, pred_next, keep_S=False)
    run_case("pendulum_T15_N256_fixed",
             classic("pendulum", "dynamics", "cost_function", horizon=15, num_samples=256,
                     lambda_=1.0, **pend), x0_pend, 3, pred_next, keep_S=True)
    run_case("pendulum_T15_N256_lbps",
             classic("pendulum", "dynamics", "cost_function", horizon=15, num_samples=256,
                     lambda_="LBPS", **pend), x0_pend, 3, pred_next, keep_S=False)
    run_case("pendulum_T15_N256_mpo",
             classic("pendulum", "dynamics", "cost_function", horizon=15, num_samples=256,
                     lambda_="MPO", **pend), x0_pend, 3, pred_next, keep_S=False)
    run_case("pendulum_T15_N200_explore",
             classic("pendulum", "dynamics", "cost_function", horizon=15, num_samples=200,
                     lambda_=0.5, exploration=0.25, **pend), x0_pend, 3, pred_next, keep_S=True)

    cart = dict(dim_state=4, dim_control=1, u_min=torch.tensor([-3.0]), u_max=torch.tensor([3.0]),
                sigmas=torch.tensor([1.0]))
    x0_cart = [0.01, 0.0, 0.02, 0.0]
    run_case("cartpole_T64_N1024_essps_sg",
             classic("cartpole", "dynamics", "stage_cost", horizon=64, num_samples=1024,
                     lambda_="ESSPS", use_sg_filter=True, **cart), x0_cart, 3, pred_next, keep_S=False)
    run_case("cartpole_T10_N100_fixed",
             classic("cartpole", "dynamics", "stage_cost", horizon=10, num_samples=100,
                     lambda_=0.001, **cart), x0_cart, 3, pred_next, keep_S=True)

    mc = dict(dim_state=2, dim_control=1, u_min=torch.tensor([-1.0]), u_max=torch.tensor([1.0]),
              sigmas=torch.tensor([1.0]))
    run_case("mountaincar_T100_N256_fixed",
             classic("mountaincar", "dynamics", "cost_func", horizon=100, num_samples=256,
                     lambda_=0.1, **mc), [-0.5, 0.0], 3, pred_next, keep_S=True)

    # MuJoCo-style cart-pole (example/mujoco_cartpole.py:20-79): continuous force, masspole = 1
    run_case("mjcartpole_T50_N256_fixed",
             classic("mujoco_cartpole", "dynamics", "cost_func", horizon=50, num_samples=256,
                     lambda_=1.0, **cart), [0.01, 0.0, 0.05, 0.0], 3, pred_next, keep_S=True)

    # ------------------------------------------------------------ goal in danger zone
    from envs.goal_in_danger_zone import GoalInDangerZoneEnv

    np.random.seed(42)
    gz = GoalInDangerZoneEnv(render_mode="rgb_array", seed=42)
    gz._set_goal(gz._danger_zone)
    gz._set_initial_state(gz._danger_zone)
    gz_x0 = np.concatenate([gz._pos, [gz._angle], gz._goal - gz._pos,
                            np.array(gz._danger_zone.center) - gz._pos]).astype(np.float32)
    gz_extra = {"goal": np.asarray(gz._goal, np.float64), "center": np.asarray(gz._danger_zone.center, np.float64),
                "radius": np.float64(gz._danger_zone.radius), "x0": gz_x0}
    if not PARTIAL:
        np.savez_compressed(os.path.join(OUT, "goalzone_env.npz"), **gz_extra)

    def goalzone(**kw):
        def make():
            rec = Recorder(gz.parallel_cost)
            solver = MPPI(dim_state=7, dim_control=2, dynamics=FeedDynamics(gz.parallel_step, rec, kw["num_samples"]),
                          cost_func=rec,
                          u_min=torch.tensor([-1.0, -1.0]), u_max=torch.tensor([1.0, 1.0]),
                          sigmas=torch.tensor([0.5, 0.5]), device=cpu, **kw)
            return solver, rec, {}

        return make

    run_case("goalzone_T30_N256_fixed", goalzone(horizon=30, num_samples=256, lambda_=1.0), gz_x0, 3, pred_next,
             keep_S=True)

    # ------------------------------------------------------------ navigation 2d
    from envs.navigation_2d import Navigation2DEnv

    nav_env = Navigation2DEnv(device=cpu)
    nav_map = nav_env._obstacle_map._map
    nav_extra = {
        "map_bits": pack_bits(nav_map),
        "map_shape": np.array(nav_map.shape, np.int64),
        "cell_size": np.float64(nav_env._obstacle_map._cell_size),
        "origin": np.array(nav_env._obstacle_map._cell_map_origin, np.int64),
        "x_lim": np.array(nav_env._obstacle_map.x_lim, np.float64),
        "y_lim": np.array(nav_env._obstacle_map.y_lim, np.float64),
        "circles": np.array([[c.center[0], c.center[1], c.radius]
                             for c in nav_env._obstacle_map.circle_obs_list], np.float64),
        "rects": np.array([[r.center[0], r.center[1], r.width, r.height]
                           for r in nav_env._obstacle_map.rectangle_obs_list], np.float64),
        "goal": nav_env._goal_pos.numpy().copy(),
        "start_state": nav_env._robot_state.numpy().copy(),
    }

    def nav(**kw):
        def make():
            rec = Recorder(nav_env.cost_function)
            solver = MPPI(dim_state=3, dim_control=2, dynamics=FeedDynamics(nav_env.dynamics, rec, kw["num_samples"]),
                          cost_func=rec,
                          u_min=nav_env.u_min, u_max=nav_env.u_max,
                          sigmas=torch.tensor([0.5, 0.5]), device=cpu, **kw)
            return solver, rec, {}

        return make

    if not PARTIAL:
        np.savez_compressed(os.path.join(OUT, "nav2d_env.npz"), **nav_extra)

    x0_nav = nav_env._robot_state.numpy().copy()
    run_case("nav2d_T50_N512_essps", nav(horizon=50, num_samples=512, lambda_="ESSPS"),
             x0_nav, 3, pred_next, keep_S=False)
    run_case("nav2d_T30_N256_fixed_explore", nav(horizon=30, num_samples=256, lambda_=1.0,
                                                 exploration=0.25),
             x0_nav, 3, pred_next, keep_S=True)
    # round 2: dense softmax at N = 4096, the other temperature rules, SG, the posterior draw
    run_case("nav2d_T30_N4096_essps", nav(horizon=30, num_samples=4096, lambda_="ESSPS"), x0_nav, 2, pred_next,
             keep_S=False, round2=True)
    run_case("nav2d_T30_N512_lbps", nav(horizon=30, num_samples=512, lambda_="LBPS"), x0_nav, 3, pred_next,
             keep_S=False, round2=True)
    run_case("nav2d_T30_N512_mpo", nav(horizon=30, num_samples=512, lambda_="MPO"), x0_nav, 3, pred_next,
             keep_S=False, round2=True)
    run_case("nav2d_T30_N512_sg", nav(horizon=30, num_samples=512, lambda_=5.0, use_sg_filter=True,
                                      sg_window_size=7, sg_poly_order=2), x0_nav, 3, pred_next, keep_S=False,
             round2=True)
    run_case("nav2d_T20_N256_posterior", nav(horizon=20, num_samples=256, lambda_=5.0), x0_nav, 3, pred_next,
             keep_S=False, round2=True, posterior_after=(0, 16))

    # ------------------------------------------------------------ racing
    import racing as racing_example  # example/racing.py (fire stubbed)
    from envs.racing_env import RacingEnv

    env = RacingEnv(device=cpu)
    obst = env._obstacle_map._map
    lane = env._lane_map._map
    racing_extra = {
        "center_path": env.racing_center_path.numpy().copy(),  # [3678,3] f32
        "center_path_f64": None,
        "obst_bits": pack_bits(obst),
        "lane_bits": pack_bits(lane),
        "map_shape": np.array(obst.shape, np.int64),
        "cell_size": np.float64(env.cell_size),
        "origin": np.array(env._obstacle_map._cell_map_origin, np.int64),
        "lane_origin": np.array(env._lane_map._cell_map_origin, np.int64),
        "x_lim": np.array(env._obstacle_map.x_lim, np.float64),
        "y_lim": np.array(env._obstacle_map.y_lim, np.float64),
        "circles": np.array([[c.center[0], c.center[1], c.radius]
                             for c in env._obstacle_map.circle_obs_list], np.float64),
        "start_state": env._robot_state.numpy().copy(),
        "lane_width": np.float64(env.line_width * 0.8),
    }
    # float64 centre path as produced by the circuit generator (LaneMap input)
    from envs.circuit_generator.path_generate import make_csv_paths

    cp64, _, _ = make_csv_paths("src/envs/circuit_generator/circuit.csv")
    racing_extra["center_path_f64"] = cp64
    if not PARTIAL:
        np.savez_compressed(os.path.join(OUT, "racing_env.npz"), **racing_extra)

    def racing_parts(T, N, lambda_=1.0, **kw):
        """(make_solver, before_solve, next_state) of a racing closed loop (example/racing.py:221-266 minus rendering)."""
        ctrl_box = {}

        def make():
            import gc

            ctrl_box.clear()  # (the previous controller and its solver go first: at C4 one solver is 30 GB)
            gc.collect()
            ctrl = racing_example.racing_controller(env, debug=False, device=cpu)
            ctrl.set_cost_map(env._obstacle_map, env._lane_map)
            rec = Recorder(ctrl.cost_function)
            ctrl.solver = MPPI(horizon=T, num_samples=N, dim_state=4, dim_control=2,
                               dynamics=FeedDynamics(env.dynamics, rec, N), cost_func=rec, u_min=env.u_min,
                               u_max=env.u_max, sigmas=torch.tensor([0.5, 0.1]), lambda_=lambda_,
                               device=cpu, **kw)
            ctrl_box["c"] = ctrl
            return ctrl.solver, rec, {}

        def before(state, k):
            ctrl = ctrl_box["c"]
            cind_in = ctrl.current_path_index
            ref, ind = ctrl.calc_ref_trajectory(state, env.racing_center_path, cind_in,
                                                ctrl.solver._horizon, DL=0.1,
                                                lookahead_distance=3,
                                                reference_path_interval=0.85)
            ctrl.reference_path, ctrl.current_path_index = ref, ind
            return {"ref_path": ref.numpy().copy(), "cind_in": np.int64(cind_in),
                    "cind_out": np.int64(ind)}

        def nxt(state, a, s):
            u = torch.clamp(a[0], env.u_min, env.u_max)
            return env.dynamics(state.unsqueeze(0), u.unsqueeze(0)).squeeze(0).detach().clone()

        return make, before, nxt

    def racing_case(name, T, N, K, keep_S, lambda_=1.0, round2=False, round5=False, eps_by_seed=False, **kw):
        if not _selected(name, round2, round5):
            return
        make, before, nxt = racing_parts(T, N, lambda_, **kw)
        run_case(name, make, env._robot_state.numpy().copy(), K, nxt, keep_S, before_solve=before, round2=round2,
                 round5=round5, eps_by_seed=eps_by_seed)

    racing_case("racing_T50_N512_fixed", 50, 512, 3, keep_S=False)
    racing_case("racing_T25_N256_fixed", 25, 256, 3, keep_S=True)
    # round 2: a dense softmax at the example's sample count, exploration + SG, ESSPS end point
    racing_case("racing_T25_N4096_dense", 25, 4096, 3, keep_S=False, lambda_=500.0, round2=True)
    racing_case("racing_T25_N512_explore_sg", 25, 512, 3, keep_S=False, lambda_=200.0, round2=True,
                exploration=0.25, use_sg_filter=True)
    racing_case("racing_T25_N1024_essps", 25, 1024, 2, keep_S=False, lambda_="ESSPS", round2=True)

    # round 5 (VERDICT r4 #2c): the other temperature rules at the examples' sample count on nav2d AND racing, and one
    # ESSPS case per end-point rule (mppi.py:361-364).  Noise by seed (not stored).
    run_case("nav2d_T30_N4096_lbps", nav(horizon=30, num_samples=4096, lambda_="LBPS"), x0_nav, 2, pred_next,
             keep_S=False, round5=True, eps_by_seed=True)
    run_case("nav2d_T30_N4096_mpo", nav(horizon=30, num_samples=4096, lambda_="MPO"), x0_nav, 3, pred_next,
             keep_S=False, round5=True, eps_by_seed=True)
    racing_case("racing_T25_N4096_lbps", 25, 4096, 2, keep_S=False, lambda_="LBPS", round5=True, eps_by_seed=True)
    racing_case("racing_T25_N4096_mpo", 25, 4096, 3, keep_S=False, lambda_="MPO", round5=True, eps_by_seed=True)
    run_case("nav2d_T30_N512_essps_at_min", nav(horizon=30, num_samples=512, lambda_="ESSPS", lambda_min=40.0,
                                                lambda_max=100.0), x0_nav, 2, pred_next, keep_S=False, round5=True,
             eps_by_seed=True)
    run_case("nav2d_T30_N512_essps_at_max", nav(horizon=30, num_samples=512, lambda_="ESSPS", lambda_max=0.5),
             x0_nav, 2, pred_next, keep_S=False, round5=True, eps_by_seed=True)

    if MODE == "fullsize":
        want = set(sys.argv[2:]) or {"c2", "c5", "c3"}
        threads = int(os.environ.get("GOLDEN_THREADS", "8"))
        torch.set_num_threads(threads)  # (elementwise ops and the reductions along dim 1 do not depend on the thread count;
        #                                 the dim-0 reductions of steps 4-6 are checked below: same bits with 1 thread)
        if "c2" in want:  # BASELINE configs[1]
            run_case_full("full_c2_nav2d_T50_N65536_essps", nav(horizon=50, num_samples=65536, lambda_="ESSPS"), x0_nav, 2,
                          pred_next, nv_fixed=256, nv_closed=64)
        if "c2_lbps" in sys.argv[2:]:  # configs[1]'s size under the reference's OTHER search rule (round 6: LBPS's default moved onto the device)
            run_case_full("full_c2_nav2d_T50_N65536_lbps", nav(horizon=50, num_samples=65536, lambda_="LBPS"), x0_nav, 2,
                          pred_next, nv_fixed=256, nv_closed=64)
        if "c5" in want:  # BASELINE configs[4]
            run_case_full("full_c5_cartpole_T64_N262144_essps_sg",
                          classic("cartpole", "dynamics", "stage_cost", horizon=64, num_samples=262144, lambda_="ESSPS",
                                  use_sg_filter=True, **cart), x0_cart, 2, pred_next, nv_fixed=256, nv_closed=32)
        if "c3" in want:  # BASELINE configs[2], the configuration the metric is quoted on
            make, before, nxt = racing_parts(50, 1 << 20, 1.0)
            run_case_full("full_c3_racing_T50_N1048576_lambda1", make, env._robot_state.numpy().copy(), 2, nxt,
                          before_solve=before, nv_fixed=64, nv_closed=8)
        if "c4" in sys.argv[2:]:  # BASELINE configs[3]: the 8 x 2^20 samples of the sharded run, UNSHARDED through the reference
            # (~35 GB of RSS, minutes per solve: only on request; the probes are few — the regime is C3's arg-min)
            make, before, nxt = racing_parts(50, 1 << 23, 1.0)
            run_case_full("full_c4_racing_T50_N8388608_lambda1", make, env._robot_state.numpy().copy(), 2, nxt,
                          before_solve=before, nv_fixed=8, nv_closed=1)
        return
    if PARTIAL:
        print(f"done ({MODE}):", sorted(ROUND2) if ONLY_ROUND2 else "")
        return
    # ------------------------------------------------------------ torch-CPU RNG stream
    rng = {}
    for seed in (0, 42):
        for n in (1000, 15000):
            torch.manual_seed(seed)
            rng[f"randn_seed{seed}_n{n}_a"] = torch.randn(n).numpy().copy()
            rng[f"randn_seed{seed}_n{n}_b"] = torch.randn(n).numpy().copy()  # consecutive draw
    np.savez_compressed(os.path.join(OUT, "torch_cpu_randn.npz"), **rng)

    # ------------------------------------------------------------ model-level pins
    # angle_normalize / map lookup on random inputs (Appendix A pins)
    g = torch.Generator().manual_seed(7)
    xs = (torch.rand(20000, generator=g) - 0.5) * 40.0
    from envs.racing_env import angle_normalize

    pins = {"an_in": xs.numpy().copy(), "an_out": angle_normalize(xs).numpy().copy()}
    pts = (torch.rand(20000, 1, 2, generator=g) - 0.5) * 90.0
    pins["occ_pts"] = pts.numpy().copy()
    pins["occ_obst"] = env._obstacle_map.compute_cost(pts).numpy().copy()
    pins["occ_lane"] = env._lane_map.compute_cost(pts).numpy().copy()
    pts2 = (torch.rand(20000, 1, 2, generator=g) - 0.5) * 22.0
    pins["occ_nav_pts"] = pts2.numpy().copy()
    pins["occ_nav"] = nav_env._obstacle_map.compute_cost(pts2).numpy().copy()
    np.savez_compressed(os.path.join(OUT, "model_pins.npz"), **pins)
    print("done")


def _example_closures(model):
    """(dynamics, cost) as example/<model>.py holds them — nested definitions inside main(), `dynamics` a TorchScript function,
    the cost a closure over the module-level TorchScript angle_normalize — rebuilt from the reference's file in a scratch
    module outside the repository."""
    import importlib.util
    import tempfile

    fn, dyn_name, cost_name = {"pendulum": ("pendulum.py", "dynamics", "cost_function"),
                               "cartpole": ("cartpole.py", "dynamics", "stage_cost"),
                               "mountaincar": ("mountaincar.py", "dynamics", "cost_func"),
                               "mjcartpole": ("mujoco_cartpole.py", "dynamics", "cost_func")}[model]
    tree = ast.parse(open(os.path.join(REF, "example", fn)).read())
    body = ["import torch\n"]
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "angle_normalize":
            body.append(ast.unparse(node) + "\n")
    main_fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    inner = [textwrap.indent(textwrap.dedent(ast.unparse(n)), "    ") for n in main_fn.body
             if isinstance(n, ast.FunctionDef) and n.name in (dyn_name, cost_name)]
    body.append("def main():\n" + "\n".join(inner) + f"\n    return {dyn_name}, {cost_name}\n")  # nested, like the example
    path = os.path.join(tempfile.mkdtemp(prefix="mppi_ref_example_"), f"ref_example_{model}.py")
    open(path, "w").write("\n".join(body))
    spec = importlib.util.spec_from_file_location(f"ref_example_{model}", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.main()


def record_closures():
    """reference_example_closures.npz: per classic-control model, what pi_mpc.recognize reads from the reference example's
    (dynamics, cost) — every form of their fingerprint (sha256 hex digests), whether each is a TorchScript function, and their
    values on recognize's probe batches (dynamics: what it returns and what it leaves in its state argument).  Hashes and
    arrays only."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    import torch

    import mppi_playground_amd  # noqa: F401  (puts pi_mpc/ and envs/ on sys.path)
    from pi_mpc import recognize

    cpu = torch.device("cpu")
    rec = {"torch": np.array(torch.__version__)}
    for model in ("pendulum", "cartpole", "mountaincar", "mjcartpole"):
        dyn, cost = _example_closures(model)
        s, a = recognize._probes(model, cpu)
        s1 = s.clone()
        out = dyn(s1, a.clone())
        info = {"t": 0, "prev_state": s, "prev_action": a, "initial_state": s}
        rec[f"{model}_dyn_fp"] = np.array(sorted(recognize.fingerprints(dyn)))
        rec[f"{model}_cost_fp"] = np.array(sorted(recognize.fingerprints(cost)))
        rec[f"{model}_dyn_is_script"] = np.array(isinstance(dyn, torch.jit.ScriptFunction))
        rec[f"{model}_cost_is_script"] = np.array(isinstance(cost, torch.jit.ScriptFunction))
        rec[f"{model}_dyn_out"] = out.numpy().copy()
        rec[f"{model}_dyn_arg"] = s1.numpy().copy()
        rec[f"{model}_cost_out"] = cost(s.clone(), a.clone(), dict(info)).numpy().copy()
    np.savez_compressed(os.path.join(OUT, "reference_example_closures.npz"), **rec)
    print("wrote reference_example_closures.npz")


if __name__ == "__main__":
    record_closures() if MODE == "closures" else main()
