"""The tail of a solve — finalize_tail in csrc/mppi_finalize.hpp, reached through mppi_finalize — on summaries written by the
test (tests/tail_cases.py), on a real MI355X: the combine of the shard summaries, the normalisation, the Savitzky-Golay step
with its warm start and history shift, and the batch-1 rollout of the solution in its three completions.

  combine   A generic handle that has done nothing else combines W summaries written here.  Action per column and the head sums
            sum e, sum e^2, sum e*c within TOL = 1e-5 relative of tail_cases.combine_reference (float64 over the fp32 argument
            the kernel forms; rows and sums are positive, so a chain of W <= 64 fused multiply-adds, expf and one quotient cost
            about (W / 2 + 3) * 2^-24 = 2.1e-6: no band), min c exactly.  Equal minima and W = 1 with sum e = 1 are exact and
            held to the bit; a shard whose factor is exactly 0 leaves the result bit-identical to the call without it; any order
            of the live shards stays within the limit; the same temperature read from the device gives the same bits.
  filter    With the one shard {0, 1, 1, 0, A} the tail's action is A bit for bit, so the filter sees rows chosen here.  The
            store_mean = 0 call must not filter and must leave warm start and history untouched; the store_mean = 1 call must
            equal pi_mpc._host.sg_filter_sequence(history, A, taps) BIT FOR BIT (same accumulation order, separate roundings:
            the library is built with contraction off), store it as the warm start and shift a'[0] into the history — over
            three consecutive solves, with the real (symmetric) coefficients and with asymmetric taps that make a reversed or
            mirrored index visible, from a zero and from a caller's history.
  batch-1   Native handles, one shard {0, 1, 1, 0, A}: action_out == A and state_out == mppi_rollout_actions(A) bit for bit at
            math 0, 1 and 2 (racing and racing_discs at T <= 63 with fast math: Model::rollout_wave against the lane-serial
            walk), within 1e-5 of the oracle's single rollout at the default level; with option lazy_state_seq the buffer reads
            all-NaN until mppi_join_state_seq, or the next mppi_sample + mppi_rollout_cost, completes it to the same bits.
Every case prints a `[tail]` line (pytest -s): its error against the limit, or "bit-identical"."""
import ctypes as C

import numpy as np
import pytest
import torch

import tail_cases as tc
from test_gpu_covariance import TOL, _need_gpu

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
E_INVALID = -1
worst = {}  # table -> largest relative error seen (printed with every case)
assert TOL == tc.TOL


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(what, got, want):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        d = np.abs(got.astype(f64) - want.astype(f64))
        first = np.argwhere(bad)[:4].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ (first at {first}); largest difference "
                             f"{np.nanmax(d):.3g}")


def _rel(got, want):
    want = np.asarray(want, f64)
    return float(np.max(np.abs(np.asarray(got, f64) - want) / np.abs(want)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


class Tail:
    """A generic handle that only ever finalizes: the summaries, the warm start and the filter are written by the test."""

    def __init__(self, T, dc, N=64):
        _need_gpu()
        from mppi_playground_amd import _capi

        self.T, self.dc, self.row = T, dc, T * dc
        f4 = C.c_float * 4
        cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=T, dim_state=2, dim_control=dc, num_samples=N, sample_offset=0,
                               inherit_count=N, u_min=f4(*[-1.0] * 4), u_max=f4(*[1.0] * 4), sigmas=f4(*[0.5] * 4), seed=11,
                               device=0)
        self.h = _capi.Handle(cfg)
        if dc > _capi.MAX_DIM_CONTROL:
            fn = lambda v: (C.c_float * dc)(*[v] * dc)  # noqa: E731
            self.h.call("mppi_set_control_limits", fn(-1.0), fn(1.0), fn(0.5), dc)
        self.action = torch.empty(self.row, device="cuda")
        self.stats = torch.empty(4, device="cuda")
        self._mean = torch.empty(self.row, device="cuda")

    def finalize(self, summaries, lam, store):
        """-> (action [row], {min c, sum e, sum e^2, sum e*c}) of one mppi_finalize over the given summaries"""
        s = _dev(summaries)
        assert s.shape[1] == tc.SUMMARY_HEAD + self.row
        self.action.fill_(float("nan"))
        self.stats.fill_(float("nan"))
        self.h.call("mppi_finalize", s.data_ptr(), int(s.shape[0]), float(lam), int(store), self.action.data_ptr(), None,
                    self.stats.data_ptr(), None)
        torch.cuda.synchronize()
        return self.action.cpu().numpy(), self.stats.cpu().numpy()

    def set_mean(self, m):
        self._m = _dev(np.asarray(m, f32).reshape(-1))
        self.h.call("mppi_set_mean", self._m.data_ptr(), 1, None)
        torch.cuda.synchronize()

    def mean(self):
        self._mean.fill_(float("nan"))
        self.h.call("mppi_get_mean", self._mean.data_ptr(), 1, None)
        torch.cuda.synchronize()
        return self._mean.cpu().numpy()

    def set_filter(self, taps, history=None):
        taps = np.ascontiguousarray(taps, f32)
        hist = None if history is None else np.ascontiguousarray(history, f32)
        self.h.call("mppi_set_sg_filter", taps.ctypes.data_as(C.c_void_p), int(len(taps)),
                    None if hist is None or hist.size == 0 else hist.ctypes.data_as(C.c_void_p))

    def refuses_filter(self, window):
        taps = np.full(max(window, 1), 0.25, f32)
        return self.h.lib.mppi_set_sg_filter(self.h.h, taps.ctypes.data_as(C.c_void_p), int(window), None)

    def history(self):
        out = np.full((self.T - 1, self.dc), np.nan, f32)
        if out.size:  # (T = 1: no row to read back)
            self.h.call("mppi_get_sg_history", out.ctypes.data_as(C.c_void_p))
        return out

    def close(self):
        self.h.close()


# ------------------------------------------------------------------------------ 1. the shard combine
def _combine_error(got, ref):
    a, st = got
    return max(_rel(st[1], ref[1]), _rel(st[2], ref[2]), _rel(st[3], ref[3]), _rel(a, ref[4]))


@pytest.mark.parametrize("name", [c.name for c in tc.SHARD_CASES])
def test_shard_combine(name):
    c = tc.shard_case(name)
    lam = float(f32(c.lam))
    ref = tc.combine_reference(c.summaries, lam)
    t = Tail(c.T, c.dc)
    first = t.finalize(c.summaries, lam, 0)   # the handle's first call of any kind
    a, st = first
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(st)), name
    err = _combine_error(first, ref)
    notes = []
    same_bits(f"{name}: min c", st[0], ref[0])
    if c.exact:
        want = tc.combine_exact(c.summaries)
        same_bits(f"{name}: head sums of an exact case", st, f32(want[:4]))
        same_bits(f"{name}: action of an exact case", a, want[4])
        notes.append("exact: bit-identical")
    if c.dead:
        alone = t.finalize(tc.without_dead(c), lam, 0)
        same_bits(f"{name}: action with and without the dead shards", a, alone[0])
        same_bits(f"{name}: head sums with and without the dead shards", st, alone[1])
        notes.append(f"{len(c.dead)} dead of {c.W}: bit-identical without")
    live = tc.without_dead(c)
    for perm in tc.permutations(len(live)):
        err = max(err, _combine_error(t.finalize(live[perm], lam, 0), ref))
    # the same temperature read from device memory (mppi_mpo_reset leaves lambda0 there without a solve): the same bits
    t.h.call("mppi_mpo_reset", lam, 0.1, 0.2)
    from mppi_playground_amd import _capi

    again = t.finalize(c.summaries, _capi.LAMBDA_DEVICE, 0)
    same_bits(f"{name}: action at MPPI_LAMBDA_DEVICE", again[0], a)
    same_bits(f"{name}: head sums at MPPI_LAMBDA_DEVICE", again[1], st)
    nxt, used = C.c_double(), C.c_double()
    t.h.call("mppi_get_lambda", C.byref(nxt), C.byref(used), None)
    assert used.value == lam and nxt.value == lam, (name, used.value, nxt.value, lam)
    worst["combine"] = max(worst.get("combine", 0.0), err)
    print(f"[tail] combine {name}: W {c.W}, row {c.T * c.dc}, max rel err {err:.3e} (limit {TOL:.0e}), "
          f"{len(tc.permutations(len(live)))} orders; {'; '.join(notes + ['device lambda: bit-identical'])}; "
          f"table max so far {worst['combine']:.3e}")
    assert err <= TOL, f"{name}: off by {err:.3e} > {TOL:.0e}"
    t.close()


# ------------------------------------------------------------------------------ 2. the filter
def _filter_solves(tag, t, taps, hist, T, dc, window):
    from pi_mpc import _host

    for k in range(tc.FILTER_SOLVES):
        A = tc.filter_row(T, dc, window, k)
        mean0 = t.mean()
        # store_mean = 0: this call must not filter, and leaves warm start and history as they were
        a, st = t.finalize(tc.one_shard(A), 1.0, 0)
        same_bits(f"{tag} solve {k}: unfiltered action (store_mean = 0)", a, A.reshape(-1))
        same_bits(f"{tag} solve {k}: head sums", st, f32([0.0, 1.0, 1.0, 0.0]))
        same_bits(f"{tag} solve {k}: warm start after store_mean = 0", t.mean(), mean0)
        same_bits(f"{tag} solve {k}: history after store_mean = 0", t.history(), hist)
        # store_mean = 1: the host statement of step 7, bit for bit
        a1, _ = t.finalize(tc.one_shard(A), 1.0, 1)
        want = _host.sg_filter_sequence(hist, a.reshape(T, dc), taps)
        same_bits(f"{tag} solve {k}: filtered action against the host statement", a1.reshape(T, dc), want)
        same_bits(f"{tag} solve {k}: stored warm start", t.mean(), a1)
        hist = np.concatenate([hist[1:], a1.reshape(T, dc)[:1]], axis=0) if T > 1 else hist
        same_bits(f"{tag} solve {k}: history after the shift", t.history(), hist)
    return hist


@pytest.mark.parametrize("T,dc,window", tc.FILTER_SHAPES, ids=[f"T{T}-dc{dc}-w{w}" for T, dc, w in tc.FILTER_SHAPES])
def test_filter_shapes(T, dc, window):
    for kind in tc.TAP_KINDS:
        taps = tc.taps(kind, T, dc, window)
        for hk in tc.HISTORY_KINDS:
            tag = f"T{T} dc{dc} w{window} {kind} taps, {hk} history"
            t = Tail(T, dc)
            t.set_mean(tc.filter_row(T, dc, window, 99))  # (a warm start that is not zero: store_mean = 0 must keep it)
            hist = tc.history(hk, T, dc)
            t.set_filter(taps, None if hk == "zero" else hist)
            same_bits(f"{tag}: history as handed in", t.history(), hist)
            hist = _filter_solves(tag, t, taps, hist, T, dc, window)
            # window = 0 after a filter: the unfiltered bits again, stored as they are
            t.h.call("mppi_set_sg_filter", None, 0, None)
            A = tc.filter_row(T, dc, window, 7)
            a, _ = t.finalize(tc.one_shard(A), 1.0, 1)
            same_bits(f"{tag}: action after window = 0", a, A.reshape(-1))
            same_bits(f"{tag}: warm start after window = 0", t.mean(), A.reshape(-1))
            same_bits(f"{tag}: history after window = 0", t.history(), hist)
            print(f"[tail] filter {tag}: {tc.FILTER_SOLVES} solves x (store_mean 0 / 1) + window 0: bit-identical")
            t.close()


@pytest.mark.parametrize("T,dc,window", tc.REFUSALS, ids=[f"T{T}-dc{dc}-w{w}" for T, dc, w in tc.REFUSALS])
def test_filter_refusals_leave_the_handle_usable(T, dc, window):
    t = Tail(T, dc)
    assert t.refuses_filter(window) == E_INVALID
    assert t.h.lib.mppi_last_error(t.h.h)
    A = tc.filter_row(T, dc, window, 0)
    a, st = t.finalize(tc.one_shard(A), 1.0, 1)   # no filter was set: the action is A, stored as it is
    same_bits(f"T{T} dc{dc} w{window}: action after the refusal", a, A.reshape(-1))
    same_bits(f"T{T} dc{dc} w{window}: warm start after the refusal", t.mean(), A.reshape(-1))
    narrow = 3 if tc.sg_admitted(T, dc, 3) else 0
    if narrow:  # an admitted window is still taken, and a second refusal keeps it
        taps = tc.taps("asymmetric", T, dc, narrow)
        t.set_filter(taps)
        assert t.refuses_filter(window) == E_INVALID
        from pi_mpc import _host

        a1, _ = t.finalize(tc.one_shard(A), 1.0, 1)
        same_bits(f"T{T} dc{dc} w{window}: the admitted filter after a refusal", a1.reshape(T, dc),
                  _host.sg_filter_sequence(np.zeros((T - 1, dc), f32), A, taps))
    print(f"[tail] refusal T{T} dc{dc} w{window}: refused, the handle's next calls bit-identical")
    t.close()


# ------------------------------------------------------------------------------ 3. the batch-1 rollout
def _rig(model, T, table):
    """(rig, base start, oracle model): a native handle driven through the C ABI, N = 256"""
    if model == "racing_discs":
        from test_gpu_racing_discs import DiscRig, case

        tab, x0, ref = case(table, T)
        return DiscRig(tab, x0, ref, T, tc.B1_SAMPLES), f32(x0), "racing"
    from test_gpu_action_cost import Rig

    x0 = tc.b1_base_start(model)
    return Rig(model, T, tc.B1_SAMPLES, x0=x0), x0, model


class B1:
    """finalize on the one shard {0, 1, 1, 0, A} of a native handle, and the two other owners of the same rollout"""

    def __init__(self, rig):
        self.rig, self.h, self.T, self.ds, self.dc = rig, rig.h, rig.T, rig.ds, rig.dc
        self.st = rig.solver._stream()
        self.action = torch.empty(self.T * self.dc, device="cuda")
        self.stats = torch.empty(4, device="cuda")

    def start(self, x0):
        self.x0 = _dev(x0)
        self.h.call("mppi_set_state", self.x0.data_ptr(), 1, self.st)

    def finalize(self, A, sync=True):
        """-> (action [T, dc], the state buffer [T + 1, ds] as a device tensor)"""
        self.summ = _dev(tc.one_shard(A))
        self.action.fill_(float("nan"))
        state = torch.zeros(self.T + 1, self.ds, device="cuda")
        self.h.call("mppi_finalize", self.summ.data_ptr(), 1, 1.0, 0, self.action.data_ptr(), state.data_ptr(),
                    self.stats.data_ptr(), self.st)
        torch.cuda.synchronize()
        return self.action.cpu().numpy().reshape(self.T, self.dc), state

    def rollout_actions(self, A):
        a = _dev(A)
        out = torch.full((1, self.T + 1, self.ds), float("nan"), device="cuda")
        self.h.call("mppi_rollout_actions", a.data_ptr(), 1, None, out.data_ptr(), self.st)
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]


def _check_batch1(model, T, table=None):
    import reroll_cases as rr
    from helpers import oracle_problem

    rig, base, omodel = _rig(model, T, table)
    b = B1(rig)
    P = oracle_problem(omodel, 1, T)
    tag0 = f"{model} T{T}" + (f" {table}" if table else "")
    for x0 in tc.b1_starts(model, base):
        b.start(x0)
        for kind in tc.B1_ACTION_KINDS:
            A = tc.b1_actions(model, T, kind)
            tag = f"{tag0} {kind} x0 {x0.tolist()}"
            S_default = None
            for math in tc.B1_MATHS:
                b.h.call("mppi_set_option", b"math", math)
                a, state = b.finalize(A)
                S = state.cpu().numpy()
                same_bits(f"{tag} math {math}: action_out against the injected row", a, A)
                assert np.all(np.isfinite(S)), (tag, math)
                same_bits(f"{tag} math {math}: state_out against mppi_rollout_actions", S, b.rollout_actions(A))
                same_bits(f"{tag} math {math}: row 0 against the caller's x0", S[0], x0)
                if math == tc.B1_DEFAULT_MATH:
                    S_default = S
            err = rr.state_error(omodel, S_default, P.rollout_single(x0, A))
            worst[model] = max(worst.get(model, 0.0), err)
            # the two lazy completions of the same rollout (default math level)
            b.h.call("mppi_set_option", b"lazy_state_seq", 1)
            a, state = b.finalize(A)
            same_bits(f"{tag} lazy: action_out", a, A)
            assert bool(torch.isnan(state).all()), f"{tag}: the pending state buffer is not all-NaN"
            b.h.call("mppi_join_state_seq", 0, b.st)
            torch.cuda.synchronize()
            same_bits(f"{tag}: mppi_join_state_seq against the in-kernel rollout", state.cpu().numpy(), S_default)
            a, state = b.finalize(A)
            assert bool(torch.isnan(state).all()), f"{tag}: the pending state buffer is not all-NaN"
            b.h.call("mppi_sample", 3, b.st)
            b.h.call("mppi_rollout_cost", b.st)
            torch.cuda.synchronize()
            same_bits(f"{tag}: the next rollout launch's rider against the in-kernel rollout", state.cpu().numpy(), S_default)
            b.h.call("mppi_set_option", b"lazy_state_seq", 0)
            wave = "rollout_wave" if tc.takes_wave_rollout(model, T, tc.B1_DEFAULT_MATH) else "lane-serial"
            print(f"[tail] batch1 {tag}: math 0 / 1 / 2 against mppi_rollout_actions, join and rider: bit-identical ({wave}); "
                  f"oracle {err:.2e} of max|S| (limit {TOL:.0e}); {model} so far {worst[model]:.2e}")
            assert err < TOL, (tag, err)
    rig.close()


_B1 = [(m, T, None) for m, T in tc.B1_CASES if m != "racing_discs"] + \
      [(m, T, tab) for m, T in tc.B1_CASES if m == "racing_discs" for tab in tc.B1_DISC_TABLES]


@pytest.mark.parametrize("model,T,table", _B1, ids=[f"{m}-T{T}" + (f"-{tab}" if tab else "") for m, T, tab in _B1])
def test_batch1_rollout(model, T, table):
    _check_batch1(model, T, table)
