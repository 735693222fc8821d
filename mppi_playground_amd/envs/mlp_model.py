"""Learned dynamics as an MPPI plugin: a small multi-layer perceptron fitted to data, with a quadratic tracking cost.

    model = MLPModel.from_module(net, goal=[...], q=[...], r=[...])      # net: nn.Sequential of Linear / ReLU / Tanh
    solver = MPPI(dim_state=4, dim_control=dc, dynamics=model.dynamics, cost_func=model.cost, ...)

`dynamics` and `cost` are plain torch code — they run anywhere, the solver's generic path included — and carry the native
tag "mlp41" / "mlp42" (by the control width), so that pi_mpc.mppi.MPPI runs them fused on the device: the weights are data
(one table, include/mppi_hip.h: mppi_set_mlp), the functor that evaluates them is one more native model.

What the device path takes: a state of 4 components, 1 or 2 controls, one or two hidden layers of at most 32 units, relu or
tanh.  Narrower layers and a narrower state are zero-padded here (rows, columns and biases: relu(0) = tanh(0) = 0 and adding
w * 0 changes no bit of a sum); the CALLER pads the state vector it hands to the solver with components that stay zero
(pad_state does it; dim_state is the width the solver must be given).

MLPModel8 is the same model with a state of 8 components and 1, 2 or 4 controls (tags "mlp81" / "mlp82" / "mlp84"): a cart
with two poles, a planar quadrotor, anything with four actuators.  Read 8 for 4 below.

The arithmetic, in fp32 and in this order (the torch code below, the device functor and tests/mlp_ref.py state the same):
    x = [s[0..3], u[0..dc-1]]          (u: the solver-clamped action, not clamped again)
    z[j] = b1[j]; for i ascending: z[j] = z[j] + W1[j][i] * x[i];  h1[j] = act(z[j])
    (second hidden layer: the same over h1)
    o[m] = b3[m]; for j ascending: o[m] = o[m] + W3[m][j] * h[j]
    next[m] = s[m] + o[m] if residual else o[m]
    cost = sum_m q[m] * (s[m] - goal[m])^2 + sum_k r[k] * u[k]^2      (terminal: the same with u = 0)

Tracking (include/mppi_hip.h: mppi_set_mlp_reference has the contract): `set_reference(goals, q)` gives every horizon step a
goal (and weights) of its own — the stage cost of step t reads row t = info["t"], the terminal cost row T-1 (the reference
solver's stale info["t"]: there is no row T; to weight the end of the horizon put the weight into q of row T-1, it counts for
the state of step T-1 and for the final state) — and `angular=[...]` names the state components that are angles: their error
is wrapped into [-pi, pi],
    d = s[m] - g_t[m];  k = rint(d * INV_TWO_PI);  d = d - TWO_PI * k        (TWO_PI = float32 6.2831855, INV_TWO_PI = 0.15915494)
so a heading needs no (cos, sin) encoding.  The reference is ONE padded float32 table [rows, 2 * DS] (row: g_t then q_t),
updated in place while its shape stays the same, so a captured graph of the callables (graph_callables=True) stays valid.

A learned terminal value (include/mppi_hip.h: mppi_set_mlp_value has the contract): `set_value(weights, biases)` gives the model
a second, smaller network V over the state — one or two hidden layers of at most 32 units, relu or tanh of its own, ONE output —
evaluated once per trajectory on its final state, and `terminal_cost` is the tagged callable to hand to
MPPI(..., terminal_cost=model.terminal_cost):
    z1[j] = b1[j]; for i ascending: z1[j] = z1[j] + W1[j][i] * s[i];  h = act(z1)        (second hidden layer: the same over h)
    V = b3; for j ascending: V = V + w3[j] * h[j]
    terminal = quad_T + (weight * V)        or, with replace_terminal, weight * V alone (the callable then returns
                                            weight * V - quad_T: the solver adds it behind the terminal call's quad_T)
The value's input is the final state as the dynamics network produced it: the `angular` mask does NOT wrap it (a limit: a critic
over an angle should be fitted on the unwrapped range the rollouts reach, or on a model whose dynamics keep the angle wrapped).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from pi_mpc.native import native_model

HIDDEN = 32  # hidden width of the device table (MPPI_MLP_HIDDEN)
TWO_PI = float(np.float32(6.2831855))       # the wrap of an angular error, as the device spells it (float32 values)
INV_TWO_PI = float(np.float32(0.15915494))


def _f32(a) -> np.ndarray:
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=np.float32)


def _provider(owner):
    return owner.native_inputs()


def _finite_weight(weight) -> float:
    w = float(weight)
    if not np.isfinite(w) or abs(w) > float(np.finfo(np.float32).max):
        raise ValueError("the value's weight must be finite (in float32)")
    return w


def _copy_value(v):
    if v is None:
        return None
    return dict(v, layers=tuple(a.copy() for a in v["layers"]), table=v["table"].copy())


class MLPModel:
    DS = 4              # state components of the native models this class tags
    CONTROLS = (1, 2)   # control widths they are compiled for

    def __init__(self, weights: Sequence, biases: Sequence, activation: str = "tanh", residual: bool = True, goal=None,
                 q=None, r=None, angular=None):
        """weights / biases: per layer, torch.nn.Linear's layout — W1 [h1, ds + dc], (W2 [h2, h1],) W3 [ds, h] with
        ds <= 4 state components, dc = 1 or 2 controls and h1, h2 <= 32.  goal, q: [ds] (defaults 0 / 1), r: [dc] (default 0).
        angular: indices (< ds) of the state components that are angles.  ValueError for anything the device path does not take."""
        if activation not in ("relu", "tanh"):
            raise ValueError("activation must be 'relu' or 'tanh'")
        self.activation = activation
        self.residual = bool(residual)
        self.version = 0
        self._set(weights, biases)
        ds, dc = self.dim_state_model, self.dim_control

        def vec(v, n, default, name):
            a = np.full(n, default, np.float32) if v is None else _f32(v).reshape(-1)
            if a.shape != (n,) or not np.all(np.isfinite(a)):
                raise ValueError(f"{name} must hold {n} finite values")
            return a

        goal4, q4 = np.zeros(self.DS, np.float32), np.zeros(self.DS, np.float32)
        goal4[:ds] = vec(goal, ds, 0.0, "goal")
        q4[:ds] = vec(q, ds, 1.0, "q")
        # (read-only: the torch callables and the device both take them from here; set_cost() replaces them for both)
        self.goal, self.q, self.r = goal4, q4, vec(r, dc, 0.0, "r")
        for a in (self.goal, self.q, self.r):
            a.flags.writeable = False
        self.set_angular(angular)
        self._ref = None            # the reference table [rows, 2 * DS] (float32, wherever set_reference was given it), or None
        self._ref_own_q = False     # its q half was given (False: it mirrors self.q)
        self._ref_mirrors = {}      # (device, dtype) -> the copy the callables read there, kept in step IN PLACE
        self.reference_version = 0
        self._value = None          # the terminal value (set_value): a dict of its padded layers, table, flags and weight, or None
        self.value_version = 0

    def set_angular(self, angular) -> None:
        """Which state components are angles: indices below the network's own state width, or None / () for none.  For the
        callables and the device alike, from the next solve on.  ValueError for an index out of range, a repeated index or a
        non-integer."""
        ds = self.dim_state_model
        idx = [] if angular is None else list(angular)
        if any(isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) for i in idx):
            raise ValueError("angular: integer indices of state components")
        if any(not 0 <= int(i) < ds for i in idx) or len({int(i) for i in idx}) != len(idx):
            raise ValueError(f"angular: distinct indices in 0..{ds - 1} (the network's own state width)")
        self.angular = tuple(sorted(int(i) for i in idx))  # (read it; change it through set_angular)

    @property
    def angular_mask(self) -> int:
        """Bit m is set when state component m is an angle (mppi_set_mlp_angular)."""
        return sum(1 << m for m in self.angular)

    @property
    def reference(self):
        """The reference table, float32 [rows, 2 * DS] (row t: the goal of step t, then its weights), or None.  It may be
        rewritten in place (a device tensor: on the device); call reference_changed() afterwards."""
        return self._ref

    def set_reference(self, goals, q=None) -> None:
        """A goal per horizon step: goals [rows, ds] (a host array, a host tensor or a device tensor; the solver needs
        rows >= horizon), q [rows, ds] or None — with None every row carries the model's own q as it stands at the solve (a
        later set_cost(q=...) shows in those rows).  set_reference(None) switches the reference off.  While the shape and the
        device stay the same the table is updated IN PLACE (a captured graph of the callables stays valid).  ValueError for a
        wrong width, non-finite values or a q of another shape."""
        if goals is None:
            self._ref, self._ref_own_q, self._ref_mirrors = None, False, {}
            self.reference_version += 1
            return
        ds, DS = self.dim_state_model, self.DS

        def tensor(v, name):
            t = v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32))
            t = t.to(torch.float32)
            if t.ndim != 2 or t.shape[1] != ds or t.shape[0] < 1:
                raise ValueError(f"{name} must be [rows, {ds}] (got {list(t.shape)})")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{name} must be finite")
            return t

        g = tensor(goals, "goals")
        qq = None if q is None else tensor(q, "q").to(g.device)
        if qq is not None and qq.shape != g.shape:
            raise ValueError(f"q must have the shape of goals {list(g.shape)} (got {list(qq.shape)})")
        tab = torch.zeros(g.shape[0], 2 * DS, dtype=torch.float32, device=g.device)
        tab[:, :ds] = g
        tab[:, DS:DS + ds] = qq if qq is not None else torch.as_tensor(np.array(self.q[:ds]), device=g.device)
        self._ref_own_q = qq is not None
        if self._ref is not None and self._ref.shape == tab.shape and self._ref.device == tab.device:
            self._ref.copy_(tab)
        else:
            self._ref, self._ref_mirrors = tab, {}
        self.reference_changed()

    def reference_changed(self) -> None:
        """Tell the callables and the solver that the reference table was rewritten in place."""
        if self._ref is not None:
            for t in self._ref_mirrors.values():
                if t is not self._ref:
                    t.copy_(self._ref)
        self.reference_version += 1

    def set_cost(self, goal=None, q=None, r=None) -> None:
        """Replace cost parameters (same shapes as the constructor's; None keeps one) for the callables and the device alike."""
        ds, dc = self.dim_state_model, self.dim_control
        for name, v, n in (("goal", goal, ds), ("q", q, ds), ("r", r, dc)):
            if v is None:
                continue
            a = _f32(v).reshape(-1)
            if a.shape != (n,) or not np.all(np.isfinite(a)):
                raise ValueError(f"{name} must hold {n} finite values")
            full = np.zeros(len(getattr(self, name)), np.float32)
            full[:n] = a
            full.flags.writeable = False
            setattr(self, name, full)
        self._torch = {}
        if q is not None and self._ref is not None and not self._ref_own_q:  # rows without weights of their own follow q
            self._ref[:, self.DS:self.DS + ds] = torch.as_tensor(np.array(self.q[:ds]), device=self._ref.device)
            self.reference_changed()

    # ------------------------------------------------------------------ the learned terminal value
    def set_value(self, weights, biases=None, activation: str = "tanh", weight: float = 1.0, replace_terminal: bool = False) -> None:
        """A value network over the state: weights / biases per layer in torch.nn.Linear's layout — W1 [h1, ds], (W2 [h2, h1],)
        W3 [1, h] with ds the network's own state width and h1, h2 <= 32; its activation and depth are its own.
        terminal = quad_T + weight * V, or weight * V alone with replace_terminal.  set_value(None) switches it off.
        ValueError for anything the device path does not take."""
        if weights is None:
            self._value = None
            self.value_version += 1
            return
        if activation not in ("relu", "tanh"):
            raise ValueError("activation must be 'relu' or 'tanh'")
        w = _finite_weight(weight)
        layers, hidden = self._value_layers(weights, biases)
        self._value = {"layers": layers, "table": np.concatenate([a.reshape(-1) for a in layers]).astype(np.float32),
                       "hidden_layers": hidden, "activation": activation, "weight": w, "replace_terminal": bool(replace_terminal)}
        self._value_torch = {}
        self.value_version += 1

    def _value_layers(self, weights, biases):
        Ws, bs = [_f32(a) for a in weights], [_f32(b).reshape(-1) for b in (biases or ())]
        if len(Ws) != len(bs) or len(Ws) not in (2, 3):
            raise ValueError("a value network with one or two hidden layers: 2 or 3 weight matrices and as many biases "
                             f"(got {len(Ws)} and {len(bs)})")
        if any(a.ndim != 2 for a in Ws) or any(a.shape[0] != b.shape[0] for a, b in zip(Ws, bs)):
            raise ValueError("every weight is a matrix [out, in] with a bias [out]")
        if any(a.shape[1] != p.shape[0] for p, a in zip(Ws[:-1], Ws[1:])):
            raise ValueError("the layers do not chain: each weight's input width is the previous layer's output width")
        ds, DS = self.dim_state_model, self.DS
        if Ws[0].shape[1] != ds:
            raise ValueError(f"the value network reads the state: input width {ds} (got {Ws[0].shape[1]})")
        if Ws[-1].shape[0] != 1:
            raise ValueError(f"the value network has ONE output (got {Ws[-1].shape[0]})")
        if any(a.shape[0] > HIDDEN for a in Ws[:-1]):
            raise ValueError(f"hidden layers of at most {HIDDEN} units run on the device")
        if not all(np.all(np.isfinite(a)) for a in Ws + bs):
            raise ValueError("weights and biases must be finite")
        # the padded layers of the table: W1[32][DS], b1[32], W2[32][32], b2[32], w3[32], b3[1]
        W1, b1 = np.zeros((HIDDEN, DS), np.float32), np.zeros(HIDDEN, np.float32)
        W1[:Ws[0].shape[0], :ds] = Ws[0]
        b1[:bs[0].shape[0]] = bs[0]
        W2, b2 = np.zeros((HIDDEN, HIDDEN), np.float32), np.zeros(HIDDEN, np.float32)
        if len(Ws) == 3:
            W2[:Ws[1].shape[0], :Ws[1].shape[1]] = Ws[1]
            b2[:bs[1].shape[0]] = bs[1]
        w3, b3 = np.zeros(HIDDEN, np.float32), np.zeros(1, np.float32)
        w3[:Ws[-1].shape[1]] = Ws[-1][0]
        b3[:] = bs[-1]
        return (W1, b1, W2, b2, w3, b3), len(Ws) - 1

    def set_value_module(self, module: torch.nn.Module, **kw) -> None:
        """set_value from nn.Sequential(Linear, act, [Linear, act,] Linear(., 1)) with act = nn.ReLU or nn.Tanh (one kind);
        keywords: weight, replace_terminal."""
        mods = list(module.children())
        lin = [m for m in mods if isinstance(m, torch.nn.Linear)]
        acts = [m for m in mods if not isinstance(m, torch.nn.Linear)]
        kinds = {torch.nn.ReLU: "relu", torch.nn.Tanh: "tanh"}
        shape_ok = (len(mods) == 2 * len(lin) - 1 and all(isinstance(m, torch.nn.Linear) for m in mods[0::2])
                    and all(type(m) in kinds for m in acts))
        if not shape_ok or len(lin) not in (2, 3) or len({type(m) for m in acts}) != 1 or any(m.bias is None for m in lin):
            raise ValueError("set_value_module takes nn.Sequential(Linear, act, [Linear, act,] Linear(., 1)) with biases and "
                             "act = nn.ReLU or nn.Tanh throughout")
        self.set_value([m.weight for m in lin], [m.bias for m in lin], activation=kinds[type(acts[0])], **kw)

    def update_value(self, weights, biases) -> None:
        """New weights of the same depth for the value (a critic learned online); activation, weight and replace_terminal stay.
        The solver uploads the table before its next solve, in stream order."""
        if self._value is None:
            raise ValueError("update_value: no value network is set (set_value)")
        layers, hidden = self._value_layers(weights, biases)
        if hidden != self._value["hidden_layers"]:
            raise ValueError("update_value keeps the value network's number of layers")
        self._value = dict(self._value, layers=layers, table=np.concatenate([a.reshape(-1) for a in layers]).astype(np.float32))
        self._value_torch = {}
        self.value_version += 1

    def set_value_weight(self, weight: float) -> None:
        """The weight of the value alone."""
        if self._value is None:
            raise ValueError("set_value_weight: no value network is set (set_value)")
        w = _finite_weight(weight)
        self._value = dict(self._value, weight=w)
        self.value_version += 1

    @property
    def value(self):
        """What set_value left: {"table", "hidden_layers", "activation", "weight", "replace_terminal", "layers"}, or None."""
        return self._value

    def _value_on(self, ref: torch.Tensor):
        key = (ref.device, ref.dtype)
        cache = self.__dict__.setdefault("_value_torch", {})
        got = cache.get(key)
        if got is None:
            got = tuple(torch.tensor(np.array(a)).to(ref.device, ref.dtype) for a in self._value["layers"])
            cache[key] = got
        return got

    def value_of(self, state: torch.Tensor) -> torch.Tensor:
        """V(state) [N] in the device's operation order (plain torch; no weight)."""
        if self._value is None:
            raise ValueError("no value network is set (set_value)")
        W1, b1, W2, b2, w3, b3 = self._value_on(state)
        act = (torch.tanh if self._value["activation"] == "tanh" else (lambda z: torch.clamp_min(z, 0.0)))
        n = state.shape[0]
        z = b1.expand(n, HIDDEN)
        for i in range(self.DS):
            z = z + W1[:, i] * state[:, i:i + 1]
        h = act(z)
        if self._value["hidden_layers"] == 2:
            z = b2.expand(n, HIDDEN)
            for i in range(HIDDEN):
                z = z + W2[:, i] * h[:, i:i + 1]
            h = act(z)
        v = b3.expand(n)
        for j in range(HIDDEN):
            v = v + w3[j] * h[:, j]
        return v

    @native_model(lambda owner: owner.model_name, "terminal", _provider)
    def terminal_cost(self, state: torch.Tensor, info=None) -> torch.Tensor:
        """What MPPI(..., terminal_cost=...) adds behind the terminal call of `cost`: weight * V(S_T) — with replace_terminal,
        minus that call's quadratic, so that the sum is weight * V alone up to one rounding.  `info` (the solver's generic
        path hands a tagged terminal callable the dict of its terminal call: t = T - 1) picks the row of a reference; without
        it the table's last row."""
        if self._value is None:
            raise ValueError("terminal_cost: no value network is set (set_value)")
        wv = self._value["weight"] * self.value_of(state)
        if self._value["replace_terminal"]:
            tab = self._ref_on(state)
            if info is None and tab is not None:
                info = {"t": tab.shape[0] - 1}
            zero = torch.zeros(state.shape[0], self.dim_control, device=state.device, dtype=state.dtype)
            return wv - self.cost(state, zero, info)
        return wv

    # ------------------------------------------------------------------ weights
    def _set(self, weights, biases) -> None:
        Ws, bs = [_f32(w) for w in weights], [_f32(b).reshape(-1) for b in biases]
        if len(Ws) != len(bs) or len(Ws) not in (2, 3):
            raise ValueError("an MLP with one or two hidden layers: 2 or 3 weight matrices and as many biases "
                             f"(got {len(Ws)} and {len(bs)})")
        if any(w.ndim != 2 for w in Ws) or any(w.shape[0] != b.shape[0] for w, b in zip(Ws, bs)):
            raise ValueError("every weight is a matrix [out, in] with a bias [out]")
        if any(w.shape[1] != p.shape[0] for p, w in zip(Ws[:-1], Ws[1:])):
            raise ValueError("the layers do not chain: each weight's input width is the previous layer's output width")
        DS = self.DS
        ds = Ws[-1].shape[0]
        dc = Ws[0].shape[1] - ds
        if not 1 <= ds <= DS:
            raise ValueError(f"the network's output (the state) has {ds} components: 1..{DS} run on the device")
        if dc not in self.CONTROLS:
            raise ValueError(f"control width {dc} (input width {Ws[0].shape[1]} - state {ds}): "
                             f"{', '.join(map(str, self.CONTROLS[:-1]))} or {self.CONTROLS[-1]} run on the device")
        if any(w.shape[0] > HIDDEN for w in Ws[:-1]):
            raise ValueError(f"hidden layers of at most {HIDDEN} units run on the device")
        if not all(np.all(np.isfinite(a)) for a in Ws + bs):
            raise ValueError("weights and biases must be finite")
        if getattr(self, "dim_control", dc) != dc or getattr(self, "dim_state_model", ds) != ds or \
                getattr(self, "hidden_layers", len(Ws) - 1) != len(Ws) - 1:
            raise ValueError("update_weights keeps the model's state width, control width and number of layers")
        self.dim_state_model, self.dim_control, self.hidden_layers = ds, dc, len(Ws) - 1
        IN = DS + dc
        # the padded layers of the table: W1[32][IN], b1[32], W2[32][32], b2[32], W3[DS][32], b3[DS]
        W1 = np.zeros((HIDDEN, IN), np.float32)
        W1[:Ws[0].shape[0], :ds] = Ws[0][:, :ds]
        W1[:Ws[0].shape[0], DS:] = Ws[0][:, ds:]
        b1 = np.zeros(HIDDEN, np.float32)
        b1[:bs[0].shape[0]] = bs[0]
        W2, b2 = np.zeros((HIDDEN, HIDDEN), np.float32), np.zeros(HIDDEN, np.float32)
        if len(Ws) == 3:
            W2[:Ws[1].shape[0], :Ws[1].shape[1]] = Ws[1]
            b2[:bs[1].shape[0]] = bs[1]
        W3, b3 = np.zeros((DS, HIDDEN), np.float32), np.zeros(DS, np.float32)
        W3[:ds, :Ws[-1].shape[1]] = Ws[-1]
        b3[:ds] = bs[-1]
        self.layers = (W1, b1, W2, b2, W3, b3)
        self.table = np.concatenate([a.reshape(-1) for a in self.layers]).astype(np.float32)
        self._torch = {}  # device -> the layers the callables evaluate, as tensors

    def update_weights(self, weights: Sequence, biases: Sequence) -> None:
        """New weights of the same shapes (a model learned online); the solver uploads them before its next solve."""
        self._set(weights, biases)
        self.version += 1

    @classmethod
    def from_module(cls, module: torch.nn.Module, **kw) -> "MLPModel":
        """nn.Sequential(Linear, act, [Linear, act,] Linear) with act = nn.ReLU or nn.Tanh (one kind)."""
        mods = list(module.children()) if not isinstance(module, torch.nn.Linear) else [module]
        lin = [m for m in mods if isinstance(m, torch.nn.Linear)]
        acts = [m for m in mods if not isinstance(m, torch.nn.Linear)]
        kinds = {torch.nn.ReLU: "relu", torch.nn.Tanh: "tanh"}
        shape_ok = (len(mods) == 2 * len(lin) - 1 and all(isinstance(m, torch.nn.Linear) for m in mods[0::2])
                    and all(type(m) in kinds for m in acts))
        if not shape_ok or len(lin) not in (2, 3) or len({type(m) for m in acts}) != 1 or any(m.bias is None for m in lin):
            raise ValueError("from_module takes nn.Sequential(Linear, act, [Linear, act,] Linear) with biases and "
                             "act = nn.ReLU or nn.Tanh throughout")
        return cls([m.weight for m in lin], [m.bias for m in lin], activation=kinds[type(acts[0])], **kw)

    # ------------------------------------------------------------------ what the solver asks for
    @property
    def model_name(self) -> str:
        return f"mlp{self.DS}{self.dim_control}"

    @property
    def dim_state(self) -> int:
        """The state width of the native model: what MPPI(dim_state=...) must be given."""
        return self.DS

    def pad_state(self, x):
        """A state of the network's own width (or any width up to dim_state), zero-padded to dim_state along its last axis."""
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        n = t.shape[-1]
        if n > self.DS:
            raise ValueError(f"a state of {n} components does not fit the model's {self.DS}")
        return t if n == self.DS else torch.nn.functional.pad(t, (0, self.DS - n))

    def native_inputs(self) -> dict:
        return {"params": [float(v) for v in np.concatenate([self.goal, self.q, self.r])],
                "mlp": {"table": self.table, "hidden_layers": self.hidden_layers, "activation": self.activation,
                        "residual": self.residual, "version": self.version, "angular": self.angular_mask,
                        "reference": self._ref, "reference_version": self.reference_version,
                        "value": None if self._value is None else dict(self._value, version=self.value_version)}}

    # ------------------------------------------------------------------ the callables
    def _on(self, ref: torch.Tensor):
        key = (ref.device, ref.dtype)
        got = self._torch.get(key)
        if got is None:
            got = tuple(torch.tensor(np.array(a)).to(ref.device, ref.dtype) for a in self.layers + (self.goal, self.q, self.r))
            self._torch[key] = got
        return got

    def _ref_on(self, ref: torch.Tensor):
        """The reference table where and as `ref` lives (one tensor per place, kept in step in place), or None."""
        if self._ref is None:
            return None
        key = (ref.device, ref.dtype)
        got = self._ref_mirrors.get(key)
        if got is None:
            got = self._ref if (self._ref.device, self._ref.dtype) == key else self._ref.to(ref.device, ref.dtype)
            self._ref_mirrors[key] = got
        return got

    def _act(self, z: torch.Tensor) -> torch.Tensor:
        return torch.tanh(z) if self.activation == "tanh" else torch.clamp_min(z, 0.0)

    @native_model(lambda owner: owner.model_name, "dynamics")
    def dynamics(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        W1, b1, W2, b2, W3, b3 = self._on(state)[:6]
        x = torch.cat((state, action), dim=1)
        z = b1.expand(x.shape[0], HIDDEN)
        for i in range(x.shape[1]):
            z = z + W1[:, i] * x[:, i:i + 1]
        h = self._act(z)
        if self.hidden_layers == 2:
            z = b2.expand(x.shape[0], HIDDEN)
            for i in range(HIDDEN):
                z = z + W2[:, i] * h[:, i:i + 1]
            h = self._act(z)
        o = b3.expand(x.shape[0], self.DS)
        for j in range(HIDDEN):
            o = o + W3[:, j] * h[:, j:j + 1]
        return state + o if self.residual else o

    @native_model(lambda owner: owner.model_name, "cost", _provider)
    def cost(self, state: torch.Tensor, action: torch.Tensor, info=None) -> torch.Tensor:
        goal, q, r = self._on(state)[6:]
        tab = self._ref_on(state)
        if tab is not None:  # the goal and the weights of this step: row info["t"] (the terminal call carries T - 1)
            row = tab[0 if info is None else info["t"]]
            goal, q = row[:self.DS], row[self.DS:]
        c = torch.zeros(state.shape[0], device=state.device, dtype=state.dtype)
        for m in range(self.DS):
            d = state[:, m] - goal[m]
            if m in self.angular:
                d = d - TWO_PI * torch.round(d * INV_TWO_PI)
            c = c + q[m] * (d * d)
        for k in range(self.dim_control):
            c = c + r[k] * (action[:, k] * action[:, k])
        return c

    def __deepcopy__(self, memo):
        new = object.__new__(type(self))
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k in ("_torch", "_ref_mirrors", "_value_torch") else (
                _copy_value(v) if k == "_value" else tuple(a.copy() for a in v) if k == "layers" else
                v.copy() if isinstance(v, np.ndarray) else v.clone() if torch.is_tensor(v) else v)
        for a in (new.goal, new.q, new.r):
            a.flags.writeable = False
        return new


class MLPModel8(MLPModel):
    """MLPModel with a state of up to 8 components and 1, 2 or 4 controls: native tags "mlp81" / "mlp82" / "mlp84"
    (MPPI(dim_state=8, ...)).  Same padding, same arithmetic, same interface; goal and q are kept with 8 entries."""
    DS = 8
    CONTROLS = (1, 2, 4)


MAX_MEMBERS = 16  # MPPI_MAX_PARTICLES: a member per particle


class MLPEnsemble:
    """A bootstrap ensemble of learned models: E networks of ONE architecture and one cost, as an MPPI plugin.

        ens = MLPEnsemble.from_modules([net0, net1, ...], goal=[...], q=[...], r=[...])
        solver = MPPI(dim_state=4, dim_control=dc, dynamics=ens.dynamics, cost_func=ens.cost, risk="cvar", risk_alpha=0.4, ...)
        solver.set_model_particles("all")        # every sample is scored under every member, the costs folded by `risk`

    `dynamics` / `cost` are the NOMINAL member's plain torch callables (the members' tag: they are all MLPModel or all
    MLPModel8): every solve without particles, the returned `state_seq` and every re-roll evaluate that one network.  The other members decide particle
    costs only (pi_mpc.mppi.MPPI: set_model_particles, set_state_particles(..., members=)); on the device they are one
    buffer of E tables (include/mppi_hip.h: mppi_set_mlp_ensemble), each padded exactly as MLPModel pads its own."""

    def __init__(self, members: Sequence[MLPModel], nominal: int = 0):
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS or not all(isinstance(m, MLPModel) for m in members):
            raise ValueError(f"an ensemble of 1..{MAX_MEMBERS} MLPModel members (got {len(members)})")
        first = members[0]
        if any(type(m) is not type(first) for m in members[1:]):
            raise ValueError("the members of an ensemble are of one class: all MLPModel or all MLPModel8")
        for m in members[1:]:
            for name in ("dim_state_model", "dim_control", "hidden_layers", "activation", "residual", "angular"):
                if getattr(m, name) != getattr(first, name):
                    raise ValueError(f"the members of an ensemble share one architecture: {name} differs "
                                     f"({getattr(m, name)!r} against {getattr(first, name)!r})")
            if not all(np.array_equal(getattr(m, n), getattr(first, n)) for n in ("goal", "q", "r")):
                raise ValueError("the members of an ensemble share one cost: goal, q and r must be equal (set_cost sets all)")
        self._members = members
        self._nominal = self._check_index(nominal)
        self._nominal_version = 0
        self._stack = None  # (member versions, the stacked tables [E, n])

    @classmethod
    def from_modules(cls, modules: Sequence[torch.nn.Module], nominal: int = 0, model_class=MLPModel, **kw) -> "MLPEnsemble":
        """One model_class.from_module(net, **kw) per network (goal=, q=, r=, residual=: the same for all); model_class:
        MLPModel or MLPModel8."""
        return cls([model_class.from_module(m, **kw) for m in modules], nominal=nominal)

    def _check_index(self, e) -> int:
        if isinstance(e, bool) or int(e) != e or not 0 <= int(e) < len(self._members):
            raise ValueError(f"member index {e!r}: the ensemble has members 0..{len(self._members) - 1}")
        return int(e)

    # ------------------------------------------------------------------ members
    @property
    def n_members(self) -> int:
        return len(self._members)

    @property
    def nominal(self) -> int:
        return self._nominal

    def member(self, e: int) -> MLPModel:
        """Member e's MLPModel (its callables run anywhere, the solver's generic path included)."""
        return self._members[self._check_index(e)]

    def set_nominal(self, e: int) -> None:
        """Which member `dynamics` / `cost` and everything outside the particle rollout evaluate, from the next solve on."""
        e = self._check_index(e)
        if e != self._nominal:
            self._nominal = e
            self._nominal_version += 1

    def update_weights(self, e: int, weights: Sequence, biases: Sequence) -> None:
        """New weights of the same shapes for member e (a model learned online); the solver uploads that member's table only."""
        self._members[self._check_index(e)].update_weights(weights, biases)

    def set_cost(self, goal=None, q=None, r=None) -> None:
        """MLPModel.set_cost for every member: there is one cost."""
        for m in self._members:
            m.set_cost(goal=goal, q=q, r=r)

    def set_reference(self, goals, q=None) -> None:
        """MLPModel.set_reference for every member: there is one cost, and ONE table — the members share the tensor (and its
        copies on other devices), so rewriting `reference` in place and reference_changed() reach every member."""
        first = self._members[0]
        first.set_reference(goals, q)
        self._share_reference()

    def _share_reference(self) -> None:
        first = self._members[0]
        for m in self._members[1:]:
            m._ref, m._ref_own_q, m._ref_mirrors = first._ref, first._ref_own_q, first._ref_mirrors
            m.reference_version = max(m.reference_version, first.reference_version) + 1

    def set_value(self, weights, biases=None, **kw) -> None:
        """MLPModel.set_value for every member: ONE value network per ensemble, shared by its members (checked on the first: a
        refused network changes none).  A value per member is not built."""
        self._members[0].set_value(weights, biases, **kw)
        for m in self._members[1:]:
            m.set_value(weights, biases, **kw)

    def set_value_module(self, module, **kw) -> None:
        self._members[0].set_value_module(module, **kw)
        for m in self._members[1:]:
            m.set_value_module(module, **kw)

    def update_value(self, weights, biases) -> None:
        self._members[0].update_value(weights, biases)
        for m in self._members[1:]:
            m.update_value(weights, biases)

    def set_value_weight(self, weight: float) -> None:
        self._members[0].set_value_weight(weight)
        for m in self._members[1:]:
            m.set_value_weight(weight)

    def set_angular(self, angular) -> None:
        """MLPModel.set_angular for every member (checked on the first: a refused mask changes none)."""
        self._members[0].set_angular(angular)
        for m in self._members[1:]:
            m.set_angular(angular)

    def reference_changed(self) -> None:
        """The shared table was rewritten in place: its copies on other devices are refreshed ONCE, every member's version moves."""
        first = self._members[0]
        first.reference_changed()
        for m in self._members[1:]:
            if m._ref is first._ref:
                m.reference_version += 1
            else:
                m.reference_changed()

    @property
    def version(self) -> int:
        """Moves whenever a member's weights or the nominal index changed."""
        return sum(m.version for m in self._members) + self._nominal_version

    @property
    def tables(self) -> np.ndarray:
        """The members' tables stacked, float32 [E, n] (row e is member(e).table)."""
        key = tuple(m.version for m in self._members)
        if self._stack is None or self._stack[0] != key:
            self._stack = (key, np.ascontiguousarray(np.stack([m.table for m in self._members]), dtype=np.float32))
        return self._stack[1]

    # ------------------------------------------------------------------ what the solver asks for
    @property
    def model_name(self) -> str:
        return self._members[0].model_name

    def __getattr__(self, name):  # (the architecture, as the members state it)
        if name in ("dim_state_model", "dim_control", "hidden_layers", "activation", "residual", "goal", "q", "r", "DS",
                    "dim_state", "pad_state", "angular", "angular_mask", "reference", "reference_version",
                    "value", "value_version", "value_of"):
            return getattr(self.__dict__["_members"][self.__dict__["_nominal"]], name)
        raise AttributeError(name)

    def native_inputs(self) -> dict:
        spec = self._members[self._nominal].native_inputs()
        spec["mlp"].update(tables=self.tables, nominal=self._nominal, version=self.version,
                           member_versions=tuple(m.version for m in self._members))
        return spec

    # ------------------------------------------------------------------ the callables: the nominal member's
    @native_model(lambda owner: owner.model_name, "dynamics")
    def dynamics(self, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        return self._members[self._nominal].dynamics(state, action)

    @native_model(lambda owner: owner.model_name, "cost", _provider)
    def cost(self, state: torch.Tensor, action: torch.Tensor, info=None) -> torch.Tensor:
        return self._members[self._nominal].cost(state, action, info)

    @native_model(lambda owner: owner.model_name, "terminal", _provider)
    def terminal_cost(self, state: torch.Tensor, info=None) -> torch.Tensor:
        return self._members[self._nominal].terminal_cost(state, info)

    def __deepcopy__(self, memo):
        import copy

        new = object.__new__(type(self))
        memo[id(self)] = new
        new.__dict__.update(_members=[copy.deepcopy(m, memo) for m in self._members], _nominal=self._nominal,
                            _nominal_version=self._nominal_version, _stack=None)
        if all(m._ref is self._members[0]._ref for m in self._members):  # (one table stays one table in the copy)
            new._share_reference()
        return new
