"""Cases of tests/test_gpu_noise_and_lookup_bits.py, shared with the script that records its fixture
(scripts/record_noise_bits.py): every consumer of the device noise source (csrc/philox.hpp: box_muller) and the padded-map
lookup at the smallest shapes at which they can go wrong, run for two consecutive solves (the second warm-started, at the next
solve index).  The recorded items of a solve: the exported noise [N, T, dc], `costs`, `action_seq`, `state_seq`.

Shapes.  N = 130: two full 64-lane tiles and a two-lane third; N = 64: one.  T = 5 at dc = 2 (and dc = 1 with four steps per
float4 group): a ragged last group; T = 4: none.  dc = 1 (pendulum), dc = 2 (racing, nav2d); no native model has dc = 4, so
that width is a generic handle's draw (sample_kernel) only.  `noise_regen` 1 (the rollout and the reduction regenerate the
noise in registers) and 0 (materialised tiles); `math` 2, 1 and, once, 0; the single launch (mppi_solve at N <= 4096) and the
multi-kernel sequence; a dense temperature (every tile of the softmax is regenerated) and lambda = 1; `noise_beta`
(sample_colored_kernel); covariance adaptation (weighted_variance_kernel); and a window of the sample stream whose second
tile straddles the global index 2^32 — the offset a rank of a sharded solve of 2^33 samples would own, set through the same
field (`shard_range` -> MppiConfig.sample_offset) as the sharding keyword sets it.
"""
import ctypes as C

import numpy as np
import torch

STRADDLE = (1 << 32) - 66  # tile 0 ends at 2^32 - 3, tile 1 (lanes 64..127) crosses 2^32 at its third lane

MK = dict(fused_solve=0)  # the multi-kernel sequence


def case(name, model, T, N, lam, options=None, offset=0, **kw):
    return dict(name=name, model=model, T=T, N=N, lam=lam, options=dict(options or {}), offset=offset, kw=kw)


CASES = [
    case("racing_regen_dense", "racing", 5, 130, 200.0, dict(MK, noise_regen=1)),
    case("racing_tiles_dense", "racing", 5, 130, 200.0, dict(MK, noise_regen=0)),
    case("racing_regen_T4_N64_math1", "racing", 4, 64, 1.0, dict(MK, noise_regen=1, math=1)),
    case("racing_tiles_math1", "racing", 5, 130, 200.0, dict(MK, noise_regen=0, math=1)),
    case("racing_regen_math0", "racing", 5, 130, 1.0, dict(MK, noise_regen=1, math=0)),
    case("racing_single_launch", "racing", 5, 130, 200.0),
    case("racing_single_launch_T4_N64_math1", "racing", 4, 64, 1.0, dict(math=1)),
    case("racing_colored", "racing", 5, 130, 200.0, dict(MK), noise_beta=[0.8, 0.3]),
    case("racing_straddle_regen", "racing", 5, 130, 200.0, dict(MK, noise_regen=1), offset=STRADDLE),
    case("racing_straddle_tiles", "racing", 5, 130, 200.0, dict(MK, noise_regen=0), offset=STRADDLE),
    case("nav2d_regen", "nav2d", 5, 130, 5.0, dict(MK, noise_regen=1)),
    case("nav2d_tiles_T4_N64", "nav2d", 4, 64, 5.0, dict(MK, noise_regen=0)),
    case("nav2d_regen_math1", "nav2d", 5, 130, 5.0, dict(MK, noise_regen=1, math=1)),
    case("nav2d_single_launch", "nav2d", 5, 130, 5.0),
    case("pendulum_regen", "pendulum", 5, 130, 1.0, dict(MK, noise_regen=1)),
    case("pendulum_tiles_T4_N64", "pendulum", 4, 64, 1.0, dict(MK, noise_regen=0)),
    case("pendulum_single_launch", "pendulum", 5, 130, 1.0),
    case("pendulum_colored", "pendulum", 5, 130, 1.0, dict(MK), noise_beta=0.7),
    case("pendulum_adaptive", "pendulum", 5, 130, 1.0, dict(MK), adapt_covariance=True),
    case("pendulum_straddle_single_launch", "pendulum", 5, 130, 1.0, offset=STRADDLE),
]
GENERIC = [dict(name=f"generic_dc{dc}_straddle", dc=dc, T=5, N=130, offset=STRADDLE) for dc in (1, 2, 4)]
ITEMS = ("eps", "costs", "action_seq", "state_seq")


def _took_single_launch(h):
    g, s = C.c_int(-1), C.c_int(-1)
    h.call("mppi_fused_geometry", C.byref(g), C.byref(s))
    return (g.value, s.value) != (0, 0)


def run(c, make):
    """{f"{item}_{k}": array} of the two solves of case `c`; make = tests/test_gpu_covariance.make."""
    from pi_mpc import mppi as solver_module

    n_global, owner = c["N"], solver_module.shard_range
    if c["offset"]:  # this handle owns [offset, offset + N) of a solve of 2 * offset + 2 N samples (rank 1 of 2)
        n_global = 2 * (c["offset"] + c["N"])
        solver_module.shard_range = lambda n, world, rank: (c["offset"], c["N"])
    try:
        solver, x0 = make(c["model"], c["T"], n_global, c["lam"], **c["kw"])
    finally:
        solver_module.shard_range = owner
    assert (solver._sample_offset, solver._local_samples) == (c["offset"], c["N"])
    for key, value in c["options"].items():
        solver.set_option(key, value)
    x, out = x0.cuda(), {}
    for k in range(2):
        a, s = solver.forward(x)
        eps = torch.empty(c["N"], c["T"], solver._dim_control, device="cuda")
        solver._h.call("mppi_export_noise", eps.data_ptr(), None, solver._stream())
        torch.cuda.synchronize()
        assert _took_single_launch(solver._h) == ("fused_solve" not in c["options"]), (c["name"], k)
        got = dict(eps=eps, costs=solver._costs, action_seq=a, state_seq=torch.as_tensor(s))
        for item in ITEMS:
            v = got[item].detach().cpu().numpy().astype(np.float32, copy=True)
            assert np.isfinite(v).all(), (c["name"], item, k)
            out[f"{item}_{k}"] = v
    assert not np.array_equal(out["eps_0"], out["eps_1"]), c["name"]  # (the solve index moved)
    return out


def run_generic(g):
    """The draw of a generic handle (sample_kernel) at two solve indices: {f"eps_{k}": [N, T, dc]}."""
    from mppi_playground_amd import _capi

    f4 = lambda *v: (C.c_float * 4)(*v)  # noqa: E731
    cfg = _capi.MppiConfig(model=_capi.MODEL_GENERIC, horizon=g["T"], dim_state=2, dim_control=g["dc"], num_samples=g["N"],
                           sample_offset=g["offset"], inherit_count=1 << 40, u_min=f4(-1, -1, -1, -1), u_max=f4(1, 1, 1, 1),
                           sigmas=f4(0.5, 0.25, 1.0, 2.0), seed=42, device=0)
    h, out = _capi.Handle(cfg), {}
    for k in range(2):
        e = torch.empty(g["N"], g["T"], g["dc"], device="cuda")
        h.call("mppi_sample", 3 + k, None)
        h.call("mppi_export_noise", e.data_ptr(), None, None)
        torch.cuda.synchronize()
        out[f"eps_{k}"] = e.cpu().numpy()
        assert np.isfinite(out[f"eps_{k}"]).all()
    h.close()
    return out
