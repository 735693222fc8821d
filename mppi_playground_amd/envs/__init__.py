"""The shipped model plugins (dynamics / cost callables) and their host-side set-up code.

Each callable keeps the reference's contract — dynamics(state[B,ds], action[B,dc]) -> [B,ds],
cost(state[B,ds], action[B,dc], info) -> [B] in torch — and additionally carries a native tag
(pi_mpc/native.py) so that pi_mpc.mppi.MPPI runs it fused on the device.  Rendering / video /
gymnasium simulators of the reference are UI and out of scope; `render()`/`close()` are no-ops.
"""

from envs.mlp_model import MLPModel  # noqa: E402,F401  (learned dynamics: an MLP whose weights are data)
from envs.mlp_model import MLPModel8  # noqa: E402,F401  (the same with 8 states and 1, 2 or 4 controls)
from envs.mlp_model import MLPEnsemble  # noqa: E402,F401  (a bootstrap ensemble of them: one particle per network)
from envs.navigation_2d_moving import MovingObstacleNav2DEnv  # noqa: E402,F401  (nav2d + moving discs, one row per horizon step)
from envs.navigation_2d_moving import SoftMovingObstacleNav2DEnv  # noqa: E402,F401  (... with a graded penalty skirt round every disc)
