/*
 * mppi_hip.h — C ABI of libmppi_hip.so: the MI355X (gfx950) implementation of the
 * pi_mpc.mppi.MPPI.forward() hot path of kohonda/mppi_playground.
 *
 * The reference is pure Python/PyTorch, so the "FFI" a maintainer would add is a ctypes
 * binding inside src/pi_mpc/mppi.py (shown in INTEGRATION.md).  Every entry point below
 * names the reference code it replaces (file:line relative to the reference repo).
 *
 * Conventions
 *   - plain C: opaque handle, POD structs, raw pointers and sizes; no torch/HIP types.
 *   - every function returns 0 on success or a negative MPPI_E_* code; the message of the
 *     last failure on a handle is available from mppi_last_error().  Nothing throws.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All device work
 *     is enqueued asynchronously on it; only the functions documented "synchronises" block.
 *   - pointers named *_dev are device pointers (HBM), *_host are host pointers.
 *   - all arithmetic is fp32 (reference dtype, mppi.py:45).
 *
 * Data layout in HBM (owned by the handle)
 *   noise   lane-major tiles: for tile b (samples 64b..64b+63) and float4 group r
 *           (flat horizon index 4r..4r+3 of the [T*dc] row) lane l's float4 lives at
 *           ((b*R + r)*64 + l), R = ceil(T*dc/4).  A wavefront therefore reads or writes one
 *           contiguous 1 KiB segment per instruction.  This is the storage of the reference's
 *           `_action_noises` [N,T,dc] (mppi.py:261-263); mppi_export_noise() converts.
 *   costs   float[N]                                    (`costs`, mppi.py:333-336)
 *   summary float[MPPI_SUMMARY_HEAD + T*dc] per shard   (see mppi_weights_reduce)
 */
#ifndef MPPI_HIP_H
#define MPPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct MppiSolver* mppi_handle_t;

enum {
    MPPI_OK = 0,
    MPPI_E_INVALID = -1,   /* bad argument / unsupported configuration */
    MPPI_E_HIP = -2,       /* a HIP runtime call failed                */
    MPPI_E_STATE = -3,     /* call sequence error (e.g. no map uploaded) */
    MPPI_E_NODEVICE = -4   /* no gfx950 device visible                 */
};

/* Native model plugins = the five shipped dynamics/cost pairs and the two
 * remaining example models.
 * MPPI_MODEL_GENERIC: the callables are opaque to the library (any torch dynamics/cost): the host
 * evaluates them on the exported actions and hands the costs back with mppi_set_costs; sampling,
 * softmax, the weighted reduction and the warm start still run here.  mppi_rollout_cost, the
 * state output of mppi_finalize and the mppi_rollout_* entry points are unavailable
 * (MPPI_E_INVALID). */
enum {
    MPPI_MODEL_GENERIC = -1,
    MPPI_MODEL_PENDULUM = 0,    /* example/pendulum.py:17-47                                  */
    MPPI_MODEL_CARTPOLE = 1,    /* example/cartpole.py:17-81                                  */
    MPPI_MODEL_MOUNTAINCAR = 2, /* example/mountaincar.py:17-55                               */
    MPPI_MODEL_NAV2D = 3,       /* src/envs/navigation_2d.py:218-279                          */
    MPPI_MODEL_RACING = 4,      /* src/envs/racing_env.py:327-372 + example/racing.py:110-159 */
    MPPI_MODEL_MJCARTPOLE = 5,  /* example/mujoco_cartpole.py:20-81 (continuous force, masspole = 1) */
    MPPI_MODEL_GOALZONE = 6,    /* src/envs/goal_in_danger_zone.py:113-156 (7-state unicycle + circle) */
    MPPI_MODEL_MLP41 = 7,       /* learned dynamics: a small MLP, 4 states, 1 control (mppi_set_mlp)  */
    MPPI_MODEL_MLP42 = 8,       /* the same with 2 controls                                           */
    MPPI_MODEL_NAV2D_DISCS = 9, /* MPPI_MODEL_NAV2D + up to MPPI_MAX_DISCS moving disc obstacles (mppi_set_discs) */
    MPPI_MODEL_RACING_DISCS = 10, /* MPPI_MODEL_RACING + up to MPPI_MAX_DISCS moving disc obstacles: opponent cars (mppi_set_discs) */
    MPPI_MODEL_NAV2D_DISCS_SOFT = 11,  /* MPPI_MODEL_NAV2D_DISCS with a graded penalty skirt round every disc (mppi_set_disc_softness) */
    MPPI_MODEL_RACING_DISCS_SOFT = 12, /* MPPI_MODEL_RACING_DISCS with the same skirt */
    MPPI_MODEL_MLP81 = 13,      /* learned dynamics: the MLP of MPPI_MODEL_MLP41 with 8 states, 1 control (mppi_set_mlp) */
    MPPI_MODEL_MLP82 = 14,      /* the same with 2 controls                                           */
    MPPI_MODEL_MLP84 = 15       /* the same with 4 controls                                           */
};

/* Racing parameter vector (mppi_set_model_params), racing_env.py:37-42,341-370, racing.py:41-46 */
enum { MPPI_RP_AMIN = 0, MPPI_RP_AMAX, MPPI_RP_SMIN, MPPI_RP_SMAX, MPPI_RP_L, MPPI_RP_VMAX, MPPI_RP_DT,
       MPPI_RP_XLO, MPPI_RP_XHI, MPPI_RP_YLO, MPPI_RP_YHI, MPPI_RP_QC, MPPI_RP_QL, MPPI_RP_QV, MPPI_RP_QO,
       MPPI_RP_QIN, MPPI_RP_QDIN, MPPI_RP_COUNT };
/* Navigation2D parameter vector, navigation_2d.py:54-72,218-279 */
enum { MPPI_NP_VMIN = 0, MPPI_NP_VMAX, MPPI_NP_WMIN, MPPI_NP_WMAX, MPPI_NP_DT, MPPI_NP_XLO, MPPI_NP_XHI,
       MPPI_NP_YLO, MPPI_NP_YHI, MPPI_NP_GX, MPPI_NP_GY, MPPI_NP_QO, MPPI_NP_COUNT };
#define MPPI_MAX_DISCS 8 /* moving discs per horizon step of MPPI_MODEL_NAV2D_DISCS / MPPI_MODEL_RACING_DISCS (the MPPI_NP_* /
                          * MPPI_RP_* parameters of nav2d / racing) */

/* Goal-in-danger-zone parameter vector, goal_in_danger_zone.py:78-87,113-156 */
enum { MPPI_GP_VMIN = 0, MPPI_GP_VMAX, MPPI_GP_WMIN, MPPI_GP_WMAX, MPPI_GP_DT, MPPI_GP_GX, MPPI_GP_GY, MPPI_GP_CX,
       MPPI_GP_CY, MPPI_GP_RADIUS, MPPI_GP_PENALTY, MPPI_GP_COUNT };

/* Learned-dynamics (MLP) cost parameters: c = sum_m q[m] * (s[m] - g[m])^2 + sum_k r[k] * u[k]^2 (mppi_set_mlp has the
 * arithmetic; mppi_set_mlp_reference replaces g, q by a row per horizon step, mppi_set_mlp_angular wraps angle errors):
 * g[4], q[4], r[dim_control] -> 9 values for MPPI_MODEL_MLP41, 10 for MPPI_MODEL_MLP42 */
enum { MPPI_MP_G = 0, MPPI_MP_Q = 4, MPPI_MP_R = 8, MPPI_MP_COUNT41 = 9, MPPI_MP_COUNT42 = 10 };
/* The same for the 8-state ids: g[8], q[8], r[dim_control] -> 17 values for MPPI_MODEL_MLP81, 18 for MPPI_MODEL_MLP82, 20 for
 * MPPI_MODEL_MLP84 */
enum { MPPI_MP8_G = 0, MPPI_MP8_Q = 8, MPPI_MP8_R = 16, MPPI_MP8_COUNT81 = 17, MPPI_MP8_COUNT82 = 18, MPPI_MP8_COUNT84 = 20 };
#define MPPI_MLP_HIDDEN 32 /* hidden width of the table; narrower layers are zero-padded by the caller */
/* mppi_set_mlp `activation` */
enum { MPPI_MLP_RELU = 0, MPPI_MLP_TANH = 1 };

#define MPPI_MAX_PARAMS 32
#define MPPI_MAX_DIM_STATE 8
#define MPPI_MAX_DIM_CONTROL 4          /* controls held by MppiConfig (native models: 1, 2 or 4)            */
#define MPPI_MAX_DIM_CONTROL_GENERIC 64 /* MPPI_MODEL_GENERIC: any dim_control up to this (mppi.py:96-98)    */
#define MPPI_SUMMARY_HEAD 4 /* {min cost, sum e, sum e^2, sum e*c} */

/* Constructor arguments that reach the device path (MPPI.__init__, mppi.py:24-47,109-121). */
typedef struct MppiConfig {
    int32_t model;          /* MPPI_MODEL_*                                                     */
    int32_t horizon;        /* T                                                                */
    int32_t dim_state;      /* must match the model (any value >= 1 for MPPI_MODEL_GENERIC)     */
    int32_t dim_control;    /* must match the model (1..MPPI_MAX_DIM_CONTROL_GENERIC for GENERIC) */
    int64_t num_samples;    /* N held by THIS handle (= the local shard when sharded)           */
    int64_t sample_offset;  /* global index of local sample 0 (0 when not sharded)              */
    int64_t inherit_count;  /* global threshold int(N_global*(1-exploration)), mppi.py:266      */
    float u_min[MPPI_MAX_DIM_CONTROL];
    float u_max[MPPI_MAX_DIM_CONTROL];
    float sigmas[MPPI_MAX_DIM_CONTROL];
    uint64_t seed;          /* Philox key (mppi.py:46,93 `seed`)                                */
    int32_t device;         /* HIP device ordinal                                               */
    int32_t reserved;
} MppiConfig;

/* Library / build information ("gfx950", version). */
const char* mppi_version(void);
/* Integer version of THIS header's function signatures; bindings compare it with the constant they were written
 * against and refuse a stale library (a changed argument list would otherwise be called with shifted arguments). */
#define MPPI_ABI_VERSION 16
int mppi_abi_version(void);
/* Number of visible HIP devices (0 => the product cannot run; callers must fail loudly). */
int mppi_device_count(void);
const char* mppi_last_error(mppi_handle_t h);

/* MPPI.__init__ buffers (mppi.py:143-180): allocates noise tiles, costs, warm start (zeroed,
 * mppi.py:157), partials.  Does NOT draw the constructor sample (mppi.py:146-148 is only an
 * RNG-stream side effect; callers that mirror the torch CPU stream draw it themselves). */
int mppi_create(const MppiConfig* cfg, mppi_handle_t* out);
int mppi_destroy(mppi_handle_t h);
/* `u_min`, `u_max`, `sigmas` constructor tensors (mppi.py:32-34,96-98,109-121) as host arrays of n = dim_control
 * values: replaces the bounds / noise scales taken from MppiConfig.  REQUIRED once, before the first sample, for
 * generic handles with dim_control > MPPI_MAX_DIM_CONTROL (the config arrays hold four); native models accept it
 * only before mppi_set_model_params.  The per-step sigma table of the covariance adaptation (mppi_get_sigma_table) starts over
 * from the new `sigmas`, adapted or not, and noise tiles already drawn from the old values are dropped.  Synchronises. */
int mppi_set_control_limits(mppi_handle_t h, const float* u_min_host, const float* u_max_host, const float* sigmas_host,
                            int n);

/* copy.deepcopy(solver) (the reference's MPPI is a plain nn.Module, src/pi_mpc/mppi.py:16: every tensor it holds is copied
 * with it).  `dst` must have been created from the same MppiConfig; after the call it continues exactly like `src`: warm
 * start (`_previous_action_seq`), noise identity, costs and minimum of the last solve (get_top_samples / weights work on
 * the copy), Savitzky-Golay taps and history, the temperature with every device-resident search / dual state (ESSPS warm
 * grid, MPO dual and Adam moments), model parameters, maps, reference window, centre path and path index, options.
 * A borrowed state (mppi_bind_state) becomes an owned copy; a pending lazily completed state sequence is completed on
 * both handles first.  Set-up path: synchronises the device. */
int mppi_clone_state(mppi_handle_t dst, mppi_handle_t src);
/* Model constants (closures' Python constants / env attributes).  params: MPPI_RP_* or MPPI_NP_*
 * layout; models without parameters accept n == 0. */
int mppi_set_model_params(mppi_handle_t h, const float* params_host, int n);
/* ObstacleMap.convert_to_torch / LaneMap._map_torch (obstacle_map_2d.py:164-166,
 * lane_map_2d.py:85-88): occupancy grid cells[nx][ny] (0/1), first index = x.
 * slot 0 = obstacle map (nav2d, racing), slot 1 = lane map (racing).  Synchronises. */
int mppi_upload_map(mppi_handle_t h, int slot, const uint8_t* cells_host, int nx, int ny, float cell_size,
                    float origin_x, float origin_y);
/* Map construction on the device, bit-exact with the reference's host loops.  Both build slot `slot` in place
 * (same geometry arguments as mppi_upload_map), run on `stream` and return after the grid is complete; the caller
 * orders them against solves in flight on OTHER streams.
 *
 * ObstacleMap.add_circle_obstacle / add_rectangle_obstacle (obstacle_map_2d.py:103-158) for a whole obstacle list:
 *   circles [n_circles][3] = (ci, cj, r): centre cell np.round(center/cell + origin) and radius ceil(radius/cell)
 *                            in cells; every disc cell i^2+j^2 <= r^2 is written at clip(ci+i), clip(cj+j) (:118-123);
 *   rects   [n_rects][4]   = (x0, x1, y0, y1): the clipped half-open slice map[x0:x1, y0:y1] = 1 (:146-158).
 * The float -> cell conversions stay with the caller (per obstacle, float64 numpy semantics). */
int mppi_build_obstacle_map(mppi_handle_t h, int slot, int nx, int ny, float cell_size, float origin_x, float origin_y,
                            const int32_t* circles_host, int n_circles, const int32_t* rects_host, int n_rects,
                            void* stream);
/* LaneMap.populate_map (lane_map_2d.py:68-88): seeds [n_seeds][2] = in-bounds centre-line cells (:71-77); a cell is
 * drivable (0) iff its Euclidean distance transform value is <= (lane_width/2)/cell (:80-82), evaluated as the
 * integer test  min_seeds(dx^2+dy^2) <= max_d2  with max_d2 = the largest integer whose float64 sqrt is <= that
 * bound (computed by the caller). */
int mppi_build_lane_map(mppi_handle_t h, int slot, int nx, int ny, float cell_size, float origin_x, float origin_y,
                        const int32_t* seeds_host, int n_seeds, int64_t max_d2, void* stream);
/* Read a slot's grid back (cells_host may be NULL to query nx, ny only).  Synchronises the device. */
int mppi_download_map(mppi_handle_t h, int slot, uint8_t* cells_host, int* nx, int* ny);
/* racing_controller.reference_path = calc_ref_trajectory(...) (example/racing.py:73-81):
 * ref [rows][4] = (x, y, yaw, v_target), rows >= T (the cost reads rows 0..T-1).  MPPI_E_INVALID on a handle of a model
 * without a reference window (every model but the two racing ones). */
int mppi_set_reference(mppi_handle_t h, const float* ref_host, int rows, void* stream);
/* Learned dynamics for MPPI_MODEL_MLP41 / MPPI_MODEL_MLP42: the weights of a multi-layer perceptron with 4 states,
 * dc = 1 / 2 controls, `hidden_layers` = 1 or 2 hidden layers of MPPI_MLP_HIDDEN = 32 units and 4 outputs, as ONE table of
 * n_floats = 32*IN + 32 + 32*32 + 32 + 4*32 + 4 fp32 values (IN = 4 + dc: 1380 / 1412), row-major, in the order
 *     W1[32][IN], b1[32], W2[32][32], b2[32], W3[4][32], b3[4]
 * (W2 / b2 are not read with one hidden layer).  A narrower layer is padded with zero rows, columns and biases, a model
 * with fewer than four states with components that stay zero: relu(0) = tanh(0) = 0 and adding w*0 or 0*x changes no bit
 * of a sum.  The step, in fp32 — at option "math" = 0 every operation rounds on its own, in exactly this order; the fast
 * levels may contract a*b + c and evaluate tanh with the hardware exponential and reciprocal:
 *     x = [s[0..3], u[0..dc-1]]                    (u: the solver-clamped action; the model does not clamp again)
 *     z[j] = b1[j]; for i = 0..IN-1: z[j] = z[j] + W1[j][i] * x[i];   h1[j] = act(z[j])             (j = 0..31)
 *     two hidden layers: the same over the 32 entries of h1 with W2, b2 -> h2
 *     o[m] = b3[m]; for j = 0..31: o[m] = o[m] + W3[m][j] * h[j]                                    (m = 0..3)
 *     next[m] = residual ? s[m] + o[m] : o[m]
 * act = fmaxf(z, 0) (MPPI_MLP_RELU) or tanh (MPPI_MLP_TANH).  Stage cost on the state a step starts from and its action,
 * terminal cost the same function of the last state with a zero action (parameters: MPPI_MP_*, mppi_set_model_params):
 *     c = 0; for m = 0..3: d = s[m] - g[m], c = c + q[m] * (d * d); for k = 0..dc-1: c = c + r[k] * (u[k] * u[k])
 * The table is staged and copied on `stream` (no host wait), like mppi_set_reference's window, and may be replaced between
 * solves (a model learned online: every tick); a lazily completed state sequence is completed with the old weights first.
 * MPPI_E_INVALID for another model's handle, a wrong count, a flag out of range or a value that is not finite.  Solves on
 * an MLP handle without a table return MPPI_E_STATE.  mppi_clone_state copies table and flags; mppi_model_step does not
 * take these models (MPPI_E_INVALID: it has no handle to take the table from).
 * MPPI_MODEL_MLP81 / MLP82 / MLP84 are the same network with DS = 8 states and dc = 1 / 2 / 4 controls: read 8 for every 4
 * above (x = [s[0..7], u[0..dc-1]], m = 0..7, IN = 8 + dc, the parameters MPPI_MP8_*), the table in the same order
 *     W1[32][IN], b1[32], W2[32][32], b2[32], W3[8][32], b3[8]
 * of n_floats = 32*IN + 32 + 32*32 + 32 + 8*32 + 8 = 1640 / 1672 / 1736 values; a model with fewer than eight states is
 * padded the same way.  Same operation order, same flags, same entry points (ensembles and particle members included). */
int mppi_set_mlp(mppi_handle_t h, const float* table_host, int n_floats, int hidden_layers, int activation, int residual,
                 void* stream);
/* Model ensembles for the learned dynamics: E = n_members networks of ONE architecture (one set of flags), each a table as
 * mppi_set_mlp takes it, laid out tables_host[E][n_floats] and kept in one device buffer, 1 <= E <= MPPI_MAX_PARTICLES.
 * mppi_set_mlp is the case E = 1.  A risk-aware solve (mppi_set_particles) may then carry every particle through a member of
 * its own (mppi_set_particle_members): the cost of (sample i, particle m) is what a plain handle holding member members[m]'s
 * table computes for sample i from x0 = particles[m] — the arithmetic of mppi_set_mlp, the same functor, read from that
 * member's table — and the fold judges a plan by the mean, the worst case or the CVaR over the members.
 * THE NOMINAL MEMBER: everything outside the particle rollout evaluates ONE network, member `nominal` — the rollout of a
 * plain solve, mppi_finalize's state sequence (a lazily completed one included), the re-rolls of mppi_top_samples /
 * mppi_rollout_samples / mppi_rollout_candidates and mppi_rollout_actions.  The members decide particle costs only.
 *   mppi_set_mlp_ensemble  checks as mppi_set_mlp does (count, flags, finite values; 0 <= nominal < E), completes a pending
 *                        lazily completed state sequence with the OLD weights first, stages and copies the E tables on
 *                        `stream`.  A buffer too small for them is reallocated (blocking: set-up path).
 *   mppi_set_mlp_member  replaces member e's table (a model learned online: one member per tick); the flags stay.  A pending
 *                        state sequence is completed with the old weights first.  MPPI_E_STATE before any table was set.
 *   mppi_set_mlp_nominal re-points the nominal member (a pending state sequence is completed under the OLD one first).
 *   mppi_get_mlp_ensemble  E and the nominal index (either pointer may be NULL); E = 0 while no table is set.
 * MPPI_E_INVALID for another model's handle, E = 0 or E > MPPI_MAX_PARTICLES, an index out of range, a wrong count, a flag out
 * of range or a value that is not finite.  mppi_clone_state copies all E tables, the flags and the nominal index. */
int mppi_set_mlp_ensemble(mppi_handle_t h, const float* tables_host /* [n_members][n_floats] */, int n_members, int n_floats,
                          int hidden_layers, int activation, int residual, int nominal, void* stream);
int mppi_set_mlp_member(mppi_handle_t h, int e, const float* table_host, int n_floats, void* stream);
int mppi_set_mlp_nominal(mppi_handle_t h, int e);
int mppi_get_mlp_ensemble(mppi_handle_t h, int* n_members_out, int* nominal_out);
/* Tracking costs for the learned-dynamics models (all five MPPI_MODEL_MLP* ids): a goal that moves along the horizon and state
 * components that are angles.  The reference is a table rows[n_rows][2 * DS] (DS = 4 or 8, the model's state width): row t is
 * the goal g_t[DS] and then the weights q_t[DS] of horizon step t; a component the network does not have is padded with g = 0,
 * q = 0.  The angular mask has bit m set when state component m is an angle.  The cost, in fp32 and in this order (at option
 * "math" = 0 every operation rounds on its own; the fast levels may contract a * b + c):
 *     g_t, q_t = row t of the reference                 (no reference: g_t = g, q_t = q of the parameters, as before)
 *     d[m] = s[m] - g_t[m]
 *     m angular:  k = rint(d[m] * INV_TWO_PI);  d[m] = d[m] - TWO_PI * k
 *                 (TWO_PI = 6.2831855f, INV_TWO_PI = 0.15915494f, rint = round half to even: the error lies in [-pi, pi])
 *     c = 0; for m ascending: c = c + q_t[m] * (d[m] * d[m]); for k ascending: c = c + r[k] * (u[k] * u[k])
 * The stage cost of step t reads row t; the terminal cost reads row T - 1 with u = 0, the rule of every time-indexed cost here
 * (the reference solver evaluates it with the stale info["t"] = T - 1): there is no row T.  To weight the END of the horizon,
 * put the weight into q of row T - 1: it counts for the state of step T - 1 and for the final state.  r stays a parameter.
 * Every kernel that evaluates the model carries both: the rollout (regenerated noise and tiles, with or without the
 * control-cost term), the single cooperative launch, the particle rollout (all particles and members share the reference) and
 * the wavefront-per-trajectory comparison kernel.
 * Without a reference and without a mask nothing changes: g and q travel in the kernel arguments as before.
 * The reference rides in the handle's first map slot: a learned-dynamics handle has no maps, and mppi_upload_map /
 * mppi_build_obstacle_map / mppi_build_lane_map return MPPI_E_INVALID on one (they were accepted and ignored before).
 *   mppi_set_mlp_reference  the handle keeps its own device copy.  A host table (on_device = 0) is checked (every value
 *                        finite, else MPPI_E_INVALID), staged and copied on `stream` without a host wait, as mppi_set_discs does
 *                        it; a device table (on_device = 1) is copied device-to-device in stream order and never meets the
 *                        host.  rows = NULL or n_rows = 0 switches the reference off.  A buffer too small for the table is
 *                        reallocated (blocking: set-up path).  A solve with 0 < n_rows < T returns MPPI_E_STATE before
 *                        anything is launched.
 *   mppi_get_mlp_reference  n_rows (0: none) and, unless `out` is NULL, the table [n_rows][2 * DS] (a host `out` waits for
 *                        `stream`).
 *   mppi_set_mlp_angular / mppi_get_mlp_angular  the mask; MPPI_E_INVALID for a bit at or above DS.  May be set before or after
 *                        the weight table: the architecture flags and the mask are composed by one owner.
 * MPPI_E_INVALID on another model's handle.  mppi_clone_state carries the table and the mask; mppi_model_step is dynamics only. */
int mppi_set_mlp_reference(mppi_handle_t h, const float* rows /* [n_rows][2 * DS] */, int n_rows, int on_device, void* stream);
int mppi_get_mlp_reference(mppi_handle_t h, float* out, int* n_rows_out, int on_device, void* stream);
int mppi_set_mlp_angular(mppi_handle_t h, uint32_t mask);
int mppi_get_mlp_angular(mppi_handle_t h, uint32_t* mask_out);
/* A learned terminal value for the learned-dynamics models: a second network V evaluated ONCE per trajectory on its final
 * state s_T (as the dynamics network produced it: the angular mask does not wrap the value's input) and added behind the
 * terminal cost.  One float32 table of 32 * DS + 1121 values,
 *     W1[32][DS], b1[32], W2[32][32], b2[32], w3[32], b3[1]
 * with unused parts zero (narrower layers; W2 and b2 with one hidden layer).  hidden_layers (1 or 2) and activation
 * (MPPI_MLP_RELU / MPPI_MLP_TANH) are the value's own, independent of the dynamics network's.  In fp32, every sum in ascending
 * index order and, at "math" = 0, every a * b + c rounded on its own:
 *     z1[j] = b1[j] + sum_i W1[j][i] * s[i];  h1 = act(z1)
 *     z2[j] = b2[j] + sum_i W2[j][i] * h1[i]; h2 = act(z2)          (two hidden layers)
 *     V = b3 + sum_j w3[j] * h2[j]                                   (one hidden layer: h1[j])
 *     terminal = quad_T + (weight * V)        quad_T: the terminal cost as it is without a value (row T - 1 of a reference)
 *     terminal = weight * V                   with replace_terminal = 1
 * Every kernel that evaluates the model's cost carries it (the same ones as the tracking cost, in the same instantiations); the
 * batch-1 rollout, the re-rolled trajectories and mppi_model_step compute states only.  Without a value nothing changes.
 *   mppi_set_mlp_value  table_host = NULL clears the value.  Otherwise checked like mppi_set_mlp (a learned-dynamics handle, the
 *                        exact count, 1 or 2 layers, a known activation, every value and the weight finite: else
 *                        MPPI_E_INVALID), staged and copied on `stream` without a host wait.
 *   mppi_get_mlp_value  the count (0: no value), layers, activation, weight and replace flag, and the table unless `out` is NULL
 *                        (waits for `stream`).
 * mppi_clone_state carries the table, the flags and the weight. */
int mppi_set_mlp_value(mppi_handle_t h, const float* table_host, int n_floats, int hidden_layers, int activation, float weight,
                       int replace_terminal, void* stream);
int mppi_get_mlp_value(mppi_handle_t h, float* out, int* n_floats_out, int* hidden_layers_out, int* activation_out,
                       float* weight_out, int* replace_terminal_out, void* stream);
/* Moving obstacles for MPPI_MODEL_NAV2D_DISCS (dynamics, parameters and maps of MPPI_MODEL_NAV2D): the predicted discs as a
 * table with one row per horizon step, discs [rows][n][4] = {cx, cy, r2, w}: centre, SQUARED radius (formed by the caller)
 * and penalty of disc j at step t; rows >= T, 0 <= n <= MPPI_MAX_DISCS.  Stage cost of step t, on the state (x, y, .) the
 * step starts from (info["t"] = t reads row t), in fp32:
 *     base = nav2d's cost (goal distance + QO * occupancy, the same lookups)
 *     pen = 0; for j = 0..n-1 (in this order): dx = x - cx, dy = y - cy; d2 = dx*dx + dy*dy; pen = pen + (d2 <= r2 ? w : 0)
 *     cost = base + pen
 * At option "math" = 0 every operation rounds on its own (two products and one add); the fast levels form
 * d2 = fma(dx, dx, dy*dy).  Overlapping discs add up; with n = 0 or no disc hit the cost is nav2d's bit for bit.
 * The TERMINAL cost reads row T-1, not a row T: the reference evaluates its terminal cost with the stale info["t"] = T-1
 * (mppi.py:318-328), the rule the racing model's reference row follows too.  A predictor that wants the discs of the
 * moment the last state is reached has no row for it.
 * mppi_set_discs pads n -> 8 (unused slots: r2 = -1, w = 0) into a buffer the handle owns, in stream order and without a
 * host wait: a host table (on_device = 0) is checked (finite, w >= 0), staged and copied like mppi_set_reference's window;
 * a device table (on_device != 0) is padded by one small kernel, so an obstacle predictor on the device never meets the
 * host — and is NOT checked (that would need a host wait): the predictor keeps its values finite and w >= 0.  A horizon whose
 * T rows (128 B each) do not fit in a block's LDS is refused at solve time (MPPI_E_INVALID).  The buffer (the handle's one step table, at least T + 1 rows from the first call on) grows, blocking on the set-up path, only when `rows` exceeds what it holds, and keeps the rows it held.  The table may be replaced
 * before every solve; re-rolls of an earlier solve (get_top_samples, a lazily completed state sequence) need the dynamics
 * only and are not affected.  MPPI_E_INVALID for another model's handle, n outside 0..8, rows < 1; solves without a table
 * or with fewer rows than the horizon return MPPI_E_STATE.  mppi_clone_state copies the table.
 * mppi_get_discs returns the PADDED table [rows][8][4] (out may be NULL to query rows and n only); host copies synchronise.
 *
 * MPPI_MODEL_RACING_DISCS (dynamics, parameters, maps, entry rules and reference window of MPPI_MODEL_RACING): the same
 * table, the same calls and the same row rule on top of racing's cost — opponent cars as discs.  In fp32:
 *     base = racing's cost ((path + velocity + obstacle + input), racing's operations in racing's order)
 *     pen  = as above, on the state (x, y, ., .) the step starts from
 *     cost = base + pen                     (added last; the stage costs are summed sequentially in fp32, like racing's)
 * With n = 0 or no disc hit the cost is racing's bit for bit.  Reference row and disc row of step t are row t of their
 * tables, the terminal cost reads row T-1 of both.  The handle keeps ONE step table [rows][40]: floats 0-7 of a row are the
 * reference row (x, y, yaw, v, sin yaw, cos yaw, 0, 0), floats 8-39 its eight padded discs.  It has two writers, each of which
 * writes its floats only, in stream order, in either order and as often as it likes without the other (the racing tick
 * rewrites the window every tick while the discs may stay): mppi_set_reference / mppi_ref_window write floats 0-7,
 * mppi_set_discs floats 8-39; mppi_get_reference and mppi_get_discs return each part as for the single-part models.  A solve
 * returns MPPI_E_STATE until BOTH parts are present with at least T rows each.  mppi_clone_state copies both parts and the
 * count.  On a plain MPPI_MODEL_RACING handle mppi_set_discs / mppi_get_discs stay MPPI_E_INVALID and the window keeps its
 * [rows][8] layout, byte for byte.  mppi_model_step takes the id and runs racing's dynamics (the discs are cost only). */
int mppi_set_discs(mppi_handle_t h, const float* discs, int rows, int n, int on_device, void* stream);
int mppi_get_discs(mppi_handle_t h, float* out, int* rows_out, int* n_out, int on_device, void* stream);
/* Soft moving discs: MPPI_MODEL_NAV2D_DISCS_SOFT / MPPI_MODEL_RACING_DISCS_SOFT are the two disc models above — same
 * dynamics, parameters, maps, entry rules, reference window, step table and mppi_set_discs / mppi_get_discs — with a graded
 * penalty SKIRT round every disc instead of the bare indicator.  Two launch-uniform numbers per handle describe it:
 *     reach  rho, finite and > 1: the skirt ends at rho * r from the centre;
 *     skirt  phi in [0, 1]: just outside the rim the penalty is phi * w (phi = 1: continuous; phi < 1: a collision stays
 *            categorically worse than a near miss).
 * With kappa = rho^2 the library forms two fp32 coefficients in double and rounds each once:
 *     a = fl32(phi * kappa / (kappa - 1)),  b = fl32(phi / (kappa - 1))
 * and charges disc j = 0..n-1 of row t in slot order.  At option "math" = 0 every operation rounds on its own, with the IEEE
 * quotient:
 *     dx = x - cx; dy = y - cy; d2 = dx*dx + dy*dy; q = d2 / r2; ramp = max(a - b*q, 0)
 *     f = (d2 <= r2) ? 1 : ramp;  pen = pen + w*f
 * The fast levels spell every fused operation out (every copy of the horizon loop forms the same bits):
 *     d2 = fma(dx, dx, dy*dy); q = d2 * rcp(r2); ramp = max(fma(-b, q, a), 0); f = (d2 <= r2) ? 1 : ramp; pen = fma(w, f, pen)
 * with rcp(r2) one v_rcp_f32 (1 ulp) on the device.  cost = base + pen, added last, as for the hard models.  The penalty is
 * linear in d2 (not in d) from phi * w at the rim to 0 at d = rho * r, and w inside: the inside test is the hard rule's own
 * compare, so with phi = 0 (a = b = 0) a soft model equals its hard model bit for bit at every math level.  Overlapping
 * discs add up, padded slots are never reached, the terminal cost reads row T-1.  One (rho, phi) per handle, not per disc.
 * On a soft handle mppi_set_discs also refuses a HOST table with r2 <= 0 in a real disc (MPPI_E_INVALID: the rule divides
 * by r2); a device table is trusted as it is.
 * mppi_set_disc_softness completes a lazily completed state sequence first and takes effect for the next launch; a soft
 * handle starts at reach = 2, skirt = 1.  MPPI_E_INVALID on a handle of any other model, for reach not finite or <= 1 and
 * for skirt outside [0, 1] or NaN.  mppi_get_disc_softness returns the pair as it was set (either pointer may be NULL).
 * mppi_clone_state carries the pair.  mppi_model_step takes the two ids and runs nav2d's / racing's dynamics. */
int mppi_set_disc_softness(mppi_handle_t h, float reach, float skirt);
int mppi_get_disc_softness(mppi_handle_t h, float* reach, float* skirt);

/* The racing control tick without the host (example/racing.py:73-81,161-218,221-266).
 *   mppi_set_center_path  `env.racing_center_path` [n][3] = (x, y, yaw) and the constants of
 *                         calc_ref_trajectory(horizon, DL, lookahead_distance, reference_path_interval): dind_host [rows]
 *                         = int(round(travel_i / DL)) for the rows = T+1 window rows (:201-205; float64 arithmetic of
 *                         the caller), v_target = env.V_MAX (:209).  Resets nothing else; synchronises (set-up path).
 *   mppi_ref_window       calc_ref_trajectory(state, path, cind, ...) as one kernel on `stream`: nearest centre-line
 *                         point (first minimum of the fp32 hypot, :189-196), ind = max(cind, ind) (:198) with the index
 *                         kept in device memory, window rows gathered straight into the model's reference table — the
 *                         same values mppi_set_reference would have uploaded, bit for bit.  state_dev [>= 2] device
 *                         pointer, or NULL for the state bound to the handle.  No host synchronisation.
 *   mppi_set/get_path_index  `racing_controller.current_path_index` (both synchronise the stream).
 *   mppi_get_reference    the current window as `reference_path` [rows][4] (device or host copy; host copies synchronise). */
int mppi_set_center_path(mppi_handle_t h, const float* path_host, int n, const int32_t* dind_host, int rows,
                         float v_target);
int mppi_ref_window(mppi_handle_t h, const float* state_dev, void* stream);
int mppi_set_path_index(mppi_handle_t h, int32_t cind, void* stream);
int mppi_get_path_index(mppi_handle_t h, int32_t* cind_out_host, void* stream);
int mppi_get_reference(mppi_handle_t h, float* ref_out, int rows, int on_device, void* stream);
/* `env.step(u)` of the shipped environments (src/envs/racing_env.py:142-163, src/envs/navigation_2d.py step) as one
 * launch, no handle needed: next = dynamics(state, clamp(u, u_min, u_max)) for native model `model` with the library
 * math in the reference's operation order; params_host = the model's MPPI_*P_* vector (cost weights may be omitted);
 * u_min_host / u_max_host [dim_control] or NULL (no pre-clamp); state_dev and next_state_dev may alias.  With
 * reached_out_dev != NULL also the goal test: *reached = norm(next[:2] - goal_xy_host) < goal_threshold (one byte). */
int mppi_model_step(int model, const float* params_host, int n_params, const float* u_min_host, const float* u_max_host,
                    const float* state_dev, const float* action_dev, float* next_state_dev, const float* goal_xy_host,
                    float goal_threshold, uint8_t* reached_out_dev, void* stream);
/* `ObstacleMap.compute_cost` / `LaneMap.compute_cost` (src/envs/obstacle_map_2d.py:168-200, src/envs/lane_map_2d.py:90-122)
 * as one launch, no handle needed — what `env.collision_check` of the examples' loops and cost plugins on the generic path
 * call: out_dev[i] = map_dev[ix][iy] with (ix, iy) = round_half_even(xy / cell_size + origin) (fp32, the reference's
 * operation order) when that lies inside the nx x ny grid (row-major float map), else 1.  Point i is the two floats at
 * xy_dev + i * stride (stride >= 2: e.g. 3 for the x, y of [x, y, theta] state rows). */
int mppi_grid_lookup(const float* map_dev, int nx, int ny, float cell_size, float origin_x, float origin_y, const float* xy_dev,
                     int64_t n, int64_t stride, float* out_dev, void* stream);

/* `_previous_action_seq` (mppi.py:157,255,452).  on_device != 0: pointer is a device pointer. */
int mppi_set_mean(mppi_handle_t h, const float* mean, int on_device, void* stream);
int mppi_get_mean(mppi_handle_t h, float* mean_out, int on_device, void* stream);
/* forward(state) argument (mppi.py:247-253), dim_state floats (copied). */
int mppi_set_state(mppi_handle_t h, const float* x0, int on_device, void* stream);
/* Zero-copy variant: the kernels of THIS solve (mppi_rollout_cost, mppi_finalize) read the state from the caller's
 * device buffer, which must stay valid and unmodified until that enqueued work ran.  mppi_rollout_cost snapshots the
 * state into the handle, and every later re-roll of that solve's samples (mppi_rollout_samples, mppi_top_samples,
 * mppi_rollout_candidates) starts from the snapshot — like the reference, whose `_state_seq_batch` is stored
 * (mppi.py:280-286,481) — so the caller may reuse or overwrite its buffer once the solve's kernels ran. */
int mppi_bind_state(mppi_handle_t h, const float* x0_dev);

/* Step 1 — `_noise_distribution.rsample` (mppi.py:261-263): eps ~ N(0, diag(sigma^2)) from the
 * device Philox4x32-10 stream, counter = (global sample index, float4 group, solve_idx): results
 * do not depend on how num_samples is sharded.  With option "noise_regen" = 1 (default) this only
 * fixes the identity of the solve's noise: the rollout and reduction kernels regenerate it in
 * registers and it is written to HBM only when an entry point needs the tiles
 * (mppi_export_noise, mppi_rollout_samples); with "noise_regen" = 0 the tiles are written here and
 * read back by both consumers (same values bit for bit). */
int mppi_sample(mppi_handle_t h, uint32_t solve_idx, void* stream);
/* Parity mode: load externally drawn noise eps[N][T][dc] (reference layout, device pointer)
 * into the tiled buffer (replaces mppi_sample for that solve). */
int mppi_inject_noise(mppi_handle_t h, const float* eps_dev, void* stream);
/* `_action_noises` / `_perturbed_action_seqs` attributes (mppi.py:261-275) in the reference
 * layout [N][T][dc]; either output may be NULL. */
int mppi_export_noise(mppi_handle_t h, float* eps_out_dev, float* actions_out_dev, void* stream);

/* Steps 1b-3 — clamp(mean + eps) (mppi.py:266-275), the N x T dynamics rollout
 * (mppi.py:280-286) and stage + terminal costs (mppi.py:291-336), fused; writes costs[N] and the
 * shard's minimum cost. */
int mppi_rollout_cost(mppi_handle_t h, void* stream);
/* `costs` (mppi.py:333-336) -> dst[N] (device or host).  Host copies synchronise. */
int mppi_get_costs(mppi_handle_t h, float* dst, int on_device, void* stream);
/* Overwrite costs[N] (used by tests and by the generic-callable path). */
int mppi_set_costs(mppi_handle_t h, const float* src, int on_device, void* stream);

/* Steps 5-6 — softmax(-costs/lambda) and sum_i w_i U_i (mppi.py:376-384), un-normalised:
 * writes the shard summary {min c, sum e, sum e^2, sum e*c, A[T*dc] = sum e_i*U_i} with
 * e_i = exp((-c_i)/lambda - max_j (-c_j)/lambda) over THIS shard.  summary_out_dev may be NULL
 * (the handle keeps its own copy). */
int mppi_weights_reduce(mppi_handle_t h, float lambda /* > 0, or MPPI_LAMBDA_DEVICE */, float* summary_out_dev,
                        void* stream);
/* Combine `num_shards` summaries (device array [num_shards][MPPI_SUMMARY_HEAD + T*dc]; NULL = this
 * handle's own, num_shards = 1 — or, with option "exchange_p2p", the summaries of all ranks from the
 * peer-to-peer buffer), form action_seq = A / sum e (mppi.py:381-385), optionally store it
 * as the next warm start (mppi.py:452), and roll it out with batch 1 (mppi.py:448-449,508-524).
 * action_out_dev [T][dc], state_seq_out_dev [T+1][ds], stats_out_dev [4] = {min c, sum e, sum e^2,
 * sum e*c} (global); any output may be NULL. */
int mppi_finalize(mppi_handle_t h, const float* summaries_dev, int num_shards, float lambda, int store_mean,
                  float* action_out_dev, float* state_seq_out_dev, float* stats_out_dev, void* stream);
/* `lambda_` = "ESSPS" | "LBPS" | "MPO" (mppi.py:183-210): the rule mppi_solve runs ON THE DEVICE when it is called with
 * lambda = MPPI_LAMBDA_DEVICE.  param = essps_target_ess (ESSPS), lbps_delta (LBPS), unused (MPO: see mppi_mpo_reset);
 * [lam_min, lam_max] = `lambda_min`, `lambda_max` (ESSPS, LBPS). */
enum { MPPI_AUTO_NONE = 0, MPPI_AUTO_ESSPS = 1, MPPI_AUTO_LBPS = 2, MPPI_AUTO_MPO = 3 };
int mppi_set_auto_lambda(mppi_handle_t h, int rule, double param, double lam_min, double lam_max);
/* MPPI.forward() of a native model in one call (mppi.py:223-460) = mppi_bind_state (x0_dev != NULL; NULL keeps the state
 * already set) + mppi_sample(solve_idx) + mppi_rollout_cost + [lambda == MPPI_LAMBDA_DEVICE: the configured rule —
 * mppi_essps_lambda_device / mppi_lbps_lambda_device before the weights, mppi_mpo_step_device after mppi_finalize] +
 * mppi_weights_reduce(lambda) + mppi_finalize(own summary — or all shards' with option "exchange_comm" /
 * "exchange_p2p" — store_mean = 1).  Same kernels and results as the individual calls; one host -> library transition
 * per solve and no host synchronisation for any temperature rule. */
int mppi_solve(mppi_handle_t h, const float* x0_dev, uint32_t solve_idx, float lambda, float* action_out_dev,
               float* state_seq_out_dev, float* stats_out_dev, void* stream);
/* Covariance adaptation of the sampling noise — the capability the reference sketches, commented out, at mppi.py:400-418
 * (after https://arxiv.org/abs/2104.00241): after the weights of a solve the diagonal covariance
 *   var[t][k] = sum_i w_i * (U_i[t][k] - ubar[t][k])^2,   w_i = e_i / sum e (the weights of mppi_weights_reduce, same fp32
 *   expression), U_i = the clamped perturbed actions of that solve (exploration samples included), ubar = A / sum e (the
 *   weighted mean of mppi.py:381-385, before the Savitzky-Golay step)
 * moves a per-step table of standard deviations s[T][dc], from which the NEXT solve draws eps[i][t][k] = z * s[t][k] (z: the
 * Philox / Box-Muller normal every solve draws; only the factor changes):
 *   s^2[t][k] <- (1 - rate) * s^2[t][k] + rate * (var[t][k] + floor),   then s clamped into [sigma_min[k], sigma_max[k]].
 * rate = 1, floor = 1e-6 (`small_cov`, mppi.py:408-411), no clamp is the sketch, literally.  Off by default: nothing changes
 * for a handle that never switches it on.  While it is on the noise is always materialised as tiles (the handle behaves like
 * "noise_regen" = 0 whatever the option says; the single launch of small problems regenerates noise, so mppi_solve takes
 * the multi-kernel sequence) and mppi_sample_posterior draws with the table too (mppi.py:416-418: `_noise_distribution`
 * follows the covariance).  Not available for sharded handles (options "exchange_p2p" / "exchange_comm": the variance would
 * need a second exchange).
 *   mppi_set_covariance_adaptation  mppi.py:400-418 on / off with 0 <= rate <= 1, floor >= 0 and the clamp
 *                         sigma_min_host / sigma_max_host [dim_control] (NULL: 0 / +inf).  Leaves the table as it is.
 *                         Set-up path: synchronises.
 *   mppi_update_covariance  mppi.py:402-411 for the solve in flight, as two launches on `stream` (the weighted second moment
 *                         over the live tiles as per-block partial rows; their fold in a fixed order and the update: no
 *                         atomics, the table is bit-reproducible).  Call it BETWEEN mppi_weights_reduce and mppi_finalize,
 *                         with the same lambda: it needs the mean that solve sampled around, which mppi_finalize
 *                         replaces.  mppi_solve does so itself while the adaptation is on.  A voided solve (NaN weights
 *                         after a temperature search that timed out) leaves the table unchanged.
 *   mppi_get_sigma_table / mppi_set_sigma_table  the table (`_covariance` of mppi.py:411 as standard deviations) as [T][dc]
 *                         floats, device or host; filled from `sigmas` by mppi_create / mppi_set_control_limits, copied by
 *                         mppi_clone_state with the settings.  Host copies out synchronise. */
int mppi_set_covariance_adaptation(mppi_handle_t h, int enable, float rate, float floor, const float* sigma_min_host,
                                   const float* sigma_max_host);
int mppi_update_covariance(mppi_handle_t h, float lambda /* > 0, or MPPI_LAMBDA_DEVICE */, void* stream);
int mppi_get_sigma_table(mppi_handle_t h, float* table_out, int on_device, void* stream);
int mppi_set_sigma_table(mppi_handle_t h, const float* table, int on_device, void* stream);
/* The control-cost term — the `action_costs` the reference fills on every solve at mppi.py:294-316 and leaves out of the
 * cost sum at :330-336 (the KL term of the MPPI objective).  Opt-in; off, nothing changes and nothing else is launched.
 * For sample i of a solve that samples around the warm start mean[T][dc] (fp32, one rounding per operation, no FMA):
 *     inv[t][k] = 0 for t = 0 (the reference fills rows 1..T-1 only), 1 / (s[t][k] * s[t][k]) for t >= 1
 *                 (s: `sigmas`, or the per-step sigma table while the covariance adaptation is on)
 *     g[t][k]   = mean[t][k] * inv[t][k]
 *     A_i       = sum over t = 0..T-1, k = 0..dc-1, in this order, of g[t][k] * U_i[t][k]
 *     cost_i    = c0_i + kappa * A_i,  kappa = weight * lambda
 * U_i is the solver-clamped perturbed action; `mean` is the real warm start for EVERY sample, the exploration samples
 * (which do not inherit it when sampling) included (mppi.py:313); c0_i is the stage + terminal cost.  Everything after
 * the rollout (minimum, temperature rules, weights, queries, mppi_get_costs) sees cost_i.
 *   mppi_set_action_cost  on / off with weight >= 0 (1 = the reference's sketch; the paper scales the term by 1 - alpha).
 *                         Needs every sigma > 0.  Leaves everything else alone; allowed between solves.  While on:
 *                         native models roll out with the term inside rollout_cost (instantiations of their own),
 *                         mppi_solve takes the multi-kernel sequence (mppi_fused_geometry reports 0 / 0) and option
 *                         "mapping" = 1 returns MPPI_E_INVALID.  Copied by mppi_clone_state.
 *   mppi_set_action_cost_lambda  the lambda of the term for mppi_rollout_cost, which has no lambda argument: a value >= 0
 *                         (0: the term is zero), or MPPI_LAMBDA_DEVICE — the temperature in the handle's device memory
 *                         WHEN THE ROLLOUT STARTS (the previous solve's ESSPS / LBPS result, the MPO dual's current
 *                         temperature); kappa = 0 while no device-resident rule has left one.  Stays until set again.
 *                         mppi_solve sets it from its own lambda argument on every call.
 *   mppi_add_action_cost  costs[i] += weight * lambda * A_i as a pass of its own over the noise tiles (materialised first if
 *                         need be) around the CURRENT mean, then the minimum key is refreshed as by mppi_set_costs.  The
 *                         generic path's way to the term (after mppi_set_costs, before mppi_weights_reduce; any
 *                         dim_control); on a native handle a second, independent evaluation: same bits as the rollout's. */
int mppi_set_action_cost(mppi_handle_t h, int enable, float weight);
int mppi_set_action_cost_lambda(mppi_handle_t h, float lambda /* >= 0, or MPPI_LAMBDA_DEVICE */);
int mppi_add_action_cost(mppi_handle_t h, float lambda /* >= 0, or MPPI_LAMBDA_DEVICE */, void* stream);
/* Temporally correlated sampling noise — an AR(1) filter along the horizon (the colored noise of iCEM and of the
 * low-frequency-sampling MPPI variants; the reference draws independent steps).  Opt-in; off, nothing changes and nothing else
 * is launched.  For sample i and control dimension k, with xi[t] the standard normal every solve draws for (i, t, k) (Philox /
 * Box-Muller, counter (global sample index, float4 group, solve index): the filtered and the unfiltered stream of one seed
 * consume the same normals), in fp32 with one rounding per operation:
 *     z[0] = xi[0],   z[t] = beta[k] * z[t-1] + alpha[k] * xi[t]  (t = 1..T-1),   alpha[k] = (float)sqrt(1 - (double)beta[k]^2)
 *     eps[i][t][k] = z[t] * s[t][k]     (s: `sigmas`, or the per-step sigma table while the covariance adaptation is on)
 * The start is stationary and the scale comes after the filter: every step keeps the marginal standard deviation s[t][k], the
 * lag-1 correlation is beta[k].  Exploration samples are filtered like the others; the filter never crosses samples, so
 * sharded handles draw the rows of the unsharded solve.  While it is on the noise is always materialised as tiles, by
 * sample_colored_kernel (the handle behaves like "noise_regen" = 0 whatever the option says, exactly as under the covariance
 * adaptation: mppi_solve takes the multi-kernel sequence and mppi_fused_geometry reports 0 / 0; candidates of other shards
 * cannot be re-rolled) and mppi_sample_posterior draws through the same filter.  Injected noise (mppi_inject_noise) is taken
 * as it is.
 *   mppi_set_noise_correlation  beta_host [dim_control], each in [0, 1) (else MPPI_E_INVALID); NULL or all zero: off.  Allowed
 *                         between solves; noise tiles that were not injected are dropped.  MPPI_E_STATE before
 *                         mppi_set_control_limits where that call is required.  Copied by mppi_clone_state.  Set-up path:
 *                         synchronises.
 *   mppi_get_noise_correlation  the current beta [dim_control] (zeros while off). */
int mppi_set_noise_correlation(mppi_handle_t h, const float* beta_host /* [dim_control]; NULL or all zero: off */);
int mppi_get_noise_correlation(mppi_handle_t h, float* beta_out_host);
/* Risk-aware solves: every sample is rolled out from a SET of start states ("particles": a filter's particles, draws from a
 * mean and a covariance) and its P costs are folded into one by a risk measure.  Opt-in; with no particles set nothing changes,
 * bit for bit, and nothing else is launched.  The noise identity of a sample, (seed, solve, i, t, k), does not depend on the
 * start state: the cost of particle m for sample i is what a plain handle computes from x0 = particles[m] with the same seed,
 * solve index and mean — the same lane_cost, decided per particle (a start outside the position clamp, racing's unit wheel
 * base, the library-math redo of a lane that left a fast path).
 *   mppi_set_particles   particles [P][dim_state] fp32, 0 <= P <= MPPI_MAX_PARTICLES; P = 0 or a null pointer switches the
 *                        feature off.  A host table (on_device = 0) is checked for finite values, staged and copied in stream
 *                        order with no host wait, like mppi_set_reference's window; a device table is copied device-to-device
 *                        on `stream` and trusted.  May be called before every solve.  A pending lazily completed state
 *                        sequence is completed first (the particle launch does not carry the rider block).  The [P][N] cost
 *                        matrix is allocated on first use and grows, blocking, on this set-up path only.  A generic handle
 *                        accepts the call and only records P (for mppi_set_particle_costs).  MPPI_E_INVALID with option
 *                        "mapping" = 1 (and that option is refused while particles are set).
 *   mppi_get_particles   the table (out may be NULL to query P only); host copies synchronise.
 *   mppi_set_risk        mode = MPPI_RISK_MEAN (default) | MPPI_RISK_WORST | MPPI_RISK_CVAR, k = the number of worst particles
 *                        averaged under CVAR.  k is checked against P where the fold is launched (under CVAR: MPPI_E_INVALID
 *                        for k < 1 or k > P), so either call may come first.
 *   mppi_get_particle_costs  the [P][N] matrix of the last rollout (row m: the costs from particle m).
 *   mppi_set_particle_costs  replaces the matrix and folds it: for the matrix what mppi_set_costs is for the vector (tests, and
 *                        the generic path: one pass of the user's loops per particle); the minimum key is the fold's.
 * The fold, for sample i with c[m] the cost from particle m — every operation rounds on its own in fp32 at every math level,
 * the division is the IEEE quotient:
 *     MEAN     a = c[0]; for m = 1..P-1: a = a + c[m];            cost = a / (float)P
 *     WORST    cost = max over m of c[m]
 *     CVAR(k)  c_(0) >= c_(1) >= ... the c[m] from largest to smallest (ties are interchangeable);
 *              a = c_(0); for j = 1..k-1: a = a + c_(j);          cost = a / (float)k
 * With P = 1 every mode returns c[0] unchanged (x / 1.0f).  CVAR(P) is the descending-order mean: the same set of addends as
 * MEAN in another order, so the two need not agree to the bit.  A NaN among the c[m] makes the folded cost NaN in every mode
 * (the ordering network would otherwise drop it); the minimum key then treats it as the plain rollout treats a NaN cost.
 * One kernel, particle_fold_kernel: a lane per sample (at most 1024 blocks, which stride over larger problems), the P values of
 * a sample in registers, a fixed compare-exchange network; it writes costs[i] and accumulates the shard minimum into the
 * double-buffered minimum key exactly as the rollout does (no memset).
 * While particles are set:
 *   mppi_rollout_cost    launches rollout_particles_kernel — a wave walks one tile from one particle, grid ceil(tiles/4) x P —
 *                        and then the fold.  Everything downstream (minimum, temperature rules, weights, queries,
 *                        mppi_get_costs, the covariance adaptation) sees the folded cost.  The snapshots a rollout takes are
 *                        the NOMINAL state (mppi_set_state / mppi_bind_state) and the mean: later re-rolls (mppi_top_samples,
 *                        mppi_rollout_samples) and mppi_finalize's state sequence start from the nominal state — the particles
 *                        decide costs only.  Regenerated noise and materialised tiles (colored noise, covariance adaptation,
 *                        injected noise) both work.  The control-cost term does not depend on the state: with
 *                        mppi_set_action_cost on, the particle rollout runs WITHOUT it and mppi_add_action_cost adds
 *                        kappa * A_i once, AFTER the fold (fold first, then the term: cost_i = fold_i + kappa * A_i).
 *   mppi_solve           takes the multi-kernel sequence; mppi_fused_geometry reports 0 / 0.
 *   sharded handles      need nothing new (costs are local to a shard); every rank must be given the same particles.
 * mppi_clone_state copies the table, P, the mode, k and the last matrix.  Stage 1 of mppi_get_timing covers the rollout plus the
 * fold (events on the two dispatches). */
#define MPPI_MAX_PARTICLES 16
enum { MPPI_RISK_MEAN = 0, MPPI_RISK_WORST = 1, MPPI_RISK_CVAR = 2 };
int mppi_set_particles(mppi_handle_t h, const float* particles, int P, int on_device, void* stream);
int mppi_get_particles(mppi_handle_t h, float* out, int* P_out, int on_device, void* stream);
int mppi_set_risk(mppi_handle_t h, int mode, int k);
int mppi_get_risk(mppi_handle_t h, int* mode_out, int* k_out);
int mppi_get_particle_costs(mppi_handle_t h, float* out /* [P][N] */, int on_device, void* stream);
int mppi_set_particle_costs(mppi_handle_t h, const float* src /* [P][N] */, int on_device, void* stream);
/* The map from particle to ensemble member (the MPPI_MODEL_MLP* ids with mppi_set_mlp_ensemble): members[P], particle m is
 * rolled out through member members[m]; NULL or P = 0: no map (every particle through the nominal member — the launch is
 * exactly the one without this feature).  Either this call or mppi_set_particles may come first: the rollout checks, before
 * anything is launched, that the map's length is the particle count and that every entry is < E (else MPPI_E_INVALID).
 * Switching the particles off (mppi_set_particles with P = 0) drops the map.  MPPI_E_INVALID for a map on a handle of another
 * model, P > MPPI_MAX_PARTICLES or a negative entry.  The block of particle m reads its entry — the member's offset into the
 * table buffer, staged on the device in stream order by the rollout that first uses the map — at a block-uniform address and
 * moves its copy of the table pointer: the weights still arrive as scalar operands.  Everything behind the rollout (the fold,
 * the minimum key, the control-cost term behind the fold, the temperature rules, sharding, both noise paths) is what it is
 * for particles.  Sharded handles: every rank must be given the same map.  mppi_clone_state copies it.
 *   mppi_get_particle_members  the map (out may be NULL to query its length only; 0: none). */
int mppi_set_particle_members(mppi_handle_t h, const int* members /* [P] */, int P);
int mppi_get_particle_members(mppi_handle_t h, int* out /* [P] */, int* P_out);
/* Lazily completed state sequences (mppi_set_option("lazy_state_seq", 1)).  The reference returns `state_seq` — the batch-1
 * rollout of the solution, mppi.py:448-449,508-524 — with the action sequence, but nothing on a control loop's critical
 * path needs it: the next solve samples around the mean, env.step applies a[0].  With the option set, mppi_finalize /
 * mppi_solve of a native model on the multi-kernel path leave those T dependent steps out of the solve's last kernel; the
 * rollout (same code, same bits) then rides in one extra block of the NEXT mppi_rollout_cost / mppi_solve launch on that
 * stream — hidden behind its N-sample rollout — or, when somebody wants the state sequence before that, runs as a one-wave
 * kernel of its own: a reader of state_seq_out_dev calls mppi_join_state_seq(h, serial, its stream) first (no-op when
 * nothing is pending; the single launch of small problems always rolls out itself).  state_seq_out_dev must stay valid
 * until then.  mppi_state_seq_serial: the number of the last mppi_finalize and whether its state sequence is pending;
 * handing that number to mppi_join_state_seq makes a reader of an OLDER solve's sequence launch nothing. */
int mppi_join_state_seq(mppi_handle_t h, uint32_t serial /* 0 = whatever is pending */, void* stream);
int mppi_state_seq_serial(mppi_handle_t h, uint32_t* serial_out, int* pending_out);
/* out2_host = {mean device time of the stand-alone state-sequence kernel [ms] (-1: none), launches} since the last call
 * (option "timing" = 1). */
int mppi_get_state_seq_timing(mppi_handle_t h, float* out2_host);
/* mppi_solve as a SINGLE LAUNCH.  For small problems (option "fused_solve" = 1, the default: num_samples <= 4096, the
 * sizes of the reference's examples; <= 16 384 under a device-resident ESSPS / LBPS search) whose noise is regenerated in
 * registers, with T*dim_control <= 128 and no sharding, mppi_solve runs ONE cooperative kernel instead of 3-9 dependent
 * launches: min(#CUs, ceil(N/64)) blocks of 512 threads (at most 32 of them up to 4096 samples) exchange the partial sums
 * of the temperature search and their partial weighted rows through 8-byte {value, solve number} cells in HBM (relaxed
 * agent-scope stores, polled); with up to 32 blocks every block runs the search's scalar step itself and no hop is spent
 * on the global minimum (a block's sums are relative to its own minimum and rescaled where they are added), beyond
 * block 0 does and broadcasts; block 0 runs the tail of the solve.  Costs and minimum are bit-identical to the
 * multi-kernel path; temperature, action and state sequences equal to rounding (another summation partition).
 * "fused_solve" = 0 keeps the multi-kernel path, = 2 takes the single launch whenever every block can be resident at once
 * (num_samples <= 512 x #CUs = 131 072; measured on par or slower than the multi-kernel path beyond the defaults above:
 * a cell round trip costs what a kernel boundary costs).  Co-residency of the blocks is checked against the kernel's own
 * occupancy before every launch configuration is used (hipOccupancyMaxActiveBlocksPerMultiprocessor x #CUs; a grid that
 * does not fit takes the multi-kernel path in the same call); what other work holds of the device at run time cannot be
 * known at launch, so a poll that cannot complete within 20 ms (option "fused_timeout_us": 100 us .. 60 s, for a GPU that is
 * shared or preempted for longer) gives up: that solve returns the PREVIOUS plan (the warm start it sampled around,
 * unchanged, and its rollout from the current state — never NaN, never a partial combine), the statistics of THAT solve
 * are NaN (the `stats_out` of that call: the stale plan is visible in the solve it happened in), the flag below is
 * raised and the handle stays on the multi-kernel path until mppi_set_option("fused_rearm", 1).  It never hangs. */
int mppi_fused_error(mppi_handle_t h);
/* Which geometry the last mppi_solve took: the grid and the trajectories per block (a multiple of 64, <= 512) of the single
 * launch, or 0 / 0 if that solve ran as separate kernels (option "fused_solve" = 0, a problem the single launch does not take,
 * a launch configuration declined by the occupancy check, or a handle demoted by mppi_fused_error).  Host bookkeeping only:
 * no synchronisation. */
int mppi_fused_geometry(mppi_handle_t h, int* blocks_out, int* spb_out);
/* Step 7 inside mppi_finalize (mppi.py:423-443,598-620): Savitzky-Golay smoothing of [history(T-1); a(T)] per control
 * dimension (symmetric-flip padding, valid cross-correlation, keep the last T), applied whenever mppi_finalize is
 * called with store_mean != 0; the smoothed sequence is what is returned, stored as the warm start and rolled out,
 * and its first row is shifted into the history.  coeffs_host [window] = first row of pinv(vander) (mppi.py:568-596);
 * history_host [T-1][dc] or NULL (keep / zeros).  window = 0 switches the filter off.  T*dc <= 1024. */
int mppi_set_sg_filter(mppi_handle_t h, const float* coeffs_host, int window, const float* history_host);
int mppi_get_sg_history(mppi_handle_t h, float* history_host);

/* Device half of the automatic temperature searches (`_compute_ess`, `_lbps_objective`,
 * `_essps_objective`, the MPO dual; mppi.py:341-370,387-398,526-566): softmax statistics of this
 * shard's costs for one lambda, out5_host = {min c, max c, sum e, sum e^2, sum e*c} with
 * e_i = exp((-c_i)/lambda - (-min c)/lambda).  ESS = (sum e)^2 / sum e^2, E_w[c] = sum e*c / sum e,
 * logsumexp(-c/lambda) = -min c/lambda + log(sum e).  The root-finders stay on the host.  Synchronises. */
int mppi_softmax_stats(mppi_handle_t h, float lambda, double* out5_host, void* stream);
/* The same for `count` (1..32) temperatures in ONE pass over the costs: out_host[count][3] =
 * {sum e, sum e^2, sum e*c} per lambda (each relative to this shard's min c).  Lets the ESSPS
 * bracketing search probe a whole grid of lambdas per round trip.  Synchronises. */
int mppi_softmax_stats_multi(mppi_handle_t h, const float* lambdas_host, int count, double* out_host, void* stream);
/* ESSPS (mppi.py:351-370): lambda in [lam_min, lam_max] with ESS(lambda) = target_ess (end-point rules of
 * mppi.py:361-364), searched on the host from two 32-temperature passes of mppi_softmax_stats_multi and an
 * inverse polynomial interpolation (within ~1e-7 relative of scipy's brentq on the same statistics).  From the second
 * search of a handle on, the first grid is clustered around the previous root (with the end points and a sparse cover
 * of the rest of the range); when the root is found well inside the cluster and the interpolation has visibly converged
 * there (polynomials of two orders agree to 1e-5) the search ends after ONE pass (~1e-6 relative), otherwise the
 * bracket is refined by the second grid as in a cold search.  Option "essps_cold" makes the next search cold.
 * Unsharded handles; synchronises once or twice. */
int mppi_essps_lambda(mppi_handle_t h, double target_ess, double lam_min, double lam_max, double* lambda_out_host,
                      void* stream);
/* The same search with NO host synchronisation: both statistics passes and both scalar steps (end-point rules /
 * refined grid, root interpolation) run as kernels on `stream` (the second pair returns at once when the first grid
 * was enough), the first grid of the NEXT search is left in device memory, and so is the temperature.  Pass
 * MPPI_LAMBDA_DEVICE as the `lambda` of mppi_weights_reduce / mppi_finalize to use it; mppi_get_lambda reads it back
 * (synchronises the stream).  Identical arithmetic to mppi_essps_lambda (both call csrc/host_search.hpp). */
#define MPPI_LAMBDA_DEVICE (-1.0f)
int mppi_essps_lambda_device(mppi_handle_t h, double target_ess, double lam_min, double lam_max, void* stream);
/* What the device-resident ESSPS search carries from one solve to the next (the first grid its last search left for the next
 * one, built around that search's root), as an opaque blob: for callers that save a solver and restore it in another process
 * (mppi_clone_state copies the same state between two handles).  mppi_essps_get_state: *bytes_out_host = the blob's size, 0
 * while no search has run; out_host NULL asks for the size only.  mppi_essps_set_state: a handle restored from the blob
 * searches on bit for bit like the one it was read from.  A blob of another size is refused.  Both synchronise the device. */
int mppi_essps_get_state(mppi_handle_t h, void* out_host, int64_t* bytes_out_host);
int mppi_essps_set_state(mppi_handle_t h, const void* in_host, int64_t bytes);
/* Passes over the costs the last device-resident search took (ESSPS: 1 or 2; LBPS: 2); 0 = none yet.  Synchronises. */
int mppi_search_passes(mppi_handle_t h, void* stream);
/* The temperature a device-resident rule left in HBM, and (lambda_used_out_host != NULL) the one the last solve's weights
 * used — the same value for ESSPS / LBPS, the previous one for MPO (mppi.py:387-398 updates it AFTER the weights).
 * Synchronises `stream` (pass the stream the solve was enqueued on). */
int mppi_get_lambda(mppi_handle_t h, double* lambda_out_host, double* lambda_used_out_host, void* stream);
/* LBPS (mppi.py:341-349,534-557) with NO host synchronisation: the reference's ~25 dependent Brent probes become two
 * 32-temperature grids (one pass over the costs each; the grid minimum is bracketed by the second, finer grid) and the
 * minimiser of the quartic through the five grid points around the minimum in log(lambda) — the float64 minimiser to 3e-7
 * on exact statistics; against the reference's own Brent (which stops 6e-5 .. 5e-3 away from it) within 1e-3 relative
 * wherever the objective is not flat to fp32 rounding.  The temperature stays in HBM (MPPI_LAMBDA_DEVICE). */
int mppi_lbps_lambda_device(mppi_handle_t h, double delta, double lam_min, double lam_max, void* stream);
/* LBPS exactly as the reference searches it (mppi.py:341-349: scipy.optimize.minimize_scalar(method="bounded"), ported
 * step for step in csrc/host_search.hpp) with NO host synchronisation: one launch (lbps_brent_kernel) runs all ~22-31
 * dependent probes; every probe evaluates the statistics of mppi_softmax_stats bit for bit (the same threads add the same
 * costs in the same order) and every block takes the same double-precision Brent step, so the temperature equals
 * mppi_lbps_lambda's TO THE BIT — at one hop through memory per probe instead of two launches and a read-back.  The
 * temperature stays in HBM (MPPI_LAMBDA_DEVICE; mppi_get_lambda reads it back, mppi_search_passes returns the number of
 * probes).  This is what mppi_solve runs for MPPI_AUTO_LBPS (option "lbps_search" = 1 selects the grid search above).
 * mppi_search_error: 1 once a poll of that kernel gave up (budget = option "fused_timeout_us"; a block never became
 * resident because the GPU is shared): the temperature of that solve is NaN; option "search_rearm" clears the flag. */
int mppi_lbps_brent_device(mppi_handle_t h, double delta, double lam_min, double lam_max, void* stream);
int mppi_search_error(mppi_handle_t h);
/* LBPS (mppi.py:341-349,534-557): argmin over [lam_min, lam_max] of -(E_w[-c] - (max c - min c) * sqrt((1-delta)/delta)
 * / sqrt(ESS)), searched on the host with Brent's bounded minimiser (scipy minimize_scalar(method="bounded"): xatol
 * 1e-5, at most 500 evaluations); every probe is one mppi_softmax_stats round trip.  Unsharded handles; synchronises. */
int mppi_lbps_lambda(mppi_handle_t h, double delta, double lam_min, double lam_max, double* lambda_out_host, void* stream);
/* MPO (mppi.py:191-200,387-398): the dual variable log T and its Adam moments live in the handle.
 *   mppi_mpo_reset  log T = log(lambda0), moments cleared; epsilon = the KL bound (0.1), lr = Adam step (0.2)
 *   mppi_mpo_step   one Adam step on loss = softplus(logT) * (epsilon + logsumexp(-c / softplus(logT))) over the LAST
 *                   solve's costs; *lambda_out_host = exp(logT), the temperature of the NEXT solve.  Synchronises.
 *   mppi_mpo_state  out4_host = {log T, first moment, second moment, step count}.
 *   mppi_mpo_set_state  the inverse (restoring a saved solver); the next solve's temperature becomes exp(log T). */
int mppi_mpo_reset(mppi_handle_t h, double lambda0, double epsilon, double lr);
int mppi_mpo_set_state(mppi_handle_t h, const double* in4_host);
int mppi_mpo_step(mppi_handle_t h, double* lambda_out_host, void* stream);
/* mppi_mpo_step without the read-back (no host synchronisation): the dual, its moments and the resulting temperature
 * stay in device memory; the NEXT solve's weights read it through MPPI_LAMBDA_DEVICE.  Call it after mppi_finalize. */
int mppi_mpo_step_device(mppi_handle_t h, void* stream);
int mppi_mpo_state(mppi_handle_t h, double* out4_host);
/* Device address of the dual's log T (fp32; read-only for the caller — valid until mppi_destroy): the reference keeps it as an
 * nn.Parameter (mppi.py:194-199); a binding can wrap this address instead of copying the value after every solve. */
int mppi_mpo_log_temperature_ptr(mppi_handle_t h, float** out_dev);

/* `_weights` (mppi.py:376) for this shard given the GLOBAL {min c, sum e}: w_out_dev[N]. */
int mppi_weights(mppi_handle_t h, float lambda, float cmin_global, float sum_e_global, float* w_out_dev,
                 void* stream);
/* `_states_prediction(state, action_seqs)` (mppi.py:508-524) for k action sequences actions_dev[k][T][dc] ->
 * states_out_dev[k][T+1][ds] (step 8 after host-side smoothing; get_samples_from_posterior).  x0_dev = the start
 * state [ds] (device), or NULL for the state of the current solve; an explicit state does not disturb the solver. */
int mppi_rollout_actions(mppi_handle_t h, const float* actions_dev, int k, const float* x0_dev, float* states_out_dev,
                         void* stream);
/* get_samples_from_posterior, sampling half (mppi.py:489-503): samples_out_dev[k][T][dc] = loc_dev[T][dc] + eps with
 * eps ~ N(0, diag(sigma^2)) (unclamped, like MultivariateNormal(loc).sample()) from the device Philox stream at the
 * RESERVED solve index `solve_idx` (counter = (sample, float4 group, solve_idx): the call consumes the solver's
 * stream the way the reference's draw consumes torch's generator; sharding does not change the samples). */
int mppi_sample_posterior(mppi_handle_t h, uint32_t solve_idx, const float* loc_dev, int k, float* samples_out_dev,
                          void* stream);
/* `_state_seq_batch[top_indices]` (mppi.py:481): re-roll the k local samples idx_dev[k] from the
 * resident noise instead of materialising S[N][T+1][ds] -> states_out_dev[k][T+1][ds]. */
int mppi_rollout_samples(mppi_handle_t h, const int64_t* idx_dev, int k, float* states_out_dev, void* stream);
/* get_top_samples (mppi.py:462-487) in one call: the k (any 1 <= k <= num_samples) samples of the last solve with the largest
 * weight = the smallest cost (radix select on the device), sorted by descending weight, their state
 * (k <= 1024: one block sorts the candidates in LDS; larger k: a multi-pass bitonic sort in HBM), their state
 * trajectories re-rolled around the mean that solve sampled (states_out_dev [k][T+1][ds]) and their softmax
 * weights softmax(-c/lambda)_i (weights_out_dev [k]).  lambda = the temperature of that solve, or
 * MPPI_LAMBDA_DEVICE = the one its finalize step left in device memory (no read-back: the call never waits for the
 * host).  Up to 4096 samples and k <= 1024 (the reference examples call this every tick with such sizes) the whole
 * query is ONE launch: a block builds the (cost, index) words of all samples, sorts them in LDS and re-rolls the first k.
 * On a shard this ranks the shard's own samples (weights still use the global normalisation); see the two calls below. */
int mppi_top_samples(mppi_handle_t h, int k, float lambda, float* states_out_dev, float* weights_out_dev, void* stream);
/* The two halves of mppi_top_samples for sharded solvers.  A candidate is (cost key << 32) | GLOBAL sample index; the
 * key is an order-preserving bijection of the fp32 cost, so candidates of all shards can be merged by sorting the
 * 64-bit words ascending, and — the device noise being a function of the global index — any rank can then weigh
 * and re-roll the k winners:
 *   mppi_top_candidates:     this shard's k smallest costs -> cand_out_dev[k] (unordered)
 *   mppi_rollout_candidates: k merged candidates -> states_out_dev[k][T+1][ds], weights_out_dev[k], sorted by
 *                            descending weight (needs regenerated noise: option "noise_regen" = 1, no injection). */
int mppi_top_candidates(mppi_handle_t h, int k, uint64_t* cand_out_dev, void* stream);
int mppi_rollout_candidates(mppi_handle_t h, const uint64_t* cand_dev, int k, float lambda, float* states_out_dev,
                            float* weights_out_dev, void* stream);

/* What RCCL reports for this handle's communicator (ncclCommCount, ncclCommUserRank): diagnostics for multi-GPU runs. */
int mppi_comm_info(mppi_handle_t h, int* count_out, int* rank_out);
/* In-library collective for sharded solves (variant A: one all_gather of the 4+T*dc-float shard summaries; the
 * reference has no counterpart, src/pi_mpc/mppi.py:102-105 is single-device).  One process per GPU; RCCL is dlopen()ed
 * (librccl.so.1) on first use, so unsharded callers do not need it.
 *   mppi_comm_unique_id  ncclGetUniqueId on ONE rank: id_out128 [128 bytes]; hand it to every rank by any host channel
 *   mppi_comm_init       ncclCommInitRank(world, rank, id) for this handle's device — collective over the job's ranks
 *   mppi_comm_exchange   one stand-alone all_gather (self-test): data_dev [4+T*dc] -> gathered_out_dev [world][4+T*dc];
 *                        synchronises
 *   option "exchange_comm" = 1: mppi_weights_reduce (summary_out_dev = NULL) ends with ncclAllGather on ITS OWN stream —
 *                        no process-group stream, no events — and mppi_finalize called with summaries_dev = NULL combines
 *                        all `world` shards; a sharded solve is then the same single call as an unsharded one
 *                        (mppi_solve).  Every rank must issue the same sequence of solves.
 *   mppi_comm_destroy    ncclCommDestroy (also done by mppi_destroy). */
int mppi_comm_unique_id(void* id_out128);
int mppi_comm_init(mppi_handle_t h, int world, int rank, const void* id128);
int mppi_comm_exchange(mppi_handle_t h, const float* data_dev, float* gathered_out_dev, void* stream);
int mppi_comm_destroy(mppi_handle_t h);

/* Peer-to-peer exchange of the shard summaries (one process per GPU, same node): instead of an all_gather between
 * mppi_weights_reduce and mppi_finalize, every rank stores its 4+T*dc summary straight into all peers' exchange
 * buffers (fine-grained device memory shared through HIP IPC, 8-byte {value, sequence} cells so that data and
 * readiness arrive in one store) and mppi_finalize polls its own buffer.
 *   mppi_p2p_alloc    allocate this rank's buffer, return its 64-byte IPC handle (exchange the handles of all
 *                     ranks with any host-side collective)
 *   mppi_p2p_connect  map the peers' buffers: handles_host [world][64] and the ranks' HIP device ordinals
 *                     peer_devices_host [world], both in rank order; refuses (MPPI_E_STATE) unless every peer device
 *                     is visible and hipDeviceCanAccessPeer says it is directly addressable
 *   mppi_p2p_exchange one stand-alone exchange (self-test): data_dev [4+T*dc] -> gathered_out_dev [world][4+T*dc];
 *                     MPPI_E_STATE if a poll timed out (~20 s).  Synchronises.
 *   option "exchange_p2p" = 1: mppi_weights_reduce publishes the summary to the peers, and mppi_finalize called with
 *                     summaries_dev = NULL combines all `world` shards from the buffer.  Every rank must issue the
 *                     same sequence of reduce / exchange calls.
 *   mppi_p2p_error    1 once any poll on this handle timed out (results of that solve are void). */
int mppi_p2p_alloc(mppi_handle_t h, int world, int rank, void* ipc_handle_out64);
int mppi_p2p_connect(mppi_handle_t h, const void* ipc_handles_host, const int32_t* peer_devices_host);
int mppi_p2p_exchange(mppi_handle_t h, const float* data_dev, float* gathered_out_dev, void* stream);
int mppi_p2p_error(mppi_handle_t h);

/* Tuning knobs (not in the reference): "math" 0 = library sin/cos/tan/fmod/div, 1 = range-checked polynomial
 * fast paths, 2 = 1 + the hardware sin/cos for model-bounded arguments (default); "fused_solve", "fused_timeout_us", "fused_rearm" (see mppi_fused_error);
 * "lazy_state_seq" (see mppi_join_state_seq; off by default);
 * "essps_cold" (any value): the next ESSPS search of this handle starts from the geometric grid instead of the one
 * clustered around its last root; "noise_regen" (see mppi_sample); "mapping" 0 = lane per trajectory (default), 1 =
 * the north star's literal wavefront-per-trajectory rollout (comparison only, ~20x slower); "reduce_blocks" grid of the weighted
 * reduction; "fold_path" who sums the reduction's partial rows: 0 = by the live-row count of earlier solves (default),
 * 1 = inside mppi_finalize whenever the rows fit its LDS, 2 = always the separate summarize kernel (both use the same
 * summation tree: results are bit-identical); "essps_merge0" 1 = round 0 of mppi_essps_lambda_device as one launch too
 * (statistics pass + select step; round 1 always is: it returns at once when round 0 finished the search) — same
 * temperature to the bit, measured no faster (default 0); "timing" (see mppi_get_timing). */
int mppi_set_option(mppi_handle_t h, const char* key, int64_t value);
/* The math level the NEXT rollout of this handle dispatches, into *level_out: 0 = library math and bounds-tested map lookups,
 * 1 = the range-checked fast paths (nav2d / racing: the padded-grid lookup), 2 = 1 + hardware sin/cos of the wrapped headings.
 * It is option "math" (clamped to 0..2) unless a launch-uniform precondition of the model's fast kernels does not hold — solver
 * bounds beyond the model's own action clamp, heading increments of pi or more, racing steering beyond 0.25 or a wheel base
 * whose reciprocal is unusable, a cell size with an all-ones significand, position limits that reach beyond one cell past the
 * map, racing maps of different geometry, a map or the parameters not set yet — then it is 0 whatever the option says.
 * Read-only: no setter, no device work, no change of behaviour. */
int mppi_get_math_level(mppi_handle_t h, int* level_out);
/* Device time per stage from HIP event pairs since the last drain (no host synchronisation while recording).  The
 * events ride on the stage's own dispatches: a stage time runs from the begin of its first kernel to the end of its
 * last, without the wait between a stream marker and the dispatch (a captured stream, and a stage that ends in a
 * collective, keep plain event records).  out[0..3] = mean ms of
 * {sample, rollout_cost, weights_reduce, finalize}, out[4..7] = number of calls averaged.
 * Enabled by mppi_set_option(h, "timing", 1).  Synchronises and clears the recorded pairs. */
int mppi_get_timing(mppi_handle_t h, float* out_ms8);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_HIP_H */
