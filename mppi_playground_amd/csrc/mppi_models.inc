// mppi_models.inc — body of the model functors; included by mppi_models.hpp once per FP-contraction
// variant with MPPI_MODEL_NS set to the namespace name.  No include guard on purpose.
namespace mppi {
namespace MPPI_MODEL_NS {

// ---------------------------------------------------------------------------------- math
// angle_normalize (src/envs/racing_env.py:20-22): ((x + pi) % (2 pi)) - pi with torch.remainder
// semantics (fmod + sign fix).  fmod is exact, so any exact evaluation of a - k*2pi with the right
// integer k reproduces it bit for bit:
//   narrow fast path (|a| < 4 pi, models that wrap their angle every step): at most one exact
//     subtraction (Sterbenz);
//   WIDE fast path (|a| < 1e5): k = trunc(a/2pi) from a reciprocal multiply, repaired when off by
//     one, and r = fma(-k, 2pi, a) (the product is exact inside the FMA and the true remainder is
//     representable, so the single rounding is exact).
template <bool FAST, bool WIDE = false, bool CHECK = true>
MPPI_HD float angle_normalize(float x, bool& bad) {
    const float a = x + PI_F;
    float r;
    if (FAST && !WIDE) {
        if (CHECK) bad = bad || !(fabsf(a) < 2.0f * TWO_PI_F);
        r = a;
        if (a >= TWO_PI_F) r = a - TWO_PI_F;
        if (a <= -TWO_PI_F) r = a + TWO_PI_F;
    } else if (FAST && WIDE) {
        bad = bad || !(fabsf(a) < 1.0e5f);
        const float sg = copysignf(1.0f, a);
        float k = truncf(a * 0.159154937f);
        const float r0 = fmaf(-k, TWO_PI_F, a);
        float adj = 0.0f;
        if (r0 * sg < 0.0f) adj = -sg;
        if (fabsf(r0) >= TWO_PI_F) adj = sg;
        k += adj;
        r = fmaf(-k, TWO_PI_F, a);
    } else {
        r = fmodf(a, TWO_PI_F);
    }
    if (r != 0.0f && r < 0.0f) r += TWO_PI_F;
    return r - PI_F;
}

// Angle wraps inside the horizon loop of the kinematic models (FAST only).  The heading that enters a
// step is always the output of a previous wrap, i.e. it lies in [-pi, pi) and fl(x + pi) in [0, 2pi):
// the modulo and the sign fix are identities and angle_normalize(x) = fl(fl(x + pi) - pi)
// (rewrap_f).  The heading that leaves a step is a wrapped angle plus an increment the host has
// bounded below pi (ctx.wrap_safe), so fl(x + pi) lies in (-pi, 3pi): one conditional subtraction and
// the sign fix remain (wrap_inc_f).  Both are bit-identical to the library path on those ranges; the
// initial state is range-checked once per trajectory (Model::check_state).
// wrap_inc_f picks the multiple of 2pi without branches: k = floor(fl(a * RN(1/2pi_f))) is -1 for a < 0, 0 on [0, 2pi_f)
// and 1 on [2pi_f, 4pi_f) (RN(1/2pi_f) is the one float for which fl(2pi_f * c) = 1 and fl(pred(2pi_f) * c) < 1), and
// fma(-k, 2pi, a) is the subtraction / addition of the branchy form rounded once, as before (k = 0: a + -0 = a, a != -0).
// Five VALU instead of eight (add, mul, floor, fma, sub); equal to the branchy form for EVERY float x in [-2pi, 2pi]
// (scripts/enum/enum_wrap_index.cpp, profiles/r07_enum_wrap_index.txt).
// rewrap_f is idempotent on the outputs of both wraps: for EVERY float r in [0, 2pi] (the 1 086 918 620 of them,
// checked exhaustively: tests/test_model_functors_host.py samples the same statement), t = fl(r - pi) satisfies
// fl(fl(t + pi) - pi) == t.  So once the heading has been through one wrap, the entry wrap of every later step is the
// identity and is skipped (Model::enter + the `wrapped` argument of step()): two dependent adds per step.
MPPI_HD float rewrap_f(float x) { return (x + PI_F) - PI_F; }
MPPI_HD float wrap_inc_f(float x) {
    const float a = x + PI_F;
    const float k = floorf(a * 0.159154937f);  // RN(1 / TWO_PI_F)
    return fmaf(-k, TWO_PI_F, a) - PI_F;
}

// x with its sign flipped when bit 31 of `m` is set
MPPI_HD float flip_sign(float x, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(x), m, 0x80000000u, 0x78));  // a ^ (b & c)
#else
    unsigned u;
    __builtin_memcpy(&u, &x, 4);
    u ^= (m & 0x80000000u);
    __builtin_memcpy(&x, &u, 4);
    return x;
#endif
}

// sin and cos of one argument.  Fast path: k = rint(x*2/pi), two-term Cody-Waite reduction with
// FMA (exact product), degree-7 / degree-6 minimax polynomials on [-pi/4, pi/4]
// (measured <= 0.76 / 0.80 ulp against double, tests/test_model_functors_host.py).  Valid for |x| <= 200.
template <bool FAST, bool CHECK = true>
MPPI_HD void sincos_f(float x, float& s, float& c, bool& bad) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST && !CHECK && MPPI_MODEL_HWTRIG) {  // wrapped heading, x in [-pi, pi): v_sin_f32 / v_cos_f32 of x / 2pi revolutions
        const float rev = x * 0.159154943f;
        s = __builtin_amdgcn_sinf(rev);
        c = __builtin_amdgcn_cosf(rev);
        return;
    }
#endif
    if (FAST) {
        if (CHECK) bad = bad || !(fabsf(x) <= 200.0f);
        const float kf = rintf(x * 0.636619747f);
        float r = fmaf(-kf, 1.57079637f, x);
        r = fmaf(-kf, -4.37113883e-8f, r);
        const float z = r * r;
        float ps = fmaf(-0.00019582892f, z, 0.008332725f);
        ps = fmaf(ps, z, -0.16666664f);
        const float sr = fmaf(ps, z * r, r);
        float pc = fmaf(2.4542922e-05f, z, -0.0013888279f);
        pc = fmaf(pc, z, 0.041666664f);
        const float t = fmaf(z * z, -pc, 0.5f * z);
        const float cr = 1.0f - t;
        // rotate (sr, cr) by q quarter turns: swap on odd q, flip the signs through the sign bit:
        // sin flips when bit 1 of q is set, cos when bit 1 of q+1 is set.  (x ^ ((q << 30) & 0x80000000))
        // is one shift + one three-input bit operation on the device.
        const int q = (int)kf;
        const float a = (q & 1) ? cr : sr;
        const float b = (q & 1) ? sr : cr;
        s = flip_sign(a, (unsigned)q << 30);
        c = flip_sign(b, (unsigned)(q + 1) << 30);
    } else {
        s = sinf(x);
        c = cosf(x);
    }
}

// sin and cos of an argument the model's own clamps keep small after the first step (the clamped pole angle of the
// cart-poles, 3 x the clamped position of the mountain car).  Hardware-trig variant (mppi::fused_hw): v_sin_f32 /
// v_cos_f32 for |x| <= 4 (abs error <= 2.7e-7 + 4 * 2^-24 / 2 of argument rounding); anything larger (a far-out initial
// state) flags the lane for the library-math redo like every other fast path.
template <bool FAST>
MPPI_HD void sincos_b(float x, float& s, float& c, bool& bad) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST && MPPI_MODEL_HWTRIG) {
        bad = bad || !(fabsf(x) <= 4.0f);
        const float rev = x * 0.159154943f;
        s = __builtin_amdgcn_sinf(rev);
        c = __builtin_amdgcn_cosf(rev);
        return;
    }
#endif
    sincos_f<FAST>(x, s, c, bad);
}

// tan of the (clamped) steering angle.  Fast path (host-checked precondition |x| <= 0.25): odd
// Taylor polynomial to x^9, truncation < 9e-9 relative (0.15 ulp).
template <bool FAST>
MPPI_HD float tan_f(float x) {
    if (FAST) {
        const float z = x * x;
        float p = fmaf(0.0218694885f, z, 0.0539682540f);    // 62/2835, 17/315
        p = fmaf(p, z, 0.133333333f);                       // 2/15
        p = fmaf(p, z, 0.333333333f);                       // 1/3
        return fmaf(p, z * x, x);
    }
    return tanf(x);
}

// x / cell, correctly rounded.  Fast path (host-checked precondition inv_cell = RN(1/cell) and the
// significand of cell is not all ones): Markstein's sequence q0 = RN(x*y), r = x - cell*q0 (exact
// in FMA), q = RN(q0 + r*y), which returns RN(x/cell).
template <bool FAST>
MPPI_HD float div_cell(float x, const MapView& m) {
    if (FAST) {
        const float q0 = x * m.inv_cell;
        const float r = fmaf(-m.cell, q0, x);
        return fmaf(r, m.inv_cell, q0);
    }
    return x / m.cell;
}

// x / c for a compile-time constant c, correctly rounded: Markstein's sequence with y = RN(1/c)
// (constant-folded, IEEE) — bit-identical to the IEEE division it replaces (c's significand must not
// be all ones: true for the 1.1f used by the cart-pole model).
template <bool FAST>
MPPI_HD float div_const(float x, float c, float inv_c) {
    if (FAST) {
        const float q0 = x * inv_c;
        return fmaf(fmaf(-c, q0, x), inv_c, q0);
    }
    return x / c;
}

// ObstacleMap.compute_cost / LaneMap.compute_cost (src/envs/obstacle_map_2d.py:168-200,
// src/envs/lane_map_2d.py:90-122): idx = round_half_even(x / cell + origin); out of bound -> oob,
// else cells[ix][iy].  Branch-free: the index is forced in range and the load is unconditional.
template <bool FAST>
MPPI_HD float occ_lookup(const MapView& m, const uint8_t* cells, float px, float py, float oob) {
    const float qx = rintf(div_cell<FAST>(px, m) + m.ox);
    const float qy = rintf(div_cell<FAST>(py, m) + m.oy);
    // |q| < 2^24 for any position the models can reach (they clamp to the map limits), so the
    // conversions are exact; negative indices wrap to huge unsigned values and fail the test
    const int ix = (int)qx, iy = (int)qy;
    const bool inb = ((unsigned)ix < (unsigned)m.nx) & ((unsigned)iy < (unsigned)m.ny);
    // nx, ny < 2^24: the 24-bit multiply-add is full rate (a 32-bit integer multiply is quarter rate)
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned lin = __umul24((unsigned)ix, (unsigned)m.ny) + (unsigned)iy;
#else
    const unsigned lin = (unsigned)ix * (unsigned)m.ny + (unsigned)iy;
#endif
    const unsigned idx = inb ? lin : 0u;
    const float v = (float)cells[idx];
    return inb ? v : oob;
}

// The same lookup on the padded grid (ModelCtx::pad), for positions the model's own clamp keeps inside
// [0, nx] x [0, ny] (host-checked, pad_map_plan; the initial state is checked by check_state): no compares, no
// selects, no float->int conversions.  t + 1.5*2^23 rounds t to the nearest-even integer in the float's
// mantissa (|t| < 2^22), so bits(t + magic) = 0x4B400000 + round(t); the low 24 bits of that are
// 0x400000 + round(t), which v_mad_u32_u24 multiplies by the row stride, and the constant everything carries
// along is already subtracted from the base pointer.  Value: the cell, or the out-of-bounds value in the pad.
MPPI_HD float occ_lookup_pad(const ModelCtx& c, const MapView& m, float px, float py) {
    const float tx = (div_cell<true>(px, m) + m.ox) + 12582912.0f;
    const float ty = (div_cell<true>(py, m) + m.oy) + 12582912.0f;
    unsigned bx, by;
#if defined(__HIP_DEVICE_COMPILE__)
    bx = __float_as_uint(tx); by = __float_as_uint(ty);
    const unsigned r = __umul24(bx, (unsigned)c.pad_stride) + by;
#else
    __builtin_memcpy(&bx, &tx, 4); __builtin_memcpy(&by, &ty, 4);
    const unsigned r = (bx & 0xFFFFFFu) * ((unsigned)c.pad_stride & 0xFFFFFFu) + by;
#endif
    return (float)c.pad[r];
}

// ---------------------------------------------------------------------------------- models
// step(ctx, s, u, sn, ss, bad): sn = dynamics(s, u); ss = what the reference leaves in S[:, t]
// after the call (== s except for mountaincar, whose dynamics mutates its input views).
// load_k(tab, t): the wave-uniform per-step constants of cost_func's info["t"] (racing: the
//   reference row, KROW floats per step); the rollout kernel copies the table into LDS once per
//   block and fetches row t+1 while step t computes.
// cost(ctx, k, s, u, pu, bad): cost_func(state, action, info{prev_action, t}).
template <int MODEL, bool FAST>
struct Model;

struct NoStepConst {};

template <bool FAST>
struct Model<MPPI_MODEL_PENDULUM, FAST> {  // example/pendulum.py:17-47
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    static MPPI_HD void check_state(const ModelCtx&, const float*, bool&) {}  // every fast path checks its own range
    static MPPI_HD void enter(float*) {}
    static constexpr int DS = 2, DC = 1;
    static MPPI_HD void step(const ModelCtx&, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        const float th = s[0], thdot = s[1];
        const float uu = clampf(u[0], -2.0f, 2.0f);
        float sth, cth;
        sincos_f<FAST>(th + PI_F, sth, cth, bad);
        float newthdot = thdot + (-15.0f * sth + 3.0f * uu) * 0.05f;
        const float newth = th + newthdot * 0.05f;
        newthdot = clampf(newthdot, -8.0f, 8.0f);
        ss[0] = s[0]; ss[1] = s[1];
        sn[0] = newth; sn[1] = newthdot;
    }
    static MPPI_HD float cost(const ModelCtx&, const K&, const float* s, const float*, const float*, bool& bad) {
        const float a = angle_normalize<FAST, true>(s[0], bad);  // theta is never wrapped by the dynamics
        return a * a + 0.1f * (s[1] * s[1]);
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_CARTPOLE, FAST> {  // example/cartpole.py:17-81
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    static MPPI_HD void check_state(const ModelCtx&, const float*, bool&) {}  // every fast path checks its own range
    static MPPI_HD void enter(float*) {}
    static constexpr int DS = 4, DC = 1;
    static MPPI_HD void step(const ModelCtx&, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        const float x = s[0], x_dt = s[1], theta = s[2], theta_dt = s[3];
        float force = 0.0f;
        if (u[0] >= 0.0f) force = 10.0f;
        if (u[0] < 0.0f) force = -10.0f;
        float sintheta, costheta;
        sincos_b<FAST>(theta, sintheta, costheta, bad);
        constexpr float TM = 1.1f, INV_TM = 1.0f / 1.1f;  // total_mass and its correctly rounded reciprocal
        const float temp = div_const<FAST>(force + 0.05f * (theta_dt * theta_dt) * sintheta, TM, INV_TM);
        const float thetaacc = (9.8f * sintheta - costheta * temp) /
                               (0.5f * (1.33333337f - div_const<FAST>(0.1f * (costheta * costheta), TM, INV_TM)));
        const float xacc = temp - div_const<FAST>(0.05f * thetaacc * costheta, TM, INV_TM);
        float newx = x + 0.02f * x_dt;
        const float newx_dt = x_dt + 0.02f * xacc;
        float newtheta = theta + 0.02f * theta_dt;
        const float newtheta_dt = theta_dt + 0.02f * thetaacc;
        newx = clampf(newx, -2.4f, 2.4f);
        newtheta = clampf(newtheta, -0.20943951f, 0.20943951f);
        ss[0] = s[0]; ss[1] = s[1]; ss[2] = s[2]; ss[3] = s[3];
        sn[0] = newx; sn[1] = newx_dt; sn[2] = newtheta; sn[3] = newtheta_dt;
    }
    static MPPI_HD float cost(const ModelCtx&, const K&, const float* s, const float*, const float*, bool& bad) {
        const float a = angle_normalize<FAST>(s[2], bad);
        return a * a + 0.1f * (s[3] * s[3]) + 0.1f * (s[0] * s[0]);
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_MJCARTPOLE, FAST> {  // example/mujoco_cartpole.py:20-81
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    static MPPI_HD void check_state(const ModelCtx&, const float*, bool&) {}
    static MPPI_HD void enter(float*) {}
    static constexpr int DS = 4, DC = 1;
    static MPPI_HD void step(const ModelCtx&, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        (void)uc;
        const float x = s[0], x_dt = s[1], theta = s[2], theta_dt = s[3];
        const float force = u[0];  // continuous force, not re-clamped by the model
        float sintheta, costheta;
        // (polynomials at every fast level: this cart-pole is not stabilised by a bang-bang force, and the 2.7e-7 of the
        // hardware sin/cos grows to 7e-6 of the state over 50 steps — measured, profiles/history_r01_r04.md)
        sincos_f<FAST>(theta, sintheta, costheta, bad);
        // total_mass = 2: the divisions by it are exact scalings in either form
        const float temp = (force + 0.5f * (theta_dt * theta_dt) * sintheta) / 2.0f;
        const float thetaacc = (9.8f * sintheta - costheta * temp) /
                               (0.5f * (1.33333337f - 1.0f * (costheta * costheta) / 2.0f));
        const float xacc = temp - 0.5f * thetaacc * costheta / 2.0f;
        float newx = x + 0.02f * x_dt;
        const float newx_dt = x_dt + 0.02f * xacc;
        float newtheta = theta + 0.02f * theta_dt;
        const float newtheta_dt = theta_dt + 0.02f * thetaacc;
        newx = clampf(newx, -1.0f, 1.0f);
        newtheta = clampf(newtheta, -0.20943951f, 0.20943951f);
        ss[0] = s[0]; ss[1] = s[1]; ss[2] = s[2]; ss[3] = s[3];
        sn[0] = newx; sn[1] = newx_dt; sn[2] = newtheta; sn[3] = newtheta_dt;
    }
    static MPPI_HD float cost(const ModelCtx&, const K&, const float* s, const float*, const float*, bool& bad) {
        const float a = angle_normalize<FAST>(s[2], bad);
        return a * a + 0.1f * (s[3] * s[3]) + 0.1f * (s[0] * s[0]);
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_GOALZONE, FAST> {  // src/envs/goal_in_danger_zone.py:113-156
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    static constexpr int DS = 7, DC = 2;
    // FAST precondition: the initial heading is a wrapped angle (every later one is: wrap_inc_f output)
    static MPPI_HD void check_state(const ModelCtx&, const float* s, bool& bad) { bad = bad || !(fabsf(s[2]) <= PI_F); }
    static MPPI_HD void enter(float*) {}
    static MPPI_HD void step(const ModelCtx& c, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        const float* P = c.P;
        const float x = s[0], y = s[1];
        const float v = uc ? u[0] : clampf(u[0], P[MPPI_GP_VMIN], P[MPPI_GP_VMAX]);
        const float omega = uc ? u[1] : clampf(u[1], P[MPPI_GP_WMIN], P[MPPI_GP_WMAX]);
        // the heading is advanced FIRST and the new heading moves the robot
        const float th_in = s[2] + omega * P[MPPI_GP_DT];
        const float theta = FAST ? wrap_inc_f(th_in) : angle_normalize<false>(th_in, bad);
        float sn_, cs_;
        sincos_f<FAST, false>(theta, sn_, cs_, bad);
        const float new_x = x + v * cs_ * P[MPPI_GP_DT];
        const float new_y = y + v * sn_ * P[MPPI_GP_DT];
#pragma unroll
        for (int j = 0; j < 7; ++j) ss[j] = s[j];
        sn[0] = new_x; sn[1] = new_y; sn[2] = theta;
        sn[3] = P[MPPI_GP_GX] - new_x; sn[4] = P[MPPI_GP_GY] - new_y;
        sn[5] = P[MPPI_GP_CX] - new_x; sn[6] = P[MPPI_GP_CY] - new_y;
    }
    static MPPI_HD float cost(const ModelCtx& c, const K&, const float* s, const float*, const float*, bool&) {
        const float* P = c.P;
        const float dist_to_goal = sqrtf(s[3] * s[3] + s[4] * s[4]);
        const float dist_to_center = sqrtf(s[5] * s[5] + s[6] * s[6]);
        const float collided = dist_to_center < P[MPPI_GP_RADIUS] ? 1.0f : 0.0f;
        return dist_to_goal + collided * P[MPPI_GP_PENALTY];
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_MOUNTAINCAR, FAST> {  // example/mountaincar.py:17-55
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    static MPPI_HD void check_state(const ModelCtx&, const float*, bool&) {}  // every fast path checks its own range
    static MPPI_HD void enter(float*) {}
    static constexpr int DS = 2, DC = 1;
    static MPPI_HD void step(const ModelCtx&, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        const float position = s[0], velocity = s[1];
        const float force = clampf(u[0], -1.0f, 1.0f);
        float s3, c3;
        sincos_b<FAST>(3.0f * position, s3, c3, bad);
        const float v1 = velocity + (force * 0.0015f - 0.0025f * c3);
        const float v2 = clampf(v1, -0.07f, 0.07f);
        const float p1 = position + v2;
        const float p2 = clampf(p1, -1.2f, 0.6f);
        ss[0] = p1; ss[1] = v1;  // `velocity +=` / `position +=` act on views of S[:, t]
        sn[0] = p2; sn[1] = v2;
    }
    static MPPI_HD float cost(const ModelCtx&, const K&, const float* s, const float*, const float*, bool&) {
        const float d = 0.45f - s[0];
        return d * d;
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_NAV2D, FAST> {  // src/envs/navigation_2d.py:218-279
    using K = NoStepConst;
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int) { return K{}; }
    // FAST precondition on the trajectory's initial heading: a wrapped angle (see rewrap_f); otherwise
    // the lane is recomputed with the library math
    static MPPI_HD void check_state(const ModelCtx& c, const float* s, bool& bad) {
        const float a = s[2] + PI_F;
        bad = bad || !(a >= 0.0f && a < TWO_PI_F);
        // the padded-grid lookup needs the position inside the model's clamp range from the first step on
        const float* P = c.P;
        bad = bad || !(s[0] >= P[MPPI_NP_XLO] && s[0] <= P[MPPI_NP_XHI] && s[1] >= P[MPPI_NP_YLO] && s[1] <= P[MPPI_NP_YHI]);
    }
    static constexpr int DS = 3, DC = 2;
    // FAST hot loops: wrap the (range-checked) initial heading once, then call step(..., wrapped = true)
    static MPPI_HD void enter(float* s) { s[2] = rewrap_f(s[2]); }
    // The cost kernels' entry takes ANY finite initial state, so that no lane ever has to be redone with the library
    // math (the redo path cost the racing kernel 18 VGPRs and two waves per SIMD): the heading is wrapped once with
    // the reference's own operation (fmod: exact, any magnitude; bit-identical to rewrap_f on its range), and a start
    // outside the position clamp — whose cell index the padded grid cannot serve — is a launch-uniform property of
    // x0 that selects a copy of the loop whose FIRST stage cost uses the bounds-tested lookup (cost(..., general)).
    static constexpr bool ENTRY_GENERAL = true;
    static MPPI_HD void enter_any(float* s) { bool ig = false; s[2] = angle_normalize<false>(s[2], ig); }
    static MPPI_HD bool start_in_box(const ModelCtx& c, const float* s) {
        const float* P = c.P;
        return s[0] >= P[MPPI_NP_XLO] && s[0] <= P[MPPI_NP_XHI] && s[1] >= P[MPPI_NP_YLO] && s[1] <= P[MPPI_NP_YHI];
    }
    static MPPI_HD void pin_hot(ModelCtx& c) {  // see Model<RACING>::pin_hot
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(c.P[MPPI_NP_XHI]), "+v"(c.P[MPPI_NP_YHI]));
#else
        (void)c;
#endif
    }
    static MPPI_HD void step(const ModelCtx& c, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false) {
        const float* P = c.P;
        const float x = s[0], y = s[1];
        // `uc` (a compile-time constant at the hot call site): the action already lies inside the model's
        // own clamp range, so the clamp is the identity
        const float v = uc ? u[0] : clampf(u[0], P[MPPI_NP_VMIN], P[MPPI_NP_VMAX]);
        const float omega = uc ? u[1] : clampf(u[1], P[MPPI_NP_WMIN], P[MPPI_NP_WMAX]);
        // range checks: only the incoming heading can be out of the narrow wrap range (host-checked
        // ctx.wrap_safe bounds the per-step increment); the wrapped heading feeds sin/cos
        const float theta = FAST ? (wrapped ? s[2] : rewrap_f(s[2])) : angle_normalize<false>(s[2], bad);
        float sn_, cs_;
        sincos_f<FAST, false>(theta, sn_, cs_, bad);
        const float new_x = x + v * cs_ * P[MPPI_NP_DT];
        const float new_y = y + v * sn_ * P[MPPI_NP_DT];
        const float th_in = theta + omega * P[MPPI_NP_DT];
        const float new_theta = FAST ? wrap_inc_f(th_in) : angle_normalize<false>(th_in, bad);
        ss[0] = s[0]; ss[1] = s[1]; ss[2] = s[2];
        sn[0] = clampf(new_x, P[MPPI_NP_XLO], P[MPPI_NP_XHI]);
        sn[1] = clampf(new_y, P[MPPI_NP_YLO], P[MPPI_NP_YHI]);
        sn[2] = new_theta;
    }
    // `general`: bounds-tested lookup in the map itself (same cell: Markstein's quotient IS the IEEE quotient)
    static MPPI_HD float cost(const ModelCtx& c, const K&, const float* s, const float*, const float*, bool&, bool general = false) {
        const float* P = c.P;
        const float dx = s[0] - P[MPPI_NP_GX], dy = s[1] - P[MPPI_NP_GY];
        const float goal_cost = sqrtf(dx * dx + dy * dy);
        const float occ = (FAST && !general) ? occ_lookup_pad(c, c.maps[0], s[0], s[1])  // host-checked: ctx.pad is set
                                             : occ_lookup<FAST>(c.maps[0], c.maps[0].cells, s[0], s[1], 1.0f);
        return goal_cost + P[MPPI_NP_QO] * occ;
    }
};

// nav2d with up to MPPI_MAX_DISCS moving disc obstacles (include/mppi_hip.h, mppi_set_discs, states the rule; mppi_discs.hpp
// is the arithmetic).  Dynamics, entry and the static-map cost are Model<NAV2D>'s.  The step-constant table holds one row
// of 8 discs per horizon step; K is only the address of row t in the block's LDS copy (one register across the step, not
// 8 x 4 floats): cost() reads the discs of its row there, each one 16-byte read at a wave-uniform address, and stops at the
// launch-uniform count (disc_count).  The terminal cost reads row T-1 like every user of the table (trajectory_cost).
template <bool FAST>
struct Model<MPPI_MODEL_NAV2D_DISCS, FAST> : Model<MPPI_MODEL_NAV2D, FAST> {
    using Base = Model<MPPI_MODEL_NAV2D, FAST>;
    struct K { const float* row; };
    static constexpr int KROW = DISC_ROW;
    static_assert(KROW == 4 * MPPI_MAX_DISCS, "one row = MPPI_MAX_DISCS discs of {cx, cy, r2, w}");
    static MPPI_HD K load_k(const float* tab, int t) { return K{tab + KROW * t}; }  // tab = ctx.ref or its LDS copy
    static MPPI_HD float cost(const ModelCtx& c, const K& k, const float* s, const float* u, const float* pu, bool& bad,
                              bool general = false) {
        const float base = Base::cost(c, NoStepConst{}, s, u, pu, bad, general);
        const float pen = disc_row_penalty<FAST>(k.row, disc_count(c), s[0], s[1]);
        return base + pen;
    }
};

template <bool FAST>
struct Model<MPPI_MODEL_RACING, FAST> {  // src/envs/racing_env.py:327-372, example/racing.py:110-159
    static constexpr int DS = 4, DC = 2;
    struct K { float xr, yr, vr, sinp, cosp; };  // reference_path[t] with sin/cos of its yaw
    static constexpr int KROW = 8;                // floats per row of the step-constant table
    static MPPI_HD K load_k(const float* tab, int t) {  // tab = ctx.ref or its LDS copy
        const float* r = tab + 8 * t;
        return K{r[0], r[1], r[3], r[4], r[5]};
    }
    static MPPI_HD void check_state(const ModelCtx& c, const float* s, bool& bad) {  // see Model<NAV2D>::check_state
        const float a = s[2] + PI_F;
        bad = bad || !(a >= 0.0f && a < TWO_PI_F);
        const float* P = c.P;
        bad = bad || !(s[0] >= P[MPPI_RP_XLO] && s[0] <= P[MPPI_RP_XHI] && s[1] >= P[MPPI_RP_YLO] && s[1] <= P[MPPI_RP_YHI]);
    }
    static MPPI_HD void enter(float* s) { s[2] = rewrap_f(s[2]); }  // see Model<NAV2D>::enter
    static constexpr bool ENTRY_GENERAL = true;                       // see Model<NAV2D>::enter_any
    static MPPI_HD void enter_any(float* s) { bool ig = false; s[2] = angle_normalize<false>(s[2], ig); }
    static MPPI_HD bool start_in_box(const ModelCtx& c, const float* s) {
        const float* P = c.P;
        return s[0] >= P[MPPI_RP_XLO] && s[0] <= P[MPPI_RP_XHI] && s[1] >= P[MPPI_RP_YLO] && s[1] <= P[MPPI_RP_YHI];
    }
    // The cost kernels work on a private copy of the launch constants whose entries listed here live in VGPRs: a VALU
    // instruction reads ONE scalar register, so v_med3_f32(x, lo, hi) with both bounds wave-uniform needs a vector copy of
    // one, which the compiler otherwise re-materialises (v_mov) in every step of the horizon loop.
    static MPPI_HD void pin_hot(ModelCtx& c) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(c.P[MPPI_RP_XHI]), "+v"(c.P[MPPI_RP_YHI]));
#else
        (void)c;
#endif
    }
    static MPPI_HD void step(const ModelCtx& c, const float* s, const float* u, float* sn, float* ss, bool& bad, bool uc = false, bool wrapped = false,
                             bool unit_L = false) {
        const float* P = c.P;
        const float x = s[0], y = s[1], v = s[3];
        const float accel = uc ? u[0] : clampf(u[0], P[MPPI_RP_AMIN], P[MPPI_RP_AMAX]);
        const float steer = uc ? u[1] : clampf(u[1], P[MPPI_RP_SMIN], P[MPPI_RP_SMAX]);
        const float theta = FAST ? (wrapped ? s[2] : rewrap_f(s[2])) : angle_normalize<false>(s[2], bad);
        float sn_, cs_;
        sincos_f<FAST, false>(theta, sn_, cs_, bad);
        const float dx = v * cs_;
        const float dy = v * sn_;
        const float vt = v * tan_f<FAST>(steer);
        float dtheta;
        if (FAST) {  // vt / L by Markstein's sequence (host-checked precondition on inv_L); exact for L = 1
            if (unit_L) {  // (compile-time at the hot call site) wheel base exactly 1: vt / 1 == vt
                dtheta = vt;
            } else {
                const float q0 = vt * c.inv_L;
                dtheta = fmaf(fmaf(-P[MPPI_RP_L], q0, vt), c.inv_L, q0);
            }
        } else {
            dtheta = vt / P[MPPI_RP_L];
        }
        const float new_x = x + dx * P[MPPI_RP_DT];
        const float new_y = y + dy * P[MPPI_RP_DT];
        const float th_in = theta + dtheta * P[MPPI_RP_DT];
        const float new_theta = FAST ? wrap_inc_f(th_in) : angle_normalize<false>(th_in, bad);
        const float new_v = v + accel * P[MPPI_RP_DT];
        ss[0] = s[0]; ss[1] = s[1]; ss[2] = s[2]; ss[3] = s[3];
        sn[0] = clampf(new_x, P[MPPI_RP_XLO], P[MPPI_RP_XHI]);
        sn[1] = clampf(new_y, P[MPPI_RP_YLO], P[MPPI_RP_YHI]);
        sn[2] = new_theta;
        sn[3] = clampf(new_v, -P[MPPI_RP_VMAX], P[MPPI_RP_VMAX]);
    }
#if defined(__HIPCC__)
    // Batch-1 rollout (mppi.py:508-524) of `acts` [T][2] spread over one wave instead of one lane walking T full
    // steps: only the heading and speed recurrences are serial (~15 dependent instructions per step, every lane
    // runs the same chain and lane t keeps what step t needs); sin/cos, the position increments and the
    // steering tangents are evaluated for all steps at once (lane t = step t), and the two position
    // recurrences are one FMA + clamp per step.  Same expressions as step() with FAST math (the FMAs step()
    // gets from contraction are written out); lane t <= T writes state row t.  T <= 63.
    static __device__ __forceinline__ void rollout_wave(const ModelCtx& c, const float* x0, const float* acts, int T,
                                                        float* out) {
        static_assert(FAST, "wave rollout exists for the fast-math variant only");
        const float* P = c.P;
        const int lane = threadIdx.x & 63;
        const float dt = P[MPPI_RP_DT];
        float accel = 0.0f, tn = 0.0f;
        if (lane < T) {
            accel = clampf(acts[2 * lane], P[MPPI_RP_AMIN], P[MPPI_RP_AMAX]);
            tn = tan_f<true>(clampf(acts[2 * lane + 1], P[MPPI_RP_SMIN], P[MPPI_RP_SMAX]));
        }
        float th_raw = x0[2], v = x0[3];
        float my_raw = th_raw, my_th = 0.0f, my_v = v;
        bool bad = false;  // (never raised on this path: the entry wrap is the library's, the in-loop fast paths are unchecked)
        // step 0: any finite heading, wrapped by the reference's own operation (enter_any); afterwards th_raw is a fixed
        // point of the wrap (see rewrap_f)
        float theta = angle_normalize<false>(th_raw, bad);
        for (int t = 0; t < T; ++t) {
            const float a_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(accel), t));
            const float tan_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tn), t));
            if (lane == t) { my_raw = th_raw; my_th = theta; my_v = v; }
            const float vt = v * tan_t;
            const float q0 = vt * c.inv_L;
            const float dtheta = fmaf(fmaf(-P[MPPI_RP_L], q0, vt), c.inv_L, q0);
            th_raw = theta = wrap_inc_f(fmaf(dtheta, dt, theta));
            v = clampf(fmaf(a_t, dt, v), -P[MPPI_RP_VMAX], P[MPPI_RP_VMAX]);
        }
        if (lane == T) { my_raw = th_raw; my_v = v; }
        float sn_, cs_;
        sincos_f<true, false>(my_th, sn_, cs_, bad);
        const float dx = my_v * cs_, dy = my_v * sn_;
        float x = x0[0], y = x0[1], my_x = x, my_y = y;
        for (int t = 0; t < T; ++t) {
            if (lane == t) { my_x = x; my_y = y; }
            const float dx_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dx), t));
            const float dy_t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dy), t));
            x = clampf(fmaf(dx_t, dt, x), P[MPPI_RP_XLO], P[MPPI_RP_XHI]);
            y = clampf(fmaf(dy_t, dt, y), P[MPPI_RP_YLO], P[MPPI_RP_YHI]);
        }
        if (lane == T) { my_x = x; my_y = y; }
        if (lane <= T) {
            float* row = out + 4 * lane;
            row[0] = my_x; row[1] = my_y; row[2] = my_raw; row[3] = my_v;
        }
    }
#endif
    static MPPI_HD float cost(const ModelCtx& c, const K& k, const float* s, const float* u, const float* pu, bool&,
                              bool general = false) {  // see Model<NAV2D>::cost
        const float* P = c.P;
        const float sinp = k.sinp, cosp = k.cosp;
        const float ex = s[0] - k.xr, ey = s[1] - k.yr;
        const float ec = sinp * ex - cosp * ey;
        const float el = -cosp * ex - sinp * ey;
        const float path_cost = P[MPPI_RP_QC] * (ec * ec) + P[MPPI_RP_QL] * (el * el);
        const float dv = s[3] - k.vr;
        const float velocity_cost = P[MPPI_RP_QV] * (dv * dv);
        float occ;
        if (FAST && !general) {  // host-checked precondition: both maps share geometry and are summed into ctx.pad (0..2)
            occ = occ_lookup_pad(c, c.maps[0], s[0], s[1]);
        } else {
            occ = occ_lookup<FAST>(c.maps[0], c.maps[0].cells, s[0], s[1], 1.0f);
            occ += occ_lookup<FAST>(c.maps[1], c.maps[1].cells, s[0], s[1], 1.0f);
        }
        const float obstacle_cost = P[MPPI_RP_QO] * occ;
        float input_cost = P[MPPI_RP_QIN] * (u[0] * u[0] + u[1] * u[1]);
        const float d0 = u[0] - pu[0], d1 = u[1] - pu[1];
        input_cost += P[MPPI_RP_QDIN] * (d0 * d0 + d1 * d1);
        return path_cost + velocity_cost + obstacle_cost + input_cost;
    }
};

// Racing among up to MPPI_MAX_DISCS moving discs — opponent cars (include/mppi_hip.h, mppi_set_discs, states the rule;
// mppi_discs.hpp is the arithmetic, exactly as nav2d's variant uses it).  Dynamics, entry rules, the pinned constants, the
// wave-parallel batch-1 rollout and the whole of racing's cost are Model<RACING>'s.  The step-constant table holds ONE row
// of RACING_DISCS_KROW = 40 floats per horizon step: racing's reference row in floats 0-7, the eight padded discs behind it
// (mppi_models.hpp), so the kernels stage T * KROW contiguous floats of ctx.ref as they do for every model.  K carries
// racing's five reference values and the address of the row's discs in the block's LDS copy; the penalty is added LAST, so
// with no disc (disc_count = 0) or no hit the cost is racing's bit for bit.
template <bool FAST>
struct Model<MPPI_MODEL_RACING_DISCS, FAST> : Model<MPPI_MODEL_RACING, FAST> {
    using Base = Model<MPPI_MODEL_RACING, FAST>;
    struct K { typename Base::K ref; const float* discs; };
    static constexpr int KROW = RACING_DISCS_KROW;
    static_assert(KROW == RACING_REF_ROW + 4 * MPPI_MAX_DISCS, "one row = the reference row + MPPI_MAX_DISCS discs of {cx, cy, r2, w}");
    static MPPI_HD K load_k(const float* tab, int t) {  // tab = ctx.ref or its LDS copy
        const float* r = tab + KROW * t;
        return K{typename Base::K{r[0], r[1], r[3], r[4], r[5]}, r + RACING_REF_ROW};
    }
    static MPPI_HD float cost(const ModelCtx& c, const K& k, const float* s, const float* u, const float* pu, bool& bad,
                              bool general = false) {
        const float base = Base::cost(c, k.ref, s, u, pu, bad, general);
        const float pen = disc_row_penalty<FAST>(k.discs, disc_count(c, MPPI_MODEL_RACING_DISCS), s[0], s[1]);
        return base + pen;
    }
};

// The soft disc models (include/mppi_hip.h, mppi_set_disc_softness, states the rule; mppi_discs.hpp is the arithmetic): the
// hard models with a graded skirt round every disc.  Step table, K, KROW, load_k, LDS staging and the entry rules are
// inherited; only cost() differs — the same base cost, the soft row penalty with the two launch-uniform coefficients
// (disc_soft), added last.
template <bool FAST>
struct Model<MPPI_MODEL_NAV2D_DISCS_SOFT, FAST> : Model<MPPI_MODEL_NAV2D_DISCS, FAST> {
    using Hard = Model<MPPI_MODEL_NAV2D_DISCS, FAST>;
    static MPPI_HD float cost(const ModelCtx& c, const typename Hard::K& k, const float* s, const float* u, const float* pu, bool& bad,
                              bool general = false) {
        const float base = Hard::Base::cost(c, NoStepConst{}, s, u, pu, bad, general);
        const DiscSoft f = disc_soft(c, MPPI_MODEL_NAV2D_DISCS_SOFT);
        const float pen = disc_row_penalty_soft<FAST>(k.row, disc_count(c, MPPI_MODEL_NAV2D_DISCS_SOFT), s[0], s[1], f.a, f.b);
        return base + pen;
    }
};
template <bool FAST>
struct Model<MPPI_MODEL_RACING_DISCS_SOFT, FAST> : Model<MPPI_MODEL_RACING_DISCS, FAST> {
    using Hard = Model<MPPI_MODEL_RACING_DISCS, FAST>;
    static MPPI_HD float cost(const ModelCtx& c, const typename Hard::K& k, const float* s, const float* u, const float* pu, bool& bad,
                              bool general = false) {
        const float base = Hard::Base::cost(c, k.ref, s, u, pu, bad, general);
        const DiscSoft f = disc_soft(c, MPPI_MODEL_RACING_DISCS_SOFT);
        const float pen = disc_row_penalty_soft<FAST>(k.discs, disc_count(c, MPPI_MODEL_RACING_DISCS_SOFT), s[0], s[1], f.a, f.b);
        return base + pen;
    }
};

// Learned dynamics: a multi-layer perceptron whose weights are data (include/mppi_hip.h, mppi_set_mlp, states the
// arithmetic; the table is ctx.ref, the flags ctx.ref_rows).  Every product-sum is written a * b + c: mppi::strict rounds
// each operation on its own (the numpy restatement of tests/mlp_ref.py, bit for bit with relu), the fast namespaces may
// contract.  The weights are wave-uniform: they are read at uniform addresses and arrive as the scalar operand of the VALU
// multiply-adds.  Shape of the code (the step is inlined once per step of a float4 group, per drain half, in the epilogue
// and per noise mode, so the network is NOT unrolled as a whole):
//   two hidden layers: layer 1 unrolled over its 32 units (h1 lives in 32 statically indexed registers), then ONE rolled
//     loop over j that forms h2[j] from h1, applies the activation and adds W3[m][j] * h2[j] into the DS outputs;
//   one hidden layer:  one rolled loop over j that forms h1[j] from the IN inputs and adds W3[m][j] * h1[j].
// Both visit every sum in ascending index order.  tanh at the fast levels: 1 - 2 / (e^(2z) + 1) with the hardware
// exponential and reciprocal (e = inf and e = 0 give +-1: no validity range, `bad` is never raised).
template <bool FAST>
MPPI_HD float mlp_act(float z, bool use_tanh) {
    if (!use_tanh) return fmaxf(z, 0.0f);
    if (FAST) {
#if defined(__HIP_DEVICE_COMPILE__)
        const float e = __builtin_amdgcn_exp2f(z * 2.88539008f);  // 2 * log2(e)
        return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
#else
        return 1.0f - 2.0f / (expf(2.0f * z) + 1.0f);
#endif
    }
    return tanhf(z);
}

// The table as the step reads it.  On the device the pointer is cast into the constant address space: the table is not written
// while a kernel runs and every address is wave-uniform, so each read is a scalar load (a plain global pointer the compiler
// cannot prove unclobbered next to the kernels' stores is read with per-lane vector loads: 64 copies of one value in VGPRs).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const float __attribute__((address_space(4)))* MlpTable;
#else
typedef const float* MlpTable;
#endif

template <int DSN, int DCN, bool FAST>
struct MlpModel {
    // The step constant is the step index itself: cost() forms the address of its reference row from it (mppi_models.hpp:
    // mlp_reference).  Nothing is staged in LDS (KROW = 0): the row is 2 * DS scalar operands where t is wave-uniform.
    struct K { int t; };
    static constexpr int KROW = 0;
    static MPPI_HD K load_k(const float*, int t) { return K{t}; }
    static MPPI_HD void check_state(const ModelCtx&, const float*, bool&) {}
    static MPPI_HD void enter(float*) {}
    static constexpr int DS = DSN, DC = DCN, IN = DS + DC, H = MPPI_MLP_HIDDEN;
    // offsets into the table: W1[H][IN], b1[H], W2[H][H], b2[H], W3[DS][H], b3[DS]
    static constexpr int OB1 = H * IN, OW2 = OB1 + H, OB2 = OW2 + H * H, OW3 = OB2 + H, OB3 = OW3 + DS * H;
    static MPPI_HD void step(const ModelCtx& c, const float* s, const float* u, float* sn, float* ss, bool&, bool = false, bool = false) {
        const MlpTable W = (MlpTable)c.ref;
        const bool use_tanh = (c.ref_rows & MLP_TANH) != 0;
        float x[IN], o[DS];
#pragma unroll
        for (int m = 0; m < DS; ++m) { x[m] = s[m]; o[m] = W[OB3 + m]; }
#pragma unroll
        for (int k = 0; k < DC; ++k) x[DS + k] = u[k];
        if (c.ref_rows & MLP_TWO_LAYERS) {
            float h1[H];
#pragma unroll
            for (int j = 0; j < H; ++j) {
                float z = W[OB1 + j];
#pragma unroll
                for (int i = 0; i < IN; ++i) z = z + W[j * IN + i] * x[i];
                h1[j] = mlp_act<FAST>(z, use_tanh);
            }
#pragma clang loop unroll(disable)
            for (int j = 0; j < H; ++j) {
                const MlpTable w2 = W + OW2 + j * H;
                float z = W[OB2 + j];
#pragma unroll
                for (int i = 0; i < H; ++i) z = z + w2[i] * h1[i];
                const float h = mlp_act<FAST>(z, use_tanh);
#pragma unroll
                for (int m = 0; m < DS; ++m) o[m] = o[m] + W[OW3 + m * H + j] * h;
            }
        } else {
#pragma clang loop unroll(disable)
            for (int j = 0; j < H; ++j) {
                const MlpTable w1 = W + j * IN;
                float z = W[OB1 + j];
#pragma unroll
                for (int i = 0; i < IN; ++i) z = z + w1[i] * x[i];
                const float h = mlp_act<FAST>(z, use_tanh);
#pragma unroll
                for (int m = 0; m < DS; ++m) o[m] = o[m] + W[OW3 + m * H + j] * h;
            }
        }
        const bool residual = (c.ref_rows & MLP_RESIDUAL) != 0;
#pragma unroll
        for (int m = 0; m < DS; ++m) {
            ss[m] = s[m];
            sn[m] = residual ? s[m] + o[m] : o[m];
        }
    }
    // cost parameters g[DS], q[DS], r[DC]: MPPI_MP_* for 4 states, MPPI_MP8_* for 8
    static constexpr int PG = 0, PQ = DS, PR = 2 * DS;
    static_assert(DS == 4 ? (PG == MPPI_MP_G && PQ == MPPI_MP_Q && PR == MPPI_MP_R)
                          : (DS == 8 && PG == MPPI_MP8_G && PQ == MPPI_MP8_Q && PR == MPPI_MP8_R),
                  "the parameter layout of include/mppi_hip.h");
    static_assert(PR + DC <= MPPI_MAX_PARAMS && OB3 + DS == mlp_table_floats(DS, DC), "parameters and table as the host sizes them");
    // Stage cost of step k.t (the terminal cost: the caller hands row T - 1 and u = 0).  Goal and weights are row k.t of the
    // reference table, or P[] when there is none (the only P[] slots that path reads: g, q, r as before); the error of an
    // angular component is wrapped into [-pi, pi] by d - TWO_PI * rint(d * INV_TWO_PI), each operation rounded on its own in
    // mppi::strict.  Both choices are launch-uniform branches: a handle without a mask executes no wrap instruction.
    static MPPI_HD float cost(const ModelCtx& c, const K& k, const float* s, const float* u, const float*, bool&) {
        const float* P = c.P;
        const MlpTable R = mlp_reference(c);
        uint32_t ang = mlp_angular(c);
#if defined(__HIP_DEVICE_COMPILE__)
        // (opaque per call: otherwise the DS tests `ang & (1 << m)` are hoisted out of the horizon loop as DS 64-bit lane masks held
        // across it — 8 or 16 SGPRs: every 8-state kernel spilled scalar registers into vector lanes.  Formed per step they are
        // transient.)
        asm volatile("" : "+s"(ang));
#endif
        float g[DS], q[DS];
        if (R) {
            const MlpTable row = R + k.t * (2 * DS);
#pragma unroll
            for (int m = 0; m < DS; ++m) { g[m] = row[m]; q[m] = row[DS + m]; }
        } else {
#pragma unroll
            for (int m = 0; m < DS; ++m) { g[m] = P[PG + m]; q[m] = P[PQ + m]; }
        }
        float a = 0.0f;
        if (ang) {
#pragma unroll
            for (int m = 0; m < DS; ++m) {
                float d = s[m] - g[m];
                if (ang & (1u << m)) {
                    const float turns = rintf(d * MLP_INV_TWO_PI);
                    d = d - MLP_TWO_PI * turns;
                }
                a = a + q[m] * (d * d);
            }
        } else {
#pragma unroll
            for (int m = 0; m < DS; ++m) {
                const float d = s[m] - g[m];
                a = a + q[m] * (d * d);
            }
        }
#pragma unroll
        for (int k2 = 0; k2 < DC; ++k2) a = a + P[PR + k2] * (u[k2] * u[k2]);
        return a;
    }
    // The learned terminal value V(s) of the final state (mppi_models.hpp: set_mlp_value; the TRACK kernels only, once per
    // trajectory behind the horizon loop).  Offsets into its table: W1[H][DS], b1[H], W2[H][H], b2[H], w3[H], b3[1].  Written
    // like step(): the weights are scalar operands, layer 1 is unrolled into 32 statically indexed registers — live only here,
    // where step()'s are dead — and layer 2 is one rolled loop; every sum in ascending index order.  One hidden layer forms V
    // from h1.  Depth and activation are the value's own flags, not the dynamics network's.
    static constexpr int VB1 = H * DS, VW2 = VB1 + H, VB2 = VW2 + H * H, VW3 = VB2 + H, VB3 = VW3 + H;
    static_assert(VB3 + 1 == mlp_value_floats(DS), "the value table as the host sizes it");
    static MPPI_HD float value(const float* table, int flags, const float* s) {
        const MlpTable W = (MlpTable)table;
        const bool use_tanh = (flags & MLP_VALUE_TANH) != 0;
        float h1[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            float z = W[VB1 + j];
#pragma unroll
            for (int i = 0; i < DS; ++i) z = z + W[j * DS + i] * s[i];
            h1[j] = mlp_act<FAST>(z, use_tanh);
        }
        float v = W[VB3];
        if (flags & MLP_VALUE_TWO_LAYERS) {
#pragma clang loop unroll(disable)
            for (int j = 0; j < H; ++j) {
                const MlpTable w2 = W + VW2 + j * H;
                float z = W[VB2 + j];
#pragma unroll
                for (int i = 0; i < H; ++i) z = z + w2[i] * h1[i];
                v = v + W[VW3 + j] * mlp_act<FAST>(z, use_tanh);
            }
        } else {
#pragma unroll
            for (int j = 0; j < H; ++j) v = v + W[VW3 + j] * h1[j];
        }
        return v;
    }
    static MPPI_HD float value(const ModelCtx& c, const float* s) {
        return value(reinterpret_cast<const float*>(c.maps[1].cells), mlp_value_flags(c), s);
    }
    // The terminal cost with the value in it: quad + (weight * V), or weight * V alone (MLP_VALUE_REPLACE).  `table` and
    // `weight` are wave-uniform: the context's, or a block's LDS copy of them (MlpValueSlot, mppi_models.hpp).
    static MPPI_HD float terminal_with_value(const float* table, int flags, float weight, float quad, const float* s) {
#if defined(__HIP_DEVICE_COMPILE__)
        // (opaque here, like the angular mask in cost(): the tests of the three flags are otherwise formed in front of the horizon
        // loop and held across it as scalar registers the loop does not have)
        asm volatile("" : "+s"(flags));
#endif
        const float wv = weight * value(table, flags, s);
        return (flags & MLP_VALUE_REPLACE) ? wv : quad + wv;
    }
    static MPPI_HD float terminal_with_value(const ModelCtx& c, float quad, const float* s) {
        return terminal_with_value(reinterpret_cast<const float*>(c.maps[1].cells), mlp_value_flags(c), mlp_value_weight(c), quad, s);
    }
    // The cost of a handle with neither reference nor mask, as it always was: every kernel that evaluates these models exists
    // in two instantiations (TRACK, mppi_rollout.hpp) and the launch site picks one (mlp_tracking), so a default solver runs the
    // kernel it ran, with no pointer, no step index and no branch in its loop.
    static MPPI_HD float cost_plain(const ModelCtx& c, const K&, const float* s, const float* u, const float*, bool&) {
        const float* P = c.P;
        float a = 0.0f;
#pragma unroll
        for (int m = 0; m < DS; ++m) {
            const float d = s[m] - P[PG + m];
            a = a + P[PQ + m] * (d * d);
        }
#pragma unroll
        for (int k2 = 0; k2 < DC; ++k2) a = a + P[PR + k2] * (u[k2] * u[k2]);
        return a;
    }
};
template <bool FAST>
struct Model<MPPI_MODEL_MLP41, FAST> : MlpModel<4, 1, FAST> {};
template <bool FAST>
struct Model<MPPI_MODEL_MLP42, FAST> : MlpModel<4, 2, FAST> {};
template <bool FAST>
struct Model<MPPI_MODEL_MLP81, FAST> : MlpModel<8, 1, FAST> {};
template <bool FAST>
struct Model<MPPI_MODEL_MLP82, FAST> : MlpModel<8, 2, FAST> {};
template <bool FAST>
struct Model<MPPI_MODEL_MLP84, FAST> : MlpModel<8, 4, FAST> {};

}  // namespace MPPI_MODEL_NS
}  // namespace mppi
