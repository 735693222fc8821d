// capi_model.hip — C ABI (include/mppi_hip.h): model parameters, maps, the reference and its device-resident window,
// env.step and grid lookups on the device.
#include <algorithm>
#include <cmath>

#include "mppi_handle.hpp"
#include "mppi_env.hpp"
#include "mppi_maps.hpp"

namespace mppi {

// (Re)build the padded grid of the FAST lookup when the maps and the model parameters allow it; otherwise
// ctx.pad stays null and the FAST=false kernels (bounds-tested lookups) are dispatched.
void refresh_pad(mppi_handle_t h, hipStream_t s) {
    h->model.ctx.pad = nullptr;
    h->model.ctx.pad_stride = 0;
    const int model = h->cfg.model;
    const bool racing = is_racing_model(model);
    if (!racing && !is_nav2d(model)) return;
    if (!h->model.params_set || !h->model.map_cells[0] || (racing && !h->model.map_cells[1])) return;
    const MapView &a = h->model.ctx.maps[0], &b = h->model.ctx.maps[1];
    if (racing && (a.nx != b.nx || a.ny != b.ny || a.cell != b.cell || a.ox != b.ox || a.oy != b.oy)) return;
    const float* P = h->model.ctx.P;
    const float xlo = P[racing ? MPPI_RP_XLO : MPPI_NP_XLO], xhi = P[racing ? MPPI_RP_XHI : MPPI_NP_XHI];
    const float ylo = P[racing ? MPPI_RP_YLO : MPPI_NP_YLO], yhi = P[racing ? MPPI_RP_YHI : MPPI_NP_YHI];
    uint32_t koff = 0;
    if (!pad_map_plan(a, xlo, xhi, ylo, yhi, koff)) return;
    const size_t n = (size_t)(a.nx + 1) * (a.ny + 1);
    if (h->model.map_pad.n < n && h->model.map_pad.alloc(n) != hipSuccess) return;
    hipLaunchKernelGGL(pad_map_kernel, dim3((unsigned)((a.ny + 1 + BLOCK - 1) / BLOCK), (unsigned)(a.nx + 1)), dim3(BLOCK), 0, s,
                       h->model.map_cells[0], racing ? h->model.map_cells[1] : (const uint8_t*)nullptr, a.nx, a.ny,
                       (uint8_t)(racing ? 2 : 1), h->model.map_pad);
    if (hipGetLastError() != hipSuccess) return;
    h->model.ctx.pad = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(h->model.map_pad.p) - (uintptr_t)koff);
    h->model.ctx.pad_stride = a.ny + 1;
}

// (re)allocate the grid of `slot` and fill in its geometry
int prepare_map(mppi_handle_t h, int slot, int nx, int ny, float cell, float ox, float oy) {
    if (!h || slot < 0 || slot > 1 || nx < 1 || ny < 1 || !(cell > 0.0f)) return fail(h, MPPI_E_INVALID, "bad map");
    if (is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "a learned-dynamics handle has no maps");  // (maps[0] carries its reference)
    const size_t n = (size_t)nx * ny;
    if (h->model.map_cells[slot].n < n) HIP_TRY(h, h->model.map_cells[slot].alloc(n));
    MapView& m = h->model.ctx.maps[slot];
    m.cells = h->model.map_cells[slot];
    m.nx = nx; m.ny = ny; m.cell = cell; m.ox = ox; m.oy = oy;
    // Markstein division needs y = RN(1/cell) and a significand of cell that is not all ones.
    uint32_t bits; std::memcpy(&bits, &cell, 4);
    const bool all_ones = (bits & 0x7fffffu) == 0x7fffffu;
    m.inv_cell = all_ones ? 0.0f : 1.0f / cell;  // host IEEE division: correctly rounded
    return MPPI_OK;
}

// small integer table host -> device (map recipes); blocking, setup path only
static int upload_ints(mppi_handle_t h, const int32_t* src, size_t count, DevBuf<int32_t>& dst) {
    if (!count) return MPPI_OK;
    HIP_TRY(h, dst.alloc(count));
    HIP_TRY(h, hipMemcpy(dst, src, sizeof(int32_t) * count, hipMemcpyHostToDevice));
    return MPPI_OK;
}

// Make sure the step table holds `rows` rows (blocking reallocation: set-up path).  The table may have two writers, so a
// larger buffer starts from the old one's rows (the stride is the same: they keep their places) and from at least T + 1
// rows, so that the racing tick's window rows do not move a T-row disc part.
int reserve_step_table(mppi_handle_t h, int rows) {
    auto& m = h->model;
    const size_t stride = (size_t)step_layout(h->cfg.model).stride;
    if ((size_t)rows * stride <= m.ref.n) return MPPI_OK;
    if (m.ref) HIP_TRY(h, hipDeviceSynchronize());
    DevBuf<float> grown;
    const size_t floats = stride * (size_t)std::max(rows, h->d.T + 1);
    HIP_TRY(h, grown.alloc(floats));
    HIP_TRY(h, hipMemset(grown, 0, sizeof(float) * floats));
    if (m.ref) HIP_TRY(h, hipMemcpy(grown, m.ref, sizeof(float) * m.ref.n, hipMemcpyDeviceToDevice));
    m.ref = std::move(grown);  // (swaps: the old buffer is freed with `grown`)
    if (m.ctx.ref) m.ctx.ref = m.ref;
    return MPPI_OK;
}

// Aim ctx.ref at the step table once every part its layout has has been written (check_ready names what is missing
// until then); ref_rows = the rows all of them cover.
void publish_step_table(mppi_handle_t h) {
    auto& m = h->model;
    const StepLayout L = step_layout(h->cfg.model);
    const int rows = !L.has_discs() ? m.ref_part_rows : !L.has_ref() ? m.disc_part_rows : std::min(m.ref_part_rows, m.disc_part_rows);
    m.ctx.ref = rows > 0 ? m.ref.p : nullptr;
    m.ctx.ref_rows = rows;
}
// the reference part of the table has `rows` rows now
static void reference_written(mppi_handle_t h, int rows) {
    h->model.ref_part_rows = rows;
    publish_step_table(h);
}

// `rows` rows of `width` floats from rows `spitch` floats apart to rows `dpitch` floats apart: between a contiguous block
// and one part of the step table, in either direction.  One plain copy where both sides are contiguous.
static hipError_t copy_rows(float* dst, size_t dpitch, const float* src, size_t spitch, size_t width, int rows, hipMemcpyKind kind,
                            hipStream_t s) {
    if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, sizeof(float) * width * (size_t)rows, kind, s);
    return hipMemcpy2DAsync(dst, sizeof(float) * dpitch, src, sizeof(float) * spitch, sizeof(float) * width, (size_t)rows, kind, s);
}

// value `f` of the padded table [rows][8][4] from the caller's [rows][n][4]: slots past n hold {0, 0, r2 = -1, w = 0}
__host__ __device__ inline float disc_padded(const float* discs, int n, size_t f) {
    const size_t t = f / DISC_ROW;
    const int j = (int)(f % DISC_ROW) / DISC_FLOATS, c = (int)(f % DISC_FLOATS);
    if (j < n) return discs[(t * n + j) * DISC_FLOATS + c];
    return c == 2 ? DISC_PAD_R2 : c == 3 ? DISC_PAD_W : 0.0f;
}

// mppi_set_discs from a device table: the padding, in stream order (one thread per value of the padded rows), into the
// disc part of the step rows (`stride` floats per row, the discs from float `off`); the other floats of a row are not touched
__global__ __launch_bounds__(BLOCK) void disc_rows_strided_kernel(const float* __restrict__ discs, int rows, int n,
                                                                  float* __restrict__ out, int stride, int off) {
    const size_t f = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f < (size_t)rows * DISC_ROW) out[(f / DISC_ROW) * (size_t)stride + off + f % DISC_ROW] = disc_padded(discs, n, f);
}

// the soft disc models' skirt: keep the pair as it was given and form the two coefficients of the rule (mppi_discs.hpp) in
// double, each rounded once
void apply_disc_softness(mppi_handle_t h, float reach, float skirt) {
    const double kappa = (double)reach * (double)reach, phi = (double)skirt;
    h->model.soft_reach = reach; h->model.soft_skirt = skirt;
    set_disc_soft(h->model.ctx, h->cfg.model, (float)(phi * kappa / (kappa - 1.0)), (float)(phi / (kappa - 1.0)));
}

// The flags word of a learned-dynamics handle (ctx.ref_rows) has this one writer: the architecture flags of the weight table
// and the angular mask are kept apart on the handle and composed here, so mppi_set_mlp / mppi_set_mlp_ensemble and
// mppi_set_mlp_angular may come in either order.
void publish_mlp_flags(mppi_handle_t h) {
    h->model.ctx.ref_rows = mlp_flags_word(h->model.mlp_arch, h->model.mlp_angular, h->model.mlp_value_set ? h->model.mlp_value_flags : 0);
}
void publish_mlp_reference(mppi_handle_t h) {
    set_mlp_reference(h->model.ctx, h->model.mlp_ref_rows > 0 ? h->model.mlp_ref.p : nullptr);
}
void publish_mlp_value(mppi_handle_t h) {
    set_mlp_value(h->model.ctx, h->model.mlp_value_set ? h->model.mlp_value.p : nullptr, h->model.mlp_value_weight);
    publish_mlp_flags(h);
}
static int mlp_arch_flags(int hidden_layers, int activation, int residual) {
    return (hidden_layers == 2 ? MLP_TWO_LAYERS : 0) | (activation == MPPI_MLP_TANH ? MLP_TANH : 0) | (residual ? MLP_RESIDUAL : 0);
}

}  // namespace mppi

extern "C" {

int mppi_set_model_params(mppi_handle_t h, const float* p, int n) {
    if (!h || n < 0 || n > MPPI_MAX_PARAMS || (n > 0 && !p)) return fail(h, MPPI_E_INVALID, "bad params");
    if (n != model_param_count(h->cfg.model)) return fail(h, MPPI_E_INVALID, "parameter count does not match the model");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD constants: roll it out first
    for (int i = 0; i < n; ++i) h->model.ctx.P[i] = p[i];
    const float* um = h->cfg.u_min; const float* uM = h->cfg.u_max;
    if (h->cfg.model == MPPI_MODEL_GOALZONE) {
        h->model.ctx.u_in_bounds = (um[0] >= p[MPPI_GP_VMIN] && uM[0] <= p[MPPI_GP_VMAX] && um[1] >= p[MPPI_GP_WMIN] &&
                              uM[1] <= p[MPPI_GP_WMAX]) ? 1 : 0;
        const float w = std::fmax(std::fabs(p[MPPI_GP_WMIN]), std::fabs(p[MPPI_GP_WMAX]));
        h->model.ctx.wrap_safe = (w * std::fabs(p[MPPI_GP_DT]) < 3.0f) ? 1 : 0;
    }
    if (is_nav2d(h->cfg.model)) {
        h->model.ctx.u_in_bounds = (um[0] >= p[MPPI_NP_VMIN] && uM[0] <= p[MPPI_NP_VMAX] && um[1] >= p[MPPI_NP_WMIN] &&
                              uM[1] <= p[MPPI_NP_WMAX]) ? 1 : 0;
        const float w = std::fmax(std::fabs(p[MPPI_NP_WMIN]), std::fabs(p[MPPI_NP_WMAX]));
        h->model.ctx.wrap_safe = (w * std::fabs(p[MPPI_NP_DT]) < 3.0f) ? 1 : 0;
    }
    if (is_racing_model(h->cfg.model)) {
        h->model.ctx.u_in_bounds = (um[0] >= p[MPPI_RP_AMIN] && uM[0] <= p[MPPI_RP_AMAX] && um[1] >= p[MPPI_RP_SMIN] &&
                              uM[1] <= p[MPPI_RP_SMAX]) ? 1 : 0;
        const float sm = std::fmax(std::fabs(p[MPPI_RP_SMIN]), std::fabs(p[MPPI_RP_SMAX]));
        const float dth = std::fabs(p[MPPI_RP_VMAX]) * std::tan(std::fmin(sm, 1.5f)) / std::fabs(p[MPPI_RP_L]) *
                          std::fabs(p[MPPI_RP_DT]);
        h->model.ctx.wrap_safe = (sm < 1.5f && dth < 3.0f) ? 1 : 0;
        h->model.ctx.tan_small = (std::fabs(p[MPPI_RP_SMIN]) <= 0.25f && std::fabs(p[MPPI_RP_SMAX]) <= 0.25f) ? 1 : 0;
        const float L = p[MPPI_RP_L];
        uint32_t bits; std::memcpy(&bits, &L, 4);
        h->model.ctx.inv_L = (L > 0.0f && (bits & 0x7fffffu) != 0x7fffffu) ? 1.0f / L : 0.0f;
        h->model.ctx.unit_L = L == 1.0f ? 1 : 0;
    }
    h->model.params_set = true;
    refresh_pad(h, nullptr);  // the padded grid depends on the position clamp limits
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(h, MPPI_E_HIP, "padded grid construction failed");
    return MPPI_OK;
}

int mppi_upload_map(mppi_handle_t h, int slot, const uint8_t* cells, int nx, int ny, float cell, float ox, float oy) {
    if (!h || !cells) return fail(h, MPPI_E_INVALID, "bad map");
    const size_t n = (size_t)(nx > 0 ? nx : 0) * (ny > 0 ? ny : 0);
    for (size_t i = 0; i < n; ++i)
        if (cells[i] > 1) return fail(h, MPPI_E_INVALID, "map cells must be 0/1 occupancy");
    if (int rc = settle_state_seq(h)) return rc;  // (a pending state sequence keeps the kernel variant of ITS solve)
    if (int rc = prepare_map(h, slot, nx, ny, cell, ox, oy)) return rc;
    HIP_TRY(h, hipMemcpy(h->model.map_cells[slot], cells, n, hipMemcpyHostToDevice));
    refresh_pad(h, nullptr);
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    return MPPI_OK;
}

int mppi_build_obstacle_map(mppi_handle_t h, int slot, int nx, int ny, float cell, float ox, float oy,
                            const int32_t* circles, int n_circles, const int32_t* rects, int n_rects, void* stream) {
    if (!h || n_circles < 0 || n_rects < 0 || (n_circles && !circles) || (n_rects && !rects))
        return fail(h, MPPI_E_INVALID, "bad obstacle list");
    for (int c = 0; c < n_circles; ++c)
        if (circles[3 * c + 2] < 0) return fail(h, MPPI_E_INVALID, "circle radius must be >= 0 cells");
    if (int rc = settle_state_seq(h)) return rc;  // (a pending state sequence keeps the kernel variant of ITS solve)
    if (int rc = prepare_map(h, slot, nx, ny, cell, ox, oy)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DevBuf<int32_t> dc, dr;  // (the recipe tables, freed on return)
    if (int rc = upload_ints(h, circles, (size_t)3 * n_circles, dc)) return rc;
    if (int rc = upload_ints(h, rects, (size_t)4 * n_rects, dr)) return rc;
    hipLaunchKernelGGL(mppi::raster_obstacles_kernel, dim3((ny + mppi::BLOCK - 1) / mppi::BLOCK, nx), dim3(mppi::BLOCK), 0,
                       s, h->model.map_cells[slot].p, nx, ny, dc.p, n_circles, dr.p, n_rects);
    const hipError_t e = hipGetLastError();
    refresh_pad(h, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // (before the recipe tables are freed)
    HIP_TRY(h, e);
    HIP_TRY(h, e2);
    return MPPI_OK;
}

int mppi_build_lane_map(mppi_handle_t h, int slot, int nx, int ny, float cell, float ox, float oy,
                        const int32_t* seeds, int n_seeds, int64_t max_d2, void* stream) {
    if (!h || n_seeds < 1 || !seeds || max_d2 < 0) return fail(h, MPPI_E_INVALID, "bad lane seeds");
    if (int rc = settle_state_seq(h)) return rc;  // (a pending state sequence keeps the kernel variant of ITS solve)
    if (int rc = prepare_map(h, slot, nx, ny, cell, ox, oy)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DevBuf<int32_t> ds;  // (freed on return)
    if (int rc = upload_ints(h, seeds, (size_t)2 * n_seeds, ds)) return rc;
    hipLaunchKernelGGL(mppi::lane_map_kernel, dim3((ny + mppi::BLOCK - 1) / mppi::BLOCK, nx), dim3(mppi::BLOCK), 0, s,
                       h->model.map_cells[slot].p, nx, ny, ds.p, n_seeds, max_d2);
    const hipError_t e = hipGetLastError();
    refresh_pad(h, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // (before the seed table is freed)
    HIP_TRY(h, e);
    HIP_TRY(h, e2);
    return MPPI_OK;
}

int mppi_download_map(mppi_handle_t h, int slot, uint8_t* cells_host, int* nx, int* ny) {
    if (!h || slot < 0 || slot > 1) return fail(h, MPPI_E_INVALID, "bad slot");
    if (!h->model.map_cells[slot]) return fail(h, MPPI_E_STATE, "map slot is empty");
    const MapView& m = h->model.ctx.maps[slot];
    if (nx) *nx = m.nx;
    if (ny) *ny = m.ny;
    if (cells_host) {
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemcpy(cells_host, h->model.map_cells[slot], (size_t)m.nx * m.ny, hipMemcpyDeviceToHost));
    }
    return MPPI_OK;
}

int mppi_set_reference(mppi_handle_t h, const float* ref, int rows, void* stream) {
    if (!h || !ref || rows < 1) return fail(h, MPPI_E_INVALID, "bad reference");
    if (is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "a learned-dynamics handle has no reference window");
    const StepLayout L = step_layout(h->cfg.model);
    if (!L.has_ref())
        return fail(h, MPPI_E_INVALID, L.has_discs() ? "a moving-disc handle has no reference window" : "the reference window belongs to the racing models");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = reserve_step_table(h, rows)) return rc;
    float* st = nullptr; hipEvent_t ev = nullptr;
    if (int rc = stage_slot(h, (size_t)rows * 8, &st, &ev)) return rc;
    for (int i = 0; i < rows; ++i) {
        float* o = st + (size_t)i * 8;
        o[0] = ref[4 * i]; o[1] = ref[4 * i + 1]; o[2] = ref[4 * i + 2]; o[3] = ref[4 * i + 3];
        o[4] = sinf(o[2]); o[5] = cosf(o[2]);  // torch.sin/cos of the fp32 scalar, racing.py:127-139
        o[6] = o[7] = 0.0f;
    }
    HIP_TRY(h, copy_rows(h->model.ref, L.stride, st, L.ref_floats, L.ref_floats, rows, hipMemcpyHostToDevice, s));  // (discs behind the row stay)
    HIP_TRY(h, hipEventRecord(ev, s));
    reference_written(h, rows);
    return MPPI_OK;
}

int mppi_set_mlp(mppi_handle_t h, const float* table, int n_floats, int hidden_layers, int activation, int residual,
                 void* stream) {
    if (!h || !table) return fail(h, MPPI_E_INVALID, "bad weight table");
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the weight table belongs to the learned-dynamics models");
    if (n_floats != mlp_table_len(h)) return fail(h, MPPI_E_INVALID, "weight table: wrong number of values for this model");
    if (hidden_layers < 1 || hidden_layers > 2 || (activation != MPPI_MLP_RELU && activation != MPPI_MLP_TANH) ||
        (residual != 0 && residual != 1))
        return fail(h, MPPI_E_INVALID, "weight table: hidden_layers 1 or 2, activation relu or tanh, residual 0 or 1");
    for (int i = 0; i < n_floats; ++i)
        if (!std::isfinite(table[i])) return fail(h, MPPI_E_INVALID, "weight table: every value must be finite");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD weights: roll it out first
    hipStream_t s = (hipStream_t)stream;
    if (!h->model.mlp) HIP_TRY(h, h->model.mlp.alloc((size_t)n_floats));
    float* st = nullptr; hipEvent_t ev = nullptr;
    if (int rc = stage_slot(h, (size_t)n_floats, &st, &ev)) return rc;
    std::memcpy(st, table, sizeof(float) * (size_t)n_floats);
    HIP_TRY(h, hipMemcpyAsync(h->model.mlp, st, sizeof(float) * (size_t)n_floats, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(ev, s));
    h->model.ctx.ref = h->model.mlp;
    h->model.mlp_arch = mlp_arch_flags(hidden_layers, activation, residual);
    publish_mlp_flags(h);
    h->model.mlp_members = 1; h->model.mlp_nominal = 0;  // (an ensemble of one, in the front of whatever the buffer holds)
    return MPPI_OK;
}

// one member's table through the staging ring into its place in the buffer, in stream order
static int upload_mlp_member(mppi_handle_t h, int e, const float* table, int n_floats, hipStream_t s) {
    float* st = nullptr; hipEvent_t ev = nullptr;
    if (int rc = stage_slot(h, (size_t)n_floats, &st, &ev)) return rc;
    std::memcpy(st, table, sizeof(float) * (size_t)n_floats);
    HIP_TRY(h, hipMemcpyAsync(h->model.mlp.p + (size_t)e * (size_t)n_floats, st, sizeof(float) * (size_t)n_floats, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(ev, s));
    return MPPI_OK;
}

int mppi_set_mlp_ensemble(mppi_handle_t h, const float* tables, int n_members, int n_floats, int hidden_layers, int activation,
                          int residual, int nominal, void* stream) {
    if (!h || !tables) return fail(h, MPPI_E_INVALID, "bad weight tables");
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the weight tables belong to the learned-dynamics models");
    if (n_members < 1 || n_members > MPPI_MAX_PARTICLES)
        return fail(h, MPPI_E_INVALID, "weight tables: 1 <= n_members <= MPPI_MAX_PARTICLES (16)");
    if (nominal < 0 || nominal >= n_members) return fail(h, MPPI_E_INVALID, "weight tables: the nominal member is one of the n_members");
    if (n_floats != mlp_table_len(h)) return fail(h, MPPI_E_INVALID, "weight table: wrong number of values for this model");
    if (hidden_layers < 1 || hidden_layers > 2 || (activation != MPPI_MLP_RELU && activation != MPPI_MLP_TANH) ||
        (residual != 0 && residual != 1))
        return fail(h, MPPI_E_INVALID, "weight table: hidden_layers 1 or 2, activation relu or tanh, residual 0 or 1");
    const size_t total = (size_t)n_members * (size_t)n_floats;
    for (size_t i = 0; i < total; ++i)
        if (!std::isfinite(tables[i])) return fail(h, MPPI_E_INVALID, "weight table: every value must be finite");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD weights: roll it out first
    hipStream_t s = (hipStream_t)stream;
    if (h->model.mlp.n < total) {  // (blocking: earlier launches may still read the old buffer)
        HIP_TRY(h, hipDeviceSynchronize());
        h->model.ctx.ref = nullptr; h->model.mlp_members = 0;
        HIP_TRY(h, h->model.mlp.alloc(total));
    }
    for (int e = 0; e < n_members; ++e)
        if (int rc = upload_mlp_member(h, e, tables + (size_t)e * (size_t)n_floats, n_floats, s)) return rc;
    h->model.mlp_members = n_members; h->model.mlp_nominal = nominal;
    h->model.ctx.ref = h->model.mlp.p + (size_t)nominal * (size_t)n_floats;
    h->model.mlp_arch = mlp_arch_flags(hidden_layers, activation, residual);
    publish_mlp_flags(h);
    return MPPI_OK;
}

int mppi_set_mlp_member(mppi_handle_t h, int e, const float* table, int n_floats, void* stream) {
    if (!h || !table) return fail(h, MPPI_E_INVALID, "bad weight table");
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the weight table belongs to the learned-dynamics models");
    if (!h->model.ctx.ref || h->model.mlp_members < 1)
        return fail(h, MPPI_E_STATE, "no weight table: call mppi_set_mlp or mppi_set_mlp_ensemble first");
    if (e < 0 || e >= h->model.mlp_members) return fail(h, MPPI_E_INVALID, "weight table: no such member");
    if (n_floats != mlp_table_len(h)) return fail(h, MPPI_E_INVALID, "weight table: wrong number of values for this model");
    for (int i = 0; i < n_floats; ++i)
        if (!std::isfinite(table[i])) return fail(h, MPPI_E_INVALID, "weight table: every value must be finite");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD weights: roll it out first
    return upload_mlp_member(h, e, table, n_floats, (hipStream_t)stream);
}

int mppi_set_mlp_nominal(mppi_handle_t h, int e) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the nominal member belongs to the learned-dynamics models");
    if (!h->model.ctx.ref || h->model.mlp_members < 1)
        return fail(h, MPPI_E_STATE, "no weight table: call mppi_set_mlp or mppi_set_mlp_ensemble first");
    if (e < 0 || e >= h->model.mlp_members) return fail(h, MPPI_E_INVALID, "nominal member: no such member");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD nominal member
    h->model.mlp_nominal = e;
    h->model.ctx.ref = h->model.mlp.p + (size_t)e * (size_t)mlp_table_len(h);
    return MPPI_OK;
}

int mppi_get_mlp_ensemble(mppi_handle_t h, int* n_members_out, int* nominal_out) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the weight tables belong to the learned-dynamics models");
    if (n_members_out) *n_members_out = h->model.ctx.ref ? h->model.mlp_members : 0;
    if (nominal_out) *nominal_out = h->model.mlp_nominal;
    return MPPI_OK;
}

int mppi_set_mlp_reference(mppi_handle_t h, const float* rows, int n_rows, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the tracking reference belongs to the learned-dynamics models");
    if (n_rows < 0) return fail(h, MPPI_E_INVALID, "tracking reference: n_rows >= 0");
    auto& m = h->model;
    if (!rows || n_rows == 0) {  // off: the cost reads goal and q from the parameters again
        m.mlp_ref_rows = 0;
        publish_mlp_reference(h);
        return MPPI_OK;
    }
    const size_t floats = (size_t)n_rows * 2 * (size_t)h->ds;
    if (!on_device)
        for (size_t i = 0; i < floats; ++i)
            if (!std::isfinite(rows[i])) return fail(h, MPPI_E_INVALID, "tracking reference: every value must be finite");
    hipStream_t s = (hipStream_t)stream;
    if (m.mlp_ref.n < floats) {  // (blocking: earlier launches may still read the old buffer)
        HIP_TRY(h, hipDeviceSynchronize());
        m.mlp_ref_rows = 0;
        publish_mlp_reference(h);
        HIP_TRY(h, m.mlp_ref.alloc(floats));
    }
    if (on_device) {
        HIP_TRY(h, hipMemcpyAsync(m.mlp_ref, rows, sizeof(float) * floats, hipMemcpyDeviceToDevice, s));
    } else {
        float* st = nullptr; hipEvent_t ev = nullptr;
        if (int rc = stage_slot(h, floats, &st, &ev)) return rc;
        std::memcpy(st, rows, sizeof(float) * floats);
        HIP_TRY(h, hipMemcpyAsync(m.mlp_ref, st, sizeof(float) * floats, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipEventRecord(ev, s));
    }
    m.mlp_ref_rows = n_rows;
    publish_mlp_reference(h);
    return MPPI_OK;
}

int mppi_get_mlp_reference(mppi_handle_t h, float* out, int* n_rows_out, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the tracking reference belongs to the learned-dynamics models");
    const int n_rows = h->model.mlp_ref_rows;
    if (n_rows_out) *n_rows_out = n_rows;
    if (!out || n_rows == 0) return MPPI_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipMemcpyAsync(out, h->model.mlp_ref, sizeof(float) * (size_t)n_rows * 2 * (size_t)h->ds,
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!on_device) HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

int mppi_set_mlp_angular(mppi_handle_t h, uint32_t mask) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the angular mask belongs to the learned-dynamics models");
    if (mask >> h->ds) return fail(h, MPPI_E_INVALID, "angular mask: a bit at or above the model's state width");
    h->model.mlp_angular = mask;
    publish_mlp_flags(h);
    return MPPI_OK;
}

int mppi_get_mlp_angular(mppi_handle_t h, uint32_t* mask_out) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the angular mask belongs to the learned-dynamics models");
    if (mask_out) *mask_out = h->model.mlp_angular;
    return MPPI_OK;
}

int mppi_set_mlp_value(mppi_handle_t h, const float* table, int n_floats, int hidden_layers, int activation, float weight,
                       int replace_terminal, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the terminal value belongs to the learned-dynamics models");
    auto& m = h->model;
    if (!table) {  // off: the terminal cost is the quadratic again
        m.mlp_value_set = false; m.mlp_value_flags = 0; m.mlp_value_weight = 0.0f;
        publish_mlp_value(h);
        return MPPI_OK;
    }
    if (n_floats != mlp_value_floats(h->ds)) return fail(h, MPPI_E_INVALID, "value table: wrong number of values for this model");
    if (hidden_layers < 1 || hidden_layers > 2 || (activation != MPPI_MLP_RELU && activation != MPPI_MLP_TANH) ||
        (replace_terminal != 0 && replace_terminal != 1))
        return fail(h, MPPI_E_INVALID, "value table: hidden_layers 1 or 2, activation relu or tanh, replace_terminal 0 or 1");
    if (!std::isfinite(weight)) return fail(h, MPPI_E_INVALID, "value table: the weight must be finite");
    for (int i = 0; i < n_floats; ++i)
        if (!std::isfinite(table[i])) return fail(h, MPPI_E_INVALID, "value table: every value must be finite");
    hipStream_t s = (hipStream_t)stream;
    if (!m.mlp_value) HIP_TRY(h, m.mlp_value.alloc((size_t)n_floats));
    float* st = nullptr; hipEvent_t ev = nullptr;
    if (int rc = stage_slot(h, (size_t)n_floats, &st, &ev)) return rc;
    std::memcpy(st, table, sizeof(float) * (size_t)n_floats);
    HIP_TRY(h, hipMemcpyAsync(m.mlp_value, st, sizeof(float) * (size_t)n_floats, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(ev, s));
    m.mlp_value_set = true;
    m.mlp_value_flags = (hidden_layers == 2 ? MLP_VALUE_TWO_LAYERS : 0) | (activation == MPPI_MLP_TANH ? MLP_VALUE_TANH : 0) |
                        (replace_terminal ? MLP_VALUE_REPLACE : 0);
    m.mlp_value_weight = weight;
    publish_mlp_value(h);
    return MPPI_OK;
}

int mppi_get_mlp_value(mppi_handle_t h, float* out, int* n_floats_out, int* hidden_layers_out, int* activation_out,
                       float* weight_out, int* replace_terminal_out, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the terminal value belongs to the learned-dynamics models");
    const auto& m = h->model;
    const int n = m.mlp_value_set ? mlp_value_floats(h->ds) : 0;
    if (n_floats_out) *n_floats_out = n;
    if (hidden_layers_out) *hidden_layers_out = n == 0 ? 0 : (m.mlp_value_flags & MLP_VALUE_TWO_LAYERS) ? 2 : 1;
    if (activation_out) *activation_out = (m.mlp_value_flags & MLP_VALUE_TANH) ? MPPI_MLP_TANH : MPPI_MLP_RELU;
    if (weight_out) *weight_out = m.mlp_value_weight;
    if (replace_terminal_out) *replace_terminal_out = (m.mlp_value_flags & MLP_VALUE_REPLACE) ? 1 : 0;
    if (!out || n == 0) return MPPI_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipMemcpyAsync(out, m.mlp_value, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

int mppi_set_discs(mppi_handle_t h, const float* discs, int rows, int n, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!has_discs(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the disc table belongs to the moving-disc models");
    if (rows < 1 || n < 0 || n > MPPI_MAX_DISCS || (n > 0 && !discs))
        return fail(h, MPPI_E_INVALID, "disc table: rows >= 1 and 0 <= n <= 8 discs per row");
    const size_t in_floats = (size_t)rows * n * DISC_FLOATS, floats = (size_t)rows * DISC_ROW;
    if (!on_device)
        for (size_t i = 0; i < in_floats; ++i)
            if (!std::isfinite(discs[i]) || (i % DISC_FLOATS == 3 && discs[i] < 0.0f))
                return fail(h, MPPI_E_INVALID, "disc table: every value must be finite and every penalty >= 0");
    if (!on_device && is_soft_discs(h->cfg.model))  // (the soft rule divides by r2)
        for (size_t i = 2; i < in_floats; i += DISC_FLOATS)
            if (!(discs[i] > 0.0f)) return fail(h, MPPI_E_INVALID, "disc table: a soft disc model needs r2 > 0 for every disc");
    hipStream_t s = (hipStream_t)stream;
    const StepLayout L = step_layout(h->cfg.model);
    if (int rc = reserve_step_table(h, rows)) return rc;
    if (on_device) {
        hipLaunchKernelGGL(disc_rows_strided_kernel, dim3((unsigned)((floats + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, discs, rows, n,
                           h->model.ref.p, L.stride, L.disc_off);
        HIP_TRY(h, hipGetLastError());
    } else {
        float* st = nullptr; hipEvent_t ev = nullptr;
        if (int rc = stage_slot(h, floats, &st, &ev)) return rc;
        for (size_t f = 0; f < floats; ++f) st[f] = disc_padded(discs, n, f);
        HIP_TRY(h, copy_rows(h->model.ref.p + L.disc_off, L.stride, st, DISC_ROW, DISC_ROW, rows, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipEventRecord(ev, s));
    }
    h->model.disc_part_rows = rows;
    set_disc_count(h->model.ctx, h->cfg.model, n);  // (disc_count: mppi_models.hpp)
    publish_step_table(h);
    return MPPI_OK;
}

int mppi_get_discs(mppi_handle_t h, float* out, int* rows_out, int* n_out, int on_device, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!has_discs(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the disc table belongs to the moving-disc models");
    const StepLayout L = step_layout(h->cfg.model);
    const int rows = h->model.disc_part_rows;  // (the discs may be there before the window is)
    if (rows < 1) return fail(h, MPPI_E_STATE, "no disc table: call mppi_set_discs first");
    if (rows_out) *rows_out = rows;
    if (n_out) *n_out = disc_count(h->model.ctx, h->cfg.model);
    if (!out) return MPPI_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, copy_rows(out, DISC_ROW, h->model.ref.p + L.disc_off, L.stride, DISC_ROW, rows,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!on_device) HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

int mppi_set_disc_softness(mppi_handle_t h, float reach, float skirt) {
    if (!h) return MPPI_E_INVALID;
    if (!is_soft_discs(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the skirt belongs to the soft moving-disc models");
    if (!std::isfinite(reach) || !(reach > 1.0f) || !(skirt >= 0.0f && skirt <= 1.0f))
        return fail(h, MPPI_E_INVALID, "disc softness: reach finite and > 1, skirt in [0, 1]");
    if (int rc = settle_state_seq(h)) return rc;  // a lazily completed state sequence belongs to the OLD constants: roll it out first
    apply_disc_softness(h, reach, skirt);
    return MPPI_OK;
}

int mppi_get_disc_softness(mppi_handle_t h, float* reach, float* skirt) {
    if (!h) return MPPI_E_INVALID;
    if (!is_soft_discs(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the skirt belongs to the soft moving-disc models");
    if (reach) *reach = h->model.soft_reach;
    if (skirt) *skirt = h->model.soft_skirt;
    return MPPI_OK;
}

int mppi_set_center_path(mppi_handle_t h, const float* path_host, int n, const int32_t* dind_host, int rows,
                         float v_target) {
    if (!h || !path_host || !dind_host || n < 1 || rows < 1) return fail(h, MPPI_E_INVALID, "bad centre path");
    if (!is_racing_model(h->cfg.model)) return fail(h, MPPI_E_INVALID, "the reference window belongs to the racing models");
    if (rows < h->d.T) return fail(h, MPPI_E_INVALID, "window shorter than the horizon");
    for (int i = 0; i < rows; ++i)
        if (dind_host[i] < 0 || (i && dind_host[i] < dind_host[i - 1])) return fail(h, MPPI_E_INVALID, "window offsets must be >= 0 and non-decreasing");
    std::vector<float> tab((size_t)n * 8, 0.0f);
    for (int i = 0; i < n; ++i) {
        float* o = tab.data() + (size_t)i * 8;
        o[0] = path_host[3 * i]; o[1] = path_host[3 * i + 1]; o[2] = path_host[3 * i + 2];
        o[4] = sinf(o[2]); o[5] = cosf(o[2]);  // the calls mppi_set_reference makes per window row
    }
    HIP_TRY(h, hipDeviceSynchronize());
    h->model.center_n = 0;
    HIP_TRY(h, h->model.center8.alloc(tab.size()));
    HIP_TRY(h, hipMemcpy(h->model.center8, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, h->model.win_dind.alloc((size_t)rows));
    HIP_TRY(h, hipMemcpy(h->model.win_dind, dind_host, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice));
    if (!h->model.path_index) HIP_TRY(h, h->model.path_index.alloc_set(1, 0));
    if (int rc = reserve_step_table(h, rows)) return rc;
    h->model.center_n = n; h->model.win_rows = rows; h->model.win_v = v_target;
    return MPPI_OK;
}

int mppi_ref_window(mppi_handle_t h, const float* state_dev, void* stream) {
    if (!h) return MPPI_E_INVALID;
    if (!h->model.center_n) return fail(h, MPPI_E_STATE, "mppi_ref_window before mppi_set_center_path");
    const RefWindowCtx w{h->model.center8, h->model.win_dind, h->model.path_index, h->model.center_n, h->model.win_rows, h->model.win_v,
                         step_layout(h->cfg.model).stride};
    hipLaunchKernelGGL(ref_window_kernel, dim3(1), dim3(REFWIN_BLOCK), 0, (hipStream_t)stream, w,
                       state_dev ? state_dev : h->core.x0_cur, h->model.ref);
    HIP_TRY(h, hipGetLastError());
    reference_written(h, h->model.win_rows);
    return MPPI_OK;
}

int mppi_set_path_index(mppi_handle_t h, int32_t cind, void* stream) {
    if (!h || cind < 0) return fail(h, MPPI_E_INVALID, "bad path index");
    if (!h->model.path_index) return fail(h, MPPI_E_STATE, "mppi_set_path_index before mppi_set_center_path");
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(h, hipMemcpy(h->model.path_index, &cind, sizeof(int32_t), hipMemcpyHostToDevice));
    return MPPI_OK;
}

int mppi_get_path_index(mppi_handle_t h, int32_t* cind_out_host, void* stream) {
    if (!h || !cind_out_host) return fail(h, MPPI_E_INVALID, "null");
    if (!h->model.path_index) return fail(h, MPPI_E_STATE, "mppi_get_path_index before mppi_set_center_path");
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(h, hipMemcpy(cind_out_host, h->model.path_index, sizeof(int32_t), hipMemcpyDeviceToHost));
    return MPPI_OK;
}

int mppi_get_reference(mppi_handle_t h, float* ref_out, int rows, int on_device, void* stream) {
    if (!h || !ref_out || rows < 1) return fail(h, MPPI_E_INVALID, "bad get_reference arguments");
    if (is_mlp(h->cfg.model)) return fail(h, MPPI_E_INVALID, "a learned-dynamics handle has no reference window");
    const StepLayout L = step_layout(h->cfg.model);
    if (L.has_discs() && !L.has_ref()) return fail(h, MPPI_E_INVALID, "a moving-disc handle has no reference window");
    if (rows > h->model.ref_part_rows)  // (the window may be there before the discs are)
        return fail(h, MPPI_E_STATE, "no reference window of that many rows");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, copy_rows(ref_out, 4, h->model.ref, L.stride, 4, rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!on_device) HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

int mppi_model_step(int model, const float* params_host, int n_params, const float* u_min_host, const float* u_max_host,
                    const float* state_dev, const float* action_dev, float* next_state_dev, const float* goal_xy_host,
                    float goal_threshold, uint8_t* reached_out_dev, void* stream) {
    ModelDims md{};
    if (is_mlp(model)) return MPPI_E_INVALID;  // (no handle: nowhere to take the weight table from)
    if (!model_dims(model, md) || n_params < 0 || n_params > MPPI_MAX_PARAMS || (n_params && !params_host) ||
        !state_dev || !action_dev || !next_state_dev || (reached_out_dev && !goal_xy_host) || md.dc > MPPI_MAX_DIM_CONTROL)
        return MPPI_E_INVALID;
    if (n_params < model_param_count(model)) return MPPI_E_INVALID;  // (the cost weights at the tail are not read by the dynamics)
    ModelCtx ctx;
    std::memset(&ctx, 0, sizeof(ctx));
    for (int i = 0; i < n_params; ++i) ctx.P[i] = params_host[i];
    StepBounds ub;
    for (int k = 0; k < MPPI_MAX_DIM_CONTROL; ++k) {
        ub.lo[k] = (u_min_host && k < md.dc) ? u_min_host[k] : -INFINITY;
        ub.hi[k] = (u_max_host && k < md.dc) ? u_max_host[k] : INFINITY;
    }
    const float gx = goal_xy_host ? goal_xy_host[0] : 0.0f, gy = goal_xy_host ? goal_xy_host[1] : 0.0f;
    hipStream_t s = (hipStream_t)stream;
#define CALL_STEP(MODEL)                                                                              \
    hipLaunchKernelGGL((model_step_kernel<MODEL>), dim3(1), dim3(WAVE), 0, s, ctx, state_dev, action_dev, ub,  \
                       next_state_dev, gx, gy, goal_threshold, reached_out_dev)
    switch (model) {
    case MPPI_MODEL_PENDULUM: CALL_STEP(MPPI_MODEL_PENDULUM); break;
    case MPPI_MODEL_CARTPOLE: CALL_STEP(MPPI_MODEL_CARTPOLE); break;
    case MPPI_MODEL_MOUNTAINCAR: CALL_STEP(MPPI_MODEL_MOUNTAINCAR); break;
    case MPPI_MODEL_NAV2D: CALL_STEP(MPPI_MODEL_NAV2D); break;
    case MPPI_MODEL_RACING: CALL_STEP(MPPI_MODEL_RACING); break;
    case MPPI_MODEL_MJCARTPOLE: CALL_STEP(MPPI_MODEL_MJCARTPOLE); break;
    case MPPI_MODEL_GOALZONE: CALL_STEP(MPPI_MODEL_GOALZONE); break;
    case MPPI_MODEL_NAV2D_DISCS: CALL_STEP(MPPI_MODEL_NAV2D_DISCS); break;  // (nav2d's dynamics: the discs are cost only)
    case MPPI_MODEL_RACING_DISCS: CALL_STEP(MPPI_MODEL_RACING); break;      // (racing's dynamics, racing's kernel)
    case MPPI_MODEL_NAV2D_DISCS_SOFT: CALL_STEP(MPPI_MODEL_NAV2D); break;   // (nav2d's dynamics, nav2d's kernel)
    case MPPI_MODEL_RACING_DISCS_SOFT: CALL_STEP(MPPI_MODEL_RACING); break;
    }
#undef CALL_STEP
    return hipGetLastError() == hipSuccess ? MPPI_OK : MPPI_E_HIP;
}

int mppi_grid_lookup(const float* map_dev, int nx, int ny, float cell_size, float origin_x, float origin_y, const float* xy_dev,
                     int64_t n, int64_t stride, float* out_dev, void* stream) {
    if (!map_dev || !xy_dev || !out_dev || nx < 1 || ny < 1 || !(cell_size > 0.0f) || n < 0 || stride < 2) return MPPI_E_INVALID;
    if (n == 0) return MPPI_OK;
    hipLaunchKernelGGL(grid_lookup_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, map_dev, nx,
                       ny, cell_size, origin_x, origin_y, xy_dev, n, stride, out_dev);
    return hipGetLastError() == hipSuccess ? MPPI_OK : MPPI_E_HIP;
}

}  // extern "C"
