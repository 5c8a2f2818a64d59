// rk4_hip.hip -- the explicit integrators on a hip_proj context: RK4
// (rk4_impl, solver_rk4.c:69-259), RK2 (rk2_impl,
// solver_rk2.c:48-211) and explicit Euler (explicit_euler_impl,
// solver_explicit_euler.c:337-582), each with max_iter = 1 per step and
// bitwise the CPU scalar solver's fields. RK2 and Euler: see rk2_step_impl
// and euler_step_impl below. RK4:
//
// Per step: four fused stage kernels (k_rk_stage: RHS + stage update +
// running k1 + 2k2 + 2k3 sum, the stage derivatives stay in registers), the
// energy equation on the new velocity, the periodic boundary copies of
// apply_boundary_conditions (solver_explicit_euler.c:231-306) on u,v,w,p,
// rho,T, the thermal BCs, then one stats / NaN pass. Stage states ping-pong
// between the context's CG work arrays (u*,v*,w*,p_new and r,p_a,p_b,x_tmp);
// the final update is written in place over u,v,w,p.
#include "ctx.hpp"
#include "rk_kernels.hpp"
#include "../host/grid_spacing.h"

// stages: the running k sums and x_tmp (RK4 / RK2); explicit Euler needs neither
static cfd_status_t ensure_rk(hip_proj_ctx* c, bool stages) {
    const size_t n = field_elems(c);
    for (int q = 0; q < 4 && stages; ++q)
        if (!c->rk_acc[q]) ST_TRY(dalloc(c, &c->rk_acc[q], n));
    if (stages && !c->xt) ST_TRY(dalloc(c, &c->xt, n));
    if (!c->dxa) ST_TRY(dalloc(c, &c->dxa, c->nx));
    if (!c->dya) ST_TRY(dalloc(c, &c->dya, c->ny));
    if (!c->rho) {
        // no per-cell density supplied: uniform rho0 (what set_density sets)
        ST_TRY(dalloc(c, &c->rho, n));
        double* h = nullptr;
        HIP_TRY(hipHostMalloc((void**)&h, n * sizeof(double), hipHostMallocDefault));
        for (size_t e = 0; e < n; ++e) h[e] = c->rho0;
        hipError_t e1 = hipMemcpyAsync(c->rho, h, n * sizeof(double), hipMemcpyHostToDevice,
                                       c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        hipHostFree(h);
        HIP_TRY(e1);
        HIP_TRY(e2);
    }
    return CFD_SUCCESS;
}

template <int S>
static void launch_stage(hip_proj_ctx* c, bool buoy, const RkCoef& rc, const Fld4& cur,
                         const Fld4& q0, const Fld4& acc, const Fld4& out) {
    auto go = [&](auto kern, dim3 grid) {
        klaunch(c, kern, grid, dim3(256), c->geo, rc, cur, q0, acc, out, c->rho, c->T, c->dxa,
                c->dya, c->src_u_row, c->src_v_col);
    };
    // x-pair stage kernel (default); CFD_HIP_RK_PAIR=0 selects the per-cell one
    if (c->env.rk_pair) {
        const dim3 g2((unsigned)((c->nx + 127) / 128), (unsigned)((c->ny + 3) / 4),
                      (unsigned)c->nz);
        with_bool(buoy, [&](auto B) { go(k_rk_stage2<S, B>, g2); });
    } else {
        with_bool(buoy, [&](auto B) { go(k_rk_stage<S, B>, cell_grid(c)); });
    }
}

static cfd_status_t step_tail(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                              ns_solver_stats_t* stats, bool velocity_bcs, const char* nan_msg);

// What every integrator here does before its kernels: refusals and
// validation (`who` prefixes the messages), the lazily allocated arrays
// (stages: the k sums and the second stage buffer set), the per-index
// spacing and the compute_source_terms tables at `iter` with time step
// src_dt, and the RHS constants.
static cfd_status_t step_head(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                              int iter, const char* who, bool stages, double src_dt, RkCoef* rcp,
                              bool* buoyp) {
    if (!c) return CFD_ERROR_INVALID;
    char msg[128];
    if (c->nranks > 1) {
        snprintf(msg, sizeof(msg), "%s: Z-slab decomposition is not supported", who);
        set_err(CFD_ERROR_UNSUPPORTED, msg);
        return CFD_ERROR_UNSUPPORTED;
    }
    ST_TRY(ctx_validate_params(c, g, prm));
    HIP_TRY(hipSetDevice(c->device));
    const bool buoy = (prm->beta != 0.0);
    const bool energy = (prm->alpha > 0.0);
    if ((buoy || energy) && !c->have_T) {
        snprintf(msg, sizeof(msg), "%s: buoyancy / energy equation need the T field", who);
        set_err(CFD_ERROR_INVALID, msg);
        return CFD_ERROR_INVALID;
    }
    ST_TRY(ensure_rk(c, stages));
    const size_t nx = c->nx, ny = c->ny, nz = c->nzg;

    // per-index spacing and compute_source_terms tables (iter-dependent decay),
    // evaluated on the host with the reference's libm expressions
    // (the grid holds nx - 1 and ny - 1 spacings: grid_spacing.h fills the
    // last slot; the pinned staging is h_src's second half, which ev_src
    // guards together with the source tables)
    HIP_TRY(hipEventSynchronize(c->ev_src));
    double* hdx = c->h_src + nx + ny;
    double* hdy = hdx + nx;
    grid_stage_spacing(g, hdx, hdy);
    HIP_TRY(hipMemcpyAsync(c->dxa, hdx, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->dya, hdy, ny * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ns_solver_params_t ps = *prm;
    ps.dt = src_dt;
    ST_TRY(upload_source_tables(c, g, &ps, iter));

    RkCoef& rc = *rcp;
    rc.inv_2dz = (nz > 1 && g->dz) ? 1.0 / (2.0 * g->dz[0]) : 0.0;
    rc.inv_dz2 = (nz > 1 && g->dz) ? 1.0 / (g->dz[0] * g->dz[0]) : 0.0;
    rc.mu = prm->mu;
    rc.beta = prm->beta;
    rc.T_ref = prm->T_ref;
    rc.g0 = prm->gravity[0];
    rc.g1 = prm->gravity[1];
    rc.g2 = prm->gravity[2];
    rc.fac = 0.0;
    *buoyp = buoy;
    return CFD_SUCCESS;
}

static cfd_status_t rk4_step_impl(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                                  ns_solver_stats_t* stats, int iter) {
    RkCoef rc;
    bool buoy = false;
    ST_TRY(step_head(c, g, prm, iter, "rk4_hip", true, prm ? prm->dt : 0.0, &rc, &buoy));
    const double dt = prm->dt;
    const Fld4 q0{{c->u, c->v, c->w, c->p}};
    const Fld4 a{{c->us, c->vs, c->ws, c->pn}};
    const Fld4 b{{c->r, c->pa, c->pb, c->xt}};
    const Fld4 acc{{c->rk_acc[0], c->rk_acc[1], c->rk_acc[2], c->rk_acc[3]}};
    timed(c, HIP_KT_RK_STAGE, [&] {
        rc.fac = 0.5 * dt;
        launch_stage<0>(c, buoy, rc, q0, q0, acc, a);
    });
    timed(c, HIP_KT_RK_STAGE, [&] { launch_stage<1>(c, buoy, rc, a, q0, acc, b); });
    timed(c, HIP_KT_RK_STAGE, [&] {
        rc.fac = dt;
        launch_stage<2>(c, buoy, rc, b, q0, acc, a);
    });
    timed(c, HIP_KT_RK_STAGE, [&] {
        rc.fac = dt / 6.0;
        launch_stage<3>(c, buoy, rc, a, q0, acc, q0);
    });
    HIP_TRY(hipGetLastError());
    c->cg_scratch_dirty = 1;  // r, p_a, p_b now hold stage values at the walls
    return step_tail(c, g, prm, stats, true, "rk4_hip: NaN/Inf in the flow field");
}

// What follows the velocity / pressure update in rk4_impl (solver_rk4.c:
// 213-247), rk2_impl (solver_rk2.c:175-201) and explicit_euler_impl
// (solver_explicit_euler.c:534-575): the energy step with prm->dt on the new
// velocity, apply_boundary_conditions' periodic copies, the thermal BCs, then
// one stats / NaN pass. velocity_bcs = false leaves the boundary cells of
// u, v, w alone (explicit Euler).
static cfd_status_t step_tail(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                              ns_solver_stats_t* stats, bool velocity_bcs, const char* nan_msg) {
    const bool energy = (prm->alpha > 0.0);
    const size_t nz = c->nzg;
    launch_init_red(c);
    if (energy) ST_TRY(ctx_energy_step(c, g, prm, false));
    // apply_boundary_conditions: periodic copies of every field (x, y, z faces)
    if (velocity_bcs)
        for (double* f : {c->u, c->v, c->w})
            launch_bc(c, f, 1, DirVals{});
    for (double* f : {c->p, c->rho, c->T})
        if (f) launch_bc(c, f, 1, DirVals{});
    if (c->T) c->T_dirty = 1;
    if (energy) ST_TRY(ctx_apply_thermal_bcs(c, prm->thermal_bc, nz > 1));
    const dim3 cg = cell_grid(c);
    hipLaunchKernelGGL(k_vel_stats, cg, dim3(256), 0, c->stream, c->geo, c->u, c->v, c->w, c->p,
                       c->red);
    ctx_queue_max_T(c);
    HIP_TRY(hipMemcpyAsync(c->h_red, c->red, 8 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    flush_timing(c);
    if (c->h_red[5]) {
        set_err(CFD_ERROR_DIVERGED, "NaN/Inf detected in energy_step_explicit");
        return CFD_ERROR_DIVERGED;
    }
    if (c->have_T && c->T_dirty) {
        c->max_T = ord_dec(c->h_red[3]);
        c->T_dirty = 0;
    }
    if (stats) {
        stats->iterations = 1;
        stats->max_velocity = std::sqrt(ord_dec(c->h_red[0]));  // red[0]: max |u|^2
        stats->max_pressure = ord_dec(c->h_red[1]);
        stats->max_temperature = c->have_T ? c->max_T : 0.0;
    }
    if (c->h_red[2]) {
        set_err(CFD_ERROR_DIVERGED, nan_msg);
        return CFD_ERROR_DIVERGED;
    }
    return CFD_SUCCESS;
}

// rk2_impl (solver_rk2.c:48-211, Heun), one step. The two updates are stage
// kernels the RK4 sequence already has:
//   Qp = clamp(Q + dt k1), k1 kept          k_rk_stage2<0> with fac = dt
//   Q' = clamp(Q + (dt/2) (k1 + k2))        k_rk_stage2<3> with fac = dt/2, acc = k1
// (stage 3 forms q0 + fac * (acc + k): the reference's k1 + k2, then half_dt
// times it). No BCs between the stages. The predictor lives in u*, v*, w*,
// p_new, which the projection step rewrites before it reads them; none of the
// CG work arrays is borrowed, so cg_scratch_dirty stays as it is.
static cfd_status_t rk2_step_impl(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                                  ns_solver_stats_t* stats, int iter) {
    RkCoef rc;
    bool buoy = false;
    ST_TRY(step_head(c, g, prm, iter, "rk2_hip", true, prm ? prm->dt : 0.0, &rc, &buoy));
    const double dt = prm->dt;
    const Fld4 q0{{c->u, c->v, c->w, c->p}};
    const Fld4 a{{c->us, c->vs, c->ws, c->pn}};
    const Fld4 acc{{c->rk_acc[0], c->rk_acc[1], c->rk_acc[2], c->rk_acc[3]}};
    timed(c, HIP_KT_RK_STAGE, [&] {
        rc.fac = dt;
        launch_stage<0>(c, buoy, rc, q0, q0, acc, a);
    });
    timed(c, HIP_KT_RK_STAGE, [&] {
        rc.fac = 0.5 * dt;
        launch_stage<3>(c, buoy, rc, a, q0, acc, q0);
    });
    HIP_TRY(hipGetLastError());
    return step_tail(c, g, prm, stats, true, "rk2_hip: NaN/Inf in the flow field");
}

// explicit_euler_impl (solver_explicit_euler.c:337-582), one step, with
// cdt = fmin(dt, 1e-4) in the update, the source-table decay and the energy
// step (a params copy with dt = cdt carries it to all three).
//
// Boundary cells. The reference computes u_new, v_new, w_new, p_new, rho_new
// (copies of the field, interior cells overwritten), copies them over the
// field, runs the energy step, then (:546-552) saves the field's boundary
// velocities into u_new.., applies the periodic copies to all six fields and
// restores the boundary velocities from u_new... So:
//   - u, v, w: the boundary cells after the step are the ones before it, and
//     u_new equals the field in every cell when the next iteration starts:
//     the boundary is never touched, and a skipped interior cell keeps its
//     value. k_euler_step copies both kinds of cell through.
//   - p: p_new's boundary cells are stale (the periodic copy goes to the
//     field only), but the periodic copies read interior cells alone (x
//     faces, then y rows from the x-completed rows, then z planes), so what
//     the boundary held before them does not matter: the result is the
//     periodic copy of the new interior, and the next iteration's stencil
//     reads exactly those ghost values.
//   - rho: rho_new is rho (skipped cells keep the initial copy), so only the
//     periodic copy acts; T: energy step, periodic copy, thermal BCs.
// The kernel writes every cell of u*, v*, w*, p_new, which then become the
// fields by pointer swap (as the projection step swaps p and p_new).
static cfd_status_t euler_step_impl(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                                    ns_solver_stats_t* stats, int iter) {
    RkCoef rc;
    bool buoy = false;
    const double cdt = prm ? fmin(prm->dt, 1e-4) : 0.0;  // DT_CONSERVATIVE_LIMIT
    ST_TRY(step_head(c, g, prm, iter, "euler_hip", false, cdt, &rc, &buoy));
    ns_solver_params_t pc = *prm;
    pc.dt = cdt;
    rc.fac = cdt;
    const Fld4 cur{{c->u, c->v, c->w, c->p}};
    const Fld4 out{{c->us, c->vs, c->ws, c->pn}};
    const dim3 g2((unsigned)((c->nx + 127) / 128), (unsigned)((c->ny + 3) / 4), (unsigned)c->nz);
    timed(c, HIP_KT_RK_STAGE, [&] {
        klaunch(c, buoy ? k_euler_step<true> : k_euler_step<false>, g2, dim3(256), c->geo, rc, cur,
                out, c->rho, c->T, c->dxa, c->dya, c->src_u_row, c->src_v_col);
    });
    HIP_TRY(hipGetLastError());
    std::swap(c->u, c->us);
    std::swap(c->v, c->vs);
    std::swap(c->w, c->ws);
    std::swap(c->p, c->pn);
    return step_tail(c, g, &pc, stats, false, "NaN/Inf detected in explicit_euler step");
}

// Host-buffer path shared by hip_{rk4,rk2,euler}_step and the device API: n
// steps with source index 0..n-1 like the reference solvers' loops.
typedef cfd_status_t (*step_fn)(hip_proj_ctx*, const grid*, const ns_solver_params_t*,
                                ns_solver_stats_t*, int);
static cfd_status_t step_iter_host(step_fn step, hip_proj_ctx_t* c, flow_field* f, const grid* g,
                                   const ns_solver_params_t* prm, ns_solver_stats_t* stats,
                                   int n_steps) {
    if (!c || !f || !g || !prm) return CFD_ERROR_INVALID;
    if (f->nx < 3 || f->ny < 3 || (f->nz > 1 && f->nz < 3)) return CFD_ERROR_INVALID;
    ST_TRY(ctx_validate_params(c, g, prm));
    if (n_steps <= 0) return CFD_SUCCESS;
    c->resident = 0;
    const int ids[4] = {HIP_FIELD_U, HIP_FIELD_V, HIP_FIELD_W, HIP_FIELD_P};
    double* hf[4] = {f->u, f->v, f->w, f->p};
    for (int q = 0; q < 4; ++q) ST_TRY(hip_proj_set_field(c, ids[q], hf[q]));
    if (f->rho) ST_TRY(hip_proj_set_field(c, HIP_FIELD_RHO, f->rho));
    if (f->T) ST_TRY(hip_proj_set_field(c, HIP_FIELD_T, f->T));
    cfd_status_t s = CFD_SUCCESS;
    for (int it = 0; it < n_steps; ++it) {
        s = step(c, g, prm, stats, it);
        if (s != CFD_SUCCESS) break;
    }
    if (s == CFD_SUCCESS || s == CFD_ERROR_DIVERGED) {
        for (int q = 0; q < 4; ++q) ST_TRY(hip_proj_get_field(c, ids[q], hf[q]));
        if (f->rho) ST_TRY(hip_proj_get_field(c, HIP_FIELD_RHO, f->rho));
        if (f->T) ST_TRY(hip_proj_get_field(c, HIP_FIELD_T, f->T));
    }
    return s;
}

#define HIP_STEP_ITER_INTERNAL(name, impl)                                                  \
    extern "C" __attribute__((visibility("hidden"))) cfd_status_t name(                    \
        hip_proj_ctx_t* c, flow_field* f, const grid* g, const ns_solver_params_t* prm,    \
        ns_solver_stats_t* stats, int n_steps) {                                           \
        return step_iter_host(impl, c, f, g, prm, stats, n_steps);                         \
    }
// hip_rk4_step and the rk4_hip plugin; solve_{rk4,rk2,explicit_euler}_method_gpu
HIP_STEP_ITER_INTERNAL(hip_rk4_step_iter_internal, rk4_step_impl)
HIP_STEP_ITER_INTERNAL(hip_rk2_step_iter_internal, rk2_step_impl)
HIP_STEP_ITER_INTERNAL(hip_euler_step_iter_internal, euler_step_impl)

extern "C" {

cfd_status_t hip_rk4_step_device(hip_proj_ctx_t* c, const grid* g, const ns_solver_params_t* prm,
                                 ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return rk4_step_impl(c, g, prm, stats, 0);
}

cfd_status_t hip_rk4_step(hip_proj_ctx_t* c, flow_field* f, const grid* g,
                          const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return hip_rk4_step_iter_internal(c, f, g, prm, stats, 1);
}

cfd_status_t hip_rk2_step_device(hip_proj_ctx_t* c, const grid* g, const ns_solver_params_t* prm,
                                 ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return rk2_step_impl(c, g, prm, stats, 0);
}

cfd_status_t hip_rk2_step(hip_proj_ctx_t* c, flow_field* f, const grid* g,
                          const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return hip_rk2_step_iter_internal(c, f, g, prm, stats, 1);
}

cfd_status_t hip_euler_step_device(hip_proj_ctx_t* c, const grid* g,
                                   const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return euler_step_impl(c, g, prm, stats, 0);
}

cfd_status_t hip_euler_step(hip_proj_ctx_t* c, flow_field* f, const grid* g,
                            const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return hip_euler_step_iter_internal(c, f, g, prm, stats, 1);
}

}  // extern "C"
