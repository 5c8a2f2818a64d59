// projection_hip.hip -- device context and step orchestration behind the
// C-ABI of include/cfd_hip/projection_hip.h.
//
// One context = one device, one HIP stream, all fields resident in HBM with a
// padded row pitch. A step is: predictor -> (p_new = p) -> pressure solve on
// p_new with the divergence right-hand side fused into the CG setup ->
// corrector + boundary restore + NaN scan + stats -> swap(p, p_new).
// The CG loop keeps alpha/beta/convergence on the device (CgState) and the
// host only polls a pinned copy of the state every few iterations, so there
// is no host round trip per iteration (the reference GPU path does two per
// iteration, poisson_cg_gpu_solve.cuh:189-203).
#include "ctx.hpp"
#include "../host/grid_spacing.h"

#include <array>
#include "poisson_solve.hpp"

static __global__ void k_init_red(unsigned long long* red) {
    if (threadIdx.x == 0) {
        red[0] = 0x8000000000000000ull;  // enc(+0.0): reference maxima start at 0.0
        red[1] = 0x8000000000000000ull;
        red[2] = 0ull;
        red[5] = 0ull;
        red[3] = 0x000FFFFFFFFFFFFFull;  // enc(-inf)
        red[4] = 0x8000000000000000ull;
    }
}

void launch_init_red(hip_proj_ctx* c) { klaunch(c, k_init_red, dim3(1), dim3(64), c->red); }

cfd_status_t ctx_validate_params(const hip_proj_ctx* c, const grid* g,
                                    const ns_solver_params_t* prm) {
    if (!g || !prm) return CFD_ERROR_INVALID;
    if (g->nx != c->nx || g->ny != c->ny || g->nz != c->nzg) {
        set_err(CFD_ERROR_INVALID, "projection_hip: grid does not match the context");
        return CFD_ERROR_INVALID;
    }
    if (g->nz > 1 && g->dz) {
        for (size_t k = 1; k < g->nz - 1; k++)
            if (fabs(g->dz[k] - g->dz[0]) > 1e-14) {  // solver_projection.c:59-66
                set_err(CFD_ERROR_INVALID, "projection_hip: non-uniform dz");
                return CFD_ERROR_INVALID;
            }
    }
    if (prm->source_func) {
        set_err(CFD_ERROR_UNSUPPORTED,
                "projection_hip: host source_func callbacks cannot run on the device");
        return CFD_ERROR_UNSUPPORTED;
    }
    if (prm->alpha > 0.0) {
        if (prm->heat_source_func) {  // host callback (gpu_shared_kernels.cuh:271-276)
            set_err(CFD_ERROR_UNSUPPORTED,
                    "projection_hip: host heat_source_func callbacks cannot run on the device");
            return CFD_ERROR_UNSUPPORTED;
        }
        // energy_step_explicit_with_workspace (energy_solver.c:55-75) refuses
        // non-uniform dx / dy after the reference's solvers have advanced the
        // velocity; here the step is refused before any device work
        if (g->dx && !grid_axis_is_uniform(g->dx, g->nx)) {
            set_err(CFD_ERROR_UNSUPPORTED, "energy_solver: non-uniform dx not supported");
            return CFD_ERROR_UNSUPPORTED;
        }
        if (g->dy && !grid_axis_is_uniform(g->dy, g->ny)) {
            set_err(CFD_ERROR_UNSUPPORTED, "energy_solver: non-uniform dy not supported");
            return CFD_ERROR_UNSUPPORTED;
        }
        const ns_thermal_bc_config_t& t = prm->thermal_bc;
        auto ok = [](bc_type_t b) {
            return b == BC_TYPE_PERIODIC || b == BC_TYPE_NEUMANN || b == BC_TYPE_DIRICHLET;
        };
        if (!ok(t.left) || !ok(t.right) || !ok(t.bottom) || !ok(t.top) ||
            (g->nz > 1 && (!ok(t.front) || !ok(t.back)))) {  // energy_solver.c:230-241
            set_err(CFD_ERROR_INVALID,
                    "energy_apply_thermal_bcs: unsupported thermal BC type on a face "
                    "(only PERIODIC, NEUMANN, DIRICHLET are valid)");
            return CFD_ERROR_INVALID;
        }
        if (c->nranks > 1 && ((t.back == BC_TYPE_PERIODIC) != (t.front == BC_TYPE_PERIODIC))) {
            set_err(CFD_ERROR_UNSUPPORTED,
                    "projection_hip: Z-slabs need periodic thermal BCs on both z faces or neither");
            return CFD_ERROR_UNSUPPORTED;
        }
    }
    return CFD_SUCCESS;
}

// The two fields init_ctx (below) leaves to their first user: rhs and x_tmp.
cfd_status_t ensure_aux(hip_proj_ctx* c, bool need_rhs, bool need_xt) {
    const size_t n = field_elems(c);
    if (need_rhs && !c->rhs) {
        cfd_status_t s = dalloc(c, &c->rhs, n);
        if (s != CFD_SUCCESS) return s;
    }
    if (need_xt && !c->xt) {
        cfd_status_t s = dalloc(c, &c->xt, n);
        if (s != CFD_SUCCESS) return s;
    }
    return CFD_SUCCESS;
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

hip_proj_config_t hip_proj_config_default(void) {
    hip_proj_config_t c;
    memset(&c, 0, sizeof(c));
    c.device = -1;
    c.poisson_method = HIP_POISSON_CG;
    c.poisson_tolerance = 1e-6;
    c.poisson_abs_tolerance = 1e-10;
    c.poisson_max_iter = 5000;
    c.poisson_check_interval = 1;
    c.sor_omega = 0.0;
    c.poll_interval = 64;
    c.kchunk = 0;
    c.verbose = 0;
    c.sweep_rows = 16;   // tools/sweep_bench.py at 512^3: 16 rows + NT hints fastest
    // r01c / r01e sweep_bench at 512^3 (profiles/r01e_sweep_variants.jsonl)
    c.sweep_variant = SW_NT_STORE | SW_NT_LOAD | SW_PREFETCH | SW_EDGE1;
    c.rhs_density = 1;
    c.poisson_fail_fatal = 1;
    c.relax_two_pass = 0;
    c.sweep_variant_fold = 0;
    c.dirty_faces = 0;
    c.dirty_sync_interval = 0;
    c.cg_variant = 0;
    return c;
}

int hip_projection_available(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n > 0 ? 1 : 0;
}

static void free_ctx(hip_proj_ctx* c) {
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    for (void* b : c->allocs) hipFree(b);
    if (c->st) hipFree(c->st);
    if (c->rxst) hipFree(c->rxst);
    if (c->rxst2) hipFree(c->rxst2);
    if (c->rb2dec) hipFree(c->rb2dec);
    if (c->bcgst) hipFree(c->bcgst);
    if (c->bcg_part) hipFree(c->bcg_part);
    for (const TransformTable& t : c->tr_tabs) {
        if (t.fwd) hipFree(t.fwd);
        if (t.inv && t.inv != t.fwd) hipFree(t.inv);
        if (t.e) hipFree(t.e);
    }
    for (hipEvent_t e : c->tr_ev)
        if (e) hipEventDestroy(e);
    if (c->partials) hipFree(c->partials);
    if (c->counter) hipFree(c->counter);
    if (c->red) hipFree(c->red);
    if (c->redg) hipFree(c->redg);
    if (c->dsum) hipFree(c->dsum);
    if (c->clk) hipFree(c->clk);
    if (c->h_state) hipHostFree(c->h_state);
    if (c->h_red) hipHostFree(c->h_red);
    if (c->h_src) hipHostFree(c->h_src);
    if (c->ev_src) hipEventDestroy(c->ev_src);
    if (c->shell_host) hipHostFree(c->shell_host);
    if (c->shell_dev) hipFree(c->shell_dev);
    for (int i = 0; i < 2; i++)
        if (c->ev_poll[i]) hipEventDestroy(c->ev_poll[i]);
    for (auto e : c->ev_pool) hipEventDestroy(e);
    if (c->ev_b) hipEventDestroy(c->ev_b);
    if (c->ev_h) hipEventDestroy(c->ev_h);
    if (c->hstream) {
        hipStreamSynchronize(c->hstream);
        hipStreamDestroy(c->hstream);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

static cfd_status_t init_ctx(hip_proj_ctx* c, size_t nx, size_t ny, size_t nz) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->grid_cap = std::max(64, prop.multiProcessorCount * 8);
    c->env = read_knobs();
    c->nx = nx;
    c->ny = ny;
    c->nz = nz;
    // every launch geometry of this context (tile_plan.hpp)
    const PlanIn in{nx, ny, nz, c->rank, c->nranks, c->kofs, c->grid_cap, c->cfg.sweep_rows,
                    c->cfg.sweep_variant, c->cfg.kchunk, c->cfg.cg_variant};
    static_cast<TilePlan&>(*c) = plan_tiles(in, c->env);

    const size_t n = field_elems(c);
    double** fields[] = {&c->u, &c->v, &c->w, &c->p, &c->us, &c->vs, &c->ws, &c->pn,
                         &c->r, &c->pa, &c->pb, &c->pc4, &c->pd4};
    for (double** f : fields) {
        cfd_status_t s = dalloc(c, f, n);
        if (s != CFD_SUCCESS) return s;
    }
    if (dalloc(c, &c->src_u_row, ny) != CFD_SUCCESS) return CFD_ERROR;
    if (dalloc(c, &c->src_v_col, nx) != CFD_SUCCESS) return CFD_ERROR;
    // source tables (ny + nx), then the integrators' staged dx[nx], dy[ny]
    HIP_TRY(hipHostMalloc((void**)&c->h_src, 2 * (nx + ny) * sizeof(double),
                          hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_src, hipEventDisableTiming));
    HIP_TRY(hipMalloc((void**)&c->st, sizeof(CgState)));
    HIP_TRY(hipMemsetAsync(c->st, 0, sizeof(CgState), c->stream));
    // x2: the single-reduction CG reduces two values per workgroup
    HIP_TRY(hipMalloc((void**)&c->partials, 2 * sizeof(double) * c->n_partials));
    HIP_TRY(hipMalloc((void**)&c->counter, 64));
    HIP_TRY(hipMemsetAsync(c->counter, 0, 64, c->stream));
    HIP_TRY(hipMalloc((void**)&c->red, 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&c->redg, 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&c->clk, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->clk, 0, 4 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMalloc((void**)&c->dsum, 4 * sizeof(double)));
    HIP_TRY(hipMemsetAsync(c->dsum, 0, 4 * sizeof(double), c->stream));
    HIP_TRY(hipHostMalloc((void**)&c->h_state, 3 * sizeof(PollSlot), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&c->h_red, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_poll[0], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_poll[1], hipEventDisableTiming));
    if (c->nranks > 1) {
        HIP_TRY(hipStreamCreateWithFlags(&c->hstream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_b, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_h, hipEventDisableTiming));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

// ---------------------------------------------------------------------------
// Placement draws of the single-reduction CG's fields (r06). The march
// (k_ccf) streams r_it and p_{it-1} in and p_it and r_{it+1} out at equal
// offsets of different fields, and how fast it runs depends on where the
// allocator placed those fields: in one process, six 512^3 contexts created
// one after another ran 1.034-1.222 ms per iteration, each one stable to
// 0.2 % (tools/alloc_lottery.py, profiles/r06s_alloc_lottery.jsonl; textbook
// CG's sweeps spread 2.5 %). So a large single-reduction context draws its CG
// fields (r, r2, the four p buffers, x) up to `draws` times, keeping every
// draw allocated until the end so that each lands on other pages, times a
// short fixed-iteration solve on each, keeps the fastest set and frees the
// others. Speed only: the fields are zeroed afterwards and the arithmetic is
// the same on any placement. The probes also try random assignments of the
// pool's buffers to the seven roles: what is slow is a PAIR of fields that
// meet (r06x: random assignments from 4 sets beat 8 sets as allocated).
// ---------------------------------------------------------------------------
static __global__ void k_probe_fill(double* f, long long n) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (long long)gridDim.x * blockDim.x) {
        const unsigned h = (unsigned)(e * 2654435761ll) >> 12;
        f[e] = (double)(h & 1023u) * (1.0 / 1024.0) - 0.5;
    }
}

static cfd_status_t placement_draws(hip_proj_ctx* c, int sets, int trials) {
    constexpr int NF = 7;
    constexpr int PROBE_IT = 16;  // probe solve: setup + 16 iterations (~20 ms at 512^3)
    double** slots[NF] = {&c->r, &c->r2, &c->pa, &c->pb, &c->pc4, &c->pd4, &c->pn};
    const size_t n = field_elems(c);
    const size_t fbytes = n * sizeof(double);
    if (!c->r2) ST_TRY(dalloc(c, &c->r2, n));
    // a short solve on a pseudo-random right-hand side (us, the predictor's
    // output buffer, free at creation), no early exit; device time by events
    hipEvent_t ea, eb;
    HIP_TRY(hipEventCreate(&ea));
    HIP_TRY(hipEventCreate(&eb));
    hipExtLaunchKernelGGL(k_probe_fill, dim3(4096), dim3(256), 0, c->stream, nullptr, nullptr, 0,
                          c->us, (long long)n);
    const double h = 1.0 / (double)(c->nx - 1);
    auto probe = [&](float* ms) -> cfd_status_t {
        double* keep_rhs = c->rhs;
        c->rhs = c->us;
        HIP_TRY(hipMemsetAsync(c->pn, 0, fbytes, c->stream));
        HIP_TRY(hipEventRecord(ea, c->stream));
        const cfd_status_t s = cg_solve(c, h, h, h, DivCoef{}, RHS_FROM_ARRAY, 0.0, 0.0, PROBE_IT, 1,
                                        false);
        c->rhs = keep_rhs;
        HIP_TRY(hipEventRecord(eb, c->stream));
        HIP_TRY(hipEventSynchronize(eb));
        HIP_TRY(hipEventElapsedTime(ms, ea, eb));
        return s == CFD_ERROR_MAX_ITER ? CFD_SUCCESS : s;
    };
    // the pool: the fields as created (set 0) and sets - 1 more allocations
    // of all seven, every one kept until the end so each lands on other pages
    std::vector<double*> pf;
    std::vector<void*> pb;
    // the allocation a field lives in: dalloc placed it allocs[i] + i x stagger
    auto base_of = [&](double* f) -> void* {
        for (size_t i = 0; i < c->allocs.size(); ++i)
            if ((char*)f - (char*)c->allocs[i] == (std::ptrdiff_t)(i * c->stagger_bytes))
                return c->allocs[i];
        return nullptr;
    };
    for (int q = 0; q < NF; ++q) {
        pf.push_back(*slots[q]);
        pb.push_back(base_of(*slots[q]));
    }
    for (int d = 1; d < sets; ++d) {
        size_t freeb = 0, total = 0;
        if (hipMemGetInfo(&freeb, &total) != hipSuccess || freeb < (size_t)(1.25 * NF * fbytes))
            break;
        // a set that cannot be allocated ends the pool (its allocated part
        // stays in it)
        bool ok = true;
        for (int q = 0; q < NF && ok; ++q) {
            double* f = nullptr;
            ok = dalloc(c, &f, n) == CFD_SUCCESS;
            if (ok) {
                pf.push_back(f);
                pb.push_back(c->allocs.back());
            }
        }
        if (!ok) {
            (void)hipGetLastError();
            break;
        }
    }
    // assignments of pool buffers to the seven roles: trial t < pool sets is
    // set t as allocated; the rest draw seven distinct buffers (a fixed LCG)
    const int npool = (int)pf.size();
    const int nsets = npool / NF;
    std::vector<std::array<int, NF>> asg;
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int t = 0; t < std::max(trials, 1); ++t) {
        std::array<int, NF> a{};
        if (t < nsets) {
            for (int q = 0; q < NF; ++q) a[q] = t * NF + q;
        } else {
            std::vector<int> idx(npool);
            for (int k = 0; k < npool; ++k) idx[k] = k;
            for (int q = 0; q < NF; ++q) {
                lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                const int k = q + (int)((lcg >> 33) % (unsigned long long)(npool - q));
                std::swap(idx[q], idx[k]);
                a[q] = idx[q];
            }
        }
        asg.push_back(a);
    }
    cfd_status_t st = CFD_SUCCESS;
    std::vector<float> ms(asg.size(), 0.f);
    size_t done = 0;
    for (; done < asg.size() && st == CFD_SUCCESS; ++done) {
        for (int q = 0; q < NF; ++q) *slots[q] = pf[asg[done][q]];
        st = probe(&ms[done]);
    }
    hipEventDestroy(ea);
    hipEventDestroy(eb);
    if (st != CFD_SUCCESS) return st;
    size_t best = 0;
    for (size_t d = 1; d < done; ++d)
        if (ms[d] < ms[best]) best = d;
    for (int q = 0; q < NF; ++q) *slots[q] = pf[asg[best][q]];
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < npool; ++k) {
        bool used = false;
        for (int q = 0; q < NF; ++q) used = used || asg[best][q] == k;
        if (used) continue;
        auto it = std::find(c->allocs.begin(), c->allocs.end(), pb[k]);
        if (pb[k] && it != c->allocs.end()) {
            c->allocs.erase(it);
            hipFree(pb[k]);
            c->bytes -= std::min(c->bytes, fbytes);
        }
    }
    c->placement_ms.clear();
    for (size_t d = 0; d < done; ++d) c->placement_ms.push_back(ms[d] / (float)PROBE_IT);
    c->placement_pick = (int)best;
    // a clean state: the probe's fields, its RHS buffer and the CG state
    for (int q = 0; q < NF; ++q) HIP_TRY(hipMemsetAsync(*slots[q], 0, fbytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->us, 0, fbytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->st, 0, sizeof(CgState), c->stream));
    c->pstats = poisson_solver_stats_t{};
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

static hip_proj_ctx* create_common(size_t nx, size_t ny, size_t nz_local, size_t nz_global,
                                   SlabComm* comm, size_t kofs, const hip_proj_config_t* cfg) {
    if (!hip_projection_available()) {
        set_err(CFD_ERROR_UNSUPPORTED, "projection_hip: no HIP device available");
        return nullptr;
    }
    hip_proj_ctx* c = new hip_proj_ctx();
    c->cfg = cfg ? *cfg : hip_proj_config_default();
    if (comm) {
        c->device = comm->device;
    } else if (c->cfg.device < 0) {
        int d = 0;
        hipGetDevice(&d);
        c->device = d;
    } else {
        c->device = c->cfg.device;
    }
    if (c->cfg.poll_interval <= 0) c->cfg.poll_interval = 64;
    c->comm = comm;
    c->rank = comm ? comm->rank : 0;
    c->nranks = comm ? comm->size : 1;
    c->nzg = nz_global;
    c->kofs = kofs;
    if (init_ctx(c, nx, ny, nz_local) != CFD_SUCCESS) {
        free_ctx(c);
        return nullptr;
    }
    // placement draws of the single-reduction CG's fields (3-D contexts of
    // >= 2^24 cells, one device or one Z-slab rank; see placement_draws and,
    // for the pool's size, Knobs::placement_draws)
    {
        const int draws = c->env.placement_draws, trials = c->env.placement_trials;
        const long long cells = (long long)nx * (long long)ny * (long long)nz_local;
        if (c->cfg.cg_variant == 1 && nz_local >= 3 && cells >= (1LL << 24) && draws > 1 &&
            c->ccgeo.tiles_x > 0 && !c->env.ccf_off) {
            // a Z-slab rank probes its own fields as one device (no halo,
            // no all-reduce: nothing collective, so ranks may differ in how
            // many sets their memory allows), the march over its local planes
            const int nr = c->nranks;
            c->nranks = 1;
            const cfd_status_t ps = placement_draws(c, draws, trials);
            c->nranks = nr;
            if (ps != CFD_SUCCESS) {
                set_err(CFD_ERROR, "projection_hip: placement draws of the CG fields failed");
                free_ctx(c);
                return nullptr;
            }
        }
    }
    if (comm && c->cfg.poisson_method != HIP_POISSON_CG) {
        // Z-slab ranks of a relaxation solver: what the first solve would set
        // up lazily on a rank thread (the aux fields, the loop state, the
        // library's code object, which a kernel attribute query loads) is set
        // up here, at creation
        bool ok = relax_preload() && ensure_aux(c, true, true) == CFD_SUCCESS;
        if (ok && !c->rxst) ok = hipMalloc((void**)&c->rxst, sizeof(RxState)) == hipSuccess;
        if (ok && !c->rxst2) ok = hipMalloc((void**)&c->rxst2, sizeof(RxState)) == hipSuccess;
        if (!ok) {
            set_err(CFD_ERROR_NOMEM, "projection_hip: slab relaxation setup failed");
            free_ctx(c);
            return nullptr;
        }
    }
    return c;
}

hip_proj_ctx_t* hip_proj_create(size_t nx, size_t ny, size_t nz, const hip_proj_config_t* cfg) {
    if (nx < 3 || ny < 3 || nz == 0 || (nz > 1 && nz < 3)) {
        set_err(CFD_ERROR_INVALID, "projection_hip: grid must be >= 3 points per active axis");
        return nullptr;
    }
    return create_common(nx, ny, nz, nz, nullptr, 0, cfg);
}

cfd_status_t hip_proj_slab_layout(size_t nz, int rank, int size, size_t* k_offset,
                                  size_t* nz_local) {
    return slab_layout(nz, rank, size, k_offset, nz_local) ? CFD_SUCCESS : CFD_ERROR_INVALID;
}

hip_proj_ctx_t* hip_proj_create_slab(size_t nx, size_t ny, size_t nz, hip_proj_comm_t* comm,
                                     const hip_proj_config_t* cfg) {
    if (!comm || !comm->impl) {
        set_err(CFD_ERROR_INVALID, "hip_proj_create_slab: no communicator");
        return nullptr;
    }
    size_t kofs = 0, nzl = 0;
    if (nx < 3 || ny < 3 ||
        hip_proj_slab_layout(nz, comm->impl->rank, comm->impl->size, &kofs, &nzl) != CFD_SUCCESS) {
        set_err(CFD_ERROR_INVALID,
                "hip_proj_create_slab: 3-D grid with at least one interior plane per rank needed");
        return nullptr;
    }
    return create_common(nx, ny, nzl, nz, comm->impl, kofs, cfg);
}

cfd_status_t hip_proj_slab_info(const hip_proj_ctx_t* c, size_t* k_offset, size_t* nz_local,
                                int* rank, int* size) {
    if (!c) return CFD_ERROR_INVALID;
    if (k_offset) *k_offset = c->kofs;
    if (nz_local) *nz_local = c->nz;
    if (rank) *rank = c->rank;
    if (size) *size = c->nranks;
    return CFD_SUCCESS;
}

void hip_proj_destroy(hip_proj_ctx_t* ctx) {
    GroupHostLock hl_(ctx);  // holds the group, not the context: safe across the free
    free_ctx(ctx);
}

size_t hip_proj_device_bytes(const hip_proj_ctx_t* ctx) { return ctx ? ctx->bytes : 0; }
size_t hip_proj_row_pitch(const hip_proj_ctx_t* ctx) { return ctx ? (size_t)ctx->px : 0; }

cfd_status_t hip_proj_synchronize(hip_proj_ctx_t* c) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    flush_timing(c);
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_set_field(hip_proj_ctx_t* c, int id, const double* host) {
    GroupHostLock hl_(c);
    if (!c || !host) return CFD_ERROR_INVALID;
    double* d = field_ptr(c, id);
    if ((id == HIP_FIELD_T || id == HIP_FIELD_RHO) && !d) {
        double** slot = (id == HIP_FIELD_T) ? &c->T : &c->rho;
        if (dalloc(c, slot, field_elems(c)) != CFD_SUCCESS) return CFD_ERROR_NOMEM;
        d = *slot;
    }
    if (!d) return CFD_ERROR_INVALID;
    c->resident = 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(copy_in(c, d, host));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (id == HIP_FIELD_T) c->have_T = c->T_dirty = 1;
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_get_field(hip_proj_ctx_t* c, int id, double* host) {
    GroupHostLock hl_(c);
    if (!c || !host) return CFD_ERROR_INVALID;
    double* d = field_ptr(c, id);
    if (!d) return CFD_ERROR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(copy_out(c, host, d));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

static __global__ void k_fill(double* f, long long n, double v) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (long long)gridDim.x * blockDim.x)
        f[e] = v;
}

cfd_status_t hip_proj_fill_field(hip_proj_ctx_t* c, int id, double value) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    double* d = field_ptr(c, id);
    if ((id == HIP_FIELD_T || id == HIP_FIELD_RHO) && !d) {
        double** slot = (id == HIP_FIELD_T) ? &c->T : &c->rho;
        if (dalloc(c, slot, field_elems(c)) != CFD_SUCCESS) return CFD_ERROR_NOMEM;
        d = *slot;
        if (id == HIP_FIELD_T) c->have_T = 1;
    }
    if (!d) return CFD_ERROR_INVALID;
    c->resident = 0;
    HIP_TRY(hipSetDevice(c->device));
    klaunch(c, k_fill, dim3(4096), dim3(256), d, (long long)field_elems(c), value);
    HIP_TRY(hipGetLastError());
    if (id == HIP_FIELD_T) c->T_dirty = 1;
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_set_density(hip_proj_ctx_t* c, double rho0) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    c->rho0 = rho0;
    // a per-cell density array (RK4, restart files) follows the uniform value
    if (c->rho) return hip_proj_fill_field(c, HIP_FIELD_RHO, rho0);
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_upload(hip_proj_ctx_t* c, const flow_field* f) {
    GroupHostLock hl_(c);
    if (!c || !f) return CFD_ERROR_INVALID;
    if (f->nx != c->nx || f->ny != c->ny || f->nz != c->nz) return CFD_ERROR_INVALID;
    cfd_status_t s;
    if ((s = hip_proj_set_field(c, HIP_FIELD_U, f->u)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_set_field(c, HIP_FIELD_V, f->v)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_set_field(c, HIP_FIELD_W, f->w)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_set_field(c, HIP_FIELD_P, f->p)) != CFD_SUCCESS) return s;
    if (f->T) {
        if ((s = hip_proj_set_field(c, HIP_FIELD_T, f->T)) != CFD_SUCCESS) return s;
    }
    c->rho0 = f->rho ? f->rho[0] : 1.0;
    if (c->rho) {  // keep an existing per-cell density in step with the field
        s = f->rho ? hip_proj_set_field(c, HIP_FIELD_RHO, f->rho)
                   : hip_proj_fill_field(c, HIP_FIELD_RHO, 1.0);
        if (s != CFD_SUCCESS) return s;
    }
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_download(hip_proj_ctx_t* c, flow_field* f) {
    GroupHostLock hl_(c);
    if (!c || !f) return CFD_ERROR_INVALID;
    cfd_status_t s;
    if ((s = hip_proj_get_field(c, HIP_FIELD_U, f->u)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_get_field(c, HIP_FIELD_V, f->v)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_get_field(c, HIP_FIELD_W, f->w)) != CFD_SUCCESS) return s;
    if ((s = hip_proj_get_field(c, HIP_FIELD_P, f->p)) != CFD_SUCCESS) return s;
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_apply_scalar_bc(hip_proj_ctx_t* c, int id, bc_type_t type) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    c->resident = 0;
    double* d = field_ptr(c, id);
    if (!d) return CFD_ERROR_INVALID;
    int mode;
    if (type == BC_TYPE_NEUMANN) mode = 0;
    else if (type == BC_TYPE_PERIODIC) mode = 1;
    else {
        set_err(CFD_ERROR_UNSUPPORTED, "hip_proj_apply_scalar_bc: only NEUMANN and PERIODIC");
        return CFD_ERROR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (mode == 1 && dist(c)) {
        // periodic z across slabs: x/y ring on every local plane, then the
        // z copy (plane 0 <- nz-2, nz-1 <- 1) as a wrap-around halo exchange
        Geo g = c->geo;
        g.lo_face = g.hi_face = 0;
        launch_bc_geo(c, g, d, mode, DirVals{});
        HIP_TRY(hipGetLastError());
        return halo(c, {d}, true);
    }
    launch_bc(c, d, mode, DirVals{});
    HIP_TRY(hipGetLastError());
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_apply_dirichlet(hip_proj_ctx_t* c, int id, const bc_dirichlet_values_t* v) {
    GroupHostLock hl_(c);
    if (!c || !v) return CFD_ERROR_INVALID;
    c->resident = 0;
    double* d = field_ptr(c, id);
    if (!d) return CFD_ERROR_INVALID;
    DirVals dv{v->left, v->right, v->top, v->bottom, v->front, v->back};
    HIP_TRY(hipSetDevice(c->device));
    launch_bc(c, d, 2, dv);
    HIP_TRY(hipGetLastError());
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_apply_thermal_bcs(hip_proj_ctx_t* c, const ns_solver_params_t* prm) {
    GroupHostLock hl_(c);
    if (!c || !prm) return CFD_ERROR_INVALID;
    c->resident = 0;
    if (!c->T) {
        set_err(CFD_ERROR_INVALID, "energy_apply_thermal_bcs: missing temperature field");
        return CFD_ERROR_INVALID;
    }
    if (prm->alpha <= 0.0) return CFD_SUCCESS;  // energy disabled: no-op (energy_solver.c:217)
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(ctx_apply_thermal_bcs(c, prm->thermal_bc, c->nzg > 1));
    c->T_dirty = 1;
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_get_poisson_stats(hip_proj_ctx_t* c, poisson_solver_stats_t* s) {
    GroupHostLock hl_(c);
    if (!c || !s) return CFD_ERROR_INVALID;
    *s = c->pstats;
    return CFD_SUCCESS;
}

void hip_proj_enable_timing(hip_proj_ctx_t* c, int enable) {
    GroupHostLock hl_(c);
    if (c) c->timing = enable ? 1 : 0;
}

void hip_proj_reset_timing(hip_proj_ctx_t* c) {
    GroupHostLock hl_(c);
    if (!c) return;
    hipStreamSynchronize(c->stream);
    flush_timing(c);
    for (int k = 0; k < HIP_KT_COUNT; k++) {
        c->kt_ms[k] = 0;
        c->kt_n[k] = 0;
    }
    if (c->clk) {
        hipMemsetAsync(c->clk, 0, 4 * sizeof(unsigned long long), c->stream);
        hipStreamSynchronize(c->stream);
    }
}

int hip_proj_get_placement(hip_proj_ctx_t* c, double* ms_per_iter, int capacity, int* picked) {
    GroupHostLock hl_(c);
    if (picked) *picked = c ? c->placement_pick : -1;
    if (!c) return 0;
    const int n = (int)c->placement_ms.size();
    for (int i = 0; i < n && i < capacity && ms_per_iter; ++i) ms_per_iter[i] = c->placement_ms[i];
    return n;
}

cfd_status_t hip_proj_get_clock_sample(hip_proj_ctx_t* c, double* mhz, long long* workgroups) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    unsigned long long h[4] = {0, 0, 0, 0};
    if (c->clk) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(h, c->clk, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (mhz) *mhz = h[1] ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
    if (workgroups) *workgroups = (long long)h[2];
    return CFD_SUCCESS;
}

int hip_proj_get_timing_n(hip_proj_ctx_t* c, double* total_ms, long long* launches,
                          int capacity) {
    GroupHostLock hl_(c);
    if (!c || capacity <= 0) return 0;
    hipStreamSynchronize(c->stream);
    flush_timing(c);
    const int n = std::min(capacity, (int)HIP_KT_COUNT);
    for (int k = 0; k < n; k++) {
        if (total_ms) total_ms[k] = c->kt_ms[k];
        if (launches) launches[k] = c->kt_n[k];
    }
    return n;
}

void hip_proj_get_timing(hip_proj_ctx_t* c, double* total_ms, long long* launches) {
    (void)hip_proj_get_timing_n(c, total_ms, launches, HIP_KT_COUNT_LEGACY);
}

int hip_proj_abi_version(void) { return HIP_PROJ_ABI_VERSION; }

}  // extern "C"

// energy_apply_thermal_bcs (energy_solver.c:204-334) on the device T:
// x faces, y faces, z faces (3-D), each a gather pass in the reference order.
cfd_status_t ctx_apply_thermal_bcs(hip_proj_ctx* c, const ns_thermal_bc_config_t& t, bool is3d) {
    ThermalFaces tf;
    const bc_type_t ty[6] = {t.left, t.right, t.bottom, t.top, t.back, t.front};
    const double v[6] = {t.dirichlet_values.left, t.dirichlet_values.right,
                         t.dirichlet_values.bottom, t.dirichlet_values.top,
                         t.dirichlet_values.back, t.dirichlet_values.front};
    for (int f = 0; f < 6; ++f) {
        tf.type[f] = (ty[f] == BC_TYPE_PERIODIC || ty[f] == BC_TYPE_NEUMANN ||
                      ty[f] == BC_TYPE_DIRICHLET) ? (int)ty[f] : -1;
        tf.val[f] = v[f];
    }
    auto blocks = [](long long n) {
        return (unsigned)std::max(1LL, std::min((n + 255) / 256, 65535LL));
    };
    klaunch(c, k_thermal_bc, dim3(blocks(2LL * c->ny * c->nz)), dim3(256), c->geo, c->T, tf, 0);
    klaunch(c, k_thermal_bc, dim3(blocks(2LL * c->nx * c->nz)), dim3(256), c->geo, c->T, tf, 1);
    if (is3d) {
        if (dist(c) && t.back == BC_TYPE_PERIODIC && t.front == BC_TYPE_PERIODIC) {
            ST_TRY(halo(c, {c->T}, true));  // z wrap across the slabs
        } else {
            klaunch(c, k_thermal_bc, dim3(blocks(2LL * c->nx * c->ny)), dim3(256), c->geo, c->T,
                    tf, 2);
        }
    }
    HIP_TRY(hipGetLastError());
    return CFD_SUCCESS;
}

cfd_status_t ctx_energy_step(hip_proj_ctx* c, const grid* g, const ns_solver_params_t* prm,
                             bool apply_bcs) {
    // energy_step_explicit_with_workspace (energy_solver.c:21-176) on the
    // current velocity, then energy_apply_thermal_bcs (:204-334)
    const size_t nz = c->nzg;
    const double dx = g->dx[0], dy = g->dy[0];
    const double dz = (nz > 1 && g->dz) ? g->dz[0] : 0.0;
    if (!c->Tn) ST_TRY(dalloc(c, &c->Tn, field_elems(c)));
    EnergyCoef ec;
    ec.inv_2dx = 1.0 / (2.0 * dx);
    ec.inv_2dy = 1.0 / (2.0 * dy);
    ec.inv_2dz = (nz > 1 && g->dz) ? 1.0 / (2.0 * dz) : 0.0;
    ec.inv_dx2 = 1.0 / (dx * dx);
    ec.inv_dy2 = 1.0 / (dy * dy);
    ec.inv_dz2 = (nz > 1 && g->dz) ? 1.0 / (dz * dz) : 0.0;
    ec.alpha = prm->alpha;
    ec.dt = prm->dt;
    timed(c, HIP_KT_ENERGY, [&] {
        klaunch(c, k_energy, cell_grid(c), dim3(256), c->geo, ec, c->T, c->u, c->v, c->w, c->Tn,
                c->red);
    });
    std::swap(c->T, c->Tn);
    if (apply_bcs) ST_TRY(ctx_apply_thermal_bcs(c, prm->thermal_bc, nz > 1));
    c->T_dirty = 1;
    return CFD_SUCCESS;
}

void ctx_queue_max_T(hip_proj_ctx* c) {
    if (!c->have_T || !c->T_dirty) return;
    // compute_max_temperature (solver_registry.c:52-62), owned planes + faces
    const int ks = (c->nz > 1 && !c->geo.lo_face) ? 1 : 0;
    const int ke = (c->nz > 1 && !c->geo.hi_face) ? (int)c->nz - 1 : (int)c->nz;
    const dim3 cg = cell_grid(c);
    hipLaunchKernelGGL(k_field_max, dim3(cg.x, cg.y, (unsigned)(ke - ks)), dim3(256), 0,
                       c->stream, c->geo, c->T, c->red + 3, ks);
}

// The sine- and cosine-transform solves work on whole z lines: a Z-slab
// context is refused before anything is uploaded or launched (as BiCGSTAB's
// refusals).
static cfd_status_t transform_refuse_slab(const hip_proj_ctx* c, int method) {
    if (transform_kind(method) < 0 || !dist(c)) return CFD_SUCCESS;
    set_err(CFD_ERROR_UNSUPPORTED,
            method == HIP_POISSON_DST
                ? "projection_hip: the DST pressure solve runs on one device, not on Z-slabs"
                : "projection_hip: the DCT pressure solve runs on one device, not on Z-slabs");
    return CFD_ERROR_UNSUPPORTED;
}

extern "C" {

static cfd_status_t step_device_impl(hip_proj_ctx_t* c, const grid* g,
                                     const ns_solver_params_t* prm, ns_solver_stats_t* stats,
                                     int iter) {
    if (!c) return CFD_ERROR_INVALID;
    cfd_status_t s = ctx_validate_params(c, g, prm);
    if (s != CFD_SUCCESS) return s;
    ST_TRY(transform_refuse_slab(c, c->cfg.poisson_method));
    HIP_TRY(hipSetDevice(c->device));
    const size_t nz = c->nzg;
    const double dx = g->dx[0], dy = g->dy[0];
    const double dz = (nz > 1 && g->dz) ? g->dz[0] : 0.0;
    const double dt = prm->dt;
    const bool buoy = (prm->beta != 0.0);
    const bool energy = (prm->alpha > 0.0);
    if ((buoy || energy) && !c->have_T) {
        set_err(CFD_ERROR_INVALID, "projection_hip: buoyancy / energy equation need the T field");
        return CFD_ERROR_INVALID;
    }

    // source-term tables: compute_source_terms at iter = 0 (solver_explicit_euler.c:317-333)
    ST_TRY(upload_source_tables(c, g, prm, iter));

    PredCoef2 pc;
    pc.two_dx = 2.0 * dx;
    pc.two_dy = 2.0 * dy;
    pc.inv_2dz = (nz > 1 && g->dz) ? 1.0 / (2.0 * dz) : 0.0;
    pc.dx_sq = dx * dx;
    pc.dy_sq = dy * dy;
    pc.inv_dz2 = (nz > 1 && g->dz) ? 1.0 / (dz * dz) : 0.0;
    pc.r_two_dx = 1.0 / pc.two_dx;
    pc.r_two_dy = 1.0 / pc.two_dy;
    pc.r_dx_sq = 1.0 / pc.dx_sq;
    pc.r_dy_sq = 1.0 / pc.dy_sq;
    pc.dt = dt;
    pc.nu = prm->mu;
    pc.beta = prm->beta;
    pc.T_ref = prm->T_ref;
    pc.g0 = prm->gravity[0];
    pc.g1 = prm->gravity[1];
    pc.g2 = prm->gravity[2];
    const unsigned npg = (unsigned)(c->pgeo.tiles_x * c->pgeo.tiles_y * c->pgeo.tiles_z);
    // slabs: the neighbours' planes of everything the stencils read
    ST_TRY(halo(c, {c->u, c->v, c->w, c->p}));
    if (buoy || energy) ST_TRY(halo(c, {c->T}));
    const unsigned np3 =
        (unsigned)(c->pgeo16.tiles_x * c->pgeo16.tiles_y * c->pgeo16.tiles_z);
    timed(c, HIP_KT_PREDICTOR, [&] {
        // PF = 0: one plane's loads per step (the plane-ahead schedule
        // measured slower, profiles/r02_step_kernels.jsonl)
        auto go = [&](auto kern, unsigned nb, int ty, const SGeo& g) {
            klaunch(c, kern, dim3(nb), dim3(64 * ty), g, pc, c->u, c->v, c->w, c->T, c->src_u_row,
                    c->src_v_col, c->us, c->vs, c->ws);
        };
        auto p3 = [&](auto FL) {
            with_bool(buoy, [&](auto B) { go(k_pred3<B, FL>, np3, PC_TY, c->pgeo16); });
        };
        if (c->pc3 == 1) p3(IntC<0>{});
        else if (c->pc3 == 2) p3(IntC<SW_NT_STORE>{});
        else if (c->pc3 == 4) p3(IntC<SW_NT_STORE | SW_NT_LOAD>{});
        else with_bool(buoy, [&](auto B) { go(k_pred2<B, 0>, npg, PR_TY, c->pgeo); });
    });
    klaunch(c, k_shell_copy, dim3(shell_blocks(c)), dim3(256), c->geo, c->u, c->v, c->w, c->us,
            c->vs, c->ws);
    HIP_TRY(hipGetLastError());
    ST_TRY(halo(c, {c->ws}));  // d(w*)/dz of the divergence

    // p_new = p (solver_projection.c:108)
    HIP_TRY(hipMemcpyAsync(c->pn, c->p, field_elems(c) * sizeof(double), hipMemcpyDeviceToDevice,
                           c->stream));

    double rho = c->rho0;
    if (rho < 1e-10) rho = 1.0;
    DivCoef dc;
    dc.two_dx = 2.0 * dx;
    dc.two_dy = 2.0 * dy;
    dc.inv_2dz = pc.inv_2dz;
    dc.rho_over_dt = c->cfg.rhs_density ? rho / dt : 1.0 / dt;

    const int method = c->cfg.poisson_method;
    cfd_status_t ps;
    if (method == HIP_POISSON_CG) {
        ps = cg_solve(c, dx, dy, dz, dc, RHS_FROM_VELOCITY, c->cfg.poisson_tolerance,
                      c->cfg.poisson_abs_tolerance, c->cfg.poisson_max_iter,
                      std::max(1, c->cfg.poisson_check_interval), true);
    } else {
        s = ensure_aux(c, true, method == HIP_POISSON_JACOBI);
        if (s != CFD_SUCCESS) return s;
        const Lap L = make_lap(dx, dy, dz);
        const int G = tile_grid(c);
        klaunch(c, k_cg_setup<true, true, false>, dim3(G), dim3(NT), c->geo, L, dc, c->us, c->vs,
                c->ws, c->rhs, c->pn, c->r, c->st, c->partials, c->counter, 0.0, 0.0, 0, 1, c->dsum,
                nullptr);
        if (method == HIP_POISSON_JACOBI)
            HIP_TRY(hipMemsetAsync(c->xt, 0, field_elems(c) * sizeof(double), c->stream));
        int maxit = c->cfg.poisson_max_iter;
        if (transform_kind(method) >= 0)
            ps = transform_solve(c, transform_kind(method), dx, dy, dz,
                                 c->cfg.poisson_tolerance, c->cfg.poisson_abs_tolerance);
        else
            ps = relax_solve(c, method, dx, dy, dz, c->cfg.poisson_tolerance,
                             c->cfg.poisson_abs_tolerance, maxit,
                             std::max(1, c->cfg.poisson_check_interval), c->cfg.sor_omega);
    }
    if (ps == CFD_ERROR_MAX_ITER && !c->cfg.poisson_fail_fatal) ps = CFD_SUCCESS;
    if (ps != CFD_SUCCESS) {
        if (ps == CFD_ERROR_MAX_ITER) set_err(CFD_ERROR_MAX_ITER, "projection_hip: pressure solve did not converge");
        return ps;
    }

    CorrCoef2 cc;
    cc.two_dx = 2.0 * dx;
    cc.two_dy = 2.0 * dy;
    cc.inv_2dz = pc.inv_2dz;
    cc.r_two_dx = pc.r_two_dx;
    cc.r_two_dy = pc.r_two_dy;
    cc.dt_over_rho = dt / rho;
    launch_init_red(c);
    timed(c, HIP_KT_CORRECTOR, [&] {
        auto c3 = [&](auto kern) {
            klaunch(c, kern, dim3(np3), dim3(64 * PC_TY), c->pgeo16, cc, c->us, c->vs, c->ws, c->pn,
                    c->u, c->v, c->w, c->red);
        };
        if (c->pc3 == 1) c3(k_corr3<0>);
        else if (c->pc3 == 2) c3(k_corr3<SW_NT_STORE>);
        else if (c->pc3 == 4) c3(k_corr3<SW_NT_STORE | SW_NT_LOAD>);
        else
            klaunch(c, k_corr2<0>, dim3(npg), dim3(64 * PR_TY), c->pgeo, cc, c->us, c->vs, c->ws,
                    c->pn, c->u, c->v, c->w, c->red);
    });
    klaunch(c, k_shell_stats, dim3(shell_blocks(c)), dim3(256), c->geo, c->u, c->v, c->w, c->pn,
            c->red);
    std::swap(c->p, c->pn);  // memcpy(field->p, p_new) (solver_projection.c:253)
    if (energy) ST_TRY(ctx_energy_step(c, g, prm, true));  // solver_projection.c:255-274
    ctx_queue_max_T(c);
    const unsigned long long* red = reduce_red(c, &s);
    if (s != CFD_SUCCESS) return s;
    HIP_TRY(hipMemcpyAsync(c->h_red, red, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    flush_timing(c);
    if (c->h_red[5]) {
        set_err(CFD_ERROR_DIVERGED, "NaN/Inf detected in energy_step_explicit");
        return CFD_ERROR_DIVERGED;
    }
    if (c->h_red[2]) {
        set_err(CFD_ERROR_DIVERGED, "projection_hip: NaN/Inf in the flow field");
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
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_mark_host_dirty(hip_proj_ctx_t* c) {
    GroupHostLock hl_(c);
    if (!c) return CFD_ERROR_INVALID;
    c->resident = 0;
    c->hash_ok = 0;
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_step_device(hip_proj_ctx_t* c, const grid* g,
                                  const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    if (c) c->resident = 0;
    return step_device_impl(c, g, prm, stats, 0);
}

}  // extern "C"

// Fields of the host-buffer step: u, v, w, p and, when present, T.
static int host_fields(hip_proj_ctx* c, flow_field* f, double** host, double** dev) {
    host[0] = f->u, host[1] = f->v, host[2] = f->w, host[3] = f->p;
    dev[0] = c->u, dev[1] = c->v, dev[2] = c->w, dev[3] = c->p;
    if (!f->T || !c->T) return 4;
    host[4] = f->T;
    dev[4] = c->T;
    return 5;
}

// Host-buffer path shared by hip_proj_step (one step, shell_ok = 1) and the
// plugin's solve (n steps, source-term iteration index 0..n-1 as in
// solver_projection.c:112). In the resident mode (cfg.dirty_faces, see
// shell_io.hip) a step on the same host arrays as the previous one uploads
// only the depth-1 boundary shell and downloads the depth-2 shell.
static cfd_status_t host_steps(hip_proj_ctx_t* c, flow_field* f, const grid* g,
                               const ns_solver_params_t* prm, ns_solver_stats_t* stats,
                               int n_steps, bool shell_ok) {
    if (!c || !f || !g || !prm) return CFD_ERROR_INVALID;
    if (f->nx < 3 || f->ny < 3 || (f->nz > 1 && f->nz < 3)) return CFD_ERROR_INVALID;
    cfd_status_t s = ctx_validate_params(c, g, prm);
    if (s != CFD_SUCCESS) return s;
    ST_TRY(transform_refuse_slab(c, c->cfg.poisson_method));
    if (n_steps <= 0) return CFD_SUCCESS;
    const bool need_T = (prm->beta != 0.0) || (prm->alpha > 0.0);
    const bool shell = shell_ok && c->cfg.dirty_faces > 0 && ctx_shell_fits(c, 2);
    const bool same = c->resident && c->res_ptr[0] == f->u && c->res_ptr[1] == f->v &&
                      c->res_ptr[2] == f->w && c->res_ptr[3] == f->p &&
                      c->res_ptr[4] == f->T && (!f->T || c->T);
    const int verify = c->cfg.dirty_verify_interval;
    if (shell && same && verify > 0 && c->hash_ok && c->res_steps % verify == 0) {
        // the guard: the interior of the host arrays must be what the
        // resident steps left there (the device holds the current interior)
        double* host[5];
        double* dev[5];
        const int nf = host_fields(c, f, host, dev);
        unsigned long long h[5], h1[5];
        ctx_host_hash(c, host, nf, false, h);
        ctx_host_hash(c, host, nf, true, h1);
        for (int q = 0; q < nf && q < c->hash_nf; ++q)
            if (h[q] != c->host_hash[q] || h1[q] != c->host_hash1[q]) {
                set_err(CFD_ERROR_INVALID,
                        "projection_hip resident mode: the interior of a host field changed "
                        "since the last step (it is not uploaded); call hip_proj_sync_host, "
                        "write the cells, then hip_proj_mark_host_dirty");
                return CFD_ERROR_INVALID;
            }
    }
    const bool full_up = !(shell && same);
    if (shell && same) {
        double* host[5];
        double* dev[5];
        const int nf = host_fields(c, f, host, dev);
        ST_TRY(ctx_shell_put(c, host, dev, nf, 1));
        if (nf == 5) c->T_dirty = 1;
    } else {
        if ((s = hip_proj_set_field(c, HIP_FIELD_U, f->u)) != CFD_SUCCESS) return s;
        if ((s = hip_proj_set_field(c, HIP_FIELD_V, f->v)) != CFD_SUCCESS) return s;
        if ((s = hip_proj_set_field(c, HIP_FIELD_W, f->w)) != CFD_SUCCESS) return s;
        if ((s = hip_proj_set_field(c, HIP_FIELD_P, f->p)) != CFD_SUCCESS) return s;
        // resident mode: T travels too, so its maximum comes from the device
        if (f->T && (need_T || shell)) {
            if ((s = hip_proj_set_field(c, HIP_FIELD_T, f->T)) != CFD_SUCCESS) return s;
        }
        c->res_steps = 0;
    }
    c->resident = 0;
    c->rho0 = f->rho ? f->rho[0] : 1.0;
    int done = 0;  // steps completed: the reference leaves them applied to field
    for (int it = 0; it < n_steps; ++it) {
        s = step_device_impl(c, g, prm, stats, it);
        if (s != CFD_SUCCESS) break;
        ++done;
    }
    // a failed step (pressure solve unconverged, communication) leaves the
    // device u, v, w, p as the completed steps made them
    const bool energy_T = prm->alpha > 0.0 && f->T && c->T;
    if (s == CFD_SUCCESS || s == CFD_ERROR_DIVERGED || done > 0) {
        ++c->res_steps;
        const int every = c->cfg.dirty_sync_interval;
        const bool shell_down = shell && s == CFD_SUCCESS && !(every > 0 && c->res_steps % every == 0);
        if (!shell_down) c->hash_ok = 0;  // the whole host field changed
        if (shell_down) {
            double* host[5];
            double* dev[5];
            const int nall = host_fields(c, f, host, dev);
            ST_TRY(ctx_shell_get(c, host, dev, energy_T ? nall : 4, 2));
        } else {
            cfd_status_t d = hip_proj_download(c, f);
            if (d != CFD_SUCCESS) return d;
            if (energy_T) {
                d = hip_proj_get_field(c, HIP_FIELD_T, f->T);
                if (d != CFD_SUCCESS) return d;
            }
        }
    } else if (shell) {
        // nothing completed: the device holds the uploaded state; make the
        // whole host field current before handing the error back
        c->hash_ok = 0;
        cfd_status_t d = hip_proj_download(c, f);
        if (d != CFD_SUCCESS) return d;
    }
    if (shell) {
        c->resident = 1;
        c->res_ptr[0] = f->u, c->res_ptr[1] = f->v, c->res_ptr[2] = f->w, c->res_ptr[3] = f->p;
        c->res_ptr[4] = f->T;
        if (verify > 0) {
            // the guard's reference: layer 1 as this step's download left it;
            // the deep interior only after a full transfer (it is untouched
            // on the host otherwise)
            double* host[5];
            double* dev[5];
            const int nf = host_fields(c, f, host, dev);
            if (full_up || !c->hash_ok || c->hash_nf != nf) {
                ctx_host_hash(c, host, nf, false, c->host_hash);
                ctx_host_hash(c, host, nf, true, c->host_hash1);
            } else if (c->res_steps % verify == 0) {
                // layer 1 changes with every shell download: its reference is
                // retaken only before a step that checks (the next one)
                ctx_host_hash(c, host, nf, true, c->host_hash1);
            }
            c->hash_nf = nf;
            c->hash_ok = 1;
        }
    }
    if (s == CFD_SUCCESS && stats && f->T && !shell) {
        // compute_max_temperature (solver_registry.c:52-62) on the host copy,
        // threaded (r06: one core took ~0.1 s of a 512^3 host-buffer step)
        stats->max_temperature = ctx_host_max(f->T, c->nx * c->ny * c->nz);
    }
    return s;
}

extern "C" __attribute__((visibility("hidden"))) cfd_status_t hip_proj_step_iter_internal(
    hip_proj_ctx_t* c, flow_field* f, const grid* g, const ns_solver_params_t* prm,
    ns_solver_stats_t* stats, int n_steps) {
    return host_steps(c, f, g, prm, stats, n_steps, false);
}

extern "C" __attribute__((visibility("hidden"))) cfd_status_t hip_proj_step_host_internal(
    hip_proj_ctx_t* c, flow_field* f, const grid* g, const ns_solver_params_t* prm,
    ns_solver_stats_t* stats) {
    return host_steps(c, f, g, prm, stats, 1, true);
}

extern "C" __attribute__((visibility("hidden"))) int hip_proj_matches_internal(const hip_proj_ctx_t* c,
                                                                    size_t nx, size_t ny,
                                                                    size_t nz) {
    return c && c->nranks == 1 && c->nx == nx && c->ny == ny && c->nzg == nz;
}

extern "C" {

cfd_status_t hip_proj_step(hip_proj_ctx_t* c, flow_field* f, const grid* g,
                           const ns_solver_params_t* prm, ns_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return host_steps(c, f, g, prm, stats, 1, true);
}

cfd_status_t hip_proj_sync_host(hip_proj_ctx_t* c, flow_field* f) {
    GroupHostLock hl_(c);
    if (!c || !f) return CFD_ERROR_INVALID;
    if (f->nx != c->nx || f->ny != c->ny || f->nz != c->nz) return CFD_ERROR_INVALID;
    ST_TRY(hip_proj_download(c, f));
    if (c->resident && f->T && c->T) ST_TRY(hip_proj_get_field(c, HIP_FIELD_T, f->T));
    c->res_steps = 0;
    c->hash_ok = 0;
    if (c->resident && c->cfg.dirty_verify_interval > 0) {  // the guard's new reference
        double* host[5];
        double* dev[5];
        const int nf = host_fields(c, f, host, dev);
        ctx_host_hash(c, host, nf, false, c->host_hash);
        ctx_host_hash(c, host, nf, true, c->host_hash1);
        c->hash_nf = nf;
        c->hash_ok = 1;
    }
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_poisson_solve(hip_proj_ctx_t* c, int method, double* x, const double* rhs,
                                    double dx, double dy, double dz,
                                    const poisson_solver_params_t* params,
                                    poisson_solver_stats_t* stats) {
    GroupHostLock hl_(c);
    return hip_proj_poisson_solve_ex(c, method, x, rhs, dx, dy, dz, params, stats,
                                     HIP_POISSON_BC_NEUMANN, nullptr);
}

static cfd_status_t poisson_solve_impl(hip_proj_ctx_t* c, int method, double* x,
                                       const double* rhs, double dx, double dy, double dz,
                                       const poisson_solver_params_t* params,
                                       poisson_solver_stats_t* stats);

cfd_status_t hip_proj_poisson_solve_ex(hip_proj_ctx_t* c, int method, double* x,
                                       const double* rhs, double dx, double dy, double dz,
                                       const poisson_solver_params_t* params,
                                       poisson_solver_stats_t* stats, int bc_mode,
                                       const double* bc_values) {
    GroupHostLock hl_(c);
    if (c) c->resident = 0;  // the solve reuses the step's pressure buffers
    if (!c || !x || !rhs) return CFD_ERROR_INVALID;
    if (bc_mode != HIP_POISSON_BC_NEUMANN && bc_mode != HIP_POISSON_BC_NONE &&
        bc_mode != HIP_POISSON_BC_FIXED)
        return CFD_ERROR_INVALID;
    if (bc_mode == HIP_POISSON_BC_FIXED && !bc_values) return CFD_ERROR_INVALID;
    if (bc_mode != HIP_POISSON_BC_NEUMANN && dist(c)) {
        set_err(CFD_ERROR_UNSUPPORTED, "hip_proj_poisson_solve_ex: caller BCs on Z-slabs");
        return CFD_ERROR_UNSUPPORTED;
    }
    if (method == HIP_POISSON_BICGSTAB) {  // refused before anything is uploaded
        const char* why = nullptr;
        if (bc_mode == HIP_POISSON_BC_FIXED)
            why = "hip_proj_poisson_solve_ex: BiCGSTAB takes BC_NEUMANN or BC_NONE, not BC_FIXED";
        else if (dist(c))
            why = "hip_proj_poisson_solve_ex: BiCGSTAB runs on one device, not on Z-slabs";
        else if (c->cfg.cg_variant == 1)
            why = "hip_proj_poisson_solve_ex: BiCGSTAB needs a cg_variant 0 context";
        if (why) {
            set_err(CFD_ERROR_UNSUPPORTED, why);
            return CFD_ERROR_UNSUPPORTED;
        }
    }
    ST_TRY(transform_refuse_slab(c, method));
    if (method == HIP_POISSON_DCT && bc_mode != HIP_POISSON_BC_NEUMANN) {
        // the cosine transform diagonalises the Neumann problem only
        set_err(CFD_ERROR_UNSUPPORTED,
                "hip_proj_poisson_solve_ex: the DCT solve takes BC_NEUMANN only");
        return CFD_ERROR_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (bc_mode == HIP_POISSON_BC_FIXED) {
        if (!c->bcfix) ST_TRY(dalloc(c, &c->bcfix, field_elems(c)));
        HIP_TRY(copy_in(c, c->bcfix, bc_values));
    }
    c->poisson_bc = bc_mode;
    const cfd_status_t s = poisson_solve_impl(c, method, x, rhs, dx, dy, dz, params, stats);
    c->poisson_bc = HIP_POISSON_BC_NEUMANN;
    return s;
}

static cfd_status_t poisson_solve_impl(hip_proj_ctx_t* c, int method, double* x,
                                       const double* rhs, double dx, double dy, double dz,
                                       const poisson_solver_params_t* params,
                                       poisson_solver_stats_t* stats) {
    double rel = 1e-6, abs_tol = 1e-10, omega = 0.0;
    int maxit = (method == HIP_POISSON_JACOBI) ? 2000 : 5000, ci = 1;
    if (params) {
        rel = params->tolerance;
        abs_tol = params->absolute_tolerance;
        maxit = params->max_iterations;
        ci = std::max(1, params->check_interval);
        omega = params->omega;
        if (params->preconditioner != POISSON_PRECOND_NONE) {
            set_err(CFD_ERROR_UNSUPPORTED, "hip_proj_poisson_solve: preconditioner not supported");
            return CFD_ERROR_UNSUPPORTED;
        }
    }
    cfd_status_t s = ensure_aux(c, true, method == HIP_POISSON_JACOBI);
    if (s != CFD_SUCCESS) return s;
    HIP_TRY(copy_in(c, c->rhs, rhs));
    HIP_TRY(copy_in(c, c->pn, x));
    if (method == HIP_POISSON_JACOBI)
        HIP_TRY(hipMemcpyAsync(c->xt, c->pn, field_elems(c) * sizeof(double),
                               hipMemcpyDeviceToDevice, c->stream));
    if (method == HIP_POISSON_CG) {
        DivCoef dc{};
        s = cg_solve(c, dx, dy, dz, dc, RHS_FROM_ARRAY, rel, abs_tol, maxit, ci, true);
    } else if (method == HIP_POISSON_BICGSTAB) {
        s = bicgstab_solve(c, dx, dy, dz, rel, abs_tol, maxit, ci);
    } else if (transform_kind(method) >= 0) {
        s = transform_solve(c, transform_kind(method), dx, dy, dz, rel, abs_tol);
    } else {
        s = relax_solve(c, method, dx, dy, dz, rel, abs_tol, maxit, ci, omega);
    }
    HIP_TRY(copy_out(c, x, c->pn));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) {
        *stats = c->pstats;
        // the direct solves report their device time (events around the solve)
        if (transform_kind(method) < 0) stats->elapsed_time_ms = 0.0;
    }
    return s;
}

// One transform pass of `method` on its own; fn: the entry point's name
static cfd_status_t transform_impl(hip_proj_ctx_t* c, int method, const char* fn,
                                   double* field_host, int axis, bool inverse) {
    GroupHostLock hl_(c);
    if (!c || !field_host) return CFD_ERROR_INVALID;
    const char* why = nullptr;
    if (axis < 0 || axis > 2) why = "axis must be 0 (x), 1 (y) or 2 (z)";
    else if (axis == 2 && c->nz == 1) why = "a 2-D context has no z axis";
    if (why) {
        char msg[96];
        snprintf(msg, sizeof(msg), "%s: %s", fn, why);
        set_err(CFD_ERROR_INVALID, msg);
        return CFD_ERROR_INVALID;
    }
    ST_TRY(transform_refuse_slab(c, method));
    c->resident = 0;  // the transform runs in the step's pressure buffers
    HIP_TRY(hipSetDevice(c->device));
    ST_TRY(ensure_aux(c, false, true));
    TransformTabs T;
    ST_TRY(tables_of(c, transform_kind(method), &T));
    // the input goes to both fields: the pass reads the interior of one and
    // writes the interior of the other, whose boundary is the caller's
    for (double* d : {c->pn, c->xt}) HIP_TRY(copy_in(c, d, field_host));
    transform_pass(c, T, axis, inverse, c->pn, c->xt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(copy_out(c, field_host, c->xt));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CFD_SUCCESS;
}

cfd_status_t hip_proj_dst_transform(hip_proj_ctx_t* c, double* field_host, int axis) {
    return transform_impl(c, HIP_POISSON_DST, "hip_proj_dst_transform", field_host, axis, false);
}

cfd_status_t hip_proj_dct_transform(hip_proj_ctx_t* c, double* field_host, int axis,
                                    int inverse) {
    return transform_impl(c, HIP_POISSON_DCT, "hip_proj_dct_transform", field_host, axis,
                          inverse != 0);
}

double hip_proj_cg_fixed_iters(hip_proj_ctx_t* c, const double* rhs_host, double dx, double dy,
                               double dz, int iters) {
    if (!rhs_host) return -1.0;
    return hip_proj_cg_fixed_iters_ex(c, rhs_host, dx, dy, dz, iters, 0.0);
}

double hip_proj_cg_fixed_iters_ex(hip_proj_ctx_t* c, const double* rhs_host, double dx,
                                  double dy, double dz, int iters, double rho_over_dt) {
    GroupHostLock hl_(c);
    if (!c || iters <= 0) return -1.0;
    if (hipSetDevice(c->device) != hipSuccess) return -1.0;
    if (!rhs_host && (!c->us || !c->vs || !c->ws)) return -1.0;
    if (rhs_host) {
        if (ensure_aux(c, true, false) != CFD_SUCCESS) return -1.0;
        if (copy_in(c, c->rhs, rhs_host) != hipSuccess) return -1.0;
    }
    hipMemsetAsync(c->pn, 0, field_elems(c) * sizeof(double), c->stream);
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    // rhs_host == NULL: the step's own right-hand side, (rho/dt) div u* of the
    // context's u*, v*, w* (the last step's predictor output), fused into the
    // CG setup exactly as the step forms it
    DivCoef dc{};
    dc.two_dx = 2.0 * dx;
    dc.two_dy = 2.0 * dy;
    dc.inv_2dz = (c->nzg > 1 && dz > 0.0) ? 1.0 / (2.0 * dz) : 0.0;
    dc.rho_over_dt = rho_over_dt;
    hipEventRecord(a, c->stream);
    // zero tolerances: no early exit, exactly `iters` iterations
    cfd_status_t s = cg_solve(c, dx, dy, dz, dc, rhs_host ? RHS_FROM_ARRAY : RHS_FROM_VELOCITY,
                              0.0, 0.0, iters, 1, false);
    (void)s;
    hipEventRecord(b, c->stream);
    hipEventSynchronize(b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a);
    hipEventDestroy(b);
    return (double)ms;
}

}  // extern "C"
