// tile_plan.hpp -- which tiles a grid gets: the launch geometry of every
// kernel family, the switches (CFD_HIP_*) that shape it, and the Z-slab split.
// Pure integer arithmetic on the C++17 standard library, no HIP header: the
// library's .hip files include it for the context (ctx.hpp), and a host
// compiler builds it alone (tests/native/tile_plan_dump.cpp, pinned by
// tests/test_tile_plan.py against tests/golden/tile_plans.json).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <optional>

#ifdef __HIPCC__
#define CFD_PLAN_HD __host__ __device__
#else
#define CFD_PLAN_HD
#endif

namespace cfdhip {

// ---- tile constants (the kernels' own: kernels.hpp, rb2.hpp, ccf.hpp) -------
constexpr int TX = 64;       // x extent of a tile = one wavefront
constexpr int TY = 4;        // y rows per tile
#ifndef CFD_PR_TY
#define CFD_PR_TY 4
#endif
constexpr int PR_TY = CFD_PR_TY;  // k_pred2 / k_corr2: rows (waves) per workgroup
constexpr int PC_TY = 16;         // k_pred3 / k_corr3: rows per workgroup
constexpr int CGS_MAX_WG = 256;   // k_cg_small: workgroups at most
constexpr int RB2_TC = 32;   // k_rb2: x pairs per tile row
constexpr int RB2_TR = 32;   // tile rows (two per wave)
constexpr int RB2_OX = 56;   // columns written per tile
constexpr int RB2_OY = 24;   // rows written per tile
constexpr int CCF_OX = 60;   // k_ccf: columns written per tile
constexpr int CCF_OY = 28;   // rows written per tile
constexpr int CCF_OY_EDGE = 29;  // ... in the edge-sum form (ccf_body EDGE)

// Sweep variants (template FL of the CG sweeps, kernels.hpp): bit 0 =
// non-temporal stores of the streamed outputs, bit 1 = non-temporal loads of
// inputs no other tile reads.
constexpr int SW_NT_STORE = 1;
constexpr int SW_NT_LOAD = 2;
// Loads of one plane step are issued through a small "bundle": without
// SW_PREFETCH the bundle of plane k is loaded at the top of iteration k (and
// its centre loads are consumed in the same iteration); with SW_PREFETCH the
// bundle of plane k+1 is issued before plane k is processed, so one plane of
// loads stays in flight across the LDS barrier and the arithmetic.
constexpr int SW_PREFETCH = 4;
// bit 3: the two x-edge cells of a row (lane 0's left, lane 63's right
// neighbour) are fetched by ONE load instruction with per-lane addresses;
// bit 4: the centre rows of the inner waves of a stencil field (rows no
// neighbouring tile re-reads as its y halo) are loaded non-temporally.
constexpr int SW_EDGE1 = 8;
constexpr int SW_NT_INNER = 16;

struct Geo {
    int nx, ny, nz;        // points of the local array, boundary included
    long long px;          // row pitch (doubles)
    long long ps;          // plane pitch (doubles)
    long long sz;          // z stencil offset: ps in 3-D, 0 in 2-D (reference stride_z)
    int k0, k1;            // interior planes [k0, k1)
    int kc;                // planes per tile
    int tiles_x, tiles_y, tiles_z;
    int lo_face, hi_face;  // local plane 0 / nz-1 is a global z face (Z-slabs: edge ranks)
    int kofs;              // global index of local plane 0 (Z-slabs)
};

struct SGeo {
    int nx, ny, nz;
    long long px, ps, sz;
    int k0, k1, kc;
    int tiles_x, tiles_y, tiles_z;  // tiles of 128 x TY x kc
    // kmode 1: the two slab-edge planes only (tz 0 -> plane k0, tz 1 -> k1-1),
    // one plane per tile; the launch covering the remaining planes uses
    // k0+1 .. k1-1. A sweep split over several launches shares one partials
    // array: this launch's workgroups own partials [part_ofs, part_ofs +
    // gridDim.x) of part_total, and the last of all part_total workgroups
    // (same stream, so the later launch) finishes the reduction.
    int kmode;
    int part_ofs, part_total;
    int kofs;  // global index of local plane 0 (Z-slabs; colour parity)
    // kmode 2 (k_rb1 on slabs): tiles cover planes [kt0, kt1) only, while
    // k0 / k1 still bound the planes that are updated
    int kt0, kt1;
    // k_rb1: x of the first tile's first output column (the narrow
    // remainder strip starts where the full-width tiles end)
    int xofs;
    // k_ccf (kmode 0 / 2): z layers tz < nz1 run kc planes from the range's
    // start; layers tz >= nz1 ("tail") run kc2 planes from plane start +
    // nz1 kc, so the last-dispatched workgroups are short (nz1 = tiles_z:
    // every layer kc planes)
    int kc2, nz1;
};

// Is k_rb2's tile (tx, ty) interior: do the 64 x 32 cells it loads, from
// (56 tx - 4, 24 ty - 4), stay off the faces (columns 1 .. nx - 3, rows
// 2 .. ny - 3)? Interior tiles march without the per-cell boundary tests.
CFD_PLAN_HD constexpr bool rb2_tile_interior(int tx, int ty, int nx, int ny) {
    const int ilo = tx * RB2_OX - 4, jlo = ty * RB2_OY - 4;
    return ilo >= 1 && ilo + 2 * RB2_TC - 1 <= nx - 3 && jlo >= 2 && jlo + RB2_TR - 1 <= ny - 3;
}

// ---- the switches -----------------------------------------------------------
// Every CFD_HIP_* switch of the solve paths and of the tiling, read ONCE when
// the context is created (read_knobs), never per step or per solve: rank
// threads of an in-process group would otherwise look the environment up
// while another thread of the process (a test fixture, the runtime) may
// change it, and that lookup is not safe against a concurrent setenv /
// putenv. Tests set the variables before they create contexts.
struct Knobs {
    bool ccf_off = false;     // CFD_HIP_CCF=0: k_cc1 + k_cc2 instead of k_ccf
    int cg_small = -1;        // CFD_HIP_CG_SMALL (-1 unset, 0 never, 1 up to 1M cells)
    int rb2_test = 0;         // CFD_HIP_RB2_TEST: force k_rb2's host paths
    int rb2_xmap = 0;         // CFD_HIP_RB2_XMAP (experiments)
    bool rb2_log = false;     // CFD_HIP_RB2_LOG (diagnostics)
    int rb2 = 1;              // CFD_HIP_RB2: 1 certified fast, 2 exact, 0 k_rb1
    int ccf_xmap = 0;         // CFD_HIP_CCF_XMAP: k_ccf tile order (experiments)
    bool cgb_rev = true;      // CFD_HIP_CGB_REV=0: sweep B marches upwards
    bool rb1_pf = true;       // CFD_HIP_RB1_PF=0: k_rb1 end-of-step loads
    bool rb1_alt = true;      // CFD_HIP_RB1_ALT=0: every k_rb1 sweep upwards
    bool rb1_fold = true;     // CFD_HIP_RB1_FOLD=0: separate k_rx_shell launch
    bool rk_pair = true;      // CFD_HIP_RK_PAIR=0: per-cell RK4 stage
    bool alloc_contig = false;  // CFD_HIP_ALLOC=contig: contiguous field allocations
    bool ccf_edge_side = true;  // CFD_HIP_CCF_EDGE_SIDE=0: slab edge march before the interior

    // ---- requests to the planner: only plan_tiles reads the members below.
    // The launch code reads what the plan made of them (TilePlan: rb1_tc,
    // pc3, ccf_tail, ccf_edge_dot, the geometries), which is validated and
    // depends on the shape and the rank; the four that share a name with a
    // plan member carry _req so that c->env.x cannot stand in for c->x.
    bool ccf_edge_dot_req = true;  // CFD_HIP_CCF_EDGE_DOT=0: one device keeps delta = (A r, r) cell by cell
    // field k starts k x 4 KiB into its allocation (r06): the march reads
    // r_it and p_{it-1} and writes p_it and r_{it+1} at equal offsets of
    // different fields, and with every field 2 MiB-aligned those streams meet
    // on the same HBM channels. 512^3 k_ccf, one box, four interleaved
    // rounds: 1.026-1.055 ms per iteration against 1.039-1.089 unstaggered
    // (2 / 1 / 8 KiB: 1.029-1.059 / 1.028-1.067 / 1.029-1.079,
    // profiles/r06l_ccf_stagger_ab.jsonl; r06k another box, same order).
    // Textbook CG's sweeps measured 0.8 % slower staggered (1.302-1.335 vs
    // 1.292-1.302 ms, r06m, where the march gained 1.044-1.048 vs
    // 1.038-1.062, profiles/r06m_stagger_both_cg_ab.jsonl), so the stagger
    // is the single-reduction contexts' default only.
    // CFD_HIP_FIELD_STAGGER=N overrides (0: aligned fields)
    std::optional<long> field_stagger;
    // CFD_HIP_ROW_PAD=N (experiments, r06): N more doubles per row (a
    // multiple of 8), so that rows do not start on 4 KiB boundaries
    int row_pad = 0;
    // k_rb1 tile width: TC = 64 (128 x 16 cells loaded, 124 x 12 written). The
    // narrower tiles (32: 64 x 32, 16: 32 x 64) need ~20 % fewer
    // workgroups at 512^3 and 1024^2 x 512 but mask their halo rows per
    // lane instead of skipping whole waves, and measured slower (0.846 /
    // 1.022 vs 0.734 ms at 512^3, profiles/r02_rb_tile_width.jsonl);
    // CFD_HIP_RB1_TC = 32 / 16 selects them (experiments)
    int rb1_tc_req = 64;
    int rb1_kc = 64;          // CFD_HIP_RB1_KC: k_rb1's longest z run (experiments)
    bool rb1_strip = true;    // CFD_HIP_RB1_STRIP=0: no TC-16 remainder strip (plan_rb1_strip)
    // CFD_HIP_RB_SPLIT=0 keeps the one-launch k_rb1 iteration with blocking
    // exchanges on Z-slabs (A/B)
    bool rb_split = true;
    std::optional<int> rb2_kc;  // CFD_HIP_RB2_KC: k_rb2's z run in place of 128 / a third
    // CFD_HIP_RB2_KC_FIXED (tests): the run length as given, so small
    // grids reach the steady steps of the march (runs of 9+ planes)
    bool rb2_kc_fixed = false;
    std::optional<int> ccf_kc;  // CFD_HIP_CCF_KC: k_ccf's z run (experiments)
    bool ccf_kc_fixed = false;  // CFD_HIP_CCF_KC_FIXED (tests): not halved on small grids
    // tail layers of shorter runs (experiments: CFD_HIP_CCF_TAIL = layers,
    // CFD_HIP_CCF_KC2 = their run length, half the run by default; default off)
    int ccf_tail_req = 0;
    std::optional<int> ccf_kc2;
    bool ccf_slab_fused = true;  // CFD_HIP_CCF_SLAB_FUSED=0: slabs reduce the march and k_cc2 apart
    // default k_pred3 / k_corr3 (r03: predictor 1.47 -> 1.25 ms, fetch
    // 45.7 -> 25.6 B/cell at 512^3, profiles/r03_pc3.jsonl);
    // CFD_HIP_PC3=0 selects k_pred2 / k_corr2, 2 / 4 the A/B forms (ctx.hpp)
    int pc3_req = 1;

    // ---- context creation (create_common)
    // placement draws (projection_hip.hip, placement_draws): a pool of 6
    // allocated sets and 40 probes: the 6 sets as allocated, then 34 random
    // assignments of pool buffers to the seven roles.
    // r06x, 512^3, contexts of one process (ms per iteration): none
    // 1.109-1.201; 8 sets 1.037-1.126; 2 sets + 16 probes 1.033-1.047
    // with one 1.198 (a pool with no good pair); 4 sets + 16 probes
    // 1.030-1.044 (profiles/r06x_placement_strategies.jsonl). r06ar,
    // twelve contexts each: 4 sets + 24 probes 1.034-1.048 (mean
    // 1.0400), 6 + 40 1.032-1.042 (1.0372), 4 + 48 1.036-1.061
    // (profiles/r06ar_placement_draws.jsonl); ~0.3 s more per context.
    // CFD_HIP_PLACEMENT_DRAWS = sets (1: off), _TRIALS = probes
    int placement_draws = 6;
    int placement_trials = 40;
};

inline Knobs read_knobs() {
    auto ienv = [](const char* name, int dflt) {
        const char* e = getenv(name);
        return e ? atoi(e) : dflt;
    };
    auto oenv = [](const char* name) {
        const char* e = getenv(name);
        return e ? std::optional<int>(atoi(e)) : std::nullopt;
    };
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    Knobs k;
    k.ccf_off = ienv("CFD_HIP_CCF", 1) == 0;
    k.cg_small = ienv("CFD_HIP_CG_SMALL", -1);
    k.rb2_test = ienv("CFD_HIP_RB2_TEST", 0);
    k.rb2_xmap = ienv("CFD_HIP_RB2_XMAP", 0);
    k.rb2_log = set("CFD_HIP_RB2_LOG");
    k.rb2 = ienv("CFD_HIP_RB2", 1);
    k.ccf_xmap = ienv("CFD_HIP_CCF_XMAP", 0);
    k.cgb_rev = ienv("CFD_HIP_CGB_REV", 1) != 0;
    k.rb1_pf = ienv("CFD_HIP_RB1_PF", 1) != 0;
    k.rb1_alt = ienv("CFD_HIP_RB1_ALT", 1) != 0;
    k.rb1_fold = ienv("CFD_HIP_RB1_FOLD", 1) != 0;
    k.rk_pair = ienv("CFD_HIP_RK_PAIR", 1) != 0;
    if (const char* e = getenv("CFD_HIP_ALLOC")) k.alloc_contig = strcmp(e, "contig") == 0;
    k.ccf_edge_side = ienv("CFD_HIP_CCF_EDGE_SIDE", 1) != 0;
    k.ccf_edge_dot_req = ienv("CFD_HIP_CCF_EDGE_DOT", 1) != 0;
    if (const char* e = getenv("CFD_HIP_FIELD_STAGGER")) k.field_stagger = atol(e);
    k.row_pad = ienv("CFD_HIP_ROW_PAD", 0);
    k.rb1_tc_req = ienv("CFD_HIP_RB1_TC", 64);
    k.rb1_kc = std::max(1, ienv("CFD_HIP_RB1_KC", 64));
    k.rb1_strip = ienv("CFD_HIP_RB1_STRIP", 1) != 0;
    k.rb_split = ienv("CFD_HIP_RB_SPLIT", 1) != 0;
    k.rb2_kc = oenv("CFD_HIP_RB2_KC");
    k.rb2_kc_fixed = set("CFD_HIP_RB2_KC_FIXED");
    k.ccf_kc = oenv("CFD_HIP_CCF_KC");
    k.ccf_kc_fixed = set("CFD_HIP_CCF_KC_FIXED");
    k.ccf_tail_req = ienv("CFD_HIP_CCF_TAIL", 0);
    k.ccf_kc2 = oenv("CFD_HIP_CCF_KC2");
    k.ccf_slab_fused = ienv("CFD_HIP_CCF_SLAB_FUSED", 1) != 0;
    k.pc3_req = ienv("CFD_HIP_PC3", 1);
    k.placement_draws = ienv("CFD_HIP_PLACEMENT_DRAWS", 6);
    k.placement_trials = std::max(1, ienv("CFD_HIP_PLACEMENT_TRIALS", 40));
    return k;
}

// ---- the Z-slab split ---------------------------------------------------------
// Interior planes 1 .. nz - 2 split as evenly as possible, lower ranks first;
// a slab is its planes plus one halo plane on each side. false: no such split
// (fewer interior planes than ranks).
inline bool slab_layout(size_t nz, int rank, int size, size_t* k_offset, size_t* nz_local) {
    if (nz < 3 || size < 1 || rank < 0 || rank >= size || (size_t)size > nz - 2) return false;
    const size_t nint = nz - 2, base = nint / (size_t)size, rem = nint % (size_t)size;
    const size_t r = (size_t)rank;
    const size_t first = 1 + r * base + std::min(r, rem);
    const size_t count = base + (r < rem ? 1 : 0);
    if (k_offset) *k_offset = first - 1;
    if (nz_local) *nz_local = count + 2;
    return true;
}

// ---- the plan -----------------------------------------------------------------
struct PlanIn {
    size_t nx = 0, ny = 0, nz = 0;  // the local array (a slab: with its halo planes)
    int rank = 0, nranks = 1;
    size_t kofs = 0;                // global index of local plane 0
    int grid_cap = 2048;            // workgroups a grid-stride launch is capped at (8 per CU)
    // hip_proj_config_t
    int sweep_rows = 0, sweep_variant = 0, kchunk = 0, cg_variant = 0;
};

struct TilePlan {
    long long px = 0, ps = 0;  // row and plane pitch (doubles)
    Geo geo{};                 // 64 x 4 tiles of the grid-stride kernels
    SGeo sgeo{};               // row-pair CG sweep tiling
    int sweep_ty = 8;          // waves (y rows) per CG sweep workgroup
    int sweep_variant = 0;     // SW_* flags of the CG sweeps, one of the variants built
    SGeo sg_edge{}, sg_int{};  // slabs: sweep B split into edge planes + interior
    int split_b = 0;
    SGeo rgeo{};               // single-pass RB-SOR tiling (k_rb1)
    int rb1_tc = 64;           // k_rb1 tile width in x pairs (64, 32, 16)
    // slabs: one k_rb1 iteration as three launches sharing one reduction --
    // interior part 1 (overlaps the R halo exchange), the two edge planes,
    // interior part 2 (overlaps the exchange of the new iterate's edge planes)
    SGeo rg_in1{}, rg_edge{}, rg_in2{};
    int split_rb = 0;
    // one device: k_rb1's full-width (TC 64) tiles stop at x = 124 T, and the
    // remaining columns run as a strip of narrow tiles (TC 16) in the same
    // grid, sharing the residual reduction (rb_strip_tc 0: none)
    SGeo rg_main{}, rg_strip{};
    int rb_strip_tc = 0;
    SGeo r2geo{};              // two-iterations-per-sweep RB-SOR tiling (k_rb2; tiles_x 0: none)
    SGeo ccgeo{};              // fused single-reduction CG tiling (k_ccf; tiles_x 0: none)
    SGeo cc_edge{}, cc_int{};  // slabs: k_ccf on the edge planes, then the rest
    // slabs, fused form: cc_int with stage c and a shared reduction, and
    // k_cc2's tiling of the two edge planes completing it (tiles_x 0: off)
    SGeo cc_int_red{}, cc2_edge{};
    int ccf_tail = 0, ccf_kc2 = 0;  // k_ccf tail layers of shorter runs (ccf_layout)
    bool ccf_edge_dot = false;      // ccgeo is the edge-sum form's tiling (one device, 60 x 29)
    SGeo pgeo{};               // predictor / corrector z-march tiling (k_pred2, k_corr2)
    SGeo pgeo16{};             // k_pred3 / k_corr3: 128 x 16 tiles, y rows in LDS
    int pc3 = 1;  // 0: k_pred2 / k_corr2; k_pred3 / k_corr3 with 1: FL 0 (default), 2: NT stores, 4: + NT loads
    size_t stagger_bytes = 0;  // field k starts k x this into its allocation
    int n_partials = 0;        // reduction slots the largest launch (or group of launches) needs
};

namespace plan_detail {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int tiles(const SGeo& g) { return g.tiles_x * g.tiles_y * g.tiles_z; }
inline void need(TilePlan& p, int n) { p.n_partials = std::max(p.n_partials, n); }

// pitches, the field stagger and the grid-stride kernels' 64 x 4 tiles
inline void plan_grid(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    const size_t nx = in.nx, ny = in.ny, nz = in.nz;
    p.stagger_bytes = (in.cg_variant == 1) ? 4096 : 0;
    if (kn.field_stagger) p.stagger_bytes = (size_t)*kn.field_stagger / 256 * 256;
    p.px = (long long)((nx + 7) / 8 * 8);
    p.px += (long long)(std::max(0, kn.row_pad) / 8 * 8);
    p.ps = p.px * (long long)ny;
    Geo& g = p.geo;
    g.nx = (int)nx;
    g.ny = (int)ny;
    g.nz = (int)nz;
    g.px = p.px;
    g.ps = p.ps;
    g.sz = (nz > 1) ? p.ps : 0;
    g.k0 = (nz > 1) ? 1 : 0;
    g.k1 = (nz > 1) ? (int)nz - 1 : 1;
    g.lo_face = (in.rank == 0) ? 1 : 0;
    g.hi_face = (in.rank == in.nranks - 1) ? 1 : 0;
    g.kofs = (int)in.kofs;
    const int nint_k = g.k1 - g.k0;
    // enough tiles to fill every CU several times, long z runs otherwise
    const long long xy_tiles = (long long)((nx + TX - 1) / TX) * (long long)((ny + TY - 1) / TY);
    const long long want = 4LL * in.grid_cap;
    int kc = (int)std::max<long long>(8, (xy_tiles * nint_k + want - 1) / want);
    kc = std::min(kc, std::max(1, nint_k));
    g.kc = std::max(1, kc);
    g.tiles_x = (int)((nx + TX - 1) / TX);
    g.tiles_y = (int)((ny + TY - 1) / TY);
    g.tiles_z = cdiv(nint_k, g.kc);
}

// row-pair CG sweeps: 128 x sweep_ty x kc tiles (kernels.hpp, k_cgA / k_cgB)
inline void plan_sweeps(TilePlan& p, const PlanIn& in) {
    const Geo& g = p.geo;
    const int nint_k = g.k1 - g.k0;
    p.sweep_ty = (in.sweep_rows == 4 || in.sweep_rows == 16) ? in.sweep_rows : 8;
    {   // variants built: 0-3 (memory hints), 4 and 7 (+ plane prefetch)
        const int v = in.sweep_variant & 63;
        if (v == 15 && p.sweep_ty >= 8) p.sweep_variant = v;
        else if ((v == 23 || v == 31) && p.sweep_ty == 16) p.sweep_variant = v;
        else p.sweep_variant = (v & SW_PREFETCH) ? ((v & 3) == 3 ? 7 : 4) : (v & 3);
    }
    SGeo& sg = p.sgeo;
    sg.nx = g.nx;
    sg.ny = g.ny;
    sg.nz = g.nz;
    sg.px = g.px;
    sg.ps = g.ps;
    sg.sz = g.sz;
    sg.k0 = g.k0;
    sg.k1 = g.k1;
    sg.kofs = g.kofs;
    sg.tiles_x = (int)((in.nx + 127) / 128);
    sg.tiles_y = (int)((in.ny + p.sweep_ty - 1) / p.sweep_ty);
    if (in.kchunk > 0) {
        sg.kc = in.kchunk;
    } else {
        // long z runs (each chunk re-reads two planes), shortened (down to
        // 4) until every CU has a workgroup: a thin slab or a mid-size grid
        // must still fill all 256 CUs. r01f at 512^3: 256-plane runs (256
        // workgroups) beat 64 by ~2 %; one 8-rank slab: 32 beat 16
        // (profiles/r01f_sweep_*). r02b: the floor was 16, which left 96^3 /
        // 128^3 at 36 / 64 workgroups; 4 takes a CG iteration from 53 to
        // 25 us / 58 to 33 us there (profiles/r02_small_grids.jsonl)
        sg.kc = 256;
        const long long want = in.grid_cap / 8;
        while (sg.kc > 4 && (long long)sg.tiles_x * sg.tiles_y * cdiv(nint_k, sg.kc) < want)
            sg.kc /= 2;
    }
    sg.kc = std::max(1, std::min(sg.kc, nint_k));
    sg.tiles_z = cdiv(nint_k, sg.kc);
    need(p, std::max(in.grid_cap, tiles(sg)));
}

// sweep B on slabs of >= 3 planes: the two edge planes (what the neighbours
// need) first, then planes k0+1 .. k1-1; one reduction over both launches
inline void plan_sweep_b_split(TilePlan& p, const PlanIn& in) {
    const SGeo& sg = p.sgeo;
    p.split_b = (in.nranks > 1 && sg.k1 - sg.k0 >= 3) ? 1 : 0;
    if (!p.split_b) return;
    SGeo& e = p.sg_edge;
    SGeo& m = p.sg_int;
    e = sg;
    e.kmode = 1;
    e.kc = 1;
    e.tiles_z = 2;
    m = sg;
    m.k0 = sg.k0 + 1;
    m.k1 = sg.k1 - 1;
    m.kc = std::max(1, std::min(sg.kc, m.k1 - m.k0));
    m.tiles_z = cdiv(m.k1 - m.k0, m.kc);
    const int ne = tiles(e), nm = tiles(m);
    e.part_ofs = 0;
    m.part_ofs = ne;
    e.part_total = m.part_total = ne + nm;
    need(p, ne + nm);
}

// single-pass RB-SOR (k_rb1): 124 x 12 cells written per 128 x 16 loaded at
// the default width (Knobs::rb1_tc_req)
inline void plan_rb1(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    SGeo& rg = p.rgeo;
    rg = p.sgeo;
    const int nint_k = rg.k1 - rg.k0;
    const int tc = (kn.rb1_tc_req == 64 || kn.rb1_tc_req == 32 || kn.rb1_tc_req == 16) ? kn.rb1_tc_req : 64;
    p.rb1_tc = tc;
    const int ox = 2 * tc - 4, oy = 1024 / tc - 4;
    rg.tiles_x = (int)((in.nx - 1 + ox - 1) / ox);
    rg.tiles_y = (int)((in.ny - 1 + oy - 1) / oy);
    rg.kc = kn.rb1_kc;
    while (rg.kc > 16 && (long long)rg.tiles_x * rg.tiles_y * cdiv(nint_k, rg.kc) < 512)
        rg.kc /= 2;
    // small grids: shorter runs (each costs a two-plane prologue) only
    // while fewer than half the CUs have a workgroup (r02b: 96^3 31 ->
    // 17 us per iteration at 4 planes; 128^3, 176 workgroups at 16
    // planes, is slower at 8 or 4; profiles/r02_small_grids.jsonl)
    while (rg.kc > 4 && (long long)rg.tiles_x * rg.tiles_y * cdiv(nint_k, rg.kc) < 128)
        rg.kc /= 2;
    rg.kc = std::max(1, std::min(rg.kc, nint_k));
    rg.tiles_z = cdiv(nint_k, rg.kc);
    need(p, tiles(rg));
}

// the last x tile of a TC-64 k_rb1 launch is partial unless 124 divides the
// row: its workgroups run a full tile's steps for a few columns
// (512^3: 14 of 124). Up to 28 such columns run instead as a strip
// of TC-16 tiles (28 columns x 60 rows, 4.8x fewer workgroups) in
// the same grid (k_rb1m). Knobs::rb1_strip false: off.
inline void plan_rb1_strip(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    const SGeo& rg = p.rgeo;
    const int nint_k = rg.k1 - rg.k0;
    p.rb_strip_tc = 0;
    if (p.rb1_tc != 64 || in.nranks != 1 || !kn.rb1_strip) return;
    const int T = (int)(in.nx / 124), R = (int)in.nx - 124 * T;
    // TC-32 strips (R in 29..60) measured slower (1024^2 x 512: 2.96 vs
    // 2.93 ms); TC-16 ones faster (512^3: 0.734 vs 0.760 ms,
    // profiles/r03_rb1_strip.jsonl)
    // R = 1 (nx = 124 T + 1): the T full tiles already store every
    // pair (cell nx - 1 is the Neumann mirror), so no strip
    const int stc = (R >= 2 && R <= 28) ? 16 : 0;
    if (!stc) return;
    p.rb_strip_tc = stc;
    SGeo& m = p.rg_main;
    SGeo& q = p.rg_strip;
    m = rg;
    m.tiles_x = T;
    q = rg;
    q.xofs = 124 * T;
    q.tiles_x = 1;
    const int oy = 1024 / stc - 4;
    q.tiles_y = (int)((in.ny - 1 + oy - 1) / oy);
    q.kc = std::max(1, std::min(rg.kc, nint_k));
    q.tiles_z = cdiv(nint_k, q.kc);
    // one grid (k_rb1m): partial slot = blockIdx.x, total = gridDim.x
    m.part_ofs = q.part_ofs = 0;
    m.part_total = q.part_total = 0;
    need(p, tiles(m) + tiles(q));
}

// k_rb1 on Z-slabs of >= 4 planes: output planes k0+1 .. k1-2 split into two
// halves around the edge planes (relax_solve_fused); Knobs::rb_split false
// keeps the one-launch iteration
inline void plan_rb1_split(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    const SGeo& rg = p.rgeo;
    p.split_rb = (in.nranks > 1 && rg.k1 - rg.k0 >= 4 && kn.rb_split) ? 1 : 0;
    if (!p.split_rb) return;
    const int a0 = rg.k0 + 1, a1 = rg.k1 - 1;  // interior output planes [a0, a1)
    const int mid = a0 + (a1 - a0) / 2;
    auto range = [&](SGeo& q, int lo, int hi) {
        q = rg;
        q.kmode = 2;
        q.kt0 = lo;
        q.kt1 = hi;
        q.kc = std::max(1, std::min(rg.kc, hi - lo));
        q.tiles_z = cdiv(hi - lo, q.kc);
    };
    range(p.rg_in1, a0, mid);
    range(p.rg_in2, mid, a1);
    p.rg_edge = rg;
    p.rg_edge.kmode = 1;
    p.rg_edge.kc = 1;
    p.rg_edge.tiles_z = 2;
    const int xy = rg.tiles_x * rg.tiles_y;
    const int n1 = xy * p.rg_in1.tiles_z, ne = xy * 2, n2 = xy * p.rg_in2.tiles_z;
    p.rg_in1.part_ofs = 0;
    p.rg_edge.part_ofs = n1;
    p.rg_in2.part_ofs = n1 + ne;
    p.rg_in1.part_total = p.rg_edge.part_total = p.rg_in2.part_total = n1 + ne + n2;
    need(p, n1 + ne + n2);
}

// two RB-SOR iterations per sweep (k_rb2, rb2.hpp): 64 x 32 cells
// loaded, 56 x 24 written; one device, 3-D. Four partials per
// workgroup (two maxima, the value range).
inline void plan_rb2(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    SGeo& r2 = p.r2geo;
    r2 = p.rgeo;
    r2.tiles_x = r2.tiles_y = r2.tiles_z = 0;
    if (!(in.nranks == 1 && in.nz > 1 && in.nx >= 8 && in.ny >= 8)) return;
    const int nint_k = r2.k1 - r2.k0;
    r2.xofs = 0;
    r2.tiles_x = (int)((in.nx - 1 + RB2_OX - 1) / RB2_OX);
    r2.tiles_y = (int)((in.ny - 1 + RB2_OY - 1) / RB2_OY);
    // 128-plane z runs: the 6-plane pipeline fill is 4.7 % of a run
    // (1024^2 x 512: 2.16 -> 2.05 ms per iteration against 64;
    // 32: 2.34, profiles/r04_rb2_kc.jsonl)
    r2.kc = 128;
    // deep grids with many columns: three runs per column (1024^2 x
    // 512: 170 planes, 2451 workgroups, 1.735-1.739 vs 1.748-1.751 ms
    // per iteration against 128 in four same-box pairs on two boxes;
    // 255: 1.78-1.80, 510: 2.02; profiles/r05as_rb2_kc_ab.jsonl)
    if (nint_k >= 384 && 3LL * r2.tiles_x * r2.tiles_y >= 8LL * std::max(1, in.grid_cap / 8))
        r2.kc = (nint_k + 2) / 3;
    if (kn.rb2_kc) r2.kc = std::max(1, *kn.rb2_kc);
    while (!kn.rb2_kc_fixed && r2.kc > 4 &&
           (long long)r2.tiles_x * r2.tiles_y * cdiv(nint_k, r2.kc) < 512)
        r2.kc /= 2;
    r2.kc = std::max(1, std::min(r2.kc, nint_k));
    r2.tiles_z = cdiv(nint_k, r2.kc);
    need(p, 2 * tiles(r2));
}

// k_ccf's z layers over P planes: runs of kc, and with tail_layers > 0 the
// last tail_layers layers runs of kc2 (< kc) covering the remaining planes,
// so the workgroups dispatched last are short and the launch's tail (each CU
// idles while the last workgroups finish) shrinks. tail_layers = 0: every
// layer kc.
inline void ccf_layout(SGeo& g, int P, int kc, int kc2, int tail_layers) {
    kc = std::max(1, std::min(kc, P));
    g.kc = kc;
    g.kc2 = kc;
    g.nz1 = g.tiles_z = (P + kc - 1) / kc;
    if (tail_layers <= 0 || kc2 <= 0 || kc2 >= kc) return;
    const int tail = std::min(P, tail_layers * kc2);
    const int bulk = P - tail;
    if (bulk <= 0) return;
    g.kc2 = kc2;
    g.nz1 = (bulk + kc - 1) / kc;
    // the bulk's last layer may be partial: the tail then starts at nz1 kc,
    // past the bulk, and covers P - nz1 kc planes
    const int rest = std::max(0, P - g.nz1 * kc);
    g.tiles_z = g.nz1 + (rest + kc2 - 1) / kc2;
}

// the fused single-reduction CG iteration (k_ccf, ccf.hpp): 64 x 32
// cells loaded, 60 x 29 written on one device (delta as an edge sum),
// 60 x 28 on Z-slabs and with Knobs::ccf_edge_dot_req false (delta = (A r, r)
// cell by cell); 3-D
inline void plan_ccf(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    p.ccf_edge_dot = in.nranks == 1 && kn.ccf_edge_dot_req;
    const int ccf_oy = p.ccf_edge_dot ? CCF_OY_EDGE : CCF_OY;
    SGeo& cg = p.ccgeo;
    cg = p.rgeo;
    cg.tiles_x = cg.tiles_y = cg.tiles_z = 0;
    if (!(in.nz >= 3 && in.nx >= 4 && in.ny >= 4)) return;
    const int nint_k = cg.k1 - cg.k0;
    cg.xofs = 0;
    cg.tiles_x = (int)((in.nx - 1 + CCF_OX - 1) / CCF_OX);
    cg.tiles_y = (int)((in.ny - 1 + ccf_oy - 1) / ccf_oy);
    // z-run length: 24 planes on deep grids, 16 on thin ones (r05;
    // r04 had 32). 512^3 on one device: 24 at 1.048-1.049 vs 32's
    // 1.059 ms per iteration in every stable pair on two boxes (20 and
    // 28 equal to 24, 40 slower; profiles/r05ao_ccf_kc_ab.jsonl). The
    // rank-0 slab shapes of 2 / 4 / 8 ranks, 512^2 x 257 / 130 / 66:
    // 16 at 0.600-0.604 / 0.316-0.319 / 0.171 ms against 24's 0.613-
    // 0.615 / 0.317-0.318 / 0.169 and 32's 0.627-0.630 / 0.334-0.335 /
    // 0.197 (profiles/r05at_ccf_kc_thin_ab.jsonl)
    // r06: one device always 24 (256^3: 0.151-0.157 vs 16's 0.159-0.168
    // ms per iteration in three same-box pairs, profiles/r06c_ccf_kc_256_ab.jsonl;
    // the 16 of r05 was measured on 512^2 slab shapes only);
    // Z-slabs: 16, and 11 on slabs of <= 100 planes (512^2 x 66, the
    // 8-rank slab: 0.1615-0.1678 vs 16's 0.1706-0.1712, 13 0.1637-0.1693,
    // 21 0.168, 32 0.189-0.197; profiles/r06c_ccf_kc_slab8_ab.jsonl)
    cg.kc = (in.nranks == 1) ? 24 : (nint_k <= 100 ? 11 : 16);
    if (kn.ccf_kc) cg.kc = std::max(1, *kn.ccf_kc);
    while (!kn.ccf_kc_fixed && cg.kc > 4 &&
           (long long)cg.tiles_x * cg.tiles_y * cdiv(nint_k, cg.kc) < 512)
        cg.kc /= 2;
    p.ccf_tail = kn.ccf_tail_req;
    p.ccf_kc2 = kn.ccf_kc2 ? *kn.ccf_kc2 : cg.kc / 2;
    ccf_layout(cg, nint_k, cg.kc, p.ccf_kc2, p.ccf_tail);
    need(p, tiles(cg));
    // Z-slabs of >= 3 planes: the edge planes' launch (kmode 1) and
    // the interior planes' (kmode 2), so the r halo overlaps the latter
    p.cc_edge = p.cc_int = cg;
    p.cc_edge.tiles_x = p.cc_int.tiles_x = 0;
    if (!(in.nranks > 1 && nint_k >= 3)) return;
    SGeo& e = p.cc_edge;
    SGeo& m = p.cc_int;
    e = m = cg;
    e.kmode = 1;
    e.kc = 1;
    e.tiles_z = 2;
    m.kmode = 2;
    m.kt0 = cg.k0 + 1;
    m.kt1 = cg.k1 - 1;
    ccf_layout(m, m.kt1 - m.kt0, cg.kc, p.ccf_kc2, p.ccf_tail);
    // fused form: the interior march with stage c (cc_int_red)
    // and k_cc2 on the two edge planes (cc2_edge, the row-pair
    // tiling of k_cc2 in kmode 1) share one reduction, the
    // interior workgroups' partials first
    if (!kn.ccf_slab_fused) return;
    SGeo& ir = p.cc_int_red;
    SGeo& ee = p.cc2_edge;
    ir = m;
    ee = p.sgeo;
    ee.kmode = 1;
    ee.kc = 1;
    ee.tiles_z = 2;
    const int ni = tiles(ir), ne = tiles(ee);
    ir.part_ofs = 0;
    ee.part_ofs = ni;
    ir.part_total = ee.part_total = ni + ne;
    need(p, ni + ne);
}

// predictor / corrector: 128 x PR_TY x kc tiles, >= ~8 workgroups per CU
// (k_pred2 / k_corr2), and k_pred3 / k_corr3: the CG sweeps' 128 x 16 tiles,
// long z runs shortened until every CU has a workgroup (one 1024-thread
// workgroup per CU: 110 KB of LDS)
inline void plan_pred_corr(TilePlan& p, const PlanIn& in, const Knobs& kn) {
    const int nint_k = p.sgeo.k1 - p.sgeo.k0;
    SGeo& pg = p.pgeo;
    pg = p.sgeo;
    pg.kmode = 0;
    pg.tiles_x = (int)((in.nx + 127) / 128);
    pg.tiles_y = (int)((in.ny + PR_TY - 1) / PR_TY);
    const long long xy = (long long)pg.tiles_x * pg.tiles_y;
    const long long zt = std::max(1LL, (4LL * in.grid_cap / PR_TY + xy - 1) / xy);
    pg.kc = (int)std::max<long long>(1, (nint_k + zt - 1) / zt);
    pg.tiles_z = cdiv(nint_k, pg.kc);
    SGeo& p3 = p.pgeo16;
    p3 = p.sgeo;
    p3.kmode = 0;
    p3.tiles_x = (int)((in.nx + 127) / 128);
    p3.tiles_y = (int)((in.ny + PC_TY - 1) / PC_TY);
    p3.kc = 256;
    while (p3.kc > 4 &&
           (long long)p3.tiles_x * p3.tiles_y * cdiv(nint_k, p3.kc) < in.grid_cap / 8)
        p3.kc /= 2;
    p3.kc = std::max(1, std::min(p3.kc, nint_k));
    p3.tiles_z = cdiv(nint_k, p3.kc);
    p.pc3 = (kn.pc3_req == 1 || kn.pc3_req == 2 || kn.pc3_req == 4) ? kn.pc3_req : 0;
}

}  // namespace plan_detail

inline TilePlan plan_tiles(const PlanIn& in, const Knobs& kn) {
    using namespace plan_detail;
    TilePlan p;
    plan_grid(p, in, kn);
    plan_sweeps(p, in);
    plan_rb1(p, in, kn);
    plan_rb2(p, in, kn);
    plan_ccf(p, in, kn);
    plan_rb1_strip(p, in, kn);
    plan_rb1_split(p, in, kn);
    plan_pred_corr(p, in, kn);
    plan_sweep_b_split(p, in);
    // k_cg_small indexes its two partial slots by CGS_MAX_WG whatever the CU count
    need(p, CGS_MAX_WG);
    return p;
}

}  // namespace cfdhip
