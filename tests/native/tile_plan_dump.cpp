// tile_plan_dump -- prints the tile plan (cfd_amd/csrc/hip/tile_plan.hpp) of
// every case read from stdin, one JSON object per line. No GPU, no HIP:
// tests/test_tile_plan.py builds it with a host compiler under ASan + UBSan.
//
// A case is one line of KEY=VALUE tokens:
//   shape=NXxNYxNZ   the global grid (required)
//   ranks=N rank=R   a Z-slab rank: its local nz and plane offset come from
//                    the planner's own slab split (default: one device)
//   grid_cap=N       default 2048
//   sweep_rows= sweep_variant= kchunk= cg_variant=   hip_proj_config_t fields
//                    (defaults: hip_proj_config_default's 16, 15, 0, 0)
//   only=sweep_variants   print only the normalised sweep_variant of the
//                    plans with config sweep_variant 0 .. 63, as one array
//   UPPER_CASE=V     the switch CFD_HIP_UPPER_CASE, set in the environment for
//                    this case and read back through read_knobs()
// Geo and SGeo records print as arrays in the order of GEO_FIELDS /
// SGEO_FIELDS below (test_tile_plan.py names them the same way); an SGeo the
// plan leaves unused (all zero) prints as null.
#include <cctype>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tile_plan.hpp"

using namespace cfdhip;

// GEO_FIELDS: nx ny nz px ps sz k0 k1 kc tiles_x tiles_y tiles_z lo_face hi_face kofs
static std::string geo_json(const Geo& g) {
    std::ostringstream o;
    o << '[' << g.nx << ',' << g.ny << ',' << g.nz << ',' << g.px << ',' << g.ps << ',' << g.sz
      << ',' << g.k0 << ',' << g.k1 << ',' << g.kc << ',' << g.tiles_x << ',' << g.tiles_y << ','
      << g.tiles_z << ',' << g.lo_face << ',' << g.hi_face << ',' << g.kofs << ']';
    return o.str();
}

// SGEO_FIELDS: nx ny nz px ps sz k0 k1 kc tiles_x tiles_y tiles_z kmode
//              part_ofs part_total kofs kt0 kt1 xofs kc2 nz1
static std::string sgeo_json(const SGeo& g) {
    const long long v[] = {g.nx, g.ny, g.nz, g.px, g.ps, g.sz, g.k0, g.k1, g.kc, g.tiles_x,
                           g.tiles_y, g.tiles_z, g.kmode, g.part_ofs, g.part_total, g.kofs,
                           g.kt0, g.kt1, g.xofs, g.kc2, g.nz1};
    bool any = false;
    for (long long x : v) any = any || x != 0;
    if (!any) return "null";
    std::ostringstream o;
    o << '[';
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o << (i ? "," : "") << v[i];
    o << ']';
    return o.str();
}

static int fail(const std::string& line, const char* why) {
    fprintf(stderr, "tile_plan_dump: %s: %s\n", why, line.c_str());
    return 2;
}

int main() {
    std::string line;
    std::vector<std::string> set_vars;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        for (const std::string& v : set_vars) unsetenv(v.c_str());
        set_vars.clear();
        PlanIn in;
        in.sweep_rows = 16;
        in.sweep_variant = 15;
        size_t nzg = 0;
        std::string only;
        std::istringstream toks(line);
        std::string tok;
        while (toks >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || eq == 0) return fail(line, "token without KEY=");
            const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
            if (std::isupper((unsigned char)key[0])) {
                const std::string name = "CFD_HIP_" + key;
                setenv(name.c_str(), val.c_str(), 1);
                set_vars.push_back(name);
            } else if (key == "shape") {
                unsigned long a = 0, b = 0, c = 0;
                if (sscanf(val.c_str(), "%lux%lux%lu", &a, &b, &c) != 3)
                    return fail(line, "shape is not NXxNYxNZ");
                in.nx = a;
                in.ny = b;
                nzg = c;
            } else if (key == "only") {
                only = val;
            } else {
                const int v = atoi(val.c_str());
                if (key == "ranks") in.nranks = v;
                else if (key == "rank") in.rank = v;
                else if (key == "grid_cap") in.grid_cap = v;
                else if (key == "sweep_rows") in.sweep_rows = v;
                else if (key == "sweep_variant") in.sweep_variant = v;
                else if (key == "kchunk") in.kchunk = v;
                else if (key == "cg_variant") in.cg_variant = v;
                else return fail(line, "unknown key");
            }
        }
        if (in.nx < 3 || in.ny < 3 || nzg == 0 || (nzg > 1 && nzg < 3))
            return fail(line, "grid must be >= 3 points per active axis");
        in.nz = nzg;
        if (in.nranks > 1 && !slab_layout(nzg, in.rank, in.nranks, &in.kofs, &in.nz))
            return fail(line, "no slab split");
        std::ostringstream o;
        o << "{\"case\":\"" << line << "\"";
        if (!only.empty()) {
            if (only != "sweep_variants") return fail(line, "only= knows sweep_variants");
            o << ",\"sweep_variants\":[";
            for (in.sweep_variant = 0; in.sweep_variant < 64; ++in.sweep_variant)
                o << (in.sweep_variant ? "," : "") << plan_tiles(in, read_knobs()).sweep_variant;
            o << "]}";
            puts(o.str().c_str());
            continue;
        }
        const TilePlan p = plan_tiles(in, read_knobs());
        o << ",\"nz_local\":" << in.nz << ",\"kofs\":" << in.kofs << ",\"px\":" << p.px
          << ",\"ps\":" << p.ps << ",\"geo\":" << geo_json(p.geo);
        const struct {
            const char* name;
            const SGeo& g;
        } sgeos[] = {{"sgeo", p.sgeo}, {"sg_edge", p.sg_edge}, {"sg_int", p.sg_int},
                     {"rgeo", p.rgeo}, {"rg_in1", p.rg_in1}, {"rg_edge", p.rg_edge},
                     {"rg_in2", p.rg_in2}, {"rg_main", p.rg_main}, {"rg_strip", p.rg_strip},
                     {"r2geo", p.r2geo}, {"ccgeo", p.ccgeo}, {"cc_edge", p.cc_edge},
                     {"cc_int", p.cc_int}, {"cc_int_red", p.cc_int_red}, {"cc2_edge", p.cc2_edge},
                     {"pgeo", p.pgeo}, {"pgeo16", p.pgeo16}};
        for (const auto& s : sgeos) o << ",\"" << s.name << "\":" << sgeo_json(s.g);
        int rb2_interior = 0;  // r2geo's tiles that k_rb2 marches without boundary tests
        for (int ty = 0; ty < p.r2geo.tiles_y; ++ty)
            for (int tx = 0; tx < p.r2geo.tiles_x; ++tx)
                rb2_interior += rb2_tile_interior(tx, ty, p.r2geo.nx, p.r2geo.ny) ? 1 : 0;
        o << ",\"rb2_interior\":" << rb2_interior << ",\"sweep_ty\":" << p.sweep_ty
          << ",\"sweep_variant\":" << p.sweep_variant << ",\"rb1_tc\":" << p.rb1_tc
          << ",\"rb_strip_tc\":" << p.rb_strip_tc << ",\"split_rb\":" << p.split_rb
          << ",\"split_b\":" << p.split_b << ",\"pc3\":" << p.pc3 << ",\"ccf_tail\":" << p.ccf_tail
          << ",\"ccf_kc2\":" << p.ccf_kc2 << ",\"ccf_edge_dot\":" << (p.ccf_edge_dot ? 1 : 0)
          << ",\"stagger_bytes\":" << p.stagger_bytes << ",\"n_partials\":" << p.n_partials << "}";
        puts(o.str().c_str());
    }
    return 0;
}
