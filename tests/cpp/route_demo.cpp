// route_demo.cpp -- a headless caller that plans over saved maps, through the drop-in facade and the C-ABI only.
// SurfelMapping::groundMaps rasters the records of the map files over the window given on the command line,
// SurfelMapping::routeGround computes two cost-to-go fields over it -- to the goal given, and to that goal or the window's far corner --
// and the path of one start in each; the fields go to stdout, a row of cells a line.  GlobalModel::routeGround does the same over the
// same ground map.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

template <typename T>
static void plane(const char *name, int field, const T *v, int nu, int nv)
{
    for (int r = 0; r < nv; ++r) {
        std::printf("%s %d %d:", name, field, r);
        for (int i = 0; i < nu; ++i) std::printf(" %lld", (long long)v[(size_t)r * nu + i]);
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 14) {
        std::printf("usage: route_demo cell_mm nu nv reach_cells body_cells soft_cells near_weight goal_u goal_v start_u start_v max_steps map files...\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    sm_ground_params gp;
    sm_default_ground_params(&gp);
    gp.cell_mm = std::atoi(argv[1]);
    gp.nu = std::atoi(argv[2]);
    gp.nv = std::atoi(argv[3]);
    gp.reach_cells = std::atoi(argv[4]);
    sm_route_params rp;
    sm_default_route_params(&rp);
    rp.body_cells = std::atoi(argv[5]);
    rp.soft_cells = std::atoi(argv[6]);
    rp.near_weight = std::atoi(argv[7]);
    rp.unknown_passable = 1;
    rp.max_steps = std::atoi(argv[12]);
    const RouteGoal goal{std::atoi(argv[8]), std::atoi(argv[9])};
    const int su = std::atoi(argv[10]), sv = std::atoi(argv[11]);
    std::vector<std::string> files;
    for (int i = 13; i < argc; ++i) files.push_back(argv[i]);
    const GroundMap g = core.groundMaps(files, &gp);
    if (!g.ok) return 1;
    const std::vector<std::vector<RouteGoal>> goals = {{goal}, {goal, RouteGoal{g.nu - 1, g.nv - 1}}};
    const std::vector<RouteStart> starts = {{0, su, sv}, {1, su, sv}};
    const RouteField r = core.routeGround(g, goals, starts, &rp);
    if (!r.ok) return 1;
    for (int f = 0; f < r.fields; ++f) {
        const sm_route_info &i = r.info[f];
        std::printf("route %d: goals %u dropped %u reachable %u max %u\n", f, i.goals_used, i.goals_dropped, i.reachable, i.max_cost);
        plane("cost", f, r.cost.data() + (size_t)f * r.nu * r.nv, r.nu, r.nv);
        plane("next", f, r.next.data() + (size_t)f * r.nu * r.nv, r.nu, r.nv);
    }
    for (size_t s = 0; s < r.paths.size(); ++s) {
        std::printf("path %zu: cost %u cells", s, r.pathCost[s]);
        for (uint32_t c : r.paths[s]) std::printf(" %u", c);
        std::printf("\n");
    }
    // the same through the model's entry point
    const RouteField again = core.getGlobalModel().routeGround(g, goals, starts, &rp);
    if (!again.ok || again.cost != r.cost || again.next != r.next || again.paths != r.paths) return 1;
    std::printf("model: the same\n");
    // calls that are refused: a goal outside the window, a ground map that failed
    if (core.routeGround(g, {{RouteGoal{g.nu, 0}}}).ok) return 1;
    if (core.routeGround(GroundMap{}, goals).ok) return 1;
    return 0;
}
