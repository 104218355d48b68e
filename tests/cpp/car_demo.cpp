// car_demo.cpp -- a headless caller that plans a car's way over saved maps, through the drop-in facade and the C-ABI only.
// SurfelMapping::groundMaps rasters the records of the map files over the window given on the command line,
// SurfelMapping::routeCar computes two cost-to-go fields over (cell, heading) -- to the goal given at any heading, and to that goal at
// heading 0 -- and the path of one start in each; the fields go to stdout, a row of cells a line, heading after heading.
// GlobalModel::routeCar does the same over the same ground map.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

template <typename T>
static void plane(const char *name, int field, int h, const T *v, int nu, int nv)
{
    for (int r = 0; r < nv; ++r) {
        std::printf("%s %d %d %d:", name, field, h, r);
        for (int i = 0; i < nu; ++i) std::printf(" %lld", (long long)v[(size_t)r * nu + i]);
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 16) {
        std::printf("usage: car_demo cell_mm nu nv reach_cells body_cells turn_cells turn_cost reverse_weight goal_u goal_v start_u start_v start_h max_steps"
                    " map files...\n");
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
    sm_route_car_params cp;
    sm_default_route_car_params(&cp);
    cp.body_cells = std::atoi(argv[5]);
    cp.turn_cells = std::atoi(argv[6]);
    cp.turn_cost = std::atoi(argv[7]);
    cp.reverse_weight = std::atoi(argv[8]);
    cp.unknown_passable = 1;
    cp.max_steps = std::atoi(argv[14]);
    const int gu = std::atoi(argv[9]), gv = std::atoi(argv[10]);
    const int su = std::atoi(argv[11]), sv = std::atoi(argv[12]), sh = std::atoi(argv[13]);
    std::vector<std::string> files;
    for (int i = 15; i < argc; ++i) files.push_back(argv[i]);
    const GroundMap g = core.groundMaps(files, &gp);
    if (!g.ok) return 1;
    const std::vector<std::vector<CarGoal>> goals = {{CarGoal{gu, gv, -1}}, {CarGoal{gu, gv, 0}}};
    const std::vector<CarStart> starts = {{0, su, sv, sh}, {1, su, sv, sh}};
    const CarField r = core.routeCar(g, goals, starts, &cp);
    if (!r.ok) return 1;
    const size_t N = (size_t)r.nu * r.nv;
    for (int f = 0; f < r.fields; ++f) {
        const sm_route_car_info &i = r.info[f];
        std::printf("car %d: goals %u dropped %u states %u cells %u max %u\n", f, i.goals_used, i.goals_dropped, i.reachable_states, i.reachable_cells,
                    i.max_cost);
        for (int h = 0; h < 8; ++h) plane("cost", f, h, r.cost.data() + ((size_t)f * 8 + h) * N, r.nu, r.nv);
        for (int h = 0; h < 8; ++h) plane("next", f, h, r.next.data() + ((size_t)f * 8 + h) * N, r.nu, r.nv);
    }
    for (size_t s = 0; s < r.paths.size(); ++s) {
        std::printf("path %zu: cost %u words", s, r.pathCost[s]);
        for (uint32_t w : r.paths[s]) std::printf(" %u/%d/%d", CarField::cell(w), CarField::heading(w), (int)CarField::reverse(w));
        std::printf("\n");
    }
    // the same through the model's entry point
    const CarField again = core.getGlobalModel().routeCar(g, goals, starts, &cp);
    if (!again.ok || again.cost != r.cost || again.next != r.next || again.paths != r.paths) return 1;
    std::printf("model: the same\n");
    // calls that are refused: a goal's heading out of range, a ground map that failed
    if (core.routeCar(g, {{CarGoal{0, 0, 8}}}).ok) return 1;
    if (core.routeCar(GroundMap{}, goals).ok) return 1;
    return 0;
}
