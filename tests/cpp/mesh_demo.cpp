// mesh_demo.cpp -- a headless caller that turns saved maps into a triangle mesh, through the drop-in facade and the C-ABI only.
// SurfelMapping::meshMaps meshes the records of the map files at voxel_mm and reach, writes the mesh to ply_path and prints its
// counts; the vertices and faces it also asks for must be the ones the counts speak of.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::printf("usage: mesh_demo voxel_mm reach ply_path map files...\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    sm_mesh_params p;
    sm_default_mesh_params(&p);
    p.voxel_mm = std::atoi(argv[1]);
    p.reach = std::atoi(argv[2]);
    std::vector<std::string> files;
    for (int i = 4; i < argc; ++i) files.push_back(argv[i]);
    std::vector<sm_mesh_vertex> vertices;
    std::vector<uint32_t> faces;
    sm_mesh_info info;
    const long n = core.meshMaps(files, &p, argv[3], &vertices, &faces, false, &info);
    if (n < 0) return 1;
    std::printf("mesh: records %llu used %llu cells %u lattice %u cubes %u vertices %u faces %u\n", (unsigned long long)info.records,
                (unsigned long long)info.counts[SM_MESH_USED], info.cells, info.lattice_points, info.cubes, info.vertices, info.faces);
    if (vertices.size() != info.vertices || faces.size() != (size_t)info.faces * 3 || n != (long)info.faces) return 1;
    for (uint32_t v : faces)
        if (v >= info.vertices) return 1;
    // the live model alone (it is empty): a valid empty mesh, no file asked for
    sm_mesh_info none;
    if (core.getGlobalModel().mesh("", p.voxel_mm, p.reach, &none) != 0 || none.vertices != 0) return 1;
    std::printf("model: faces %u\n", none.faces);
    // the output may not be one of the sources
    if (core.meshMaps(files, &p, files[0]) >= 0) return 1;
    return 0;
}
