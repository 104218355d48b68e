// lidar_reader_check.cpp -- KittiReader's lidar flag without a GPU: off by default, the scan instead of the depth image, an empty
// scan as a frame with no points, both flags at once, and the members put back when the flag is switched off.  Prints one line
// per frame; exit 0 if everything is as the header of facade/KittiReader.h says.
#include <cstdio>
#include "../../surfelmapping_amd/csrc/facade/KittiReader.h"

#define CHECK(c) do { if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { std::printf("usage: lidar_reader_check dataset_dir with_right(0|1)\n"); return 2; }
    const bool right = argv[2][0] == '1';
    KittiReader reader(argv[1], right, true, 0, true);
    CHECK(reader.good());
    CHECK(!reader.velodyne && reader.numPoints == 0);
    CHECK(reader.setUseLidar(true));
    CHECK(reader.veloToCam[15] == 1.0f && reader.veloToCam[12] == 0.0f);
    for (int k = 0; k < (int)reader.numFrames(); ++k) {
        CHECK(reader.getNext());
        CHECK(!reader.depth && reader.velodyne && reader.rgb);
        CHECK(right == (reader.rgbRight != nullptr));
        std::printf("frame %d points %u first %.9g\n", k, reader.numPoints, reader.numPoints ? reader.velodyne[0] : 0.0f);
    }
    CHECK(reader.setUseLidar(false));
    CHECK(!reader.velodyne && reader.numPoints == 0);
    return 0;
}
