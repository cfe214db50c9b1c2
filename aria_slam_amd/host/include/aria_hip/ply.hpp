// The ASCII PLY file HipMapper::exportPLY and HipTsdfVolume::exportPLY write (the reference's Mapper::exportPLY,
// src/legacy/Mapper.cpp:170-200): float x y z, uchar red green blue with r = g = b = the record's gray byte, coordinates in
// ostream's default format. One text for both, so the two files cannot drift apart.
#pragma once
#include <ostream>

namespace aria::adapters::hip {

// Records: a container of structs with `float X[3]` and a `gray` byte (aria_map_point, aria_tsdf_point).
template <class Records>
void writePLY(std::ostream& file, const Records& recs) {
    file << "ply\n";
    file << "format ascii 1.0\n";
    file << "element vertex " << recs.size() << "\n";
    file << "property float x\n";
    file << "property float y\n";
    file << "property float z\n";
    file << "property uchar red\n";
    file << "property uchar green\n";
    file << "property uchar blue\n";
    file << "end_header\n";
    for (const auto& p : recs) {
        const int g = p.gray;
        file << p.X[0] << " " << p.X[1] << " " << p.X[2] << " " << g << " " << g << " " << g << "\n";
    }
}

}  // namespace aria::adapters::hip
