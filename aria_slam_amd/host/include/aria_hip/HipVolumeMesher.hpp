// aria::adapters::hip::HipVolumeMesher -- the mesh of the volume over the C-ABI (include/aria_orb_hip.h, "mesh of the volume"):
// the records of a HipTsdfVolume contoured into a closed, oriented triangle mesh by marching tetrahedra, the surface a map
// viewer (the reference's roadmap item H21), a mesh tool or a collision query asks for. The reference has no code for it; the
// definition is the NumPy restatement aria_slam_amd/mesh_ref.py, which the device equals byte for byte.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "aria_hip/HipTsdfVolume.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct VolumeMesherConfig {
    int nx = 256, ny = 256, nz = 128;    // the volume's geometry
    float voxel = 0.05f;
    float origin[3] = {-6.4f, -6.4f, 0.0f};
    int min_weight = 2;
    void* stream = nullptr;
    int device = 0;
    // the geometry (dims, voxel, origin), min_weight and device of a volume
    static VolumeMesherConfig fromVolume(const HipTsdfVolume& volume);
};

struct VolumeMesh {
    std::vector<aria_mesh_vertex> vertices;
    std::vector<aria_mesh_triangle> triangles;
};

class HipVolumeMesher {
public:
    explicit HipVolumeMesher(const VolumeMesherConfig& cfg = {});
    ~HipVolumeMesher();

    // Remembers the volume's records and rebuilds the word per voxel. A volume of other dims, voxel or origin than this
    // mesher's is refused. The volume's stream is synchronised first through its check(); a deferred error of the volume is
    // thrown here, not swallowed. Call it again after the volume changed.
    void update(HipTsdfVolume& volume);
    // (vertices, triangles) of the last update; blocks.
    std::pair<std::int64_t, std::int64_t> count();
    // The whole mesh in canonical order; blocks.
    VolumeMesh extract();
    // The same where the outputs lie in HBM; enqueued, check() synchronises.
    void extractDevice(aria_mesh_vertex* d_vertices, std::int64_t vcap, aria_mesh_triangle* d_triangles, std::int64_t tcap,
                       std::int64_t* d_counts);
    // ASCII PLY: the header and vertex lines HipTsdfVolume::exportPLY writes, plus `element face` with
    // `property list uchar int vertex_indices`. Returns the mesh's (vertices, triangles).
    std::pair<std::size_t, std::size_t> exportPLY(const std::string& filename);
    int check() { return aria_mesh_check(h_.get()); }
    const aria_mesh_config& config() const { return cfg_; }
    aria_mesh_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipVolumeMesher", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipVolumeMesher", where, rc); }
    aria_mesh_config cfg_{};
    detail::StageOwner<aria_mesh_t, aria_mesh_destroy> h_;
};

}  // namespace aria::adapters::hip
