// See aria_hip/HipVolumeMesher.hpp.
#include "aria_hip/HipVolumeMesher.hpp"

#include <fstream>
#include <stdexcept>

namespace aria::adapters::hip {

VolumeMesherConfig VolumeMesherConfig::fromVolume(const HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    VolumeMesherConfig c;
    c.nx = v.nx; c.ny = v.ny; c.nz = v.nz;
    c.voxel = v.voxel;
    for (int a = 0; a < 3; a++) c.origin[a] = v.origin[a];
    c.min_weight = v.min_weight;
    c.device = v.device;
    return c;
}

HipVolumeMesher::HipVolumeMesher(const VolumeMesherConfig& cfg) {
    aria_mesh_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.nx = cfg.nx; cfg_.ny = cfg.ny; cfg_.nz = cfg.nz;
    cfg_.min_weight = cfg.min_weight;
    cfg_.voxel = cfg.voxel;
    for (int a = 0; a < 3; a++) cfg_.origin[a] = cfg.origin[a];
    expect("aria_mesh_create", aria_mesh_create(&cfg_, h_.out()));
}

HipVolumeMesher::~HipVolumeMesher() = default;

void HipVolumeMesher::update(HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    bool same = v.nx == cfg_.nx && v.ny == cfg_.ny && v.nz == cfg_.nz && v.voxel == cfg_.voxel;
    for (int a = 0; a < 3; a++) same = same && v.origin[a] == cfg_.origin[a];
    if (!same) fail("update: the volume has another geometry (dims, voxel or origin)", ARIA_E_INVALID);
    // its stream is not this handle's: drain it. The check reports the volume's deferred error once, so it must not be dropped.
    expect("update: the volume reports a deferred error", volume.check());
    expect("aria_mesh_update_from_volume_device",
           aria_mesh_update_from_volume_device(h_.get(), aria_tsdf_device_voxels(volume.handle())));
}

std::pair<std::int64_t, std::int64_t> HipVolumeMesher::count() {
    std::int64_t n[2] = {0, 0};
    const int rc = aria_mesh_extract(h_.get(), nullptr, 0, nullptr, 0, n);
    if (rc != ARIA_OK && rc != ARIA_E_OUTPUT_TOO_SMALL) fail("aria_mesh_extract", rc);
    return {n[0], n[1]};
}

VolumeMesh HipVolumeMesher::extract() {
    const auto n = count();
    VolumeMesh m;
    m.vertices.resize((std::size_t)n.first);
    m.triangles.resize((std::size_t)n.second);
    std::int64_t got[2] = {0, 0};
    expect("aria_mesh_extract",
           aria_mesh_extract(h_.get(), m.vertices.empty() ? nullptr : m.vertices.data(), n.first,
                             m.triangles.empty() ? nullptr : m.triangles.data(), n.second, got));
    return m;
}

void HipVolumeMesher::extractDevice(aria_mesh_vertex* d_vertices, std::int64_t vcap, aria_mesh_triangle* d_triangles, std::int64_t tcap,
                                    std::int64_t* d_counts) {
    expect("aria_mesh_extract_device", aria_mesh_extract_device(h_.get(), d_vertices, vcap, d_triangles, tcap, d_counts));
}

std::pair<std::size_t, std::size_t> HipVolumeMesher::exportPLY(const std::string& filename) {
    const VolumeMesh m = extract();
    std::ofstream file(filename);
    if (!file.is_open()) throw std::runtime_error("HipVolumeMesher: failed to open " + filename);
    file << "ply\n";
    file << "format ascii 1.0\n";
    file << "element vertex " << m.vertices.size() << "\n";
    file << "property float x\n";
    file << "property float y\n";
    file << "property float z\n";
    file << "property uchar red\n";
    file << "property uchar green\n";
    file << "property uchar blue\n";
    file << "element face " << m.triangles.size() << "\n";
    file << "property list uchar int vertex_indices\n";
    file << "end_header\n";
    for (const aria_mesh_vertex& p : m.vertices) {
        const int g = p.gray;
        file << p.X[0] << " " << p.X[1] << " " << p.X[2] << " " << g << " " << g << " " << g << "\n";
    }
    for (const aria_mesh_triangle& t : m.triangles) file << "3 " << t.v[0] << " " << t.v[1] << " " << t.v[2] << "\n";
    if (!file) throw std::runtime_error("HipVolumeMesher: cannot write " + filename);
    return {m.vertices.size(), m.triangles.size()};
}

}  // namespace aria::adapters::hip
