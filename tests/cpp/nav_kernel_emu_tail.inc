}  // namespace
// Drivers of the emulated kernels (see nav_kernel_emu_head.inc): the launch geometry and the launch order of nav_grid.hip's
// entry points.
namespace {
// ip: nx ny nz up_axis band0 band1 min_weight occ_count free_count radius block_d2 soft_d2 penalty unknown_penalty allow_unknown
NavParams emu_params(const int* ip, float occ_tsdf) {
    NavParams P{};
    P.nx = ip[0]; P.ny = ip[1]; P.nz = ip[2]; P.up_axis = ip[3]; P.band0 = ip[4]; P.band1 = ip[5];
    P.nu = P.up_axis == 0 ? P.ny : P.nx;
    P.nv = P.up_axis == 2 ? P.ny : P.nz;
    P.min_weight = ip[6]; P.occ_count = ip[7]; P.free_count = ip[8];
    P.radius = ip[9]; P.block_d2 = ip[10]; P.soft_d2 = ip[11]; P.penalty = ip[12]; P.unknown_penalty = ip[13]; P.allow_unknown = ip[14];
    P.occ_tsdf = occ_tsdf;
    return P;
}
template <typename F>
void emu_launch(int n, F&& lane) {
    blockIdx = dim3e();
    for (int b = 0; b < (n + NAV_BLOCK - 1) / NAV_BLOCK; b++)
        for (int t = 0; t < NAV_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            lane();
        }
}
}  // namespace
extern "C" {
void emu_columns(const int* ip, float occ_tsdf, const unsigned long long* vol, uint8_t* cells) {
    const NavParams P = emu_params(ip, occ_tsdf);
    emu_launch(P.nu * P.nv, [&] { k_nav_columns(P, vol, cells); });
}
// aria_nav_set_cells_device: returns the refusal word
int emu_set_cells(const int* ip, const uint8_t* in, uint8_t* cells, int* err) {
    const NavParams P = emu_params(ip, 0.0f);
    int bad = 0;
    emu_launch(P.nu * P.nv, [&] { k_nav_validate(in, P.nu * P.nv, &bad, err); });
    emu_launch(P.nu * P.nv, [&] { k_nav_adopt(in, P.nu * P.nv, &bad, cells); });
    return bad;
}
// rules 3-5 on the cells: span is scratch
void emu_rebuild(const int* ip, const uint8_t* cells, uint8_t* span, uint16_t* d2, uint16_t* cost, uint32_t* cm) {
    const NavParams P = emu_params(ip, 0.0f);
    const int n = P.nu * P.nv;
    emu_launch(n, [&] { k_nav_span(P, cells, span); });
    emu_launch(n, [&] { k_nav_clearance(P, span, d2); });
    emu_launch(n, [&] { k_nav_cost(P, cells, d2, cost); });
    emu_launch(n, [&] { k_nav_moves(P.nu, P.nv, cost, cm); });
}
void emu_trace(int nu, int nv, const uint32_t* cm, const uint16_t* d2, const int32_t* fields, const int32_t* goals, int n_goals,
               const int32_t* queries, int n_queries, aria_nav_record* records, int32_t* paths, int path_cap, int* err) {
    emu_launch(n_queries, [&] { k_nav_trace(nu, nv, cm, d2, fields, goals, n_goals, queries, n_queries, records, paths, path_cap, err); });
}
}
