}  // namespace
// Drivers of the emulated kernels (see icp_kernel_emu_head.inc): the launch geometry of icp_track.hip's
// aria_icp_debug_system_device and aria_icp_track_batch_device. The parameters come from the library's own icp_params, in the
// pasted text.
#include <vector>
namespace {
// fp: min_depth max_depth dist_max reach; dp: min_pivot eps; maps: live depth normal; lay: the three strides, then the three pitches
IcpMaps emu_maps(const float* const* maps, const int64_t* lay, int W, int H) {
    return IcpMaps{maps[0], maps[1], maps[2], lay[0], lay[1], lay[2], (int)lay[3], (int)lay[4], (int)lay[5], W, H};
}
template <typename F>
void emu_per_frame(int n, F&& body) {
    blockIdx = dim3e();
    for (int b = 0; b < (n + ICP_BLOCK - 1) / ICP_BLOCK; b++)
        for (int t = 0; t < ICP_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            body();
        }
}
void emu_accumulate(const IcpParams& P, const IcpFrame* frames, const IcpMaps& m, int n, int stride, int level, int plain, long long* acc) {
    const int wl = (m.W + stride - 1) / stride, hl = (m.H + stride - 1) / stride, ppl = plain ? 1 : ICP_PPL;
    for (int f = 0; f < n; f++)
        for (int y = 0; y < (hl + ICP_TILE_H * ppl - 1) / (ICP_TILE_H * ppl); y++)
            for (int x = 0; x < (wl + ICP_TILE_W - 1) / ICP_TILE_W; x++)
                for (int t = 0; t < ICP_BLOCK; t++) {
                    blockIdx.x = x; blockIdx.y = y; blockIdx.z = f; threadIdx.x = t;
                    if (plain) k_icp_accumulate<1>(P, frames, m, stride, level, acc);
                    else k_icp_accumulate<ICP_PPL>(P, frames, m, stride, level, acc);
                }
}
}  // namespace
extern "C" {
void emu_icp_system(const double* K, const float* fp, const double* dp, int min_corr, const float* const* maps, const int64_t* lay,
                    const double* Tm, const double* trel, int n, int W, int H, int stride, int plain, long long* out) {
    const IcpParams P = icp_params(K, fp[0], fp[1], fp[2], fp[3], min_corr, dp[0], dp[1]);
    std::vector<IcpFrame> frames((size_t)n);
    std::vector<long long> acc((size_t)n * ICP_ROWS * ICP_ROW, 0);
    emu_per_frame(n, [&] { k_icp_set(Tm, trel, n, frames.data()); });
    emu_accumulate(P, frames.data(), emu_maps(maps, lay, W, H), n, stride, 0, plain, acc.data());
    emu_per_frame(n, [&] { k_icp_export(n, acc.data(), out); });
}
void emu_icp_track(const double* K, const float* fp, const double* dp, int min_corr, int n_levels, const int* strides, const int* iterations,
                   const float* const* maps, const int64_t* lay, const double* Tm, const double* T0, const uint8_t* mask, int n, int W,
                   int H, int plain, double* out, aria_icp_result* results, int* err) {
    const IcpParams P = icp_params(K, fp[0], fp[1], fp[2], fp[3], min_corr, dp[0], dp[1]);
    std::vector<IcpFrame> frames((size_t)n);
    std::vector<IcpState> states((size_t)n);
    std::vector<long long> acc((size_t)n * ICP_ROWS * ICP_ROW, 0);
    const IcpMaps m = emu_maps(maps, lay, W, H);
    emu_per_frame(n, [&] { k_icp_prepare(Tm, T0, mask, n, frames.data(), states.data(), err); });
    int total = 0, done = 0;
    for (int l = 0; l < n_levels; l++) total += iterations[l];
    for (int l = 0; l < n_levels; l++)
        for (int it = 0; it < iterations[l]; it++) {
            emu_accumulate(P, frames.data(), m, n, strides[l], l, plain, acc.data());
            const int last = ++done == total ? 1 : 0;
            emu_per_frame(n, [&] { k_icp_solve(P, n, l, last, frames.data(), states.data(), acc.data(), Tm, T0, out, results); });
        }
}
}
