}  // namespace
// Drivers of the emulated kernels (see ray_kernel_emu_head.inc): the launch geometry of tsdf_raycast.hip's
// aria_ray_update_from_volume_device and aria_ray_cast_batch_device. The parameters come from the library's own ray_params, in
// the pasted text.
#include <vector>
extern "C" {
// ip: nx ny nz min_weight skip; fp: voxel ox oy oz near far step; K: fx fy cx cy. Returns n_steps.
int emu_ray_steps(const int* ip, const float* fp, const double* K) { return ray_params(ip, ip[3], ip[4], fp[0], fp + 1, fp[4], fp[5], fp[6], K).n_steps; }
int emu_ray_words(const int* ip) { return (ip[0] / 8 * (ip[1] / 8) * (ip[2] / 8) + 31) / 32; }
void emu_ray_bricks(const int* ip, const float* fp, const double* K, const unsigned long long* vol, uint32_t* words) {
    const RayParams P = ray_params(ip, ip[3], ip[4], fp[0], fp + 1, fp[4], fp[5], fp[6], K);
    const int n_bricks = P.nx / 8 * (P.ny / 8) * (P.nz / 8), n_runs = P.nx / 8 * P.ny * P.nz;
    std::vector<uint8_t> flags((size_t)n_bricks, 0);
    blockIdx = dim3e();
    for (int b = 0; b < (n_runs + RAY_BLOCK - 1) / RAY_BLOCK; b++)
        for (int t = 0; t < RAY_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            k_ray_bricks(P, vol, flags.data());
        }
    for (int b = 0; b < (emu_ray_words(ip) + RAY_BLOCK - 1) / RAY_BLOCK; b++)
        for (int t = 0; t < RAY_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            k_ray_brick_words(n_bricks, flags.data(), words);
        }
}
void emu_ray_cast(const int* ip, const float* fp, const double* K, const unsigned long long* vol, const uint32_t* words, const double* ext,
                  const uint8_t* mask, int n_views, int W, int H, float* depth, int64_t depth_stride, int depth_pitch, float* normal,
                  int64_t normal_stride, int normal_pitch, uint8_t* gray, int64_t gray_stride, int gray_pitch, uint8_t* shade,
                  int64_t shade_stride, int shade_pitch, aria_ray_view* recs, int* err) {
    const RayParams P = ray_params(ip, ip[3], ip[4], fp[0], fp + 1, fp[4], fp[5], fp[6], K);
    std::vector<RayView> views((size_t)std::max(n_views, 1));
    blockIdx = dim3e();
    for (int b = 0; b < (n_views + RAY_BLOCK - 1) / RAY_BLOCK; b++)
        for (int t = 0; t < RAY_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            k_ray_prepare(P, ext, mask, n_views, views.data(), recs, err);
        }
    for (int f = 0; f < n_views; f++)
        for (int y = 0; y < (H + RAY_TILE - 1) / RAY_TILE; y++) for (int x = 0; x < (W + RAY_TILE - 1) / RAY_TILE; x++)
            for (int t = 0; t < RAY_BLOCK; t++) {
                blockIdx.x = x; blockIdx.y = y; blockIdx.z = f; threadIdx.x = t;
                k_ray_march(P, views.data(), vol, words, W, H, depth, depth_stride, depth_pitch, normal, normal_stride, normal_pitch, gray,
                            gray_stride, gray_pitch, shade, shade_stride, shade_pitch, recs);
            }
    if (recs) {
        blockIdx = dim3e();
        for (int b = 0; b < (n_views + RAY_BLOCK - 1) / RAY_BLOCK; b++)
            for (int t = 0; t < RAY_BLOCK; t++) {
                blockIdx.x = b; threadIdx.x = t;
                k_ray_finish(views.data(), n_views, recs);
            }
    }
}
}
