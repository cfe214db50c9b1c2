}  // namespace
// Drivers of the emulated kernels (see tsdf_kernel_emu_head.inc): the launch geometry of tsdf_volume.hip's
// aria_tsdf_integrate_batch_device. The parameters come from the library's own tsdf_params / tsdf_with_image, in the pasted text.
#include <vector>
extern "C" {
int emu_frame_bytes() { return (int)sizeof(TsdfFrame); }
// ip: nx ny nz max_weight W H; fp: voxel ox oy oz trunc min_depth max_depth; K: fx fy cx cy
void emu_integrate(const int* ip, const float* fp, const double* K, const double* ext, const uint8_t* mask, int n_frames,
                   const float* depth, int64_t depth_stride, int depth_pitch, const uint8_t* img, int64_t img_stride, int img_pitch,
                   int cull, int group, unsigned long long* vol, void* frames, int* err) {
    const TsdfParams P = tsdf_with_image(tsdf_params(ip, ip[3], fp[0], fp + 1, fp[4], fp[5], fp[6], K), ip[4], ip[5]);
    TsdfFrame* F = (TsdfFrame*)frames;
    blockIdx = dim3e();
    for (int b = 0; b < (n_frames + TSDF_BLOCK - 1) / TSDF_BLOCK; b++)
        for (int t = 0; t < TSDF_BLOCK; t++) {
            blockIdx.x = b; threadIdx.x = t;
            k_tsdf_prepare(P, ext, mask, n_frames, F, err);
        }
    // the frames in groups of `group` (a multiple of 32, or all of them), as the library cuts a call whose tile words do not fit
    const int tiles = (P.nx / TSDF_TILE_X) * (P.ny / TSDF_TILE_Y) * (P.nz / TSDF_TILE_Z);
    if (group <= 0 || group > n_frames) group = n_frames;
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int n = std::min(group, n_frames - f0), words = (n + 31) / 32;
        std::vector<uint32_t> tile_words((size_t)tiles * words, 0xFFFFFFFFu);
        blockIdx = dim3e();
        for (int w = 0; w < words; w++) for (int b = 0; b < (tiles + TSDF_BLOCK - 1) / TSDF_BLOCK; b++) for (int t = 0; t < TSDF_BLOCK; t++) {
            blockIdx.x = b; blockIdx.y = w; threadIdx.x = t;
            k_tsdf_cull(P, F + f0, n, words, cull, tile_words.data());
        }
        for (int z = 0; z < P.nz / TSDF_TILE_Z; z++) for (int y = 0; y < P.ny / TSDF_TILE_Y; y++) for (int x = 0; x < P.nx / TSDF_TILE_X; x++)
            for (int t = 0; t < TSDF_BLOCK; t++) {
                blockIdx.x = x; blockIdx.y = y; blockIdx.z = z; threadIdx.x = t;
                k_tsdf_integrate(P, F + f0, words, tile_words.data(), depth + f0 * depth_stride, depth_stride, depth_pitch,
                                 img ? img + f0 * img_stride : nullptr, img_stride, img_pitch, vol);
            }
    }
}
}
