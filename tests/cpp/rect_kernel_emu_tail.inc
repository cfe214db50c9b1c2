// Drivers of the emulated kernels (see rect_kernel_emu_head.inc): the launch geometry of rectify.hip's aria_rect_create,
// aria_rect_remap_batch_device and aria_rect_points_batch_device.
static RectCam emu_cam(const double* p) {   // fx fy cx cy, dist[5], R[9], new K[4]
    RectCam c{};
    c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3];
    c.k1 = p[4]; c.k2 = p[5]; c.p1 = p[6]; c.p2 = p[7]; c.k3 = p[8];
    for (int i = 0; i < 9; i++) c.R[i] = p[9 + i];
    c.nfx = p[18]; c.nfy = p[19]; c.ncx = p[20]; c.ncy = p[21];
    return c;
}
extern "C" {
int emu_map_pitch(int dst_w) { return (dst_w + 3) & ~3; }
int emu_group() { return RECT_GROUP; }
// map: emu_map_pitch(dst_w) * dst_h words, 16-byte aligned
void emu_build_map(const double* cam, int src_w, int src_h, int dst_w, int dst_h, uint32_t* map) {
    const RectCam c = emu_cam(cam);
    const int pitch = emu_map_pitch(dst_w);
    const int64_t words = (int64_t)pitch * dst_h;
    for (int64_t b = 0; b < (words + RECT_BLOCK - 1) / RECT_BLOCK; b++)
        for (int t = 0; t < RECT_BLOCK; t++) {
            blockIdx.x = (int)b; threadIdx.x = t;
            k_rect_build_map(c, src_w, src_h, dst_w, dst_h, pitch, map);
        }
}
void emu_remap(const uint32_t* map, int dst_w, int dst_h, const uint8_t* src, int64_t src_stride, int src_pitch, int src_w, int src_h,
               int rows_ok, int n_frames, int group, uint8_t* dst, int64_t dst_stride, int dst_pitch, int fill) {
    const int pitch = emu_map_pitch(dst_w);
    const int gx = (dst_w + RECT_TILE_W - 1) / RECT_TILE_W, gy = (dst_h + RECT_TILE_H - 1) / RECT_TILE_H;
    const int gz = (n_frames + group - 1) / group;
    g_src = src; g_src_stride = src_stride; g_src_pitch = src_pitch; g_src_w = src_w; g_src_h = src_h; g_src_frames = n_frames;
    for (int z = 0; z < gz; z++) for (int y = 0; y < gy; y++) for (int x = 0; x < gx; x++) for (int t = 0; t < RECT_BLOCK; t++) {
        blockIdx.x = x; blockIdx.y = y; blockIdx.z = z; threadIdx.x = t;
        k_rect_remap(map, pitch, dst_w, dst_h, src, src_stride, src_pitch, src_w, src_h, rows_ok, n_frames, group, dst, dst_stride, dst_pitch,
                     (uint32_t)fill);
    }
    g_src = nullptr;
}
// loads of emu_remap calls that left the source images since the last call of this function
long emu_bad_loads() { const long n = g_bad_loads; g_bad_loads = 0; return n; }
void emu_points(const double* cam, const void* kp_in, const int* counts, int64_t kp_stride, int n_frames, void* kp_out, int* err) {
    const RectCam c = emu_cam(cam);
    for (int f = 0; f < n_frames; f++) for (int64_t b = 0; b < (kp_stride + RECT_BLOCK - 1) / RECT_BLOCK; b++)
        for (int t = 0; t < RECT_BLOCK; t++) {
            blockIdx.x = (int)b; blockIdx.y = f; threadIdx.x = t;
            k_rect_points(c, (const RectKp*)kp_in, counts, kp_stride, (RectKp*)kp_out, err);
        }
}
}
