// Drivers of the emulated fisheye (KB4) kernels; follows rect_kernel_emu_tail.inc (emu_cam, emu_map_pitch, emu_remap) in the
// build of tests/test_fisheye_kernel_emulation.py. The launch geometry is that of rectify.hip's aria_rect_create and
// aria_rect_points_batch_device; the camera's dist[0..3] are k1..k4.
extern "C" {
void emu_build_map_kb4(const double* cam, int src_w, int src_h, int dst_w, int dst_h, uint32_t* map) {
    const RectCam c = emu_cam(cam);
    const int pitch = emu_map_pitch(dst_w);
    const int64_t words = (int64_t)pitch * dst_h;
    for (int64_t b = 0; b < (words + RECT_BLOCK - 1) / RECT_BLOCK; b++)
        for (int t = 0; t < RECT_BLOCK; t++) {
            blockIdx.x = (int)b; threadIdx.x = t;
            k_rect_build_map_kb4(c, src_w, src_h, dst_w, dst_h, pitch, map);
        }
}
void emu_points_kb4(const double* cam, const void* kp_in, const int* counts, int64_t kp_stride, int n_frames, void* kp_out, int* err) {
    const RectCam c = emu_cam(cam);
    for (int f = 0; f < n_frames; f++) for (int64_t b = 0; b < (kp_stride + RECT_BLOCK - 1) / RECT_BLOCK; b++)
        for (int t = 0; t < RECT_BLOCK; t++) {
            blockIdx.x = (int)b; blockIdx.y = f; threadIdx.x = t;
            k_rect_points_kb4(c, (const RectKp*)kp_in, counts, kp_stride, (RectKp*)kp_out, err);
        }
}
}
