// Drivers of the emulated kernels (see det_kernel_emu_head.inc): the launch geometry of detect_stage.hip's det_launch_pre and
// aria_det_postprocess_batch_device, with the tables built by the file's own det_build_table.
extern "C" {
void emu_table(int src, int dst, uint32_t* out) { det_build_table(src, dst, out); }
void emu_pre(const uint8_t* img, int n_frames, int W, int H, int row_stride, int64_t frame_stride, int C, int swap_rb, int in_w, int in_h,
             int half, void* out) {
    std::vector<uint32_t> xt(in_w), yt(in_h);
    det_build_table(W, in_w, xt.data()); det_build_table(H, in_h, yt.data());
    const int lanes = ((in_w + 3) / 4) * in_h, gx = (lanes + DET_BLOCK - 1) / DET_BLOCK;
    for (int f = 0; f < n_frames; f++) for (int bx = 0; bx < gx; bx++) for (int t = 0; t < DET_BLOCK; t++) {
        blockIdx.x = bx; blockIdx.y = f; threadIdx.x = t;
        if (half) { if (C == 1) k_det_preprocess<__half, 1>(img, W, H, row_stride, frame_stride, swap_rb, xt.data(), yt.data(), in_w, in_h, (__half*)out);
                    else k_det_preprocess<__half, 3>(img, W, H, row_stride, frame_stride, swap_rb, xt.data(), yt.data(), in_w, in_h, (__half*)out); }
        else { if (C == 1) k_det_preprocess<float, 1>(img, W, H, row_stride, frame_stride, swap_rb, xt.data(), yt.data(), in_w, in_h, (float*)out);
               else k_det_preprocess<float, 3>(img, W, H, row_stride, frame_stride, swap_rb, xt.data(), yt.data(), in_w, in_h, (float*)out); }
    }
}
void emu_post(const float* raw, int n_frames, int n_cand, float sx, float sy, float conf, float nms, const int* ids, int n_ids,
              aria_detection* dets, int* ndets, int det_cap, aria_box* boxes, int* nboxes, int box_cap, int* err) {
    DetClasses cls{}; cls.n = n_ids; for (int k = 0; k < n_ids; k++) cls.ids[k] = ids[k];
    for (int f = 0; f < n_frames; f++) {
        std::barrier<> bar(DET_BLOCK); g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < DET_BLOCK; t++) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = f;
            k_det_postprocess(raw, n_cand, sx, sy, conf, nms, cls, dets, ndets, det_cap, boxes, nboxes, box_cap, err); });
        for (auto& x : th) x.join();
    }
}
}
