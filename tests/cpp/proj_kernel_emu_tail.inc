// Tail of the host build of proj_search.hip's plain text (tests/test_proj_kernel_emulation.py): the search of one valid frame
// restated around the pasted functions -- every keypoint offered to proj_candidate in ascending AND in descending order (the
// running top-2 may depend on neither), the claims by the minimum of proj_claim_key -- then the pasted k_proj_resolve and
// k_proj_from_map under the launch geometry of the library. Test infrastructure only.
static ProjParams make_params(const double* K, double min_depth, float radius, float ratio, int th, int mod, const float* scale) {
    ProjParams p{};
    p.fx = K[0]; p.fy = K[1]; p.cx = K[2]; p.cy = K[3]; p.min_depth = min_depth;
    p.radius = radius; p.ratio = ratio; p.th = th; p.mod = mod;
    for (int l = 0; l < 8; l++) p.scale[l] = scale[l];
    return p;
}

extern "C" {

// Returns the number of candidates that lie outside the cell range the kernel would walk (must be 0), or -1 when the two
// offer orders disagree.
int emu_search(const double* pose, const aria_keypoint* kp, const uint8_t* desc, int n, int64_t kp_stride, int width, int height,
               const aria_proj_landmark* land, int first, int count, int land_cap, const double* K, double min_depth, float radius,
               float ratio, int th, int mod, const float* scale, aria_proj_obs* obs, int* claims) {
    const ProjParams prm = make_params(K, min_depth, radius, ratio, th, mod, scale);
    const int gx = (width + 31) >> PJ_CELL_LOG2, gy = (height + 31) >> PJ_CELL_LOG2;
    int outside = 0;
    for (int k = 0; k < n; k++) claims[k] = PJ_NONE;
    for (int i = 0; i < land_cap; i++) obs[i] = proj_not_visible();
    for (int i = 0; i < count; i++) {
        const aria_proj_landmark& lm = land[first + i];
        const ProjView pv = proj_project(pose, lm.X, lm.octave, prm, width, height);
        if (!pv.visible) continue;
        const int oi = proj_clamp_octave(lm.octave);
        const float r = prm.radius * proj_level_scale(prm, oi);
        uint64_t a[4];
        std::memcpy(a, lm.desc, 32);
        const int cx0 = proj_cell(pv.u - r - 1.0f, gx), cx1 = proj_cell(pv.u + r + 1.0f, gx);
        const int cy0 = proj_cell(pv.v - r - 1.0f, gy), cy1 = proj_cell(pv.v + r + 1.0f, gy);
        int m1 = PJ_NONE, m2 = PJ_NONE, r1 = PJ_NONE, r2 = PJ_NONE;
        for (int pass = 0; pass < 2; pass++)
            for (int j = 0; j < n; j++) {
                const int k = pass ? n - 1 - j : j;
                if (!proj_candidate(pv.u, pv.v, r, oi, kp[k].x, kp[k].y, kp[k].octave, prm.mod)) continue;
                uint64_t b[4];
                std::memcpy(b, desc + (int64_t)k * 32, 32);
                const int key = (proj_hamming(a, b) << PJ_KSHIFT) | k;
                if (pass) proj_top2(key, r1, r2);
                else {
                    proj_top2(key, m1, m2);
                    const int cx = proj_cell(kp[k].x, gx), cy = proj_cell(kp[k].y, gy);
                    outside += cx < cx0 || cx > cx1 || cy < cy0 || cy > cy1;
                }
            }
        if (m1 != r1 || m2 != r2) return -1;
        // the merge of two disjoint halves must give the same two keys
        {
            int a1 = PJ_NONE, a2 = PJ_NONE, b1 = PJ_NONE, b2 = PJ_NONE;
            for (int k = 0; k < n; k++) {
                if (!proj_candidate(pv.u, pv.v, r, oi, kp[k].x, kp[k].y, kp[k].octave, prm.mod)) continue;
                uint64_t b[4];
                std::memcpy(b, desc + (int64_t)k * 32, 32);
                const int key = (proj_hamming(a, b) << PJ_KSHIFT) | k;
                if (k & 1) proj_top2(key, a1, a2);
                else proj_top2(key, b1, b2);
            }
            proj_top2_merge(a1, a2, b1, b2);
            if (b1 != m1 || b2 != m2) return -1;
        }
        const aria_proj_obs o = proj_decide(pv.u, pv.v, m1, m2, prm);
        obs[i] = o;
        if (o.flags & 4) claims[o.kp_idx] = min(claims[o.kp_idx], proj_claim_key(o.hamming, i));
    }
    const int range[2] = {first, count}, ok = 1;
    blockDim.x = PJ_BLOCK;
    for (blockIdx.x = 0; blockIdx.x < (unsigned)((land_cap + PJ_BLOCK - 1) / PJ_BLOCK); blockIdx.x++)
        for (threadIdx.x = 0; threadIdx.x < PJ_BLOCK; threadIdx.x++) k_proj_resolve(range, land_cap, &ok, claims, kp_stride, obs);
    return outside;
}

void emu_from_map(const aria_map_point* arena, long long size, long long capacity, long long first, long long max_count, int pair_base,
                  int view, const aria_keypoint* kp, const uint8_t* desc, const int* n_kp, int64_t kp_stride, int n_slots,
                  aria_proj_landmark* land, int* nland, int* err) {
    blockDim.x = PJ_BLOCK;
    const unsigned blocks = (unsigned)std::max<long long>((max_count + PJ_BLOCK - 1) / PJ_BLOCK, 1);
    for (blockIdx.x = 0; blockIdx.x < blocks; blockIdx.x++)
        for (threadIdx.x = 0; threadIdx.x < PJ_BLOCK; threadIdx.x++)
            k_proj_from_map(arena, &size, capacity, first, max_count, pair_base, view, kp, desc, n_kp, kp_stride, n_slots, land, nland, err);
}

int emu_is_finite(double v) { return proj_is_finite(v) ? 1 : 0; }

}  // extern "C"
