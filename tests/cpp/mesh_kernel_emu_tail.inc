
}  // namespace

// Tail of the host build of the mesh functions (see mesh_kernel_emu_head.inc): the three passes of tsdf_mesh.hip with the
// lanes of every chunk taken in order. What k_mesh_count, k_mesh_scan and k_mesh_emit do across lanes (the prefix inside a
// chunk, the scan over chunks) is plain running sums here; everything per voxel and per cell is the kernel file's own text.
extern "C" {

unsigned long long emu_mesh_table(int p, int mask) { return MESH_TABLE[p][mask]; }

int emu_mesh_block() { return MESH_BLOCK; }

// The scan's totals and comparison over chunk counts, with the kernel's 64-bit carries. totals: two words.
int emu_mesh_scan(const int* vcount, const int* tcount, long long n_chunks, long long vcap, long long tcap, long long* voff, long long* toff,
                  long long* totals) {
    long long vcarry = 0, tcarry = 0;
    for (long long c = 0; c < n_chunks; c++) {
        if (voff) voff[c] = vcarry;
        if (toff) toff[c] = tcarry;
        vcarry += vcount[c];
        tcarry += tcount[c];
    }
    totals[0] = vcarry;
    totals[1] = tcarry;
    return mesh_count_errors(vcarry, tcarry, vcap, tcap);
}

// dims: nx, ny, nz, min_weight; geom: voxel, ox, oy, oz. words: n_vox; the four chunk arrays: n_vox / 256. Returns the
// deferred-error bits.
int emu_mesh_extract(const int* dims, const float* geom, const unsigned long long* vol, uint32_t* words, int* vcount, int* tcount,
                     long long* voff, long long* toff, aria_mesh_vertex* vertices, long long vcap, aria_mesh_triangle* triangles,
                     long long tcap, long long* totals) {
    const MeshGeom G{dims[0], dims[1], dims[2], (uint32_t)dims[3], geom[0], geom[1], geom[2], geom[3]};
    const size_t n_vox = (size_t)G.nx * G.ny * G.nz, n_chunks = n_vox / MESH_BLOCK;
    for (size_t c = 0; c < n_chunks; c++) {
        int prefix = 0, n_tri = 0;
        for (int t = 0; t < MESH_BLOCK; t++) {
            const size_t idx = c * MESH_BLOCK + t;
            const uint32_t word = mesh_voxel(vol, G, idx);
            words[idx] = word | ((uint32_t)prefix << MESH_W_PREFIX);
            prefix += __popc(word & MESH_W_EDGES);
            n_tri += (int)(word >> MESH_W_NTRI);
        }
        vcount[c] = prefix;
        tcount[c] = n_tri;
    }
    const int bits = emu_mesh_scan(vcount, tcount, (long long)n_chunks, vcap, tcap, voff, toff, totals);
    const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
    for (size_t c = 0; c < n_chunks; c++) {
        if (vcount[c] == 0 && tcount[c] == 0) continue;
        long long tpos = toff[c];
        for (int t = 0; t < MESH_BLOCK; t++) {
            const size_t idx = c * MESH_BLOCK + t;
            const uint32_t word = words[idx];
            if ((word & MESH_W_EDGES) != 0 && vcap > 0) {
                const int i = (int)(idx % G.nx), j = (int)(idx / G.nx % G.ny), k = (int)(idx / sz);
                long long pos = voff[c] + (long long)((word >> MESH_W_PREFIX) & MESH_W_PREFIX_MASK);
                for (int d = 1; d < 8; d++) {
                    if (!((word >> (d - 1)) & 1u)) continue;
                    if (pos < vcap) vertices[pos] = mesh_vertex(G, i, j, k, d, vol[idx], vol[idx + (d & 1) + ((d >> 1) & 1) * sy + ((d >> 2) & 1) * sz]);
                    pos++;
                }
            }
            if ((word >> MESH_W_LIVE) & 1u) {
                const int n = mesh_cell_triangles(G, words, voff, idx, (word >> MESH_W_INSIDE) & 0xFFu, triangles, tpos, tcap);
                if (n != (int)(word >> MESH_W_NTRI)) return -1;         // the parked count and the emitted triangles disagree
                tpos += n;
            }
        }
    }
    return bits;
}

}  // extern "C"
