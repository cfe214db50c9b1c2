}  // namespace

// The kernels' loops around the pasted functions, one lane after the other.
extern "C" {

unsigned emu_ilog2_q8(unsigned num, unsigned den) { return bow_ilog2_q8(num, den); }
unsigned emu_idf(unsigned n_frames, unsigned n_w) { return bow_idf(n_frames, n_w); }

// k_bow_majority: ones[256] and the member count of one word -> its 32 bytes (members == 0: untouched)
void emu_majority(const unsigned* ones, unsigned members, uint8_t* word) {
    if (members == 0) return;
    for (int lane = 0; lane < 64; lane++) {
        unsigned nib = 0;
        for (int j = 0; j < 4; j++) nib |= bow_majority_bit(ones[4 * lane + j], members) << j;
        uint8_t& b = word[lane >> 1];
        b = (lane & 1) ? (uint8_t)((b & 0x0F) | (nib << 4)) : (uint8_t)((b & 0xF0) | nib);
    }
}

// k_bow_hist (transform form) and k_bow_store: the norm
long long emu_norm(const uint16_t* tf, const uint16_t* idf, int V) {
    unsigned long long n = 0;
    for (int w = 0; w < V; w++) n += bow_weighted(tf[w], idf[w]);
    return (long long)n;
}

// k_bow_score and the score of k_bow_topk
void emu_score(const uint16_t* tf_q, int n_q, const uint16_t* tf_d, int n_d, const uint16_t* idf, int V, long long* S, double* score) {
    unsigned long long s = 0;
    for (int w = 0; w < V; w++) s += bow_term(bow_weighted(tf_q[w], idf[w]), (unsigned)n_d, bow_weighted(tf_d[w], idf[w]), (unsigned)n_q);
    *S = (long long)s;
    *score = bow_score((long long)s, n_q, n_d);
}

// the rounds of k_bow_topk over score bit patterns (0 = gated): out[k] = the index of hit k or -1; returns the count
int emu_topk(const unsigned long long* bits, int size, int K, int* out) {
    unsigned long long prev_bits = ~0ull;
    int prev_idx = -1, found = 0;
    for (int k = 0; k < K; k++) {
        unsigned long long best_bits = 0;
        int best_idx = INT_MAX;
        for (int e = size - 1; e >= 0; e--) {                     // any order of the entries gives the same winner
            const unsigned long long b = bits[e];
            if (b && bow_hit_before(prev_bits, prev_idx, b, e) && bow_hit_before(b, e, best_bits, best_idx)) {
                best_bits = b;
                best_idx = e;
            }
        }
        out[k] = best_bits ? best_idx : -1;
        prev_bits = best_bits;
        prev_idx = best_idx;
        if (best_bits) found++;
    }
    return found;
}

}  // extern "C"
