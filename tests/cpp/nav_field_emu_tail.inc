// The relaxation schedule of k_nav_field under the shim of nav_kernel_emu_head.inc: nav_relax is the library's text; the loop
// below restates the kernel's rounds with the lanes of a phase one after the other, which is one of the interleavings the
// kernel allows (rule 6's least solution does not depend on which). lds: the pitch of nu + 1 words; plain: the all-cell sweep.
// Returns the rounds, negative when the bound was reached.
#include <vector>
extern "C" int emu_field(int nu, int nv, const uint32_t* cm, int gu, int gv, int32_t* D, int lds, int plain, int max_rounds) {
    const int n = nu * nv, pitch = lds ? nu + 1 : nu;
    std::vector<uint32_t> buf((size_t)pitch * nv);
    volatile uint32_t* E = lds ? buf.data() : reinterpret_cast<uint32_t*>(D);
    const bool goal_in = gu >= 0 && gu < nu && gv >= 0 && gv < nv;
    if (!goal_in || (cm[gv * nu + gu] & 0xFFFFu) == NAV_BLOCKED) {
        for (int c = 0; c < n; c++) D[c] = (int32_t)NAV_INF;
        return 0;
    }
    for (int c = 0; c < n; c++) E[(c / nu) * pitch + c % nu] = NAV_INF;
    E[gv * pitch + gu] = cm[gv * nu + gu] & 0xFFFFu;
    int r = 0;
    bool settled = false;
    while (r < max_rounds && !settled) {
        bool changed = false;
        if (plain) {
            for (int t = 0; t < NAV_BLOCK; t++)
                for (int c = t; c < n; c += NAV_BLOCK) changed |= nav_relax(E, cm, c, (c / nu) * pitch + c % nu, pitch);
        } else {
            for (int t = 0; t < NAV_BLOCK; t++)
                for (int v = t; v < nv; v += NAV_BLOCK) {
                    for (int u = 0; u < nu; u++) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                    for (int u = nu - 2; u >= 0; u--) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                }
            for (int t = 0; t < NAV_BLOCK; t++)
                for (int u = t; u < nu; u += NAV_BLOCK) {
                    for (int v = 0; v < nv; v++) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                    for (int v = nv - 2; v >= 0; v--) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                }
        }
        r++;
        settled = !changed;
    }
    for (int c = 0; c < n; c++) {
        const uint32_t e = E[(c / nu) * pitch + c % nu];
        D[c] = e >= NAV_INF ? (int32_t)NAV_INF : (int32_t)(e - (cm[c] & 0xFFFFu));
    }
    return settled ? r : -r;
}
