
// ---- tail: the parameters, and the kernels' use of the rule functions with the lanes of a wave one after the other -----------
static AlertParams emu_params(const int* ip, const float* fp, const long long* lp) {
    AlertParams P;
    std::memset(&P, 0, sizeof(P));
    P.width = ip[0]; P.height = ip[1]; P.zone_top = ip[2]; P.zone_bottom = ip[3]; P.bound0 = ip[4]; P.bound1 = ip[5];
    P.max_dets = ip[6]; P.min_valid = ip[7]; P.zone_num = ip[8]; P.zone_den = ip[9]; P.det_num = ip[10]; P.det_den = ip[11];
    P.obstacle_dangerous = ip[12]; P.n_dangerous = ip[13]; P.max_events = ip[14];
    for (int i = 0; i < 32; i++) P.dangerous[i] = ip[15 + i];
    P.min_depth = fp[0]; P.max_depth = fp[1]; P.zone_alert_m = fp[2]; P.default_depth = fp[3]; P.crit_m = fp[4]; P.high_m = fp[5];
    P.medium_m = fp[6]; P.beep_m = fp[7];
    for (int i = 0; i < 4; i++) P.cooldown_ns[i] = lp[i];
    return P;
}

extern "C" {

int emu_column_zone(int x, int width) { return alert_column_zone(x, width); }

long long emu_rank(long long n, int num, int den) { return alert_rank(n, num, den); }

int emu_valid(const int* ip, const float* fp, const long long* lp, float d) { return alert_valid_depth(emu_params(ip, fp, lp), d) ? 1 : 0; }

// rule 1 of one frame as k_alert_measure's setup applies it: rects[64][4], used[64] (0 no source, 1 source, 2 source with an empty
// rectangle); returns the error bits, *seen as the kernel's second word
int emu_sources(const int* ip, const float* fp, const long long* lp, const aria_detection* dets, int count, int det_cap, int* rects, int* used,
                int* seen) {
    const AlertParams P = emu_params(ip, fp, lp);
    bool bad = false;
    int err = 0;
    const int n_det = dets ? alert_det_count(count, det_cap, P.max_dets, &bad) : 0;
    if (bad) err |= ERRBIT_ALERT_INPUT;
    else if (dets && count > P.max_dets && count > *seen) *seen = count;
    for (int s = 0; s < ALERT_SOURCES; s++) {
        used[s] = 0;
        rects[4 * s] = rects[4 * s + 1] = rects[4 * s + 2] = rects[4 * s + 3] = 0;
        if (s >= 3 + n_det) continue;
        aria_detection d;
        std::memset(&d, 0, sizeof(d));
        if (s >= 3) d = dets[s - 3];
        const AlertRect r = alert_source_rect(P, s, d);
        used[s] = alert_rect_empty(r) ? 2 : 1;
        rects[4 * s] = r.x0; rects[4 * s + 1] = r.y0; rects[4 * s + 2] = r.x1; rects[4 * s + 3] = r.y1;
    }
    return err;
}

// k_alert_arbitrate, one track after the other and the 64 lanes of its wave one after the other
int emu_arbitrate(const int* ip, const float* fp, const long long* lp, const int* track_offset, int n_tracks, const long long* timestamps,
                  int n_frames, const aria_alert_meas* meas, const aria_detection* dets, const int* ndets, int det_cap, aria_alert_state* states,
                  aria_alert_event* events, int event_cap, int* nevents) {
    const AlertParams P = emu_params(ip, fp, lp);
    int err = 0;
    for (int track = 0; track < n_tracks; track++) {
        const int f0 = track_offset[track], f1 = track_offset[track + 1];
        if (f0 < 0 || f1 < f0 || f1 > n_frames) { nevents[track] = 0; err |= ERRBIT_ALERT_INPUT; continue; }
        aria_alert_state* st = states + track;
        long long total = 0, prev = 0;
        bool have_prev = false;
        for (int f = f0; f < f1; f++) {
            const long long ts = timestamps[f];
            if (have_prev && ts < prev) { err |= ERRBIT_ALERT_INPUT; continue; }
            prev = ts; have_prev = true;
            int n_det = 0;
            if (ndets) {
                bool bad;
                n_det = alert_det_count(ndets[f], det_cap, P.max_dets, &bad);
                if (bad) err |= ERRBIT_ALERT_INPUT;
            }
            AlertCand c[ALERT_SOURCES];
            int rank[ALERT_SOURCES], n_cand = 0;
            for (int lane = 0; lane < ALERT_SOURCES; lane++) {
                const bool is_source = lane < 3 + n_det;
                aria_detection d;
                std::memset(&d, 0, sizeof(d));
                if (is_source && lane >= 3) d = dets[(size_t)f * det_cap + (lane - 3)];
                c[lane] = alert_classify(P, lane, is_source, meas[(size_t)f * ALERT_SOURCES + lane], d);
                n_cand += c[lane].cand;
            }
            for (int lane = 0; lane < ALERT_SOURCES; lane++) {
                rank[lane] = 0;
                for (int j = 0; j < ALERT_SOURCES; j++)
                    if (c[j].cand && alert_precedes(c[j].priority, c[j].distance, c[j].direction, j, c[lane].priority, c[lane].distance,
                                                    c[lane].direction, lane))
                        rank[lane]++;
            }
            int announced = 0;
            for (int r = 0; r < n_cand && announced < P.max_events; r++) {
                int src = -1, hits = 0;
                for (int lane = 0; lane < ALERT_SOURCES; lane++)
                    if (c[lane].cand && rank[lane] == r) { if (src < 0) src = lane; hits++; }
                if (hits != 1) return -100 - r;                          // rule 4 is not a strict total order
                const int key = alert_key(c[src].class_id, c[src].direction), prio = c[src].priority;
                if (!alert_may_announce(st->last_prio1[key], st->last_ns[key], prio, ts, P.cooldown_ns[prio])) continue;
                st->last_prio1[key] = (uint8_t)(prio + 1);
                st->last_ns[key] = ts;
                if (total < (long long)event_cap) {
                    aria_alert_event e;
                    e.frame = f; e.source = src; e.class_id = c[src].class_id; e.direction = c[src].direction; e.priority = prio;
                    e.distance = c[src].distance; e.flags = c[src].flags; e.reserved = 0;
                    events[(size_t)track * event_cap + (size_t)total] = e;
                }
                total++;
                announced++;
            }
        }
        st->events_total += total;
        nevents[track] = (int)total;
        if (total > (long long)event_cap) err |= ERRBIT_ALERT_CAP;
    }
    return err;
}

}  // extern "C"
