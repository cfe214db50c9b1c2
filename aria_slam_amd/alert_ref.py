"""Obstacle alerts, restated in NumPy: the DEFINITION of what aria_alert_* computes (include/aria_orb_hip.h, "obstacle
alerts"). The reference has the port IAudioFeedback (include/interfaces/IAudioFeedback.hpp:7-78) and a sketch of the
caller, NavigationAudioEngine (docs/milestones/H16_AUDIO_FEEDBACK.md:393-493), with no depth source and no canAnnounce;
the rules below restate the sketch wherever it has them and the device equals this file bit for bit.

The order statistic is np.sort's, not a radix selection, and the arbitration is plain loops, so that this file and the
kernels do not share a mistake. fp32 arithmetic is spelled with np.float32 operands, one rounding per operation. The
defaults for band, percentiles and zone_alert_m are assumptions nobody has tuned on a recording."""
from collections import namedtuple

import numpy as np

MEAS_DTYPE = np.dtype([("distance", "<f4"), ("n_valid", "<i4"), ("k", "<i4"), ("flags", "<i4")])
EVENT_DTYPE = np.dtype([("frame", "<i4"), ("source", "<i4"), ("class_id", "<i4"), ("direction", "<i4"), ("priority", "<i4"),
                        ("distance", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
STATE_DTYPE = np.dtype([("last_ns", "<i8", (256,)), ("last_prio1", "u1", (256,)), ("events_total", "<i8"), ("reserved", "<i8")])
DETECTION_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"), ("class_id", "<i4")])

SOURCES, MAX_DETS = 64, 61
LOW, MEDIUM, HIGH, CRITICAL = 0, 1, 2, 3                 # AudioPriority
CENTER, LEFT, RIGHT = 0, 1, 2                            # AudioDirection; BEHIND (3) is never produced
BEEP, CRITICAL_ALERT, INTERRUPT, NO_DEPTH = 1, 2, 4, 8
MEAS_SOURCE, MEAS_OK = 1, 2
OK, E_INVALID, E_OUTPUT_TOO_SMALL = 0, -1, -5

F = np.float32

Config = namedtuple("Config", "width height zone_top zone_bottom max_dets min_valid min_depth max_depth zone_pct det_pct "
                              "zone_alert_m default_depth crit_m high_m medium_m beep_m obstacle_dangerous dangerous "
                              "max_events_per_frame cooldown_ns")


def config(**kw):
    d = dict(width=752, height=480, zone_top=120, zone_bottom=480, max_dets=32, min_valid=16, min_depth=0.1, max_depth=20.0,
             zone_pct=(5, 100), det_pct=(1, 2), zone_alert_m=3.0, default_depth=5.0, crit_m=1.0, high_m=2.0, medium_m=3.0, beep_m=1.5,
             obstacle_dangerous=1, dangerous=(0, 1, 2, 3, 5, 7), max_events_per_frame=2,
             cooldown_ns=(2000_000_000, 800_000_000, 500_000_000, 0))
    d.update(kw)
    for name in ("min_depth", "max_depth", "zone_alert_m", "default_depth", "crit_m", "high_m", "medium_m", "beep_m"):
        d[name] = F(d[name])
    d["dangerous"] = tuple(int(c) for c in d["dangerous"])
    d["cooldown_ns"] = tuple(int(c) for c in d["cooldown_ns"])
    return Config(**d)


def valid_config(c):
    """What aria_alert_create accepts."""
    ok = 1 <= c.width <= 8192 and 1 <= c.height <= 8192 and 0 <= c.zone_top < c.zone_bottom <= c.height
    ok = ok and 0 <= c.max_dets <= MAX_DETS and c.min_valid >= 1
    ok = ok and np.isfinite(c.min_depth) and np.isfinite(c.max_depth) and 0 < c.min_depth <= c.max_depth
    ok = ok and all(0 <= n < d for n, d in (c.zone_pct, c.det_pct))
    ok = ok and all(np.isfinite(v) for v in (c.zone_alert_m, c.default_depth, c.crit_m, c.high_m, c.medium_m, c.beep_m))
    ok = ok and len(c.dangerous) <= 32 and 0 <= c.max_events_per_frame <= SOURCES and all(v >= 0 for v in c.cooldown_ns)
    return bool(ok)


# ---- rule 1 ------------------------------------------------------------------------------------------------------------
def direction(nrm):
    """0.35f / 0.65f, as the compares fall (H16:463-468); a NaN is CENTER."""
    nrm = F(nrm)
    return LEFT if nrm < F(0.35) else RIGHT if nrm > F(0.65) else CENTER


def column_zone(x, width):
    return direction((F(x) + F(0.5)) / F(width))


def zone_bounds(width):
    """(first CENTER column, first RIGHT column), by the per-column test."""
    zones = [column_zone(x, width) for x in range(width)]
    b0 = next((x for x, z in enumerate(zones) if z != LEFT), width)
    b1 = next((x for x, z in enumerate(zones) if z == RIGHT), width)
    return b0, b1


def det_count(count, det_cap, max_dets):
    """(detections that are sources, the count was bad)."""
    if count < 0 or count > det_cap:
        return 0, True
    return min(int(count), max_dets), False


def source_rect(c, source, det=None):
    """(x0, y0, x1, y1): columns [x0, x1), rows [y0, y1)."""
    if source < 3:
        b0, b1 = zone_bounds(c.width)
        x0, x1 = ((b0, b1), (0, b0), (b1, c.width))[source]
        return x0, c.zone_top, x1, c.zone_bottom
    corners = [F(det[n]) for n in ("x1", "y1", "x2", "y2")]
    if not all(np.isfinite(v) and abs(float(v)) <= 2.0 ** 20 for v in corners):
        return 0, 0, 0, 0
    ax, ay, bx, by = (int(np.trunc(v)) for v in corners)
    return max(0, ax), max(0, ay), min(c.width, bx), min(c.height, by)


# ---- rule 2 ------------------------------------------------------------------------------------------------------------
def order_statistic(values, c, pct):
    """values: the fp32 depths of a rectangle, any shape. Returns the aria_alert_meas of a source."""
    v = np.asarray(values, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = v[(v >= c.min_depth) & (v <= c.max_depth)]
    n = int(v.size)
    if n < c.min_valid:
        return F(-1.0), n, 0, MEAS_SOURCE
    k = (n * int(pct[0])) // int(pct[1])
    return np.sort(v)[k], n, k, MEAS_SOURCE | MEAS_OK


def measure(depth, c, dets=None, ndets=None):
    """depth [F, H, >= W] fp32 (columns beyond W are padding). dets [F, det_cap] DETECTION_DTYPE and ndets [F], or None.
    Returns (meas [F, 64], status, dets_seen)."""
    depth = np.asarray(depth, np.float32)
    n_frames = depth.shape[0]
    meas = np.zeros((n_frames, SOURCES), MEAS_DTYPE)
    meas["distance"] = F(-1.0)
    status, seen = OK, 0
    for f in range(n_frames):
        n_det = 0
        if ndets is not None:
            n_det, bad = det_count(int(ndets[f]), dets.shape[1], c.max_dets)
            if bad:
                status = E_INVALID
            elif ndets[f] > c.max_dets:
                seen = max(seen, int(ndets[f]))
        for s in range(3 + n_det):
            x0, y0, x1, y1 = source_rect(c, s, dets[f, s - 3] if s >= 3 else None)
            if x0 >= x1 or y0 >= y1:
                meas[f, s] = (F(-1.0), 0, 0, MEAS_SOURCE)
            else:
                meas[f, s] = order_statistic(depth[f, y0:y1, x0:x1], c, c.zone_pct if s < 3 else c.det_pct)
    return meas, status, seen


# ---- rules 3-6 ---------------------------------------------------------------------------------------------------------
def dangerous(c, class_id):
    return bool(c.obstacle_dangerous) if class_id == -1 else class_id in c.dangerous


def priority(c, class_id, distance):
    """H16:470-478."""
    distance = F(distance)
    if distance < c.crit_m:
        return CRITICAL
    if distance < c.high_m and dangerous(c, class_id):
        return HIGH
    if distance < c.medium_m:
        return MEDIUM
    return LOW


def classify(c, source, m, det=None):
    """Rule 3 for a source: None, or (class_id, direction, priority, distance, flags)."""
    measured = bool(m["flags"] & MEAS_OK)
    flags = 0
    if source < 3:
        if not measured or not (F(m["distance"]) < c.zone_alert_m):
            return None
        class_id, direc, dist = -1, source, F(m["distance"])
    else:
        class_id = int(det["class_id"])
        with np.errstate(all="ignore"):
            cx = (F(det["x1"]) + F(det["x2"])) / F(2.0)
            direc = direction(cx / F(c.width))
        dist = F(m["distance"]) if measured else c.default_depth
        flags = 0 if measured else NO_DEPTH
    prio = priority(c, class_id, dist)
    if dist < c.beep_m:
        flags |= BEEP
    if prio == CRITICAL:
        flags |= CRITICAL_ALERT | INTERRUPT
    return class_id, direc, prio, dist, flags


def order_key(cand):
    """Rule 4 as a sort key of (source, class_id, direction, priority, distance, flags)."""
    source, _, direc, prio, dist, _ = cand
    return (-prio, float(dist), direc, source)


def key_of(class_id, direc):
    ck = 0 if class_id == -1 else 1 + min(max(class_id, 0), 83)
    return ck * 3 + direc


def new_state(n=1):
    return np.zeros(n, STATE_DTYPE)


def frame_candidates(c, f, meas, dets, ndets):
    n_det = 0
    if ndets is not None:
        n_det, _ = det_count(int(ndets[f]), dets.shape[1], c.max_dets)
    out = []
    for s in range(3 + n_det):
        r = classify(c, s, meas[f, s], dets[f, s - 3] if s >= 3 else None)
        if r is not None:
            out.append((s,) + r)
    return sorted(out, key=order_key)


def arbitrate(c, track_offset, timestamps, meas, states, event_cap, dets=None, ndets=None):
    """Rules 3-6. states [n_tracks] STATE_DTYPE, advanced in place. Returns (events: a list of EVENT_DTYPE arrays with ALL the
    events of each track, nevents [n_tracks], status); the device writes the first event_cap of each."""
    n_tracks = len(track_offset) - 1
    n_frames = len(timestamps)
    status_invalid = status_cap = False
    all_events, nevents = [], np.zeros(n_tracks, np.int32)
    for tr in range(n_tracks):
        f0, f1 = int(track_offset[tr]), int(track_offset[tr + 1])
        ev = []
        if f0 < 0 or f1 < f0 or f1 > n_frames:
            status_invalid = True
            all_events.append(np.zeros(0, EVENT_DTYPE))
            continue
        st = states[tr]
        prev = None
        for f in range(f0, f1):
            t = int(timestamps[f])
            if prev is not None and t < prev:
                status_invalid = True
                continue
            prev = t
            if ndets is not None and det_count(int(ndets[f]), dets.shape[1], c.max_dets)[1]:
                status_invalid = True
            announced = 0
            for source, class_id, direc, prio, dist, flags in frame_candidates(c, f, meas, dets, ndets):
                if announced >= c.max_events_per_frame:
                    break
                key = key_of(class_id, direc)
                last1 = int(st["last_prio1"][key])
                if last1 == 0 or prio + 1 > last1 or t - int(st["last_ns"][key]) >= c.cooldown_ns[prio]:
                    st["last_prio1"][key] = prio + 1
                    st["last_ns"][key] = t
                    ev.append((f, source, class_id, direc, prio, dist, flags, 0))
                    announced += 1
        st["events_total"] += len(ev)
        nevents[tr] = len(ev)
        status_cap = status_cap or len(ev) > event_cap
        all_events.append(np.array(ev, EVENT_DTYPE) if ev else np.zeros(0, EVENT_DTYPE))
    return all_events, nevents, E_INVALID if status_invalid else E_OUTPUT_TOO_SMALL if status_cap else OK


def run(c, depth, track_offset, timestamps, states, event_cap, dets=None, ndets=None):
    """measure, then arbitrate. Returns (events, nevents, status, meas)."""
    meas, st_m, _ = measure(depth, c, dets, ndets)
    events, nevents, st_a = arbitrate(c, track_offset, timestamps, meas, states, event_cap, dets, ndets)
    status = E_INVALID if E_INVALID in (st_m, st_a) else st_a
    return events, nevents, status, meas


# ---- what is said (H16:480-487) ------------------------------------------------------------------------------------------
def c_fixed1(x):
    """printf("%.1f") of an fp32 value: the decimal expansion of the exact binary value, round-half-even on it."""
    from decimal import ROUND_HALF_EVEN, Decimal
    return str(Decimal(float(F(x))).quantize(Decimal("0.1"), rounding=ROUND_HALF_EVEN))


def message(event, names=None, obstacle_name="obstacle"):
    """The text spoken for an event: name [+ ", " + distance with one decimal + " meters" when distance < 5.0f]."""
    cid = int(event["class_id"])
    name = obstacle_name if cid == -1 else names[cid] if names is not None and 0 <= cid < len(names) else "object"
    dist = F(event["distance"])
    return name + (", %s meters" % c_fixed1(dist) if dist < F(5.0) else "")


def audio_calls(event, names=None):
    """The calls on IAudioFeedback an event makes, in order, as tuples."""
    calls = [("speak", message(event, names), int(event["priority"]), bool(event["flags"] & INTERRUPT))]
    if event["flags"] & BEEP:
        calls.append(("playBeep", int(event["direction"]), 800, 200, F(0.8)))
    if event["flags"] & CRITICAL_ALERT:
        calls.append(("playCriticalAlert", int(event["direction"])))
    return calls
