"""Obstacle alerts on the MI355X (aria_alert_*, kernels in aria_slam_amd/csrc/alert_stage.hip) against their definition, the
NumPy restatement aria_slam_amd/alert_ref.py: measurements, events, counts and states are BITWISE equal. The selection is exact
and the arbitration is integer arithmetic and fp32 compares, so a difference is a bug, never a tolerance. Every output lies
between guard bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_cases as AC   # noqa: E402
from aria_slam_amd import alert_ref as R   # noqa: E402

ARIA_E_INVALID, ARIA_E_NO_DEVICE, ARIA_E_OUTPUT_TOO_SMALL = -1, -2, -5
GUARD_EVENTS = 3                                          # guard records beyond every track's event_cap


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def work(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return s


def _dev(torch, work, a):
    with torch.cuda.stream(work):
        t = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to("cuda:0")       # a copy: the shared cases are read-only
    work.synchronize()
    return t


def _full(torch, work, nbytes, value=AC.GUARD):
    with torch.cuda.stream(work):
        t = torch.full((max(nbytes, 1),), value, dtype=torch.uint8, device="cuda:0")
    work.synchronize()
    return t


def _handle(aria, work, cfg, **kw):
    return aria.HipObstacleAlerter.from_ref_config(cfg, stream=work.cuda_stream, **kw)


def _measure_dev(torch, work, h, depth, dets, ndets):
    """measure_batch_device with one guard frame of records in front of and behind the output."""
    n, H, pitch = depth.shape
    d_meas = _full(torch, work, 16 * 64 * (n + 2))
    out = d_meas[16 * 64:]
    h.measure_batch_device(_dev(torch, work, depth), H * pitch, pitch, n, out, None if dets is None else _dev(torch, work, dets),
                           None if ndets is None else _dev(torch, work, ndets), 0 if dets is None else dets.shape[1])
    status = h.status()
    raw = d_meas.cpu().numpy()
    assert (raw[:16 * 64] == AC.GUARD).all() and (raw[16 * 64 * (n + 1):] == AC.GUARD).all(), "records outside the frames were touched"
    return raw[16 * 64:16 * 64 * (n + 1)].view(R.MEAS_DTYPE).reshape(n, 64), status, out


def _report(name, got, want):
    bad = np.argwhere(got != want)
    print("%s: %d of %d records differ" % (name, len(bad), want.size))
    for f, s in bad[:8]:
        print("   frame %d source %d: got %s want %s" % (f, s, got[f, s], want[f, s]))


@pytest.mark.parametrize("pct", ["default", "first", "last"])
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("W,H", AC.SIZES)
def test_measurement_equals_the_restatement(aria, torch_cuda, work, W, H, pad, pct):
    """Twelve frames per size (tests/alert_cases.py measure_case): 1-pixel, empty, inverted, full-image, off-image, clipped and
    non-finite rectangles; a left edge at each of x % 4 = 0..3; all depths invalid; n = min_valid - 1 and n = min_valid; one
    repeated value with rank k inside the run; patterns that differ only in the lowest mantissa bits, only in the exponent and
    only in the middle bits; denormals, -0.0f, negatives, Inf and NaN among valid values; 61 detections; a count above max_dets
    and counts outside [0, det_cap]. pct: the default percentiles, k = 0 and k = n - 1. pad = 5: pitch = width + 5 with NaN in
    the padding. A lane's loop over rows and columns takes several passes only at 300 x 200."""
    case = AC.measure_case(W, H, pad, pct)
    h = _handle(aria, work, case.cfg)
    try:
        got, status, _ = _measure_dev(torch_cuda, work, h, case.depth, case.dets, case.ndets)
        _report("%dx%d pad %d %s" % (W, H, pad, pct), got, case.meas)
        assert got.tobytes() == case.meas.tobytes()
        assert np.isfinite(got["distance"]).all()
        assert status == ARIA_E_INVALID == case.status and h.dets_seen() == 63 == case.seen       # counts 65 and -1; count 63
        assert h.status() == 0 and h.dets_seen() == 0                # reported once
        # the host form, and zones only
        got_h, status_h = h.measure(case.depth, case.dets, case.ndets)
        assert got_h.tobytes() == case.meas.tobytes() and status_h == ARIA_E_INVALID
        zones, status_z = h.measure(case.depth)
        want_z = R.measure(case.depth, case.cfg)[0]
        assert zones.tobytes() == want_z.tobytes() and status_z == 0
        assert (zones["flags"][:, 3:] == 0).all() and zones[:, :3].tobytes() == case.meas[:, :3].tobytes()
    finally:
        h.close()


def test_default_zones_on_a_seeded_frame(aria, torch_cuda, work):
    """752 x 480 under the defaults, zones only: 94 680, 81 360 and 94 680 pixels a zone."""
    case = AC.default_zones()
    h = _handle(aria, work, case.cfg)
    try:
        got, status, _ = _measure_dev(torch_cuda, work, h, case.depth, None, None)
        _report("default zones", got, case.meas)
        print(got[0, :3])
        assert got.tobytes() == case.meas.tobytes() and status == 0
        assert (got["flags"][0, :3] == R.MEAS_SOURCE | R.MEAS_OK).all() and got["distance"][0, R.RIGHT] < 0.9 < got["distance"][0, R.LEFT]
    finally:
        h.close()


def _frames_dev(torch, work, case):
    return tuple(_dev(torch, work, a) for a in (case.timestamps, case.meas, case.dets, case.ndets))


def _arbitrate_dev(torch, work, h, case, track_offset=None, states=None, event_cap=None, frames=None):
    """arbitrate_batch_device with guard records behind every track's events, a guard state and a guard count behind the last.
    frames: the timestamps, measurements, detections and counts already in HBM."""
    off = case.track_offset if track_offset is None else np.asarray(track_offset, np.int32)
    cap = case.event_cap if event_cap is None else event_cap
    n_tracks, n_frames = len(off) - 1, len(case.timestamps)
    before = case.states[0] if states is None else states
    d_states = _dev(torch, work, np.concatenate([before.view(np.uint8).reshape(-1), np.full(2320, AC.GUARD, np.uint8)]))
    d_events = _full(torch, work, 32 * (cap * n_tracks + GUARD_EVENTS))
    d_nev = _full(torch, work, 4 * (n_tracks + 1))
    d_ts, d_meas, d_dets, d_ndets = frames or _frames_dev(torch, work, case)
    h.arbitrate_batch_device(_dev(torch, work, off), n_tracks, d_ts, n_frames, d_meas, d_states, d_events, cap, d_nev, d_dets, d_ndets,
                             case.dets.shape[1])
    status = h.status()
    raw_s = d_states.cpu().numpy()
    assert (raw_s[2320 * n_tracks:] == AC.GUARD).all()
    raw_n = d_nev.cpu().numpy()
    assert (raw_n[4 * n_tracks:] == AC.GUARD).all()
    nev = raw_n[:4 * n_tracks].view(np.int32)
    raw_e = d_events.cpu().numpy()
    assert (raw_e[32 * cap * n_tracks:] == AC.GUARD).all(), "events beyond the last track's capacity were touched"
    ev = raw_e[:32 * cap * n_tracks].view(R.EVENT_DTYPE).reshape(n_tracks, cap)
    for t in range(n_tracks):
        assert (ev[t, min(int(nev[t]), cap):].view(np.uint8) == AC.GUARD).all(), "track %d: slots beyond its events were touched" % t
    return ev, nev, raw_s[:2320 * n_tracks].view(R.STATE_DTYPE), status


def _check_arb(torch, work, h, case, name, frames=None):
    ev, nev, states, status = _arbitrate_dev(torch, work, h, case, frames=frames)
    print("%s: events per track %s, status %d" % (name, nev.tolist()[:12], status))
    assert nev.tobytes() == case.nevents.tobytes(), (name, nev, case.nevents)
    for t, want in enumerate(case.events):
        n = min(len(want), case.event_cap)
        if ev[t, :n].tobytes() != want[:n].tobytes():
            bad = [i for i in range(n) if ev[t, i] != want[i]]
            print("   track %d: first difference at event %d: got %s want %s" % (t, bad[0], ev[t, bad[0]], want[bad[0]]))
        assert ev[t, :n].tobytes() == want[:n].tobytes(), (name, t)
    assert states.tobytes() == case.states[1].tobytes(), name
    assert status == case.status and h.status() == 0
    return ev, nev, states


@pytest.mark.parametrize("name", ["timeline", "sketch", "full_house", "many_tracks", "long_track"])
def test_arbitration_equals_the_restatement(aria, torch_cuda, work, name):
    """The hand-written timeline of rule 5 (cooldown met exactly and missed by a nanosecond, escalation, de-escalation,
    max_events_per_frame, a full tie, a decreasing timestamp), the sketch's own case, 64 candidates in one frame and none in the
    next, 33 tracks of different lengths (0 and 1 among them) in one call, and one track of 60 random frames."""
    case = getattr(AC, name)()
    h = _handle(aria, work, case.cfg)
    try:
        ev, nev, _ = _check_arb(torch_cuda, work, h, case, name)
        if name == "full_house":
            assert np.bincount(ev[0, :nev[0]]["frame"], minlength=3)[:2].tolist() == [64, 0]
        # the host form gives the same, and slots it does not write keep the caller's bytes
        states = case.states[0].copy()
        fill = np.full((len(case.nevents), case.event_cap), AC.GUARD, np.uint8).repeat(32, axis=1).view(R.EVENT_DTYPE)
        ev_h, nev_h, rc = h.arbitrate(case.track_offset, case.timestamps, case.meas, states, case.event_cap, case.dets, case.ndets, events=fill)
        assert rc == case.status and nev_h.tobytes() == nev.tobytes() and ev_h.tobytes() == ev.tobytes()
        assert states.tobytes() == case.states[1].tobytes()
    finally:
        h.close()


def test_a_track_in_one_call_and_in_three_chunks(aria, torch_cuda, work):
    """60 frames in one call, and as [0, 13), [13, 27), [27, 60) through the state: the events and the final state are bytewise
    equal. The same track at two places of a batch of three gives the same events and states at both."""
    torch = torch_cuda
    case = AC.long_track()
    h = _handle(aria, work, case.cfg)
    try:
        ev, nev, states = _check_arb(torch, work, h, case, "long track")
        st = case.states[0].copy()
        parts = []
        for a, b in ((0, 13), (13, 27), (27, 60)):
            e, n, st, status = _arbitrate_dev(torch, work, h, case, track_offset=[a, b], states=st.copy())
            assert status == 0
            parts.append(e[0, :n[0]])
        chunks = np.concatenate(parts)
        assert len(chunks) == nev[0] and chunks.tobytes() == ev[0, :nev[0]].tobytes()
        assert st.tobytes() == states.tobytes() and st["events_total"][0] == nev[0]
        # two empty tracks behind it
        e3, n3, s3, status = _arbitrate_dev(torch, work, h, case, track_offset=[0, 60, 60, 60], states=R.new_state(3))
        assert n3.tolist() == [nev[0], 0, 0] and status == 0
    finally:
        h.close()
    # the same frames twice in one batch, another track between them
    cfg, (ts, meas, dets, ndets) = AC.random_frames(7, 60)
    mid = AC.random_frames(8, 25)[1]
    ts2, meas2, dets2, ndets2 = (np.concatenate([a, b, a]) for a, b in zip((ts, meas, dets, ndets), mid))
    ts2[60:85] += ts[-1] - mid[0][0] + 1
    ts2[85:] += ts2[84] - ts[0] + 1
    twice = AC.make_arb(cfg, ts2, meas2, dets2, ndets2, [0, 60, 85, 145], 400)
    h = _handle(aria, work, cfg)
    try:
        ev2, nev2, states2 = _check_arb(torch, work, h, twice, "twice")
        assert nev2[0] == nev2[2] == nev[0]
        a, b = ev2[0, :nev2[0]].copy(), ev2[2, :nev2[2]].copy()
        b["frame"] -= 85
        assert a.tobytes() == b.tobytes() == ev[0, :nev[0]].tobytes()
        assert states2["last_prio1"][0].tobytes() == states2["last_prio1"][2].tobytes()
        assert (states2["last_ns"][2] - states2["last_ns"][0])[states2["last_prio1"][0] != 0].tolist() == [int(ts2[85] - ts2[0])] * int((states2["last_prio1"][0] != 0).sum())
    finally:
        h.close()


def test_two_tracks_share_frames_under_different_thresholds(aria, torch_cuda, work):
    """The same 60 frames in HBM under two handles: the defaults, and zone_alert_m 1.0 with crit_m 0.5."""
    a, b = AC.long_track(), AC.long_track(zone_alert_m=1.0, crit_m=0.5)
    assert a.meas.tobytes() == b.meas.tobytes() and a.timestamps.tobytes() == b.timestamps.tobytes()
    ha, hb = _handle(aria, work, a.cfg), _handle(aria, work, b.cfg)
    try:
        frames = _frames_dev(torch_cuda, work, a)
        before = [t.cpu().numpy().tobytes() for t in frames]
        ea, na, _ = _check_arb(torch_cuda, work, ha, a, "defaults", frames)
        eb, nb, _ = _check_arb(torch_cuda, work, hb, b, "stricter", frames)
        assert ea[0, :na[0]].tobytes() != eb[0, :nb[0]].tobytes()
        assert [t.cpu().numpy().tobytes() for t in frames] == before          # frames are only read
    finally:
        ha.close()
        hb.close()


def test_event_cap_exceeded(aria, torch_cuda, work):
    """event_cap = 3: the total is above the capacity, three events are written, the guards behind them are intact, the state
    is the one a large capacity leaves, and ARIA_E_OUTPUT_TOO_SMALL is reported once. event_cap = 0 with no event buffer too."""
    small, large = AC.long_track(event_cap=3), AC.long_track()
    assert small.nevents[0] == large.nevents[0] > 3 and small.states[1].tobytes() == large.states[1].tobytes()
    h = _handle(aria, work, small.cfg)
    try:
        ev, nev, states = _check_arb(torch_cuda, work, h, small, "cap 3")
        assert ev[0].tobytes() == large.events[0][:3].tobytes()
        L = aria.load_library()
        torch = torch_cuda
        d_states, d_nev = _dev(torch, work, small.states[0]), _full(torch, work, 8)
        args = [_dev(torch, work, x) for x in (small.track_offset, small.timestamps, small.meas, small.dets, small.ndets)]
        rc = L.aria_alert_arbitrate_batch_device(h._h, args[0].data_ptr(), 1, args[1].data_ptr(), 60, args[2].data_ptr(), args[3].data_ptr(),
                                                 args[4].data_ptr(), AC.DET_CAP, d_states.data_ptr(), None, 0, d_nev.data_ptr())
        assert rc == 0 and h.status() == ARIA_E_OUTPUT_TOO_SMALL and h.status() == 0
        assert d_nev.cpu().numpy()[:4].view(np.int32)[0] == nev[0] and d_states.cpu().numpy().tobytes() == large.states[1].tobytes()
    finally:
        h.close()


def test_bad_track_offsets_are_deferred(aria, torch_cuda, work):
    """Offsets that decrease or leave [0, n_frames]: the track is skipped, its state and event slots are untouched, the other
    tracks are unaffected."""
    case = AC.long_track()
    h = _handle(aria, work, case.cfg)
    try:
        ev, nev, states, status = _arbitrate_dev(torch_cuda, work, h, case, track_offset=[0, 60, 30, 61, 61], states=R.new_state(4))
        assert status == ARIA_E_INVALID and nev.tolist() == [case.nevents[0], 0, 0, 0] and h.status() == 0
        assert states[0].tobytes() == case.states[1][0].tobytes() and not states[1:].tobytes().strip(b"\0")
        want = R.new_state(4)
        assert R.arbitrate(case.cfg, np.array([0, 60, 30, 61, 61], np.int32), case.timestamps, case.meas, want, 400, case.dets, case.ndets)[2] == -1
        assert want.tobytes() == states.tobytes()
    finally:
        h.close()


def test_run_batch_device_on_analytic_depth(aria, torch_cuda, work):
    """tsdf_cases' analytic scene (a plane and a sphere from three poses) as 80 x 60 depth maps, with two boxes a frame: measure
    and arbitrate in one call through the handle's buffer equal the restatement's run(), events, counts and state."""
    import tsdf_cases as TC
    torch = torch_cuda
    d, _, _ = TC.scene_frames()
    depth = np.ascontiguousarray(d, np.float32).reshape(3, TC.H, TC.W)
    cfg = R.config(width=TC.W, height=TC.H, zone_top=TC.H // 4, zone_bottom=TC.H, zone_alert_m=6.0, medium_m=4.0, max_dets=8)
    dets = np.zeros((3, 8), R.DETECTION_DTYPE)
    for f in range(3):
        dets[f, 0] = AC.det(TC.W * 0.4, TC.H * 0.3, TC.W * 0.6, TC.H * 0.7, 0)
        dets[f, 1] = AC.det(2, 2, 20, 20, 56)
    ndets = np.full(3, 2, np.int32)
    ts = np.array([0, 100 * AC.MS, 1000 * AC.MS], np.int64)
    off = np.array([0, 3], np.int32)
    want_states = R.new_state(1)
    want_ev, want_n, want_status, want_meas = R.run(cfg, depth, off, ts, want_states, 16, dets, ndets)
    assert want_n[0] >= 2 and want_status == 0 and ((want_meas["flags"] & R.MEAS_OK) != 0)[:, :5].any()
    h = _handle(aria, work, cfg)
    try:
        d_states = _dev(torch, work, np.concatenate([R.new_state(1).view(np.uint8), np.full(64, AC.GUARD, np.uint8)]))
        d_events, d_nev = _full(torch, work, 32 * 16 + 32), _full(torch, work, 8)
        h.run_batch_device(_dev(torch, work, depth), TC.W * TC.H, TC.W, 3, _dev(torch, work, off), 1, _dev(torch, work, ts), d_states, d_events,
                           16, d_nev, _dev(torch, work, dets), _dev(torch, work, ndets), 8)
        assert h.status() == 0
        n = int(d_nev.cpu().numpy()[:4].view(np.int32)[0])
        raw = d_events.cpu().numpy()
        print("analytic scene: %d events" % n, raw[:32 * n].view(R.EVENT_DTYPE))
        assert n == want_n[0] and raw[:32 * n].tobytes() == want_ev[0].tobytes() and (raw[32 * n:] == AC.GUARD).all()
        assert (d_nev.cpu().numpy()[4:] == AC.GUARD).all()
        s = d_states.cpu().numpy()
        assert s[:2320].tobytes() == want_states.tobytes() and (s[2320:] == AC.GUARD).all()
        # the host form
        st = R.new_state(1)
        ev_h, nev_h, rc = h.run(depth, ts, st, 16, dets=dets, ndets=ndets)
        assert rc == 0 and nev_h[0] == n and ev_h[0, :n].tobytes() == want_ev[0].tobytes() and st.tobytes() == want_states.tobytes()
    finally:
        h.close()


def test_lifecycle_and_refusals(aria, torch_cuda, work):
    """Create refuses a bad struct size and a device that is not there; a borrowed stream is reported and survives close; a
    second close is a no-op; NULL pointers, negative counts, a pitch below the width and detections without counts are refused
    before anything is enqueued; n_frames = 0 and n_tracks = 0 are accepted; a second live handle of another size measures its
    own size."""
    from aria_slam_amd import _lib
    torch = torch_cuda
    L = aria.load_library()
    cfg = _lib.AlertConfig()
    L.aria_alert_default_config(C.byref(cfg))
    hh = C.c_void_p()
    cfg.struct_size += 4
    assert L.aria_alert_create(C.byref(cfg), C.byref(hh)) == ARIA_E_INVALID and not hh.value
    cfg.struct_size -= 4
    cfg.device = torch.cuda.device_count()
    assert L.aria_alert_create(C.byref(cfg), C.byref(hh)) == ARIA_E_NO_DEVICE and not hh.value
    assert ("device %d not present" % cfg.device) in L.aria_last_hip_error().decode()

    small, big = AC.measure_case(37, 19, 0), AC.measure_case(64, 24, 5)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    h = aria.HipObstacleAlerter.from_ref_config(small.cfg, stream=s.cuda_stream)
    own = aria.HipObstacleAlerter.from_ref_config(big.cfg)
    try:
        assert h.stream == s.cuda_stream and own.stream and own.stream != s.cuda_stream
        assert h.ref_config == small.cfg and own.ref_config == big.cfg
        for x in (h, own):
            assert x.status() == 0 and x.dets_seen() == 0
            x.check()
        n, H, pitch = small.depth.shape
        d_depth, d_dets, d_ndets = (_dev(torch, work, a) for a in (small.depth, small.dets, small.ndets))
        d_meas = _full(torch, work, 16 * 64 * n)
        m = lambda **k: L.aria_alert_measure_batch_device(   # noqa: E731
            h._h, k.get("depth", d_depth.data_ptr()), k.get("stride", H * pitch), k.get("pitch", pitch), k.get("n", n),
            k.get("dets", d_dets.data_ptr()), k.get("ndets", d_ndets.data_ptr()), k.get("cap", AC.DET_CAP), k.get("meas", d_meas.data_ptr()))
        for k in (dict(depth=None), dict(meas=None), dict(n=-1), dict(pitch=36), dict(stride=-1), dict(dets=None), dict(ndets=None), dict(cap=-1)):
            assert m(**k) == ARIA_E_INVALID, k
        assert h.status() == 0 and (d_meas.cpu().numpy() == AC.GUARD).all()       # nothing was enqueued
        assert m(n=0) == 0 and m(dets=None, ndets=None, cap=0) == 0 and h.status() == 0
        assert m() == 0 and h.status() == ARIA_E_INVALID             # the case's bad counts, deferred
        assert d_meas.cpu().numpy().view(R.MEAS_DTYPE).tobytes() == small.meas.tobytes()
        # both handles alive: each measures its own size
        got, status, _ = _measure_dev(torch, work, own, big.depth, big.dets, big.ndets)
        assert got.tobytes() == big.meas.tobytes()
        tl = AC.timeline()
        a = [_dev(torch, work, x) for x in (tl.track_offset, tl.timestamps, tl.meas, tl.dets, tl.ndets, tl.states[0])]
        d_ev, d_nev = _full(torch, work, 32 * 32), _full(torch, work, 4)
        arb = lambda **k: L.aria_alert_arbitrate_batch_device(   # noqa: E731
            h._h, k.get("off", a[0].data_ptr()), k.get("tracks", 1), k.get("ts", a[1].data_ptr()), k.get("n", 9), k.get("meas", a[2].data_ptr()),
            a[3].data_ptr(), a[4].data_ptr(), AC.DET_CAP, k.get("states", a[5].data_ptr()), k.get("ev", d_ev.data_ptr()), k.get("cap", 32),
            k.get("nev", d_nev.data_ptr()))
        for k in (dict(off=None), dict(tracks=-1), dict(ts=None), dict(n=-1), dict(meas=None), dict(states=None), dict(ev=None), dict(cap=-1),
                  dict(nev=None)):
            assert arb(**k) == ARIA_E_INVALID, k
        assert arb(tracks=0) == 0 and h.status() == 0 and (d_ev.cpu().numpy() == AC.GUARD).all()
        assert L.aria_alert_run_batch_device(h._h, None, 0, pitch, 1, None, None, 0, a[0].data_ptr(), 1, a[1].data_ptr(), a[5].data_ptr(),
                                             d_ev.data_ptr(), 32, d_nev.data_ptr()) == ARIA_E_INVALID
        assert L.aria_alert_measure(h._h, None, 0, pitch, 1, None, None, 0, None) == ARIA_E_INVALID
        assert L.aria_alert_arbitrate(h._h, None, 1, None, 0, None, None, None, 0, None, None, 0, None) == ARIA_E_INVALID
    finally:
        h.close()
        own.close()
    h.close()                                                        # a second close is a no-op
    with torch.cuda.stream(s):
        x = torch.arange(8, device="cuda:0") * 2
    s.synchronize()
    assert int(x.sum()) == 56
