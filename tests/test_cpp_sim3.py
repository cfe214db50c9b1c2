"""Loop alignment through the C++ adapters on the GPU (aria_hip/HipSim3Aligner.hpp: HipSim3Aligner, makeSim3Verifier)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aria_slam_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# The restatement's worst error over the ground-truth cases of tests/sim3_cases.py (tools/sim3_gap.py, pinned by
# tests/test_sim3_host.py): rotation (deg), translation over s, relative scale. The adapters are allowed twice that, as the
# device is in tests/test_gpu_sim3.py.
GT_WORST = (0.1034, 0.01361, 0.00588)
BOOTSTRAP = 1

# The closed walk run through the restatements alone (tools/sim3_walk.py; pinned by tests/test_sim3_walk_host.py): the error of
# the optimised end pose against the scene's truth with the aligned loop edge, rotation 0.00762 deg and translation 0.007367
# units, and the restatement's scale, 0.685703 for a truth of 1 / 1.5 (a relative error of 0.028555: the loop's baseline is
# 0.32 units at depths of 4 to 12, so the image sees s weakly). The bounds are twice these. With the unit-length edge the
# restatement's own run ends 0.680728 units from the truth, 46 times the translation bound.
WALK_REF = (0.00762, 0.007367)
WALK_SCALE_REF = 0.028555


def test_host_adapters_export_the_aligner(aria):
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    so = os.path.join(PKG, "libaria_hip_adapters.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert "aria::adapters::hip::HipSim3Aligner::estimate(" in syms
    assert "aria::adapters::hip::HipSim3Aligner::estimateAgainstMap(" in syms
    assert "aria::adapters::hip::makeSim3Verifier(" in syms
    hdr = open(os.path.join(PKG, "host", "include", "aria_hip", "MapTracker.hpp")).read()
    assert "int anchorPair() const" in hdr


def test_cpp_sim3_selftest(aria):
    """tests/cpp/sim3_selftest.cpp.

    - estimate: 400 correspondences between two clouds with X2 = 2 R X1 + t, 0.3 px of pixel noise, a fifth of them re-paired:
      the similarity within twice the restatement's worst error over its ground-truth cases (the scene is milder than those:
      no depth noise), s = 2 found; two correspondences give no model.
    - estimateAgainstMap on the map a MapTracker bootstraps, keyframe 1 = the pair's second view, keyframe 2 = its first, the
      join on the device through both views of one pair: every match has a landmark on both sides, one map so s = 1, and the
      similarity is the inverse of the tracker's pose -- the same bounds -- whose translation is one map unit long (the
      two-view stage's |t| = 1 to 1e-6), although the scene's baseline is 0.5.
    - makeSim3Verifier overwrites a candidate's relative pose (R = I, t = (0, 0, 1)) with that edge when n_inliers >= 20, leaves
      it as it was when the gate is not met or a keyframe is unknown, never rejects by itself, and passes a rejection of the
      verifier in front of it through without aligning.
    - the closed walk of tools/sim3_walk.py, formula for formula: a generated 3-D scene, 16 keyframes that return to within
      0.32 units of their start, trajectory and map drifted in scale by 1.5 at the end. The first and the last pair are
      triangulated (HipMapper), the verifier runs behind a stand-in for the two-view verification that hands over the true
      rotation and direction at length 1, and the pose graph (HipPoseGraphOptimizer, 20 iterations) is optimised with the
      verifier's edge and with the unit-length one. With the verifier the edge is in map units and s is recovered, and the
      optimised end pose lies within twice the restatement's error of the truth (measured on the restatement: 0.00762 deg,
      0.007367 units; bound 0.01524 deg, 0.014734 units). The same script with the parent's unit-length edge misses that
      bound (the restatement: 0.680728 units)."""
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    src = os.path.join(ROOT, "tests", "cpp", "sim3_selftest.cpp")
    exe = os.path.join(ROOT, "build", "sim3_selftest")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host", "include"),
                           src, "-o", exe, "-L" + PKG, "-laria_hip_adapters", "-laria_orb_hip", "-lz", "-Wl,-rpath," + PKG])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    kv = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    e = kv["estimate"]
    assert e[0] == "1" and float(e[1]) <= 2 * GT_WORST[0] and float(e[2]) <= 2 * GT_WORST[1] and float(e[3]) <= 2 * GT_WORST[2]
    assert 300 <= int(e[4]) <= 330 and float(e[5]) < 1.0            # 80 of 400 re-paired; 0.3 px of noise
    assert kv["too_few"] == ["0"]
    b = kv["bootstrap"]
    assert int(b[0]) == BOOTSTRAP and int(b[1]) > 300 and int(b[2]) >= 0
    a = kv["against_map"]
    assert a[0] == "1" and float(a[1]) <= 2 * GT_WORST[0] and float(a[2]) <= 2 * GT_WORST[1] and float(a[3]) <= 2 * GT_WORST[2]
    assert int(a[4]) == int(b[1]) == int(a[7]) and int(a[5]) > 0.9 * int(a[4])      # every mapped keypoint is joined
    assert abs(float(a[6]) - 1.0) <= 2 * GT_WORST[1]                 # the edge is one map unit long
    v = kv["verifier"]
    assert v[:2] == ["1", "1"] and float(v[2]) <= 2 * GT_WORST[0] and float(v[3]) <= 2 * GT_WORST[1]
    assert abs(float(v[4]) - 1.0) <= 2 * GT_WORST[2] and int(v[5]) == int(a[4]) and int(v[6]) == int(a[5])
    assert kv["gate"] == ["1", "0", "0.0", "0.0", "1.0", "1.0"]
    assert kv["unknown"] == ["1", "0", "1.0", "0", "1"]
    # the closed walk: 16 keyframes back to within 0.32 units of the start, the last pair's map 1.5 times the first pair's
    assert [int(x) for x in kv["walk_map"]] == [300, 300]
    w = kv["walk_edge"]
    assert w[:2] == ["1", "1"] and int(w[3]) == 300 and int(w[4]) > 240           # 43 of the 300 matches are mis-paired
    assert abs(float(w[2]) * 1.5 - 1.0) <= 2 * WALK_SCALE_REF                     # s is recovered
    assert abs(float(w[6]) - float(w[7])) <= 2 * WALK_REF[1] and float(w[8]) <= 2 * WALK_REF[1]   # the edge is in map units
    assert abs(float(w[7]) - 0.318342) < 1e-5                                     # where the unit-length edge says 1
    al, un = [float(x) for x in kv["walk_aligned"]], [float(x) for x in kv["walk_unit"]]
    print("end pose: aligned %.5f deg %.6f (restatement %.5f %.6f, bound twice that), unit-length %.5f deg %.6f" % (tuple(al) + WALK_REF + tuple(un)))
    assert al[0] <= 2 * WALK_REF[0] and al[1] <= 2 * WALK_REF[1]                  # the graph brings the end pose to the start
    assert un[1] > 2 * WALK_REF[1] and un[1] > 0.5                                # the parent's edge misses the bound


def test_euroc_frontend_loop_align_flag(aria, tmp_path):
    """The driver flag on the synthetic image sequence (a 2-D shift of a flat scene, 12 frames): plumbing only. The sequence
    is too short for a loop (30 frames between) and flat, so no candidate reaches the aligner; what the run shows is that the
    flag builds the aligner behind the reference verifier (the printed line, the output file created), that every other output
    file is byte for byte what it is without the flag, and that the flag is refused without --track-map. The accuracy check is
    test_cpp_sim3_selftest's closed walk."""
    from test_frontend_io import _make_dataset
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    _make_dataset(aria, str(tmp_path), 6, w=640, h=480)          # 6 synthetic pairs
    exe = os.path.join(PKG, "euroc_frontend")
    outs = {}
    for tag, extra in (("off", []), ("on", ["--loop-align", "sim3", "--loop-align-out", str(tmp_path / "align.txt")])):
        files = {k: str(tmp_path / ("%s_%s" % (tag, k))) for k in ("pose.txt", "track.txt", "opt.txt", "frames.csv")}
        run = subprocess.run([exe, str(tmp_path), "1000", "--csv", files["frames.csv"], "--pose", files["pose.txt"], "--track-map",
                              files["track.txt"], "--loop", "--loop-verify", "reference", "--optimize", files["opt.txt"]] + extra,
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        outs[tag] = (run.stdout, {k: open(v, "rb").read() for k, v in files.items()})
    assert outs["on"][1] == outs["off"][1] and all(len(v) > 0 for v in outs["off"][1].values())
    line = [l for l in outs["on"][0].splitlines() if l.startswith("loop align sim3")]
    assert len(line) == 1 and line[0].split()[:7] == ["loop", "align", "sim3", "candidates", "0", "replaced", "0"], outs["on"][0]
    assert not [l for l in outs["off"][0].splitlines() if l.startswith("loop align")]
    assert os.path.exists(str(tmp_path / "align.txt")) and open(str(tmp_path / "align.txt")).read() == ""
    for flags in (["--pose", str(tmp_path / "p.txt"), "--loop", "--loop-verify", "reference", "--loop-align", "sim3"],
                  ["--pose", str(tmp_path / "p.txt"), "--track-map", str(tmp_path / "t.txt"), "--loop", "--loop-align", "sim3"],
                  ["--pose", str(tmp_path / "p.txt"), "--track-map", str(tmp_path / "t.txt"), "--loop", "--loop-verify", "reference",
                   "--loop-align", "se3"]):
        bad = subprocess.run([exe, str(tmp_path), "1000"] + flags, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--track-map" in bad.stderr and "--loop-verify reference" in bad.stderr
