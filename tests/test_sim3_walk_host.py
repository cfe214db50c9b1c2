"""The closed walk of the loop alignment selftest, through the restatements alone (tools/sim3_walk.py): the numbers
tests/test_cpp_sim3.py doubles for its bounds are what the script gives, the aligned edge closes the loop and the unit-length one
does not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim3_walk as W   # noqa: E402


def test_walk_reference_numbers():
    r = W.run()
    s = r["sim"]
    assert s["valid"] == 1 and s["map_points"] == 600 and s["n_corr"] == 300 and s["n_inliers"] == 257
    assert abs(s["s"] - 0.685703) < 1e-5 and abs(abs(s["s"] * W.DRIFT - 1.0) - 0.028555) < 1e-5
    assert abs(s["t_true_len"] - 0.318342) < 1e-5 and abs(s["edge_t_err"] - 0.007195) < 1e-5
    assert abs(r["aligned"][0] - 0.00762) < 1e-4 and abs(r["aligned"][1] - 0.007367) < 1e-5      # WALK_REF of test_cpp_sim3.py
    assert abs(r["unit"][1] - 0.680728) < 1e-4 and abs(r["before"][1] - 0.527791) < 1e-5
    assert r["unit"][1] > 40 * r["aligned"][1]                       # the unit-length edge leaves the end pose where it was, or worse


def test_selftest_and_script_share_the_scene_constants():
    src = open(os.path.join(ROOT, "tests", "cpp", "sim3_selftest.cpp")).read()
    assert "K_FRAMES = %d, N_POINTS = %d" % (W.K_FRAMES, W.N_POINTS) in src
    assert "DRIFT = %.1f, RADIUS = %.1f, CLOSE = %.2f" % (W.DRIFT, W.RADIUS, W.CLOSE) in src
    assert "2654435761LL + 12345LL" in src
