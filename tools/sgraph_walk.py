#!/usr/bin/env python3
"""The closed walk of tools/sim3_walk.py carried through the Sim(3) pose graph and the map correction, restatements alone
(CPU): the scene of sim3_walk.scene() (16 keyframes, scale drifted to 1.5 at the last one), the first and the last pair
triangulated (map_ref), the loop aligned (sim3_ref), then
  - graph_ref.optimize(20) with the loop edge [R t]                         (what the SE(3) graph makes of the loop),
  - sgraph_ref.optimize(20) with the loop edge (R, t, s)                    (the 7-DoF graph),
  - sgraph_ref.correct_points on the two pairs' points by their anchor keyframes 0 and L - 1,
once with the edge the alignment finds (s a few percent off) and once with the scene's exact edge (s = 1 / 1.5), which is what
the drift law is measured with. Prints the ATE (no alignment, all 16 camera centres against the scene's truth) of each, the
largest difference of a vertex scale from the drift law 1.5^(-i/15), and WALK_REF, WALK_SE3 and SCALE_GAP as
tests/test_sgraph_host.py holds them.
Usage: tools/sgraph_walk.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim3_walk as W   # noqa: E402

ITERATIONS = 20


def centres(poses_c2w):
    return np.asarray(poses_c2w)[:, :3, 3]


def ate(c, truth):
    """(rms, max) distance of the camera centres, nothing aligned."""
    d = np.sqrt(((np.asarray(c) - np.asarray(truth)) ** 2).sum(1))
    return float(np.sqrt((d * d).mean())), float(d.max())


def walk():
    """The walk's graph: (true centres, camera-to-world drifted poses, odometry edges [(i, j, 1, Z)], the loop's aria_sim3
    result dict, the two pairs' map points, the pair -> anchor vertex table)."""
    from aria_slam_amd import map_ref as M
    from aria_slam_amd import sim3_ref as N
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
    true, drifted, kp, _pts = W.scene()
    K, L, n = W.K_FRAMES, W.K_FRAMES - 1, W.N_POINTS
    frames = []
    for i in range(K):
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"], k["size"], k["response"] = kp[i, :, 0], kp[i, :, 1], 31.0, 1.0
        frames.append(k)
    ident = np.zeros(n, MATCH_DTYPE)
    ident["query_idx"] = ident["train_idx"] = np.arange(n)
    points = np.concatenate([M.triangulate_pair(frames[0], frames[1], ident, drifted[0], drifted[1], pair=0),
                             M.triangulate_pair(frames[L - 1], frames[L], ident, drifted[L - 1], drifted[L], pair=1)])
    corr, _back = N.associate(points, 1, 0, 2, 1, drifted[L][:3].ravel(), drifted[0][:3].ravel(), frames[L], frames[0],
                              W.loop_matches(), kp_stride=n)
    sim = N.estimate(corr, pair=L)
    c2w = np.array([np.linalg.inv(T) for T in drifted])
    odo = [(i - 1, i, 1.0, drifted[i - 1] @ np.linalg.inv(drifted[i])) for i in range(1, K)]
    truth = np.array([np.linalg.inv(T)[:3, 3] for T in true])
    T_true = true[0] @ np.linalg.inv(true[L])                       # camera L's coordinates -> camera 0's, the scene's truth
    return dict(truth=truth, c2w=c2w, odo=odo, sim=sim, exact=(T_true, 1.0 / W.DRIFT), points=points, pair_vertex=np.array([0, L - 1], np.int32), frames=frames,
                drifted=drifted)


def loop_rt(sim):
    Z = np.eye(4)
    Z[:3, :3], Z[:3, 3] = np.asarray(sim["R"], np.float64).reshape(3, 3), np.asarray(sim["t"], np.float64)
    return Z


def run(edge="exact"):
    """edge "exact": the scene's true loop edge (R, t of the truth, s = 1 / 1.5), what the drift law is measured with;
    "aligned": the (R, t, s) sim3_ref.estimate finds, s a few percent off."""
    from aria_slam_amd import graph_ref as G
    from aria_slam_amd import sgraph_ref as S
    w = walk()
    L = W.K_FRAMES - 1
    Z, s = w["exact"] if edge == "exact" else (loop_rt(w["sim"]), float(w["sim"]["s"]))
    out = dict(s=s, before=ate(centres(w["c2w"]), w["truth"]))
    g = G.PoseGraphOptimizer()
    sg = S.Sim3GraphOptimizer()
    for opt in (g, sg):
        for i in range(W.K_FRAMES):
            opt.set_initial_pose(i, w["c2w"][i])
        for i, j, _w, Zo in w["odo"]:
            opt.add_odometry_edge(i, j, Zo)
    g.add_loop_edge(0, L, Z)
    sg.add_loop_edge(0, L, Z, s)
    old = sg.vertices()
    g.optimize(ITERATIONS)
    sg.optimize(ITERATIONS)
    out["se3"] = ate(centres(np.array(g.poses)), w["truth"])
    out["sim3"] = ate(centres(np.array(sg.poses)), w["truth"])
    law = W.DRIFT ** (-np.arange(W.K_FRAMES) / (W.K_FRAMES - 1.0))
    out["scales"], out["centres"] = np.array(sg.scales), centres(np.array(sg.poses))
    out["scale_gap"] = float(np.abs(out["scales"] - law).max())
    moved, stats = S.correct_points(w["points"], w["pair_vertex"], 0, old, sg.vertices())
    out["stats"] = stats
    # the corrected points of pair 1 against the scene's: their depth in keyframe L - 1 was 1.5^(14/15) too large
    out["points_before"], out["points_after"] = w["points"], moved
    return out


def main():
    a = run("aligned")
    print("aligned edge: loop s %.6f (truth %.6f), ATE rms %.6f max %.6f (SE(3) graph, same [R t]: %.6f %.6f), "
          "largest |s_i - 1.5^(-i/15)| %.3e" % ((a["s"], 1.0 / W.DRIFT) + a["sim3"] + a["se3"] + (a["scale_gap"],)))
    r = run("exact")
    print("exact edge: loop s %.6f" % r["s"])
    for k, name in (("before", "drifted chain, nothing optimised"), ("se3", "graph_ref.optimize(%d), edge [R t]" % ITERATIONS),
                    ("sim3", "sgraph_ref.optimize(%d), edge (R, t, s)" % ITERATIONS)):
        print("ATE %-40s rms %.6f max %.6f" % (name, r[k][0], r[k][1]))
    print("scales " + " ".join("%.4f" % s for s in r["scales"]))
    print("largest |s_i - 1.5^(-i/15)| %.3e" % r["scale_gap"])
    print("corrected points: moved %d, left alone %d, refused %d" % r["stats"])
    print("WALK_REF = (%.6f, %.6f)    # sgraph_ref: ATE rms, max over the 16 centres" % r["sim3"])
    print("WALK_SE3 = (%.6f, %.6f)    # graph_ref with the same [R t]" % r["se3"])
    print("SCALE_GAP = %.3e           # largest |s_i - 1.5^(-i/15)|" % r["scale_gap"])


if __name__ == "__main__":
    main()
