#!/usr/bin/env python3
"""The closed walk of tests/cpp/sim3_selftest.cpp, run through the restatements alone (CPU): a generated 3-D scene, 16 keyframes
on a circle that returns to within 0.31 units of its start, the trajectory and the map drifted in scale by a known factor
(1.5 at the last keyframe). The first and the last pair are triangulated (map_ref), the loop's match list is joined with the
map (sim3_ref.associate) and aligned (sim3_ref.estimate), and the pose graph (graph_ref) is optimised twice: with the aligned
edge [R t], and with the unit-length edge a two-view verification hands over. Prints the error of the optimised end pose against
the scene's truth for both, the number tests/test_cpp_sim3.py doubles for its bound.

The script and the selftest share every formula of the scene (an integer generator, no library random numbers), so they build
the same frames up to the last bit of sin and cos.
Usage: tools/sim3_walk.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_FRAMES, N_POINTS, DRIFT, RADIUS, CLOSE = 16, 300, 1.5, 1.0, 0.95
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375


def u01(k):
    """The scene's generator: ((k * 2654435761 + 12345) mod 2^32) / 2^32."""
    return ((int(k) * 2654435761 + 12345) % (1 << 32)) / 4294967296.0


def camera(i):
    """World-to-camera [R | t] (4x4) of true keyframe i, and its centre."""
    th = i * (2.0 * np.pi * CLOSE) / (K_FRAMES - 1)
    c = np.array([RADIUS * np.sin(th), 0.1 * RADIUS * np.sin(2.0 * th), RADIUS * (np.cos(th) - 1.0)])
    a = np.radians(3.0) * np.sin(th)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ c
    return T, c


def scene():
    """(true poses, drifted poses, keypoints per frame (K, N, 2) float32, points)."""
    true = [camera(i) for i in range(K_FRAMES)]
    drifted, cd = [], true[0][1].copy()
    for i in range(K_FRAMES):
        if i:
            cd = cd + DRIFT ** (i / (K_FRAMES - 1.0)) * (true[i][1] - true[i - 1][1])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = true[i][0][:3, :3], -true[i][0][:3, :3] @ cd
        drifted.append(T)
    pts = np.zeros((N_POINTS, 3))
    for j in range(N_POINTS):
        u, v, z = 100.0 + 550.0 * u01(3 * j), 80.0 + 320.0 * u01(3 * j + 1), 4.0 + 8.0 * u01(3 * j + 2)
        pts[j] = [(u - CX) / FX * z, (v - CY) / FY * z, z]
    kp = np.zeros((K_FRAMES, N_POINTS, 2), np.float32)
    for i in range(K_FRAMES):
        Y = pts @ true[i][0][:3, :3].T + true[i][0][:3, 3]
        for j in range(N_POINTS):
            nx, ny = 0.6 * (u01(1000003 + 2 * (i * N_POINTS + j)) - 0.5), 0.6 * (u01(1000004 + 2 * (i * N_POINTS + j)) - 0.5)
            kp[i, j] = FX * Y[j, 0] / Y[j, 2] + CX + nx, FY * Y[j, 1] / Y[j, 2] + CY + ny
    return [t[0] for t in true], drifted, kp, pts


def loop_matches():
    """Keyframe L (query) against keyframe 0 (train): i <-> i, every seventh paired with its neighbour."""
    from aria_slam_amd._lib import MATCH_DTYPE
    m = np.zeros(N_POINTS, MATCH_DTYPE)
    m["query_idx"] = np.arange(N_POINTS)
    m["train_idx"] = [(j + 1) % N_POINTS if j % 7 == 3 else j for j in range(N_POINTS)]
    m["distance"] = 10.0
    return m


def end_error(X0, XL, T_true):
    """(rotation error in degrees, translation error) of the optimised transform keyframe L -> keyframe 0 against the truth."""
    from aria_slam_amd import pose_ref as P
    E = np.linalg.inv(X0) @ XL
    return P.rotation_error_deg(E[:3, :3], T_true[:3, :3]), float(np.linalg.norm(E[:3, 3] - T_true[:3, 3]))


def run():
    from aria_slam_amd import graph_ref as G
    from aria_slam_amd import map_ref as M
    from aria_slam_amd import sim3_ref as N
    from aria_slam_amd._lib import KP_DTYPE, MATCH_DTYPE
    true, drifted, kp, _pts = scene()
    L = K_FRAMES - 1
    frames = []
    for i in range(K_FRAMES):
        k = np.zeros(N_POINTS, KP_DTYPE)
        k["x"], k["y"], k["size"], k["response"] = kp[i, :, 0], kp[i, :, 1], 31.0, 1.0
        frames.append(k)
    ident = np.zeros(N_POINTS, MATCH_DTYPE)
    ident["query_idx"] = ident["train_idx"] = np.arange(N_POINTS)
    points = np.concatenate([M.triangulate_pair(frames[0], frames[1], ident, drifted[0], drifted[1], pair=0),
                             M.triangulate_pair(frames[L - 1], frames[L], ident, drifted[L - 1], drifted[L], pair=1)])
    loop = loop_matches()
    corr, _back = N.associate(points, 1, 0, 2, 1, drifted[L][:3].ravel(), drifted[0][:3].ravel(), frames[L], frames[0], loop,
                              kp_stride=N_POINTS)
    sim = N.estimate(corr, pair=L)
    T_true = true[0] @ np.linalg.inv(true[L])                       # camera L's coordinates -> camera 0's
    aligned = np.eye(4)
    aligned[:3, :3], aligned[:3, 3] = np.asarray(sim["R"], np.float64), np.asarray(sim["t"], np.float64)
    unit = T_true.copy()
    unit[:3, 3] = unit[:3, 3] / np.linalg.norm(unit[:3, 3])         # what recoverPose hands over: the direction, length 1
    out = {}
    for name, edge in (("aligned", aligned), ("unit", unit)):
        g = G.PoseGraphOptimizer()
        for i in range(K_FRAMES):                                   # vertices are camera-to-world; Z_ij = X_i^-1 X_j
            g.set_initial_pose(i, np.linalg.inv(drifted[i]))
            if i:
                g.add_odometry_edge(i - 1, i, drifted[i - 1] @ np.linalg.inv(drifted[i]))
        g.add_loop_edge(0, L, edge)                                 # X_0^-1 X_L: camera L's coordinates -> camera 0's
        g.optimize(20)
        out[name] = end_error(g.get_optimized_pose(0), g.get_optimized_pose(L), T_true)
    out["before"] = end_error(np.linalg.inv(drifted[0]), np.linalg.inv(drifted[L]), T_true)
    out["sim"] = dict(valid=sim["valid"], s=float(sim["s"]), n_corr=len(corr), n_inliers=sim["n_inliers"], rms_px=float(sim["rms_px"]),
                      t_len=float(np.linalg.norm(aligned[:3, 3])), t_true_len=float(np.linalg.norm(T_true[:3, 3])),
                      edge_t_err=float(np.linalg.norm(aligned[:3, 3] - T_true[:3, 3])), map_points=len(points))
    return out


def main():
    r = run()
    s = r["sim"]
    print("map points %d, correspondences %d, inliers %d, s %.6f (truth %.6f), rms %.3f px" %
          (s["map_points"], s["n_corr"], s["n_inliers"], s["s"], 1.0 / DRIFT, s["rms_px"]))
    print("loop edge: |t| %.6f, truth %.6f, |t - t_true| %.6f (the unit-length edge: 1)" % (s["t_len"], s["t_true_len"], s["edge_t_err"]))
    for k in ("before", "aligned", "unit"):
        print("end pose %-8s rotation %.5f deg, translation %.6f" % (k, r[k][0], r[k][1]))
    print("WALK_REF = (%.5f, %.6f)    # the restatement's end-pose error with the aligned edge: rotation (deg), translation" % r["aligned"])


if __name__ == "__main__":
    main()
