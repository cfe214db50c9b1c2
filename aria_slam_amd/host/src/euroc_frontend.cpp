// euroc_frontend <dataset_path> [max_features=2000] [--legacy-order] [--csv out.csv] [--loop] [--loop-verify reference]
//                [--devices N] [--shards K] [--batch B] [--decode-threads T] [--pose FILE] [--map FILE.ply] [--track-map FILE2] [--pnp-solver dlt|p3p] [--local-map K] [--local-radius PX] [--bundle FILE3] [--bundle-window N]
//                [--loop-bow V] [--loop-bow-top K] [--loop-bow-vocab FILE] [--loop-capacity N]
//                [--optimize FILE] [--fuse FILE] [--eval FILE] [--eval-align none|se3|sim3] [--rpe-delta N]
//                [--stereo BASELINE_M] [--stereo-out FILE] [--rectify] [--dense FILE] [--volume FILE.ply] [--voxel M] [--mesh FILE2.ply] [--plan FILE] [--render PREFIX] [--render-every N] [--alerts FILE] [--track-dense FILE2]
//
// The feature front-end of the reference's only end-to-end harness, src/euroc_eval.cpp:128-176, driven through the
// ports instead of cv::cuda::ORB / cv::cuda::DescriptorMatcher: for every image of an ASL/EuRoC sequence
//   extract ORB (2000 features by default, euroc_eval.cpp:88) -> kNN-2 + ratio 0.75 against the previous frame
// (:168-175) -> report; with --loop also the loop-closure candidate step of :103, 230-247 (every frame with >= 8 matches
// becomes a keyframe: detect against the HBM-resident database with LoopClosureDetector(200, 0.4, 50)'s parameters, then
// add). The later stages of that loop are flags of their own below (--pose, --map, --loop-verify, --optimize, --fuse); YOLO
// (it needs model weights) and the visualisation are out of scope.
//
// --devices N / --shards K: the sequence is cut into K contiguous shards (default K = N) with a one-frame halo
// (aria_hip/Shard.hpp); every shard gets its own host thread and its own extractor + matcher handles (PipelineFactory's
// HIP mode) on device (shard mod N), and the per-frame results are merged in frame order -- the reference's loop over a
// recorded sequence, spread over the GPUs of a node. No data crosses between shards. The loop-closure step consumes the
// merged stream in frame order on device 0 afterwards (it is a sequential scan over the sequence by nature), so --loop
// gives the same keyframes and loops for every K. K > N runs several logical shards on one device.
//
// --batch B (round 4): every shard runs the CHUNKED pipeline of aria_hip/BatchFrontEnd.hpp instead of one processFrame call
// per image -- T decode workers fill pinned buffers, the copy stream uploads chunk c + 1 while the compute stream extracts
// all B frames of chunk c in one batch pass and matches its B pairs in one launch (the kernels bench.py measures), results
// come back per chunk. Same per-frame results (hashes, keyframes, loops) as the frame-at-a-time run; the summary names
// decode, staging and kernel time apart. The loop-closure step then runs over the merged stream as in the sharded mode.
//
// --pose FILE: the pose stage of euroc_eval.cpp:178-201 on the frame-at-a-time path (one shard, no --batch): previous ->
// current by essential-matrix RANSAC + recoverPose on the device (FrontEndConfig::estimate_pose, EuRoC cam0 intrinsics);
// current_pose = current_pose * [R t] when n_pose_inliers > 10 (:191-206). FILE gets one TUM line per frame,
// "timestamp tx ty tz qx qy qz qw" of current_pose. Without the flag nothing of this runs and the output is unchanged.
// --map FILE.ply (needs --pose): the mapping step of euroc_eval.cpp:218-222, 291, 326 -- after every accepted pose update
// the previous -> current pair is triangulated on the device (aria_hip/HipMapper.hpp) with the previous and the updated
// current_pose as world-to-camera extrinsics and the previous image for colour; at the end filterOutliers, then the PLY
// export, and "map N points -> FILE" is printed. The composition current_pose * delta is the reference's and is not
// geometrically consistent after the first pair; the batch form with pose records is.
// --track-map FILE2 (needs --pose): the trajectory and a map of its own in one frame and one scale (aria_hip/MapTracker.hpp,
// DESIGN.md section 24). The first accepted pair is bootstrapped by the pose stage at unit baseline and triangulated; each
// later frame is placed by PnP on the device against the points of the previous pair; a frame for which PnP finds no pose, or
// one with n_inliers <= 10, falls back to the pose stage's delta; the new pair is triangulated with the two extrinsics.
// FILE2 gets one TUM line per frame (world-to-camera poses), and "track pnp A fallback B bootstrap C held D map N -> FILE2"
// is printed. --pose FILE, --map and the CSV are byte-identical with and without it. --pnp-solver dlt|p3p chooses the PnP
// step's minimal solver (default dlt; p3p places a frame against a planar map, where the DLT finds no pose).
// --local-map K [--local-radius PX] (needs --track-map; default 0 = off): every step first tries guided matching (aria_hip/
// HipProjectionMatcher.hpp) -- the landmarks of the last K triangulated pairs projected by the predicted
// pose, searched in a window of PX px at octave 0, PnP on the result -- and goes down the path above only when that places no
// pose. "track local L of the last K pairs, radius PX px" is printed after the track line. Without the flag nothing changes.
//
// --loop-bow V [--loop-bow-top K] [--loop-bow-vocab FILE] [--loop-capacity N] (needs --loop; default 0 = off): place recognition
// in front of the exact loop check (aria_hip/HipPlaceIndex.hpp, HipLoopDetector::setPlaceIndex). The loop step then runs over the
// merged stream as in the sharded mode. The vocabulary of V words is loaded from FILE when it exists; otherwise it is trained, in
// a pre-pass over that stream, on at most 256 of the frames that can be keyframes, sampled evenly, and written to FILE when one
// is named. The keyframe database holds N keyframes (default 500, the reference's), the index as many bags. One line
// "loop bow words V iterations I entries E queries Q candidates C" is printed (I = 0: loaded).
//
// --loop-verify reference (needs --loop): a loop candidate is accepted as LoopClosureDetector accepts it -- F-RANSAC on its
// ratio-0.7 list, then E-RANSAC + recoverPose on the F inliers with computeRelativePose's K (aria_hip/
// HipFundamentalEstimator.hpp, makeReferenceVerifier; LoopClosure.cpp:116-195) -- instead of by the list's length alone.
// The loop step then runs over the merged stream as in the sharded mode, keeping the keypoints of the keyframes the
// database holds. Keyframes are the default run's; the loops are a subset of its. Without the flag nothing changes.
//
// --loop-align sim3 [--loop-align-out FILE] (needs --loop, --loop-verify reference and --track-map; unsharded): after the
// reference verification has accepted a candidate, the landmarks the two keyframes own in the tracker's map are joined through
// the candidate's match list and aligned (aria_hip/HipSim3Aligner.hpp, makeSim3Verifier). A valid alignment with at least 20
// inliers (ORB-SLAM's constant, untuned) replaces the candidate's unit-length relative pose by [R t] in map units, which is
// what --optimize then hands the pose graph; otherwise the candidate stays as it was. s is reported, and used by --loop-correct. FILE gets one line
// per accepted loop: query id, match id, s, n_corr, n_inliers, rms_px, replaced (0 or 1); one line "loop align sim3
// candidates C replaced R" is printed. Off by default; without the flag every output is what it was, byte for byte.
//
// --loop-correct [--loop-correct-map FILE.ply] (needs --optimize and --loop-align sim3): the final optimisation runs the Sim(3)
// pose graph (aria_hip/HipSim3GraphOptimizer.hpp; include/aria_orb_hip.h, "Sim(3) pose-graph optimisation") instead of the SE(3)
// one, over the trajectory the map lives in: every frame is a vertex with the camera-to-world inverse (host, fp64) of its
// --track-map pose, consecutive frames are joined by their relative pose at s = 1, and every loop candidate whose alignment
// was accepted (replaced = 1) adds the edge match -> query with the aligner's (R, t, s) at 10x; a candidate that was not
// aligned adds nothing. After optimize(50) the tracker's map is corrected: the points of a pair move with the first frame whose
// MapTracker::anchorPair() is that pair. --optimize FILE then gets the corrected poses [R_new t_new] of that trajectory
// (camera-to-world, s dropped), FILE.ply the corrected map, and "loop correct edges E moved M left L refused R" is printed.
// Without the flag every output is what it was, byte for byte. On the synthetic flat-scene sequence no candidate reaches the
// aligner, so there the flag is run for its plumbing only; what it is for is tests/cpp/sgraph_selftest.cpp's closed walk.
//
// --bundle FILE3 [--bundle-window N] (needs --track-map): local bundle adjustment of the tracked trajectory, post hoc as
// --optimize is (aria_hip/HipBundleAdjuster.hpp; the reference names the step, README.md:1162, and has no code for it). The
// tracker's steps are recorded in a WindowBuilder; windows of N frames (default 10, at most 16) with stride N - 2 are adjusted
// in order with their first two poses fixed -- two fixed poses remove the monocular gauge, scale included -- and a window's
// refined poses and points seed the next. FILE3 gets one TUM line per frame and one trailing comment line per window with
// chi2_initial, chi2_final and rms_px.
// --optimize FILE (needs --pose, --loop and --loop-verify reference, so that accepted candidates carry relative_pose): the
// pose graph of euroc_eval.cpp through aria_hip/HipPoseGraphOptimizer.hpp -- setInitialPose(frame, current_pose) and
// addOdometryEdge(frame - 1, frame, delta) exactly where :211-215 adds them (after every accepted pose update; the first
// vertex added is the fixed one and an edge to a frame without a vertex is dropped, as in the reference), one
// addLoopEdge(query_id, match_id, relative_pose) per accepted loop candidate (:235), then the final optimize(50) and one
// TUM line per frame from getOptimizedPose (:282-288). DEVIATIONS: (1) the loop step of this driver runs post hoc over the
// merged stream, so the reference's optimize(10) after every loop and its reset of current_pose to the optimised pose
// (:237-238) are NOT reproduced; the odometry chain is the one --pose writes. (2) A frame without an accepted pose is no
// vertex; its line holds the optimised pose of the last vertex before it, as its --pose line holds current_pose (the
// reference's class would answer the identity for it). Without the flag nothing changes; --pose FILE and the CSV are
// byte-identical with and without it.
//
// --fuse FILE (needs --pose; the sequence needs mav0/imu0): the SensorFusion EKF of euroc_eval.cpp on the device (include/
// aria_orb_hip.h, "visual-inertial fusion"). Every frame first hands the filter the IMU samples between the previous image and
// this one (:139-142, the ranges of EuRoCReader::getNext), then, when its pose was accepted, addVisualPose(timestamp, R, t)
// with the RELATIVE R, t of recoverPose (unit-length t), which is what :209 passes -- not the accumulated current_pose. The
// whole track runs as one aria_fuse_run after the last frame; FILE gets one TUM line per frame of the fused position and
// orientation after that frame's events (the filter's initial state before the first accepted pose), and "fused N updates
// ..." is printed. Without the flag nothing changes; --pose FILE and the CSV are byte-identical with and without it.
//
// --eval FILE (needs --pose; the sequence needs ground truth, mav0/state_groundtruth_estimate0): the last step of
// euroc_eval.cpp on the device (include/aria_orb_hip.h, "trajectory evaluation"). Ground truth is sampled at every frame's
// timestamp (:247-252, EuRoCReader::getGroundTruth) and the --pose trajectory, plus the --optimize and --fuse trajectories when
// those flags are given, are scored against it by position in the trajectory, as :285-288 pairs them. FILE gets one line per
// trajectory, "name align n_poses n_used ate_raw rpe_raw align_valid scale ate_rmse ate_mean ate_max rpe_aligned sigma1 sigma2
// sigma3": the reference's computeATE / computeRPE (no alignment) and the figures after the alignment --eval-align chooses
// (default sim3: a chain of unit-length translations has no scale of its own); --rpe-delta N is computeRPE's delta (default
// 10). Frames the filter had not been initialised for take no part in the --fuse line. The reference's two-line "Trajectory
// Error" report (:303-305) is printed with its raw numbers, for the --optimize trajectory when there is one (the reference
// reports the optimised poses), else for --pose. Without the flag nothing changes and every other output is byte-identical.
//
// --stereo BASELINE_M [--stereo-out FILE] (frame-at-a-time path; the sequence needs a mav0/cam1 image of equal timestamp for
// every cam0 image, and the pairs must be RECTIFIED -- or --rectify given, see below): sparse stereo on the device (include/
// aria_orb_hip.h, "sparse stereo"; aria_hip/HipStereoMatcher.hpp). The right image of every frame is extracted by a second
// extractor and every left keypoint gets a depth. One line per frame, "timestamp matched median_depth", goes to FILE (to the
// standard output with the prefix "stereo " without --stereo-out). With --pose as well, the relative translation of every
// accepted pose (|t| = 1 from recoverPose) is multiplied by the metric scale recovered from the two frames' stereo
// observations when that is valid, before it is chained into current_pose, and the line gets two more columns, "scale_valid
// scale" (0 1 for a frame without an accepted pose). Without --stereo nothing of this runs and every output is byte-identical.
//
// --rectify (frame-at-a-time path; the sequence needs mav0/cam0/sensor.yaml, and mav0/cam1/sensor.yaml with --stereo): the
// distortion the reference parses and never applies (radial-tangential, or equidistant = fisheye = kb4) is removed on the device (include/aria_orb_hip.h, "rectification";
// aria_hip/HipRectifier.hpp). Without --stereo every cam0 image is undistorted before extraction (new K = cam0's K) and the
// pose and map stages take that K. With --stereo both images of a frame are rectified with the rotations built from the two
// T_BS, and the stereo, pose and map stages take the rectified K; a BASELINE_M of 0 then means the calibration's baseline. A
// missing sensor.yaml is an error message and exit status 1. Without the flag every output is byte-identical.
//
// --dense FILE (needs --stereo BASELINE_M, which brings cam1 and the baseline; composes with --rectify): dense stereo on the
// device (include/aria_orb_hip.h, "dense stereo"; aria_hip/HipDenseStereo.hpp) on the pair the sparse stage sees. FILE gets
// one line per frame, "timestamp valid_share median_depth": the share of the pixels with a positive disparity and the depth
// at index n / 2 of their ascending depths. Without the flag nothing of this runs and every output is byte-identical.
//
// --volume FILE.ply [--voxel M] (needs --pose, --stereo and --dense): dense depth fusion on the device (include/
// aria_orb_hip.h, "dense depth fusion"; aria_hip/HipTsdfVolume.hpp). Every frame's dense depth map is integrated, with the left
// image for gray, at the --pose chain's current_pose taken as world-to-camera extrinsics (as --map takes it), whose accepted
// relative translations carry the --stereo scale. A frame without an accepted pose, or without a valid scale, is left out. The
// volume has the default 256 x 256 x 128 voxels of M metres (default 0.05) and is centred on the first camera. At the end the
// surface points are written as PLY (the --map header and vertex format) and "volume <points> <observed voxels>" is printed.
// Without the flag nothing of this runs and every output is byte-identical.
//
// --mesh FILE2.ply (needs --volume): the mesh of the volume on the device (include/aria_orb_hip.h, "mesh of the volume"; aria_hip/
// HipVolumeMesher.hpp). After the volume is built and its points are written, its records are contoured by marching tetrahedra
// and FILE2 gets the triangle mesh as PLY: the --volume header and vertex lines plus "element face" / "property list uchar int
// vertex_indices". Exactly one line "mesh <vertices> <triangles>" is printed. Without the flag nothing of this runs and every
// output is byte-identical.
//
// --plan FILE (needs --volume): path planning on the device (include/aria_orb_hip.h, "path planning"; aria_hip/
// HipPathPlanner.hpp). After the volume is built its band [ny/2 - 8, ny/2 + 16) around the first camera's height is collapsed into
// the traversability grid of the x-z plane (up_axis 1, the stage's default radii and penalties, which nobody has tuned on a
// recording), and a path is planned from the cell under the first camera centre of the --pose chain to the cell under the last
// (the centre of a world-to-camera pose [R|t] is -R^T t). FILE gets one "x y z" line per path cell, the cell's centre at the
// middle of the band, and exactly one line "plan <status> <cost> <cells>" is printed (status 0 OK, 1 UNREACHABLE, 2 OUT_OF_GRID;
// FILE is then empty). Without the flag nothing of this runs and every output is byte-identical.
//
// --render PREFIX [--render-every N] (needs --volume): ray casting of the volume on the device (include/aria_orb_hip.h, "ray
// casting of the volume"; aria_hip/HipVolumeRenderer.hpp). After the volume is built it is cast at every N-th (default 10) of
// the poses a frame was integrated at, in batches of at most 64 views (one batch up to that), at the frame's size and the volume's intrinsics, with the stage's defaults
// (0.3 to 10 m, step = the voxel). Per view PREFIX_<frame>_depth.pgm (16-bit, millimetres, most significant byte first, 0 = no
// hit) and PREFIX_<frame>_shade.pgm (8-bit, the head-light shade) are written, <frame> being the frame's index in the
// sequence, and exactly one line "render <views> <hit pixels>" is printed. Without the flag nothing of this runs and every
// other output is byte-identical.
//
// --track-dense FILE2 (needs --volume): frame-to-model tracking on the device (include/aria_orb_hip.h, "frame-to-model tracking";
// aria_hip/DenseTracker.hpp). A DenseTracker with a volume of its own (the --volume geometry) takes every frame's dense depth
// map: it predicts the pose from the --pose chain's step, casts its volume there, tracks the depth map against that view, falls
// back to the prediction where the tracker reports valid = 0, and integrates the frame at the result. FILE2 gets one TUM line
// per frame, "track-dense tracked A lost B -> FILE2" is printed and the count of lost frames goes to stderr; with --eval the
// trajectory is scored as "track-dense". Without the flag nothing of this runs and every other output is byte-identical.
//
// --alerts FILE (needs --dense): obstacle alerts on the device (include/aria_orb_hip.h, "obstacle alerts"; aria_hip/
// HipObstacleAlerter.hpp). Every frame's dense depth map goes through a HipObstacleAlerter of the frame's size with the stage's
// defaults (the band is the lower three quarters of the image; nobody has tuned them on a recording), at the timestamp
// llround(seconds * 1e9) ns. This driver sets no object detector, so the sources are the three zones. The events are played
// through a RecordingAudioFeedback, and FILE gets one line per event: "timestamp_ns frame source class_id direction priority
// distance flags | call; call; ..." with the calls the event made on the port. "alerts <events> <frames>" is printed. Without the
// flag nothing of this runs and every output is byte-identical.
//
// Prints the progress line every 100 frames like the reference (:271-277) and a summary; --csv writes
// "frame,timestamp,keypoints,matches,hash,keyframe,loop_match_id,loop_score" per frame, hash = FNV-1a 64 over the frame's
// keypoint records, descriptor rows and match records (what the parity test compares with the oracle's).
#include <algorithm>
#include <array>
#include <cmath>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <fstream>
#include <iomanip>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "aria_hip/AslSequence.hpp"
#include "aria_hip/BatchFrontEnd.hpp"
#include "aria_hip/FrontEnd.hpp"
#include "aria_hip/HipFactory.hpp"
#include "aria_hip/HipFundamentalEstimator.hpp"
#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPlaceIndex.hpp"
#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipBundleAdjuster.hpp"
#include "aria_hip/HipSim3Aligner.hpp"
#include "aria_hip/MapTracker.hpp"
#include "aria_hip/HipObstacleAlerter.hpp"
#include "aria_hip/HipPathPlanner.hpp"
#include "aria_hip/HipVolumeMesher.hpp"
#include "aria_hip/HipVolumeRenderer.hpp"
#include "aria_hip/DenseTracker.hpp"
#include "aria_hip/HipPoseGraphOptimizer.hpp"
#include "aria_hip/HipSim3GraphOptimizer.hpp"
#include "aria_hip/HipDenseStereo.hpp"
#include "aria_hip/HipRectifier.hpp"
#include "aria_hip/HipSensorFusion.hpp"
#include "aria_hip/HipStereoMatcher.hpp"
#include "aria_hip/HipTrajectoryEvaluator.hpp"
#include "aria_hip/HipTsdfVolume.hpp"
#include "aria_hip/OrbHipExtractor.hpp"
#include "aria_hip/Shard.hpp"
#include "aria_orb_hip.h"

using namespace aria;

static std::uint64_t fnv1a(const void* p, std::size_t n, std::uint64_t h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (std::size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

namespace {
struct FrameRecord {
    std::size_t keypoints = 0, matches = 0;
    std::uint64_t hash = 0;
    bool is_keyframe = false;
    long long loop_match_id = -1;
    double loop_score = 0.0;
    std::unique_ptr<core::Frame> frame;      // kept only for the loop-closure step of a sharded / batched run, and only if it can be a keyframe
};

std::uint64_t frame_hash(const core::Frame& f, const std::vector<core::Match>& m) {
    std::uint64_t h = 14695981039346656037ull;
    h = fnv1a(f.keypoints.data(), f.keypoints.size() * sizeof(core::KeyPoint), h);
    h = fnv1a(f.descriptors.data(), f.numKeypoints() * 32, h);
    return fnv1a(m.data(), m.size() * sizeof(core::Match), h);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "Usage: %s <dataset_path> [max_features] [--legacy-order] [--csv file] [--loop] [--loop-verify reference] [--devices N] [--shards K] [--batch B] [--decode-threads T] [--pose file] [--map file.ply] [--track-map file] [--local-map K] [--local-radius PX] [--bundle file] [--bundle-window N] [--optimize file] [--loop-correct] [--loop-correct-map file.ply] [--fuse file] [--eval file] [--eval-align none|se3|sim3] [--rpe-delta N] [--stereo baseline_m] [--stereo-out file] [--rectify] [--dense file] [--volume file.ply] [--voxel m] [--mesh file2.ply] [--plan file] [--render prefix] [--render-every n] [--alerts file]\n"
                             "  --track-dense file2: frame-to-model tracking of the --dense depth maps against a volume of its own (needs --volume): one TUM line per frame\n"
                             "  --alerts file: obstacle alerts from the --dense depth maps (zones; needs --dense): one line per announced event\n"
                             "  --render prefix: the --volume map cast at every n-th integrated pose (--render-every n, default 10; needs --volume):\n"
                             "                   prefix_<frame>_depth.pgm (16-bit mm) and prefix_<frame>_shade.pgm per view\n"
                             "  --mesh file2.ply: the --volume map as a triangle mesh (watertight marching tetrahedra; needs --volume)\n"
                             "  --plan file: a path over the --volume map from the cell under the first camera of the --pose chain to the cell under the last\n"
                             "               (needs --volume): one x y z line per path cell\n"
                             "  --volume file.ply: dense depth fusion of the --dense depth maps along the --pose chain (needs --pose, --stereo, --dense): the surface\n"
                             "                     points of a TSDF volume centred on the first camera; --voxel m is the voxel edge (default 0.05)\n"
                             "  --dense file: dense stereo (census + SGM, 64 disparities) on the --stereo pairs: valid share and median depth, one line per frame\n"
                             "  --rectify: undistort cam0 (with --stereo: rectify cam0 and cam1) on the device from mav0/cam*/sensor.yaml; --stereo 0 then takes\n"
                             "             the calibration's baseline\n"
                             "  --stereo baseline_m: sparse stereo over mav0/cam1 (rectified pairs): a depth per keypoint, one line per frame; with --pose the\n"
                             "                       relative translations take the metric scale\n"
                             "  --eval file: ATE / RPE of the --pose (and --optimize, --fuse) trajectories against the sequence's ground truth (needs --pose)\n"
                             "  --fuse file: EKF visual-inertial fusion over imu0 and the --pose stage's relative poses (needs --pose), one TUM line per frame\n"
                             "  --pnp-solver dlt|p3p: the minimal solver of --track-map's PnP step (default dlt: the 6-point DLT, which places no frame on a\n"
                             "                        planar scene; p3p needs four map points and handles planes)\n"
                             "  --local-map K [--local-radius PX]: --track-map first places a frame by guided matching against the landmarks of the last K\n"
                             "                        pairs (projection by the predicted pose, window of PX px at octave 0, default 15), so a frame\n"
                             "                        after a blank one keeps the map's frame and scale (default 0: off)\n"
                             "  --loop-bow V [--loop-bow-top K] [--loop-bow-vocab file] [--loop-capacity N]: place recognition in front of the loop check (needs --loop):\n"
                             "                 a bag-of-words index of V words names the K (default 10) keyframes that are matched exactly; the vocabulary is\n"
                             "                 loaded from the file, or trained on at most 256 frames of the run and written there; N keyframes are kept (default 500)\n"
                             "  --bundle file: local bundle adjustment of the --track-map trajectory in windows of --bundle-window N frames (default 10, at most 16),\n"
                             "                 stride N - 2, the first two poses of a window fixed (needs --track-map)\n"
                             "  --optimize file: pose graph over the --pose chain and the verified loops (needs --pose, --loop, --loop-verify reference), final optimize(50);\n"
                             "                   the per-loop optimize(10) and reset of current_pose of the reference are not reproduced (the loop step is post hoc)\n"
                             "  --loop-correct [--loop-correct-map file.ply]: the final optimisation is the Sim(3) graph over the --track-map trajectory, loop edges\n"
                             "                   carry the accepted alignments' scale, and the tracker's map is corrected by each pair's anchor frame (needs --optimize\n"
                             "                   and --loop-align sim3); plumbing only on a sequence without loops\n", argv[0]);
        return -1;                                                        // euroc_eval.cpp:64-70
    }
    int max_features = 2000, devices = 1, shards = 0, batch = 0, decode_threads = 4;
    bool legacy = false, loop = false;
    std::string bundle_file;
    int bundle_window = 10;
    std::string pnp_solver_name = "dlt";
    int local_map = 0;
    double local_radius = 15.0;
    int loop_bow = 0, loop_bow_top = 10, loop_capacity = 500;
    bool loop_bow_given = false;
    std::string loop_bow_vocab;
    std::string loop_align, loop_align_out, loop_correct_map;
    bool loop_correct = false;
    std::string csv, pose_file, map_file, track_file, loop_verify, optimize_file, fuse_file, eval_file, eval_align = "sim3";
    int rpe_delta = 10;
    double stereo_baseline = 0.0;
    bool stereo = false, rectify = false;
    std::string stereo_file, dense_file, volume_file, mesh_file, plan_file, alerts_file, render_prefix, dense_track_file;
    int render_every = 10;
    double voxel = 0.05;
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--legacy-order")) legacy = true;
        else if (!std::strcmp(argv[i], "--loop")) loop = true;
        else if (!std::strcmp(argv[i], "--csv") && i + 1 < argc) csv = argv[++i];
        else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) devices = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--shards") && i + 1 < argc) shards = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--batch") && i + 1 < argc) batch = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--decode-threads") && i + 1 < argc) decode_threads = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--pose") && i + 1 < argc) pose_file = argv[++i];
        else if (!std::strcmp(argv[i], "--map") && i + 1 < argc) map_file = argv[++i];
        else if (!std::strcmp(argv[i], "--track-map") && i + 1 < argc) track_file = argv[++i];
        else if (!std::strcmp(argv[i], "--pnp-solver") && i + 1 < argc) pnp_solver_name = argv[++i];
        else if (!std::strcmp(argv[i], "--local-map") && i + 1 < argc) local_map = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--local-radius") && i + 1 < argc) local_radius = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--bundle") && i + 1 < argc) bundle_file = argv[++i];
        else if (!std::strcmp(argv[i], "--bundle-window") && i + 1 < argc) bundle_window = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--loop-verify") && i + 1 < argc) loop_verify = argv[++i];
        else if (!std::strcmp(argv[i], "--loop-bow") && i + 1 < argc) { loop_bow = std::atoi(argv[++i]); loop_bow_given = true; }
        else if (!std::strcmp(argv[i], "--loop-bow-top") && i + 1 < argc) { loop_bow_top = std::atoi(argv[++i]); loop_bow_given = true; }
        else if (!std::strcmp(argv[i], "--loop-bow-vocab") && i + 1 < argc) { loop_bow_vocab = argv[++i]; loop_bow_given = true; }
        else if (!std::strcmp(argv[i], "--loop-capacity") && i + 1 < argc) loop_capacity = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--loop-align") && i + 1 < argc) loop_align = argv[++i];
        else if (!std::strcmp(argv[i], "--loop-align-out") && i + 1 < argc) loop_align_out = argv[++i];
        else if (!std::strcmp(argv[i], "--loop-correct")) loop_correct = true;
        else if (!std::strcmp(argv[i], "--loop-correct-map") && i + 1 < argc) loop_correct_map = argv[++i];
        else if (!std::strcmp(argv[i], "--optimize") && i + 1 < argc) optimize_file = argv[++i];
        else if (!std::strcmp(argv[i], "--fuse") && i + 1 < argc) fuse_file = argv[++i];
        else if (!std::strcmp(argv[i], "--eval") && i + 1 < argc) eval_file = argv[++i];
        else if (!std::strcmp(argv[i], "--eval-align") && i + 1 < argc) eval_align = argv[++i];
        else if (!std::strcmp(argv[i], "--rpe-delta") && i + 1 < argc) rpe_delta = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--stereo") && i + 1 < argc) { stereo = true; stereo_baseline = std::atof(argv[++i]); }
        else if (!std::strcmp(argv[i], "--stereo-out") && i + 1 < argc) stereo_file = argv[++i];
        else if (!std::strcmp(argv[i], "--rectify")) rectify = true;
        else if (!std::strcmp(argv[i], "--dense") && i + 1 < argc) dense_file = argv[++i];
        else if (!std::strcmp(argv[i], "--volume") && i + 1 < argc) volume_file = argv[++i];
        else if (!std::strcmp(argv[i], "--mesh") && i + 1 < argc) mesh_file = argv[++i];
        else if (!std::strcmp(argv[i], "--voxel") && i + 1 < argc) voxel = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--plan") && i + 1 < argc) plan_file = argv[++i];
        else if (!std::strcmp(argv[i], "--alerts") && i + 1 < argc) alerts_file = argv[++i];
        else if (!std::strcmp(argv[i], "--render") && i + 1 < argc) render_prefix = argv[++i];
        else if (!std::strcmp(argv[i], "--track-dense") && i + 1 < argc) dense_track_file = argv[++i];
        else if (!std::strcmp(argv[i], "--render-every") && i + 1 < argc) render_every = std::atoi(argv[++i]);
        else max_features = std::atoi(argv[i]);
    }
    if (devices < 1) devices = 1;
    if (shards < 1) shards = devices;
    if (batch < 0) batch = 0;
    if (decode_threads < 1) decode_threads = 1;
    if (!loop_verify.empty() && (loop_verify != "reference" || !loop)) {
        std::fprintf(stderr, "--loop-verify reference needs --loop (the only verification mode is 'reference')\n");
        return -1;
    }
    const bool verify_reference = !loop_verify.empty();
    if ((!loop_align.empty() || !loop_align_out.empty()) && (loop_align != "sim3" || !verify_reference || track_file.empty() || shards > 1 || batch > 0)) {
        std::fprintf(stderr, "--loop-align sim3 [--loop-align-out FILE] needs --loop, --loop-verify reference and --track-map, unsharded "
                             "(the only alignment mode is 'sim3')\n");
        return 1;
    }
    const bool align_sim3 = !loop_align.empty();
    if (loop_bow_given && (!loop || loop_bow < 1 || loop_bow > 4096 || loop_bow_top < 1 || loop_bow_top > 32)) {
        std::fprintf(stderr, "--loop-bow V (1..4096), --loop-bow-top K (1..32) and --loop-bow-vocab need --loop\n");
        return 1;
    }
    if (loop_capacity < 1 || (loop_capacity != 500 && !loop)) {
        std::fprintf(stderr, "--loop-capacity N >= 1 needs --loop\n");
        return 1;
    }
    if (!optimize_file.empty() && (pose_file.empty() || !verify_reference)) {
        std::fprintf(stderr, "--optimize needs --pose, --loop and --loop-verify reference (loop edges carry the verified relative pose)\n");
        return -1;
    }
    if ((loop_correct || !loop_correct_map.empty()) && (!loop_correct || optimize_file.empty() || !align_sim3)) {
        std::fprintf(stderr, "--loop-correct [--loop-correct-map FILE.ply] needs --optimize and --loop-align sim3 (the map it corrects is --track-map's)\n");
        return 1;
    }
    if (!fuse_file.empty() && pose_file.empty()) {
        std::fprintf(stderr, "--fuse needs --pose (the filter is updated with the pose stage's relative poses)\n");
        return 1;
    }
    const int eval_mode = eval_align == "none" ? ARIA_EVAL_ALIGN_NONE : eval_align == "se3" ? ARIA_EVAL_ALIGN_SE3
                          : eval_align == "sim3" ? ARIA_EVAL_ALIGN_SIM3 : -1;
    if (!eval_file.empty() && (pose_file.empty() || eval_mode < 0 || rpe_delta < 1)) {
        std::fprintf(stderr, "--eval needs --pose, --eval-align none|se3|sim3 and --rpe-delta >= 1\n");
        return 1;
    }
    const int pnp_solver = pnp_solver_name == "dlt" ? ARIA_PNP_SOLVER_DLT6 : pnp_solver_name == "p3p" ? ARIA_PNP_SOLVER_P3P : -1;
    if (pnp_solver < 0) {
        std::fprintf(stderr, "--pnp-solver takes dlt or p3p\n");
        return 1;
    }
    if (!track_file.empty() && pose_file.empty()) {
        std::fprintf(stderr, "--track-map needs --pose (it bootstraps from, and falls back to, the pose stage)\n");
        return 1;
    }
    if (local_map < 0 || (local_map > 0 && track_file.empty()) || !(local_radius >= 0.0 && local_radius <= 1024.0)) {
        std::fprintf(stderr, "--local-map K >= 0 needs --track-map; --local-radius 0..1024\n");
        return 1;
    }
    if (!bundle_file.empty() && (track_file.empty() || bundle_window < 3 || bundle_window > ARIA_BA_MAX_POSES)) {
        std::fprintf(stderr, "--bundle needs --track-map and --bundle-window 3..16\n");
        return 1;
    }
    if (!map_file.empty() && pose_file.empty()) {
        std::fprintf(stderr, "--map needs --pose (it triangulates along the estimated trajectory)\n");
        return -1;
    }
    if (!pose_file.empty() && (batch > 0 || devices > 1 || shards > 1)) {
        std::fprintf(stderr, "--pose runs on the frame-at-a-time path only (no --batch, --devices, --shards)\n");
        return -1;
    }
    if ((stereo || !stereo_file.empty()) && (!stereo || !(stereo_baseline > 0 || (rectify && stereo_baseline == 0)) || batch > 0 || devices > 1 || shards > 1)) {
        std::fprintf(stderr, "--stereo needs a baseline in metres > 0 (or 0 with --rectify: the calibration's) and runs on the frame-at-a-time path only (no --batch, --devices, --shards); "
                             "--stereo-out needs --stereo\n");
        return 1;
    }
    if (!dense_file.empty() && !stereo) {
        std::fprintf(stderr, "--dense needs --stereo baseline_m (cam1 and the baseline)\n");
        return 1;
    }
    if (!volume_file.empty() && (pose_file.empty() || !stereo || dense_file.empty() || !(voxel > 0))) {
        std::fprintf(stderr, "--volume needs --pose (the trajectory), --stereo baseline_m (its metric scale), --dense file (the depth maps) and --voxel > 0\n");
        return 1;
    }
    if (!mesh_file.empty() && volume_file.empty()) {
        std::fprintf(stderr, "--mesh needs --volume file.ply (the map it contours)\n");
        return 1;
    }
    if (!plan_file.empty() && volume_file.empty()) {
        std::fprintf(stderr, "--plan needs --volume file.ply (the map it plans over)\n");
        return 1;
    }
    if (!render_prefix.empty() && (volume_file.empty() || render_every < 1)) {
        std::fprintf(stderr, "--render needs --volume file.ply (the map it casts) and --render-every >= 1\n");
        return 1;
    }
    if (!dense_track_file.empty() && volume_file.empty()) {
        std::fprintf(stderr, "--track-dense needs --volume file.ply (the geometry of the map it tracks against)\n");
        return 1;
    }
    if (!alerts_file.empty() && dense_file.empty()) {
        std::fprintf(stderr, "--alerts needs --dense file (the depth maps it measures)\n");
        return 1;
    }
    if (rectify && (batch > 0 || devices > 1 || shards > 1)) {
        std::fprintf(stderr, "--rectify runs on the frame-at-a-time path only (no --batch, --devices, --shards)\n");
        return 1;
    }
    {
        // --devices names HIP ordinals 0 .. N-1: refuse up front what the machine does not have (FactoryConfig::cuda_device,
        // include/factory/PipelineFactory.hpp:24, is taken on trust by the reference)
        int ndev = 0;
        const int rc = aria_device_count(&ndev);
        if (rc != ARIA_OK || ndev < devices) {
            std::fprintf(stderr, "--devices %d: %d HIP device%s present%s%s\n", devices, ndev, ndev == 1 ? "" : "s",
                         rc != ARIA_OK ? ": " : "", rc != ARIA_OK ? aria_status_string(rc) : "");
            return -1;
        }
    }
    io::AslSequence seq;
    if (!seq.load(argv[1])) {
        std::fprintf(stderr, "Failed to load dataset from %s\n", argv[1]);
        return -1;                                                        // euroc_eval.cpp:75-78
    }
    std::printf("Loaded: %zu images\n", seq.size());
    const std::size_t N = seq.size();
    if (!eval_file.empty() && !seq.hasGroundTruth()) {
        std::fprintf(stderr, "--eval: the sequence has no mav0/state_groundtruth_estimate0/data.csv with 17-field rows\n");
        return 1;
    }
    if (stereo && !seq.hasStereo()) {
        std::fprintf(stderr, "--stereo: the sequence has no mav0/cam1 image of equal timestamp for every cam0 image\n");
        return 1;
    }
    if (rectify) {
        for (int c = 0; c < (stereo ? 2 : 1); c++) {
            if (!seq.hasCalibration(c)) {
                std::fprintf(stderr, "--rectify: the sequence has no mav0/cam%d/sensor.yaml with intrinsics\n", c);
                return 1;
            }
            const std::string& model = seq.calibration(c).distortion_model;
            if (seq.calibration(c).rectModel() < 0) {
                std::fprintf(stderr, "--rectify: cam%d's distortion model '%s' is neither radial-tangential nor equidistant (fisheye, kb4)\n", c,
                             model.c_str());
                return 1;
            }
        }
        if (stereo && seq.calibration(0).rectModel() != seq.calibration(1).rectModel()) {
            std::fprintf(stderr, "--rectify: cam0's distortion model '%s' and cam1's '%s' differ: the cameras of a rig share one model\n",
                         seq.calibration(0).distortion_model.c_str(), seq.calibration(1).distortion_model.c_str());
            return 1;
        }
    }
    double stereo_baseline_used = stereo_baseline;
    struct StereoLine { int matched = 0; float median_depth = 0.0f; int scale_valid = 0; double scale = 1.0; };
    std::vector<StereoLine> stereo_lines(stereo ? N : 0);
    struct DenseLine { double valid_share = 0.0; float median_depth = 0.0f; };
    std::vector<DenseLine> dense_lines(dense_file.empty() ? 0 : N);
    std::vector<aria_fuse_state> fused_states;                             // --eval: what --fuse and --optimize leave
    std::vector<double> optimized_xyz;
    if ((std::size_t)shards > N && N > 0) shards = (int)N;

    std::vector<FrameRecord> rec(N);
    std::vector<std::string> errors((size_t)shards);
    std::atomic<std::size_t> done{0};
    int w = 0, h = 0;
    const bool sharded = shards > 1;
    // the loop step over the merged stream, after the shards (--loop-verify: it needs the keyframes' keypoints)
    const bool posthoc_loop = loop && (sharded || batch > 0 || verify_reference || loop_bow > 0 || loop_capacity != 500);
    std::vector<pipeline::BatchStats> bstats((size_t)shards);
    // --pose: current_pose per frame (4x4 row-major), chained as euroc_eval.cpp:202-206 does
    std::vector<std::array<double, 16>> traj(pose_file.empty() ? 0 : N);
    long long n_pose_updates = 0;
    // --fuse: the visual record of every frame (euroc_eval.cpp:209), filled where the pose is accepted
    std::vector<aria_fuse_visual> fuse_visual(fuse_file.empty() ? 0 : N);
    std::size_t map_points = 0;
    // --track-map: world-to-camera pose per frame, and how each step was made (TrackStep::Source)
    std::vector<std::array<double, 16>> track_traj(track_file.empty() ? 0 : N);
    long long track_steps[5] = {0, 0, 0, 0, 0};   // indexed by TrackStep::Source
    std::size_t track_points = 0;
    // --loop-align sim3: the anchor pair of every tracked frame, and the tracker (its map) kept for the loop step
    std::vector<int> track_anchor(align_sim3 ? N : 0, -1);
    std::unique_ptr<adapters::hip::MapTracker> kept_tracker;
    // --loop-correct: the Sim(3) loop edges, from = the matched keyframe (keyframe 2 of the alignment), to = the query (keyframe 1)
    struct CorrectEdge { int from, to; adapters::hip::GraphPose Z; double s; };
    std::vector<CorrectEdge> correct_edges;
    adapters::hip::PoseIntrinsics track_K;
    // --bundle: what the tracker did, step by step, and the sequence frame its first frame is
    adapters::hip::WindowBuilder bundle_builder;
    adapters::hip::PoseIntrinsics bundle_K;
    long long bundle_first = -1;
    long long volume_points = 0, volume_observed = 0;   // --volume
    long long mesh_vertices = 0, mesh_triangles = 0;    // --mesh
    long long alert_events = 0, alert_frames = 0;       // --alerts
    std::vector<std::string> alert_lines;
    long long render_views = 0, render_hits = 0;        // --render
    std::vector<std::array<double, 16>> dense_traj(dense_track_file.empty() ? 0 : N);   // --track-dense
    long long dense_tracked = 0, dense_lost = 0;
    aria_nav_record plan_record{ARIA_NAV_INF, 0, 0, ARIA_NAV_OUT_OF_GRID};   // --plan: a sequence without frames has no start
    // --optimize: the reference's PoseGraphOptimizer over the device (euroc_eval.cpp:211-215, 235, 282-288)
    std::unique_ptr<adapters::hip::HipPoseGraphOptimizer> graph;
    if (!optimize_file.empty()) graph = std::make_unique<adapters::hip::HipPoseGraphOptimizer>();
    std::vector<long long> last_vertex(graph ? N : 0, -1);                 // per frame: the last frame at or before it that is a vertex
    auto graphPose = [](const std::array<double, 16>& T) {
        adapters::hip::GraphPose m = adapters::hip::GraphPose::Identity();
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) m(a, b) = T[(size_t)(a * 4 + b)];
        return m;
    };
    const auto t0 = std::chrono::steady_clock::now();

    // one shard = one FrontEnd (its own extractor + matcher handles on its device) over frames [first, hi)
    auto run_shard = [&](int s) {
        try {
            const pipeline::ShardPlan sp = pipeline::shardPlan(N, s, shards);
            if (batch > 0) {
                pipeline::BatchFrontEndConfig bc;
                bc.hip_device = s % devices;
                bc.max_features = max_features;
                bc.chunk = batch;
                bc.decode_threads = decode_threads;
                bc.legacy_order = legacy;
                pipeline::BatchFrontEnd bfe(bc);
                bfe.run(seq, sp.first, sp.lo, sp.hi, [&](std::size_t i, const core::Frame& f, const std::vector<core::Match>& m) {
                    FrameRecord& o = rec[i];
                    o.keypoints = f.numKeypoints();
                    o.matches = m.size();
                    o.hash = frame_hash(f, m);
                    // only frames that can become keyframes are kept for the loop step (>= keyframe_min_matches matches,
                    // euroc_eval.cpp:179): a long sequence does not hold a copy of every frame until the end
                    if (posthoc_loop && (int)m.size() >= pipeline::FrontEndConfig{}.keyframe_min_matches) o.frame = std::make_unique<core::Frame>(f);
                    ++done;
                });
                bstats[(size_t)s] = bfe.stats();
                if (s == 0) { w = bfe.width(); h = bfe.height(); }
                return;
            }
            factory::HipFactoryConfig fc;                                 // PipelineFactory's HIP mode (aria_hip/HipFactory.hpp)
            fc.hip_device = s % devices;
            fc.max_features = max_features;
            fc.frontend.legacy_order = legacy;
            fc.enable_loop_closure = loop && !posthoc_loop;               // LoopClosureDetector(200, 0.4, 50), euroc_eval.cpp:103
            fc.frontend.estimate_pose = !pose_file.empty();
            std::vector<std::uint8_t> gray, warped;
            int fw = 0, fh = 0;
            // --rectify: the maps are built before the first frame; every later stage sees the new K
            std::unique_ptr<adapters::hip::HipRectifier> rectifier;
            adapters::hip::PoseIntrinsics new_K{};
            if (rectify) {
                adapters::hip::RectifierConfig rc;
                rc.n_cameras = stereo ? 2 : 1;
                rc.model = seq.calibration(0).rectModel();
                rc.device = fc.hip_device;
                for (int c = 0; c < rc.n_cameras; c++) {
                    const io::AslCalibration& cal = seq.calibration(c);
                    rc.cam[c].K = adapters::hip::PoseIntrinsics{cal.intrinsics[0], cal.intrinsics[1], cal.intrinsics[2], cal.intrinsics[3]};
                    for (int k = 0; k < 5; k++) rc.cam[c].dist[k] = cal.distortion[k];
                    for (int k = 0; k < 16; k++) rc.cam[c].T_BS[k] = cal.T_BS[k];
                }
                rc.src_width = seq.calibration(0).width;
                rc.src_height = seq.calibration(0).height;
                if (rc.src_width <= 0 || rc.src_height <= 0) seq.read(sp.first, gray, rc.src_width, rc.src_height);   // no resolution: key
                rectifier = std::make_unique<adapters::hip::HipRectifier>(rc);
                new_K = rectifier->newK();
                fc.frontend.pose_intrinsics = new_K;
                if (stereo && stereo_baseline == 0) stereo_baseline_used = rectifier->baseline();
            }
            auto warp = [&](int cam, std::vector<std::uint8_t>& img, int iw, int ih) {
                if (!rectifier) return;
                if (iw != rectifier->config().src_width || ih != rectifier->config().src_height)
                    throw std::runtime_error("--rectify: an image is not of the calibration's resolution");
                rectifier->remap(cam, img.data(), warped);
                img.swap(warped);
            };
            std::unique_ptr<pipeline::FrontEnd> fe = factory::createHip(fc);
            auto t_last = std::chrono::steady_clock::now();
            std::array<double, 16> current_pose = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            std::unique_ptr<adapters::hip::HipMapper> mapper;           // --map
            std::vector<std::uint8_t> prev_gray;
            int pw = 0, ph = 0;
            if (!map_file.empty()) {
                adapters::hip::MapperConfig mc;
                mc.device = fc.hip_device;
                if (rectifier) mc.K = new_K;
                mapper = std::make_unique<adapters::hip::HipMapper>(mc);
            }
            std::unique_ptr<adapters::hip::MapTracker> tracker;         // --track-map
            if (!track_file.empty()) {
                adapters::hip::MapperConfig mc;
                mc.device = fc.hip_device;
                if (rectifier) mc.K = new_K;
                tracker = std::make_unique<adapters::hip::MapTracker>(mc, 10, 1024, pnp_solver);
                track_K = mc.K;
                if (local_map > 0) tracker->setLocalMap(local_map, (float)local_radius);
                if (!bundle_file.empty()) {
                    tracker->setWindowBuilder(&bundle_builder);
                    bundle_K = mc.K;
                }
            }
            // --stereo: the right image has an extractor of its own; the observations of the previous frame stay for the scale
            std::unique_ptr<adapters::hip::OrbHipExtractor> right_extractor;
            std::unique_ptr<adapters::hip::HipStereoMatcher> stereo_matcher;
            adapters::hip::StereoObservations stereo_cur, stereo_prev;
            std::vector<std::uint8_t> right_gray;
            core::Frame right_frame;
            std::unique_ptr<adapters::hip::HipDenseStereo> dense_stereo;   // --dense: made at the first pair, for its size
            std::unique_ptr<adapters::hip::HipTsdfVolume> volume;          // --volume: centred on the first camera, the world origin
            std::unique_ptr<adapters::hip::DenseTracker> dense_tracker;    // --track-dense: the same geometry, its own volume
            adapters::hip::DenseDepth dense_map;
            std::vector<std::pair<std::size_t, std::array<double, 12>>> integrated;   // --render: frame index and [R|t] of each integration
            int render_w = 0, render_h = 0;
            adapters::hip::RecordingAudioFeedback alert_audio;             // --alerts: made at the first pair, for its size
            std::unique_ptr<adapters::hip::HipObstacleAlerter> alerter;
            if (!volume_file.empty()) {
                adapters::hip::TsdfVolumeConfig vc;
                if (rectifier) vc.K = new_K;
                vc.voxel = (float)voxel;
                vc.trunc = 4.0f * vc.voxel;
                vc.device = fc.hip_device;
                vc.centreOn(0.0f, 0.0f, 0.0f);
                volume = std::make_unique<adapters::hip::HipTsdfVolume>(vc);
                if (!dense_track_file.empty()) dense_tracker = std::make_unique<adapters::hip::DenseTracker>(vc);
            }
            if (stereo) {
                adapters::hip::StereoConfig sc;
                sc.baseline = stereo_baseline_used;
                if (rectifier) sc.K = new_K;
                sc.device = fc.hip_device;
                right_extractor = std::make_unique<adapters::hip::OrbHipExtractor>(max_features, nullptr, fc.hip_device);
                stereo_matcher = std::make_unique<adapters::hip::HipStereoMatcher>(sc);
            }
            for (std::size_t i = sp.first; i < sp.hi; i++) {
                seq.read(i, gray, fw, fh);
                warp(0, gray, fw, fh);
                const pipeline::FrontEndResult& r = fe->processFrame(gray.data(), fw, fh, seq.at(i).timestamp);
                if (i < sp.lo) continue;                                   // the halo frame only provides the previous descriptors
                if (stereo) {
                    int rw = 0, rh = 0;
                    seq.readRight(i, right_gray, rw, rh);
                    if (rw != fw || rh != fh) throw std::runtime_error("--stereo: cam1 image size differs from cam0's at " + seq.at(i).path);
                    warp(1, right_gray, rw, rh);
                    right_extractor->extract(right_gray.data(), rw, rh, right_frame);
                    std::swap(stereo_prev, stereo_cur);
                    stereo_cur = stereo_matcher->match(gray.data(), right_gray.data(), fw, fh, *r.frame, right_frame);
                    stereo_lines[i].matched = (int)stereo_cur.matches.size();
                    stereo_lines[i].median_depth = stereo_cur.medianDepth();
                    if (!dense_file.empty()) {
                        if (!dense_stereo) {
                            adapters::hip::DenseStereoConfig dc;
                            dc.baseline = stereo_baseline_used;
                            if (rectifier) dc.K = new_K;
                            dc.device = fc.hip_device;
                            dc.max_width = fw;
                            dc.max_height = fh;
                            dense_stereo = std::make_unique<adapters::hip::HipDenseStereo>(dc);
                        }
                        adapters::hip::DenseDepth dm = dense_stereo->compute(gray.data(), right_gray.data(), fw, fh);
                        dense_lines[i].valid_share = dm.validShare();
                        dense_lines[i].median_depth = dm.medianDepth();
                        if (!alerts_file.empty()) {
                            if (!alerter) {
                                adapters::hip::ObstacleAlerterConfig ac;
                                ac.width = fw;
                                ac.height = fh;
                                ac.device = fc.hip_device;
                                alerter = std::make_unique<adapters::hip::HipObstacleAlerter>(ac, &alert_audio);
                            }
                            const long long t_ns = std::llround(seq.at(i).timestamp * 1e9);
                            std::size_t call = 0;                          // the frame's calls on the port, in the events' order
                            for (const aria_alert_event& e : alerter->process(dm.depth.data(), {}, t_ns)) {
                                char head[160];
                                std::snprintf(head, sizeof(head), "%lld %zu %d %d %d %d %.9g %d |", t_ns, i, e.source, e.class_id, e.direction,
                                              e.priority, (double)e.distance, e.flags);
                                std::string line = head;
                                const std::size_t n_calls = 1 + ((e.flags & ARIA_ALERT_BEEP) ? 1 : 0) + ((e.flags & ARIA_ALERT_CRITICAL_ALERT) ? 1 : 0);
                                for (std::size_t k = 0; k < n_calls && call < alert_audio.log.size(); k++) line += (k ? "; " : " ") + alert_audio.log[call++];
                                alert_lines.push_back(line);
                                alert_events++;
                            }
                            alert_audio.log.clear();
                            alert_frames++;
                        }
                        if (volume) dense_map = std::move(dm);
                    }
                }
                if (!traj.empty()) {
                    std::array<double, 16> chain_step{};                   // --track-dense: this frame's step of the chain, if any
                    bool stepped = false;
                    if (r.pose && r.pose->n_pose_inliers > 10) {           // euroc_eval.cpp:191
                        std::array<double, 16> d = adapters::hip::poseMatrix(*r.pose);
                        const std::array<double, 16> c = current_pose;
                        if (stereo && r.previous) {                        // view 1 = previous frame: the query side in the legacy order
                            const bool q1 = fc.frontend.legacy_order;
                            const aria_stereo_scale sc = stereo_matcher->scale(*r.pose, r.matches, q1, q1 ? stereo_prev.obs : stereo_cur.obs,
                                                                               q1 ? stereo_cur.obs : stereo_prev.obs);
                            stereo_lines[i].scale_valid = sc.valid;
                            stereo_lines[i].scale = sc.scale;
                            if (sc.valid)
                                for (int a = 0; a < 3; a++) d[(size_t)(a * 4 + 3)] *= sc.scale;
                        }
                        for (int a = 0; a < 4; a++)
                            for (int b = 0; b < 4; b++) {
                                double v = 0.0;
                                for (int k = 0; k < 4; k++) v += c[(size_t)(a * 4 + k)] * d[(size_t)(k * 4 + b)];
                                current_pose[(size_t)(a * 4 + b)] = v;     // current_pose = current_pose * delta (:206)
                            }
                        n_pose_updates++;
                        chain_step = d;
                        stepped = true;
                        if (!fuse_visual.empty()) {                        // euroc_eval.cpp:209: the relative R, t
                            aria_fuse_visual& v = fuse_visual[i];
                            for (int a = 0; a < 3; a++) {
                                for (int b = 0; b < 3; b++) v.R[a * 3 + b] = d[(size_t)(a * 4 + b)];
                                v.p[a] = d[(size_t)(a * 4 + 3)];
                            }
                            v.accept = 1;
                        }
                        if (graph) {                                       // euroc_eval.cpp:211-215
                            graph->setInitialPose((int)i, graphPose(current_pose));
                            if (i > 0) graph->addOdometryEdge((int)i - 1, (int)i, graphPose(d));
                            last_vertex[i] = (long long)i;
                        }
                        // --volume: this frame's depth map at the updated pose, when the translation carries a metric scale
                        if (volume && stereo_lines[i].scale_valid &&
                            volume->integrate(dense_map.depth.data(), fw, fh, current_pose.data(), gray.data()) && !render_prefix.empty()) {
                            std::array<double, 12> e;
                            std::copy(current_pose.begin(), current_pose.begin() + 12, e.begin());
                            integrated.emplace_back(i, e);
                            render_w = fw; render_h = fh;
                        }
                        if (mapper && r.previous)                          // euroc_eval.cpp:218-222: view 1 = previous frame
                            mapper->triangulateExtrinsics(*r.previous, *r.frame, r.matches, c.data(), current_pose.data(),
                                                          prev_gray.data(), pw, ph, fc.frontend.legacy_order);
                    }
                    traj[i] = current_pose;
                    if (dense_tracker) {
                        dense_tracker->step(dense_map.depth.data(), fw, fh, stepped ? chain_step.data() : nullptr, gray.data());
                        dense_traj[i] = dense_tracker->pose();
                    }
                    if (graph && last_vertex[i] < 0 && i > 0) last_vertex[i] = last_vertex[i - 1];
                }
                if (tracker) {                                             // view 1 = previous frame: the query side in the legacy order
                    if (r.previous && bundle_first < 0) bundle_first = (long long)i - 1;
                    if (r.previous) track_steps[tracker->track(*r.previous, *r.frame, r.matches, fc.frontend.legacy_order, r.pose).source]++;
                    track_traj[i] = tracker->pose();
                    if (align_sim3) track_anchor[i] = tracker->anchorPair();
                }
                if (mapper) { prev_gray.swap(gray); pw = fw; ph = fh; }
                FrameRecord& o = rec[i];
                o.keypoints = r.frame->numKeypoints();
                o.matches = r.matches.size();
                o.hash = frame_hash(*r.frame, r.matches);
                o.is_keyframe = r.is_keyframe;
                if (r.loop) { o.loop_match_id = (long long)r.loop->match_id; o.loop_score = r.loop->score; }
                if (posthoc_loop && (int)r.matches.size() >= fc.frontend.keyframe_min_matches) o.frame = std::make_unique<core::Frame>(*r.frame);
                const std::size_t d = ++done;
                if (s == 0) { w = fw; h = fh; }
                if (!sharded && d % 100 == 0) {                            // euroc_eval.cpp:271-277
                    const auto now = std::chrono::steady_clock::now();
                    const double fps = 100.0 / std::chrono::duration<double>(now - t_last).count();
                    t_last = now;
                    std::printf("Frame %zu/%zu | FPS: %.1f | keypoints: %zu | matches: %zu\n", d, N, fps, o.keypoints, o.matches);
                }
            }
            if (mapper) {                                                  // euroc_eval.cpp:291, 326
                mapper->filterOutliers();
                mapper->exportPLY(map_file);
                map_points = mapper->size();
            }
            if (tracker) track_points = tracker->mapper().size();
            if (tracker && align_sim3) kept_tracker = std::move(tracker);
            if (dense_tracker) {
                dense_tracked = dense_tracker->framesTracked();
                dense_lost = dense_tracker->framesLost();
            }
            if (volume) {
                volume_points = (long long)volume->exportPLY(volume_file);
                volume_observed = (long long)volume->observedVoxels();
            }
            if (volume && !mesh_file.empty()) {
                adapters::hip::HipVolumeMesher mesher(adapters::hip::VolumeMesherConfig::fromVolume(*volume));
                mesher.update(*volume);
                const auto counts = mesher.exportPLY(mesh_file);
                mesh_vertices = (long long)counts.first;
                mesh_triangles = (long long)counts.second;
            }
            if (volume && !render_prefix.empty() && !integrated.empty()) {
                adapters::hip::HipVolumeRenderer renderer(adapters::hip::VolumeRendererConfig::fromVolume(*volume));
                renderer.update(*volume);
                std::vector<std::size_t> frames;
                std::vector<std::array<double, 12>> views;
                for (std::size_t k = 0; k < integrated.size(); k += (std::size_t)render_every) {
                    frames.push_back(integrated[k].first);
                    views.push_back(integrated[k].second);
                }
                const std::size_t px = (std::size_t)render_w * render_h, chunk = 64;   // one batch up to 64 views: bounded memory on a long sequence
                for (std::size_t c0 = 0; c0 < frames.size(); c0 += chunk) {
                    const std::size_t n = std::min(chunk, frames.size() - c0);
                    const std::vector<std::array<double, 12>> part(views.begin() + (std::ptrdiff_t)c0, views.begin() + (std::ptrdiff_t)(c0 + n));
                    const adapters::hip::RenderedViews rv = renderer.castBatch(part, render_w, render_h);
                    for (std::size_t k = 0; k < n; k++) {
                        const std::string base = render_prefix + "_" + std::to_string(frames[c0 + k]);
                        adapters::hip::HipVolumeRenderer::writeDepthPGM(base + "_depth.pgm", rv.depth.data() + k * px, render_w, render_h);
                        adapters::hip::HipVolumeRenderer::writeGrayPGM(base + "_shade.pgm", rv.shade.data() + k * px, render_w, render_h);
                    }
                    render_hits += rv.hitPixels();
                }
                render_views = (long long)frames.size();
            }
            std::ofstream pf;
            if (!plan_file.empty()) pf.open(plan_file);                    // created even when there is nothing to plan
            if (volume && !plan_file.empty() && sp.hi > sp.first) {
                adapters::hip::HipPathPlanner planner(adapters::hip::PathPlannerConfig::fromVolume(*volume));
                planner.update(*volume);
                auto cell_under = [&](const std::array<double, 16>& T) {    // the camera centre -R^T t of a world-to-camera pose
                    float c[3];
                    for (int a = 0; a < 3; a++) c[a] = (float)-(T[(size_t)a] * T[3] + T[(size_t)(4 + a)] * T[7] + T[(size_t)(8 + a)] * T[11]);
                    return planner.cellOf(c[0], c[1], c[2]);
                };
                const std::array<std::int32_t, 2> start = cell_under(traj[sp.first]), goal = cell_under(traj[sp.hi - 1]);
                const adapters::hip::PlanResult pr = planner.plan({goal}, {{start[0], start[1], 0}}, planner.nu() * planner.nv());
                plan_record = pr.records[0];
                pf << std::setprecision(9);
                for (int k = 0; k < plan_record.n_cells; k++) {
                    const std::int32_t c = pr.paths[(size_t)k];
                    const std::array<float, 3> X = planner.centreOf(c % planner.nu(), c / planner.nu());
                    pf << X[0] << ' ' << X[1] << ' ' << X[2] << '\n';
                }
            }
        } catch (const std::exception& e) {
            errors[(size_t)s] = e.what();
        }
    };
    if (!sharded) {
        run_shard(0);
    } else {
        std::vector<std::thread> th;
        for (int s = 0; s < shards; s++) th.emplace_back(run_shard, s);
        for (auto& t : th) t.join();
    }
    for (int s = 0; s < shards; s++)
        if (!errors[(size_t)s].empty()) { std::fprintf(stderr, "shard %d: %s\n", s, errors[(size_t)s].c_str()); return 1; }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // the loop-closure step of a sharded or batched run: the merged stream, in frame order (euroc_eval.cpp:230-247)
    if (posthoc_loop && N > 0) {
        factory::HipFactoryConfig fc;
        fc.max_features = max_features;
        adapters::hip::HipLoopDetector ld(fc.loop_min_frames_between, fc.loop_min_score, fc.loop_min_matches,
                                          ((max_features + 8 * 64 + 63) / 64) * 64, loop_capacity, nullptr, 0);
        std::shared_ptr<adapters::hip::HipPlaceIndex> place;
        int place_iters = 0;
        if (loop_bow > 0) {
            adapters::hip::PlaceIndexConfig pc;
            pc.words = loop_bow;
            pc.rows = std::min(((max_features + 8 * 64 + 63) / 64) * 64, 4096);
            pc.capacity = loop_capacity;
            pc.top_k = loop_bow_top;
            pc.min_frames_between = fc.loop_min_frames_between;
            place = std::make_shared<adapters::hip::HipPlaceIndex>(pc);
            const bool have_file = !loop_bow_vocab.empty() && std::ifstream(loop_bow_vocab).good();
            if (have_file) {
                place->load(loop_bow_vocab);
                if (place->words() != loop_bow) {
                    std::fprintf(stderr, "--loop-bow-vocab %s holds %d words, --loop-bow asks for %d\n", loop_bow_vocab.c_str(), place->words(), loop_bow);
                    return 1;
                }
            } else {
                // the pre-pass: at most 256 of the frames that can be keyframes, sampled evenly over the sequence
                std::vector<const core::Frame*> cand, pick;
                for (std::size_t i = 1; i < N; i++)
                    if ((int)rec[i].matches >= fc.frontend.keyframe_min_matches && rec[i].frame) cand.push_back(rec[i].frame.get());
                const std::size_t want = std::min<std::size_t>(cand.size(), 256);
                std::size_t rows = 0;
                for (std::size_t k = 0; k < want; k++) {
                    pick.push_back(cand[k * cand.size() / want]);
                    rows += pick.back()->numKeypoints();
                }
                if (rows < (std::size_t)loop_bow) {
                    std::fprintf(stderr, "--loop-bow %d: the %zu training frames hold %zu descriptors, fewer than the words asked for\n", loop_bow,
                                 pick.size(), rows);
                    return 1;
                }
                place_iters = place->train(pick);
                if (!loop_bow_vocab.empty()) place->save(loop_bow_vocab);
            }
            ld.setPlaceIndex(place, loop_bow_top);
        }
        std::unique_ptr<adapters::hip::HipFundamentalEstimator> fund;
        std::unique_ptr<adapters::hip::HipPoseEstimator> pose;
        std::deque<std::size_t> held;                                  // keyframes in the database, oldest first
        std::unique_ptr<adapters::hip::HipSim3Aligner> aligner;        // --loop-align sim3
        std::ofstream align_out;
        long long align_candidates = 0, align_replaced = 0;
        std::vector<adapters::hip::Sim3Report> detect_reports;        // --loop-correct: what the verifier said during one detect()
        if (verify_reference) {
            fund = std::make_unique<adapters::hip::HipFundamentalEstimator>();
            pose = std::make_unique<adapters::hip::HipPoseEstimator>(adapters::hip::referenceLoopIntrinsics());
            adapters::hip::HipLoopDetector::Verifier reference =
                adapters::hip::makeReferenceVerifier(*fund, *pose, fc.loop_min_matches, [&](std::uint64_t id) {
                    return id < N && rec[(size_t)id].frame ? rec[(size_t)id].frame.get() : nullptr;
                });
            if (align_sim3 && kept_tracker) {
                // after the reference verification has accepted a candidate: the two keyframes' landmarks, joined through its
                // match list and aligned; a valid alignment with >= 20 inliers replaces the unit-length edge by [R t] in map units
                aligner = std::make_unique<adapters::hip::HipSim3Aligner>(track_K);
                if (!loop_align_out.empty()) { align_out.open(loop_align_out); align_out << std::setprecision(17); }
                auto lookup = [&](std::uint64_t id) -> std::optional<adapters::hip::KeyframeInMap> {
                    if (id >= N || !rec[(size_t)id].frame || track_anchor[(size_t)id] < 0) return std::nullopt;
                    adapters::hip::KeyframeInMap k;
                    k.anchor_pair = track_anchor[(size_t)id];
                    k.anchor_view = 2;                                     // the tracker's points index the last frame as view 2
                    for (int q = 0; q < 12; q++) k.pose[(size_t)q] = track_traj[(size_t)id][(size_t)q];
                    k.frame = rec[(size_t)id].frame.get();
                    return k;
                };
                auto report = [&](const adapters::hip::Sim3Report& r) {
                    align_candidates++;
                    align_replaced += r.replaced ? 1 : 0;
                    if (loop_correct) detect_reports.push_back(r);
                    if (align_out.is_open())
                        align_out << r.query_id << ' ' << r.match_id << ' ' << r.s << ' ' << r.n_corr << ' ' << r.n_inliers << ' ' << r.rms_px
                                  << ' ' << (r.replaced ? 1 : 0) << '\n';
                };
                ld.setVerifier(adapters::hip::makeSim3Verifier(*aligner, kept_tracker->mapper().handle(), lookup, reference, 20, report));
            } else {
                ld.setVerifier(reference);
            }
        }
        for (std::size_t i = 1; i < N; i++) {
            FrameRecord& o = rec[i];
            if ((int)o.matches < fc.frontend.keyframe_min_matches || !o.frame) continue;
            core::KeyFrame kf;
            kf.id = i;                                                     // FrontEnd numbers frames from 0 in sequence order
            kf.timestamp = seq.at(i).timestamp;
            kf.frame = *o.frame;
            kf.frame.id = i;
            detect_reports.clear();
            auto lp = ld.detect(kf);
            ld.addKeyFrame(kf);
            o.is_keyframe = true;
            if (verify_reference) {                                    // keep the keypoints of the 500 keyframes held
                held.push_back(i);
                if (held.size() > (std::size_t)loop_capacity) { rec[held.front()].frame.reset(); held.pop_front(); }
            }
            if (lp) { o.loop_match_id = (long long)lp->match_id; o.loop_score = lp->score; }
            if (lp && graph)                                               // euroc_eval.cpp:235
                graph->addLoopEdge((int)lp->query_id, (int)lp->match_id, adapters::hip::loopRelativePose(*lp));
            if (lp && loop_correct)                                        // the accepted alignment of this candidate, if there is one
                for (const adapters::hip::Sim3Report& r : detect_reports)
                    if (r.replaced && r.query_id == lp->query_id && r.match_id == lp->match_id) {
                        correct_edges.push_back({(int)lp->match_id, (int)lp->query_id, adapters::hip::loopRelativePose(*lp), r.s});
                        break;
                    }
        }
        if (aligner)
            std::printf("loop align sim3 candidates %lld replaced %lld%s%s\n", align_candidates, align_replaced,
                        loop_align_out.empty() ? "" : " -> ", loop_align_out.c_str());
        if (place)
            std::printf("loop bow words %d iterations %d entries %d queries %lld candidates %lld\n", place->words(), place_iters, place->size(),
                        ld.placeQueries(), ld.placeCandidates());
    }

    long long total_kp = 0, total_matches = 0, n_keyframes = 0, n_loops = 0;
    std::ofstream out;
    if (!csv.empty()) { out.open(csv); out << std::setprecision(17); out << "frame,timestamp,keypoints,matches,hash,keyframe,loop_match_id,loop_score\n"; }
    for (std::size_t i = 0; i < N; i++) {
        const FrameRecord& o = rec[i];
        total_kp += (long long)o.keypoints;
        total_matches += (long long)o.matches;
        n_keyframes += o.is_keyframe ? 1 : 0;
        n_loops += o.loop_match_id >= 0 ? 1 : 0;
        if (out.is_open())
            out << i << ',' << std::to_string(seq.at(i).timestamp) << ',' << o.keypoints << ',' << o.matches << ',' << o.hash << ','
                << (o.is_keyframe ? 1 : 0) << ',' << o.loop_match_id << ',' << o.loop_score << '\n';
    }
    std::printf("frames %zu size %dx%d mean_keypoints %.2f mean_matches %.2f fps %.1f (PNG decode + H2D + extract + match + D2H; %d shard%s on %d device%s)\n",
                N, w, h, N ? (double)total_kp / N : 0.0, N > 1 ? (double)total_matches / (N - 1) : 0.0, N / secs, shards,
                shards > 1 ? "s" : "", devices, devices > 1 ? "s" : "");
    if (batch > 0) {
        pipeline::BatchStats t;
        for (const pipeline::BatchStats& b : bstats) {
            t.frames += b.frames; t.chunks += b.chunks; t.decode_s += b.decode_s; t.h2d_s += b.h2d_s; t.h2d_bytes += b.h2d_bytes;
            t.gpu_s += b.gpu_s; t.d2h_s += b.d2h_s; t.d2h_bytes += b.d2h_bytes; t.deliver_s += b.deliver_s; t.wall_s = std::max(t.wall_s, b.wall_s);
        }
        // stage times are summed over shards and chunks; the stages overlap (decode of chunk c + 1 and its upload run beside
        // the kernels of chunk c), so they do not add up to the wall time
        std::printf("batch %d frames/chunk, %zu chunks, %d decode threads/shard | decode %.3f s (%.0f frames/s) | H2D %.3f s (%.2f GB/s) | "
                    "extract+match kernels %.3f s (%.0f frames/s) | D2H %.3f s (%.2f GB/s) | deliver %.3f s | wall %.3f s\n",
                    batch, t.chunks, decode_threads, t.decode_s, t.decode_s > 0 ? t.frames / t.decode_s : 0.0, t.h2d_s,
                    t.h2d_s > 0 ? t.h2d_bytes / t.h2d_s * 1e-9 : 0.0, t.gpu_s, t.gpu_s > 0 ? t.frames / t.gpu_s : 0.0, t.d2h_s,
                    t.d2h_s > 0 ? t.d2h_bytes / t.d2h_s * 1e-9 : 0.0, t.deliver_s, t.wall_s);
    }
    if (loop) std::printf("keyframes %lld loops %lld\n", n_keyframes, n_loops);
    // one TUM line per frame: "timestamp tx ty tz qx qy qz qw" of a 4x4 row-major pose
    auto write_tum = [&](const std::string& path, auto&& pose_of) {
        std::ofstream tf(path);
        tf << std::fixed << std::setprecision(9);
        for (std::size_t i = 0; i < N; i++) {
            const std::array<double, 16> T = pose_of(i);
            double q[4];                                                   // rotation -> quaternion (x, y, z, w)
            const double tr = T[0] + T[5] + T[10];
            if (tr > 0) {
                const double s = std::sqrt(tr + 1.0) * 2;
                q[3] = 0.25 * s; q[0] = (T[9] - T[6]) / s; q[1] = (T[2] - T[8]) / s; q[2] = (T[4] - T[1]) / s;
            } else if (T[0] > T[5] && T[0] > T[10]) {
                const double s = std::sqrt(1.0 + T[0] - T[5] - T[10]) * 2;
                q[3] = (T[9] - T[6]) / s; q[0] = 0.25 * s; q[1] = (T[1] + T[4]) / s; q[2] = (T[2] + T[8]) / s;
            } else if (T[5] > T[10]) {
                const double s = std::sqrt(1.0 + T[5] - T[0] - T[10]) * 2;
                q[3] = (T[2] - T[8]) / s; q[0] = (T[1] + T[4]) / s; q[1] = 0.25 * s; q[2] = (T[6] + T[9]) / s;
            } else {
                const double s = std::sqrt(1.0 + T[10] - T[0] - T[5]) * 2;
                q[3] = (T[4] - T[1]) / s; q[0] = (T[2] + T[8]) / s; q[1] = (T[6] + T[9]) / s; q[2] = 0.25 * s;
            }
            tf << seq.at(i).timestamp << ' ' << T[3] << ' ' << T[7] << ' ' << T[11] << ' ' << q[0] << ' ' << q[1] << ' ' << q[2]
               << ' ' << q[3] << '\n';
        }
    };
    if (!pose_file.empty()) {
        write_tum(pose_file, [&](std::size_t i) { return traj[i]; });
        std::printf("pose updates %lld of %zu frames -> %s\n", n_pose_updates, N > 0 ? N - 1 : 0, pose_file.c_str());
    }
    if (!fuse_file.empty()) {                                              // euroc_eval.cpp:139-142, 209
        if (seq.imu().empty()) { std::fprintf(stderr, "--fuse: the sequence has no mav0/imu0/data.csv\n"); return 1; }
        std::vector<aria_imu_sample> samples;
        std::vector<int> imu_end(N);
        for (std::size_t i = 0; i < N; i++) {
            for (std::size_t k = seq.imuBegin(i); k < seq.imuEnd(i); k++) {
                const io::AslImu& m = seq.imu()[k];
                aria_imu_sample sm{};
                sm.t = m.timestamp;
                for (int a = 0; a < 3; a++) { sm.accel[a] = m.accel[a]; sm.gyro[a] = m.gyro[a]; }
                samples.push_back(sm);
            }
            imu_end[i] = (int)samples.size();
            fuse_visual[i].t = seq.at(i).timestamp;
            if (!fuse_visual[i].accept) fuse_visual[i].R[0] = fuse_visual[i].R[4] = fuse_visual[i].R[8] = 1.0;
        }
        std::vector<aria_fuse_state> states(N);
        try {
            adapters::hip::HipSensorFusion fusion;
            fusion.run(samples.data(), (int)samples.size(), imu_end.data(), fuse_visual.data(), (int)N, states.data());
        } catch (const std::exception& e) {
            std::fprintf(stderr, "--fuse: %s\n", e.what());
            return 1;
        }
        if (!eval_file.empty()) fused_states = states;
        std::ofstream tf(fuse_file);
        tf << std::fixed << std::setprecision(9);
        long long predicted = 0, skipped = 0, ignored = 0, updates = 0;
        for (std::size_t i = 0; i < N; i++) {
            const aria_fuse_state& st = states[i];
            tf << seq.at(i).timestamp << ' ' << st.p[0] << ' ' << st.p[1] << ' ' << st.p[2] << ' ' << st.q[1] << ' ' << st.q[2] << ' '
               << st.q[3] << ' ' << st.q[0] << '\n';
            predicted += st.n_predicted; skipped += st.n_skipped; ignored += st.n_ignored; updates += st.n_updates;
        }
        std::printf("fused %lld updates | imu samples %zu: %lld predicted %lld skipped %lld before the first pose -> %s\n", updates,
                    samples.size(), predicted, skipped, ignored, fuse_file.c_str());
    }
    if (graph && loop_correct) {                                           // the Sim(3) graph over the tracker's trajectory
        if (!kept_tracker) { std::fprintf(stderr, "--loop-correct: no tracker map was kept\n"); return 1; }
        try {
            adapters::hip::HipSim3GraphOptimizer sg;
            auto poseOf = [&](std::size_t i) {
                adapters::hip::GraphPose T = adapters::hip::GraphPose::Identity();
                for (int a = 0; a < 4; a++)
                    for (int b = 0; b < 4; b++) T(a, b) = track_traj[i][(size_t)(a * 4 + b)];
                return T;
            };
            for (std::size_t i = 0; i < N; i++) {
                const adapters::hip::GraphPose X = adapters::hip::cameraToWorld(poseOf(i));
                sg.setInitialPose((int)i, X);
                if (i > 0) {                                               // Z = X_{i-1}^-1 X_i = T_{i-1} T_i^-1
                    const adapters::hip::GraphPose Tp = poseOf(i - 1);
                    adapters::hip::GraphPose Z = adapters::hip::GraphPose::Identity();
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 4; b++) {
                            double v = 0.0;
                            for (int k = 0; k < 4; k++) v += Tp(a, k) * X(k, b);
                            Z(a, b) = v;
                        }
                    sg.addOdometryEdge((int)i - 1, (int)i, Z);
                }
            }
            for (const CorrectEdge& e : correct_edges) sg.addLoopEdge(e.from, e.to, e.Z, e.s);
            sg.optimize(50);
            std::vector<int> pair_anchor;                                  // pair id -> the first frame that owns it
            for (std::size_t i = 0; i < N; i++) {
                const int p = track_anchor[i];
                if (p < 0) continue;
                if ((std::size_t)p >= pair_anchor.size()) pair_anchor.resize((std::size_t)p + 1, -1);
                if (pair_anchor[(std::size_t)p] < 0) pair_anchor[(std::size_t)p] = (int)i;
            }
            const aria_sgraph_correct_stats cs = sg.correctMap(kept_tracker->mapper().handle(), pair_anchor, 0);
            if (!loop_correct_map.empty()) kept_tracker->mapper().exportPLY(loop_correct_map);
            auto corrected = [&](std::size_t i) {
                const adapters::hip::GraphPose m = sg.getOptimizedPose((int)i);
                std::array<double, 16> T{};
                for (int a = 0; a < 4; a++)
                    for (int b = 0; b < 4; b++) T[(size_t)(a * 4 + b)] = m(a, b);
                return T;
            };
            write_tum(optimize_file, corrected);
            if (!eval_file.empty())
                for (std::size_t i = 0; i < N; i++) {
                    const std::array<double, 16> T = corrected(i);
                    for (int a = 0; a < 3; a++) optimized_xyz.push_back(T[(size_t)(a * 4 + 3)]);
                }
            const aria_sgraph_result& gr = sg.lastResult();
            std::printf("sim3 pose graph %zu vertices %zu edges | chi2 %.6g -> %.6g in %d iterations (%d solves, %d PCG iterations) -> %s\n",
                        sg.numVertices(), sg.numEdges(), gr.chi2_initial, gr.chi2_final, gr.iterations_done, gr.trials, gr.pcg_iterations,
                        optimize_file.c_str());
            std::printf("loop correct edges %zu moved %d left %d refused %d%s%s\n", correct_edges.size(), cs.moved, cs.left_alone, cs.refused,
                        loop_correct_map.empty() ? "" : " -> ", loop_correct_map.c_str());
        } catch (const std::exception& e) {
            std::fprintf(stderr, "--loop-correct: %s\n", e.what());
            return 1;
        }
    } else if (graph) {                                                    // euroc_eval.cpp:282-288
        graph->optimize(50);
        write_tum(optimize_file, [&](std::size_t i) {
            if (last_vertex[i] < 0) return traj[i];                        // before the first vertex: current_pose, the identity
            const adapters::hip::GraphPose m = graph->getOptimizedPose((int)last_vertex[i]);
            std::array<double, 16> T{};
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) T[(size_t)(a * 4 + b)] = m(a, b);
            return T;
        });
        if (!eval_file.empty())
            for (std::size_t i = 0; i < N; i++) {
                std::array<double, 16> T = traj[i];
                if (last_vertex[i] >= 0) {
                    const adapters::hip::GraphPose m = graph->getOptimizedPose((int)last_vertex[i]);
                    for (int a = 0; a < 3; a++) T[(size_t)(a * 4 + 3)] = m(a, 3);
                }
                for (int a = 0; a < 3; a++) optimized_xyz.push_back(T[(size_t)(a * 4 + 3)]);
            }
        const aria_graph_result& gr = graph->lastResult();
        std::printf("pose graph %zu vertices %zu edges | chi2 %.6g -> %.6g in %d iterations (%d solves, %d PCG iterations) -> %s\n",
                    graph->numVertices(), graph->numEdges(), gr.chi2_initial, gr.chi2_final, gr.iterations_done, gr.trials,
                    gr.pcg_iterations, optimize_file.c_str());
    }
    if (!map_file.empty()) std::printf("map %zu points -> %s\n", map_points, map_file.c_str());
    if (!track_file.empty()) {
        write_tum(track_file, [&](std::size_t i) { return track_traj[i]; });
        std::printf("track pnp %lld fallback %lld bootstrap %lld held %lld map %zu -> %s\n", track_steps[2], track_steps[3],
                    track_steps[1], track_steps[0], track_points, track_file.c_str());
        if (local_map > 0) std::printf("track local %lld of the last %d pairs, radius %.1f px\n", track_steps[4], local_map, local_radius);
    }
    if (!bundle_file.empty()) {
        // windows in order; a window's refined poses and points seed the next (WindowBuilder::store)
        std::vector<std::string> lines;
        const int frames = bundle_builder.frames();
        if (frames >= 3) {
            adapters::hip::HipBundleAdjuster adjuster(bundle_K, -1.0, 1e-6, 10, 1);        // post hoc on device 0, as --optimize is
            for (int first = 0; first + 2 < frames; first += bundle_window - 2) {
                const int n = std::min(bundle_window, frames - first);
                adapters::hip::BundleWindow w = bundle_builder.window(first, n);
                const adapters::hip::BundleResult r = adjuster.optimize(w, 0);
                bundle_builder.store(w);
                char buf[256];
                std::snprintf(buf, sizeof(buf), "# window %d %d points %d observations %zu chi2_initial %.9g chi2_final %.9g rms_px %.6f",
                              first, n, w.nPoints(), w.obs.size(), r.record.chi2_initial, r.record.chi2_final, r.record.rms_px);
                lines.push_back(buf);
            }
        }
        write_tum(bundle_file, [&](std::size_t i) {
            const long long k = (long long)i - bundle_first;
            if (bundle_first < 0 || k < 0 || k >= frames) return track_traj[i];
            std::array<double, 16> T{};
            const std::array<double, 12>& p = bundle_builder.pose((int)k);
            for (int c = 0; c < 12; c++) T[(std::size_t)c] = p[(std::size_t)c];
            T[15] = 1.0;
            return T;
        });
        std::ofstream bf(bundle_file, std::ios::app);
        for (const std::string& l : lines) bf << l << '\n';
        std::printf("bundle %d frames %zu windows of %d -> %s\n", frames, lines.size(), bundle_window, bundle_file.c_str());
    }
    if (stereo) {
        std::ofstream sf;
        if (!stereo_file.empty()) sf.open(stereo_file);
        long long matched = 0, scaled = 0;
        for (std::size_t i = 0; i < N; i++) {
            const StereoLine& l = stereo_lines[i];
            char line[160];
            int n = std::snprintf(line, sizeof(line), "%.9f %d %.9f", seq.at(i).timestamp, l.matched, (double)l.median_depth);
            if (!pose_file.empty()) std::snprintf(line + n, sizeof(line) - (size_t)n, " %d %.9f", l.scale_valid, l.scale);
            if (sf.is_open()) sf << line << '\n';
            else std::printf("stereo %s\n", line);
            matched += l.matched;
            scaled += l.scale_valid;
        }
        std::printf("stereo baseline %.6g m | mean matched %.2f per frame", stereo_baseline_used, N ? (double)matched / N : 0.0);
        if (!pose_file.empty()) std::printf(" | %lld relative poses scaled", scaled);
        std::printf("%s%s\n", stereo_file.empty() ? "" : " -> ", stereo_file.c_str());
    }
    if (!dense_file.empty()) {
        std::ofstream df(dense_file);
        double share = 0.0;
        for (std::size_t i = 0; i < N; i++) {
            char line[160];
            std::snprintf(line, sizeof(line), "%.9f %.9f %.9f", seq.at(i).timestamp, dense_lines[i].valid_share,
                          (double)dense_lines[i].median_depth);
            df << line << '\n';
            share += dense_lines[i].valid_share;
        }
        std::printf("dense 64 disparities | mean valid share %.4f -> %s\n", N ? share / N : 0.0, dense_file.c_str());
    }
    if (!volume_file.empty()) std::printf("volume %lld %lld\n", volume_points, volume_observed);
    if (!mesh_file.empty()) std::printf("mesh %lld %lld\n", mesh_vertices, mesh_triangles);
    if (!plan_file.empty()) std::printf("plan %d %d %d\n", plan_record.status, plan_record.cost, plan_record.n_cells);
    if (!render_prefix.empty()) std::printf("render %lld %lld\n", render_views, render_hits);
    if (!dense_track_file.empty()) {
        write_tum(dense_track_file, [&](std::size_t i) { return dense_traj[i]; });
        std::printf("track-dense tracked %lld lost %lld -> %s\n", dense_tracked, dense_lost, dense_track_file.c_str());
        std::fprintf(stderr, "track-dense: %lld of %lld tracked frames lost\n", dense_lost, dense_tracked);
    }
    if (!alerts_file.empty()) {
        std::ofstream af(alerts_file);
        for (const std::string& l : alert_lines) af << l << '\n';
        std::printf("alerts %lld %lld\n", alert_events, alert_frames);
    }
    if (!eval_file.empty()) {                                              // euroc_eval.cpp:247-252, 294-305
        try {
            aria_eval_config ec;
            aria_eval_default_config(&ec);
            ec.align_mode = eval_mode;
            ec.rpe_delta = rpe_delta;
            adapters::hip::HipTrajectoryEvaluator ev(&ec);
            std::vector<aria_eval_truth> gt(seq.groundTruth().size()), truth;
            static_assert(sizeof(io::AslGroundTruth) == sizeof(aria_eval_truth), "AslGroundTruth has aria_eval_truth's layout");
            std::memcpy(gt.data(), seq.groundTruth().data(), gt.size() * sizeof(aria_eval_truth));
            std::vector<double> ts(N);
            for (std::size_t i = 0; i < N; i++) ts[i] = seq.at(i).timestamp;
            if (ev.sampleGroundTruth(gt, ts, truth) != ARIA_OK) {
                std::fprintf(stderr, "--eval: the ground truth is not usable (a non-finite field or decreasing timestamps)\n");
                return 1;
            }
            std::vector<double> pose_xyz;
            for (std::size_t i = 0; i < N; i++)
                for (int a = 0; a < 3; a++) pose_xyz.push_back(traj[i][(size_t)(a * 4 + 3)]);
            const int off[2] = {0, (int)N};
            std::ofstream ef(eval_file);
            ef << std::setprecision(17);
            aria_eval_result report{};
            auto score = [&](const char* name, const void* est, int kind) {
                aria_eval_result r{};
                if (ev.evaluateBatch(est, kind, off, (int)N, 1, truth.data(), (int)N, false, nullptr, nullptr, &r) != ARIA_OK)
                    throw std::runtime_error(std::string("trajectory '") + name + "' holds a non-finite position");
                ef << name << ' ' << eval_align << ' ' << r.n_poses << ' ' << r.n_used << ' ' << r.ate_raw << ' ' << r.rpe_raw << ' '
                   << r.align_valid << ' ' << r.scale << ' ' << r.ate_rmse << ' ' << r.ate_mean << ' ' << r.ate_max << ' '
                   << r.rpe_aligned << ' ' << r.sigma[0] << ' ' << r.sigma[1] << ' ' << r.sigma[2] << '\n';
                std::printf("eval %s: %d of %d poses | raw ATE %.4f m RPE %.4f m | %s-aligned ATE rmse %.4f mean %.4f max %.4f m RPE %.4f m scale %.6g\n",
                            name, r.n_used, r.n_poses, r.ate_raw, r.rpe_raw, eval_align.c_str(), r.ate_rmse, r.ate_mean, r.ate_max,
                            r.rpe_aligned, r.scale);
                return r;
            };
            report = score("pose", pose_xyz.data(), ARIA_EVAL_EST_XYZ);
            if (!optimized_xyz.empty()) report = score("optimize", optimized_xyz.data(), ARIA_EVAL_EST_XYZ);
            if (!fused_states.empty()) score("fuse", fused_states.data(), ARIA_EVAL_EST_FUSE_STATE);
            if (!dense_traj.empty()) {
                std::vector<double> dense_xyz;
                for (std::size_t i = 0; i < N; i++)
                    for (int a = 0; a < 3; a++) dense_xyz.push_back(dense_traj[i][(size_t)(a * 4 + 3)]);
                score("track-dense", dense_xyz.data(), ARIA_EVAL_EST_XYZ);
            }
            std::printf("\nTrajectory Error:\n  ATE (RMSE): %.4f m\n  RPE (RMSE): %.4f m\n", report.ate_raw, report.rpe_raw);   // :303-305
        } catch (const std::exception& e) {
            std::fprintf(stderr, "--eval: %s\n", e.what());
            return 1;
        }
    }
    return 0;
}
