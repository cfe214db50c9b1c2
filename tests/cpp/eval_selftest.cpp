// Drives aria::adapters::hip::HipTrajectoryEvaluator and AslSequence's ground truth from tests/test_gpu_eval.py and
// tests/test_eval_host.py:
//   eval_selftest gt <dataset_path>
//       prints "rows N" and one "gt" line of 17 %.17g fields per ground-truth row. Needs no GPU.
//   eval_selftest run <script>
//       the script holds "mode <0|1|2>", "delta <N>", "gt <17 doubles>" rows, "q <t>" query timestamps and
//       "e <x y z> [used]" estimate positions, one estimate per query. Samples the ground truth at the queries (prints one
//       "truth" line per query: valid and the 17 fields), scores the estimate against it (prints "result" with every field of
//       aria_eval_result and one "err" line per pose) and prints DONE. Needs a GPU.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "aria_hip/AslSequence.hpp"
#include "aria_hip/HipTrajectoryEvaluator.hpp"

using namespace aria;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: eval_selftest gt <dataset> | run <script>\n"); return 2; }
    if (!std::strcmp(argv[1], "gt")) {
        io::AslSequence seq;
        if (!seq.load(argv[2])) { std::fprintf(stderr, "cannot load %s\n", argv[2]); return 2; }
        std::printf("rows %zu\n", seq.groundTruth().size());
        for (const io::AslGroundTruth& g : seq.groundTruth()) {
            const double* d = &g.timestamp;
            std::printf("gt");
            for (int k = 0; k < 17; k++) std::printf(" %.17g", d[k]);
            std::printf("\n");
        }
        return 0;
    }
    std::ifstream in(argv[2]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    try {
        std::vector<aria_eval_truth> gt, truth;
        std::vector<double> ts, xyz, err;
        std::vector<std::uint8_t> mask;
        int mode = ARIA_EVAL_ALIGN_SIM3, delta = 10;
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string op;
            ss >> op;
            if (op == "mode") ss >> mode;
            else if (op == "delta") ss >> delta;
            else if (op == "gt") {
                aria_eval_truth g{};
                double* d = &g.t;
                for (int k = 0; k < 17; k++) ss >> d[k];
                gt.push_back(g);
            } else if (op == "q") {
                double t;
                ss >> t;
                ts.push_back(t);
            } else if (op == "e") {
                double x, y, z;
                int used = 1;
                ss >> x >> y >> z;
                if (!(ss >> used)) used = 1;
                xyz.insert(xyz.end(), {x, y, z});
                mask.push_back((std::uint8_t)(used != 0));
            }
        }
        adapters::hip::HipTrajectoryEvaluator ev;
        ev.setAlignMode(mode);
        ev.setRpeDelta(delta);
        std::vector<int> valid;
        const int rc = ev.sampleGroundTruth(gt, ts, truth, &valid);
        std::printf("sample_status %d\n", rc);
        for (std::size_t i = 0; i < truth.size(); i++) {
            const double* d = &truth[i].t;
            std::printf("truth %d", valid[i]);
            for (int k = 0; k < 17; k++) std::printf(" %.17g", d[k]);
            std::printf("\n");
        }
        const aria_eval_result r = ev.evaluate(xyz, truth, &mask, &err);
        std::printf("result %.17g %.17g %.17g", r.ate_raw, r.rpe_raw, r.scale);
        for (int k = 0; k < 9; k++) std::printf(" %.17g", r.R[k]);
        for (int k = 0; k < 3; k++) std::printf(" %.17g", r.t[k]);
        for (int k = 0; k < 3; k++) std::printf(" %.17g", r.sigma[k]);
        std::printf(" %.17g %.17g %.17g %.17g %d %d %d %d %d\n", r.ate_rmse, r.ate_mean, r.ate_max, r.rpe_aligned, r.n_poses, r.n_used,
                    r.n_rpe_pairs, r.align_valid, r.valid);
        for (double e : err) std::printf("err %.17g\n", e);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("DONE\n");
    return 0;
}
