// Drives aria::adapters::hip::HipPoseGraphOptimizer through the reference class's methods on a script that
// tests/test_gpu_graph.py writes, so that the C++ adapter, the Python adapter and the NumPy restatement see the same calls:
//   P id m00 .. m33          setInitialPose(id, M)          (16 doubles, row-major)
//   O from to s m00 .. m33   addOdometryEdge(from, to, M, s)
//   L from to s m00 .. m33   addLoopEdge(from, to, M, s)
//   LC from to s m00 .. m33  the same through a core::LoopCandidate's relative_pose and loopRelativePose (the driver's way)
//   OPT n                    optimize(n)
//   GET id                   prints "pose id m00 .. m33" of getOptimizedPose(id)
//   ALL                      prints "all N" and N lines "allpose k m00 .. m33" of getAllPoses()
//   CLEAR                    clear()
// and after every OPT "result chi2_initial chi2_final iterations_done trials pcg_iterations valid stop_reason". Doubles are
// printed with %.17g (round-trip exact). Ends with DONE.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "aria_hip/HipPoseGraphOptimizer.hpp"

using namespace aria;
using adapters::hip::GraphPose;

namespace {
GraphPose readPose(std::istringstream& in) {
    GraphPose T = GraphPose::Identity();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double v = 0;
            in >> v;
            T(r, c) = v;
        }
    return T;
}
void printPose(const char* tag, int id, const GraphPose& T) {
    std::printf("%s %d", tag, id);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) std::printf(" %.17g", T(r, c));
    std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: graph_selftest script.txt\n");
        return 2;
    }
    try {
        adapters::hip::HipPoseGraphOptimizer opt;
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            std::string op;
            in >> op;
            if (op == "P") {
                int id;
                in >> id;
                opt.setInitialPose(id, readPose(in));
            } else if (op == "O" || op == "L") {
                int a, b;
                double s;
                in >> a >> b >> s;
                const GraphPose Z = readPose(in);
                if (op == "O") opt.addOdometryEdge(a, b, Z, s);
                else opt.addLoopEdge(a, b, Z, s);
            } else if (op == "LC") {
                int a, b;
                double s;
                in >> a >> b >> s;
                const GraphPose Z = readPose(in);
                core::LoopCandidate cand;
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) adapters::hip::detail::setEntry(cand.relative_pose, r, c, Z(r, c), 0);
                opt.addLoopEdge(a, b, adapters::hip::loopRelativePose(cand), s);
            } else if (op == "OPT") {
                int n;
                in >> n;
                opt.optimize(n);
                const aria_graph_result& r = opt.lastResult();
                std::printf("result %.17g %.17g %d %d %d %d %d\n", r.chi2_initial, r.chi2_final, r.iterations_done, r.trials,
                            r.pcg_iterations, r.valid, r.stop_reason);
            } else if (op == "GET") {
                int id;
                in >> id;
                printPose("pose", id, opt.getOptimizedPose(id));
            } else if (op == "ALL") {
                const std::vector<GraphPose> all = opt.getAllPoses();
                std::printf("all %zu\n", all.size());
                for (std::size_t k = 0; k < all.size(); k++) printPose("allpose", (int)k, all[k]);
            } else if (op == "CLEAR") {
                opt.clear();
            }
        }
        std::printf("graph %zu %zu\n", opt.numVertices(), opt.numEdges());
        std::printf("DONE\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "graph_selftest: %s\n", e.what());
        return 1;
    }
    return 0;
}
