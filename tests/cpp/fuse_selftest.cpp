// Drives aria::adapters::hip::HipSensorFusion through the ISensorFusion port from a script (tests/test_gpu_fuse.py):
//   I t ax ay az gx gy gz      predictIMU
//   V t qw qx qy qz px py pz   updateVO
//   G                          print "state" (getFusedPose, getVelocity, the pose covariance's diagonal, initialised)
//   R                          reset()
//   P t qw qx qy qz px py pz   reset(pose)
// and prints DONE. Needs a GPU.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "aria_hip/HipSensorFusion.hpp"

using namespace aria;

static core::Pose readPose(std::istringstream& ss) {
    core::Pose p;
    double q[4];
    ss >> p.timestamp >> q[0] >> q[1] >> q[2] >> q[3] >> p.position(0) >> p.position(1) >> p.position(2);
    p.orientation = core::Quaternion{q[0], q[1], q[2], q[3]};
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: fuse_selftest script\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    try {
        interfaces::SensorFusionPtr port = std::make_unique<adapters::hip::HipSensorFusion>();
        auto* impl = static_cast<adapters::hip::HipSensorFusion*>(port.get());
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string op;
            ss >> op;
            if (op == "I") {
                core::ImuMeasurement m;
                ss >> m.timestamp >> m.accel(0) >> m.accel(1) >> m.accel(2) >> m.gyro(0) >> m.gyro(1) >> m.gyro(2);
                port->predictIMU(m);
            } else if (op == "V") {
                port->updateVO(readPose(ss));
            } else if (op == "R") {
                port->reset();
            } else if (op == "P") {
                port->reset(readPose(ss));
            } else if (op == "G") {
                const core::Pose p = port->getFusedPose();
                const core::Vector3 v = port->getVelocity();
                std::printf("state %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", p.timestamp, p.position(0),
                            p.position(1), p.position(2), p.orientation.w, p.orientation.x, p.orientation.y, p.orientation.z, v(0), v(1),
                            v(2));
                for (int k = 0; k < 6; k++) std::printf(" %.17g", p.covariance(k, k));
                std::printf(" %.17g %d\n", p.covariance(0, 4), impl->isInitialized() ? 1 : 0);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("DONE\n");
    return 0;
}
