// fitness_runner — getFitnessScore through the C++ adaptor (include/rsreg/pcl_compat.hpp), for tests/test_fitness_score_gpu.py.
//   fitness_runner <src.bin> <tgt.bin>   (packed float32 xyz)
// Prints `name value` lines, the scores as C99 hex floats: icp_host (default range), icp_host_range (0.9), icp_device, ndt,
// state_error (1: getFitnessScore before align() threw rsreg::Error with RSREG_ERR_STATE).
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "rsreg/pcl_compat.hpp"

using namespace rsreg;
using Cloud = PointCloud<PointXYZRGB>;

static Cloud::Ptr load(const char *path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<float> xyz(bytes / 4);
    f.read(reinterpret_cast<char *>(xyz.data()), (std::streamsize)bytes);
    auto c = std::make_shared<Cloud>();
    for (size_t i = 0; i + 2 < xyz.size(); i += 3) {
        PointXYZRGB p{};
        p.x = xyz[i];
        p.y = xyz[i + 1];
        p.z = xyz[i + 2];
        c->push_back(p);
    }
    return c;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <src.bin> <tgt.bin>\n", argv[0]);
        return 2;
    }
    try {
        auto src = load(argv[1]), tgt = load(argv[2]);
        auto ctx = std::make_shared<Context>(0);
        IterativeClosestPoint<PointXYZRGB, PointXYZRGB> icp(ctx);
        icp.setMaxCorrespondenceDistance(0.01);
        icp.setInputSource(src);
        icp.setInputTarget(tgt);
        int state_error = 0;
        try {
            (void)icp.getFitnessScore();
        } catch (const Error &e) {
            state_error = e.status == RSREG_ERR_STATE;
        }
        Cloud out;
        icp.align(out);
        std::printf("icp_host %a\n", icp.getFitnessScore());
        std::printf("icp_host_range %a\n", icp.getFitnessScore(0.9));
        DeviceCloud<PointXYZRGB> dsrc(*src, ctx), dtgt(*tgt, ctx), dout(ctx);
        IterativeClosestPoint<PointXYZRGB, PointXYZRGB> dicp(ctx);
        dicp.setMaxCorrespondenceDistance(0.01);
        dicp.setInputSource(dsrc);
        dicp.setInputTarget(dtgt);
        dicp.align(dout);
        std::printf("icp_device %a\n", dicp.getFitnessScore());
        NormalDistributionsTransform<PointXYZRGB, PointXYZRGB> ndt(ctx);
        ndt.setResolution(1.0f);
        ndt.setInputSource(src);
        ndt.setInputTarget(tgt);
        Cloud nout;
        ndt.align(nout);
        std::printf("ndt %a\n", ndt.getFitnessScore());
        std::printf("state_error %d\n", state_error);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
