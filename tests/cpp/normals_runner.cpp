// normals_runner — pcl::NormalEstimation (setKSearch, setViewPoint) through the C++ adaptor (include/rsreg/pcl_compat.hpp),
// for tests/test_normals_gpu.py: the surveyed edge extractor's first step (src/edge_extractor.hpp:9-15).
//   normals_runner <in.bin> <width> <height> <k> <vx> <vy> <vz> <out_host.bin> <out_device.bin>
// in: 32-byte PointXYZRGB records; out: 32-byte Normal records, once from a host cloud and once from a cloud that stays in HBM.
// Prints the size, width, height and is_dense of both results.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Normals = rsreg::PointCloud<rsreg::Normal>;

static void save(const Normals &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::Normal)));
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <k> <vx> <vy> <vz> <out_host.bin> <out_device.bin>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr frame(new Cloud);
        frame->width = (uint32_t)std::atoi(argv[2]);
        frame->height = (uint32_t)std::atoi(argv[3]);
        frame->is_dense = false;
        frame->points.resize((size_t)frame->width * frame->height);
        std::ifstream f(argv[1], std::ios::binary);
        f.read(reinterpret_cast<char *>(frame->points.data()), (std::streamsize)(frame->size() * sizeof(rsreg::PointXYZRGB)));
        if (!f) throw std::runtime_error("short input file");
        rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> ne;
        ne.setInputCloud(frame);
        ne.setKSearch(std::atoi(argv[4]));
        ne.setViewPoint((float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]));
        Normals host;
        ne.compute(host);
        save(host, argv[8]);
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame);
        rsreg::DeviceCloud<rsreg::Normal> dev_normals;
        ne.compute(dev, dev_normals);
        Normals out;
        dev_normals.download(out);
        save(out, argv[9]);
        float vx, vy, vz;
        ne.getViewPoint(vx, vy, vz);
        std::printf("size %zu\nsize_device %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\nk %d\n", host.size(), out.size(), host.width, host.height,
                    (int)host.is_dense, (int)out.is_dense, ne.getKSearch());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
