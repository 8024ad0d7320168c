// fpfh_runner — pcl::NormalEstimation -> pcl::FPFHEstimation (setKSearch) through the C++ adaptor (include/rsreg/pcl_compat.hpp),
// for tests/test_fpfh_gpu.py: the first two steps of a feature-based pre-alignment.
//   fpfh_runner <in.bin> <width> <height> <k_normals> <k> <out_host.bin> <out_device.bin>
// in: 32-byte PointXYZRGB records; out: 132-byte FPFHSignature33 records, once from host clouds and once from clouds that stay in
// HBM.  Prints the size, width, height and is_dense of both results, and whether setRadiusSearch was refused.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Normals = rsreg::PointCloud<rsreg::Normal>;
using Features = rsreg::PointCloud<rsreg::FPFHSignature33>;

static void save(const Features &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::FPFHSignature33)));
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <k_normals> <k> <out_host.bin> <out_device.bin>\n", argv[0]);
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
        Normals::Ptr normals(new Normals);
        ne.compute(*normals);
        rsreg::FPFHEstimation<rsreg::PointXYZRGB, rsreg::Normal, rsreg::FPFHSignature33> fe;
        fe.setInputCloud(frame);
        fe.setInputNormals(normals);
        fe.setKSearch(std::atoi(argv[5]));
        int refused = 0;
        try {
            fe.setRadiusSearch(0.05);
        } catch (const rsreg::Error &) {
            refused = 1;
        }
        Features host;
        fe.compute(host);
        save(host, argv[6]);
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame);
        rsreg::DeviceCloud<rsreg::Normal> dev_normals;
        ne.compute(dev, dev_normals);
        rsreg::DeviceCloud<rsreg::FPFHSignature33> dev_features;
        fe.compute(dev, dev_normals, dev_features);
        Features out;
        dev_features.download(out);
        save(out, argv[7]);
        std::printf("size %zu\nsize_device %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\nk %d\nradius_refused %d\n", host.size(), out.size(), host.width,
                    host.height, (int)host.is_dense, (int)out.is_dense, fe.getKSearch(), refused);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
