// plane_seg_runner — pcl::SACSegmentation and pcl::ExtractIndices through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_plane_seg_gpu.py.
//   plane_seg_runner <in.bin> <n> <threshold> <max_iterations> <seed> <optimize 0|1> <perpendicular 0|1> <eps_angle> <out_prefix>
// in: 32-byte PointXYZRGB records.  Writes, once from a host cloud (<prefix>host_*) and once from a cloud that stays in HBM
// (<prefix>dev_*): inliers.bin (int32), coeff.bin (the coefficients as floats; empty when no model was found), rest.bin (the
// records ExtractIndices keeps with setNegative(true)) and plane.bin (the ones it keeps without).  The axis is z.  Prints the counts.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rsreg/pcl_compat.hpp"

using Point = rsreg::PointXYZRGB;
using Cloud = rsreg::PointCloud<Point>;

template <typename T> static void save(const std::vector<T> &v, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

static void save_cloud(const Cloud &c, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.points.size() * sizeof(Point)));
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in.bin> <n> <threshold> <max_iterations> <seed> <optimize> <perpendicular> <eps_angle> <out_prefix>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr cloud(new Cloud);
        cloud->width = (uint32_t)std::atoi(argv[2]);
        cloud->height = 1;
        cloud->is_dense = true;
        cloud->points.resize(cloud->width);
        std::ifstream f(argv[1], std::ios::binary);
        f.read(reinterpret_cast<char *>(cloud->points.data()), (std::streamsize)(cloud->size() * sizeof(Point)));
        if (!f) throw std::runtime_error("short input file");
        const std::string prefix = argv[9];

        rsreg::SACSegmentation<Point> seg;
        if (seg.getMaxIterations() != 50 || seg.getProbability() != 0.99 || !seg.getOptimizeCoefficients() || seg.getDistanceThreshold() != 0.0 ||
            seg.getModelType() != rsreg::SACMODEL_PLANE)
            throw std::runtime_error("the defaults are not PCL's");
        seg.setModelType(std::atoi(argv[7]) ? rsreg::SACMODEL_PERPENDICULAR_PLANE : rsreg::SACMODEL_PLANE);
        seg.setMethodType(rsreg::SAC_RANSAC);
        seg.setDistanceThreshold(std::atof(argv[3]));
        seg.setMaxIterations(std::atoi(argv[4]));
        seg.setSeed(std::strtoull(argv[5], nullptr, 10));
        seg.setOptimizeCoefficients(std::atoi(argv[6]) != 0);
        const float z[3] = {0.f, 0.f, 1.f};
        seg.setAxis(z);                                  // (ignored by SACMODEL_PLANE, as in PCL)
        seg.setEpsAngle(std::atof(argv[8]));

        rsreg::PointIndices host, device;
        rsreg::ModelCoefficients host_c, device_c;
        seg.setInputCloud(cloud);
        seg.segment(host, host_c);
        rsreg::DeviceCloud<Point> dev(*cloud);
        seg.setInputCloud(dev);
        seg.segment(device, device_c);
        save(host.indices, prefix + "host_inliers.bin");
        save(host_c.values, prefix + "host_coeff.bin");
        save(device.indices, prefix + "dev_inliers.bin");
        save(device_c.values, prefix + "dev_coeff.bin");

        rsreg::ExtractIndices<Point> ex;
        ex.setInputCloud(cloud);
        ex.setIndices(host);
        Cloud plane, rest;
        ex.filter(plane);
        ex.setNegative(true);
        ex.filter(rest);
        save_cloud(plane, prefix + "host_plane.bin");
        save_cloud(rest, prefix + "host_rest.bin");
        rsreg::DeviceCloud<Point> dplane, drest;
        ex.filter(dev, drest);
        ex.setNegative(false);
        ex.filter(dev, dplane);
        Cloud back;
        dplane.download(back);
        save_cloud(back, prefix + "dev_plane.bin");
        drest.download(back);
        save_cloud(back, prefix + "dev_rest.bin");
        std::printf("inliers %zu\ninliers_device %zu\nrest %zu\niterations %d\nskipped %d\n", host.indices.size(), device.indices.size(), rest.size(),
                    seg.result().iterations, seg.result().skipped);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
