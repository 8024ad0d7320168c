// iinormals_runner — pcl::IntegralImageNormalEstimation through the C++ adaptor (include/rsreg/pcl_compat.hpp), set up as the
// surveyed edge extractor sets it up (src/edge_extractor.hpp:9-15), for tests/test_iinormals_gpu.py.
//   iinormals_runner <in.bin> <width> <height> <factor> <smoothing> <vx> <vy> <vz> <out_host.bin> <out_device.bin>
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
    if (argc < 11) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <factor> <smoothing> <vx> <vy> <vz> <out_host.bin> <out_device.bin>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr cloud(new Cloud);
        cloud->width = (uint32_t)std::atoi(argv[2]);
        cloud->height = (uint32_t)std::atoi(argv[3]);
        cloud->is_dense = false;
        cloud->points.resize((size_t)cloud->width * cloud->height);
        std::ifstream f(argv[1], std::ios::binary);
        f.read(reinterpret_cast<char *>(cloud->points.data()), (std::streamsize)(cloud->size() * sizeof(rsreg::PointXYZRGB)));
        if (!f) throw std::runtime_error("short input file");
        Normals::Ptr normals(new Normals);
        rsreg::IntegralImageNormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> ne;
        ne.setNormalEstimationMethod(ne.AVERAGE_3D_GRADIENT);
        ne.setMaxDepthChangeFactor((float)std::atof(argv[4]));
        ne.setNormalSmoothingSize((float)std::atof(argv[5]));
        ne.setViewPoint((float)std::atof(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8]));
        ne.setInputCloud(cloud);
        ne.compute(*normals);
        save(*normals, argv[9]);
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*cloud);
        rsreg::DeviceCloud<rsreg::Normal> dev_normals;
        ne.compute(dev, dev_normals);
        Normals out;
        dev_normals.download(out);
        save(out, argv[10]);
        std::printf("size %zu\nsize_device %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\n", normals->size(), out.size(), normals->width,
                    normals->height, (int)normals->is_dense, (int)out.is_dense);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
