// voxelgrid_runner — rsreg::VoxelGrid through the C++ adaptor (include/rsreg/pcl_compat.hpp), for tests/test_voxelgrid_cpp_gpu.py.
//   voxelgrid_runner <in.bin> <n> <lx> <ly> <lz> <min_points> <out_host.bin> <out_gpu.bin> <out_device.bin>   (32-byte PointXYZRGB records)
// The same cloud three ways: the sequential host filter, the GPU filter of a host cloud (in place), the GPU filter of a device
// cloud (in place).  Prints the sizes and what getNrDivisions / getMinBoxCoordinates / getDivisionMultiplier return.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;

static void save(const Cloud &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::PointXYZRGB)));
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in.bin> <n> <lx> <ly> <lz> <min_points> <out_host.bin> <out_gpu.bin> <out_device.bin>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr cloud(new Cloud);
        cloud->width = (uint32_t)std::atoi(argv[2]);
        cloud->height = 1;
        cloud->is_dense = false;
        cloud->points.resize(cloud->width);
        std::ifstream f(argv[1], std::ios::binary);
        f.read(reinterpret_cast<char *>(cloud->points.data()), (std::streamsize)(cloud->size() * sizeof(rsreg::PointXYZRGB)));
        if (!f) throw std::runtime_error("short input file");
        const float lx = (float)std::atof(argv[3]), ly = (float)std::atof(argv[4]), lz = (float)std::atof(argv[5]);
        const unsigned min_points = (unsigned)std::atoi(argv[6]);

        rsreg::VoxelGrid<rsreg::PointXYZRGB> host;   // no context: the sequential restatement
        host.setInputCloud(cloud);
        if (lx == ly && ly == lz) host.setLeafSize(lx); else host.setLeafSize(lx, ly, lz);
        host.setMinimumPointsNumberPerVoxel(min_points);
        Cloud out_host;
        host.filter(out_host);
        save(out_host, argv[7]);

        rsreg::VoxelGrid<rsreg::PointXYZRGB> gpu(rsreg::Context::Default());
        Cloud::Ptr again(new Cloud(*cloud));
        gpu.setInputCloud(again);
        gpu.setLeafSize(lx, ly, lz);
        gpu.setMinimumPointsNumberPerVoxel(min_points);
        gpu.filter(*again);   // the output is the input
        save(*again, argv[8]);

        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*cloud);
        gpu.filter(dev, dev);
        Cloud out_dev;
        dev.download(out_dev);
        save(out_dev, argv[9]);

        const auto div = gpu.getNrDivisions(), mn = gpu.getMinBoxCoordinates(), mx = gpu.getMaxBoxCoordinates(), mul = gpu.getDivisionMultiplier();
        std::printf("host %zu\ngpu %zu\ndevice %zu\nwidth %u\nheight %u\ndense %d\n", out_host.size(), again->size(), out_dev.size(), out_dev.width,
                    out_dev.height, (int)out_dev.is_dense);
        std::printf("div_b %d,%d,%d\nmin_b %d,%d,%d\nmax_b %d,%d,%d\ndivb_mul %d,%d,%d\nleaves %llu\n", div[0], div[1], div[2], mn[0], mn[1], mn[2], mx[0],
                    mx[1], mx[2], mul[0], mul[1], mul[2], (unsigned long long)gpu.info().n_leaves);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
