// fpfh_radius_runner — pcl::NormalEstimation (setRadiusSearch) -> pcl::FPFHEstimationOMP (setRadiusSearch) through the C++
// adaptor (include/rsreg/pcl_compat.hpp), for tests/test_fpfh_radius_gpu.py.
//   fpfh_radius_runner <in.bin> <width> <height> <radius_normals> <radius> <k> <out_host.bin> <out_device.bin> <out_k.bin>
//   fpfh_radius_runner refuse     FPFHEstimationOMP::compute with both searches set, then with neither: no device call is made
// in: 32-byte PointXYZRGB records; out: 132-byte FPFHSignature33 records by radius, once from host clouds and once from clouds that
// stay in HBM, and by k (the bytes of FPFHEstimation).  Prints the size, width, height and is_dense of the results.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Normals = rsreg::PointCloud<rsreg::Normal>;
using Features = rsreg::PointCloud<rsreg::FPFHSignature33>;
using Estimator = rsreg::FPFHEstimationOMP<rsreg::PointXYZRGB, rsreg::Normal, rsreg::FPFHSignature33>;

static void save(const Features &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::FPFHSignature33)));
}

// 0 when compute() throws RSREG_ERR_INVALID_ARG with `word` in its message
static int refused(Estimator &fe, const char *word)
{
    try {
        Features out;
        fe.compute(out);
    } catch (const rsreg::Error &e) {
        return e.status == RSREG_ERR_INVALID_ARG && std::strstr(e.what(), word) ? 0 : 1;
    }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "refuse") == 0) {
        Cloud::Ptr one(new Cloud);
        one->points.resize(1);
        one->width = one->height = 1;
        Normals::Ptr normal(new Normals);
        normal->points.resize(1);
        normal->width = normal->height = 1;
        Estimator fe;
        fe.setInputCloud(one);
        fe.setInputNormals(normal);
        int bad = refused(fe, "neither");
        fe.setKSearch(10);
        fe.setRadiusSearch(0.05);
        fe.setNumberOfThreads(8);
        bad += refused(fe, "both");
        fe.setKSearch(0);
        bad += fe.getRadiusSearch() == 0.05 && fe.getKSearch() == 0 ? 0 : 1;
        fe.setRadiusSearch(0);
        bad += refused(fe, "neither");
        std::printf("refused %s\n", bad ? "no" : "yes");
        return bad ? 1 : 0;
    }
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <radius_normals> <radius> <k> <out_host.bin> <out_device.bin> <out_k.bin> | refuse\n",
                     argv[0]);
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
        ne.setRadiusSearch(std::atof(argv[4]));
        Normals::Ptr normals(new Normals);
        ne.compute(*normals);
        Estimator fe;
        fe.setInputCloud(frame);
        fe.setInputNormals(normals);
        fe.setRadiusSearch(std::atof(argv[5]));
        fe.setNumberOfThreads(4);
        Features host;
        fe.compute(host);
        save(host, argv[7]);
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame);
        rsreg::DeviceCloud<rsreg::Normal> dev_normals;
        ne.compute(dev, dev_normals);
        rsreg::DeviceCloud<rsreg::FPFHSignature33> dev_features;
        fe.compute(dev, dev_normals, dev_features);
        Features out;
        dev_features.download(out);
        save(out, argv[8]);
        // by k: rsreg_cloud_fpfh
        const double radius = fe.getRadiusSearch();
        fe.setRadiusSearch(0.0);
        fe.setKSearch(std::atoi(argv[6]));
        Features by_k;
        fe.compute(by_k);
        save(by_k, argv[9]);
        std::printf("size %zu\nsize_device %zu\nsize_k %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\nradius %.17g\nk %d\n", host.size(), out.size(),
                    by_k.size(), host.width, host.height, (int)host.is_dense, (int)out.is_dense, radius, fe.getKSearch());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
