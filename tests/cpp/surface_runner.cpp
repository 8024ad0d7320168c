// surface_runner — pcl::NormalEstimation and pcl::FPFHEstimationOMP with setSearchSurface and setRadiusSearch through the C++
// adaptor (include/rsreg/pcl_compat.hpp), for tests/test_surface_gpu.py.
//   surface_runner <queries.bin> <nq> <surface.bin> <width> <height> <radius_normals> <radius> <out_dir>
//   surface_runner refuse     compute() with a search surface and setKSearch: refused as not built, no device call is made
// queries, surface: 32-byte PointXYZRGB records.  The surface's normals come from NormalEstimation on the surface itself; then the
// normals and the descriptors of the queries over the surface, once from host clouds and once from clouds that stay in HBM:
// <out_dir>/normals_host.bin, normals_dev.bin (32-byte pcl::Normal records), fpfh_host.bin, fpfh_dev.bin (132-byte records).
// Prints the size, width, height and is_dense of the results.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Normals = rsreg::PointCloud<rsreg::Normal>;
using Features = rsreg::PointCloud<rsreg::FPFHSignature33>;
using NormalEstimator = rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal>;
using Estimator = rsreg::FPFHEstimationOMP<rsreg::PointXYZRGB, rsreg::Normal, rsreg::FPFHSignature33>;

template <typename CloudT> static void save(const CloudT &c, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(c.points[0])));
}

static Cloud::Ptr load(const char *path, uint32_t width, uint32_t height)
{
    Cloud::Ptr c(new Cloud);
    c->width = width;
    c->height = height;
    c->is_dense = true;
    c->points.resize((size_t)width * height);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(c->points.data()), (std::streamsize)(c->size() * sizeof(rsreg::PointXYZRGB)));
    if (!f) throw std::runtime_error("short input file");
    return c;
}

// 0 when compute() throws RSREG_ERR_INVALID_ARG with `word` in its message
template <typename E, typename Out> static int refused(E &est, const char *word)
{
    try {
        Out out;
        est.compute(out);
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
        NormalEstimator ne;
        ne.setInputCloud(one);
        ne.setSearchSurface(one);
        ne.setKSearch(10);
        int bad = refused<NormalEstimator, Normals>(ne, "not built");
        Estimator fe;
        fe.setInputCloud(one);
        fe.setSearchSurface(one);
        fe.setInputNormals(normal);
        fe.setKSearch(10);
        bad += refused<Estimator, Features>(fe, "not built");
        std::printf("refused %s\n", bad ? "no" : "yes");
        return bad ? 1 : 0;
    }
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <queries.bin> <nq> <surface.bin> <width> <height> <radius_normals> <radius> <out_dir> | refuse\n", argv[0]);
        return 2;
    }
    try {
        const std::string dir = argv[8];
        Cloud::Ptr queries = load(argv[1], (uint32_t)std::atoi(argv[2]), 1);
        Cloud::Ptr surface = load(argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]));
        const double radius_normals = std::atof(argv[6]), radius = std::atof(argv[7]);
        NormalEstimator ne;
        ne.setInputCloud(surface);
        ne.setRadiusSearch(radius_normals);
        Normals::Ptr surface_normals(new Normals);
        ne.compute(*surface_normals);
        // from host clouds
        ne.setInputCloud(queries);
        ne.setSearchSurface(surface);
        Normals query_normals;
        ne.compute(query_normals);
        save(query_normals, dir + "/normals_host.bin");
        Estimator fe;
        fe.setInputCloud(queries);
        fe.setSearchSurface(surface);
        fe.setInputNormals(surface_normals);
        fe.setRadiusSearch(radius);
        Features host;
        fe.compute(host);
        save(host, dir + "/fpfh_host.bin");
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev_queries(*queries), dev_surface(*surface);
        rsreg::DeviceCloud<rsreg::Normal> dev_surface_normals(*surface_normals), dev_query_normals;
        ne.setSearchSurface(dev_surface);
        ne.compute(dev_queries, dev_query_normals);
        Normals out_normals;
        dev_query_normals.download(out_normals);
        save(out_normals, dir + "/normals_dev.bin");
        fe.setSearchSurface(dev_surface);
        rsreg::DeviceCloud<rsreg::FPFHSignature33> dev_features;
        fe.compute(dev_queries, dev_surface_normals, dev_features);
        Features out;
        dev_features.download(out);
        save(out, dir + "/fpfh_dev.bin");
        std::printf("size %zu\nsize_device %zu\nsize_normals %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\ndense_normals %d\n", host.size(), out.size(),
                    query_normals.size(), host.width, host.height, (int)host.is_dense, (int)out.is_dense, (int)query_normals.is_dense);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
