// plane_runner — pcl::IterativeClosestPointWithNormals through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_plane_cpp_gpu.py: point-to-plane ICP, 5 cm gate, exactly <iterations> iterations.
//   plane_runner <source.bin> <n_source> <target.bin> <n_target> <normals.bin> <k> <iterations>
// source, target: 32-byte PointXYZRGB records; normals: 32-byte Normal records of the target.
// Route "records": IterativeClosestPointWithNormals<PointXYZRGBNormal, PointXYZRGBNormal> on host clouds whose 48-byte records
// carry the normals.  Route "device": NormalEstimation (k) -> setInputTargetNormals on clouds that stay in HBM.  Prints the
// sixteen floats of each final transformation (column-major) as hexadecimal words, with the iteration and pair counts.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using NCloud = rsreg::PointCloud<rsreg::PointXYZRGBNormal>;
using Normals = rsreg::PointCloud<rsreg::Normal>;

template <typename CloudT> static void load(CloudT &c, const char *path, size_t n)
{
    c.width = (uint32_t)n;
    c.height = 1;
    c.is_dense = false;
    c.points.resize(n);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(c.points.data()), (std::streamsize)(n * sizeof(c.points[0])));
    if (!f) throw std::runtime_error("short input file");
}

static NCloud::Ptr with_normals(const Cloud &c, const Normals *n)
{
    NCloud::Ptr out(new NCloud);
    out->width = c.width;
    out->height = c.height;
    out->is_dense = c.is_dense;
    out->points.resize(c.size());
    for (size_t i = 0; i < c.size(); ++i) {
        rsreg::PointXYZRGBNormal &p = out->points[i];
        p.x = c[i].x; p.y = c[i].y; p.z = c[i].z;
        p.rgba = c[i].rgba;
        if (n) { p.normal_x = (*n)[i].normal_x; p.normal_y = (*n)[i].normal_y; p.normal_z = (*n)[i].normal_z; p.curvature = (*n)[i].curvature; }
    }
    return out;
}

template <typename Icp> static void report(const char *route, const Icp &icp)
{
    const rsreg::Matrix4f T = icp.getFinalTransformation();
    std::printf("%s", route);
    for (int i = 0; i < 16; ++i) {
        uint32_t w;
        std::memcpy(&w, T.data() + i, 4);
        std::printf(" %08x", w);
    }
    std::printf(" iterations %d pairs %llu\n", icp.result().iterations, (unsigned long long)icp.result().n_correspondences);
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <source.bin> <n_source> <target.bin> <n_target> <normals.bin> <k> <iterations>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr src(new Cloud), tgt(new Cloud);
        Normals nrm;
        load(*src, argv[1], (size_t)std::atol(argv[2]));
        load(*tgt, argv[3], (size_t)std::atol(argv[4]));
        load(nrm, argv[5], tgt->size());
        const int k = std::atoi(argv[6]), iterations = std::atoi(argv[7]);
        {
            rsreg::IterativeClosestPointWithNormals<rsreg::PointXYZRGBNormal, rsreg::PointXYZRGBNormal> icp;
            icp.setMaxCorrespondenceDistance(0.05);
            icp.setMaximumIterations(iterations);
            icp.setFixedIterationCount(true);
            icp.setInputSource(with_normals(*src, nullptr));
            icp.setInputTarget(with_normals(*tgt, &nrm));
            NCloud aligned;
            icp.align(aligned);
            if (aligned.size() != src->size()) throw std::runtime_error("aligned cloud: wrong size");
            report("records", icp);
        }
        {
            rsreg::DeviceCloud<rsreg::PointXYZRGB> dsrc(*src), dtgt(*tgt), aligned;
            rsreg::DeviceCloud<rsreg::Normal> dnrm;
            rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> ne(rsreg::Context::Default());
            ne.setKSearch(k);
            ne.compute(dtgt, dnrm);
            rsreg::IterativeClosestPointWithNormals<rsreg::PointXYZRGB, rsreg::PointXYZRGB> icp;
            icp.setMaxCorrespondenceDistance(0.05);
            icp.setMaximumIterations(iterations);
            icp.setFixedIterationCount(true);
            icp.setInputSource(dsrc);
            icp.setInputTarget(dtgt);
            icp.setInputTargetNormals(dnrm);
            icp.align(aligned);
            report("device", icp);
            std::printf("fitness %.17g\n", icp.getFitnessScore(0.0025));
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
