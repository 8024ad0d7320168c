// rejector_runner — Registration::addCorrespondenceRejector through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_rejectors_cpp_gpu.py: 5 cm gate, exactly <iterations> iterations, no guess.
//   rejector_runner <source.bin> <n_source> <target.bin> <n_target> <source_normals.bin> <target_normals.bin> <iterations>
// source, target: 32-byte PointXYZRGB records; the normals: 32-byte Normal records, one per record of their cloud.
// Route "points":  IterativeClosestPoint<PointXYZRGB, PointXYZRGB> with [OneToOne, MedianDistance].
// Route "normals": IterativeClosestPoint<PointXYZRGBNormal, PointXYZRGBNormal> with [SurfaceNormal 0.7, MedianDistance 1.5]: both
//                  clouds hand over the normals inside their 48-byte records.
// Route "beside":  IterativeClosestPointWithNormals<PointXYZRGB, PointXYZRGB> with [SurfaceNormal 0.7, Trimmed 0.8]: the normals
//                  beside the clouds (setInputSourceNormals, setInputTargetNormals), point-to-plane estimation.
// Prints per route the sixteen floats of the final transformation (column-major) as hexadecimal words, the iteration and pair
// counts, and per rejector of the chain "n_in n_out median" of the last iteration.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using NCloud = rsreg::PointCloud<rsreg::PointXYZRGBNormal>;
using Normals = rsreg::PointCloud<rsreg::Normal>;
namespace reg = rsreg::registration;

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

static NCloud::Ptr with_normals(const Cloud &c, const Normals &n)
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
        p.normal_x = n[i].normal_x; p.normal_y = n[i].normal_y; p.normal_z = n[i].normal_z; p.curvature = n[i].curvature;
    }
    return out;
}

template <typename Icp> static void setup(Icp &icp, int iterations)
{
    icp.setMaxCorrespondenceDistance(0.05);
    icp.setMaximumIterations(iterations);
    icp.setFixedIterationCount(true);
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
    std::printf(" iterations %d pairs %llu", icp.result().iterations, (unsigned long long)icp.result().n_correspondences);
    for (const auto &r : icp.getCorrespondenceRejectors())
        std::printf(" | %llu %llu %.17g", (unsigned long long)r->stat().n_in, (unsigned long long)r->stat().n_out, r->stat().median_distance);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <source.bin> <n_source> <target.bin> <n_target> <source_normals.bin> <target_normals.bin> <iterations>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr src(new Cloud), tgt(new Cloud);
        Normals src_n, tgt_n;
        load(*src, argv[1], (size_t)std::atol(argv[2]));
        load(*tgt, argv[3], (size_t)std::atol(argv[4]));
        load(src_n, argv[5], src->size());
        load(tgt_n, argv[6], tgt->size());
        const int iterations = std::atoi(argv[7]);
        {
            rsreg::IterativeClosestPoint<rsreg::PointXYZRGB, rsreg::PointXYZRGB> icp;
            setup(icp, iterations);
            reg::CorrespondenceRejectorTrimmed::Ptr trimmed(new reg::CorrespondenceRejectorTrimmed);
            reg::CorrespondenceRejectorOneToOne::Ptr one(new reg::CorrespondenceRejectorOneToOne);
            reg::CorrespondenceRejectorMedianDistance::Ptr median(new reg::CorrespondenceRejectorMedianDistance);
            if (median->getMedianFactor() != 1.0 || trimmed->getOverlapRatio() != 0.5) throw std::runtime_error("defaults");
            icp.addCorrespondenceRejector(trimmed);
            icp.addCorrespondenceRejector(one);
            icp.addCorrespondenceRejector(median);
            if (!icp.removeCorrespondenceRejector(0) || icp.removeCorrespondenceRejector(7) || icp.getCorrespondenceRejectors().size() != 2)
                throw std::runtime_error("removeCorrespondenceRejector");
            icp.setInputSource(src);
            icp.setInputTarget(tgt);
            Cloud aligned;
            icp.align(aligned);
            if (aligned.size() != src->size()) throw std::runtime_error("aligned cloud: wrong size");
            report("points", icp);
            std::printf("median %.17g\n", median->getMedianDistance());
            icp.clearCorrespondenceRejectors();   // no chain: the plain alignment again
            icp.align(aligned);
            report("plain", icp);
        }
        {
            rsreg::IterativeClosestPoint<rsreg::PointXYZRGBNormal, rsreg::PointXYZRGBNormal> icp;
            setup(icp, iterations);
            reg::CorrespondenceRejectorSurfaceNormal::Ptr normal(new reg::CorrespondenceRejectorSurfaceNormal);
            reg::CorrespondenceRejectorMedianDistance::Ptr median(new reg::CorrespondenceRejectorMedianDistance);
            if (normal->getThreshold() != 1.0) throw std::runtime_error("defaults");
            normal->setThreshold(0.7);
            median->setMedianFactor(1.5);
            icp.addCorrespondenceRejector(normal);
            icp.addCorrespondenceRejector(median);
            icp.setInputSource(with_normals(*src, src_n));
            icp.setInputTarget(with_normals(*tgt, tgt_n));
            NCloud aligned;
            icp.align(aligned);
            report("normals", icp);
        }
        {
            rsreg::IterativeClosestPointWithNormals<rsreg::PointXYZRGB, rsreg::PointXYZRGB> icp;
            setup(icp, iterations);
            reg::CorrespondenceRejectorSurfaceNormal::Ptr normal(new reg::CorrespondenceRejectorSurfaceNormal);
            reg::CorrespondenceRejectorTrimmed::Ptr trimmed(new reg::CorrespondenceRejectorTrimmed);
            normal->setThreshold(0.7);
            trimmed->setOverlapRatio(0.8);
            icp.addCorrespondenceRejector(normal);
            icp.addCorrespondenceRejector(trimmed);
            icp.setInputSource(src);
            icp.setInputSourceNormals(src_n);
            icp.setInputTarget(tgt);
            icp.setInputTargetNormals(tgt_n);
            Cloud aligned;
            icp.align(aligned);
            report("beside", icp);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
