// gicp_runner — pcl::GeneralizedIterativeClosestPoint through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_gicp_cpp.py: plane-to-plane ICP at the gate and the epsilons given.
//   gicp_runner <source.bin> <n_source> <target.bin> <n_target> <source_cov.bin> <target_cov.bin> <gate> <epsilon> <k>
// source, target: 32-byte PointXYZRGB records; the covariance files: six doubles a record.
// Route "given": setSourceCovariances / setTargetCovariances with the files' records.  Route "computed": none are given, the
// class computes them itself (setCorrespondenceRandomness(k)) as PCL does.  Prints the sixteen floats of each final
// transformation (column-major) as hexadecimal words, with the iteration, evaluation and pair counts, and the fitness score.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Gicp = rsreg::GeneralizedIterativeClosestPoint<rsreg::PointXYZRGB, rsreg::PointXYZRGB>;

template <typename T> static void read_records(std::vector<T> &v, const char *path, size_t n)
{
    v.resize(n);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * sizeof(T)));
    if (!f) throw std::runtime_error("short input file");
}

static void load(Cloud &c, const char *path, size_t n)
{
    c.width = (uint32_t)n;
    c.height = 1;
    c.is_dense = false;
    c.points.resize(n);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(c.points.data()), (std::streamsize)(n * sizeof(c.points[0])));
    if (!f) throw std::runtime_error("short input file");
}

static void report(const char *route, Gicp &gicp)
{
    const rsreg::Matrix4f T = gicp.getFinalTransformation();
    std::printf("%s", route);
    for (int i = 0; i < 16; ++i) {
        uint32_t w;
        std::memcpy(&w, T.data() + i, 4);
        std::printf(" %08x", w);
    }
    std::printf(" iterations %d evaluations %d pairs %llu converged %d fitness %.17g\n", gicp.result().iterations, gicp.result().inner_evaluations,
                (unsigned long long)gicp.result().n_correspondences, gicp.hasConverged() ? 1 : 0, gicp.getFitnessScore(0.0025));
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <source.bin> <n_source> <target.bin> <n_target> <source_cov.bin> <target_cov.bin> <gate> <epsilon> <k>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr src(new Cloud), tgt(new Cloud);
        load(*src, argv[1], (size_t)std::atol(argv[2]));
        load(*tgt, argv[3], (size_t)std::atol(argv[4]));
        auto cs = std::make_shared<rsreg::GicpCovariances>(), ct = std::make_shared<rsreg::GicpCovariances>();
        read_records(*cs, argv[5], src->size());
        read_records(*ct, argv[6], tgt->size());
        const double gate = std::atof(argv[7]), epsilon = std::atof(argv[8]);
        const int k = std::atoi(argv[9]);
        for (int route = 0; route < 2; ++route) {
            Gicp gicp;
            gicp.setMaxCorrespondenceDistance(gate);
            gicp.setTransformationEpsilon(epsilon);
            gicp.setRotationEpsilon(epsilon);
            gicp.setMaximumIterations(60);
            gicp.setMaximumOptimizerIterations(20);
            gicp.setCorrespondenceRandomness(k);
            gicp.setInputSource(src);
            gicp.setInputTarget(tgt);
            if (route == 0) {
                gicp.setSourceCovariances(cs);
                gicp.setTargetCovariances(ct);
            }
            Cloud aligned;
            gicp.align(aligned);
            if (aligned.size() != src->size()) throw std::runtime_error("aligned cloud: wrong size");
            report(route == 0 ? "given" : "computed", gicp);
            if (route == 0) {   // the aligned cloud: the source's colours, xyz under the final transformation
                const rsreg::Matrix4f T = gicp.getFinalTransformation();
                const float *m = T.data();
                const rsreg::PointXYZRGB &p = (*src)[0], &a = aligned[0];
                const float x = ((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12];
                if (a.rgba != p.rgba || !(std::fabs(a.x - x) <= 1e-5f)) throw std::runtime_error("aligned cloud: first record is not the source's under T");
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
