// gicp6d_runner — pcl::GeneralizedIterativeClosestPoint6D through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_gicp6d_cpp.py: GICP over correspondences in (x, y, z, w L', w a', w b').
//   gicp6d_runner <source.bin> <n_source> <target.bin> <n_target> <source_cov.bin> <target_cov.bin> <source_lab.bin> <target_lab.bin>
//                 <gate> <epsilon> <lab_weight>
// source, target: 32-byte PointXYZRGB records; the covariance files: six doubles a record; the colour files: three floats a record.
// Route "given": setSourceLab / setTargetLab with the files' records.  Route "computed": none are given, the class converts the
// clouds' own rgb words.  Prints the sixteen floats of each final transformation (column-major) as hexadecimal words, with the
// iteration, evaluation and pair counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Gicp6d = rsreg::GeneralizedIterativeClosestPoint6D<rsreg::PointXYZRGB, rsreg::PointXYZRGB>;

template <typename Vec> static void read_records(Vec &v, const char *path, size_t n)
{
    v.resize(n);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * sizeof(v[0])));
    if (!f) throw std::runtime_error("short input file");
}

static void load(Cloud &c, const char *path, size_t n)
{
    c.width = (uint32_t)n;
    c.height = 1;
    c.is_dense = false;
    read_records(c.points, path, n);
}

int main(int argc, char **argv)
{
    if (argc < 12) {
        std::fprintf(stderr, "usage: %s <source.bin> <n_source> <target.bin> <n_target> <source_cov.bin> <target_cov.bin> <source_lab.bin> <target_lab.bin> "
                             "<gate> <epsilon> <lab_weight>\n", argv[0]);
        return 2;
    }
    try {
        Cloud::Ptr src(new Cloud), tgt(new Cloud);
        load(*src, argv[1], (size_t)std::atol(argv[2]));
        load(*tgt, argv[3], (size_t)std::atol(argv[4]));
        auto cs = std::make_shared<rsreg::GicpCovariances>(), ct = std::make_shared<rsreg::GicpCovariances>();
        read_records(*cs, argv[5], src->size());
        read_records(*ct, argv[6], tgt->size());
        auto ls = std::make_shared<rsreg::LabColours>(), lt = std::make_shared<rsreg::LabColours>();
        read_records(*ls, argv[7], src->size());
        read_records(*lt, argv[8], tgt->size());
        const double gate = std::atof(argv[9]), epsilon = std::atof(argv[10]);
        const float weight = (float)std::atof(argv[11]);
        for (int route = 0; route < 2; ++route) {
            Gicp6d gicp(weight);
            gicp.setMaxCorrespondenceDistance(gate);
            gicp.setTransformationEpsilon(epsilon);
            gicp.setRotationEpsilon(epsilon);
            gicp.setMaximumIterations(60);
            gicp.setMaximumOptimizerIterations(20);
            gicp.setInputSource(src);
            gicp.setInputTarget(tgt);
            gicp.setSourceCovariances(cs);
            gicp.setTargetCovariances(ct);
            if (route == 0) {
                gicp.setSourceLab(ls);
                gicp.setTargetLab(lt);
            }
            Cloud aligned;
            gicp.align(aligned);
            if (aligned.size() != src->size()) throw std::runtime_error("aligned cloud: wrong size");
            if (aligned[0].rgba != (*src)[0].rgba) throw std::runtime_error("aligned cloud: the colours are not the source's");
            const rsreg::Matrix4f T = gicp.getFinalTransformation();
            std::printf("%s", route == 0 ? "given" : "computed");
            for (int i = 0; i < 16; ++i) {
                uint32_t w;
                std::memcpy(&w, T.data() + i, 4);
                std::printf(" %08x", w);
            }
            std::printf(" iterations %d evaluations %d pairs %llu converged %d\n", gicp.result().iterations, gicp.result().inner_evaluations,
                        (unsigned long long)gicp.result().n_correspondences, gicp.hasConverged() ? 1 : 0);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
