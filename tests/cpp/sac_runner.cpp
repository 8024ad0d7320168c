// sac_runner — pcl::registration::CorrespondenceRejectorSampleConsensus and TransformationEstimationSVD through the C++ adaptor
// (include/rsreg/pcl_compat.hpp), for tests/test_sac_gpu.py: the fourth step of a feature-based pre-alignment.
//   sac_runner <source.bin> <target.bin> <corr.bin> <threshold> <max_iterations> <seed> <refine 0|1> <out_prefix>
// source, target: 32-byte PointXYZRGB records; corr: 12-byte Correspondence records.  Writes the kept list and the best
// transformation (16 floats, column-major) from host clouds -- <out_prefix>kept_host.bin, t_host.bin -- and from clouds that stay in
// HBM -- kept_device.bin, t_device.bin -- and the SVD fit over the kept list, svd.bin.  Prints the two sizes.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>

#include "rsreg/pcl_compat.hpp"

using Point = rsreg::PointXYZRGB;
using Cloud = rsreg::PointCloud<Point>;
using Rejector = rsreg::registration::CorrespondenceRejectorSampleConsensus<Point>;

template <typename T, typename Vec> static void load(const char *path, Vec &out)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    out.resize((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char *>(out.data()), (std::streamsize)(out.size() * sizeof(T)));
    if (!f) throw std::runtime_error("short input file");
}

static Cloud::Ptr load_cloud(const char *path)
{
    Cloud::Ptr c(new Cloud);
    load<Point>(path, c->points);
    c->width = (uint32_t)c->points.size();
    c->height = 1;
    c->is_dense = false;
    return c;
}

static void save(const void *p, size_t bytes, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char *>(p), (std::streamsize)bytes);
}

static void configure(Rejector &r, char **argv)
{
    r.setInlierThreshold(std::atof(argv[4]));
    r.setMaximumIterations(std::atoi(argv[5]));
    r.setSeed(std::strtoull(argv[6], nullptr, 10));
    r.setRefineModel(std::atoi(argv[7]) != 0);
}

int main(int argc, char **argv)
{
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <source.bin> <target.bin> <corr.bin> <threshold> <max_iterations> <seed> <refine> <out_prefix>\n", argv[0]);
        return 2;
    }
    try {
        const Cloud::Ptr source = load_cloud(argv[1]), target = load_cloud(argv[2]);
        std::shared_ptr<rsreg::Correspondences> corr(new rsreg::Correspondences);
        load<rsreg::Correspondence>(argv[3], *corr);
        const std::string prefix = argv[8];
        rsreg::Correspondences kept, kept_dev;
        Rejector host;
        configure(host, argv);
        host.setInputSource(source);
        host.setInputTarget(target);
        host.setInputCorrespondences(corr);
        host.getCorrespondences(kept);
        const rsreg::Matrix4f t_host = host.getBestTransformation();
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<Point> dsource(*source), dtarget(*target);
        Rejector dev;
        configure(dev, argv);
        dev.setInputSource(dsource);
        dev.setInputTarget(dtarget);
        dev.getRemainingCorrespondences(*corr, kept_dev);
        const rsreg::Matrix4f t_dev = dev.getBestTransformation();
        rsreg::Matrix4f svd = rsreg::Matrix4f::Identity();
        rsreg::registration::TransformationEstimationSVD<Point> est;
        est.estimateRigidTransformation(*source, *target, kept, svd);
        save(kept.data(), kept.size() * sizeof(rsreg::Correspondence), prefix + "kept_host.bin");
        save(kept_dev.data(), kept_dev.size() * sizeof(rsreg::Correspondence), prefix + "kept_device.bin");
        save(t_host.data(), 64, prefix + "t_host.bin");
        save(t_dev.data(), 64, prefix + "t_device.bin");
        save(svd.data(), 64, prefix + "svd.bin");
        std::printf("kept_host %zu\nkept_device %zu\n", kept.size(), kept_dev.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
