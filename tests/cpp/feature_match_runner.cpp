// feature_match_runner — pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> through the C++ adaptor
// (include/rsreg/pcl_compat.hpp), for tests/test_feature_match_gpu.py: the third step of a feature-based pre-alignment.
//   feature_match_runner <source.bin> <target.bin> <max_distance | max> <out_prefix>
// source, target: 132-byte FPFHSignature33 records.  Writes the forward and the reciprocal list (12-byte Correspondence records) from
// host clouds -- <out_prefix>fwd_host.bin, rec_host.bin -- and from clouds that stay in HBM -- fwd_device.bin, rec_device.bin.  Prints the
// four sizes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>

#include "rsreg/pcl_compat.hpp"

using Features = rsreg::PointCloud<rsreg::FPFHSignature33>;
using Matcher = rsreg::registration::CorrespondenceEstimation<rsreg::FPFHSignature33, rsreg::FPFHSignature33>;

static Features::Ptr load(const char *path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    Features::Ptr c(new Features);
    c->points.resize((size_t)bytes / sizeof(rsreg::FPFHSignature33));
    c->width = (uint32_t)c->points.size();
    c->height = 1;
    c->is_dense = false;
    f.read(reinterpret_cast<char *>(c->points.data()), (std::streamsize)(c->points.size() * sizeof(rsreg::FPFHSignature33)));
    if (!f) throw std::runtime_error("short input file");
    return c;
}

static void save(const rsreg::Correspondences &c, const std::string &path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.data()), (std::streamsize)(c.size() * sizeof(rsreg::Correspondence)));
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <source.bin> <target.bin> <max_distance | max> <out_prefix>\n", argv[0]);
        return 2;
    }
    try {
        const Features::Ptr source = load(argv[1]), target = load(argv[2]);
        const bool dflt = std::strcmp(argv[3], "max") == 0;
        const double max_distance = dflt ? std::numeric_limits<double>::max() : std::atof(argv[3]);
        const std::string prefix = argv[4];
        rsreg::Correspondences fwd, rec, fwd_dev, rec_dev;
        Matcher host;
        host.setInputSource(source);
        host.setInputTarget(target);
        if (dflt) {   // PCL's default argument
            host.determineCorrespondences(fwd);
            host.determineReciprocalCorrespondences(rec);
        } else {
            host.determineCorrespondences(fwd, max_distance);
            host.determineReciprocalCorrespondences(rec, max_distance);
        }
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<rsreg::FPFHSignature33> dsource(*source), dtarget(*target);
        Matcher dev;
        dev.setInputSource(dsource);
        dev.setInputTarget(dtarget);
        dev.determineCorrespondences(fwd_dev, max_distance);
        dev.determineReciprocalCorrespondences(rec_dev, max_distance);
        save(fwd, prefix + "fwd_host.bin");
        save(rec, prefix + "rec_host.bin");
        save(fwd_dev, prefix + "fwd_device.bin");
        save(rec_dev, prefix + "rec_device.bin");
        std::printf("fwd_host %zu\nrec_host %zu\nfwd_device %zu\nrec_device %zu\n", fwd.size(), rec.size(), fwd_dev.size(), rec_dev.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
