// scia_runner — pcl::SampleConsensusInitialAlignment through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_scia_cpp_gpu.py: the pose from descriptor neighbours, every hypothesis scored over every source record.
//   scia_runner <source.bin> <target.bin> <source_features.bin> <target_features.bin> <max_correspondence_distance> <max_iterations>
//               <seed> <k> <nr_samples> <min_sample_distance> <huber 0|1> <guess.bin or -> <out_prefix>
// source, target: 32-byte PointXYZRGB records; features: 132-byte FPFHSignature33 records; guess: 16 floats, column-major.
// Writes the final transformation (16 floats, column-major) and the aligned source from host clouds -- <out_prefix>t_host.bin,
// aligned_host.bin -- and from clouds that stay in HBM -- t_device.bin, aligned_device.bin.  Prints what hasConverged, the fitness
// score and the result's winner say.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>

#include "rsreg/pcl_compat.hpp"

using Point = rsreg::PointXYZRGB;
using Feature = rsreg::FPFHSignature33;
using Cloud = rsreg::PointCloud<Point>;
using Features = rsreg::PointCloud<Feature>;
using Align = rsreg::SampleConsensusInitialAlignment<Point, Point, Feature>;

template <typename CloudT> static typename CloudT::Ptr load_cloud(const char *path)
{
    typename CloudT::Ptr c(new CloudT);
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    c->points.resize((size_t)bytes / sizeof(c->points[0]));
    f.read(reinterpret_cast<char *>(c->points.data()), (std::streamsize)(c->points.size() * sizeof(c->points[0])));
    if (!f) throw std::runtime_error("short input file");
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

static void configure(Align &a, char **argv)
{
    a.setMaxCorrespondenceDistance(std::atof(argv[5]));
    a.setMaximumIterations(std::atoi(argv[6]));
    a.setSeed(std::strtoull(argv[7], nullptr, 10));
    a.setCorrespondenceRandomness(std::atoi(argv[8]));
    a.setNumberOfSamples(std::atoi(argv[9]));
    a.setMinSampleDistance((float)std::atof(argv[10]));
    a.setErrorFunction(std::atoi(argv[11]) ? Align::HUBER_PENALTY : Align::TRUNCATED_ERROR);
}

int main(int argc, char **argv)
{
    if (argc < 14) {
        std::fprintf(stderr, "usage: %s <source.bin> <target.bin> <source_features.bin> <target_features.bin> <max_correspondence_distance> <max_iterations> <seed> <k> "
                             "<nr_samples> <min_sample_distance> <huber> <guess.bin or -> <out_prefix>\n", argv[0]);
        return 2;
    }
    try {
        const Cloud::Ptr source = load_cloud<Cloud>(argv[1]), target = load_cloud<Cloud>(argv[2]);
        const Features::Ptr sfeat = load_cloud<Features>(argv[3]), tfeat = load_cloud<Features>(argv[4]);
        const bool with_guess = std::strcmp(argv[12], "-") != 0;
        rsreg::Matrix4f guess = rsreg::Matrix4f::Identity();
        if (with_guess) {
            std::ifstream f(argv[12], std::ios::binary);
            f.read(reinterpret_cast<char *>(guess.data()), 64);
            if (!f) throw std::runtime_error("short guess file");
        }
        const std::string prefix = argv[13];
        Align host;
        configure(host, argv);
        host.setInputSource(source);
        host.setInputTarget(target);
        host.setSourceFeatures(sfeat);
        host.setTargetFeatures(tfeat);
        Cloud aligned;
        if (with_guess) host.align(aligned, guess); else host.align(aligned);
        const rsreg::Matrix4f t_host = host.getFinalTransformation();
        // the same on clouds that stay in HBM
        rsreg::DeviceCloud<Point> dsource(*source), dtarget(*target), daligned;
        rsreg::DeviceCloud<Feature> dsfeat(*sfeat), dtfeat(*tfeat);
        Align dev;
        configure(dev, argv);
        dev.setInputSource(dsource);
        dev.setInputTarget(dtarget);
        dev.setSourceFeatures(dsfeat);
        dev.setTargetFeatures(dtfeat);
        if (with_guess) dev.align(daligned, guess); else dev.align(daligned);
        Cloud aligned_dev;
        daligned.download(aligned_dev);
        const rsreg::Matrix4f t_dev = dev.getFinalTransformation();
        bool threw = false;
        try {   // (a third object: a refused call leaves no result behind)
            Align nine;
            configure(nine, argv);
            nine.setInputSource(dsource);
            nine.setInputTarget(dtarget);
            nine.setSourceFeatures(dsfeat);
            nine.setTargetFeatures(dtfeat);
            nine.setNumberOfSamples(9);
            rsreg::DeviceCloud<Point> unused;
            nine.align(unused);
        } catch (const std::exception &) {
            threw = true;
        }
        save(t_host.data(), 64, prefix + "t_host.bin");
        save(t_dev.data(), 64, prefix + "t_device.bin");
        save(aligned.points.data(), aligned.points.size() * sizeof(Point), prefix + "aligned_host.bin");
        save(aligned_dev.points.data(), aligned_dev.points.size() * sizeof(Point), prefix + "aligned_device.bin");
        std::printf("converged_host %d\nconverged_device %d\nfitness_host %.17g\nfitness_device %.17g\nwinner_host %d\nwinner_device %d\nvalid_host %llu\n"
                    "valid_device %llu\nrefused_9_samples %d\n",
                    (int)host.hasConverged(), (int)dev.hasConverged(), host.getFitnessScore(), dev.getFitnessScore(), host.getResult().best_hypothesis,
                    dev.getResult().best_hypothesis, (unsigned long long)host.getResult().n_valid, (unsigned long long)dev.getResult().n_valid, (int)threw);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
