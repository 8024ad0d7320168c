// cluster_runner — pcl::EuclideanClusterExtraction through the C++ adaptor (include/rsreg/pcl_compat.hpp), for
// tests/test_clusters_gpu.py.
//   cluster_runner <in.bin> <width> <height> <tolerance> <min_cluster_size> <max_cluster_size> <clusters_host.bin> <clusters_device.bin>
// in: 32-byte PointXYZRGB records.  clusters: int32 words -- the number of clusters, then for every cluster its size and its record
// indices; once from a host cloud and once from a cloud that stays in HBM.  Prints the number of clusters of both.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Extraction = rsreg::EuclideanClusterExtraction<rsreg::PointXYZRGB>;

static void save(const std::vector<rsreg::PointIndices> &clusters, const char *path)
{
    std::vector<int> words{(int)clusters.size()};
    for (const rsreg::PointIndices &c : clusters) {
        words.push_back((int)c.indices.size());
        words.insert(words.end(), c.indices.begin(), c.indices.end());
    }
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(words.data()), (std::streamsize)(words.size() * sizeof(int)));
}

int main(int argc, char **argv)
{
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <tolerance> <min_cluster_size> <max_cluster_size> <clusters_host.bin> "
                             "<clusters_device.bin>\n", argv[0]);
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

        Extraction ec;
        if (ec.getClusterTolerance() != 0.0 || ec.getMinClusterSize() != 1 || ec.getMaxClusterSize() != 2147483647)
            throw std::runtime_error("the defaults are not PCL's");
        ec.setClusterTolerance(std::atof(argv[4]));
        ec.setMinClusterSize(std::atoi(argv[5]));
        ec.setMaxClusterSize(std::atoi(argv[6]));
        ec.setInputCloud(frame);
        std::vector<rsreg::PointIndices> host, device;
        ec.extract(host);
        save(host, argv[7]);

        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame);
        ec.setInputCloud(dev);
        ec.extract(device);
        save(device, argv[8]);
        std::printf("clusters %zu\nclusters_device %zu\n", host.size(), device.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
