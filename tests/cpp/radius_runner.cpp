// radius_runner — pcl::RadiusOutlierRemoval and pcl::NormalEstimation (setRadiusSearch) through the C++ adaptor
// (include/rsreg/pcl_compat.hpp), for tests/test_radius_gpu.py and tests/test_radius_cpu.py.
//   radius_runner <in.bin> <width> <height> <radius> <min_neighbors> <negative> <keep_organized> <vx> <vy> <vz>
//                 <ror_host.bin> <ror_device.bin> <normals_host.bin> <normals_device.bin>
//   radius_runner refuse        NormalEstimation::compute with both searches set, then with neither: no device call is made
// in: 32-byte PointXYZRGB records; the filter's output: the kept records; the estimator's: 32-byte Normal records; each once from a
// host cloud and once from a cloud that stays in HBM.  Prints size, width, height and is_dense of the results.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using Normals = rsreg::PointCloud<rsreg::Normal>;

template <typename C> static void save(const C &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(c.points[0])));
}

// 0 when compute() throws RSREG_ERR_INVALID_ARG with `word` in its message
static int refused(rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> &ne, const char *word)
{
    try {
        Normals out;
        ne.compute(out);
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
        rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> ne;
        ne.setInputCloud(one);
        int bad = refused(ne, "neither");
        ne.setKSearch(10);
        ne.setRadiusSearch(0.03);
        bad += refused(ne, "both");
        ne.setKSearch(0);
        bad += ne.getRadiusSearch() == 0.03 && ne.getKSearch() == 0 ? 0 : 1;
        ne.setRadiusSearch(0);
        bad += refused(ne, "neither");
        std::printf("refused %s\n", bad ? "no" : "yes");
        return bad ? 1 : 0;
    }
    if (argc < 15) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <radius> <min_neighbors> <negative> <keep_organized> <vx> <vy> <vz> "
                             "<ror_host.bin> <ror_device.bin> <normals_host.bin> <normals_device.bin> | refuse\n", argv[0]);
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
        const double radius = std::atof(argv[4]);

        rsreg::RadiusOutlierRemoval<rsreg::PointXYZRGB> ror;
        ror.setInputCloud(frame);
        ror.setRadiusSearch(radius);
        ror.setMinNeighborsInRadius(std::atoi(argv[5]));
        ror.setNegative(std::atoi(argv[6]) != 0);
        ror.setKeepOrganized(std::atoi(argv[7]) != 0);
        Cloud kept_host;
        ror.filter(kept_host);
        save(kept_host, argv[11]);
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame), dev_kept;
        ror.filter(dev, dev_kept);
        Cloud kept;
        dev_kept.download(kept);
        save(kept, argv[12]);
        std::printf("ror_size %zu\nror_size_device %zu\nror_width %u\nror_height %u\nror_dense %d\nror_dense_device %d\nror_kept %llu\n", kept_host.size(),
                    kept.size(), kept_host.width, kept_host.height, (int)kept_host.is_dense, (int)kept.is_dense, (unsigned long long)ror.kept());

        rsreg::NormalEstimation<rsreg::PointXYZRGB, rsreg::Normal> ne;
        ne.setInputCloud(frame);
        ne.setRadiusSearch(radius);
        ne.setViewPoint((float)std::atof(argv[8]), (float)std::atof(argv[9]), (float)std::atof(argv[10]));
        Normals host;
        ne.compute(host);
        save(host, argv[13]);
        rsreg::DeviceCloud<rsreg::Normal> dev_normals;
        ne.compute(dev, dev_normals);
        Normals out;
        dev_normals.download(out);
        save(out, argv[14]);
        std::printf("size %zu\nsize_device %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\nradius %.17g\n", host.size(), out.size(), host.width,
                    host.height, (int)host.is_dense, (int)out.is_dense, ne.getRadiusSearch());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
