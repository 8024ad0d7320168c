// sor_runner — the reference's pre-filter (src/capture.hpp:112-132: PassThrough on z, then StatisticalOutlierRemoval with
// 50 neighbours and 1.5 sigma) through the C++ adaptor (include/rsreg/pcl_compat.hpp), for tests/test_sor_gpu.py.
//   sor_runner <in.bin> <width> <height> <out_host.bin> <out_device.bin>   (32-byte PointXYZRGB records)
// Unlike the reference, the limits are set BEFORE PassThrough runs, and the filtered cloud is what comes back.
// Prints `kept <n>` and the threshold as a C99 hex float.
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;

static Cloud::Ptr prefilter(const Cloud::Ptr &frame, rsreg_sor_stats *stats)
{
    Cloud::Ptr in_range(new Cloud), inliers(new Cloud);
    rsreg::PassThrough<rsreg::PointXYZRGB> pass;
    pass.setInputCloud(frame);
    pass.setFilterFieldName("z");
    pass.setFilterLimits(0.2, 2.5);
    pass.filter(*in_range);
    rsreg::StatisticalOutlierRemoval<rsreg::PointXYZRGB> sor;
    sor.setInputCloud(in_range);
    sor.setMeanK(50);
    sor.setStddevMulThresh(1.5);
    sor.filter(*inliers);
    *stats = sor.stats();
    return inliers;
}

static void save(const Cloud &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::PointXYZRGB)));
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <out_host.bin> <out_device.bin>\n", argv[0]);
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
        rsreg_sor_stats stats{};
        const Cloud::Ptr host = prefilter(frame, &stats);
        save(*host, argv[4]);
        // the same on clouds that stay in HBM, filtered in place
        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame);
        rsreg::PassThrough<rsreg::PointXYZRGB> pass;
        pass.setFilterFieldName("z");
        pass.setFilterLimits(0.2, 2.5);
        pass.filter(dev, dev);
        rsreg::StatisticalOutlierRemoval<rsreg::PointXYZRGB> sor;
        sor.setMeanK(50);
        sor.setStddevMulThresh(1.5);
        sor.filter(dev, dev);
        Cloud out;
        dev.download(out);
        save(out, argv[5]);
        std::printf("kept %zu\nkept_device %zu\nwidth %u\nheight %u\nthreshold %a\n", host->size(), out.size(), host->width, host->height, stats.threshold);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
