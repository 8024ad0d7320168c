// iss_runner — pcl::ISSKeypoint3D through the C++ adaptor (include/rsreg/pcl_compat.hpp), for tests/test_iss_gpu.py and
// tests/test_iss_cpu.py.
//   iss_runner <in.bin> <width> <height> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors>
//              <indices_host.bin> <indices_device.bin> <keypoints_host.bin> <keypoints_device.bin>
//   iss_runner refuse        compute() after setBorderRadius(0.1), then after setNormalRadius(0.1): no device call is made
// in: 32-byte PointXYZRGB records; indices: int32, ascending; keypoints: the 32-byte records; each once from a host cloud and
// once from a cloud that stays in HBM.  Prints the sizes and the shape of the results.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>

#include "rsreg/pcl_compat.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;
using ISS = rsreg::ISSKeypoint3D<rsreg::PointXYZRGB, rsreg::PointXYZRGB>;

static void save(const void *p, size_t bytes, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char *>(p), (std::streamsize)bytes);
}

// 0 when compute() throws RSREG_ERR_INVALID_ARG with "not built" in its message
static int refused(ISS &iss)
{
    try {
        Cloud out;
        iss.compute(out);
    } catch (const rsreg::Error &e) {
        return e.status == RSREG_ERR_INVALID_ARG && std::strstr(e.what(), "not built") ? 0 : 1;
    }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "refuse") == 0) {
        Cloud::Ptr one(new Cloud);
        one->points.resize(1);
        one->width = one->height = 1;
        ISS iss;
        iss.setInputCloud(one);
        iss.setSalientRadius(0.06);
        iss.setNonMaxRadius(0.04);
        iss.setBorderRadius(0.1);
        int bad = refused(iss);
        iss.setBorderRadius(0.0);
        iss.setNormalRadius(0.1);
        bad += refused(iss);
        std::printf("refused %s\n", bad ? "no" : "yes");
        return bad ? 1 : 0;
    }
    if (argc < 13) {
        std::fprintf(stderr, "usage: %s <in.bin> <width> <height> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors> "
                             "<indices_host.bin> <indices_device.bin> <keypoints_host.bin> <keypoints_device.bin> | refuse\n", argv[0]);
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

        ISS iss;
        iss.setInputCloud(frame);
        iss.setSalientRadius(std::atof(argv[4]));
        iss.setNonMaxRadius(std::atof(argv[5]));
        iss.setThreshold21(std::atof(argv[6]));
        iss.setThreshold32(std::atof(argv[7]));
        iss.setMinNeighbors(std::atoi(argv[8]));
        Cloud host;
        iss.compute(host);
        save(iss.getKeypointsIndices().data(), iss.getKeypointsIndices().size() * sizeof(int), argv[9]);
        save(host.points.data(), host.size() * sizeof(rsreg::PointXYZRGB), argv[11]);
        const size_t n_host = iss.getKeypointsIndices().size();

        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev(*frame), dev_out;
        iss.compute(dev, dev_out);
        Cloud out;
        dev_out.download(out);
        save(iss.getKeypointsIndices().data(), iss.getKeypointsIndices().size() * sizeof(int), argv[10]);
        save(out.points.data(), out.size() * sizeof(rsreg::PointXYZRGB), argv[12]);
        std::printf("size %zu\nsize_device %zu\nindices %zu\nindices_device %zu\nwidth %u\nheight %u\ndense %d\ndense_device %d\n", host.size(), out.size(),
                    n_host, iss.getKeypointsIndices().size(), host.width, host.height, (int)host.is_dense, (int)out.is_dense);

        iss.setBorderRadius(0.1);
        std::printf("border_refused %s\n", refused(iss) ? "no" : "yes");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
