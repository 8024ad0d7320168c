// depthcloud_runner — rsreg::DepthToCloud through the C++ host layer (include/rsreg/capture.hpp), for tests/test_depthcloud_cpp_gpu.py.
//   depthcloud_runner <params.bin> <depth.bin> <depth_stride> <color.bin> <color_stride> <crop 0|1> <out_host.bin> <out_device.bin> <out_abi.bin>
// params.bin: a rsreg_depth_params as the test wrote it (the class takes its intrinsics, extrinsics, scale and layout from it;
// the window comes from setReferenceCrop).  The same frame three ways: the class into a host cloud, the class into a device
// cloud, and the C ABI called directly with the test's struct.  Prints the shapes.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

#include "rsreg/capture.hpp"

using Cloud = rsreg::PointCloud<rsreg::PointXYZRGB>;

static std::vector<char> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void save(const Cloud &c, const char *path)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(c.points.data()), (std::streamsize)(c.size() * sizeof(rsreg::PointXYZRGB)));
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <params.bin> <depth.bin> <depth_stride> <color.bin> <color_stride> <crop> <host.bin> <device.bin> <abi.bin>\n", argv[0]);
        return 2;
    }
    try {
        const std::vector<char> pb = slurp(argv[1]), depth = slurp(argv[2]), color = slurp(argv[4]);
        if (pb.size() != sizeof(rsreg_depth_params)) throw std::runtime_error("params.bin is not a rsreg_depth_params");
        rsreg_depth_params p;
        std::memcpy(&p, pb.data(), sizeof(p));
        const size_t dstride = (size_t)std::atol(argv[3]), cstride = (size_t)std::atol(argv[5]);

        rsreg::DepthToCloud<rsreg::PointXYZRGB> cap;
        cap.setDepthIntrinsics(p.depth);
        cap.setColorIntrinsics(p.color);
        cap.setExtrinsics(p.rotation, p.translation);
        cap.setDepthScale(p.depth_scale);
        cap.setColorLayout(p.color_bytes_per_pixel, p.color_bgr != 0);
        cap.setReferenceCrop(std::atoi(argv[6]) != 0);

        Cloud host;
        cap.compute(depth.data(), dstride, color.data(), cstride, host);
        save(host, argv[7]);

        rsreg::DeviceCloud<rsreg::PointXYZRGB> dev;
        cap.compute(depth.data(), dstride, color.data(), cstride, dev);
        Cloud from_dev;
        dev.download(from_dev);
        save(from_dev, argv[8]);

        rsreg::DeviceCloud<rsreg::PointXYZRGB> abi;
        rsreg::check(rsreg_cloud_from_depth(abi.context()->get(), depth.data(), dstride, color.data(), cstride, &p, abi.handle()), abi.context()->get());
        Cloud from_abi;
        abi.download(from_abi);
        save(from_abi, argv[9]);

        std::printf("host %zu %u %u %d\ndevice %zu %u %u %d\nabi %zu %u %u %d\n", host.size(), host.width, host.height, (int)host.is_dense, from_dev.size(),
                    from_dev.width, from_dev.height, (int)from_dev.is_dense, from_abi.size(), from_abi.width, from_abi.height, (int)from_abi.is_dense);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
