// capture.hpp — the capture step of the C++ host layer: a depth frame and a colour frame -> an organized PointXYZRGB cloud.
//
// The reference builds its clouds with rs2::pointcloud (map_to, calculate) and convert_to_pcl (src/capture.hpp:72-107: the
// three-fifths centre crop) or convert_to_pcl_new (src/capture_opencv.hpp:128-160: the whole frame).  rsreg::DepthToCloud is
// those two steps over the C ABI (include/rsreg.h, "capture", states the contract): into a DeviceCloud, the cloud is built in
// HBM from the two images (5 bytes a pixel over the link, not the 32 of a record); into a host PointCloud, the sequential host
// restatement runs -- the same bytes from both.  librealsense is not needed: intrinsics and extrinsics are handed over
// as the numbers rs2_intrinsics / rs2_extrinsics hold.
#pragma once

#include "pcl_compat.hpp"

namespace rsreg {

template <typename PointT = PointXYZRGB> class DepthToCloud {
    static_assert(sizeof(PointT) == 32, "DepthToCloud writes 32-byte PointXYZRGB records");

  public:
    DepthToCloud() { rsreg_depth_params_default(1, 1, &prm_); }
    // rs2_intrinsics of the depth and of the colour stream: width, height, ppx, ppy, fx, fy, model, coeffs[5]
    void setDepthIntrinsics(const rsreg_intrinsics &in) { prm_.depth = in; }
    void setColorIntrinsics(const rsreg_intrinsics &in) { prm_.color = in; }
    // rs2_extrinsics depth -> colour: rotation 9 floats column-major, translation 3 (metres)
    void setExtrinsics(const float rotation[9], const float translation[3])
    {
        for (int i = 0; i < 9; ++i) prm_.rotation[i] = rotation[i];
        for (int i = 0; i < 3; ++i) prm_.translation[i] = translation[i];
    }
    void setDepthScale(float metres_per_unit) { prm_.depth_scale = metres_per_unit; }
    // bytes per colour pixel (3 or 4) and their order: bgr = true is the reference's ("BGR due to Camera Model")
    void setColorLayout(int bytes_per_pixel, bool bgr)
    {
        prm_.color_bytes_per_pixel = bytes_per_pixel;
        prm_.color_bgr = bgr ? 1 : 0;
    }
    // true: convert_to_pcl's three-fifths centre crop, its shape and is_dense = true; false (default): the whole frame, is_dense = false
    void setReferenceCrop(bool on) { crop_ = on; }
    bool getReferenceCrop() const { return crop_; }
    // the parameters compute() hands over: the window and the shape follow the depth intrinsics
    rsreg_depth_params params() const
    {
        rsreg_depth_params window, p = prm_;
        const uint32_t w = (uint32_t)(p.depth.width > 0 ? p.depth.width : 0), h = (uint32_t)(p.depth.height > 0 ? p.depth.height : 0);
        if (crop_) rsreg_depth_params_reference(w, h, &window); else rsreg_depth_params_default(w, h, &window);
        p.r0 = window.r0, p.r1 = window.r1, p.c0 = window.c0, p.c1 = window.c1;
        p.out_width = window.out_width, p.out_height = window.out_height, p.is_dense = window.is_dense;
        return p;
    }
    // depth: rows of uint16, depth_stride bytes apart; color: rows of 3- or 4-byte pixels, color_stride bytes apart (host memory)
    void compute(const void *depth, size_t depth_stride, const void *color, size_t color_stride, DeviceCloud<PointT> &out) const
    {
        const rsreg_depth_params p = params();
        check(rsreg_cloud_from_depth(out.context()->get(), depth, depth_stride, color, color_stride, &p, out.handle()), out.context()->get());
    }
    void compute(const void *depth, size_t depth_stride, const void *color, size_t color_stride, PointCloud<PointT> &out) const
    {
        const rsreg_depth_params p = params();
        PointVector<PointT> pts = uninitialized_points<PointT>((size_t)p.out_width * p.out_height);
        uint32_t w = 0, h = 0;
        int dense = 0;
        check(rsreg_depth_to_cloud(depth, depth_stride, color, color_stride, &p, pts.data(), pts.size(), &w, &h, &dense));
        out.points = std::move(pts);
        out.width = w;
        out.height = h;
        out.is_dense = dense != 0;
    }
    // the two images already in HBM (engine extra: rsreg_cloud_from_depth_device); they must stay alive and unchanged until the
    // next synchronising call on the context has returned
    void computeDevice(const void *d_depth, size_t depth_stride, const void *d_color, size_t color_stride, DeviceCloud<PointT> &out) const
    {
        const rsreg_depth_params p = params();
        check(rsreg_cloud_from_depth_device(out.context()->get(), d_depth, depth_stride, d_color, color_stride, &p, out.handle()), out.context()->get());
    }

  private:
    rsreg_depth_params prm_;
    bool crop_ = false;
};

}  // namespace rsreg
