// pcl_compat.hpp — header-only C++ host layer over the C ABI (include/rsreg.h).
//
// The reference (hyunminch/realsense-pointcloud) is compiled C++ that calls PCL classes; this
// header offers the same class surface — names, argument meaning, error behaviour — for
// exactly the calls its registration schemes make, so that a scheme written
// against PCL compiles against `rsreg::` with a namespace switch:
//
//   pcl::PointXYZRGB / pcl::PointCloud<T> / ::Ptr          src/types.hpp:8-10
//   pcl::IterativeClosestPoint<S,T>                         src/incremental_icp.hpp:37,46-63
//   pcl::NormalDistributionsTransform<S,T>                  src/ndt_edge_based_registration.hpp:37-43,71-104
//   pcl::ApproximateVoxelGrid<T>                            src/icp_edge_based_registration.hpp:38,47,59-60
//   pcl::transformPointCloud(in, out, Matrix4f)             src/incremental_icp.hpp:63
//   pcl::io::loadPCDFile / savePCDFileBinary                src/main.cpp:81,87
//   Eigen::Matrix4f, AngleAxisf * Translation3f products    src/icp_edge...hpp:81-92 (as rsreg::Matrix4f helpers)
//
// No PCL, Eigen or Boost is needed.  All numerics run on the MI355X through librsreg.so; a
// missing GPU makes the calls throw rsreg::Error (there is no CPU fallback).
#pragma once

#include <sys/mman.h>

#include <array>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <new>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../rsreg.h"
#include "lzf.hpp"

namespace rsreg {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(int status, rsreg_ctx *ctx = nullptr)
{
    if (status == RSREG_OK) return;
    std::string msg = std::string("rsreg: ") + rsreg_status_string(status);
    if (ctx) msg += std::string(" (") + rsreg_last_error(ctx) + ")";
    throw Error(status, msg);
}

// (id, version) of a device cloud: the pair changes whenever its records in HBM are rewritten (rsreg_cloud_version)
inline std::pair<uint64_t, uint64_t> cloud_stamp(const rsreg_cloud *c)
{
    uint64_t id = 0, version = 0;
    check(rsreg_cloud_version(c, &id, &version));
    return {id, version};
}

// ---- pcl::PointXYZRGB: 32 bytes, 16-byte aligned, rgb at byte 16
struct alignas(16) PointXYZRGB {
    float x = 0.f, y = 0.f, z = 0.f, data3 = 1.f;
    union {
        struct { uint8_t b, g, r, a; };
        float rgb;
        uint32_t rgba;
    };
    uint32_t pad_[3] = {0, 0, 0};
    PointXYZRGB() : rgba(0xff000000u) {}
    PointXYZRGB(float x_, float y_, float z_) : x(x_), y(y_), z(z_), rgba(0xff000000u) {}
};
static_assert(sizeof(PointXYZRGB) == 32, "PointXYZRGB must stay byte-compatible with pcl::PointXYZRGB");

// ---- pcl::Normal: 32 bytes, 16-byte aligned -- normal[3] + 0.f, then curvature and three words of padding
struct alignas(16) Normal {
    union {
        float data_n[4];
        float normal[3];
        struct { float normal_x, normal_y, normal_z; };
    };
    union {
        struct { float curvature; };
        float data_c[4];
    };
    Normal() : data_n{0.f, 0.f, 0.f, 0.f}, data_c{0.f, 0.f, 0.f, 0.f} {}
    Normal(float nx, float ny, float nz) : data_n{nx, ny, nz, 0.f}, data_c{0.f, 0.f, 0.f, 0.f} {}
};
static_assert(sizeof(Normal) == 32, "Normal must stay byte-compatible with pcl::Normal");

// ---- pcl::PointXYZRGBNormal: 48 bytes, 16-byte aligned -- data[4], data_n[4], then rgb, curvature and two words of padding
// (the reference declares it as rgb_normal_point, src/types.hpp:11-12, and never uses it)
struct alignas(16) PointXYZRGBNormal {
    float x = 0.f, y = 0.f, z = 0.f, data3 = 1.f;
    union {
        float data_n[4];
        float normal[3];
        struct { float normal_x, normal_y, normal_z; };
    };
    union {
        struct { uint8_t b, g, r, a; };
        float rgb;
        uint32_t rgba;
    };
    float curvature = 0.f;
    uint32_t pad_[2] = {0, 0};
    PointXYZRGBNormal() : data_n{0.f, 0.f, 0.f, 0.f}, rgba(0xff000000u) {}
};
static_assert(sizeof(PointXYZRGBNormal) == 48, "PointXYZRGBNormal must stay byte-compatible with pcl::PointXYZRGBNormal");
static_assert(offsetof(PointXYZRGBNormal, x) == 0 && offsetof(PointXYZRGBNormal, data_n) == 16 && offsetof(PointXYZRGBNormal, rgba) == 32 &&
                  offsetof(PointXYZRGBNormal, curvature) == 36,
              "PointXYZRGBNormal: xyz at 0, the normal at 16, rgb at 32, curvature at 36");

// ---- storage of a cloud's points.  pcl::PointCloud keeps a std::vector with Eigen's aligned allocator; this one is
// aligned too and can hand out records WITHOUT constructing them one by one, for the callers that overwrite every
// record right away (a download of the merged cloud of 16 frames spent 25 ms of a 60 ms scheme constructing 4.9 M
// points on one thread before the copy touched them).
namespace detail {
inline bool &skip_point_init()
{
    static thread_local bool skip = false;
    return skip;
}
template <class T> struct point_allocator {
    using value_type = T;
    point_allocator() = default;
    template <class U> point_allocator(const point_allocator<U> &) {}
    // Large clouds sit on 2 MB pages where the kernel hands them out on request (what numpy does for its arrays): the
    // first touch of a 157 MB merged cloud is 75 page faults instead of 38 000 (20 ms of a 54 ms scheme).
    T *allocate(size_t n)
    {
        const size_t bytes = n * sizeof(T), huge = (size_t)2 << 20;
        const bool large = bytes >= 2 * huge;
        void *p = nullptr;
        if (posix_memalign(&p, large ? huge : (alignof(T) > sizeof(void *) ? alignof(T) : sizeof(void *)), bytes ? bytes : 1) != 0) throw std::bad_alloc();
#ifdef MADV_HUGEPAGE
        if (large) (void)madvise(p, bytes, MADV_HUGEPAGE);
#endif
        return static_cast<T *>(p);
    }
    void deallocate(T *p, size_t) { std::free(p); }
    template <class U> void construct(U *p)
    {
        if (!skip_point_init()) ::new (static_cast<void *>(p)) U();
    }
    template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a)
    {
        ::new (static_cast<void *>(p)) U(std::forward<A0>(a0), std::forward<A>(a)...);
    }
    template <class U> bool operator==(const point_allocator<U> &) const { return true; }
    template <class U> bool operator!=(const point_allocator<U> &) const { return false; }
};
}  // namespace detail

template <typename PointT> using PointVector = std::vector<PointT, detail::point_allocator<PointT>>;

// n records the caller is about to overwrite, all of them (their contents are unspecified until then)
template <typename PointT> inline PointVector<PointT> uninitialized_points(size_t n)
{
    static_assert(std::is_trivially_copyable<PointT>::value && std::is_trivially_destructible<PointT>::value,
                  "records that may stay unconstructed must be plain data");
#if defined(RSREG_PCL_COMPAT_FAST_UNINIT) && defined(__GLIBCXX__) && !defined(_GLIBCXX_DEBUG) && !defined(_GLIBCXX_SANITIZE_VECTOR)
    // OPT-IN (-DRSREG_PCL_COMPAT_FAST_UNINIT; this repository's own runners set it): libstdc++ only, not its debug mode nor
    // annotated containers.  The storage is reserved and the end pointer moved, no per-record call at all (the portable
    // default below goes through the allocator's construct() once per record: 1 ms of doing nothing for a merged cloud of
    // 4.9 M points).  It reaches into libstdc++'s private _M_impl through a cast to a type the vector is not -- formally
    // undefined behaviour, which is why an integrator's toolchain gets the portable path unless it asks.
    struct Open : PointVector<PointT> {
        void grow_unconstructed(size_t m)
        {
            this->reserve(m);
            this->_M_impl._M_finish = this->_M_impl._M_start + m;
        }
    };
    PointVector<PointT> v;
    static_cast<Open &>(v).grow_unconstructed(n);
    return v;
#else
    struct Guard {
        bool before = detail::skip_point_init();
        Guard() { detail::skip_point_init() = true; }
        ~Guard() { detail::skip_point_init() = before; }
    } guard;
    return PointVector<PointT>(n);
#endif
}

// ---- pcl::PointCloud<PointT>
template <typename PointT> struct PointCloud {
    using Ptr = std::shared_ptr<PointCloud<PointT>>;
    using ConstPtr = std::shared_ptr<const PointCloud<PointT>>;
    PointVector<PointT> points;
    uint32_t width = 0, height = 0;
    bool is_dense = true;

    size_t size() const { return points.size(); }
    bool empty() const { return points.empty(); }
    bool isOrganized() const { return height > 1; }
    void clear() { points.clear(); width = height = 0; }
    void push_back(const PointT &p) { points.push_back(p); width = (uint32_t)points.size(); height = 1; }
    PointT &operator[](size_t i) { return points[i]; }
    const PointT &operator[](size_t i) const { return points[i]; }

    // concatenation: width = size, height = 1, dense only if both are
    PointCloud &operator+=(const PointCloud &rhs)
    {
        points.insert(points.end(), rhs.points.begin(), rhs.points.end());
        width = (uint32_t)points.size();
        height = 1;
        is_dense = is_dense && rhs.is_dense;
        return *this;
    }
    PointCloud operator+(const PointCloud &rhs) const
    {
        PointCloud out = *this;
        out += rhs;
        return out;
    }
};

// ---- Eigen::Matrix4f stand-in: 16 floats, column-major
struct Matrix4f {
    float m[16];
    Matrix4f() { std::memset(m, 0, sizeof(m)); }
    static Matrix4f Identity()
    {
        Matrix4f r;
        r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.f;
        return r;
    }
    float &operator()(int r, int c) { return m[c * 4 + r]; }
    float operator()(int r, int c) const { return m[c * 4 + r]; }
    const float *data() const { return m; }
    float *data() { return m; }
    Matrix4f operator*(const Matrix4f &o) const
    {
        Matrix4f r;
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 4; ++i) {
                float s = 0.f;
                for (int k = 0; k < 4; ++k) s += m[k * 4 + i] * o.m[j * 4 + k];
                r.m[j * 4 + i] = s;
            }
        return r;
    }
    bool operator==(const Matrix4f &o) const { return std::memcmp(m, o.m, sizeof(m)) == 0; }
    bool operator!=(const Matrix4f &o) const { return !(*this == o); }
    // (Eigen::Translation3f(t) * Eigen::AngleAxisf(angle, axis)).matrix() pieces
    static Matrix4f RotationX(float a) { Matrix4f r = Identity(); const float c = std::cos(a), s = std::sin(a); r(1, 1) = c; r(1, 2) = -s; r(2, 1) = s; r(2, 2) = c; return r; }
    static Matrix4f RotationY(float a) { Matrix4f r = Identity(); const float c = std::cos(a), s = std::sin(a); r(0, 0) = c; r(0, 2) = s; r(2, 0) = -s; r(2, 2) = c; return r; }
    static Matrix4f RotationZ(float a) { Matrix4f r = Identity(); const float c = std::cos(a), s = std::sin(a); r(0, 0) = c; r(0, 1) = -s; r(1, 0) = s; r(1, 1) = c; return r; }
    static Matrix4f Translation(float x, float y, float z) { Matrix4f r = Identity(); r(0, 3) = x; r(1, 3) = y; r(2, 3) = z; return r; }
};

// ---- one execution context per (device, stream); shared default on device 0
class Context {
  public:
    explicit Context(int device = 0, void *stream = nullptr) { check(rsreg_ctx_create(device, stream, &ctx_)); }
    ~Context() { if (ctx_) rsreg_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    rsreg_ctx *get() const { return ctx_; }
    void wait_downloads() { check(rsreg_ctx_wait_downloads(ctx_), ctx_); }   // every DeviceCloud::download_async of this context has landed
    // what a frame loop is about to need, made on a thread of the context while the caller goes on (rsreg_ctx_prepare)
    void prepare(size_t frame_bytes, size_t model_bytes, bool side_streams) { check(rsreg_ctx_prepare(ctx_, frame_bytes, model_bytes, side_streams ? RSREG_PREPARE_SIDE_STREAMS : 0u), ctx_); }
    // A context holds ONE ICP target index, ONE ICP source and ONE NDT voxel grid.  The object that
    // uploaded each of them last is remembered here, so that a second registration object sharing
    // the context (e.g. the default one) re-uploads its own clouds instead of silently using another's.
    const void *icp_target_owner = nullptr, *icp_source_owner = nullptr, *ndt_target_owner = nullptr;
    static std::shared_ptr<Context> Default()
    {
        static std::shared_ptr<Context> ctx = std::make_shared<Context>(0);
        return ctx;
    }
  private:
    rsreg_ctx *ctx_ = nullptr;
};

// ---- a cloud resident in HBM (rsreg_cloud): what the frame loop hands from step to step without
// leaving the GPU (filter -> align -> transformPointCloud -> operator+, icp_edge_based_registration.hpp:75-120)
template <typename PointT> class DeviceCloud {
  public:
    using Ptr = std::shared_ptr<DeviceCloud<PointT>>;
    explicit DeviceCloud(std::shared_ptr<Context> ctx = Context::Default()) : ctx_(std::move(ctx))
    {
        check(rsreg_cloud_create(ctx_->get(), &h_), ctx_->get());
    }
    explicit DeviceCloud(const PointCloud<PointT> &host, std::shared_ptr<Context> ctx = Context::Default()) : DeviceCloud(std::move(ctx))
    {
        upload(host);
    }
    ~DeviceCloud() { if (h_) rsreg_cloud_destroy(h_); }
    DeviceCloud(const DeviceCloud &) = delete;
    DeviceCloud &operator=(const DeviceCloud &) = delete;
    void upload(const PointCloud<PointT> &host)
    {
        check(rsreg_cloud_upload(h_, host.points.data(), host.size(), sizeof(PointT), host.width, host.height, host.is_dense), ctx_->get());
    }
    // upload() that returns once the records are staged: the PCIe copy runs beside the main stream's work, and whoever
    // touches this cloud next waits for it (rsreg_cloud_upload_async).  `host` may change as soon as this returns.
    void upload_async(const PointCloud<PointT> &host)
    {
        check(rsreg_cloud_upload_async(h_, host.points.data(), host.size(), sizeof(PointT), host.width, host.height, host.is_dense), ctx_->get());
    }
    // upload_async() that returns before `host` has been read (rsreg_cloud_upload_deferred): a thread of the context
    // stages the records and queues their copy.  `host` must stay as it is until a call that reads or rewrites this
    // cloud has returned -- the frame loops hand over the caller's frames, which stay put for the whole registration.
    void upload_deferred(const PointCloud<PointT> &host)
    {
        check(rsreg_cloud_upload_deferred(h_, host.points.data(), host.size(), sizeof(PointT), host.width, host.height, host.is_dense), ctx_->get());
    }
    void download(PointCloud<PointT> &host) const
    {
        size_t n = 0, stride = 0;
        uint32_t w = 0, h = 0;
        int dense = 0;
        check(rsreg_cloud_info(h_, &n, &stride, &w, &h, &dense), ctx_->get());
        if (n && stride != sizeof(PointT)) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: record size of the device cloud differs");
        PointVector<PointT> pts = uninitialized_points<PointT>(n);
        check(rsreg_cloud_download(h_, pts.data(), n), ctx_->get());
        host.points = std::move(pts);
        host.width = w;
        host.height = h;
        host.is_dense = dense != 0;
    }
    // engine extra: download() that returns at once -- the records as they are now go to dst[0 .. size()) beside whatever
    // the GPU does next; dst belongs to the copy until Context::wait_downloads() has returned (rsreg_cloud_download_async)
    void download_async(PointT *dst, size_t capacity) const
    {
        check(rsreg_cloud_download_async(h_, dst, capacity), ctx_->get());
    }
    void info(size_t &n, uint32_t &width, uint32_t &height, bool &is_dense) const
    {
        size_t stride = 0;
        int dense = 0;
        check(rsreg_cloud_info(h_, &n, &stride, &width, &height, &dense), ctx_->get());
        is_dense = dense != 0;
    }
    size_t size() const
    {
        size_t n = 0;
        check(rsreg_cloud_info(h_, &n, nullptr, nullptr, nullptr, nullptr), ctx_->get());
        return n;
    }
    // *this += other (PointCloud::operator+=): grows in place
    DeviceCloud &operator+=(const DeviceCloud &other)
    {
        check(rsreg_cloud_concat(ctx_->get(), h_, other.h_, h_), ctx_->get());
        return *this;
    }
    // out = a + b (a's records first); out may be a or b
    static void concatenate(const DeviceCloud &a, const DeviceCloud &b, DeviceCloud &out)
    {
        check(rsreg_cloud_concat(a.ctx_->get(), a.h_, b.h_, out.h_), a.ctx_->get());
    }
    rsreg_cloud *handle() const { return h_; }
    const std::shared_ptr<Context> &context() const { return ctx_; }

  private:
    std::shared_ptr<Context> ctx_;
    rsreg_cloud *h_ = nullptr;
};

namespace detail {
template <typename PointT> void copy_aligned(const PointCloud<PointT> &src, PointCloud<PointT> &out)
{
    out.points = src.points;  // fields other than xyz are the source's (PCL copies the input first)
    out.width = src.width;
    out.height = src.height;
    out.is_dense = src.is_dense;
}
}  // namespace detail

namespace detail {
template <typename PointT, typename = void> struct has_normal : std::false_type {};
template <typename PointT> struct has_normal<PointT, decltype((void)std::declval<PointT &>().normal_x)> : std::true_type {};
}  // namespace detail

// ---- pcl::registration::CorrespondenceRejector and the four rejectors an ICP object's chain takes (rsreg.h:
// rsreg_icp_set_rejectors holds the contract and the stated deviations).  The objects carry a kind and a value; the rejection
// itself runs inside the alignment, on the GPU, in the order the rejectors were added.
namespace registration {
class CorrespondenceRejector {
  public:
    using Ptr = std::shared_ptr<CorrespondenceRejector>;
    using ConstPtr = std::shared_ptr<const CorrespondenceRejector>;
    virtual ~CorrespondenceRejector() = default;
    int kind() const { return kind_; }
    double value() const { return value_; }
    // engine extra: the pairs in front of and behind this rejector in the last iteration of the last align()
    const rsreg_rejector_stat &stat() const { return stat_; }
    void set_stat_(const rsreg_rejector_stat &s) { stat_ = s; }

  protected:
    CorrespondenceRejector(int kind, double value) : kind_(kind), value_(value) {}
    int kind_;
    double value_;
    rsreg_rejector_stat stat_{};
};

class CorrespondenceRejectorMedianDistance : public CorrespondenceRejector {
  public:
    using Ptr = std::shared_ptr<CorrespondenceRejectorMedianDistance>;
    CorrespondenceRejectorMedianDistance() : CorrespondenceRejector(RSREG_REJECTOR_MEDIAN_DISTANCE, 1.0) {}
    void setMedianFactor(double factor) { value_ = factor; }
    double getMedianFactor() const { return value_; }
    double getMedianDistance() const { return stat_.median_distance; }   // of the last iteration of the last align(): a SQUARED distance, as in PCL
};

class CorrespondenceRejectorOneToOne : public CorrespondenceRejector {
  public:
    using Ptr = std::shared_ptr<CorrespondenceRejectorOneToOne>;
    CorrespondenceRejectorOneToOne() : CorrespondenceRejector(RSREG_REJECTOR_ONE_TO_ONE, 0.0) {}
};

class CorrespondenceRejectorSurfaceNormal : public CorrespondenceRejector {
  public:
    using Ptr = std::shared_ptr<CorrespondenceRejectorSurfaceNormal>;
    CorrespondenceRejectorSurfaceNormal() : CorrespondenceRejector(RSREG_REJECTOR_SURFACE_NORMAL, 1.0) {}
    void setThreshold(double threshold) { value_ = threshold; }
    double getThreshold() const { return value_; }
};

class CorrespondenceRejectorTrimmed : public CorrespondenceRejector {
  public:
    using Ptr = std::shared_ptr<CorrespondenceRejectorTrimmed>;
    CorrespondenceRejectorTrimmed() : CorrespondenceRejector(RSREG_REJECTOR_TRIMMED, 0.5) {}
    void setOverlapRatio(double ratio) { value_ = ratio; }
    double getOverlapRatio() const { return value_; }
};
}  // namespace registration

// ---- pcl::IterativeClosestPoint
template <typename PointSource, typename PointTarget> class IterativeClosestPoint {
  public:
    using SourcePtr = typename PointCloud<PointSource>::Ptr;
    using TargetPtr = typename PointCloud<PointTarget>::Ptr;

    explicit IterativeClosestPoint(std::shared_ptr<Context> ctx = Context::Default()) : ctx_(std::move(ctx))
    {
        rsreg_icp_params_default(&prm_);
        final_ = Matrix4f::Identity();
    }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    void setMaxCorrespondenceDistance(double d)
    {
        if (d != prm_.max_correspondence_distance) target_dirty_ = true;  // the index cell size derives from it
        prm_.max_correspondence_distance = d;
    }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setTransformationRotationEpsilon(double e) { prm_.transformation_rotation_epsilon = e; }
    void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
    void setInputSource(const SourcePtr &cloud) { source_ = cloud; dsource_ = nullptr; source_dirty_ = true; }
    void setInputTarget(const TargetPtr &cloud) { target_ = cloud; dtarget_ = nullptr; target_dirty_ = true; }  // PCL rebuilds its kd-tree here too
    // optional correspondence filters (off by default; the reference constructs a trimmed rejector and never attaches it)
    void setUseReciprocalCorrespondences(bool on) { prm_.use_reciprocal_correspondences = on ? 1 : 0; }
    // addCorrespondenceRejector (CorrespondenceRejectorTrimmed with setOverlapRatio (ratio)); <= 0 or >= 1: none
    void setTrimmedRejectorOverlapRatio(double ratio) { prm_.trim_overlap_ratio = ratio; }
    // Registration::addCorrespondenceRejector and its companions: the chain runs in this order in every iteration, behind the two
    // filters above.  A CorrespondenceRejectorSurfaceNormal reads the normals of both clouds: inside the records (PointXYZRGBNormal)
    // or beside them (setInputSourceNormals; setInputTargetNormals of IterativeClosestPointWithNormals)
    using CorrespondenceRejectorPtr = registration::CorrespondenceRejector::Ptr;
    void addCorrespondenceRejector(const CorrespondenceRejectorPtr &rejector)
    {
        if (!rejector) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: addCorrespondenceRejector(null)");
        if (rejectors_.size() >= RSREG_MAX_REJECTORS) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: a rejector chain has at most 8 entries");
        rejectors_.push_back(rejector);
    }
    std::vector<CorrespondenceRejectorPtr> getCorrespondenceRejectors() const { return rejectors_; }
    bool removeCorrespondenceRejector(unsigned int i)
    {
        if (i >= rejectors_.size()) return false;
        rejectors_.erase(rejectors_.begin() + i);
        return true;
    }
    void clearCorrespondenceRejectors() { rejectors_.clear(); }
    // one normal per source record; the cloud must stay alive and unchanged until align has returned
    void setInputSourceNormals(const PointCloud<Normal> &normals) { src_normals_ = &normals; src_normals_dirty_ = true; }
    // engine knobs without a PCL counterpart
    void setFixedIterationCount(bool on) { prm_.criteria_mode = on ? RSREG_CRITERIA_FIXED : RSREG_CRITERIA_PCL; }
    void setPipelineMode(int mode) { prm_.pipeline_mode = mode; }

    void align(PointCloud<PointSource> &output) { align(output, Matrix4f::Identity()); }
    void align(PointCloud<PointSource> &output, const Matrix4f &guess)
    {
        if (!source_ || !target_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource / setInputTarget not called");
        rsreg_ctx *c = ctx_->get();
        // the source first (the reference's order, incremental_icp.hpp:57-58): it is loaded on a stream of its own,
        // beside the target's index build
        if (source_dirty_ || ctx_->icp_source_owner != this) {
            check(rsreg_icp_set_source(c, source_->points.data(), source_->size(), sizeof(PointSource), source_->is_dense), c);
            source_dirty_ = false;
            ctx_->icp_source_owner = this;
            src_normals_dirty_ = true;   // (a new source drops the normals of the one before)
        }
        if (target_dirty_ || ctx_->icp_target_owner != this) {
            check(rsreg_icp_set_target(c, target_->points.data(), target_->size(), sizeof(PointTarget), target_->is_dense,
                                       prm_.max_correspondence_distance), c);
            target_dirty_ = false;
            ctx_->icp_target_owner = this;
            target_normals_set_ = false;
            target_set_(c, true);
        } else {
            target_set_(c, false);
        }
        // `output = input` (PCL copies the input cloud first, then rewrites xyz) is made inside the call, by the host threads that
        // write the aligned positions anyway (rsreg_icp_align_records): the records are never constructed or copied here
        set_rejectors_(c);
        PointCloud<PointSource> tmp;
        tmp.points = uninitialized_points<PointSource>(source_->size());
        tmp.width = source_->width;
        tmp.height = source_->height;
        tmp.is_dense = source_->is_dense;
        if (source_->size())
            check(rsreg_icp_align_records(c, guess.data(), &prm_, &res_, source_->points.data(), tmp.points.data(), sizeof(PointSource)), c);
        else
            check(rsreg_icp_align(c, guess.data(), &prm_, &res_, nullptr, 0), c);
        std::memcpy(final_.m, res_.transform, sizeof(final_.m));
        fetch_rejector_stats_(c);
        output = std::move(tmp);
    }
    // the same calls on clouds resident in HBM: nothing is uploaded or downloaded (the handles must
    // stay alive and unchanged until align has returned); output may be the source cloud itself
    void setInputSource(const DeviceCloud<PointSource> &cloud) { dsource_ = &cloud; source_.reset(); source_dirty_ = true; }
    void setInputTarget(const DeviceCloud<PointTarget> &cloud) { dtarget_ = &cloud; target_.reset(); target_dirty_ = true; }
    // engine extra: with a device cloud as the target, keep the context's index when it was built from that very cloud
    // (unchanged since) by another ICP object of the same context, instead of building it again.  Off by default: PCL
    // rebuilds its kd-tree at every setInputTarget.
    void setReuseTargetIndex(bool on) { reuse_target_index_ = on; }
    void align(DeviceCloud<PointSource> &output) { align(output, Matrix4f::Identity()); }
    void align(DeviceCloud<PointSource> &output, const Matrix4f &guess)
    {
        if (!dsource_ || !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource / setInputTarget (device clouds) not called");
        rsreg_ctx *c = ctx_->get();
        const auto t0 = std::chrono::steady_clock::now();
        // a device cloud rewritten in place since it was loaded (filter(x, x), +=, a transform or an alignment into it) is
        // loaded again: PCL would see the new points through its pointer
        if (!source_dirty_ && cloud_stamp(dsource_->handle()) != source_stamp_) source_dirty_ = true;
        if (!target_dirty_ && cloud_stamp(dtarget_->handle()) != target_stamp_) target_dirty_ = true;
        if (source_dirty_ || ctx_->icp_source_owner != this) {
            check(rsreg_icp_set_source_cloud(c, dsource_->handle()), c);
            source_stamp_ = cloud_stamp(dsource_->handle());
            source_dirty_ = false;
            ctx_->icp_source_owner = this;
            src_normals_dirty_ = true;
        }
        t1_ = std::chrono::steady_clock::now();
        if (target_dirty_ || ctx_->icp_target_owner != this) {
            if (!(reuse_target_index_ && rsreg_icp_target_is_cloud(c, dtarget_->handle(), prm_.max_correspondence_distance)))
                check(rsreg_icp_set_target_cloud(c, dtarget_->handle(), prm_.max_correspondence_distance), c);
            target_stamp_ = cloud_stamp(dtarget_->handle());
            target_dirty_ = false;
            ctx_->icp_target_owner = this;
            target_normals_set_ = false;
            target_set_(c, true);
        } else {
            target_set_(c, false);
        }
        set_rejectors_(c);
        const auto t2 = std::chrono::steady_clock::now();
        check(rsreg_icp_align_cloud(c, guess.data(), &prm_, &res_, output.handle()), c);
        std::memcpy(final_.m, res_.transform, sizeof(final_.m));
        fetch_rejector_stats_(c);
        const auto t3 = std::chrono::steady_clock::now();
        call_ms[0] += std::chrono::duration<double, std::milli>(t1_ - t0).count();
        call_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1_).count();
        call_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    }
    // engine extra: host time of the device-cloud align() calls so far, in ms -- [0] loading the source (and waiting for whatever
    // still makes it), [1] the target's index, [2] the alignment itself
    double call_ms[3] = {0, 0, 0};
    bool hasConverged() const { return res_.converged != 0; }
    Matrix4f getFinalTransformation() const { return final_; }
    int getConvergenceState() const { return res_.state; }
    // Registration::getFitnessScore(max_range) of the last align() (host or device clouds): the mean squared distance from every
    // finite source point at the final pose to its nearest target point, over the points whose SQUARED distance is <= max_range
    // (PCL's quirk, kept); DBL_MAX when none is.  Throws rsreg::Error before an align() of the current source and target.
    double getFitnessScore(double max_range = std::numeric_limits<double>::max())
    {
        rsreg_ctx *c = ctx_->get();
        if (source_dirty_ || target_dirty_ || ctx_->icp_source_owner != this || ctx_->icp_target_owner != this)
            throw Error(RSREG_ERR_STATE, "rsreg: getFitnessScore before align() of the current source and target");
        double score = 0;
        check(rsreg_icp_fitness_score(c, max_range, &score, nullptr), c);
        return score;
    }
    const rsreg_icp_result &result() const { return res_; }
    virtual ~IterativeClosestPoint() = default;

  protected:
    // the context holds this object's target (`fresh`: it has just been set): what a derived class hands over with it
    // (IterativeClosestPointWithNormals: the target's normals, which a new target drops)
    // (here: a target whose records carry normals hands them over when the chain's normal test will read them)
    virtual void target_set_(rsreg_ctx *c, bool fresh)
    {
        if (!has_normal_rejector_() || !target_) return;
        if (fresh || !target_normals_set_) set_target_record_normals_(c, detail::has_normal<PointTarget>());
    }
    bool has_normal_rejector_() const
    {
        for (const auto &r : rejectors_)
            if (r->kind() == RSREG_REJECTOR_SURFACE_NORMAL) return true;
        return false;
    }
    // this object's chain onto the context (another object's may be there), and the source's normals if the chain reads them
    void set_rejectors_(rsreg_ctx *c)
    {
        rsreg_rejector chain[RSREG_MAX_REJECTORS];
        for (size_t i = 0; i < rejectors_.size(); ++i) chain[i] = rsreg_rejector{rejectors_[i]->kind(), 0, rejectors_[i]->value()};
        check(rsreg_icp_set_rejectors(c, rejectors_.empty() ? nullptr : chain, (int32_t)rejectors_.size()), c);
        if (!has_normal_rejector_() || !src_normals_dirty_) return;
        if (src_normals_)
            check(rsreg_icp_set_source_normals(c, src_normals_->points.data(), src_normals_->size(), sizeof(Normal)), c);
        else
            set_source_record_normals_(c, detail::has_normal<PointSource>());
        src_normals_dirty_ = false;
    }
    void fetch_rejector_stats_(rsreg_ctx *c)
    {
        if (rejectors_.empty()) return;
        rsreg_rejector_stat st[RSREG_MAX_REJECTORS];
        int32_t n = 0;
        if (rsreg_icp_rejector_stats(c, st, RSREG_MAX_REJECTORS, &n) != RSREG_OK) return;   // (an alignment that never searched)
        for (size_t i = 0; i < rejectors_.size() && i < (size_t)n; ++i) rejectors_[i]->set_stat_(st[i]);
    }
    void set_source_record_normals_(rsreg_ctx *c, std::true_type)
    {
        if (!source_) throw Error(RSREG_ERR_STATE, "rsreg: a device-cloud source needs setInputSourceNormals");
        const char *rec = reinterpret_cast<const char *>(source_->points.data());
        check(rsreg_icp_set_source_normals(c, source_->size() ? rec + offsetof(PointSource, data_n) : nullptr, source_->size(), sizeof(PointSource)), c);
    }
    void set_source_record_normals_(rsreg_ctx *, std::false_type)
    {
        throw Error(RSREG_ERR_STATE, "rsreg: the source's points carry no normals: setInputSourceNormals");
    }
    void set_target_record_normals_(rsreg_ctx *c, std::true_type)
    {
        const char *rec = reinterpret_cast<const char *>(target_->points.data());
        check(rsreg_icp_set_target_normals(c, target_->size() ? rec + offsetof(PointTarget, data_n) : nullptr, target_->size(), sizeof(PointTarget)), c);
        target_normals_set_ = true;
    }
    void set_target_record_normals_(rsreg_ctx *, std::false_type) {}   // (rsreg_icp_begin refuses the chain: RSREG_ERR_STATE)
    std::vector<CorrespondenceRejectorPtr> rejectors_;
    const PointCloud<Normal> *src_normals_ = nullptr;
    bool src_normals_dirty_ = true, target_normals_set_ = false;
    std::shared_ptr<Context> ctx_;
    rsreg_icp_params prm_;
    rsreg_icp_result res_{};
    Matrix4f final_;
    SourcePtr source_;
    TargetPtr target_;
    const DeviceCloud<PointSource> *dsource_ = nullptr;
    const DeviceCloud<PointTarget> *dtarget_ = nullptr;
    bool source_dirty_ = true, target_dirty_ = true, reuse_target_index_ = false;
    std::pair<uint64_t, uint64_t> source_stamp_{0, 0}, target_stamp_{0, 0};   // (id, version) of the device clouds as loaded
    std::chrono::steady_clock::time_point t1_;
};

// ---- pcl::IterativeClosestPointWithNormals: point-to-plane ICP with PCL's default estimator,
// TransformationEstimationPointToPlaneLLS (rsreg.h: rsreg_estimation, RSREG_NUM_PLANE_SUMS; the two stated deviations from
// PCL are there).  The target's normals come inside the target's records (a host cloud of PointXYZRGBNormal: xyz at stride
// 48, the normals at byte 16) or beside them: setInputTargetNormals, for PointXYZRGB targets plus NormalEstimation's output,
// on the host or in HBM.  align(out) copies the source records as IterativeClosestPoint does; the normals of the SOURCE
// records, if they carry any, are not rotated in `out` (PCL rotates them; nothing downstream reads them).
template <typename PointSource, typename PointTarget>
class IterativeClosestPointWithNormals : public IterativeClosestPoint<PointSource, PointTarget> {
    using Base = IterativeClosestPoint<PointSource, PointTarget>;

  public:
    explicit IterativeClosestPointWithNormals(std::shared_ptr<Context> ctx = Context::Default()) : Base(std::move(ctx))
    {
        this->prm_.estimation = RSREG_ESTIMATION_POINT_TO_PLANE_LLS;
    }
    // one normal per target record; the cloud must stay alive and unchanged until align has returned
    void setInputTargetNormals(const PointCloud<Normal> &normals) { normals_ = &normals; dnormals_ = nullptr; normals_dirty_ = true; }
    void setInputTargetNormals(const DeviceCloud<Normal> &normals) { dnormals_ = &normals; normals_ = nullptr; normals_dirty_ = true; }

  protected:
    void target_set_(rsreg_ctx *c, bool fresh) override
    {
        if (dnormals_ && cloud_stamp(dnormals_->handle()) != normals_stamp_) normals_dirty_ = true;   // (rewritten in place since)
        if (!fresh && !normals_dirty_) return;
        if (dnormals_) {
            check(rsreg_icp_set_target_normals_cloud(c, dnormals_->handle()), c);
            normals_stamp_ = cloud_stamp(dnormals_->handle());
        } else if (normals_) {
            check(rsreg_icp_set_target_normals(c, normals_->points.data(), normals_->size(), sizeof(Normal)), c);
        } else {
            set_record_normals_(c, detail::has_normal<PointTarget>());
        }
        normals_dirty_ = false;
    }

  private:
    void set_record_normals_(rsreg_ctx *c, std::true_type)
    {
        if (!this->target_) throw Error(RSREG_ERR_STATE, "rsreg: a device-cloud target needs setInputTargetNormals");
        const char *rec = reinterpret_cast<const char *>(this->target_->points.data());
        check(rsreg_icp_set_target_normals(c, this->target_->size() ? rec + offsetof(PointTarget, data_n) : nullptr, this->target_->size(),
                                           sizeof(PointTarget)), c);
    }
    void set_record_normals_(rsreg_ctx *, std::false_type)
    {
        throw Error(RSREG_ERR_STATE, "rsreg: the target's points carry no normals: setInputTargetNormals");
    }
    const PointCloud<Normal> *normals_ = nullptr;
    const DeviceCloud<Normal> *dnormals_ = nullptr;
    bool normals_dirty_ = true;
    std::pair<uint64_t, uint64_t> normals_stamp_{0, 0};
};

// ---- pcl::GeneralizedIterativeClosestPoint: plane-to-plane ICP (rsreg.h: the rsreg_gicp_* section holds the contract and the
// stated deviations from PCL -- I - (1 - eps) n n^T in the place of the SVD rebuild, f64 fixed-order sums, Gauss-Newton with step
// halving in the place of PCL's BFGS).  Covariances: six doubles a record (xx, xy, xz, yy, yz, zz) in the caller's order; a cloud
// without them gets its own from rsreg_cloud_gicp_covariances on a device cloud, with setCorrespondenceRandomness' k, as PCL
// computes them in computeTransformation when none are given.
using GicpCovariances = std::vector<std::array<double, 6>>;
template <typename PointSource, typename PointTarget> class GeneralizedIterativeClosestPoint {
  public:
    using SourcePtr = typename PointCloud<PointSource>::Ptr;
    using TargetPtr = typename PointCloud<PointTarget>::Ptr;
    using CovariancesPtr = std::shared_ptr<const GicpCovariances>;

    explicit GeneralizedIterativeClosestPoint(std::shared_ptr<Context> ctx = Context::Default()) : ctx_(std::move(ctx))
    {
        rsreg_gicp_params_default(&prm_);
        final_ = Matrix4f::Identity();
    }
    virtual ~GeneralizedIterativeClosestPoint() = default;
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; source_cov_dirty_ = target_cov_dirty_ = true; }
    int getCorrespondenceRandomness() const { return prm_.k_correspondences; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setMaximumOptimizerIterations(int n) { prm_.max_inner_iterations = n; }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    void setMaxCorrespondenceDistance(double d)
    {
        if (d != prm_.max_correspondence_distance) target_dirty_ = true;  // the index cell size derives from it
        prm_.max_correspondence_distance = d;
    }
    void setInputSource(const SourcePtr &cloud) { source_ = cloud; source_cov_.reset(); source_dirty_ = true; }
    void setInputTarget(const TargetPtr &cloud) { target_ = cloud; target_cov_.reset(); target_dirty_ = true; }
    // one record per source / target point; call them after setInputSource / setInputTarget (a new cloud drops them, as in PCL)
    void setSourceCovariances(const CovariancesPtr &cov) { source_cov_ = cov; source_cov_dirty_ = true; }
    void setTargetCovariances(const CovariancesPtr &cov) { target_cov_ = cov; target_cov_dirty_ = true; }

    void align(PointCloud<PointSource> &output) { align(output, Matrix4f::Identity()); }
    void align(PointCloud<PointSource> &output, const Matrix4f &guess)
    {
        if (!source_ || !target_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource / setInputTarget not called");
        rsreg_ctx *c = ctx_->get();
        bool source_new = false, target_new = false;
        if (source_dirty_ || ctx_->icp_source_owner != this) {
            check(rsreg_icp_set_source(c, source_->points.data(), source_->size(), sizeof(PointSource), source_->is_dense), c);
            source_dirty_ = false;
            source_cov_dirty_ = true;   // (a new source drops the covariances of the one before)
            source_new = true;
            ctx_->icp_source_owner = this;
        }
        if (target_dirty_ || ctx_->icp_target_owner != this) {
            check(rsreg_icp_set_target(c, target_->points.data(), target_->size(), sizeof(PointTarget), target_->is_dense,
                                       prm_.max_correspondence_distance), c);
            target_dirty_ = false;
            target_cov_dirty_ = true;
            target_new = true;
            ctx_->icp_target_owner = this;
        }
        if (source_cov_dirty_) {
            if (source_cov_) check(rsreg_gicp_set_source_covariances(c, source_cov_->data(), source_cov_->size(), sizeof(std::array<double, 6>)), c);
            else compute_covariances_(*source_, true);
            source_cov_dirty_ = false;
        }
        if (target_cov_dirty_) {
            if (target_cov_) check(rsreg_gicp_set_target_covariances(c, target_cov_->data(), target_cov_->size(), sizeof(std::array<double, 6>)), c);
            else compute_covariances_(*target_, false);
            target_cov_dirty_ = false;
        }
        sync_more_(c, source_new, target_new);
        PointCloud<PointSource> tmp;
        detail::copy_aligned(*source_, tmp);   // `output = input`, then xyz <- final * xyz
        check(run_(c, guess.data(), tmp.size() ? tmp.points.data() : nullptr, sizeof(PointSource)), c);
        std::memcpy(final_.m, res_.transform, sizeof(final_.m));
        output = std::move(tmp);
    }
    bool hasConverged() const { return res_.converged != 0; }
    Matrix4f getFinalTransformation() const { return final_; }
    double getFitnessScore(double max_range = std::numeric_limits<double>::max())
    {
        rsreg_ctx *c = ctx_->get();
        if (source_dirty_ || target_dirty_ || ctx_->icp_source_owner != this || ctx_->icp_target_owner != this)
            throw Error(RSREG_ERR_STATE, "rsreg: getFitnessScore before align() of the current source and target");
        double score = 0;
        check(rsreg_icp_fitness_score(c, max_range, &score, nullptr), c);
        return score;
    }
    const rsreg_gicp_result &result() const { return res_; }

  protected:
    // what a derived alignment (GeneralizedIterativeClosestPoint6D) hands the context besides clouds and covariances, and its loop
    virtual void sync_more_(rsreg_ctx *, bool /*source_new*/, bool /*target_new*/) {}
    virtual int run_(rsreg_ctx *c, const float *guess, void *aligned_out, size_t stride) { return rsreg_gicp_align(c, guess, &prm_, &res_, aligned_out, stride); }
    template <typename PointT> void compute_covariances_(const PointCloud<PointT> &cloud, bool source)
    {
        rsreg_ctx *c = ctx_->get();
        DeviceCloud<PointT> dev(cloud, ctx_);
        rsreg_cloud *cov = nullptr;
        check(rsreg_cloud_create(c, &cov), c);
        int rc = rsreg_cloud_gicp_covariances(c, dev.handle(), prm_.k_correspondences, prm_.gicp_epsilon, cov);
        if (!rc) rc = source ? rsreg_gicp_set_source_covariances_cloud(c, cov) : rsreg_gicp_set_target_covariances_cloud(c, cov);
        if (!rc) rc = rsreg_ctx_synchronize(c);   // (the copy reads `cov` on the context's stream: done before the handle goes)
        rsreg_cloud_destroy(cov);
        check(rc, c);
    }
    std::shared_ptr<Context> ctx_;
    rsreg_gicp_params prm_;
    rsreg_gicp_result res_{};
    Matrix4f final_;
    SourcePtr source_;
    TargetPtr target_;
    CovariancesPtr source_cov_, target_cov_;
    bool source_dirty_ = true, target_dirty_ = true, source_cov_dirty_ = true, target_cov_dirty_ = true;
};

// ---- pcl::GeneralizedIterativeClosestPoint6D: GICP whose correspondences are nearest neighbours in (x, y, z, w L', w a', w b')
// (rsreg.h: the GICP6D section).  Otherwise GICP's surface.  The colours come from the clouds' own rgb words (rsreg_cloud_lab on a
// device cloud) unless setSourceLab / setTargetLab hand them in: three floats L', a', b' a record, in the caller's order.
using LabColours = std::vector<std::array<float, 3>>;
template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint6D : public GeneralizedIterativeClosestPoint<PointSource, PointTarget> {
    using Base = GeneralizedIterativeClosestPoint<PointSource, PointTarget>;

  public:
    using LabPtr = std::shared_ptr<const LabColours>;
    explicit GeneralizedIterativeClosestPoint6D(float lab_weight = 0.032f, std::shared_ptr<Context> ctx = Context::Default())
        : Base(std::move(ctx)), lab_weight_(lab_weight)
    {
    }
    void setLabWeight(float w) { lab_weight_ = w; }
    float getLabWeight() const { return lab_weight_; }
    void setInputSource(const typename Base::SourcePtr &cloud) { Base::setInputSource(cloud); source_lab_.reset(); source_lab_dirty_ = true; }
    void setInputTarget(const typename Base::TargetPtr &cloud) { Base::setInputTarget(cloud); target_lab_.reset(); target_lab_dirty_ = true; }
    // one record per source / target point; call them after setInputSource / setInputTarget (a new cloud drops them)
    void setSourceLab(const LabPtr &lab) { source_lab_ = lab; source_lab_dirty_ = true; }
    void setTargetLab(const LabPtr &lab) { target_lab_ = lab; target_lab_dirty_ = true; }

  protected:
    void sync_more_(rsreg_ctx *c, bool source_new, bool target_new) override
    {
        if (source_new || source_lab_dirty_) {
            if (source_lab_) check(rsreg_gicp_set_source_lab(c, source_lab_->data(), source_lab_->size(), sizeof(std::array<float, 3>)), c);
            else compute_lab_(*this->source_, true);
            source_lab_dirty_ = false;
        }
        if (target_new || target_lab_dirty_) {
            if (target_lab_) check(rsreg_gicp_set_target_lab(c, target_lab_->data(), target_lab_->size(), sizeof(std::array<float, 3>)), c);
            else compute_lab_(*this->target_, false);
            target_lab_dirty_ = false;
        }
    }
    int run_(rsreg_ctx *c, const float *guess, void *aligned_out, size_t stride) override
    {
        return rsreg_gicp6d_align(c, guess, &this->prm_, (double)lab_weight_, &this->res_, aligned_out, stride);
    }

  private:
    template <typename PointT> void compute_lab_(const PointCloud<PointT> &cloud, bool source)
    {
        rsreg_ctx *c = this->ctx_->get();
        DeviceCloud<PointT> dev(cloud, this->ctx_);
        rsreg_cloud *lab = nullptr;
        check(rsreg_cloud_create(c, &lab), c);
        int rc = rsreg_cloud_lab(c, dev.handle(), lab);
        if (!rc) rc = source ? rsreg_gicp_set_source_lab_cloud(c, lab) : rsreg_gicp_set_target_lab_cloud(c, lab);
        if (!rc) rc = rsreg_ctx_synchronize(c);   // (the copy reads `lab` on the context's stream: done before the handle goes)
        rsreg_cloud_destroy(lab);
        check(rc, c);
    }
    float lab_weight_;
    LabPtr source_lab_, target_lab_;
    bool source_lab_dirty_ = true, target_lab_dirty_ = true;
};

// ---- pcl::NormalDistributionsTransform
template <typename PointSource, typename PointTarget> class NormalDistributionsTransform {
  public:
    using SourcePtr = typename PointCloud<PointSource>::Ptr;
    using TargetPtr = typename PointCloud<PointTarget>::Ptr;

    explicit NormalDistributionsTransform(std::shared_ptr<Context> ctx = Context::Default()) : ctx_(std::move(ctx))
    {
        rsreg_ndt_params_default(&prm_);
        final_ = Matrix4f::Identity();
    }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setStepSize(double s) { prm_.step_size = s; }
    void setResolution(float r)
    {
        if ((double)r != prm_.resolution) target_dirty_ = true;
        prm_.resolution = r;
    }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    // engine extra: search the voxels by PCL's own centroid arithmetic (float running sum per voxel in input order,
    // rsreg_ndt_set_centroid_mode) instead of the rounded f64 mean
    void setPclCentroids(bool on)
    {
        if (on != pcl_centroids_) target_dirty_ = true;
        pcl_centroids_ = on;
    }
    void setInputSource(const SourcePtr &cloud) { source_ = cloud; dsource_ = nullptr; fit_fresh_ = false; }
    void setInputTarget(const TargetPtr &cloud) { target_ = cloud; dtarget_ = nullptr; target_dirty_ = true; fit_fresh_ = false; }

    void align(PointCloud<PointSource> &output) { align(output, Matrix4f::Identity()); }
    void align(PointCloud<PointSource> &output, const Matrix4f &guess)
    {
        if (!source_ || !target_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource / setInputTarget not called");
        rsreg_ctx *c = ctx_->get();
        if (target_dirty_ || ctx_->ndt_target_owner != this) {
            check(rsreg_ndt_set_centroid_mode(c, pcl_centroids_ ? 1 : 0), c);
            check(rsreg_ndt_set_target(c, target_->points.data(), target_->size(), sizeof(PointTarget), target_->is_dense,
                                       prm_.resolution), c);
            target_dirty_ = false;
            ctx_->ndt_target_owner = this;
        }
        PointCloud<PointSource> tmp;
        detail::copy_aligned(*source_, tmp);
        check(rsreg_ndt_align(c, source_->points.data(), source_->size(), sizeof(PointSource), source_->is_dense, guess.data(),
                              &prm_, &res_, tmp.points.data(), sizeof(PointSource)), c);
        std::memcpy(final_.m, res_.transform, sizeof(final_.m));
        fit_fresh_ = true;
        output = std::move(tmp);
    }
    void setInputSource(const DeviceCloud<PointSource> &cloud) { dsource_ = &cloud; source_.reset(); fit_fresh_ = false; }
    void setInputTarget(const DeviceCloud<PointTarget> &cloud) { dtarget_ = &cloud; target_.reset(); target_dirty_ = true; fit_fresh_ = false; }
    void align(DeviceCloud<PointSource> &output) { align(output, Matrix4f::Identity()); }
    void align(DeviceCloud<PointSource> &output, const Matrix4f &guess)
    {
        if (!dsource_ || !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource / setInputTarget (device clouds) not called");
        rsreg_ctx *c = ctx_->get();
        if (!target_dirty_ && cloud_stamp(dtarget_->handle()) != target_stamp_) target_dirty_ = true;   // rewritten in place since
        if (target_dirty_ || ctx_->ndt_target_owner != this) {
            check(rsreg_ndt_set_centroid_mode(c, pcl_centroids_ ? 1 : 0), c);
            check(rsreg_ndt_set_target_cloud(c, dtarget_->handle(), prm_.resolution), c);
            target_stamp_ = cloud_stamp(dtarget_->handle());
            target_dirty_ = false;
            ctx_->ndt_target_owner = this;
        }
        check(rsreg_ndt_align_cloud(c, dsource_->handle(), guess.data(), &prm_, &res_, output.handle()), c);
        std::memcpy(final_.m, res_.transform, sizeof(final_.m));
        fit_fresh_ = true;
    }
    bool hasConverged() const { return res_.converged != 0; }
    Matrix4f getFinalTransformation() const { return final_; }
    double getTransformationProbability() const { return res_.trans_probability; }
    // Registration::getFitnessScore(max_range) of the last align(), against the target's POINTS as PCL scores NDT; the same
    // squared-range quirk and DBL_MAX as IterativeClosestPoint::getFitnessScore.  Throws rsreg::Error before an align().
    double getFitnessScore(double max_range = std::numeric_limits<double>::max())
    {
        rsreg_ctx *c = ctx_->get();
        if (!fit_fresh_ || ctx_->ndt_target_owner != this)
            throw Error(RSREG_ERR_STATE, "rsreg: getFitnessScore before align() of the current source and target");
        double score = 0;
        check(rsreg_ndt_fitness_score(c, max_range, &score, nullptr), c);
        return score;
    }
    int getFinalNumIteration() const { return res_.iterations; }
    const rsreg_ndt_result &result() const { return res_; }

  private:
    std::shared_ptr<Context> ctx_;
    rsreg_ndt_params prm_;
    rsreg_ndt_result res_{};
    Matrix4f final_;
    SourcePtr source_;
    TargetPtr target_;
    const DeviceCloud<PointSource> *dsource_ = nullptr;
    const DeviceCloud<PointTarget> *dtarget_ = nullptr;
    bool target_dirty_ = true, pcl_centroids_ = false;
    bool fit_fresh_ = false;   // the last align() is of the current source and target (getFitnessScore)
    std::pair<uint64_t, uint64_t> target_stamp_{0, 0};   // (id, version) of the device target as loaded
};

// ---- pcl::ApproximateVoxelGrid (host, sequential: order-dependent by definition)
// Default-constructed: the sequential host filter.  With a Context: the same filter on the GPU
// (csrc/voxel.hip), same records in the same order.
template <typename PointT> class ApproximateVoxelGrid {
  public:
    ApproximateVoxelGrid() = default;
    explicit ApproximateVoxelGrid(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz; }
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void filter(PointCloud<PointT> &output)  // output may be *input (the reference filters in place)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        PointVector<PointT> out = uninitialized_points<PointT>(input_->size());
        size_t n_out = 0;
        if (ctx_)
            check(rsreg_approx_voxel_grid_gpu(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), leaf_, out.data(),
                                              &n_out), ctx_->get());
        else
            check(rsreg_approx_voxel_grid(input_->points.data(), input_->size(), sizeof(PointT), leaf_, out.data(), &n_out));
        out.resize(n_out);
        output.points = std::move(out);
        output.width = (uint32_t)n_out;
        output.height = 1;
        output.is_dense = false;
    }
    // the filter on a cloud resident in HBM (always the GPU filter); output may be the input
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)
    {
        check(rsreg_cloud_filter(input.context()->get(), input.handle(), leaf_, output.handle()), input.context()->get());
    }
    // the same on the context's side stream: returns once the size of the result is known, the voxel sums still
    // running; whatever touches `output` next waits for them.  `input` must stay alive and unchanged until then;
    // output must not be the input (rsreg_cloud_filter_async)
    void filter_async(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)
    {
        check(rsreg_cloud_filter_async(input.context()->get(), input.handle(), leaf_, output.handle()), input.context()->get());
    }
  private:
    float leaf_[3] = {1.f, 1.f, 1.f};  // PCL default: IncrementalICP never sets it (incremental_icp.hpp:36)
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::VoxelGrid<PointT>: one centroid per occupied leaf, in ascending leaf index; a leaf's points are added in ascending
// input index (include/rsreg.h, "pcl::VoxelGrid", is the contract and states that one choice).  Default-constructed: the
// sequential host restatement.  With a Context: the GPU filter (csrc/voxel.hip), the same bytes.  Not built: the filter-field
// limits (run PassThrough first) and the saved leaf layout.
template <typename PointT> class VoxelGrid {
  public:
    VoxelGrid() { rsreg_voxel_grid_params_default(&prm_); }
    explicit VoxelGrid(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { rsreg_voxel_grid_params_default(&prm_); }
    void setLeafSize(float lx, float ly, float lz) { prm_.leaf[0] = lx; prm_.leaf[1] = ly; prm_.leaf[2] = lz; }
    void setLeafSize(float l) { setLeafSize(l, l, l); }
    void setDownsampleAllData(bool on) { prm_.downsample_all_data = on ? 1 : 0; }
    bool getDownsampleAllData() const { return prm_.downsample_all_data != 0; }
    void setMinimumPointsNumberPerVoxel(unsigned int n) { prm_.min_points_per_voxel = n; }
    unsigned int getMinimumPointsNumberPerVoxel() const { return prm_.min_points_per_voxel; }
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    // of the last filter(): three ints each, as PCL's Eigen::Vector3i
    std::array<int, 3> getMinBoxCoordinates() const { return {info_.min_b[0], info_.min_b[1], info_.min_b[2]}; }
    std::array<int, 3> getMaxBoxCoordinates() const { return {info_.max_b[0], info_.max_b[1], info_.max_b[2]}; }
    std::array<int, 3> getNrDivisions() const { return {info_.div_b[0], info_.div_b[1], info_.div_b[2]}; }
    std::array<int, 3> getDivisionMultiplier() const { return {info_.divb_mul[0], info_.divb_mul[1], info_.divb_mul[2]}; }
    const rsreg_voxel_grid_info &info() const { return info_; }   // engine extra: the counts, and whether the leaf was too small
    void filter(PointCloud<PointT> &output)  // output may be *input
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        PointVector<PointT> out = uninitialized_points<PointT>(input_->size());
        size_t n_out = 0;
        if (ctx_)
            check(rsreg_voxel_grid_gpu(ctx_->get(), input_->points.data(), input_->size(), sizeof(PointT), &prm_, out.data(), &n_out, &info_),
                  ctx_->get());
        else
            check(rsreg_voxel_grid(input_->points.data(), input_->size(), sizeof(PointT), prm_.leaf, prm_.downsample_all_data,
                                   prm_.min_points_per_voxel, out.data(), &n_out, &info_));
        out.resize(n_out);
        const uint32_t w = input_->width, h = input_->height;
        const bool dense = input_->is_dense;
        output.points = std::move(out);
        // (PCL: a leaf too small for the box leaves the output a copy of the input)
        output.width = info_.overflowed ? w : (uint32_t)n_out;
        output.height = info_.overflowed ? h : 1;
        output.is_dense = info_.overflowed ? dense : true;
    }
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)  // output may be the input
    {
        check(rsreg_cloud_voxel_grid(input.context()->get(), input.handle(), &prm_, output.handle(), &info_), input.context()->get());
    }
  private:
    rsreg_voxel_grid_params prm_;
    rsreg_voxel_grid_info info_{};
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::PassThrough<PointT> for the fields "x", "y" and "z" (csrc/filters.hip, rsreg_cloud_passthrough): the first step of the
// reference's pre-filter (src/capture.hpp:112-132).  A record with a non-finite coordinate is always removed.  Any other field
// name throws RSREG_ERR_INVALID_ARG from filter() (PCL warns and returns an empty cloud).  Always on the GPU: the host-cloud
// form goes through a temporary DeviceCloud.
template <typename PointT> class PassThrough {
  public:
    PassThrough() = default;
    explicit PassThrough(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void setFilterFieldName(const std::string &name) { field_ = name; }
    void setFilterLimits(float lo, float hi) { lo_ = lo; hi_ = hi; }
    void setNegative(bool negative) { negative_ = negative; }
    void setFilterLimitsNegative(bool negative) { negative_ = negative; }   // (PCL's older spelling)
    void setKeepOrganized(bool keep) { keep_organized_ = keep; }
    void filter(PointCloud<PointT> &output)  // output may be *input
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        filter(tmp, tmp);
        tmp.download(output);
    }
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)  // output may be the input
    {
        const int field = field_ == "x" ? 0 : (field_ == "y" ? 1 : (field_ == "z" ? 2 : -1));
        check(rsreg_cloud_passthrough(input.context()->get(), input.handle(), field, lo_, hi_, negative_, keep_organized_, output.handle()),
              input.context()->get());
    }
  private:
    std::string field_;
    float lo_ = FLT_MIN, hi_ = FLT_MAX;   // PCL's defaults
    bool negative_ = false, keep_organized_ = false;
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::StatisticalOutlierRemoval<PointT> with an exact k-nearest-neighbour search on the GPU (csrc/filters.hip,
// rsreg_cloud_sor): the second step of the reference's pre-filter.  PCL's defaults: mean_k = 1, stddev_mult = 0.
template <typename PointT> class StatisticalOutlierRemoval {
  public:
    StatisticalOutlierRemoval() = default;
    explicit StatisticalOutlierRemoval(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void setMeanK(int k) { mean_k_ = k; }
    void setStddevMulThresh(double m) { stddev_mult_ = m; }
    void setNegative(bool negative) { negative_ = negative; }
    void filter(PointCloud<PointT> &output)  // output may be *input
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        filter(tmp, tmp);
        tmp.download(output);
    }
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)  // output may be the input
    {
        check(rsreg_cloud_sor(input.context()->get(), input.handle(), mean_k_, stddev_mult_, negative_, output.handle(), &stats_),
              input.context()->get());
    }
    const rsreg_sor_stats &stats() const { return stats_; }   // engine extra: the last filter()'s mean, stddev and threshold
  private:
    int mean_k_ = 1;
    double stddev_mult_ = 0.0;
    bool negative_ = false;
    rsreg_sor_stats stats_{};
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::RadiusOutlierRemoval<PointT> over an exact radius search on the GPU (csrc/radius_kernels.hpp,
// rsreg_cloud_radius_outlier_removal): a record is removed when it has min_neighbors or fewer neighbours within the radius, itself
// counted, the compare at the radius strict (include/rsreg.h states the one deviation from PCL's dense-cloud shortcut).  PCL's
// defaults: radius 0 (filter() refuses it), min_neighbors 1.
template <typename PointT> class RadiusOutlierRemoval {
  public:
    RadiusOutlierRemoval() = default;
    explicit RadiusOutlierRemoval(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void setRadiusSearch(double radius) { radius_ = radius; }
    double getRadiusSearch() const { return radius_; }
    void setMinNeighborsInRadius(int m) { min_neighbors_ = m; }
    int getMinNeighborsInRadius() const { return min_neighbors_; }
    void setNegative(bool negative) { negative_ = negative; }
    void setKeepOrganized(bool keep) { keep_organized_ = keep; }
    void filter(PointCloud<PointT> &output)  // output may be *input
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        filter(tmp, tmp);
        tmp.download(output);
    }
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)  // output may be the input
    {
        check(rsreg_cloud_radius_outlier_removal(input.context()->get(), input.handle(), radius_, min_neighbors_, negative_, keep_organized_,
                                                 output.handle(), &n_kept_),
              input.context()->get());
    }
    uint64_t kept() const { return n_kept_; }   // engine extra: the last filter()'s number of kept records
  private:
    double radius_ = 0.0;
    int min_neighbors_ = 1;
    bool negative_ = false, keep_organized_ = false;
    uint64_t n_kept_ = 0;
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::EuclideanClusterExtraction<PointT> over the exact radius search on the GPU (csrc/cluster_kernels.hpp,
// rsreg_cloud_euclidean_clusters; include/rsreg.h holds the contract and the stated deviations: ties between equal sizes go to the
// cluster with the lower smallest record, a non-finite record belongs to no cluster).  extract(): the clusters by size descending,
// the record indices of each ascending.  PCL's defaults: tolerance 0 (extract() refuses it), sizes 1 .. INT_MAX.  No setIndices,
// no setSearchMethod.
struct PointIndices {
    std::vector<int> indices;
};

template <typename PointT> class EuclideanClusterExtraction {
  public:
    EuclideanClusterExtraction() { rsreg_cluster_params_default(&params_); }
    explicit EuclideanClusterExtraction(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { rsreg_cluster_params_default(&params_); }
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud, dinput_ = nullptr; }
    void setInputCloud(const DeviceCloud<PointT> &cloud) { dinput_ = &cloud, input_.reset(); }   // (must outlive extract())
    void setClusterTolerance(double tolerance) { params_.tolerance = tolerance; }
    double getClusterTolerance() const { return params_.tolerance; }
    void setMinClusterSize(int m) { params_.min_cluster_size = (uint32_t)m; }
    int getMinClusterSize() const { return (int)params_.min_cluster_size; }
    void setMaxClusterSize(int m) { params_.max_cluster_size = (uint32_t)m; }
    int getMaxClusterSize() const { return (int)params_.max_cluster_size; }
    void extract(std::vector<PointIndices> &clusters)
    {
        if (dinput_) return extract(*dinput_, clusters);
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        extract(tmp, clusters);
    }
    void extract(const DeviceCloud<PointT> &input, std::vector<PointIndices> &clusters)
    {
        rsreg_ctx *c = input.context()->get();
        const size_t n = input.size();
        std::vector<uint32_t> indices(n), offsets(n + 1);
        uint32_t found = 0;
        check(rsreg_cloud_euclidean_clusters(c, input.handle(), &params_, nullptr, indices.data(), offsets.data(), (uint32_t)n, &found), c);
        clusters.assign(found, PointIndices{});
        for (uint32_t k = 0; k < found; ++k) clusters[k].indices.assign(indices.begin() + offsets[k], indices.begin() + offsets[k + 1]);
    }
  private:
    rsreg_cluster_params params_;
    typename PointCloud<PointT>::Ptr input_;
    const DeviceCloud<PointT> *dinput_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::SACSegmentation<PointT> on the GPU for SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE with SAC_RANSAC
// (csrc/plane_seg_kernels.hpp, rsreg_cloud_plane_segment; include/rsreg.h holds the contract and the stated deviations: the
// counter-based sampler, the cosine form of the axis test, the double sums of the refinement).  segment(): the inliers' record
// indices ascending and the four coefficients; both empty when no model was found, as in PCL.  PCL's defaults: max_iterations 50,
// probability 0.99, optimize_coefficients on, distance_threshold 0.  setSeed is the one addition.  No setIndices, no other model or
// method: setModelType / setMethodType throw RSREG_ERR_INVALID_ARG for them.
enum SacModel { SACMODEL_PLANE = 0, SACMODEL_PERPENDICULAR_PLANE = 9 };   // pcl::SacModel's values
constexpr int SAC_RANSAC = 0;                                             // pcl::SAC_RANSAC

struct ModelCoefficients {
    std::vector<float> values;
};

template <typename PointT> class SACSegmentation {
  public:
    SACSegmentation() { rsreg_plane_params_default(&params_); }
    explicit SACSegmentation(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { rsreg_plane_params_default(&params_); }
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud, dinput_ = nullptr; }
    void setInputCloud(const DeviceCloud<PointT> &cloud) { dinput_ = &cloud, input_.reset(); }   // (must outlive segment())
    void setModelType(int model)
    {
        if (model != SACMODEL_PLANE && model != SACMODEL_PERPENDICULAR_PLANE)
            throw Error(RSREG_ERR_INVALID_ARG, "rsreg: SACSegmentation fits SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE only");
        model_ = model;
    }
    int getModelType() const { return model_; }
    void setMethodType(int method)
    {
        if (method != SAC_RANSAC) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: SACSegmentation runs SAC_RANSAC only");
    }
    int getMethodType() const { return SAC_RANSAC; }
    void setDistanceThreshold(double threshold) { params_.distance_threshold = threshold; }
    double getDistanceThreshold() const { return params_.distance_threshold; }
    void setMaxIterations(int n) { params_.max_iterations = n; }
    int getMaxIterations() const { return params_.max_iterations; }
    void setProbability(double p) { params_.probability = p; }
    double getProbability() const { return params_.probability; }
    void setOptimizeCoefficients(bool on) { params_.optimize_coefficients = on ? 1 : 0; }
    bool getOptimizeCoefficients() const { return params_.optimize_coefficients != 0; }
    template <typename Vector3> void setAxis(const Vector3 &axis) { for (int k = 0; k < 3; ++k) params_.axis[k] = (double)axis[k]; }   // (Eigen::Vector3f, float[3], ..)
    void setAxis(double x, double y, double z) { params_.axis[0] = x, params_.axis[1] = y, params_.axis[2] = z; }
    const double *getAxis() const { return params_.axis; }
    void setEpsAngle(double eps) { params_.eps_angle = eps; }
    double getEpsAngle() const { return params_.eps_angle; }
    void setSeed(uint64_t seed) { params_.seed = seed; }
    void segment(PointIndices &inliers, ModelCoefficients &coefficients)
    {
        if (dinput_) return segment(*dinput_, inliers, coefficients);
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        segment(tmp, inliers, coefficients);
    }
    void segment(const DeviceCloud<PointT> &input, PointIndices &inliers, ModelCoefficients &coefficients)
    {
        rsreg_ctx *c = input.context()->get();
        rsreg_plane_params p = params_;
        if (model_ == SACMODEL_PLANE) p.axis[0] = p.axis[1] = p.axis[2] = p.eps_angle = 0.0;   // (PCL's plain plane model ignores the axis)
        const size_t n = input.size();
        std::vector<int32_t> idx(n);
        float coeff[4];
        size_t found = 0;
        check(rsreg_cloud_plane_segment(c, input.handle(), &p, coeff, n ? idx.data() : nullptr, n, &found, &result_), c);
        inliers.indices.assign(idx.begin(), idx.begin() + (found < n ? found : n));
        if (result_.found) coefficients.values.assign(coeff, coeff + 4);
        else coefficients.values.clear();
    }
    const rsreg_plane_result &result() const { return result_; }   // engine extra: the last segment()'s iterations, sample and sums
  private:
    rsreg_plane_params params_;
    rsreg_plane_result result_{};
    int model_ = SACMODEL_PLANE;
    typename PointCloud<PointT>::Ptr input_;
    const DeviceCloud<PointT> *dinput_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::ExtractIndices<PointT> on the GPU (rsreg_cloud_extract_indices): the records an index list names, in its order and with
// its repeats; setNegative(true): the records it does not name, in input order.  No setKeepOrganized, no setUserFilterValue.
template <typename PointT> class ExtractIndices {
  public:
    ExtractIndices() = default;
    explicit ExtractIndices(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointT>::Ptr &cloud) { input_ = cloud; }
    void setIndices(const std::shared_ptr<const PointIndices> &indices) { indices_.assign(indices->indices.begin(), indices->indices.end()); }
    void setIndices(const PointIndices &indices) { indices_.assign(indices.indices.begin(), indices.indices.end()); }
    void setNegative(bool negative) { negative_ = negative; }
    bool getNegative() const { return negative_; }
    void filter(PointCloud<PointT> &output)  // output may be *input
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        DeviceCloud<PointT> tmp(*input_, ctx_ ? ctx_ : Context::Default());
        filter(tmp, tmp);
        tmp.download(output);
    }
    void filter(const DeviceCloud<PointT> &input, DeviceCloud<PointT> &output)  // output may be the input
    {
        check(rsreg_cloud_extract_indices(input.context()->get(), input.handle(), indices_.data(), indices_.size(), negative_, output.handle(), &n_kept_),
              input.context()->get());
    }
    uint64_t kept() const { return n_kept_; }   // engine extra: the last filter()'s number of kept records
  private:
    std::vector<int32_t> indices_;
    bool negative_ = false;
    uint64_t n_kept_ = 0;
    typename PointCloud<PointT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::ISSKeypoint3D<PointInT, PointOutT> over the exact radius search on the GPU (csrc/iss_kernels.hpp,
// rsreg_cloud_iss_keypoints; include/rsreg.h holds the contract and the one stated deviation, the eigen-solve): the records whose
// scatter over the salient radius has eigenvalue ratios below the two thresholds and whose smallest eigenvalue no neighbour within
// the non-max radius exceeds, in ascending record index, every byte of a record kept.  PCL's defaults: both radii 0 (compute()
// refuses them), thresholds 0.975, min_neighbors 5.  Border estimation is not built: setBorderRadius / setNormalRadius above 0
// make compute() throw RSREG_ERR_INVALID_ARG.  No setIndices, no setSearchSurface.
template <typename PointInT, typename PointOutT = PointInT> class ISSKeypoint3D {
    static_assert(sizeof(PointOutT) == sizeof(PointInT), "the keypoints are the input's records");
  public:
    ISSKeypoint3D() { rsreg_iss_params_default(&params_); }
    explicit ISSKeypoint3D(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { rsreg_iss_params_default(&params_); }
    void setInputCloud(const typename PointCloud<PointInT>::Ptr &cloud) { input_ = cloud, dinput_ = nullptr; }
    void setInputCloud(const DeviceCloud<PointInT> &cloud) { dinput_ = &cloud, input_.reset(); }   // (must outlive compute())
    void setSalientRadius(double radius) { params_.salient_radius = radius; }
    void setNonMaxRadius(double radius) { params_.non_max_radius = radius; }
    void setThreshold21(double gamma_21) { params_.gamma_21 = gamma_21; }
    void setThreshold32(double gamma_32) { params_.gamma_32 = gamma_32; }
    void setMinNeighbors(int min_neighbors) { params_.min_neighbors = min_neighbors; }
    void setBorderRadius(double radius) { border_radius_ = radius; }
    void setNormalRadius(double radius) { normal_radius_ = radius; }
    void compute(PointCloud<PointOutT> &output)
    {
        check_built();
        if (dinput_) {
            DeviceCloud<PointOutT> out(dinput_->context());
            compute(*dinput_, out);
            out.download(output);
            return;
        }
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        const std::shared_ptr<Context> ctx = ctx_ ? ctx_ : Context::Default();
        DeviceCloud<PointInT> tmp(*input_, ctx);
        DeviceCloud<PointOutT> out(ctx);
        compute(tmp, out);
        out.download(output);
    }
    void compute(const DeviceCloud<PointInT> &input, DeviceCloud<PointOutT> &output)
    {
        check_built();
        rsreg_ctx *c = input.context()->get();
        indices_.assign(input.size(), 0);
        uint64_t found = 0;
        check(rsreg_cloud_iss_keypoints(c, input.handle(), &params_, output.handle(), indices_.data(), indices_.size(), &found), c);
        indices_.resize((size_t)found);
    }
    const std::vector<int> &getKeypointsIndices() const { return indices_; }   // (PCL hands out a PointIndices: these are its indices)
  private:
    void check_built() const
    {
        if (border_radius_ > 0.0 || normal_radius_ > 0.0)
            throw Error(RSREG_ERR_INVALID_ARG, "rsreg: ISSKeypoint3D: border estimation (setBorderRadius / setNormalRadius) is not built");
    }
    rsreg_iss_params params_;
    double border_radius_ = 0.0, normal_radius_ = 0.0;
    std::vector<int> indices_;
    typename PointCloud<PointInT>::Ptr input_;
    const DeviceCloud<PointInT> *dinput_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::NormalEstimation<PointInT, PointOutT> on the GPU: with setKSearch (3 .. 64) over an exact k-nearest-neighbour search
// (csrc/normals_kernels.hpp, rsreg_cloud_normals), or with setRadiusSearch over an exact radius search (csrc/radius_kernels.hpp,
// rsreg_cloud_normals_radius; any number of neighbours, fewer than three give NaNs).  As in PCL exactly one of the two is set:
// compute() refuses both and neither before any device call; setKSearch(0) / setRadiusSearch(0) unset them.  PointOutT: 32-byte
// records laid out as pcl::Normal.  The covariance is the one the formula defines, in double about the query point -- PCL's float
// accumulation about the origin is not reproduced (include/rsreg.h states the deviation).  setSearchSurface (a host cloud, or a
// DeviceCloud that must outlive the calls): the neighbours come from that cloud (csrc/surface_kernels.hpp,
// rsreg_cloud_normals_radius_surface), with setRadiusSearch only -- setKSearch with a surface is not built and compute() says so.
// No setIndices.
template <typename PointInT, typename PointOutT = Normal> class NormalEstimation {
    static_assert(sizeof(PointOutT) == 32, "the output records are laid out as pcl::Normal");
  public:
    NormalEstimation() = default;
    explicit NormalEstimation(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointInT>::Ptr &cloud) { input_ = cloud; }
    void setKSearch(int k) { k_ = k; }
    int getKSearch() const { return k_; }
    void setRadiusSearch(double radius) { radius_ = radius; }
    double getRadiusSearch() const { return radius_; }
    void setViewPoint(float vx, float vy, float vz) { vp_[0] = vx; vp_[1] = vy; vp_[2] = vz; }
    void getViewPoint(float &vx, float &vy, float &vz) const { vx = vp_[0]; vy = vp_[1]; vz = vp_[2]; }
    void setSearchSurface(const typename PointCloud<PointInT>::Ptr &surface) { surface_ = surface, dsurface_ = nullptr; }
    void setSearchSurface(const DeviceCloud<PointInT> &surface) { dsurface_ = &surface, surface_.reset(); }
    void compute(PointCloud<PointOutT> &output)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        check_search();
        const std::shared_ptr<Context> ctx = dsurface_ ? dsurface_->context() : ctx_ ? ctx_ : Context::Default();
        DeviceCloud<PointInT> tmp(*input_, ctx);
        DeviceCloud<PointOutT> normals(ctx);
        compute(tmp, normals);
        normals.download(output);
    }
    void compute(const DeviceCloud<PointInT> &input, DeviceCloud<PointOutT> &output)
    {
        check_search();
        rsreg_ctx *c = input.context()->get();
        if (surface_) {
            DeviceCloud<PointInT> tmp(*surface_, input.context());
            check(rsreg_cloud_normals_radius_surface(c, input.handle(), tmp.handle(), radius_, vp_, output.handle()), c);
        } else if (dsurface_)
            check(rsreg_cloud_normals_radius_surface(c, input.handle(), dsurface_->handle(), radius_, vp_, output.handle()), c);
        else if (radius_ != 0.0)
            check(rsreg_cloud_normals_radius(c, input.handle(), radius_, vp_, output.handle()), c);
        else
            check(rsreg_cloud_normals(c, input.handle(), k_, vp_, output.handle()), c);
    }
  private:
    void check_search() const
    {
        if (k_ != 0 && radius_ != 0.0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: both setKSearch and setRadiusSearch are set: set one of them to 0");
        if (k_ == 0 && radius_ == 0.0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: neither setKSearch nor setRadiusSearch is set");
        if ((surface_ || dsurface_) && k_ != 0)
            throw Error(RSREG_ERR_INVALID_ARG, "rsreg: NormalEstimation: setKSearch with setSearchSurface is not built; use setRadiusSearch");
    }
    int k_ = 0;                            // PCL's defaults: no search set (compute() refuses it)
    double radius_ = 0.0;
    float vp_[3] = {0.f, 0.f, 0.f};
    typename PointCloud<PointInT>::Ptr input_, surface_;
    const DeviceCloud<PointInT> *dsurface_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::FPFHSignature33: the 33 floats of a Fast Point Feature Histogram, three blocks of 11 bins
struct FPFHSignature33 {
    float histogram[33];
    static int descriptorSize() { return 33; }
};
static_assert(sizeof(FPFHSignature33) == 132, "pcl::FPFHSignature33 is 33 floats");

// ---- pcl::FPFHEstimation<PointInT, PointNT, PointOutT> on the GPU with setKSearch (2 .. 64) over the exact k-nearest-neighbour
// search (csrc/fpfh_kernels.hpp, rsreg_cloud_fpfh; include/rsreg.h holds the contract).  PointNT: records that begin with
// normal_x, normal_y, normal_z (pcl::Normal); PointOutT: 132-byte records laid out as pcl::FPFHSignature33.  PCL's two quirks are
// kept (the weight is 1 / squared distance, the record's own SPFH does not enter); the pair features are computed in double, not
// in float (the stated deviation).  setRadiusSearch is refused here: FPFHEstimationOMP, below, takes either search and,
// with a radius, a search surface.  No setSearchSurface, no setIndices.
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33> class FPFHEstimation {
    static_assert(sizeof(PointOutT) == 132, "the output records are laid out as pcl::FPFHSignature33");
    static_assert(sizeof(PointNT) >= 12 && sizeof(PointNT) % 4 == 0, "the normals' records begin with three floats");
  public:
    FPFHEstimation() = default;
    explicit FPFHEstimation(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointInT>::Ptr &cloud) { input_ = cloud; }
    void setInputNormals(const typename PointCloud<PointNT>::Ptr &normals) { normals_ = normals; }
    void setKSearch(int k) { k_ = k; }
    int getKSearch() const { return k_; }
    void setRadiusSearch(double radius)
    {
        if (radius != 0.0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: FPFHEstimation::setRadiusSearch is not built; use setKSearch");
    }
    void compute(PointCloud<PointOutT> &output)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        if (!normals_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputNormals not called");
        const std::shared_ptr<Context> ctx = ctx_ ? ctx_ : Context::Default();
        DeviceCloud<PointInT> tmp(*input_, ctx);
        DeviceCloud<PointNT> tmp_normals(*normals_, ctx);
        DeviceCloud<PointOutT> features(ctx);
        compute(tmp, tmp_normals, features);
        features.download(output);
    }
    void compute(const DeviceCloud<PointInT> &input, const DeviceCloud<PointNT> &normals, DeviceCloud<PointOutT> &output)
    {
        if (k_ == 0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setKSearch not called");
        check(rsreg_cloud_fpfh(input.context()->get(), input.handle(), normals.handle(), k_, output.handle()), input.context()->get());
    }
  private:
    int k_ = 0;                            // PCL's default: no search set (compute() refuses it)
    typename PointCloud<PointInT>::Ptr input_;
    typename PointCloud<PointNT>::Ptr normals_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::FPFHEstimationOMP<PointInT, PointNT, PointOutT> on the GPU: with setKSearch (2 .. 64) the bytes of FPFHEstimation
// (rsreg_cloud_fpfh), with setRadiusSearch over the exact radius search (csrc/fpfh_radius_kernels.hpp, rsreg_cloud_fpfh_radius;
// include/rsreg.h holds the contract): a support of fixed metric size, any number of neighbours, the histogram sums in double (the
// stated deviation).  As in PCL exactly one of the two is set: compute() refuses both and neither before any device call;
// setKSearch(0) / setRadiusSearch(0) unset them.  setNumberOfThreads is accepted and ignored.  setSearchSurface (a host cloud, or a
// DeviceCloud that must outlive the calls): the descriptors of the input cloud's records over that cloud, whose normals
// setInputNormals must then hold, as in PCL (csrc/surface_kernels.hpp, rsreg_cloud_fpfh_radius_surface) -- with setRadiusSearch
// only: setKSearch with a surface is not built and compute() says so.  No setIndices.
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33> class FPFHEstimationOMP {
    static_assert(sizeof(PointOutT) == 132, "the output records are laid out as pcl::FPFHSignature33");
    static_assert(sizeof(PointNT) >= 12 && sizeof(PointNT) % 4 == 0, "the normals' records begin with three floats");
  public:
    explicit FPFHEstimationOMP(unsigned int nr_threads = 0) : threads_(nr_threads) {}
    explicit FPFHEstimationOMP(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputCloud(const typename PointCloud<PointInT>::Ptr &cloud) { input_ = cloud; }
    void setInputNormals(const typename PointCloud<PointNT>::Ptr &normals) { normals_ = normals; }
    void setKSearch(int k) { k_ = k; }
    int getKSearch() const { return k_; }
    void setRadiusSearch(double radius) { radius_ = radius; }
    double getRadiusSearch() const { return radius_; }
    void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }
    void setSearchSurface(const typename PointCloud<PointInT>::Ptr &surface) { surface_ = surface, dsurface_ = nullptr; }
    void setSearchSurface(const DeviceCloud<PointInT> &surface) { dsurface_ = &surface, surface_.reset(); }
    void compute(PointCloud<PointOutT> &output)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        if (!normals_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputNormals not called");
        check_search();
        const std::shared_ptr<Context> ctx = dsurface_ ? dsurface_->context() : ctx_ ? ctx_ : Context::Default();
        DeviceCloud<PointInT> tmp(*input_, ctx);
        DeviceCloud<PointNT> tmp_normals(*normals_, ctx);
        DeviceCloud<PointOutT> features(ctx);
        compute(tmp, tmp_normals, features);
        features.download(output);
    }
    // normals: the input's, or with a search surface the surface's
    void compute(const DeviceCloud<PointInT> &input, const DeviceCloud<PointNT> &normals, DeviceCloud<PointOutT> &output)
    {
        check_search();
        rsreg_ctx *c = input.context()->get();
        if (surface_) {
            DeviceCloud<PointInT> tmp(*surface_, input.context());
            check(rsreg_cloud_fpfh_radius_surface(c, input.handle(), tmp.handle(), normals.handle(), radius_, output.handle(), nullptr), c);
        } else if (dsurface_)
            check(rsreg_cloud_fpfh_radius_surface(c, input.handle(), dsurface_->handle(), normals.handle(), radius_, output.handle(), nullptr), c);
        else if (radius_ != 0.0)
            check(rsreg_cloud_fpfh_radius(c, input.handle(), normals.handle(), radius_, output.handle()), c);
        else
            check(rsreg_cloud_fpfh(c, input.handle(), normals.handle(), k_, output.handle()), c);
    }
  private:
    void check_search() const
    {
        if (k_ != 0 && radius_ != 0.0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: both setKSearch and setRadiusSearch are set: set one of them to 0");
        if (k_ == 0 && radius_ == 0.0) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: neither setKSearch nor setRadiusSearch is set");
        if ((surface_ || dsurface_) && k_ != 0)
            throw Error(RSREG_ERR_INVALID_ARG, "rsreg: FPFHEstimationOMP: setKSearch with setSearchSurface is not built; use setRadiusSearch");
    }
    int k_ = 0;                            // PCL's defaults: no search set (compute() refuses it)
    double radius_ = 0.0;
    unsigned int threads_ = 0;
    typename PointCloud<PointInT>::Ptr input_, surface_;
    const DeviceCloud<PointInT> *dsurface_ = nullptr;
    typename PointCloud<PointNT>::Ptr normals_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::Correspondence / pcl::Correspondences: a source row, its match in the target and their SQUARED distance
struct Correspondence {
    int index_query = 0;
    int index_match = -1;
    float distance = std::numeric_limits<float>::max();
    Correspondence() = default;
    Correspondence(int query, int match, float d) : index_query(query), index_match(match), distance(d) {}
};
static_assert(sizeof(Correspondence) == 12 && sizeof(Correspondence) == sizeof(rsreg_correspondence), "pcl::Correspondence is 12 bytes");
using Correspondences = std::vector<Correspondence>;

namespace registration {

// ---- pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> on the GPU: every valid source descriptor's
// nearest valid target descriptor by an exact brute-force search in the 33-dimensional space (csrc/feature_kernels.hpp,
// rsreg_cloud_feature_correspondences; include/rsreg.h holds the contract).  Records that start with 33 floats; a match AT
// max_distance is kept; the list is ordered by index_query.  Host clouds are uploaded into temporaries; the overloads that take
// DeviceClouds leave everything but the list in HBM.  No setIndices, no rejectors.
template <typename PointSource = FPFHSignature33, typename PointTarget = FPFHSignature33> class CorrespondenceEstimation {
    static_assert(sizeof(PointSource) >= 132 && sizeof(PointSource) % 4 == 0 && sizeof(PointTarget) >= 132 && sizeof(PointTarget) % 4 == 0,
                  "descriptor records start with 33 floats");
  public:
    CorrespondenceEstimation() = default;
    explicit CorrespondenceEstimation(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void setInputSource(const typename PointCloud<PointSource>::Ptr &cloud) { source_ = cloud, dsource_ = nullptr; }
    void setInputTarget(const typename PointCloud<PointTarget>::Ptr &cloud) { target_ = cloud, dtarget_ = nullptr; }
    // engine extra: descriptors that are in HBM already (what FPFHEstimation::compute left there); the clouds must outlive the calls
    void setInputSource(const DeviceCloud<PointSource> &cloud) { dsource_ = &cloud, source_.reset(); }
    void setInputTarget(const DeviceCloud<PointTarget> &cloud) { dtarget_ = &cloud, target_.reset(); }
    void determineCorrespondences(Correspondences &out, double max_distance = std::numeric_limits<double>::max()) { run(out, max_distance, 0); }
    void determineReciprocalCorrespondences(Correspondences &out, double max_distance = std::numeric_limits<double>::max()) { run(out, max_distance, 1); }
  private:
    void run(Correspondences &out, double max_distance, int reciprocal)
    {
        if (!source_ && !dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource not called");
        if (!target_ && !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputTarget not called");
        const std::shared_ptr<Context> ctx = dsource_ ? dsource_->context() : dtarget_ ? dtarget_->context() : ctx_ ? ctx_ : Context::Default();
        std::unique_ptr<DeviceCloud<PointSource>> tmp_source;
        std::unique_ptr<DeviceCloud<PointTarget>> tmp_target;
        if (!dsource_) tmp_source.reset(new DeviceCloud<PointSource>(*source_, ctx));
        if (!dtarget_) tmp_target.reset(new DeviceCloud<PointTarget>(*target_, ctx));
        const DeviceCloud<PointSource> &s = dsource_ ? *dsource_ : *tmp_source;
        const DeviceCloud<PointTarget> &t = dtarget_ ? *dtarget_ : *tmp_target;
        size_t n = 0, found = 0;
        check(rsreg_cloud_info(s.handle(), &n, nullptr, nullptr, nullptr, nullptr), ctx->get());
        out.resize(n);
        check(rsreg_cloud_feature_correspondences(ctx->get(), s.handle(), t.handle(), max_distance, reciprocal,
                                                  reinterpret_cast<rsreg_correspondence *>(out.data()), n, &found), ctx->get());
        out.resize(found);
    }
    typename PointCloud<PointSource>::Ptr source_;
    typename PointCloud<PointTarget>::Ptr target_;
    const DeviceCloud<PointSource> *dsource_ = nullptr;
    const DeviceCloud<PointTarget> *dtarget_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// a host cloud or a cloud in HBM as the DeviceCloud a call takes: host clouds are uploaded into a temporary that lives as long as this
template <typename PointT> struct DeviceInput {
    DeviceInput(const typename PointCloud<PointT>::Ptr &host, const DeviceCloud<PointT> *dev, const std::shared_ptr<Context> &ctx)
    {
        if (!dev) tmp_.reset(new DeviceCloud<PointT>(*host, ctx));
        cloud_ = dev ? dev : tmp_.get();
    }
    rsreg_cloud *handle() const { return cloud_->handle(); }
  private:
    std::unique_ptr<DeviceCloud<PointT>> tmp_;
    const DeviceCloud<PointT> *cloud_ = nullptr;
};

// ---- pcl::registration::CorrespondenceRejectorSampleConsensus<PointT> on the GPU: RANSAC over a correspondence list, thousands of
// hypotheses each scored against every pair (csrc/sac_kernels.hpp, rsreg_cloud_sac_correspondences; include/rsreg.h holds the
// contract and the stated deviations from PCL: the sampler, the stopping rule's off-by-one, the refit).  setRefineModel(true) is ONE
// refit round over the inliers, not PCL's refineModel.  Engine extras: setSeed, setProbability, setMinSampleDistance, getResult.
template <typename PointT> class CorrespondenceRejectorSampleConsensus {
    static_assert(sizeof(PointT) >= 12 && sizeof(PointT) % 4 == 0, "records start with x, y, z floats");
  public:
    CorrespondenceRejectorSampleConsensus() { rsreg_sac_params_default(&prm_); std::memset(&res_, 0, sizeof res_); }
    explicit CorrespondenceRejectorSampleConsensus(std::shared_ptr<Context> ctx) : CorrespondenceRejectorSampleConsensus() { ctx_ = std::move(ctx); }
    void setInputSource(const typename PointCloud<PointT>::Ptr &cloud) { source_ = cloud, dsource_ = nullptr; }
    void setInputTarget(const typename PointCloud<PointT>::Ptr &cloud) { target_ = cloud, dtarget_ = nullptr; }
    void setInputSource(const DeviceCloud<PointT> &cloud) { dsource_ = &cloud, source_.reset(); }   // (the clouds must outlive the calls)
    void setInputTarget(const DeviceCloud<PointT> &cloud) { dtarget_ = &cloud, target_.reset(); }
    void setInlierThreshold(double threshold) { prm_.inlier_threshold = threshold; }
    double getInlierThreshold() const { return prm_.inlier_threshold; }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    int getMaximumIterations() const { return prm_.max_iterations; }
    void setRefineModel(bool on) { prm_.refit_rounds = on ? 1 : 0; }
    void setSeed(uint64_t seed) { prm_.seed = seed; }
    void setProbability(double p) { prm_.probability = p; }
    void setMinSampleDistance(double d) { prm_.min_sample_distance = d; }
    void setInputCorrespondences(const std::shared_ptr<const Correspondences> &corr) { input_ = corr; }
    void getCorrespondences(Correspondences &out)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCorrespondences not called");
        getRemainingCorrespondences(*input_, out);
    }
    void getRemainingCorrespondences(const Correspondences &in, Correspondences &out)
    {
        if (!source_ && !dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource not called");
        if (!target_ && !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputTarget not called");
        const std::shared_ptr<Context> ctx = dsource_ ? dsource_->context() : dtarget_ ? dtarget_->context() : ctx_ ? ctx_ : Context::Default();
        const DeviceInput<PointT> s(source_, dsource_, ctx), t(target_, dtarget_, ctx);
        Correspondences kept(in.size());
        size_t found = 0;
        check(rsreg_cloud_sac_correspondences(ctx->get(), s.handle(), t.handle(), reinterpret_cast<const rsreg_correspondence *>(in.data()), in.size(), &prm_,
                                              reinterpret_cast<rsreg_correspondence *>(kept.data()), kept.size(), &found, &res_), ctx->get());
        kept.resize(found);
        out.swap(kept);
    }
    Matrix4f getBestTransformation() const
    {
        Matrix4f T = Matrix4f::Identity();
        if (res_.found) std::memcpy(T.data(), res_.transform, sizeof res_.transform);
        return T;
    }
    const rsreg_sac_result &getResult() const { return res_; }
  private:
    rsreg_sac_params prm_;
    rsreg_sac_result res_;
    std::shared_ptr<const Correspondences> input_;
    typename PointCloud<PointT>::Ptr source_, target_;
    const DeviceCloud<PointT> *dsource_ = nullptr, *dtarget_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::registration::TransformationEstimationSVD<PointSource, PointTarget>::estimateRigidTransformation with a
// correspondence list (rsreg_cloud_estimate_rigid_svd): the fit over the finite pairs, summed in double in a fixed order on the GPU
template <typename PointSource, typename PointTarget = PointSource> class TransformationEstimationSVD {
  public:
    TransformationEstimationSVD() = default;
    explicit TransformationEstimationSVD(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    void estimateRigidTransformation(const PointCloud<PointSource> &source, const PointCloud<PointTarget> &target, const Correspondences &corr, Matrix4f &T) const
    {
        const std::shared_ptr<Context> ctx = ctx_ ? ctx_ : Context::Default();
        const DeviceCloud<PointSource> s(source, ctx);
        const DeviceCloud<PointTarget> t(target, ctx);
        estimateRigidTransformation(s, t, corr, T);
    }
    void estimateRigidTransformation(const DeviceCloud<PointSource> &source, const DeviceCloud<PointTarget> &target, const Correspondences &corr, Matrix4f &T) const
    {
        check(rsreg_cloud_estimate_rigid_svd(source.context()->get(), source.handle(), target.handle(), reinterpret_cast<const rsreg_correspondence *>(corr.data()),
                                             corr.size(), T.data(), nullptr), source.context()->get());
    }
  private:
    std::shared_ptr<Context> ctx_;
};

}  // namespace registration

// ---- pcl::IntegralImageNormalEstimation<PointInT, PointOutT> for organized clouds (csrc/iinormals_kernels.hpp,
// rsreg_cloud_integral_normals), with the calls of src/edge_extractor.hpp:9-15.  AVERAGE_3D_GRADIENT, the IGNORE border policy
// and no depth-dependent smoothing are what is implemented: compute() refuses anything else.  The window sums are the double
// sums of the window's elements, not differences of PCL's table (include/rsreg.h states the deviation).
template <typename PointInT, typename PointOutT = Normal> class IntegralImageNormalEstimation {
    static_assert(sizeof(PointOutT) == 32, "the output records are laid out as pcl::Normal");
  public:
    enum NormalEstimationMethod { COVARIANCE_MATRIX = 0, AVERAGE_3D_GRADIENT = 1, AVERAGE_DEPTH_CHANGE = 2, SIMPLE_3D_GRADIENT = 3 };
    enum BorderPolicy { BORDER_POLICY_IGNORE = 0, BORDER_POLICY_MIRROR = 1 };
    IntegralImageNormalEstimation() { rsreg_iin_params_default(&prm_); }
    explicit IntegralImageNormalEstimation(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { rsreg_iin_params_default(&prm_); }
    void setInputCloud(const typename PointCloud<PointInT>::Ptr &cloud) { input_ = cloud; }
    void setNormalEstimationMethod(NormalEstimationMethod method) { prm_.method = (int)method; }
    void setMaxDepthChangeFactor(float factor) { prm_.max_depth_change_factor = factor; }
    void setNormalSmoothingSize(float size) { prm_.normal_smoothing_size = size; }
    void setDepthDependentSmoothing(bool on) { prm_.depth_dependent_smoothing = on ? 1 : 0; }
    void setBorderPolicy(BorderPolicy policy) { prm_.border_policy = (int)policy; }
    void setViewPoint(float vx, float vy, float vz) { prm_.viewpoint[0] = vx; prm_.viewpoint[1] = vy; prm_.viewpoint[2] = vz; }
    void getViewPoint(float &vx, float &vy, float &vz) const { vx = prm_.viewpoint[0]; vy = prm_.viewpoint[1]; vz = prm_.viewpoint[2]; }
    void compute(PointCloud<PointOutT> &output)
    {
        if (!input_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputCloud not called");
        const std::shared_ptr<Context> ctx = ctx_ ? ctx_ : Context::Default();
        DeviceCloud<PointInT> tmp(*input_, ctx);
        DeviceCloud<PointOutT> normals(ctx);
        compute(tmp, normals);
        normals.download(output);
    }
    void compute(const DeviceCloud<PointInT> &input, DeviceCloud<PointOutT> &output)
    {
        check(rsreg_cloud_integral_normals(input.context()->get(), input.handle(), &prm_, output.handle(), nullptr), input.context()->get());
    }
  private:
    rsreg_iin_params prm_;
    typename PointCloud<PointInT>::Ptr input_;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::transformPointCloud(in, out, Matrix4f); in and out may be the same object
template <typename PointT>
void transformPointCloud(const PointCloud<PointT> &in, PointCloud<PointT> &out, const Matrix4f &T,
                         const std::shared_ptr<Context> &ctx = Context::Default())
{
    PointVector<PointT> pts = uninitialized_points<PointT>(in.size());
    check(rsreg_transform_cloud(ctx->get(), in.points.data(), pts.data(), in.size(), sizeof(PointT), in.is_dense, T.data()),
          ctx->get());
    const uint32_t w = in.width, h = in.height;
    const bool dense = in.is_dense;
    out.points = std::move(pts);
    out.width = w;
    out.height = h;
    out.is_dense = dense;
}

template <typename PointT> void transformPointCloud(const DeviceCloud<PointT> &in, DeviceCloud<PointT> &out, const Matrix4f &T)
{
    check(rsreg_cloud_transform(in.context()->get(), in.handle(), T.data(), out.handle()), in.context()->get());
}

// ---- pcl::SampleConsensusPrerejective<PointSource, PointTarget, FeatureT> on the GPU: poses from three source records and a random
// one of each one's k nearest descriptors (setCorrespondenceRandomness), pre-rejected on their edge lengths, the survivors scored
// against the whole target cloud by an exact nearest-point search (csrc/prerej_kernels.hpp, rsreg_cloud_prerejective; include/rsreg.h
// holds the contract and the stated deviations from PCL: the sampler, the double error, three samples and nothing else).  align()
// makes two calls, rsreg_cloud_feature_knn and rsreg_cloud_prerejective, and writes the source moved by the final transformation.
// Engine extras: setSeed, setSelectByInliers (the winner by support first, not PCL's lowest error), getResult, the device overloads.
template <typename PointSource, typename PointTarget = PointSource, typename FeatureT = FPFHSignature33> class SampleConsensusPrerejective {
    static_assert(sizeof(PointSource) >= 12 && sizeof(PointSource) % 4 == 0 && sizeof(PointTarget) >= 12 && sizeof(PointTarget) % 4 == 0,
                  "records start with x, y, z floats");
    static_assert(sizeof(FeatureT) >= 132 && sizeof(FeatureT) % 4 == 0, "descriptor records start with 33 floats");
  public:
    SampleConsensusPrerejective() { rsreg_prerej_params_default(&prm_); reset(); }
    explicit SampleConsensusPrerejective(std::shared_ptr<Context> ctx) : SampleConsensusPrerejective() { ctx_ = std::move(ctx); }
    void setInputSource(const typename PointCloud<PointSource>::Ptr &cloud) { source_ = cloud, dsource_ = nullptr; }
    void setInputTarget(const typename PointCloud<PointTarget>::Ptr &cloud) { target_ = cloud, dtarget_ = nullptr; }
    void setSourceFeatures(const typename PointCloud<FeatureT>::Ptr &features) { sfeat_ = features, dsfeat_ = nullptr; }
    void setTargetFeatures(const typename PointCloud<FeatureT>::Ptr &features) { tfeat_ = features, dtfeat_ = nullptr; }
    void setInputSource(const DeviceCloud<PointSource> &cloud) { dsource_ = &cloud, source_.reset(); }   // (the clouds must outlive the calls)
    void setInputTarget(const DeviceCloud<PointTarget> &cloud) { dtarget_ = &cloud, target_.reset(); }
    void setSourceFeatures(const DeviceCloud<FeatureT> &features) { dsfeat_ = &features, sfeat_.reset(); }
    void setTargetFeatures(const DeviceCloud<FeatureT> &features) { dtfeat_ = &features, tfeat_.reset(); }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    int getMaximumIterations() const { return prm_.max_iterations; }
    void setNumberOfSamples(int n)
    {
        if (n != 3) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: SampleConsensusPrerejective: only three samples are built");
    }
    int getNumberOfSamples() const { return 3; }
    void setCorrespondenceRandomness(int k) { k_ = k; }
    int getCorrespondenceRandomness() const { return k_; }
    void setSimilarityThreshold(float t) { prm_.similarity_threshold = t; }
    float getSimilarityThreshold() const { return prm_.similarity_threshold; }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    double getMaxCorrespondenceDistance() const { return prm_.max_correspondence_distance; }
    void setInlierFraction(float f) { prm_.inlier_fraction = f; }
    float getInlierFraction() const { return (float)prm_.inlier_fraction; }
    void setSeed(uint64_t seed) { prm_.seed = seed; }
    void setSelectByInliers(bool on) { prm_.select_by_inliers = on ? 1 : 0; }
    void align(PointCloud<PointSource> &output)
    {
        const std::shared_ptr<Context> ctx = context();
        run(ctx);
        if (source_) {
            transformPointCloud(*source_, output, getFinalTransformation(), ctx);
        } else {
            DeviceCloud<PointSource> moved(ctx);
            transformPointCloud(*dsource_, moved, getFinalTransformation());
            moved.download(output);
        }
    }
    void align(DeviceCloud<PointSource> &output)
    {
        if (!dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource (device cloud) not called");
        run(context());
        transformPointCloud(*dsource_, output, getFinalTransformation());
    }
    bool hasConverged() const { return res_.found != 0; }
    Matrix4f getFinalTransformation() const
    {
        Matrix4f T = Matrix4f::Identity();
        if (res_.found) std::memcpy(T.data(), res_.transform, sizeof res_.transform);
        return T;
    }
    const std::vector<int> &getInliers() const { return inliers_; }
    double getFitnessScore() const { return res_.fitness; }   // the winner's error: the sum of its inliers' squared distances / their number
    const rsreg_prerej_result &getResult() const { return res_; }
  private:
    void reset()
    {
        std::memset(&res_, 0, sizeof res_);
        res_.best_hypothesis = -1;
        inliers_.clear();
    }
    std::shared_ptr<Context> context() const
    {
        return dsource_ ? dsource_->context() : dtarget_ ? dtarget_->context() : dsfeat_ ? dsfeat_->context() : dtfeat_ ? dtfeat_->context()
             : ctx_ ? ctx_ : Context::Default();
    }
    void run(const std::shared_ptr<Context> &ctx)
    {
        if (!source_ && !dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource not called");
        if (!target_ && !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputTarget not called");
        if (!sfeat_ && !dsfeat_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setSourceFeatures not called");
        if (!tfeat_ && !dtfeat_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setTargetFeatures not called");
        reset();
        const registration::DeviceInput<PointSource> s(source_, dsource_, ctx);
        const registration::DeviceInput<PointTarget> t(target_, dtarget_, ctx);
        const registration::DeviceInput<FeatureT> fs(sfeat_, dsfeat_, ctx), ft(tfeat_, dtfeat_, ctx);
        size_t n = 0, nf = 0, found = 0;
        check(rsreg_cloud_info(s.handle(), &n, nullptr, nullptr, nullptr, nullptr), ctx->get());
        check(rsreg_cloud_info(fs.handle(), &nf, nullptr, nullptr, nullptr, nullptr), ctx->get());
        if (n != nf) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: the source and its features differ in size");
        if (k_ < 1 || k_ > 16) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setCorrespondenceRandomness needs 1 .. 16");
        std::vector<int32_t> nbr(n * (size_t)k_, -1);
        check(rsreg_cloud_feature_knn(ctx->get(), fs.handle(), ft.handle(), k_, nbr.data(), nullptr), ctx->get());
        std::vector<int> in(n);
        check(rsreg_cloud_prerejective(ctx->get(), s.handle(), t.handle(), nbr.data(), k_, &prm_, in.data(), in.size(), &found, &res_), ctx->get());
        in.resize(found);
        inliers_.swap(in);
    }
    rsreg_prerej_params prm_;
    rsreg_prerej_result res_;
    int k_ = 2;                            // PCL's default
    std::vector<int> inliers_;
    typename PointCloud<PointSource>::Ptr source_;
    typename PointCloud<PointTarget>::Ptr target_;
    typename PointCloud<FeatureT>::Ptr sfeat_, tfeat_;
    const DeviceCloud<PointSource> *dsource_ = nullptr;
    const DeviceCloud<PointTarget> *dtarget_ = nullptr;
    const DeviceCloud<FeatureT> *dsfeat_ = nullptr, *dtfeat_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- pcl::SampleConsensusInitialAlignment<PointSource, PointTarget, FeatureT> on the GPU: poses from nr_samples source records that
// keep a minimum distance from one another and a random one of each one's k nearest descriptors; none is thrown away, every one is
// scored over every source record by a bounded penalty of its exact nearest-point distance (csrc/scia_kernels.hpp,
// rsreg_cloud_initial_alignment; include/rsreg.h holds the contract and the stated deviations from PCL: the sampler, the double sum,
// no persistent relaxation of the minimum distance, a guess given as an argument and not told from the identity).  As in PCL,
// setMaxCorrespondenceDistance is compared with the SQUARED distance.  align() makes two calls, rsreg_cloud_feature_knn and
// rsreg_cloud_initial_alignment, and writes the source moved by the final transformation.
// Engine extras: setSeed, getResult, the device overloads.
template <typename PointSource, typename PointTarget = PointSource, typename FeatureT = FPFHSignature33> class SampleConsensusInitialAlignment {
    static_assert(sizeof(PointSource) >= 12 && sizeof(PointSource) % 4 == 0 && sizeof(PointTarget) >= 12 && sizeof(PointTarget) % 4 == 0,
                  "records start with x, y, z floats");
    static_assert(sizeof(FeatureT) >= 132 && sizeof(FeatureT) % 4 == 0, "descriptor records start with 33 floats");
  public:
    enum ErrorFunction { TRUNCATED_ERROR = RSREG_SCIA_TRUNCATED, HUBER_PENALTY = RSREG_SCIA_HUBER };
    SampleConsensusInitialAlignment() { rsreg_scia_params_default(&prm_); reset(); }
    explicit SampleConsensusInitialAlignment(std::shared_ptr<Context> ctx) : SampleConsensusInitialAlignment() { ctx_ = std::move(ctx); }
    void setInputSource(const typename PointCloud<PointSource>::Ptr &cloud) { source_ = cloud, dsource_ = nullptr; }
    void setInputTarget(const typename PointCloud<PointTarget>::Ptr &cloud) { target_ = cloud, dtarget_ = nullptr; }
    void setSourceFeatures(const typename PointCloud<FeatureT>::Ptr &features) { sfeat_ = features, dsfeat_ = nullptr; }
    void setTargetFeatures(const typename PointCloud<FeatureT>::Ptr &features) { tfeat_ = features, dtfeat_ = nullptr; }
    void setInputSource(const DeviceCloud<PointSource> &cloud) { dsource_ = &cloud, source_.reset(); }   // (the clouds must outlive the calls)
    void setInputTarget(const DeviceCloud<PointTarget> &cloud) { dtarget_ = &cloud, target_.reset(); }
    void setSourceFeatures(const DeviceCloud<FeatureT> &features) { dsfeat_ = &features, sfeat_.reset(); }
    void setTargetFeatures(const DeviceCloud<FeatureT> &features) { dtfeat_ = &features, tfeat_.reset(); }
    void setMaximumIterations(int n) { prm_.max_iterations = n; }
    int getMaximumIterations() const { return prm_.max_iterations; }
    void setMinSampleDistance(float d) { prm_.min_sample_distance = d; }
    float getMinSampleDistance() const { return (float)prm_.min_sample_distance; }
    void setNumberOfSamples(int n) { prm_.nr_samples = n; }
    int getNumberOfSamples() const { return prm_.nr_samples; }
    void setCorrespondenceRandomness(int k) { k_ = k; }
    int getCorrespondenceRandomness() const { return k_; }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    double getMaxCorrespondenceDistance() const { return prm_.max_correspondence_distance; }
    void setErrorFunction(ErrorFunction f) { prm_.error_function = (int32_t)f; }
    ErrorFunction getErrorFunction() const { return (ErrorFunction)prm_.error_function; }
    void setSeed(uint64_t seed) { prm_.seed = seed; }
    void align(PointCloud<PointSource> &output) { align_host(output, nullptr); }
    void align(PointCloud<PointSource> &output, const Matrix4f &guess) { align_host(output, guess.data()); }
    void align(DeviceCloud<PointSource> &output) { align_device(output, nullptr); }
    void align(DeviceCloud<PointSource> &output, const Matrix4f &guess) { align_device(output, guess.data()); }
    bool hasConverged() const { return res_.found != 0; }
    Matrix4f getFinalTransformation() const
    {
        Matrix4f T;
        std::memcpy(T.data(), res_.transform, sizeof res_.transform);
        return T;
    }
    double getFitnessScore() const { return res_.error; }   // the winner's error (the guess's when nothing beat it)
    const rsreg_scia_result &getResult() const { return res_; }
  private:
    void reset()
    {
        std::memset(&res_, 0, sizeof res_);
        const Matrix4f eye = Matrix4f::Identity();
        std::memcpy(res_.transform, eye.data(), sizeof res_.transform);
        res_.best_hypothesis = -1;
        for (int i = 0; i < 8; ++i) res_.sample[i] = res_.match[i] = -1;
        res_.error = std::numeric_limits<double>::infinity();
    }
    std::shared_ptr<Context> context() const
    {
        return dsource_ ? dsource_->context() : dtarget_ ? dtarget_->context() : dsfeat_ ? dsfeat_->context() : dtfeat_ ? dtfeat_->context()
             : ctx_ ? ctx_ : Context::Default();
    }
    void align_host(PointCloud<PointSource> &output, const float *guess)
    {
        const std::shared_ptr<Context> ctx = context();
        run(ctx, guess);
        if (source_) {
            transformPointCloud(*source_, output, getFinalTransformation(), ctx);
        } else {
            DeviceCloud<PointSource> moved(ctx);
            transformPointCloud(*dsource_, moved, getFinalTransformation());
            moved.download(output);
        }
    }
    void align_device(DeviceCloud<PointSource> &output, const float *guess)
    {
        if (!dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource (device cloud) not called");
        run(context(), guess);
        transformPointCloud(*dsource_, output, getFinalTransformation());
    }
    void run(const std::shared_ptr<Context> &ctx, const float *guess)
    {
        if (!source_ && !dsource_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputSource not called");
        if (!target_ && !dtarget_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setInputTarget not called");
        if (!sfeat_ && !dsfeat_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setSourceFeatures not called");
        if (!tfeat_ && !dtfeat_) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setTargetFeatures not called");
        reset();
        const registration::DeviceInput<PointSource> s(source_, dsource_, ctx);
        const registration::DeviceInput<PointTarget> t(target_, dtarget_, ctx);
        const registration::DeviceInput<FeatureT> fs(sfeat_, dsfeat_, ctx), ft(tfeat_, dtfeat_, ctx);
        size_t n = 0, nf = 0;
        check(rsreg_cloud_info(s.handle(), &n, nullptr, nullptr, nullptr, nullptr), ctx->get());
        check(rsreg_cloud_info(fs.handle(), &nf, nullptr, nullptr, nullptr, nullptr), ctx->get());
        if (n != nf) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: the source and its features differ in size");
        if (k_ < 1 || k_ > 16) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: setCorrespondenceRandomness needs 1 .. 16");
        std::vector<int32_t> nbr(n * (size_t)k_, -1);
        check(rsreg_cloud_feature_knn(ctx->get(), fs.handle(), ft.handle(), k_, nbr.data(), nullptr), ctx->get());
        check(rsreg_cloud_initial_alignment(ctx->get(), s.handle(), t.handle(), nbr.data(), k_, &prm_, guess, nullptr, &res_), ctx->get());
    }
    rsreg_scia_params prm_;
    rsreg_scia_result res_;
    int k_ = 10;                           // PCL's default
    typename PointCloud<PointSource>::Ptr source_;
    typename PointCloud<PointTarget>::Ptr target_;
    typename PointCloud<FeatureT>::Ptr sfeat_, tfeat_;
    const DeviceCloud<PointSource> *dsource_ = nullptr;
    const DeviceCloud<PointTarget> *dtarget_ = nullptr;
    const DeviceCloud<FeatureT> *dsfeat_ = nullptr, *dtfeat_ = nullptr;
    std::shared_ptr<Context> ctx_;
};

// ---- extract_edge_features (src/edge_extractor.hpp:7-39): the RGB-Canny edge points of an organized cloud
inline std::shared_ptr<PointCloud<PointXYZRGB>> extract_edge_features(const std::shared_ptr<PointCloud<PointXYZRGB>> &cloud,
                                                                      const std::shared_ptr<Context> &ctx = Context::Default())
{
    auto out = std::make_shared<PointCloud<PointXYZRGB>>();
    if ((size_t)cloud->width * cloud->height != cloud->size()) throw Error(RSREG_ERR_INVALID_ARG, "rsreg: edge extraction needs an organized cloud");
    PointVector<PointXYZRGB> pts = uninitialized_points<PointXYZRGB>(cloud->size());
    size_t n = 0;
    check(rsreg_extract_edge_features(ctx->get(), cloud->points.data(), cloud->width, cloud->height, sizeof(PointXYZRGB), pts.data(), nullptr, &n),
          ctx->get());
    pts.resize(n);
    out->points = std::move(pts);
    out->width = (uint32_t)n;
    out->height = 1;
    out->is_dense = cloud->is_dense;
    return out;
}

// the same on a frame that already lies in HBM (out: width = number of edge points, height = 1)
inline void extract_edge_features(const DeviceCloud<PointXYZRGB> &cloud, DeviceCloud<PointXYZRGB> &out)
{
    check(rsreg_cloud_edge_features(cloud.context()->get(), cloud.handle(), out.handle()), cloud.context()->get());
}
// ... queued by a thread of the context on a stream of its own (rsreg_cloud_edge_features_async): returns at once, `out` is
// complete when a call that takes it has waited for it.  `cloud` must stay as it is until then.
inline void extract_edge_features_async(const DeviceCloud<PointXYZRGB> &cloud, DeviceCloud<PointXYZRGB> &out)
{
    check(rsreg_cloud_edge_features_async(cloud.context()->get(), cloud.handle(), out.handle()), cloud.context()->get());
}

// ---- pcl::io: PCD files with FIELDS x y z rgb (ascii, binary, binary_compressed), as the reference reads/writes
// (src/main.cpp:53,81,87)
namespace io {

inline int loadPCDFile(const std::string &path, PointCloud<PointXYZRGB> &cloud)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return -1;
    std::string line, data_mode;
    std::vector<std::string> fields, types;
    std::vector<int> sizes;
    size_t n = 0;
    uint32_t width = 0, height = 1;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string key;
        ss >> key;
        if (key == "FIELDS") { std::string s; while (ss >> s) fields.push_back(s); }
        else if (key == "SIZE") { int s; while (ss >> s) sizes.push_back(s); }
        else if (key == "TYPE") { std::string s; while (ss >> s) types.push_back(s); }
        else if (key == "WIDTH") ss >> width;
        else if (key == "HEIGHT") ss >> height;
        else if (key == "POINTS") ss >> n;
        else if (key == "DATA") { ss >> data_mode; break; }
    }
    if (n == 0) n = (size_t)width * height;
    int ix = -1, iy = -1, iz = -1, ic = -1;
    for (size_t k = 0; k < fields.size(); ++k) {
        if (fields[k] == "x") ix = (int)k;
        else if (fields[k] == "y") iy = (int)k;
        else if (fields[k] == "z") iz = (int)k;
        else if (fields[k] == "rgb" || fields[k] == "rgba") ic = (int)k;
    }
    if (ix < 0 || iy < 0 || iz < 0) return -2;
    // the header is untrusted input: every field needs a SIZE and a TYPE, sizes are positive, and the fields this reader
    // copies four bytes of (x, y, z, the packed colour) are four bytes wide; the body must fit what is left of the file
    if (sizes.size() != fields.size() || types.size() != fields.size()) return -2;
    for (int sz : sizes)
        if (sz <= 0 || sz > 8) return -2;
    if (sizes[ix] != 4 || sizes[iy] != 4 || sizes[iz] != 4 || (ic >= 0 && sizes[ic] != 4)) return -2;
    size_t remaining = 0;
    {
        const std::streampos here = f.tellg();
        f.seekg(0, std::ios::end);
        const std::streampos end = f.tellg();
        f.seekg(here);
        if (here < 0 || end < here) return -4;
        remaining = (size_t)(end - here);
    }
    {
        size_t rec_bytes = 0;
        for (int sz : sizes) rec_bytes += (size_t)sz;
        // ascii needs at least "0 " per field; the binary forms are checked exactly below
        const size_t least = data_mode == "binary" ? rec_bytes : (data_mode == "ascii" ? 2 * fields.size() - 1 : 0);
        if (n > 0 && least > 0 && n > remaining / least + 1) return -4;
        if (n > (size_t)1 << 32) return -4;
    }
    cloud.points.assign(n, PointXYZRGB());
    cloud.width = width;
    cloud.height = height;
    bool dense = true;
    if (data_mode == "ascii") {
        for (size_t i = 0; i < n; ++i) {
            PointXYZRGB &p = cloud.points[i];
            for (size_t k = 0; k < fields.size(); ++k) {
                std::string tok;
                if (!(f >> tok)) return -4;
                if ((int)k == ic) {
                    if (types[k] == "F") { float v = std::stof(tok); std::memcpy(&p.rgba, &v, 4); }
                    else p.rgba = (uint32_t)std::stoul(tok);
                } else {
                    const float v = std::stof(tok);
                    if ((int)k == ix) p.x = v; else if ((int)k == iy) p.y = v; else if ((int)k == iz) p.z = v;
                }
            }
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) dense = false;
        }
    } else if (data_mode == "binary") {
        size_t rec = 0;
        std::vector<size_t> off(fields.size());
        for (size_t k = 0; k < fields.size(); ++k) { off[k] = rec; rec += (size_t)sizes[k]; }
        if (rec * n > remaining) return -4;
        std::vector<char> buf(rec * n);
        f.read(buf.data(), (std::streamsize)buf.size());
        if ((size_t)f.gcount() != buf.size()) return -4;
        for (size_t i = 0; i < n; ++i) {
            PointXYZRGB &p = cloud.points[i];
            const char *r = buf.data() + i * rec;
            std::memcpy(&p.x, r + off[ix], 4);
            std::memcpy(&p.y, r + off[iy], 4);
            std::memcpy(&p.z, r + off[iz], 4);
            if (ic >= 0) std::memcpy(&p.rgba, r + off[ic], 4);
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) dense = false;
        }
    } else if (data_mode == "binary_compressed") {
        // u32 compressed size, u32 uncompressed size, LZF stream of the fields one after the other
        uint32_t csize = 0, usize = 0;
        f.read(reinterpret_cast<char *>(&csize), 4);
        f.read(reinterpret_cast<char *>(&usize), 4);
        size_t rec = 0;
        std::vector<size_t> foff(fields.size());
        for (size_t k = 0; k < fields.size(); ++k) { foff[k] = rec * n; rec += (size_t)sizes[k]; }
        if (!f || (size_t)usize != rec * n || remaining < 8 || (size_t)csize > remaining - 8) return -4;
        std::vector<uint8_t> comp(csize), soa(usize);
        f.read(reinterpret_cast<char *>(comp.data()), (std::streamsize)csize);
        if (!f || (usize && lzf::decode(comp.data(), csize, soa.data(), usize) != usize)) return -4;
        for (size_t i = 0; i < n; ++i) {
            PointXYZRGB &p = cloud.points[i];
            std::memcpy(&p.x, soa.data() + foff[ix] + 4 * i, 4);
            std::memcpy(&p.y, soa.data() + foff[iy] + 4 * i, 4);
            std::memcpy(&p.z, soa.data() + foff[iz] + 4 * i, 4);
            if (ic >= 0) std::memcpy(&p.rgba, soa.data() + foff[ic] + 4 * i, 4);
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) dense = false;
        }
    } else {
        return -3;
    }
    cloud.is_dense = dense;
    return 0;
}

inline int savePCDFileBinary(const std::string &path, const PointCloud<PointXYZRGB> &cloud)
{
    std::ofstream f(path, std::ios::binary);
    if (!f) return -1;
    f << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
      << "WIDTH " << cloud.width << "\nHEIGHT " << cloud.height << "\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << cloud.size()
      << "\nDATA binary\n";
    for (const PointXYZRGB &p : cloud.points) {
        f.write(reinterpret_cast<const char *>(&p.x), 12);
        f.write(reinterpret_cast<const char *>(&p.rgba), 4);
    }
    return f ? 0 : -1;
}

// pcl::io::savePCDFileBinaryCompressed: same header, DATA binary_compressed, LZF over the SoA body
inline int savePCDFileBinaryCompressed(const std::string &path, const PointCloud<PointXYZRGB> &cloud)
{
    std::ofstream f(path, std::ios::binary);
    if (!f) return -1;
    const size_t n = cloud.size();
    std::vector<uint8_t> soa(16 * n);
    for (size_t i = 0; i < n; ++i) {
        const PointXYZRGB &p = cloud.points[i];
        std::memcpy(soa.data() + 4 * i, &p.x, 4);
        std::memcpy(soa.data() + 4 * (n + i), &p.y, 4);
        std::memcpy(soa.data() + 4 * (2 * n + i), &p.z, 4);
        std::memcpy(soa.data() + 4 * (3 * n + i), &p.rgba, 4);
    }
    std::vector<uint8_t> comp(lzf::max_encoded_size(soa.size()));
    const uint32_t usize = (uint32_t)soa.size();
    const uint32_t csize = (uint32_t)lzf::encode(soa.data(), soa.size(), comp.data(), comp.size());
    if (usize && !csize) return -1;
    f << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
      << "WIDTH " << cloud.width << "\nHEIGHT " << cloud.height << "\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << n
      << "\nDATA binary_compressed\n";
    f.write(reinterpret_cast<const char *>(&csize), 4);
    f.write(reinterpret_cast<const char *>(&usize), 4);
    f.write(reinterpret_cast<const char *>(comp.data()), csize);
    return f ? 0 : -1;
}

}  // namespace io
}  // namespace rsreg
