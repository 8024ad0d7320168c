// voxel_host.cpp — pcl::ApproximateVoxelGrid<PointXYZRGB>::filter on the host.
//
// Reference call sites: src/incremental_icp.hpp:54-55 (default 1 m leaf),
// src/icp_edge_based_registration.hpp:47,59-60,75-76, src/ndt_edge_based_registration.hpp:45,
// 57-58,68-69 (1 cm leaf, also in place).  The filter is a sequential stream over the points
// with a 512-slot hash history that flushes on collision: its output
// depends on the input ORDER and may hold several centroids per voxel, so a parallel version
// cannot reproduce it record for record.  It runs on ~30 k-point edge clouds and is O(N);
// it stays on the host for parity (DESIGN.md "what stays on the host").
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/rsreg.h"

namespace {

struct Slot {
    int ix = 0, iy = 0, iz = 0, count = 0;
    float acc[7] = {0, 0, 0, 0, 0, 0, 0};  // x y z rgb-as-float r g b
};

// The cell index of the contract (include/rsreg.h): the integer c, or INT32_MIN when c is a NaN or outside [-2^31, 2^31).  That is
// what x86's conversion instruction delivers, and therefore PCL; written out, because in C++ the plain cast is undefined there.
inline int32_t cell_i32(float c) { return (c >= -2147483648.0f && c < 2147483648.0f) ? static_cast<int32_t>(c) : INT32_MIN; }

void emit(unsigned char *out, size_t &n_out, size_t stride, const Slot &s)
{
    const float n = static_cast<float>(s.count);
    float c[7];
    for (int k = 0; k < 7; ++k) c[k] = s.acc[k] / n;
    unsigned char *rec = out + n_out * stride;  // a default PointXYZRGB: zeros, data[3] = 1
    ++n_out;
    std::memset(rec, 0, stride);
    const float one = 1.0f;
    std::memcpy(rec, c, 12);
    std::memcpy(rec + 12, &one, 4);
    const int rgb = (static_cast<int>(c[4]) << 16) | (static_cast<int>(c[5]) << 8) | static_cast<int>(c[6]);
    std::memcpy(rec + 16, &rgb, 4);
}

}  // namespace

extern "C" int rsreg_approx_voxel_grid(const void *in, size_t n, size_t stride, const float leaf[3], void *out,
                                       size_t *n_out)
{
    if (!leaf || !n_out || (n && (!in || !out)) || stride < 20) return RSREG_ERR_INVALID_ARG;
    if (!(leaf[0] > 0) || !(leaf[1] > 0) || !(leaf[2] > 0)) return RSREG_ERR_INVALID_ARG;
    constexpr int kHist = 512;
    std::vector<Slot> hist(kHist);
    const float inv[3] = {1.0f / leaf[0], 1.0f / leaf[1], 1.0f / leaf[2]};
    // in == out is allowed, and the output can only fall behind the input (a record is emitted
    // after at least one more input record has been read) except in the final flush -- but the
    // slot an emission frees may still be read as input later, so an aliased call works aside
    std::vector<unsigned char> aside;
    unsigned char *result = static_cast<unsigned char *>(out);
    if (in == out) {
        aside.resize(n * stride);
        result = aside.data();
    }
    size_t count = 0;
    const unsigned char *src = static_cast<const unsigned char *>(in);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char *rec = src + i * stride;
        float xyz[3], rgbf;
        unsigned char bgra[4];
        std::memcpy(xyz, rec, 12);
        std::memcpy(&rgbf, rec + 16, 4);
        std::memcpy(bgra, rec + 16, 4);
        if (!std::isfinite(xyz[0]) || !std::isfinite(xyz[1]) || !std::isfinite(xyz[2])) continue;
        const int32_t ix = cell_i32(std::floor(xyz[0] * inv[0]));
        const int32_t iy = cell_i32(std::floor(xyz[1] * inv[1]));
        const int32_t iz = cell_i32(std::floor(xyz[2] * inv[2]));
        const uint32_t h = (static_cast<uint32_t>(ix) * 7171u + static_cast<uint32_t>(iy) * 3079u + static_cast<uint32_t>(iz) * 4231u) & (kHist - 1);
        Slot &s = hist[h];
        if (s.count && (s.ix != ix || s.iy != iy || s.iz != iz)) {
            emit(result, count, stride, s);
            s = Slot();
        }
        s.ix = ix; s.iy = iy; s.iz = iz;
        ++s.count;
        const float add[7] = {xyz[0], xyz[1], xyz[2], rgbf, float(bgra[2]), float(bgra[1]), float(bgra[0])};
        for (int k = 0; k < 7; ++k) s.acc[k] += add[k];
    }
    for (const Slot &s : hist)
        if (s.count) emit(result, count, stride, s);
    if (in == out && count) std::memcpy(out, result, count * stride);
    *n_out = count;
    return RSREG_OK;
}

// ---- pcl::VoxelGrid<PointXYZRGB>::filter on the host: the contract of include/rsreg.h ("pcl::VoxelGrid") restated
// sequentially -- the box of the finite records, a leaf index per record, a stable sort by it, and per leaf float sums in
// ascending input index.  No context; the second implementation the GPU filter (voxel.hip) is compared with.
namespace {

// float -> int32 as the contract defines it: saturating (a leaf coordinate past int32 is outside what PCL defines)
inline int32_t sat_i32(float f)
{
    if (f >= 2147483648.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return static_cast<int32_t>(f);
}

}  // namespace

extern "C" void rsreg_voxel_grid_params_default(rsreg_voxel_grid_params *p)
{
    if (!p) return;
    p->leaf[0] = p->leaf[1] = p->leaf[2] = 0.0f;   // PCL's default: no leaf set, filter() refuses
    p->downsample_all_data = 1;
    p->min_points_per_voxel = 0;
}

extern "C" int rsreg_voxel_grid(const void *in, size_t n, size_t stride, const float leaf[3], int downsample_all_data,
                                uint32_t min_points, void *out, size_t *n_out, rsreg_voxel_grid_info *info)
{
    if (!leaf || !n_out || (n && (!in || !out)) || stride < 20 || (stride & 3)) return RSREG_ERR_INVALID_ARG;
    float inv[3];
    for (int a = 0; a < 3; ++a) {
        if (!(leaf[a] > 0) || !std::isfinite(leaf[a])) return RSREG_ERR_INVALID_ARG;
        inv[a] = 1.0f / leaf[a];
        if (!std::isfinite(inv[a])) return RSREG_ERR_INVALID_ARG;
    }
    rsreg_voxel_grid_info nfo;
    std::memset(&nfo, 0, sizeof nfo);
    *n_out = 0;
    const unsigned char *src = static_cast<const unsigned char *>(in);
    auto xyz_of = [&](size_t i, float p[3]) { std::memcpy(p, src + i * stride, 12); };
    // the box of the finite records
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    std::vector<uint32_t> finite;
    for (size_t i = 0; i < n; ++i) {
        float p[3];
        xyz_of(i, p);
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
        for (int a = 0; a < 3; ++a) {
            if (finite.empty() || p[a] < mn[a]) mn[a] = p[a];
            if (finite.empty() || p[a] > mx[a]) mx[a] = p[a];
        }
        finite.push_back(static_cast<uint32_t>(i));
    }
    nfo.n_finite = finite.size();
    if (finite.empty()) {
        if (info) *info = nfo;
        return RSREG_OK;
    }
    // "leaf size too small": the number of leaves of the box passes int32
    bool overflow = false;
    unsigned long long cells = 1;
    for (int a = 0; a < 3 && !overflow; ++a) {
        const float ext = mx[a] - mn[a];
        const float v = ext * inv[a];
        if (!(v < 2147483648.0f)) { overflow = true; break; }
        cells *= static_cast<unsigned long long>(static_cast<int64_t>(v) + 1);   // (each factor <= 2^31: checked after every step)
        if (cells > static_cast<unsigned long long>(INT32_MAX)) overflow = true;
    }
    if (overflow) {
        if (in != out) std::memmove(out, in, n * stride);
        *n_out = n;
        nfo.overflowed = 1;
        nfo.n_out = n;
        if (info) *info = nfo;
        return RSREG_OK;
    }
    uint32_t mul[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = mn[a] * inv[a], hi = mx[a] * inv[a];
        nfo.min_b[a] = sat_i32(std::floor(lo));
        nfo.max_b[a] = sat_i32(std::floor(hi));
        nfo.div_b[a] = static_cast<int32_t>(static_cast<uint32_t>(nfo.max_b[a]) - static_cast<uint32_t>(nfo.min_b[a]) + 1u);
    }
    mul[0] = 1u;
    mul[1] = static_cast<uint32_t>(nfo.div_b[0]);
    mul[2] = static_cast<uint32_t>(nfo.div_b[0]) * static_cast<uint32_t>(nfo.div_b[1]);
    for (int a = 0; a < 3; ++a) nfo.divb_mul[a] = static_cast<int32_t>(mul[a]);
    // (leaf index, input position), sorted by leaf; the positions of a leaf stay ascending
    std::vector<std::pair<uint32_t, uint32_t>> order(finite.size());
    for (size_t k = 0; k < finite.size(); ++k) {
        float p[3];
        xyz_of(finite[k], p);
        uint32_t idx = 0;
        for (int a = 0; a < 3; ++a) {
            const float s = p[a] * inv[a];
            const float rel = std::floor(s) - static_cast<float>(nfo.min_b[a]);
            idx += static_cast<uint32_t>(sat_i32(rel)) * mul[a];
        }
        order[k] = {idx, finite[k]};
    }
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return x.first < y.first; });
    // the centroids go aside: `out` may be `in`
    std::vector<unsigned char> result;
    size_t count = 0, leaves = 0;
    for (size_t a = 0; a < order.size();) {
        size_t b = a;
        float sum[7] = {0, 0, 0, 0, 0, 0, 0};   // x y z r g b a
        for (; b < order.size() && order[b].first == order[a].first; ++b) {
            const unsigned char *rec = src + static_cast<size_t>(order[b].second) * stride;
            float p[3];
            std::memcpy(p, rec, 12);
            const float add[7] = {p[0], p[1], p[2], float(rec[18]), float(rec[17]), float(rec[16]), float(rec[19])};
            for (int k = 0; k < 7; ++k) sum[k] = sum[k] + add[k];
        }
        ++leaves;
        const size_t pts = b - a;
        a = b;
        if (pts < min_points) continue;
        const float cnt = static_cast<float>(pts);
        result.resize((count + 1) * stride, 0);
        unsigned char *rec = result.data() + count * stride;
        ++count;
        const float c[4] = {sum[0] / cnt, sum[1] / cnt, sum[2] / cnt, 1.0f};
        std::memcpy(rec, c, 16);
        uint32_t rgba = 0xff000000u;   // a default PointXYZRGB
        if (downsample_all_data)
            rgba = (static_cast<uint32_t>(sum[6] / cnt) << 24) | (static_cast<uint32_t>(sum[3] / cnt) << 16) |
                   (static_cast<uint32_t>(sum[4] / cnt) << 8) | static_cast<uint32_t>(sum[5] / cnt);
        std::memcpy(rec + 16, &rgba, 4);
    }
    if (count) std::memcpy(out, result.data(), count * stride);
    *n_out = count;
    nfo.n_leaves = leaves;
    nfo.n_out = count;
    if (info) *info = nfo;
    return RSREG_OK;
}
