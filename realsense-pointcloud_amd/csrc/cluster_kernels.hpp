// cluster_kernels.hpp — pcl::EuclideanClusterExtraction on a cloud resident in HBM (include/rsreg.h: rsreg_cloud_euclidean_clusters,
// rsreg_cloud_cluster_filter): the connected components of the graph the exact radius search defines, as a lock-free union-find fused
// into the walk of radius_kernels.hpp, then the ranking of the components.  Included by filters.hip only.
//
// PCL 1.9.1 segmentation/impl/extract_clusters.hpp, recalled (not available to check against; include/rsreg.h is the contract):
//   for every unprocessed point, ascending: a seed queue grows by radiusSearch(tolerance) of each of its points until it stops;
//   the finished queue is a cluster when min_pts_per_cluster <= its size <= max_pts_per_cluster; its indices are sorted;
//   std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters)   // size descending
// A seed queue is a connected component of "j is within the tolerance of i" (radius_kernels.hpp: float32 d2 < r2, strictly, symmetric),
// and a component does not depend on where its queue started: a set partition, specified to equality.
//
// Nodes are ORIGINAL RECORD INDICES (the tag a point of the index carries in .w).  parent[i] <= i at all times and a hook puts the
// HIGHER root under the LOWER one, so a tree's root is the smallest record index of the tree, and of the component once every edge
// has been linked: the result does not depend on how the races fell.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "radius_kernels.hpp"

namespace rsreg {

constexpr uint32_t kClusterNone = 0xffffffffu;   // the root, rank or label of a record that belongs to no cluster

// ------------------------------------------------------------------------------ union-find (k_cluster_hook only)
// While links run, a parent word is read and written by waves on every XCD: reads bypass the non-coherent L2 of the reader's XCD
// (a plain load may be served stale from it), writes are integer atomics.  Every write LOWERS a word (the CAS hooks a root under a
// smaller root, the halving is an atomicMin with an ancestor), so a stale value is an ancestor the record once had: following it
// costs steps, never the answer, and the CAS -- which compares with the word itself -- decides whether a hook took place.
__device__ __forceinline__ uint32_t cluster_parent(const uint32_t *parent, uint32_t i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as of some moment during the call, with path halving: every node on the way is pointed at its grandparent.
// Ends: x strictly decreases.
__device__ __forceinline__ uint32_t cluster_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = cluster_parent(parent, x);
    while (p != x) {
        const uint32_t g = cluster_parent(parent, p);
        if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// joins the trees of a and b; returns the root both had when it was done.  A failed CAS returns what `hi` hangs under by now, below
// hi: every retry works on a strictly smaller pair, and nothing here waits for what another wave does.
__device__ __forceinline__ uint32_t cluster_link(uint32_t *parent, uint32_t a, uint32_t b)
{
    uint32_t ra = cluster_find(parent, a), rb = cluster_find(parent, b);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return lo;
        ra = cluster_find(parent, was);
        rb = cluster_find(parent, lo);
    }
    return ra;
}

// a lane's share of a query's edges: the hits with a LOWER record index (each edge once, from its higher end; the record itself
// and nothing else is skipped: an exact copy has another index).  `root`: the lane's latest knowledge of the query's root, an
// ancestor of the query at all times.  The hit's way up (halved as in cluster_find) ends where it MEETS that record -- the hit is in
// the query's tree, and the word of `root` itself, the one word every wave of a large component would read, is not loaded -- or at
// a root that is another record: only then the two trees are linked.
struct ClusterLink {
    uint32_t *parent;
    uint32_t q, root;
    __device__ __forceinline__ void operator()(const float4 &t)
    {
        uint32_t x = __float_as_uint(t.w);
        if (x >= q) return;
        uint32_t p = cluster_parent(parent, x);
        while (p != root && p != x) {
            const uint32_t g = cluster_parent(parent, p);
            if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = p;
            p = g;
        }
        if (p != root) root = cluster_link(parent, root, x);
    }
};

// parent[i] = i: every record a tree of its own (the non-finite ones stay that way; k_cluster_flatten gives them no root)
__global__ __launch_bounds__(kBlock) void k_cluster_init(uint32_t n, uint32_t *parent, uint32_t *size)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    size[i] = 0u;
}

// One workgroup of ONE wave per query, queries in cell order (the grid-stride loop of k_radius_count): the walk, every hit below the
// query linked to it.
__global__ __launch_bounds__(kKnnWave) void k_cluster_hook(PointGridDev g, RadiusQuery rq, uint32_t *parent)
{
    const int lane = (int)threadIdx.x;
    for (uint32_t j = blockIdx.x; j < g.n; j += gridDim.x) {
        const float4 q = g.pts[j];
        const uint32_t qi = __float_as_uint(q.w);
        ClusterLink f{parent, qi, cluster_parent(parent, qi)};
        radius_walk(g, q, rq, lane, f);
    }
}

// A launch of its own: the kernel boundary makes every hook visible, and nothing writes a parent word here, so plain loads do.
// root[i] = the smallest record of i's component, size[root] = the component's records; kClusterNone for a non-finite record.
__global__ __launch_bounds__(kBlock) void k_cluster_flatten(const char *rec, size_t stride, uint32_t n, const uint32_t *parent, uint32_t *root, uint32_t *size)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t x = kClusterNone;
    if (i < n) {
        const float *p = rec_xyz(rec, stride, i);
        if (finite3(p[0], p[1], p[2])) {
            x = i;
            for (uint32_t up = parent[x]; up != x; up = parent[x]) x = up;
        }
        root[i] = x;
    }
    // one add per (wave, root), not per record: the records of a large component would queue up at one word
    unsigned long long todo = __ballot(x != kClusterNone);
    while (todo) {
        const uint32_t r = __shfl(x, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(x == r);
        if (x == r && (same & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0ull) atomicAdd(size + r, (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// ------------------------------------------------------------------------------ ranking
// The order of the clusters is (size descending, smallest record ascending).  A component's smallest record is its root, and the
// keys are written in record order, so a STABLE sort by n - size alone gives that order: among equal sizes the roots stay ascending.
// key[i] = n - size for a root whose component is within the bounds (below n: a size is 1 or more), n for every other record:
// they end up behind the clusters.  val[i] = i.
__global__ __launch_bounds__(kBlock) void k_cluster_keys(uint32_t n, const uint32_t *root, const uint32_t *size, uint32_t min_size, uint32_t max_size,
                                                         uint32_t *keys, uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = size[i];
    keys[i] = (root[i] == i && m >= min_size && m <= max_size) ? n - m : n;
    vals[i] = i;
}

// The sorted pair c is the cluster of rank c while its key is below n.  rank[record] = c for the root of cluster c, kClusterNone for
// every other record (vals is a permutation: every word is written); sizes[c] = the cluster's records, 0 from the number of clusters
// on and at n (the exclusive prefix sum of sizes[0 .. n] is offsets); *n_clusters = where the keys reach n.
__global__ __launch_bounds__(kBlock) void k_cluster_rank(uint32_t n, const uint32_t *keys, const uint32_t *vals, uint32_t *rank, uint32_t *sizes,
                                                         uint32_t *n_clusters)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n) return;
    if (c == n) {
        sizes[n] = 0u;
        if (keys[n - 1] < n) *n_clusters = n;
        return;
    }
    const uint32_t k = keys[c];
    const bool is_cluster = k < n;
    rank[vals[c]] = is_cluster ? c : kClusterNone;
    sizes[c] = is_cluster ? n - k : 0u;
    if (!is_cluster && (c == 0 || keys[c - 1] < n)) *n_clusters = c;
}

// label[i] = the rank of record i's cluster, -1 without one (non-finite, or a component outside the bounds); and the pair (label, i)
// of the sort that lists the clusters' records -- written in record order, so a stable sort leaves a cluster's records ascending.
// The key of a record without a cluster is n: behind every cluster.  keys, vals: nullable together.
__global__ __launch_bounds__(kBlock) void k_cluster_labels(uint32_t n, const uint32_t *root, const uint32_t *rank, int32_t *label, uint32_t *keys,
                                                           uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root[i];
    const uint32_t c = r == kClusterNone ? kClusterNone : rank[r];
    label[i] = (int32_t)c;   // (kClusterNone is -1)
    if (keys) {
        keys[i] = c == kClusterNone ? n : c;
        vals[i] = i;
    }
}

// rsreg_cloud_cluster_filter: kept when the record's rank lies in [rank_lo, rank_hi) (negative: when it does not; a record without a
// cluster is outside every range)
__global__ __launch_bounds__(kBlock) void k_cluster_filter_flags(const int32_t *label, uint32_t n, uint32_t rank_lo, uint32_t rank_hi, int negative,
                                                                 uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t c = label[i];
    const bool inside = c >= 0 && (uint32_t)c >= rank_lo && (uint32_t)c < rank_hi;
    flags[i] = (negative ? !inside : inside) ? 1u : 0u;
}

}  // namespace rsreg
