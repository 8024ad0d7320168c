"""A reference of pcl::EuclideanClusterExtraction (rsreg_cloud_euclidean_clusters, rsreg_cloud_cluster_filter) as include/rsreg.h
defines it, numpy and tests/radius_ref.py only, independent of the engine:

  * the adjacency is radius_ref.search's: record j is joined to record i when float32 d2(i, j) < float32(float64(tol) * float64(tol)),
    strictly; finite records only;
  * the components come from PCL's seed loop, written out: the outer loop over the records ascending, a queue that grows by the
    neighbours of each of its entries, the two bounds compared with the FINISHED queue (a component outside them is dropped whole), a
    sort of the queue's indices;
  * the clusters are then sorted by size descending with a STABLE sort: the seed loop finds the components in the order of their
    smallest record, so among equal sizes the one with the lower smallest record comes first -- the tie rule of the contract;
  * a non-finite record is never a seed: it belongs to no cluster (the contract's stated deviation);
  * labels[i] = the rank of record i's cluster, -1 without one; indices = the clusters' records one cluster after the other;
    offsets[c] .. offsets[c + 1] = cluster c's slice of indices.

from_groups() gives the same three arrays from a partition that is KNOWN (a construction's), without any search.
"""
import numpy as np

import radius_ref as R

INT_MAX = 2 ** 31 - 1


class Clusters:
    """clusters: list of ascending int64 arrays, ranked; labels (n,) int32; indices uint32; offsets (len(clusters) + 1,) uint32;
    components: the number of components before the bounds; sizes: their sizes in seed order."""

    @property
    def n_clusters(self):
        return len(self.clusters)


def _finish(n, found, min_size, max_size):
    """found: the components in the order of their smallest record, each an ascending array."""
    c = Clusters()
    c.components = len(found)
    c.sizes = np.array([len(f) for f in found], np.int64)
    kept = [f for f in found if min_size <= len(f) <= max_size]
    c.clusters = sorted(kept, key=lambda f: -len(f))          # (Python's sort is stable)
    c.labels = np.full(n, -1, np.int32)
    for rank, f in enumerate(c.clusters):
        c.labels[f] = rank
    c.indices = (np.concatenate(c.clusters) if c.clusters else np.zeros(0, np.int64)).astype(np.uint32)
    c.offsets = np.concatenate([[0], np.cumsum([len(f) for f in c.clusters])]).astype(np.uint32)
    return c


def extract(xyz, tolerance, min_size=1, max_size=INT_MAX, nb=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    nb = nb if nb is not None else R.search(xyz, tolerance)
    point_of = np.full(n, -1, np.int64)                       # record -> its distinct point in nb
    point_of[nb.orig] = nb.inv
    off, idx = nb.off, nb.idx
    processed = ~nb.fin                                       # (copied by ~)
    found = []
    for i in range(n):
        if processed[i]:
            continue
        queue = [i]
        processed[i] = True
        at = 0
        while at < len(queue):
            u = point_of[queue[at]]
            nbrs = idx[off[u]:off[u + 1]]
            new = nbrs[~processed[nbrs]]
            if len(new):
                processed[new] = True
                queue.extend(new.tolist())
            at += 1
        found.append(np.sort(np.array(queue, np.int64)))
    return _finish(n, found, min_size, max_size)


def from_groups(group, min_size=1, max_size=INT_MAX):
    """group (n,): the component of every record as any integer, negative for a record without one."""
    group = np.asarray(group, np.int64)
    order = np.argsort(group, kind="stable")
    order = order[group[order] >= 0]
    cuts = np.flatnonzero(np.diff(group[order])) + 1
    found = np.split(order, cuts) if len(order) else []
    found.sort(key=lambda f: f[0])                            # the seed loop's order: by smallest record
    return _finish(len(group), found, min_size, max_size)


def adjacency(nb, n):
    """The same graph as a scipy CSR matrix over all n records (a non-finite record has no entry)."""
    from scipy.sparse import csr_matrix
    lens = np.diff(nb.off)[nb.inv]
    rows = np.repeat(nb.orig, lens)
    cols = np.concatenate([nb.idx[nb.off[u]:nb.off[u + 1]] for u in nb.inv]) if len(nb.inv) else np.zeros(0, np.int64)
    return csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))


def filter_keep(labels, rank_lo, rank_hi, negative=False):
    """The records rsreg_cloud_cluster_filter keeps: rank in [rank_lo, rank_hi); a label of -1 is outside every range."""
    if rank_lo > rank_hi:
        raise ValueError("rank_lo must not exceed rank_hi")
    lab = np.asarray(labels).astype(np.int64)
    inside = (lab >= 0) & (lab >= rank_lo) & (lab < rank_hi)
    return ~inside if negative else inside
