"""tests/cluster_ref.py and tests/cluster_cases.py held against each other and against scipy, without a device: the reference of
rsreg_cloud_euclidean_clusters is PCL's seed loop over radius_ref's adjacency; its partition must be that of
scipy.sparse.csgraph.connected_components over the same adjacency, and that of the constructions whose components are known.
Beside them the figures the inputs of tests/test_clusters_gpu.py were chosen for, the size of rsreg_cluster_params and its
defaults, and that filters.hip compiles for gfx950 with the new kernels free of spills, scratch and LDS."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as K
import cluster_ref as CR
import radius_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _ref(name, tol):
    xyz = K.input_cloud(name).xyz
    nb = R.search(xyz, tol)
    return nb, CR.extract(xyz, tol, nb=nb)


def _same(a, b):
    return (a.n_clusters == b.n_clusters and a.labels.tobytes() == b.labels.tobytes() and a.indices.tobytes() == b.indices.tobytes()
            and a.offsets.tobytes() == b.offsets.tobytes())


SCIPY = [("uniform5000", 0.05), ("uniform5000", 0.1), ("non_finite", 0.1), ("sphere5000", 0.03), ("lattice", K.R_AT), ("lattice", K.R_FACE),
         ("snake_small", K.R_FACE), ("snake_small_cut", K.R_FACE)]


@pytest.mark.parametrize("name,tol", SCIPY)
def test_seed_loop_against_scipy(name, tol):
    from scipy.sparse.csgraph import connected_components
    xyz = K.input_cloud(name).xyz
    nb, c = _ref(name, tol)
    adj = CR.adjacency(nb, len(xyz))
    assert (adj != adj.T).nnz == 0                                    # the graph is symmetric
    _, comp = connected_components(adj, directed=False)
    comp = np.where(nb.fin, comp, -1)                                 # (scipy makes a non-finite record a component of its own)
    want = CR.from_groups(comp)
    print("clusters: %s at %g: %d components, the largest %d" % (name, tol, c.components, c.sizes.max()))
    assert c.components == len(np.unique(comp[nb.fin])) and _same(c, want)
    assert (c.labels[~nb.fin] == -1).all() and (c.labels[nb.fin] >= 0).all()
    # the shape of the three arrays: a partition of the finite records, ascending inside a cluster, sizes descending, ties by smallest record
    assert np.array_equal(np.sort(c.indices), np.flatnonzero(nb.fin)) and c.offsets[0] == 0 and c.offsets[-1] == len(c.indices)
    sizes, first = np.diff(c.offsets.astype(np.int64)), c.indices[c.offsets[:-1]].astype(np.int64)
    assert all((np.diff(f) > 0).all() for f in c.clusters)
    assert ((np.diff(sizes) < 0) | ((np.diff(sizes) == 0) & (np.diff(first) > 0))).all()


def test_bounds_drop_whole_components():
    xyz = K.input_cloud("uniform5000").xyz
    nb, every = _ref("uniform5000", 0.05)
    c = CR.extract(xyz, 0.05, 3, 14, nb=nb)
    kept = (every.sizes >= 3) & (every.sizes <= 14)
    assert c.n_clusters == kept.sum() and c.components == every.components
    assert sorted(np.diff(c.offsets).tolist()) == sorted(every.sizes[kept].tolist())
    inside = np.isin(every.labels, np.flatnonzero((np.diff(every.offsets) >= 3) & (np.diff(every.offsets) <= 14)))
    assert np.array_equal(c.labels >= 0, inside)


def test_snakes_are_what_their_construction_says():
    rows, width = K.SNAKE_SMALL
    assert len(K.input_cloud("snake_small")) == rows * width + rows - 1
    for name, cut in (("snake_small", None), ("snake_small_cut", 4), ("snake_large", None), ("snake_large_cut", K.SNAKE_CUT)):
        shape = K.SNAKE_SMALL if "small" in name else K.SNAKE_LARGE
        xyz, group = K.snake_groups(*shape, cut=cut)
        assert xyz.tobytes() == K.input_cloud(name).xyz.tobytes()
        assert (xyz.astype(np.float64) / K.H == np.round(xyz.astype(np.float64) / K.H)).all()      # exact in float32
        _, face = _ref(name, K.R_FACE)
        assert _same(face, CR.from_groups(group))
        if cut is not None:
            assert sorted(face.sizes.tolist()) == sorted(K.snake_sizes(*shape, cut))
        else:
            assert face.sizes.tolist() == [len(xyz)]
        _, at = _ref(name, K.R_AT)                                    # AT the tolerance: nothing is joined
        assert _same(at, CR.from_groups(np.arange(len(xyz)))) and at.n_clusters == len(xyz) and (at.labels == np.arange(len(xyz))).all()
    assert len(K.input_cloud("snake_large")) == 71959 > 65536


def test_blobs_are_one_component_each():
    xyz, group = K.blobs_groups()
    _, c = _ref("blobs", K.BLOB_TOL)
    assert _same(c, CR.from_groups(group))
    assert np.diff(c.offsets).tolist() == list(K.BLOB_SIZES) + [1] * K.BLOB_ISOLATED
    first = c.indices[c.offsets[:-1]].astype(np.int64)
    assert (np.diff(first[:3]) > 0).all() and (np.diff(first[6:]) > 0).all()    # the ties: by smallest record


def test_figures_of_the_frames():
    _, c = _ref("frame_pass", 0.02)
    assert (c.components, int(c.sizes.max()), int((c.sizes == 1).sum())) == (1446, 27781, 1078)
    assert _ref("frame_pass", 0.01)[1].components == 35151
    _, c = _ref("uniform5000", 0.05)
    assert (c.components, int(c.sizes.max())) == (2562, 22)
    _, c = _ref("frame_raw", 0.03)
    assert c.components == 36 and 6558 in c.sizes.tolist()
    xyz = K.input_cloud("frame_raw").xyz
    origin = np.flatnonzero((xyz == 0).all(axis=1))
    assert len(origin) == 6558 and len(np.unique(c.labels[origin])) == 1


def test_filter_keep_masks():
    labels = np.array([0, -1, 2, 1, 0, -1, 3], np.int32)
    assert CR.filter_keep(labels, 0, 1).tolist() == [True, False, False, False, True, False, False]
    assert CR.filter_keep(labels, 1, 3).tolist() == [False, False, True, True, False, False, False]
    assert CR.filter_keep(labels, 1, 3, negative=True).tolist() == [True, True, False, False, True, True, True]
    assert CR.filter_keep(labels, 0, 2 ** 32 - 1).tolist() == [True, False, True, True, True, False, True]
    assert not CR.filter_keep(labels, 2, 2).any()
    with pytest.raises(ValueError):
        CR.filter_keep(labels, 2, 1)


def test_library_and_adaptors(rs):
    from rsreg_amd import EuclideanClusterExtraction, api, lib
    lib.build()
    handle = lib.lib()
    for name in ("rsreg_cluster_params_default", "rsreg_cloud_euclidean_clusters", "rsreg_cloud_cluster_filter"):
        assert name in lib.EXPORTS and getattr(handle, name) is not None
    assert "cluster_kernels.hpp" in lib.HEADERS and "filters.hip" in lib.SOURCES and not any("cluster" in s for s in lib.SOURCES)
    assert handle.rsreg_version() == 4
    assert ctypes.sizeof(lib.ClusterParams) == 16
    header = open(os.path.join(ROOT, "include", "rsreg.h")).read()
    body = re.search(r"typedef struct rsreg_cluster_params \{(.*?)\} rsreg_cluster_params;", header, re.S).group(1)
    assert re.findall(r"^\s*(\w+) (\w+);", body, re.M) == [("double", "tolerance"), ("uint32_t", "min_cluster_size"), ("uint32_t", "max_cluster_size")]
    p = lib.ClusterParams(1.0, 7, 7)
    handle.rsreg_cluster_params_default(ctypes.byref(p))
    assert (p.tolerance, p.min_cluster_size, p.max_cluster_size) == (0.0, 1, 2 ** 31 - 1)       # PCL's defaults; the tolerance has none
    q = api.cluster_params(0.02, 8)
    assert (q.tolerance, q.min_cluster_size, q.max_cluster_size) == (0.02, 8, 2 ** 31 - 1)
    with pytest.raises(lib.RsregError):
        api.cluster_params(0.02, -1)
    assert EuclideanClusterExtraction is api.EuclideanClusterExtraction
    for name in ("euclidean_clusters", "cluster_filter"):
        assert hasattr(api.DeviceCloud, name)
    ec = EuclideanClusterExtraction()
    assert (ec.getClusterTolerance(), ec.getMinClusterSize(), ec.getMaxClusterSize()) == (0.0, 1, 2 ** 31 - 1)
    ec.setClusterTolerance(0.02)
    ec.setMinClusterSize(8)
    ec.setMaxClusterSize(25000)
    assert (ec.getClusterTolerance(), ec.getMinClusterSize(), ec.getMaxClusterSize()) == (0.02, 8, 25000)
    with pytest.raises(lib.RsregError):      # no input cloud: refused before any device call -- there is no device here
        ec.extract()


def test_filters_compile_for_gfx950_without_spill_or_scratch(tmp_path):
    """hipcc cross-compiles filters.hip (which includes cluster_kernels.hpp) for gfx950; the compiler's resource remarks show no new
    kernel spilling, using scratch or LDS."""
    from rsreg_amd import lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *lib._flags(False), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(lib.CSRC, "filters.hip"), "-o", str(tmp_path / "filters.dev.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", r.stdout)
    for kernel in ("k_cluster_init", "k_cluster_hook", "k_cluster_flatten", "k_cluster_keys", "k_cluster_rank", "k_cluster_labels", "k_cluster_filter_flags"):
        mine = [b for b in blocks if re.match(r"_ZN5rsreg\d+%sE" % kernel, b)]
        assert len(mine) == 1, kernel
        fig = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", mine[0])}
        print(kernel, fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0 and fig["VGPRs Spill"] == 0 and fig["LDS Size [bytes/block]"] == 0
