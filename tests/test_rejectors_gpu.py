"""The ICP rejector chain (include/rsreg.h: rsreg_icp_set_rejectors) on the GPU against tests/rejectors_ref.py: pair by pair over
whole alignments on both source paths, on ties and edges, above 65 536 records, in point-to-plane mode, through align(), its
refusals, and whether it helps on a source with flying pixels.  The loop and the inputs live in tests/rejector_cases.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rejector_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


@pytest.fixture(scope="module")
def two(api):
    a, b = api.Context(0), api.Context(0)
    yield a, b
    a.close()
    b.close()


# ---- 1. pair by pair over whole alignments, the plain source path here and the merged one in a child with RSREG_SORT_SMALL=1
@pytest.fixture(scope="module")
def plain_lockstep(api):
    return K.run_lockstep_cases(api, merged=False)


@pytest.fixture(scope="module")
def plain_edges(api):
    return K.run_edge_cases(api, merged=False)


def test_lockstep_in_the_callers_order(plain_lockstep):
    assert len(plain_lockstep) == 2 * (len(K.CHAINS) + 1)
    for name, seen in plain_lockstep.items():
        assert len(seen) == K.ITERATIONS, name
        assert all(kept < in_play for in_play, kept in seen), (name, seen)       # every chain removes pairs in every iteration
        assert all(kept >= 3 for _, kept in seen), (name, seen)


def test_ties_and_edges_in_the_callers_order(plain_edges):
    assert {"median-in-tie", "factor-0", "one-to-one-copies", "one-to-one,trimmed", "normal-strict", "m-0", "m-1", "m-2", "one-target"} <= set(plain_edges)


def test_both_on_the_merged_path(plain_lockstep, plain_edges):
    """RSREG_SORT_SMALL=1 (read when the library loads its switches: a process of its own): the same sources merged into weighted
    distinct points in Morton order.  The child asserts everything the parent did; the counts it saw are the parent's."""
    env = dict(os.environ, RSREG_SORT_SMALL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rejector_cases.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert got["lockstep"] == json.loads(json.dumps(plain_lockstep))
    assert got["edges"] == json.loads(json.dumps(plain_edges))


# ---- 3. a source above 65 536 records: the merged path without the switch
def test_large_source_with_copies(api, two):
    src, tgt, guess = K.pair("big-lattice")
    src_n, tgt_n = K.normals_of(api, two[0], "big-src", src), K.normals_of(api, two[0], "big-tgt", tgt)
    seen = K.lockstep(api, two[0], two[1], src, tgt, guess, K.CHAINS["normal,one-to-one,median"], src_n=src_n, tgt_n=tgt_n, expect_merged=True)
    assert len(seen) == K.ITERATIONS and all(3 <= s[1] < s[0] for s in seen)
    seen = K.lockstep(api, two[0], two[1], src, tgt, guess, K.CHAINS["trimmed,one-to-one"], reciprocal=1, iterations=2, expect_merged=True)
    assert all(3 <= s[1] < s[0] for s in seen)


# ---- 4. point-to-plane with [3, 1]: plane sums [0] and [1] are the kept count and the kept pairs' d2 (asserted inside the loop)
def test_point_to_plane(api, two):
    src, tgt, guess = K.frames()
    src_n, tgt_n = K.normals_of(api, two[0], "frames-src", src), K.normals_of(api, two[0], "frames-tgt", tgt)
    seen = K.lockstep(api, two[0], two[1], src, tgt, guess, [(3, 0.7), (1, 1.0)], plane=True, src_n=src_n, tgt_n=tgt_n)
    assert len(seen) == K.ITERATIONS and all(3 <= s[1] < s[0] for s in seen)


# ---- 5. whole alignments through align(): the chain runs between the staged kernels whatever pipeline is asked for
@pytest.mark.parametrize("chain", ["one-to-one,median", "normal,one-to-one,median"])
def test_align_gives_the_stepwise_result(api, two, chain):
    src, tgt, guess = K.frames()
    src_n, tgt_n = K.normals_of(api, two[0], "frames-src", src), K.normals_of(api, two[0], "frames-tgt", tgt)
    want = K.stepwise(api, two[0], src, tgt, guess, K.CHAINS[chain], src_n, tgt_n)
    plain = K.stepwise(api, two[0], src, tgt, guess, [])
    assert want[1] < plain[1] and want[0] == K.ITERATIONS
    for pipeline in (0, 2):
        icp = K.make_icp(api, two[1], src, tgt, K.CHAINS[chain], src_n=src_n, tgt_n=tgt_n, pipeline=pipeline)
        icp.align(guess)
        assert (icp.result.iterations, icp.result.n_correspondences) == want[:2], pipeline
        np.testing.assert_array_equal(icp.getFinalTransformation(), want[2])
        icp.align(guess)                                                       # a restarted alignment starts from the normals as handed in
        np.testing.assert_array_equal(icp.getFinalTransformation(), want[2])


# ---- 6. refusals, and the empty chain
def test_refusals(api, two):
    from rsreg_amd import lib
    L, ctx = lib.lib(), two[0]
    src, tgt, guess = K.pair("lattice")
    icp = K.make_icp(api, ctx, src, tgt)
    icp.begin(None)
    icp.end()

    def set_chain(entries):
        arr = (lib.Rejector * max(len(entries), 1))()
        for k, (kind, value) in enumerate(entries):
            arr[k].kind, arr[k].value = kind, value
        return L.rsreg_icp_set_rejectors(ctx.h, arr, len(entries))

    assert set_chain([(2, 0.0)]) == 0
    for bad in ([(0, 1.0)], [(5, 1.0)], [(1, float("nan"))], [(1, -0.5)], [(4, 0.0)], [(4, 1.0)], [(4, float("nan"))], [(2, 0.0)] * 9):
        assert set_chain(bad) == lib.RSREG_ERR_INVALID_ARG, bad
    assert set_chain([(1, 0.0), (1, float("inf"))] + [(2, 0.0)] * 6) == 0      # a factor of 0 or +inf and eight entries are fine
    # the normal test without normals on either side, then on one side only
    p = api.icp_params(max_iterations=2, criteria_mode=1, max_correspondence_distance=K.GATE)
    assert set_chain([(3, 0.5)]) == 0
    assert L.rsreg_icp_begin(ctx.h, None, C.byref(p)) == lib.RSREG_ERR_STATE
    n = np.zeros((len(src), 3), np.float32)
    assert L.rsreg_icp_set_source_normals(ctx.h, n.ctypes.data, len(n) - 1, 12) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_icp_set_source_normals(ctx.h, n.ctypes.data, len(n), 12) == 0
    assert L.rsreg_icp_begin(ctx.h, None, C.byref(p)) == lib.RSREG_ERR_STATE    # the target's are still missing
    t = np.zeros((len(tgt), 3), np.float32)
    assert L.rsreg_icp_set_target_normals(ctx.h, t.ctypes.data, len(t), 12) == 0
    assert L.rsreg_icp_begin(ctx.h, None, C.byref(p)) == 0
    stat = (lib.RejectorStat * 1)()
    assert L.rsreg_icp_rejector_stats(ctx.h, stat, 1, None) == lib.RSREG_ERR_STATE   # no search yet
    assert L.rsreg_icp_search(ctx.h, None, None) == 0
    got = C.c_int32(0)
    assert L.rsreg_icp_rejector_stats(ctx.h, None, 0, C.byref(got)) == 0 and got.value == 1
    assert L.rsreg_icp_end(ctx.h, None, None, 0) == 0
    # a new source drops the source's normals
    icp.setInputSource(K.cloud(src))
    icp._sync_inputs()
    assert set_chain([(3, 0.5)]) == 0
    assert L.rsreg_icp_begin(ctx.h, None, C.byref(p)) == lib.RSREG_ERR_STATE
    assert set_chain([]) == 0


def test_an_empty_chain_changes_nothing(api):
    """A context that had a chain and lost it, against a context that never had one: the same bytes, search, sums and transform."""
    src, tgt, guess = K.frames()
    fresh, used = api.Context(0), api.Context(0)
    out = []
    for ctx, first in ((fresh, None), (used, K.CHAINS["one-to-one,median"])):
        if first:
            K.stepwise(api, ctx, src, tgt, guess, first)
        icp = K.make_icp(api, ctx, src, tgt, [], pipeline=1)
        icp.begin(guess)
        i, d = icp.search()
        s = icp.sums()
        icp.end()
        icp.align(guess)
        out.append((i.tobytes(), d.tobytes(), s.tobytes(), icp.getFinalTransformation().tobytes(), icp.result.n_correspondences))
    assert out[0] == out[1]
    fresh.close()
    used.close()


# ---- 7. usefulness
def test_chain_is_not_worse_on_flying_pixels(api, two):
    """The 50 k "bench" pair with a fifth of the source 2 to 4 cm off the surface, 5 cm gate, 30 iterations from a coarse guess
    0.0056 off the truth (rejector_cases.outlier_pair): |T - ground truth|_F with [ONE_TO_ONE, MEDIAN_DISTANCE] against no chain.
    The same loop in numpy (filters_ref.search + rejectors_ref.apply_chain + Umeyama in float64) ends 0.00527 off with the chain
    and 0.01112 off without: the input separates them."""
    src, tgt, truth, guess = K.outlier_pair()
    err = {}
    for name, chain in (("chain", K.OUTLIER_CHAIN), ("none", [])):
        icp = K.make_icp(api, two[0], src, tgt, chain, iterations=K.OUTLIER_ITERATIONS, gate=K.OUTLIER_GATE)
        icp.align(guess)
        err[name] = float(np.linalg.norm(icp.getFinalTransformation().astype(np.float64) - truth))
    print("flying pixels: |T - truth|_F = %.6f with [2, 1], %.6f without" % (err["chain"], err["none"]))
    assert err["chain"] <= err["none"], err
