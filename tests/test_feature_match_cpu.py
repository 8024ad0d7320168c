"""Feature matching without a GPU: the numpy reference (tests/feature_match_ref.py) against independent computations and its own
cases, the host-only slice rule (csrc/feature_plan.hpp) compiled on its own, the exported symbols, the refusals that need no
device and the size of rsreg_correspondence.  What is checked here is the yardstick of tests/test_feature_match_gpu.py and the
host side of the feature, not the kernels."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import feature_match_cases as K
import feature_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _d2_float64(src, tgt):
    """|s|^2 + |t|^2 - 2 s.t in float64: for the `exact` case every term is a small multiple of 2^-4, so this is the exact distance
    by a route that shares nothing with the reference's loop."""
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    return (s * s).sum(axis=1)[:, None] + (t * t).sum(axis=1)[None, :] - 2.0 * (s @ t.T)


def test_exact_case_equals_an_independent_float64_selection():
    src, tgt = K.exact()
    d2 = R.d2_matrix(src, tgt)
    d64 = _d2_float64(src, tgt)
    assert (d2.astype(np.float64) == d64).all()
    idx, dist = R.knn_from_d2(d2, R.valid_rows(src), R.valid_rows(tgt), 16)
    want = np.argsort(d64, axis=1, kind="stable")[:, :16]                    # stable: the lowest index among equals
    assert (idx == want).all() and (dist == np.take_along_axis(d64, want, axis=1)).all()
    ties = (d2 == dist[:, :1]).sum(axis=1)
    inside = (np.diff(dist, axis=1) == 0).any(axis=1)                        # two of the 16 kept at one distance
    at_the_cut = (d2 == dist[:, -1:]).sum(axis=1) > (dist == dist[:, -1:]).sum(axis=1)   # a row at the 16th distance is left out
    print("exact: of %d source rows %d have more than one nearest row, %d a tie among their 16, %d a tie at the cut; %d distinct d2 in %d pairs" %
          (len(src), (ties > 1).sum(), inside.sum(), at_the_cut.sum(), len(np.unique(d2)), d2.size))
    assert (ties > 1).mean() > 0.1 and inside.mean() > 0.9 and at_the_cut.mean() > 0.3   # ties are everywhere, or the case proves nothing
    pairs = R.correspondences_from_d2(d2, R.valid_rows(src), R.valid_rows(tgt))
    assert [p[1] for p in pairs] == d64.argmin(axis=1).tolist() and [p[0] for p in pairs] == list(range(len(src)))
    back = d64.argmin(axis=0)
    recip = R.correspondences_from_d2(d2, R.valid_rows(src), R.valid_rows(tgt), reciprocal=True)
    assert [(p[0], p[1]) for p in recip] == [(i, int(j)) for i, j in enumerate(d64.argmin(axis=1)) if back[j] == i]
    assert 0 < len(recip) < len(pairs)


def test_order_case_tells_summation_orders_apart():
    """Reversed bin order and a float64 sum rounded once DO give other bits than the contract's order on this case."""
    src, tgt = K.order()
    src, tgt = src[:200], tgt[:500]
    ref = R.d2_matrix(src, tgt)
    rev = np.zeros_like(ref)
    for b in reversed(range(R.DIM)):
        diff = src[:, b, None] - tgt[None, :, b]
        rev += diff * diff
    wide = np.zeros(ref.shape, np.float64)
    for b in range(R.DIM):
        diff = src[:, b, None].astype(np.float64) - tgt[None, :, b].astype(np.float64)
        wide += diff * diff
    wide = wide.astype(np.float32)
    print("order: reversed differs on %.1f %% of the pairs, float64-rounded on %.1f %%" % (100 * (rev != ref).mean(), 100 * (wide != ref).mean()))
    assert (rev != ref).mean() > 0.05 and (wide != ref).mean() > 0.05
    assert np.abs(rev.astype(np.float64) - ref).max() <= 1e-5 * ref.max()     # ... and only in the last bits


def test_rules_on_a_hand_made_pair():
    """Three source rows, three target rows on a line (bin 0 alone differs): distances by hand."""
    def rows(xs):
        out = np.zeros((len(xs), R.DIM), np.float32)
        out[:, 0] = xs
        return out
    src, tgt = rows([0.0, 1.0, 10.0]), rows([0.5, 0.5, 9.0])
    idx, d2 = R.knn(src, tgt, 2)
    assert idx.tolist() == [[0, 1], [0, 1], [2, 0]] and d2.tolist() == [[0.25, 0.25], [0.25, 0.25], [1.0, 90.25]]
    assert R.correspondences(src, tgt) == [(0, 0, 0.25), (1, 0, 0.25), (2, 2, 1.0)]
    # target 0's nearest source is row 0 (the tie with row 1 goes to the lower index): row 1 loses its good forward match
    assert R.correspondences(src, tgt, reciprocal=True) == [(0, 0, 0.25), (2, 2, 1.0)]
    assert R.correspondences(src, tgt, max_distance=0.5) == [(0, 0, 0.25), (1, 0, 0.25)]            # AT the bound: kept
    below = float(np.sqrt(np.float64(np.nextafter(np.float32(0.25), np.float32(0)))))
    assert below * below < 0.25 and R.correspondences(src, tgt, max_distance=below) == []
    assert R.correspondences(src, tgt, max_distance=0.0) == []
    assert R.correspondences(tgt, tgt, max_distance=0.0, reciprocal=True) == [(0, 0, 0.0), (2, 2, 0.0)]   # row 1 matches its copy, row 0
    assert R.correspondences(tgt, tgt, max_distance=0.0) == [(0, 0, 0.0), (1, 0, 0.0), (2, 2, 0.0)]
    src[1, 32] = np.nan
    idx, d2 = R.knn(src, tgt, 1)
    assert idx.tolist() == [[0], [-1], [2]] and d2.tolist() == [[0.25], [0.0], [1.0]]
    big = rows([3e38, -3e38])
    assert R.knn(big, big, 2)[1].tolist() == [[0.0, np.inf], [0.0, np.inf]]                          # an overflow is +inf, never NaN
    assert R.as_records(R.correspondences(src, tgt)).tobytes() == np.array([(0, 0, 0.25), (2, 2, 1.0)], R.CORRESPONDENCE_DTYPE).tobytes()


def test_real_rows_have_genuine_ties():
    src, tgt = K.real()
    assert src.dtype == np.float32 and src.shape[1] == 33 and R.valid_rows(src).all() and R.valid_rows(tgt).all()
    assert len(np.unique(tgt, axis=0)) < len(tgt) - 100                     # repeated rows
    assert (tgt == 0).mean() > 0.2                                           # zero bins
    d2 = R.d2_matrix(src, tgt)
    ties = (d2 == d2.min(axis=1)[:, None]).sum(axis=1)
    print("real: %d x %d rows, %d source rows with more than one nearest target row" % (len(src), len(tgt), (ties > 1).sum()))
    assert (ties > 1).sum() >= 100


@pytest.mark.parametrize("ns,nt", K.COPIES_SIZES)
def test_copies_case_lowest_index_wins(ns, nt):
    src, tgt, planted = K.copies(ns, nt, 200 + ns)
    _, slices = K.plan(ns, nt)
    if nt > K.TILE:
        assert {0, K.TILE - 1, K.TILE} <= set(planted.tolist())
    assert len(planted) >= min(nt, 2) and (slices == 1 or len(planted) >= 2 * slices)
    for k in K.KS + K.KS_EDGE:
        if len(planted) < k:
            continue
        idx, d2 = R.knn(src, tgt, k)
        for row in {0, ns // 2}:
            assert idx[row].tolist() == planted[:k].tolist() and (d2[row] == d2[row, 0]).all()
        assert (d2[0] == 0).all() and (ns == 1 or d2[ns // 2, 0] > 0)


def test_holes_case():
    src, tgt = K.holes()
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    assert not sv[0] and not tv[-1] and 36 <= (~sv).sum() <= 37 and 36 <= (~tv).sum() <= 37
    idx, d2 = R.knn(src, tgt, 5)
    assert (idx[~sv] == -1).all() and (d2[~sv] == 0).all() and (idx[sv] >= 0).all()
    assert not np.isin(idx[sv], np.flatnonzero(~tv)).any()                   # never a match
    pairs = R.correspondences(src, tgt)
    assert [p[0] for p in pairs] == np.flatnonzero(sv).tolist()              # never a query
    for k in K.KS + K.KS_EDGE:
        assert R.valid_rows(K.few_valid(k)).sum() == k
        R.knn(src, K.few_valid(k), k)
        with pytest.raises(ValueError):
            R.knn(src, K.few_valid(k - 1), k)


def test_overflow_case():
    """What the GPU test relies on, on the reference alone: +inf everywhere, never a NaN; source rows at +inf from every target row
    get the lowest valid indices; rows whose nearest is finite and whose 16th is not."""
    src, tgt = K.overflow()
    assert R.valid_rows(src).all() and R.valid_rows(tgt).all() and 100 <= len(src) <= 500 and 100 <= len(tgt) <= 500
    d2 = R.d2_matrix(src, tgt)
    assert not np.isnan(d2).any()
    share = np.isinf(d2).mean()
    with np.errstate(over="ignore"):
        diff = src[:, None, K.OVERFLOW_BIN] - tgt[None, :, K.OVERFLOW_BIN]
    idx4, d4 = R.knn(src, tgt, 4)
    all_inf = np.isinf(d4).all(axis=1)
    idx16, d16 = R.knn(src, tgt, 16)
    mixed = np.isfinite(d16[:, 0]) & np.isinf(d16[:, -1])
    print("overflow: %d x %d, +inf share %.2f, pairs whose difference overflows %d, rows with all four nearest at +inf %d, with a finite nearest and a +inf 16th %d" %
          (len(src), len(tgt), share, int(np.isinf(diff).sum()), int(all_inf.sum()), int(mixed.sum())))
    assert 0.25 <= share <= 0.75
    assert np.isinf(diff).sum() > 100                                        # 3e38 - -3e38: the difference itself
    assert all_inf.sum() >= 10 and (idx4[all_inf] == np.arange(4)).all()     # every target row is valid: the four lowest indices
    assert np.isinf(d2[all_inf]).all() and (idx16[all_inf] == np.arange(16)).all()
    assert mixed.sum() >= 5
    assert np.isinf(d2[-1]).all() and (src[-1].astype(np.float64) ** 2 < K.BIG).all()   # finite squares, a sum that overflows
    assert np.isfinite(d2[-2]).any() and d2[-2].min() > 1e30                 # far from every target row, at a finite distance from some
    # correspondences: +inf matches are kept at DBL_MAX with distance inf, and exactly they are dropped at 1e30 (1e60 > FLT_MAX)
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    for reciprocal in (False, True):
        kept = R.correspondences_from_d2(d2, sv, tv, R.DBL_MAX, reciprocal)
        cut = R.correspondences_from_d2(d2, sv, tv, 1e30, reciprocal)
        assert any(np.isinf(p[2]) for p in kept) and cut == [p for p in kept if np.isfinite(p[2])] and 0 < len(cut) < len(kept)
    assert len(R.correspondences_from_d2(d2, sv, tv)) == len(src)


def test_reciprocal_tie_at_infinity_on_a_hand_made_pair():
    """Source rows at 3e38, 2e38, 0 and target rows at -3e38, -3e38, 1 along bin 0.  Every distance but the last pair's is +inf
    (3e38 - -3e38 overflows in the difference, 2e38 - -3e38 too, 0 - -3e38 in the square), and +inf ties with +inf: every all-inf row
    takes index 0.  Source row 1's forward match is target 0, whose nearest source is row 0: not reciprocal."""
    def rows(xs):
        out = np.zeros((len(xs), R.DIM), np.float32)
        out[:, 0] = xs
        return out
    src, tgt = rows([3e38, 2e38, 0.0]), rows([-3e38, -3e38, 1.0])
    inf = np.inf
    assert R.d2_matrix(src, tgt).tolist() == [[inf, inf, inf], [inf, inf, inf], [inf, inf, 1.0]]
    assert R.correspondences(src, tgt) == [(0, 0, inf), (1, 0, inf), (2, 2, 1.0)]
    assert R.correspondences(src, tgt, reciprocal=True) == [(0, 0, inf), (2, 2, 1.0)]
    assert R.correspondences(src, tgt, max_distance=1e30) == [(2, 2, 1.0)] == R.correspondences(src, tgt, max_distance=1e30, reciprocal=True)
    assert R.knn(src, tgt, 3)[0].tolist() == [[0, 1, 2], [0, 1, 2], [2, 0, 1]]


def test_denormal_cases():
    """Squared distances below FLT_MIN from inputs that are all normal floats (or zeros): what is tested is the arithmetic of a
    pair, not the upload."""
    for name in K.DENORMALS:
        src, tgt = K.denormal(name)
        for rows in (src, tgt):
            assert ((rows == 0) | (np.abs(rows) >= K.FLT_MIN)).all() and R.valid_rows(rows).all()
        d2 = R.d2_matrix(src, tgt)
        den = (d2 > 0) & (d2 < K.FLT_MIN)
        _, d4 = R.knn(src, tgt, 4)
        den4 = (d4 > 0) & (d4 < K.FLT_MIN)
        print("denormal %s: %d x %d, denormal d2 %.1f %%, of the four nearest %.1f %%, zero %d, distinct values %d" %
              (name, len(src), len(tgt), 100 * den.mean(), 100 * den4.mean(), int((d2 == 0).sum()), len(np.unique(d2))))
        if name == "order":
            assert den.mean() >= 0.5 and den4.mean() >= 0.5 and not (d2 == 0).any()
            assert (src != 0).all() and (tgt != 0).all()
        elif name == "exact":
            assert den.all() and len(np.unique(d2)) < d2.size // 50
            ties = (d2 == d2.min(axis=1)[:, None]).sum(axis=1)
            assert (ties > 1).mean() > 0.1                                   # ties present, at the nearest itself
            # a difference of 0.25 * 2^-73 squares to half the smallest denormal and rounds to 0 (to even): the bits are a matter of rounding there
            assert np.float32(np.ldexp(np.float32(0.25), -73)) ** 2 == 0 and (np.ldexp(np.float32(0.5), -73) ** 2).view(np.uint32) == 2
        else:
            assert (d2.view(np.uint32) == 0).all() and np.signbit(src).any() and not np.signbit(src).all()
            idx, _ = R.knn(src, tgt, 16)
            assert (idx == np.arange(16)).all()


def test_self_rows_case():
    """source == target at k > 1 on the reference: column 0 is the lowest valid copy at d2 = 0, and the copies of a row come before
    every other row, in index order."""
    rows = K.self_rows()
    valid = R.valid_rows(rows)
    assert (~valid).sum() == 3
    idx, d2 = R.knn(rows, rows, 16)
    _, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    many = 0
    for i in np.flatnonzero(valid)[::7]:
        same = np.flatnonzero(valid & (inverse == inverse[i]))
        m = min(len(same), 16)
        assert idx[i, :m].tolist() == same[:m].tolist() and (d2[i, :m] == 0).all() and (m == 16 or d2[i, m] > 0)
        many += 1 < len(same)
    assert many > 20 and (idx[~valid] == -1).all()


def test_records_keep_the_rows_and_fill_the_rest():
    rows = K.order_rows(10, 1)
    for stride in (132, 144, 160):
        rec = K.records(rows, stride, seed=stride)
        assert rec.dtype.itemsize == stride and len(rec) == 10
        raw = rec.view(np.uint8).reshape(10, stride)
        assert raw[:, :132].tobytes() == rows.tobytes()
        assert stride == 132 or len(np.unique(raw[:, 132:])) > 8


def test_slice_rule():
    """csrc/feature_plan.hpp compiled alone (plain g++, under AddressSanitizer and UBSan) on a table of (ns, nt): at least one
    slice, no slice shorter than one tile unless the target is, the slices tile [0, nt) without gap or overlap, the grid fits one
    launch dimension, and tests/feature_match_cases.py restates the rule correctly."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "feature_plan_rule")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "cpp", "feature_plan_rule.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], input="".join("%d %d\n" % p for p in K.PLAN_TABLE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0].split() == ["constants", str(K.QUERIES), str(K.TILE), str(K.FILL)]
    assert len(lines) == 1 + len(K.PLAN_TABLE)
    several = 0
    for line, (ns, nt) in zip(lines[1:], K.PLAN_TABLE):
        v = [int(x) for x in line.split()]
        assert v[:2] == [ns, nt]
        qblocks, slices, begins = v[2], v[3], v[4:]
        assert (qblocks, slices) == K.plan(ns, nt) and qblocks == -(-ns // K.QUERIES)
        assert slices >= 1 and len(begins) == slices + 1
        assert begins[0] == 0 and begins[-1] == nt                            # covers [0, nt) ...
        lengths = np.diff(begins)
        assert (lengths >= (K.TILE if nt >= K.TILE else nt)).all()            # ... no overlap, never shorter than a tile unless nt is
        assert begins == [K.slice_begin(s, slices, nt) for s in range(slices + 1)]
        assert qblocks * slices < 2 ** 26 + K.FILL                            # one launch dimension holds the grid
        assert slices == 1 or qblocks * slices < 2 * K.FILL                   # fills the CUs a few times over, not more
        assert slices == max(1, nt // K.TILE) or qblocks * slices >= K.FILL   # ... and does so whenever the target is long enough
        several += slices > 1
    assert several >= 10 and K.plan(1, 20000)[1] > 100 and K.plan(3000, 16) == (47, 1) and K.plan(65, 2500)[1] > 1


@pytest.fixture(scope="module")
def L(rs):
    from rsreg_amd import lib
    lib.build()
    return lib


def test_library_exports_both_symbols(L):
    handle = L.lib()
    for name in ("rsreg_cloud_feature_knn", "rsreg_cloud_feature_correspondences"):
        assert name in L.EXPORTS and getattr(handle, name) is not None
    assert "features.hip" in L.SOURCES
    assert C.sizeof(L.Correspondence) == 12
    from rsreg_amd import api
    assert api.CORRESPONDENCE_DTYPE.itemsize == 12 and api.CORRESPONDENCE_DTYPE == R.CORRESPONDENCE_DTYPE
    assert callable(api.DeviceCloud.feature_knn) and callable(api.DeviceCloud.feature_correspondences)
    assert all(hasattr(api.CorrespondenceEstimation, m) for m in ("setInputSource", "setInputTarget", "determineCorrespondences",
                                                                  "determineReciprocalCorrespondences"))
    assert handle.rsreg_version() == 4


def test_null_clouds_are_refused_without_a_device(L):
    handle = L.lib()
    idx, d2 = np.full(4, 7, np.int32), np.full(4, 7, np.float32)
    assert handle.rsreg_cloud_feature_knn(None, None, None, 1, idx.ctypes.data, d2.ctypes.data) == L.RSREG_ERR_INVALID_ARG
    out, found = np.full(4, 7, R.CORRESPONDENCE_DTYPE), C.c_size_t(99)
    assert handle.rsreg_cloud_feature_correspondences(None, None, None, 1.0, 0, out.ctypes.data, 4, C.byref(found)) == L.RSREG_ERR_INVALID_ARG
    assert (idx == 7).all() and (d2 == 7).all() and found.value == 99 and (out["index_query"] == 7).all()
    from rsreg_amd import api
    ce = api.CorrespondenceEstimation()
    with pytest.raises(L.RsregError) as e:
        ce.determineCorrespondences()
    assert e.value.status == L.RSREG_ERR_INVALID_ARG


def test_correspondence_is_twelve_bytes():
    """sizeof(rsreg_correspondence), from the C compiler: the layout of pcl::Correspondence."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "size")
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "rsreg.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(rsreg_correspondence), ' \
              'offsetof(rsreg_correspondence, index_query), offsetof(rsreg_correspondence, index_match), offsetof(rsreg_correspondence, distance)); return 0; }\n'
        r = subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        assert subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split() == ["12", "0", "4", "8"]
