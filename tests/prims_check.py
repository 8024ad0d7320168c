"""Run by tests/test_primitives_gpu.py in a child process: the library's radix sort (csrc/osort.hpp), prefix sums
(csrc/oscan.hpp) and compaction look-back (csrc/compact.hpp), through the test harness tests/cpp/prims.hip, against plain
numpy references, case by case.  Prints one JSON line per case ({"id", "ok", "detail"}) and a last {"done": ...} line.

    python tests/prims_check.py <harness .so> [--only SUBSTRING]

Every case is generated from a seed of its own.  Importing this module only defines the case grid (CASES); it neither
loads the harness nor touches a GPU, and it imports neither torch nor the product."""
import ctypes as C
import json
import sys
import time
import zlib

import numpy as np

SORT_TILE = {32: 4096, 64: 2048}     # pairs a workgroup sorts (osort.hpp: os_tile<K>())
SCAN_TILE, SCAN_SELF_TOP = 1024, 4096  # values a workgroup scans; beyond this many workgroups k_oscan_top runs (oscan.hpp)
COMPACT_TILE = 4096                  # elements a workgroup compacts; a look-back window is 64 predecessors (compact.hpp)

SORT_MODES = ("cleared", "product", "hist_ready", "reuse")   # prims.hip sort_case: modes 0 .. 3
DISTS = ("equal", "ones", "sorted", "reverse", "distinct16", "top_digit", "skew99")
BAD_ARGS = ("n_2^30", "end_bit_above_width", "plan_for_fewer", "plan_small_called_multi", "plan_multi_called_small")


def _sort_sizes(w):
    t = SORT_TILE[w]
    return [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 65535, 65536, 65537, 300007, 10 ** 6 + 3]


SORT_RANGES = {32: [(0, 1), (0, 7), (0, 8), (0, 9), (0, 10), (0, 22), (0, 31), (0, 32), (5, 29)],
               64: [(0, 33), (0, 43), (0, 61), (0, 64), (5, 37)]}
SORT_HUGE = {32: 16 * 10 ** 6, 64: 8 * 10 ** 6}   # many times the workgroups the GPU holds at once
SCAN_SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, SCAN_TILE * SCAN_SELF_TOP, SCAN_TILE * SCAN_SELF_TOP + 1, 16777233]
SCAN_HUGE = 49 * 1024 * SCAN_TILE - 1024 * SCAN_TILE + 3   # uint32 only: 49 153 workgroup sums, 49 chunks of k_oscan_top (the last holds one)
SCAN_KINDS = {32: ("counts", "wrap"), 64: ("counts", "big")}
COMPACT_SIZES = [1, 4095, 4096, 4097, 64 * 4096 - 1, 64 * 4096 + 1, 65 * 4096 + 1, 129 * 4096, 3 * 10 ** 7]
COMPACT_FLAGS = (("zero", "one"), ("one", "alt"), ("alt", "rand1"), ("rand1", "runs"), ("runs", "zero"))


def _sort_case(w, n, rng_, dist, mode):
    return dict(kind="sort", w=w, n=n, begin=rng_[0], end=rng_[1], dist=dist, mode=mode,
                id="sort-u%d-n%d-b%d-e%d-%s-%s" % (w, n, rng_[0], rng_[1], dist, mode))


def _cases():
    out = []
    for w in (32, 64):
        full = (0, w)
        t = SORT_TILE[w]
        for n in _sort_sizes(w) + [SORT_HUGE[w]]:
            out.append(_sort_case(w, n, full, "uniform", "product"))
        for r in SORT_RANGES[w]:
            for n in (65, t - 1, 2 * t + 1, 300007):
                if r != full:   # (the full range: the sizes above)
                    out.append(_sort_case(w, n, r, "uniform", "product"))
        for r in ([full] if w == 32 else [full, (0, 43)]):
            for dist in DISTS:
                for n in (1000, t + 1, 300007, 10 ** 6 + 3):
                    out.append(_sort_case(w, n, r, dist, "product"))
        r = (0, 32) if w == 32 else (0, 43)
        for mode in SORT_MODES:
            for n in (1000, t + 1, 65537, 300007):
                out.append(_sort_case(w, n, r, "uniform", mode))
            out.append(_sort_case(w, 300007, r, "skew99", mode))
        for dist in ("uniform", "distinct16"):
            out.append(dict(kind="streams", w=w, ns=(1000, t + 1, 65537, 300007), begin=r[0], end=r[1], dist=dist,
                            id="sort-u%d-4streams-b%d-e%d-%s" % (w, r[0], r[1], dist)))
        for which, name in enumerate(BAD_ARGS):
            out.append(dict(kind="bad_args", w=w, which=which, id="sort-u%d-rejects-%s" % (w, name)))
    for w in (32, 64):
        for kind in SCAN_KINDS[w]:
            for n in SCAN_SIZES + ([SCAN_HUGE] if w == 32 else []):
                layouts = [(0, 0, 0), (1, 1, 5)]                     # (offset, in place, init)
                if n in (4097, SCAN_TILE * SCAN_SELF_TOP + 1):
                    layouts += [(1, 0, 5), (0, 1, 0)]
                out.append(dict(kind="scan", w=w, n=n, values=kind, layouts=layouts, id="scan-u%d-n%d-%s" % (w, n, kind)))
    for k, n in enumerate(COMPACT_SIZES):
        for fa, fb in COMPACT_FLAGS:
            out.append(dict(kind="compact", n=n, fa=fa, fb=fb, at=(0, 1, 7)[k % 3], id="compact-n%d-%s-%s" % (n, fa, fb)))
    return list({c["id"]: c for c in out}.values())   # (the grids overlap: each case once, in first-seen order)


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------- data

def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def _uniform(rng, n, bits):
    """n values of `bits` random bits (uint64)."""
    if bits == 0:
        return np.zeros(n, np.uint64)
    return rng.integers(0, (1 << bits) - 1, size=n, dtype=np.uint64, endpoint=True)


def _field(rng, n, width, dist):
    """the sort keys' bits inside the range (uint64, `width` bits)"""
    top = (1 << width) - 1
    if dist == "uniform":
        return _uniform(rng, n, width)
    if dist == "equal":
        return np.full(n, _uniform(rng, 1, width)[0], np.uint64)
    if dist == "ones":
        return np.full(n, top, np.uint64)
    if dist in ("sorted", "reverse"):
        f = np.sort(_uniform(rng, n, width))
        return f if dist == "sorted" else f[::-1].copy()
    if dist == "distinct16":
        return _uniform(rng, 16, width)[rng.integers(0, 16, size=n)]
    if dist == "top_digit":   # only the last pass's digit varies
        last = 8 * ((width - 1) // 8)
        low = _uniform(rng, 1, last)[0] if last else np.uint64(0)
        return (_uniform(rng, n, width - last) << np.uint64(last)) | low
    if dist == "skew99":      # 99 % of the keys one value: one digit of every pass
        f = np.full(n, _uniform(rng, 1, width)[0], np.uint64)
        some = rng.random(n) < 0.01
        f[some] = _uniform(rng, int(some.sum()), width)
        return f
    raise ValueError(dist)


def _sort_input(case_id, w, n, begin, end, dist):
    """keys (the range's bits by `dist`, every bit outside the range random), values (a permutation of arbitrary uint32)"""
    rng = _rng(case_id)
    width = end - begin
    f = _field(rng, n, width, dist)
    outside = _uniform(rng, n, w) & ~np.uint64(((1 << width) - 1) << begin)
    keys = (f << np.uint64(begin)) | outside
    if dist == "ones" and (begin, end) == (0, w):
        assert (keys == np.uint64(2 ** w - 1)).all()
    keys = keys.astype(np.uint32 if w == 32 else np.uint64)
    salt = int(rng.integers(0, 2 ** 32))
    vals = ((rng.permutation(n).astype(np.uint64) * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return keys, vals


def _digits(keys, begin, end):
    return (keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)


def _hist(keys, begin, end):
    """passes x 256 digit counts, as k_os_hist leaves them"""
    passes = (end - begin + 7) // 8
    h = np.zeros((passes, 256), np.uint32)
    k = keys.astype(np.uint64)
    for p in range(passes):
        bit = begin + 8 * p
        d = (k >> np.uint64(bit)) & np.uint64((1 << min(8, end - bit)) - 1)
        h[p] = np.bincount(d.astype(np.int64), minlength=256)[:256]
    return h


def _flags(rng, n, kind):
    i = np.arange(n)
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "one":
        return np.ones(n, np.uint8)
    if kind == "alt":
        return (i & 1).astype(np.uint8)
    if kind == "rand1":
        return (rng.random(n) < 0.01).astype(np.uint8)
    if kind == "runs":        # flags in 3 of every 100 workgroups only: runs of 97 empty ones, longer than a look-back window
        busy = (i // COMPACT_TILE) % 100 < 3
        return (busy & (rng.random(n) < 0.5)).astype(np.uint8)
    raise ValueError(kind)


# -------------------------------------------------------------------------------------------------------------- checks

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _first_diff(got, want, what):
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    i = int(bad[0])
    return "%s: %d of %d differ, first at %d (got %#x, want %#x)" % (what, len(bad), len(want), i, int(got[i]), int(want[i]))


class HipError(RuntimeError):
    pass


def _call(fn, *args):
    e = fn(*args)
    if e != 0:
        raise HipError("hipError_t %d" % e)


def _check_sort(L, c):
    w, n, begin, end = c["w"], c["n"], c["begin"], c["end"]
    keys, vals = _sort_input(c["id"], w, n, begin, end, c["dist"])
    perm = np.argsort(_digits(keys, begin, end), kind="stable")
    want_k, want_v = keys[perm], vals[perm]
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    info = np.zeros(4, np.int32)
    hist = np.ascontiguousarray(_hist(keys, begin, end)) if c["mode"] == "hist_ready" else np.zeros(1, np.uint32)
    fn = L.prims_osort_u32 if w == 32 else L.prims_osort_u64
    _call(fn, _p(keys), _p(vals), C.c_size_t(n), C.c_uint(begin), C.c_uint(end), C.c_int(SORT_MODES.index(c["mode"])), _p(hist), _p(ko), _p(vo), _p(info))
    errs = [e for e in (_first_diff(ko, want_k, "keys"), _first_diff(vo, want_v, "values")) if e]
    if not (info[0] == info[1] == info[2]):
        errs.append("in_first %d, osort_ends_in_first %d, radix32_plan.ends_in_first %d" % tuple(info[:3]))
    if not info[3]:
        errs.append("a guard element behind an output (or the hist_ready region of the scratch) was written")
    return errs


def _check_streams(L, c):
    w, ns, begin, end = c["w"], c["ns"], c["begin"], c["end"]
    parts = [_sort_input("%s/%d" % (c["id"], s), w, n, begin, end, c["dist"]) for s, n in enumerate(ns)]
    keys, vals = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    info = np.zeros(5, np.int32)
    fn = L.prims_osort_streams_u32 if w == 32 else L.prims_osort_streams_u64
    _call(fn, _p(keys), _p(vals), _p(np.array(ns, np.uint64)), C.c_uint(begin), C.c_uint(end), _p(ko), _p(vo), _p(info))
    errs, at = [], 0
    for s, (k, v) in enumerate(parts):
        perm = np.argsort(_digits(k, begin, end), kind="stable")
        n = len(k)
        for e in (_first_diff(ko[at:at + n], k[perm], "stream %d keys" % s), _first_diff(vo[at:at + n], v[perm], "stream %d values" % s)):
            if e:
                errs.append(e)
        at += n
    if not info[4]:
        errs.append("a guard element behind an output was written")
    return errs


def _check_bad_args(L, c):
    out = np.full(4, -1, np.int32)
    _call(L.prims_osort_bad_args, C.c_int(c["w"]), C.c_int(c["which"]), _p(out))
    errs = []
    if out[0] != 1:   # hipErrorInvalidValue
        errs.append("returned hipError_t %d, not hipErrorInvalidValue (1)" % out[0])
    if out[1] != 0:
        errs.append("%d operations queued on the stream" % out[1])
    if out[2] != 1:
        errs.append("the stream is not idle")
    if out[3] != 1:
        errs.append("*in_first left %d" % out[3])
    return errs


def _check_scan(L, c):
    w, n = c["w"], c["n"]
    dt = np.uint32 if w == 32 else np.uint64
    rng = _rng(c["id"])
    hi = {"counts": 1 << 12, "wrap": 1 << 32, "big": 1 << 40}[c["values"]]
    x = rng.integers(0, hi, size=n, dtype=np.uint64).astype(dt)
    incl = np.cumsum(x, dtype=dt)
    fn = L.prims_oscan_u32 if w == 32 else L.prims_oscan_u64
    init_t = C.c_uint32 if w == 32 else C.c_uint64
    errs = []
    for offset, inplace, init in c["layouts"]:
        for inclusive in (0, 1):
            want = incl + dt(init) if inclusive else incl - x + dt(init)
            got = np.empty_like(x)
            guards = np.zeros(2, np.int32)
            _call(fn, _p(x), _p(got), C.c_size_t(n), C.c_int(inclusive), C.c_size_t(offset), C.c_int(inplace), init_t(init), _p(guards))
            tag = "%s offset %d %s init %d" % ("inclusive" if inclusive else "exclusive", offset, "in place" if inplace else "apart", init)
            e = _first_diff(got, want, tag)
            if e:
                errs.append(e)
            if not guards[0]:
                errs.append(tag + ": an element in front of or behind the output was written")
            if not guards[1]:
                errs.append(tag + ": the input was changed")
    if w == 64 and c["values"] == "big" and n > 4096 and not int(incl[-1]) >> 32:
        errs.append("the case's total does not pass 2^32")
    return errs


def _check_compact(L, c):
    n = c["n"]
    rng = _rng(c["id"])
    fa, fb = _flags(rng, n, c["fa"]), _flags(rng, n, c["fb"])
    ia, ib = np.cumsum(fa, dtype=np.uint32), np.cumsum(fb, dtype=np.uint32)
    ea, eb, tot = np.empty(n, np.uint32), np.empty(n, np.uint32), np.zeros(2, np.uint32)
    guards = np.zeros(2, np.int32)
    _call(L.prims_compact_counts, _p(fa), _p(fb), C.c_size_t(n), C.c_uint32(c["at"]), _p(ea), _p(eb), _p(tot), _p(guards))
    errs = [e for e in (_first_diff(ea, ia - fa, "count a"), _first_diff(eb, ib - fb, "count b")) if e]
    if (int(tot[0]), int(tot[1])) != (int(ia[-1]), int(ib[-1])):
        errs.append("totals (%d, %d), want (%d, %d)" % (tot[0], tot[1], ia[-1], ib[-1]))
    if not guards[0]:
        errs.append("a scratch word in front of `at` or behind the plan's end was written")
    if not guards[1]:
        errs.append("a guard element behind an output was written")
    return errs


CHECKS = {"sort": _check_sort, "streams": _check_streams, "bad_args": _check_bad_args, "scan": _check_scan, "compact": _check_compact}


def main(argv):
    so = argv[1]
    only = argv[argv.index("--only") + 1] if "--only" in argv else ""
    L = C.CDLL(so)
    count = C.c_int(0)
    if L.prims_device_count(C.byref(count)) != 0 or count.value < 1:
        print(json.dumps({"done": False, "error": "no HIP device"}), flush=True)
        return 2
    t0, failed = time.time(), 0
    for c in CASES:
        if only not in c["id"]:
            continue
        t = time.time()
        try:
            errs = CHECKS[c["kind"]](L, c)
        except HipError as e:
            # (a HIP error may leave the device unusable: nothing more is started on it)
            print(json.dumps({"id": c["id"], "ok": False, "detail": str(e)}), flush=True)
            print(json.dumps({"done": False, "error": "%s: %s; the remaining cases were not run" % (c["id"], e)}), flush=True)
            return 1
        failed += bool(errs)
        print(json.dumps({"id": c["id"], "ok": not errs, "detail": "; ".join(errs)[:2000], "s": round(time.time() - t, 3)}), flush=True)
    print(json.dumps({"done": True, "failed": failed, "seconds": round(time.time() - t0, 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
