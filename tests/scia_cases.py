"""Cases of rsreg_cloud_error_transforms, rsreg_cloud_initial_alignment_hypotheses and rsreg_cloud_initial_alignment
(tests/test_scia_cpu.py, tests/test_scia_gpu.py), at the smallest sizes that reach each branch.  The clouds, tables and transforms are
tests/prerej_cases.py's; the two large cases follow the recipes of tests/prerej_edge_cases.py (a source of 8 193 tiles scored against
five target points under four DISTINCT transforms; 16 385 hypotheses of which two are valid), so the brute-force reference of every
case takes a second or two on the CPU.

What each constructed case is FOR is asserted on the reference by tests/test_scia_cpu.py; the GPU tests compare bits.

max_correspondence_distance is compared with the SQUARED distance (PCL's quirk, kept): THR = RANGE * RANGE.
"""
import collections
import functools
import math

import numpy as np

import prerej_cases as C
import prerej_edge_cases as PE
import sac_edge_cases as E
import scia_ref as R

TRUNCATED, HUBER = R.TRUNCATED, R.HUBER
THR = C.RANGE * C.RANGE
INF_DISTANCE = R.DEFAULT_DISTANCE          # sqrt(DBL_MAX): +inf as a float
BATCH_SIZES = (15, 16, 17, C.MAX_BATCH + 1)


# ---- scoring: name -> (source, target, transforms, error_function, max_correspondence_distance)
def lattice_pair():
    """(source 100, target 216): the target is the integer lattice 0 .. 5 cubed, a source record a lattice point + (0.25, 0, 0) or
    + (0.375, 0, 0): under the identity e is EXACTLY 0.0625 or 0.140625, and every other target record is at least 0.39 away"""
    g = np.arange(6, dtype=np.float32)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(80)
    src = tgt[rng.choice(len(tgt), 100, replace=False)].copy()
    src[:, 0] += np.where(np.arange(100) % 2 == 0, np.float32(0.25), np.float32(0.375))
    return src, tgt


STEP_E = np.float32(0.0625)
STEP_THRS = collections.OrderedDict([("one_step_below_e", float(np.nextafter(STEP_E, np.float32(0)))), ("at_e", float(STEP_E)),
                                     ("one_step_above_e", float(np.nextafter(STEP_E, np.float32(1))))])
SCALES = (-40, -20, 20, 40)


def scaled_transforms(Ts, e):
    out = np.array(Ts, np.float32)
    out[:, :3, 3] = np.ldexp(out[:, :3, 3], e)
    return out


def _score_cases():
    src, tgt = C.base_pair()
    Ts = C.transforms()
    c = collections.OrderedDict()
    for fn, tag in ((TRUNCATED, "truncated"), (HUBER, "huber")):
        for n in C.SOURCE_SIZES:
            c["%s_source_%d" % (tag, n)] = (src[:n], tgt, Ts, fn, THR)
        for H in BATCH_SIZES:
            c["%s_transforms_%d" % (tag, H)] = (src[:129], tgt, C.transforms(H, 3), fn, THR)
        ls, lt = lattice_pair()
        for name, thr in STEP_THRS.items():
            c["%s_thr_%s" % (tag, name)] = (ls, lt, np.eye(4, dtype=np.float32)[None], fn, thr)
        c["%s_thr_inf" % tag] = (src, tgt, Ts, fn, INF_DISTANCE)
        c["%s_thr_denormal" % tag] = (np.concatenate([tgt[:60], src[:40]]), tgt, Ts[:2], fn, 1e-40)   # (only e == 0 is within it)
        s2, t2 = C.SCORE_CASES["nonfinite_records"][:2]
        c["%s_nonfinite_records" % tag] = (s2, t2, Ts, fn, THR)
        c["%s_target_empty" % tag] = (src[:129], np.zeros((0, 3), np.float32), Ts[:3], fn, THR)
        c["%s_target_all_nan" % tag] = (src[:129], np.full((5, 3), np.nan, np.float32), Ts[:3], fn, THR)
        c["%s_source_empty" % tag] = (src[:0], tgt, Ts[:3], fn, THR)
        c["%s_transforms_none" % tag] = (src[:129], tgt, Ts[:0], fn, THR)
    for e in SCALES:   # cloud and thr times 2^e (thr is a SQUARED distance: 2^2e): the truncated errors keep their bytes
        c["truncated_scale_2^%+d" % e] = (E.scaled(src[:129], e), E.scaled(tgt, e), scaled_transforms(Ts[:7], e), TRUNCATED, math.ldexp(THR, 2 * e))
    return c


SCORE_CASES = _score_cases()
SCALE_BASE = "truncated_scale_base"
SCORE_CASES[SCALE_BASE] = (C.base_pair()[0][:129], C.base_pair()[1], C.transforms()[:7], TRUNCATED, THR)


def step_pairs():
    """[(label, source (1, 3), target, e float32, [thr ..])]: prerej_edge_cases.range_pairs (e exact: 0, 2^-149, 2^-148, 0.0625,
    0.875, the largest float below 2^127, +inf) with the thr one float step below e, at e and one step above, 2^-149 and +inf"""
    out = []
    for label, s, t, e in PE.range_pairs():
        thrs = {float(np.float32(2.0 ** -149)), math.inf}
        if np.isfinite(e) and e > 0:
            thrs |= {float(e), float(np.nextafter(e, np.float32(np.inf))), float(np.nextafter(e, np.float32(0)))}
        out.append((label, s, t, e, sorted(v for v in thrs if v > 0)))
    return out


@functools.lru_cache(maxsize=None)
def batch_cap_reference():
    """the errors of the 256 rows of prerej_edge_cases.batch_cap_below_256 (truncated, thr 1): those of its 4 distinct transforms"""
    src, tgt, Ts, pick, rng = PE.batch_cap_below_256()
    return R.error_transforms(Ts, src, tgt, TRUNCATED, rng * rng)[pick]


# ---- the sampler: name -> (source, target, table, params, count)
HYP_COUNT = 96
MSD_HALF, MSD_ABOVE_CLOUD = 0.52, 2.0      # at 0.52 about half of the candidates that meet an accepted sample are refused (unit box); no pair is 2 apart
LATE_ELIGIBLE = (5, 40, 77, 110)


def _hyp_cases():
    src, tgt, true_of = C.pair()
    n = len(src)
    c = collections.OrderedDict()
    for nr in (3, 4, 8):
        for k in (1, 5, 16):
            c["nr_%d_k_%d" % (nr, k)] = (src, tgt, C.table(n, n, k, true_of, 0.7, 10 + k, minus=(0, 7, 64, n - 1)), dict(nr_samples=nr, seed=nr * k), HYP_COUNT)
    one = C.table(n, n, 2, true_of, 0.7, 35)
    c["msd_half"] = (src, tgt, one, dict(min_sample_distance=MSD_HALF, seed=1), HYP_COUNT)
    c["msd_half_nr_4"] = (src, tgt, one, dict(min_sample_distance=MSD_HALF, nr_samples=4, seed=2), HYP_COUNT)
    c["msd_above_cloud"] = (src, tgt, one, dict(min_sample_distance=MSD_ABOVE_CLOUD, seed=3), HYP_COUNT)
    c["msd_square_inf"] = (src, tgt, one, dict(min_sample_distance=1e200, seed=3), 32)
    c["all_ineligible"] = (src, tgt, np.full((n, 2), -1, np.int32), dict(seed=4), 32)
    c["late_draws"] = (src, tgt, C.table(n, n, 2, true_of, 0.7, 36, minus=[i for i in range(n) if i not in LATE_ELIGIBLE]), dict(seed=5), HYP_COUNT)
    ts, tt = PE.twins()
    c["coincident_sources"] = (ts, tt, PE.true_table(np.arange(40)), dict(seed=6), HYP_COUNT)
    c["one_target_record"] = (src, tgt, np.full((n, 1), 7, np.int32), dict(seed=7), 32)
    for ns, nr in ((3, 3), (4, 4), (8, 8), (3, 4), (1, 3), (7, 8)):
        s, t, tr = C.pair(ns, 9)
        c["ns_%d_nr_%d" % (ns, nr)] = (s, t, PE.true_table(tr), dict(nr_samples=nr, seed=8), 32)
    s2, t2 = src.copy(), tgt.copy()
    s2[[3, 50, 51, 52]] = [[np.nan, 0, 0], [0, np.inf, 0], [np.nan] * 3, [0, 0, -np.inf]]
    t2[true_of[[10, 20, 30, 31, 32]]] = [[np.nan] * 3, [0, -np.inf, 0], [np.inf, 0, 0], [np.nan, 1, 1], [1, np.nan, 1]]
    c["nonfinite_records"] = (s2, t2, PE.true_table(true_of), dict(seed=9), HYP_COUNT)
    c["seed_2_63"] = (src, tgt, one, dict(seed=1 << 63, nr_samples=5), HYP_COUNT)
    c["source_empty"] = (src[:0], tgt, np.zeros((0, 2), np.int32), dict(seed=1), 8)
    return c


HYP_CASES = _hyp_cases()


# ---- the full call: name -> (source, target, table, guess or None, params)
PLANT_H, PLANT_DECOY_H, PLANT_K = C.ROUND, 5, 16


@functools.lru_cache(maxsize=None)
def planted_case():
    """C.ROUND + 1 hypotheses on a 40-record pair, every row of the table eligible, k = 16.  The target carries one more record, NaN,
    and every entry of the table names it -- except the three cells hypothesis PLANT_H = 16 384 draws, which hold its records' true
    matches, and the three cells hypothesis 5 draws, which hold wrong (finite) records.  Any other hypothesis is valid only if its
    three (record, column) draws all fall on those six cells.  So hypothesis 5 holds the lowest error through the whole first round and
    the ONLY hypothesis of the second round takes it."""
    src, tgt, true_of = C.pair(40, 6)
    tgt = np.concatenate([tgt, np.full((1, 3), np.nan, np.float32)])
    nbr = np.full((40, PLANT_K), 40, np.int32)
    seed = 11
    every = np.zeros((40, 1), np.int32)          # (eligibility is all the sampler reads of the table)
    cells = {}
    for h, good in ((PLANT_H, True), (PLANT_DECOY_H, False)):
        ids, _ = R.sampler(src, every, seed, h, 3, 0.0)
        assert len(ids) == 3
        for j, s in enumerate(ids):
            col = int(R.draw_index(seed, h, R.DRAWS + j, PLANT_K))
            assert (s, col) not in cells, "the two planted hypotheses share a cell: pick another seed"
            cells[(s, col)] = int(true_of[s]) if good else int(true_of[(s + 7) % 40])
    for (s, col), t in cells.items():
        nbr[s, col] = t
    return src, tgt, nbr, None, dict(max_iterations=C.ROUND + 1, max_correspondence_distance=THR, seed=seed)


RECOVERY_SEED = 0


@functools.lru_cache(maxsize=None)
def recovery_case():
    """400 points in the unit box and their copy under TURN (120 degrees, 0.5 m); 60 % of the rows of the table are random in both of
    their k = 2 columns, 40 % hold the true match in one; 256 iterations, samples at least 0.2 apart, thr = RANGE^2"""
    src, tgt, true_of = C.pair(400, 12)
    nbr = C.table(400, 400, 2, true_of, 0.4, 50)
    return src, tgt, nbr, None, dict(max_iterations=256, max_correspondence_distance=THR, min_sample_distance=0.2, seed=RECOVERY_SEED)


def _align_cases():
    src, tgt, true_of = C.pair()
    n = len(src)
    c = collections.OrderedDict()
    good = C.table(n, n, 2, true_of, 0.7, 35)
    random_rows = C.table(n, n, 2, true_of, 0.0, 37)
    turn = C.TURN.astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    base = dict(max_iterations=96, max_correspondence_distance=THR)
    c["truncated"] = (src, tgt, good, None, dict(base, seed=1))
    c["huber"] = (src, tgt, good, None, dict(base, seed=1, error_function=HUBER))
    c["nr_4_msd"] = (src, tgt, good, None, dict(base, seed=2, nr_samples=4, min_sample_distance=0.3))
    c["nr_8_k_16"] = (src, tgt, C.table(n, n, 16, true_of, 0.9, 38, minus=(0, 7, 64, n - 1)), None, dict(base, seed=3, nr_samples=8))
    c["thr_inf_truncated"] = (src, tgt, good, None, dict(max_iterations=32, seed=4))               # every error is +0: hypothesis 0 or the first valid one wins
    c["thr_inf_huber"] = (src, tgt, good, None, dict(max_iterations=32, seed=4, error_function=HUBER))
    c["tie_lower_h_wins"] = (src, tgt, random_rows, None, dict(max_iterations=64, max_correspondence_distance=1e-12, seed=5))
    c["guess_better"] = (src, tgt, random_rows, turn, dict(base, seed=6))
    c["guess_worse"] = (src, tgt, good, eye, dict(base, seed=6))
    nan_guess = turn.copy()
    nan_guess[1, 2] = np.nan
    c["guess_huber_inf"] = (src, tgt, np.full((n, 2), -1, np.int32), nan_guess, dict(base, seed=6, error_function=HUBER))   # its error is +inf: identity
    c["msd_above_cloud"] = (src, tgt, good, None, dict(base, seed=7, min_sample_distance=MSD_ABOVE_CLOUD))
    c["msd_above_cloud_guess"] = (src, tgt, good, turn, dict(base, seed=7, min_sample_distance=MSD_ABOVE_CLOUD))
    for it in (0, 1, 2):
        c["iterations_%d" % it] = (src, tgt, PE.true_table(true_of), None, dict(base, max_iterations=it, seed=8))
        c["iterations_%d_guess" % it] = (src, tgt, PE.true_table(true_of), eye, dict(base, max_iterations=it, seed=8))
    s2, t2 = HYP_CASES["nonfinite_records"][:2]
    c["nonfinite_records"] = (s2, t2, PE.true_table(true_of), None, dict(base, seed=9))
    c["source_empty"] = (src[:0], tgt, np.zeros((0, 2), np.int32), turn, dict(base))
    c["target_empty"] = (src, tgt[:0], np.full((n, 2), -1, np.int32), turn, dict(base))
    c["past_a_batch"] = (src, tgt, good, None, dict(base, max_iterations=C.MAX_BATCH + 1, seed=10))
    return c


ALIGN_CASES = _align_cases()


def align_case(name):
    return planted_case() if name == "planted_past_a_round" else recovery_case() if name == "recovery" else ALIGN_CASES[name]


ALL_ALIGN = list(ALIGN_CASES) + ["planted_past_a_round", "recovery"]


@functools.lru_cache(maxsize=None)
def align_reference(name):
    """scia_ref.initial_alignment's result of a case, computed once a process"""
    from rsreg_amd import api
    src, tgt, nbr, guess, prm = align_case(name)
    return R.initial_alignment(api, src, tgt, nbr, guess=guess, **prm)


@functools.lru_cache(maxsize=None)
def hyp_reference(name):
    from rsreg_amd import api
    src, tgt, nbr, prm, count = HYP_CASES[name]
    return R.hypotheses(api, src, tgt, nbr, prm.get("seed", 0), 0, count, prm.get("nr_samples", 3), prm.get("min_sample_distance", 0.0))


@functools.lru_cache(maxsize=None)
def score_reference(name):
    src, tgt, Ts, fn, mcd = SCORE_CASES[name]
    return R.error_transforms(Ts, src, tgt, fn, mcd)
