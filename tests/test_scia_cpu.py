"""CPU: the numpy reference of the SampleConsensusInitialAlignment contract (tests/scia_ref.py) on hand values, the struct layouts of
the Python binding against the header, and -- before the GPU is asked anything -- that the reference itself satisfies what each
constructed case of tests/scia_cases.py claims: a hypothesis accepted at a candidate draw >= 40, one that exhausts all 56 draws, a
minimum sample distance that rejects about half the candidates, the exact tie, the planted winner past a round, the recoverable pose.
"""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

import prerej_cases as C
import prerej_edge_cases as PE
import prerej_ref as PR
import scia_cases as K
import scia_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF32 = np.float32(np.inf)


def _api():
    from rsreg_amd import api
    return api


def test_generator_is_the_one_of_the_sections_before():
    """where the first three candidate draws are distinct, eligible and finite and no distance is asked, the sample is prerejective's:
    the same index(h, d, ns) for d = 0, 1, 2"""
    src, tgt, true_of = C.pair()
    nbr = C.table(len(src), len(tgt), 2, true_of, 0.7, 35)
    same = 0
    for h in range(64):
        ids, draws = R.sampler(src, nbr, 3, h, 3, 0.0)
        _, want, _ = PR.hypothesis(_api(), src, tgt, nbr, 3, h, 0.9)
        if len(set(want)) == 3:
            assert tuple(ids) == tuple(want) and draws == [0, 1, 2], h
            same += 1
        assert int(R.draw_index(3, h, 7, 120)) == int(PR.S.draw_index(3, h, 7, 120))
    assert same >= 55


def test_functors_on_hand_values():
    thr = np.float32(0.25)
    e = np.float32([0.0, 0.125, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), 1.0, np.inf])
    t = R.truncated_terms(e, thr)
    assert t.dtype == np.float64 and t.tolist() == [0.0, 0.5, 1.0, 1.0, 1.0, 1.0]
    # AT thr both branches agree: e / thr == 1.0, and Huber's 0.5 e^2 == 0.5 thr (2 e - thr)
    assert float(np.float32(0.25) / thr) == 1.0
    hub = R.huber_terms(e, thr)
    assert hub[:3].tolist() == [0.0, 0.5 * 0.125 * 0.125, 0.03125] and (0.5 * 0.25) * (2.0 * 0.25 - 0.25) == 0.03125
    assert hub[4] == 0.125 * 1.75 and hub[5] == math.inf
    just = float(e[3])
    assert hub[3] == (0.5 * 0.25) * (2.0 * just - 0.25) and hub[3] > hub[2]
    # one float step below thr the truncated term is below 1: the division is a float32 one
    below = np.nextafter(thr, np.float32(0))
    assert R.truncated_terms(below, thr) == float(np.float32(below / thr)) < 1.0
    # thr = +inf: +0 for every finite e, 1 for e = +inf; Huber: 0.5 e^2, +inf
    assert R.truncated_terms(np.float32([0.0, 3.0, 1e38, np.inf]), INF32).tolist() == [0.0, 0.0, 0.0, 1.0]
    assert R.huber_terms(np.float32([2.0, np.inf]), INF32).tolist() == [2.0, math.inf]
    # a denormal thr divides as IEEE
    d = np.float32(2.0 ** -148)
    assert R.truncated_terms(np.float32([2.0 ** -149, 2.0 ** -148, 2.0 ** -147]), d).tolist() == [0.5, 1.0, 1.0]
    assert R.threshold(R.DEFAULT_DISTANCE) == INF32 and R.threshold(1e-40) > 0 and R.threshold(1e-60) == 0


def test_struct_layouts_match_the_header():
    from rsreg_amd import lib as L
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "rsreg.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(rsreg_scia_params), offsetof(rsreg_scia_params, nr_samples), offsetof(rsreg_scia_params, error_function),
           offsetof(rsreg_scia_params, max_iterations), offsetof(rsreg_scia_params, seed));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rsreg_scia_result), offsetof(rsreg_scia_result, found), offsetof(rsreg_scia_result, sample),
           offsetof(rsreg_scia_result, match), offsetof(rsreg_scia_result, n_valid), offsetof(rsreg_scia_result, error));
    printf("%d %d\n", (int)RSREG_SCIA_TRUNCATED, (int)RSREG_SCIA_HUBER);
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    P, Q = L.SciaParams, L.SciaResult
    assert [int(v) for v in out[:5]] == [ctypes.sizeof(P), P.nr_samples.offset, P.error_function.offset, P.max_iterations.offset, P.seed.offset] == [40, 16, 20, 24, 32]
    assert [int(v) for v in out[5:11]] == [ctypes.sizeof(Q), Q.found.offset, Q.sample.offset, Q.match.offset, Q.n_valid.offset, Q.error.offset] == [152, 64, 72, 104, 136, 144]
    assert [int(v) for v in out[11:]] == [L.SCIA_TRUNCATED, L.SCIA_HUBER] == [R.TRUNCATED, R.HUBER]
    for name in ("rsreg_scia_params_default", "rsreg_cloud_error_transforms", "rsreg_cloud_initial_alignment_hypotheses", "rsreg_cloud_initial_alignment"):
        assert name in L.EXPORTS


def test_defaults():
    p = _api().scia_params()
    assert p.max_correspondence_distance == R.DEFAULT_DISTANCE and p.min_sample_distance == 0.0
    assert (p.nr_samples, p.error_function, p.max_iterations, p.seed) == (3, 0, 10, 0)


def test_step_cases_are_exact():
    """the lattice: e is exactly 0.0625 (even records) or 0.140625; one float step below thr the term is below 1, one step above it is 1"""
    src, tgt = K.lattice_pair()
    e, fin = R.nearest(np.eye(4, dtype=np.float32), src, tgt)
    assert fin.all() and (e[0::2] == K.STEP_E).all() and (e[1::2] == np.float32(0.140625)).all()
    terms = {name: R.truncated_terms(e, R.threshold(thr)) for name, thr in K.STEP_THRS.items()}
    assert (terms["one_step_below_e"] == 1.0).all()                                 # thr one step below e: e is one step ABOVE thr
    assert (terms["at_e"][0::2] == 1.0).all() and (terms["at_e"][1::2] == 1.0).all()
    assert (terms["one_step_above_e"][0::2] < 1.0).all() and (terms["one_step_above_e"][0::2] > 0.99999).all() and (terms["one_step_above_e"][1::2] == 1.0).all()
    for label, s, t, e1, thrs in K.step_pairs():
        want = {"0": 0.0, "2^-149": 2.0 ** -149, "2^-148": 2.0 ** -148, "0.0625": 0.0625, "0.875": 0.875, "below 2^127": 2.0 ** 127 * (1 - 2.0 ** -24), "+inf": math.inf}[label]
        assert float(e1) == want and len(thrs) >= 2


def test_scoring_cases_claims():
    assert (K.score_reference("truncated_thr_inf")[:7] == 0.0).all() and not np.signbit(K.score_reference("truncated_thr_inf")[:7]).any()
    assert (K.score_reference("truncated_thr_inf")[[9, 10]] == 300.0).all()          # a transform that holds inf or NaN: every term is 1
    assert np.isinf(K.score_reference("huber_thr_inf")[[9, 10]]).all()
    den = K.score_reference("truncated_thr_denormal")
    assert den[0] == 40.0 and den[1] == round(den[1]) and 90.0 <= den[1] <= 100.0    # the identity: the 60 target records find themselves; only e == 0 is within thr
    assert (K.score_reference("truncated_target_empty") == 129.0).all() and np.isinf(K.score_reference("huber_target_all_nan")).all()
    assert (K.score_reference("huber_source_empty") == 0.0).all() and len(K.score_reference("huber_transforms_none")) == 0
    non = K.score_reference("truncated_nonfinite_records")
    assert np.isfinite(non).all()
    base = K.score_reference(K.SCALE_BASE)
    assert 0 < base[1] < 129 and len(set(base.tolist())) >= 6
    for e in K.SCALES:                                                               # scaled by a power of two: the same bytes
        assert K.score_reference("truncated_scale_2^%+d" % e).tobytes() == base.tobytes(), e
    cap = K.batch_cap_reference()
    assert C.batch_cap(PE.CAP_N) == 255 and len(cap) == 256 and len({cap[0], cap[254], cap[255]}) == 3 and np.isfinite(cap[[0, 254, 255]]).all()


def test_sampler_cases_claims():
    src, tgt, nbr, prm, count = K.HYP_CASES["late_draws"]
    late = exhausted = 0
    for h in range(count):
        ids, draws = R.sampler(src, nbr, prm["seed"], h, 3, 0.0)
        late += len(ids) == 3 and draws[-1] >= 40
        exhausted += len(ids) < 3
        assert set(ids) <= set(K.LATE_ELIGIBLE)
    assert late >= 3 and exhausted >= 3, (late, exhausted)
    # the distance that rejects about half the candidates: of the candidates that reach the distance test (eligible, finite, new)
    src, tgt, nbr, prm, count = K.HYP_CASES["msd_half"]
    msd2 = K.MSD_HALF * K.MSD_HALF
    tried = refused = 0
    for h in range(count):
        ids = []
        for d in range(R.DRAWS):
            if len(ids) == 3:
                break
            c = int(R.draw_index(prm["seed"], h, d, len(src)))
            if nbr[c, 0] < 0 or c in ids:
                continue
            if ids:
                tried += 1
            if all(float(PR.S.l2_simple(src[c], src[s])) >= msd2 for s in ids):
                ids.append(c)
            else:
                refused += 1
    assert 0.35 < refused / tried < 0.65, (refused, tried)
    Ts, valid, words = K.hyp_reference("msd_half")
    assert valid.sum() >= count // 2
    for name in ("msd_above_cloud", "msd_square_inf", "all_ineligible", "ns_3_nr_4", "ns_1_nr_3", "ns_7_nr_8", "source_empty"):
        Ts, valid, words = K.hyp_reference(name)
        assert not valid.any() and (words == -1).all() and np.isnan(Ts).all(), name
    for name in ("ns_3_nr_3", "ns_4_nr_4", "ns_8_nr_8"):
        Ts, valid, words = K.hyp_reference(name)
        nr = int(name[-1])
        assert valid.sum() >= 8 and all(sorted(w[:nr]) == list(range(nr)) for w in words[valid]), name
    Ts, valid, words = K.hyp_reference("coincident_sources")                        # the twins 2 i and 2 i + 1 are accepted side by side: the solve decides
    assert valid.all() and any(len({int(v) // 2 for v in w[:3]}) < 3 for w in words)
    Ts, valid, words = K.hyp_reference("nonfinite_records")
    assert 0 < valid.sum() < len(valid) and ((words[~valid, 0] >= 0).any())         # filled, but a target record is not finite
    assert not np.isin(words[:, :3], [3, 50, 51, 52]).any()
    Ts, valid, words = K.hyp_reference("nr_8_k_16")
    assert valid.sum() > 80 and (words[valid] >= 0).all()
    assert (K.hyp_reference("nr_3_k_5")[2][:, 3:8] == -1).all() and (K.hyp_reference("nr_3_k_5")[2][:, 11:] == -1).all()


def test_full_call_cases_claims():
    eye = np.eye(4, dtype=np.float32)
    r = K.align_reference("tie_lower_h_wins")
    lowest = np.nanmin(r.errors)
    tied = np.flatnonzero(r.errors == lowest)
    assert lowest == 120.0 and len(tied) >= 2 and r.best_hypothesis == tied[0] == np.flatnonzero(r.valid)[0] and r.found
    r = K.align_reference("guess_better")
    assert not r.found and r.best_hypothesis == -1 and r.transform.tobytes() == C.TURN.astype(np.float32).tobytes() and r.n_valid == 95
    assert r.error < np.nanmin(r.errors) and np.isnan(r.errors[95]) and r.sample == (-1,) * 8
    r = K.align_reference("guess_worse")
    assert r.found and r.error < 1.0 and np.linalg.norm(r.transform.astype(np.float64) - C.TURN) < 1e-4
    r = K.align_reference("guess_huber_inf")
    assert not r.found and r.error == math.inf and (r.transform == eye).all() and r.n_valid == 0
    r = K.align_reference("msd_above_cloud")
    assert not r.found and r.n_valid == 0 and r.error == math.inf and (r.transform == eye).all() and np.isnan(r.errors).all()
    r = K.align_reference("msd_above_cloud_guess")
    assert not r.found and r.n_valid == 0 and r.error < 1.0 and r.transform.tobytes() == C.TURN.astype(np.float32).tobytes()
    for it, found, found_guess in ((0, False, False), (1, True, False), (2, True, True)):
        a, b = K.align_reference("iterations_%d" % it), K.align_reference("iterations_%d_guess" % it)
        assert a.found == found and b.found == found_guess and len(a.errors) == it, it
        assert a.n_valid == it and b.n_valid == max(it - 1, 0)
        assert (b.transform == eye).all() or b.found
        assert b.error == 120.0 or b.found                                           # the identity as a guess: every term is 1
    assert K.align_reference("iterations_0").error == math.inf
    r = K.align_reference("source_empty")
    assert not r.found and r.error == math.inf and (r.transform == eye).all()
    r = K.align_reference("target_empty")
    assert not r.found and r.error == 120.0 and r.transform.tobytes() == C.TURN.astype(np.float32).tobytes()
    for name in ("thr_inf_truncated", "thr_inf_huber"):
        r = K.align_reference(name)
        assert r.found and r.best_hypothesis == np.flatnonzero(r.valid)[0] or name.endswith("huber")
    assert (K.align_reference("thr_inf_truncated").errors[K.align_reference("thr_inf_truncated").valid] == 0.0).all()
    r = K.align_reference("past_a_batch")
    assert r.found and r.n_valid == C.MAX_BATCH + 1
    h = K.align_reference("huber")
    assert h.found and np.isfinite(h.errors[h.valid]).all()


def test_planted_winner_lies_past_a_round():
    r = K.align_reference("planted_past_a_round")
    assert r.n_valid == 2 and r.valid[K.PLANT_DECOY_H] and r.valid[K.PLANT_H] and K.PLANT_H == C.ROUND
    assert r.found and r.best_hypothesis == K.PLANT_H and r.errors[K.PLANT_H] < r.errors[K.PLANT_DECOY_H]
    assert np.linalg.norm(r.transform.astype(np.float64) - C.TURN) < 1e-4


def test_recoverable_pose():
    """the bar of the two sibling estimators on the same construction: within 1e-4 Frobenius of the truth"""
    r = K.align_reference("recovery")
    err = float(np.linalg.norm(r.transform.astype(np.float64) - C.TURN))
    print("recovery: winner %d of %d valid, error %.3g, |T - truth|_F = %.3g" % (r.best_hypothesis, r.n_valid, r.error, err))
    assert r.found and err <= 1e-4
