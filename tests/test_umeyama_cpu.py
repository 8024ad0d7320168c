"""The small solve that ends every ICP iteration -- 17 f64 sums in, a 4 x 4 float transform out (Eigen::umeyama without
scaling) -- on flat, thin, mirrored, far, half-turned, collinear and coincident matches, against a 60-digit reference
written from the definition (tests/umeyama_ref.py).  CPU part: the host forms of csrc/host_linalg.hpp (the C ABI's cold solve;
tests/cpp/linalg_runner.cpp: cold, warm from the identity, warm after another solve), the oracle's solve, and the two
neighbours NDT runs on the host (eig_sym3, svd_solve<6>).  tests/test_umeyama_gpu.py holds the device forms to the same table.

The table (tests/umeyama_cases.py) is fixed and every row runs in every form; nothing is skipped or filtered.

The bound of a well-posed case, per entry of T (umeyama_ref.bound), term by term:
  * half a float32 ulp of the reference entry: the one rounding the code makes, float(R) and float(t);
  * C * 2^-52 * kappa: the f64 error of the solve through the conditioning of the polar factor, kappa = s1 / (s2 + s3), or
    s1 / (s2 - s3) where det U det V < 0 (the last column of U is flipped: the two smallest singular values pull against
    each other);
  * family `far`: C * 2^-52 |mu_q| |mu_p| / s2, what the cancellation in sums / n - mu_q mu_p^T leaves of sigma.  C scales
    this term too: adding n = 1000 terms in f64 already outgrows the term taken once (reference from the sums against
    reference from the pairs, no solver involved: 1.47 x), see umeyama_ref.C;
  * for t = mu_q - R mu_p: the error of R, both terms above, once more times |mu_p|.
C is one constant for all families (umeyama_ref.C and the two measured ratios it came from).  Where the answer is the
identity by rule rather than by conditioning (`one-point`: sigma is exactly zero; `line-still`: collinear matches that
coincide) kappa is taken as 1.
"""
import numpy as np
import pytest

import umeyama_cases as uc
import umeyama_ref as ur
from umeyama_cases import check_rigid, expected

IDS = [c["id"] for c in uc.CASES]
WELL = [c["id"] for c in uc.CASES if c["posed"] == "well"]
ILL = [c["id"] for c in uc.CASES if c["posed"] == "ill"]
PINNED = [c["id"] for c in uc.CASES if c["posed"] == "well" or c["identity"]]
HOST_FORMS = ("abi", "cold", "warm-from-identity", "warm-after-full")


@pytest.fixture(scope="module")
def L(rs):
    from rsreg_amd import lib
    lib.build()
    return lib


@pytest.fixture(scope="module")
def refs():
    return {c["id"]: ur.from_pairs(c["P"], c["Q"]) for c in uc.CASES}


@pytest.fixture(scope="module")
def host(rs, L):
    """{form: {id: 4 x 4 float32}} and {"V": {form: {id: 9 f64}}} for the four host forms, plus both SVDs of every sigma."""
    from rsreg_amd import api
    uc.build_runner()
    S = np.array([c["sums"] for c in uc.CASES])
    full = uc.BY_ID["full-n1000"]["sums"]
    v_far = uc.orthonormalised(uc.V_ARBITRARY)
    sig = np.array([uc.sigma_as_the_code_does(s).ravel() for s in S])
    recs = [(1, S), (3, sig)] + [(2, uc.IDENT, s[None]) for s in S] + [(2, v_far, np.array([full, s])) for s in S]
    out = uc.run_runner(recs)
    n = len(S)
    assert (out[0]["ok"] == 1).all()
    T = {"abi": {}, "cold": {}, "warm-from-identity": {}, "warm-after-full": {}}
    V = {"warm-from-identity": {}, "warm-after-full": {}, "before": {}}
    for i, c in enumerate(uc.CASES):
        T["abi"][c["id"]] = np.asarray(api.umeyama_from_sums(c["sums"]), np.float32)
        T["cold"][c["id"]] = uc.T_rowmajor(out[0]["T"][i])
        wi, wf = out[2 + i], out[2 + n + i]
        assert wi["ok"][0] == 1 and (wf["ok"] == 1).all()
        T["warm-from-identity"][c["id"]] = uc.T_rowmajor(wi["T"][0])
        V["warm-from-identity"][c["id"]] = wi["V"][0].copy()
        T["warm-after-full"][c["id"]] = uc.T_rowmajor(wf["T"][1])
        V["warm-after-full"][c["id"]] = wf["V"][1].copy()
        V["before"][c["id"]] = wf["V"][0].copy()
    return {"T": T, "V": V, "svd": {c["id"]: out[1][i] for i, c in enumerate(uc.CASES)}}


# ------------------------------------------------------------------------------------------------ the table itself
def test_table_is_whole():
    """Every family at every size; what each family promises about its own input holds, by the reference alone."""
    by = {}
    for c in uc.CASES:
        by.setdefault(c["family"], []).append(len(c["P"]))
    assert set(by) == set(uc.FAMILIES)
    for fam in ("full", "wall", "thin", "mirror", "half-turn", "far", "line", "near-one-point"):
        assert set(by[fam]) == set(uc.SIZES), fam
    assert set(by["triangle"]) == {3} and set(by["one-point"]) == {4, 64, 1024} and set(by["equal-s"]) == {6, 8}
    assert len(uc.CASES) == 155
    for c in uc.CASES:
        assert c["P"].dtype == np.float32 and c["Q"].dtype == np.float32 and np.isfinite(c["sums"]).all()
        if c["exact_zero"]:   # sigma computed in f64 the way the code computes it
            assert (uc.sigma_as_the_code_does(c["sums"]) == 0).all(), c["id"]
        if c["family"] == "line":   # exactly collinear: dyadic coordinates, the cross products are exact in f64
            d = (c["P"][1:] - c["P"][0]).astype(np.float64)
            assert (np.cross(d, d[0]) == 0).all() and np.abs(d).max() > 0, c["id"]
            if c["identity"]:
                assert np.array_equal(c["P"], c["Q"])


def test_far_start_is_far(host):
    """What the warm start meets: the V an unrelated `full` solve left is nowhere near the identity."""
    v = next(iter(host["V"]["before"].values())).reshape(3, 3)
    np.testing.assert_allclose(v @ v.T, np.eye(3), atol=1e-14)
    assert np.abs(v - np.eye(3)).max() > 0.5


@pytest.mark.parametrize("cid", PINNED)
def test_case_is_well_designed(refs, cid):
    """A case whose own bound exceeds 1e-3 is mis-designed."""
    _, B = expected(uc.BY_ID[cid], refs[cid])
    assert np.isfinite(B).all() and B.max() < 1e-3, B.max()


def test_mirror_and_rank_families_are_what_they_say(refs):
    for c in uc.CASES:
        r, s = refs[c["id"]], refs[c["id"]]["s"]
        if c["family"] == "mirror" and len(c["P"]) > 3:
            assert r["sign"] == -1 and s[2] > 1e-3 * s[0], c["id"]   # the S[2] = -1 branch with a third singular value that counts
        if c["family"] in ("triangle",) or (c["family"] == "wall" and "noise" not in c["id"]):
            assert s[2] < 1e-13 * s[0] < s[1], c["id"]   # rank 2 by the code's rule
        if c["family"] == "line":
            assert s[1] < 1e-13 * s[0], c["id"]   # rank 1
        if c["family"] == "equal-s":
            assert s[1] > s[0] * (1 - 1e-6)
    thin = {c["id"]: refs[c["id"]]["s"] for c in uc.CASES if c["family"] == "thin" and len(c["P"]) > 3}
    ratios = np.array([s[2] / s[0] for s in thin.values()])
    assert (ratios > 1e-13).any() and (ratios < 1e-13).any() and ((ratios > 1e-14) & (ratios < 1e-11)).any()   # either side of the rank rule, and near it


# ------------------------------------------------------------------------------------------------ well-posed: against the reference
@pytest.mark.parametrize("form", HOST_FORMS)
@pytest.mark.parametrize("cid", PINNED)
def test_host_forms_match_reference(host, refs, cid, form):
    T = host["T"][form][cid]
    Tref, B = expected(uc.BY_ID[cid], refs[cid])
    err = np.abs(T.astype(np.float64) - Tref)
    assert (err <= B).all(), "worst error / bound %.3g\n%s" % ((err[:3] / B[:3]).max(), T)
    check_rigid(T)


@pytest.mark.parametrize("cid", PINNED)
def test_oracle_matches_reference(orc, refs, cid):
    """The checker of every parity test, held to the same reference and the same bound, the rows whose answer is the
    identity by rule (one point, a line that has not moved) included."""
    T = np.asarray(orc.umeyama_from_sums(uc.BY_ID[cid]["sums"]), np.float32)
    Tref, B = expected(uc.BY_ID[cid], refs[cid])
    err = np.abs(T.astype(np.float64) - Tref)
    assert (err <= B).all(), "worst error / bound %.3g" % (err[:3] / B[:3]).max()
    check_rigid(T)


@pytest.mark.parametrize("cid", PINNED)
def test_warm_start_does_not_move_the_answer(host, refs, cid):
    """T from the V an unrelated solve left equals T from V = I within the bound (not bit for bit: the sweeps differ)."""
    _, B = expected(uc.BY_ID[cid], refs[cid])
    a, b = host["T"]["warm-after-full"][cid].astype(np.float64), host["T"]["warm-from-identity"][cid].astype(np.float64)
    assert (np.abs(a - b) <= B).all(), "warm\n%s\ncold\n%s" % (a, b)


@pytest.mark.parametrize("cid", [c["id"] for c in uc.CASES if c["exact_zero"]])
def test_zero_cross_covariance_forgets_the_warm_start(host, cid):
    """sigma exactly zero: R is exactly the identity, t exactly mu_q - mu_p (dyadic), and the V handed to the next
    iteration is the identity again, whatever V came in (Eigen: nothing is ever rotated away from U = V = I)."""
    c = uc.BY_ID[cid]
    want = np.eye(4, dtype=np.float32)
    want[:3, 3] = (c["Q"][0].astype(np.float64) - c["P"][0].astype(np.float64)).astype(np.float32)
    for form in HOST_FORMS:
        np.testing.assert_array_equal(host["T"][form][cid], want, err_msg=form)
    assert np.abs(host["V"]["before"][cid] - uc.IDENT).max() > 0.5
    np.testing.assert_array_equal(host["V"]["warm-after-full"][cid], uc.IDENT)
    np.testing.assert_array_equal(host["V"]["warm-from-identity"][cid], uc.IDENT)


def test_completed_columns_are_orthonormal():
    """complete_u3 over a sweep of the angle between V's column and the columns of U already found, 1 to 89 degrees, rank 1
    and rank 2, twenty frames: U^T U = I to 4 * 2^-52.  After the second projection pass what is left along a found column
    is the rounding of three products and sums on unit vectors (under 2 * 2^-52), and normalising adds half an ulp per entry;
    a single pass leaves the first pass's rounding error divided by the norm that survived, up to 8 times as much at the
    switch to unit vectors (1/64 of the squared norm).  Above that switch the completed column is V's column less its part along the columns found; below it, it is not."""
    uc.build_runner()
    V0s, As, meta = uc.completion_sweep()
    (r,) = uc.run_runner([(7, V0s, As)])
    sides = {"from V": 0, "unit vector": 0}
    for i, m in enumerate(meta):
        U, V, s = r["U"][i].reshape(3, 3), r["V"][i].reshape(3, 3), r["s"][i]
        assert s[m["rank"] - 1] > 0.2 and (s[m["rank"]:] < 1e-13 * s[0]).all(), (m, s)
        assert np.abs(U.T @ U - np.eye(3)).max() <= 4 * ur.EPS, (m, np.abs(U.T @ U - np.eye(3)).max() / ur.EPS)
        k = m["rank"]
        w = V[:, k] - U[:, :k] @ (U[:, :k].T @ V[:, k])   # (the V that came out: Jacobi turns columns of W that are rounding noise freely)
        nn = float(w @ w)
        if nn > 1.01 / 64:
            sides["from V"] += 1
            assert np.abs(U[:, k] - w / np.sqrt(nn)).max() <= 8 * ur.EPS / np.sqrt(nn), m
        elif nn < 1 / 64 / 1.01:
            sides["unit vector"] += 1
            if k == 1:   # (the last column has one direction whoever picks it)
                assert np.abs(U[:, k] - w / np.sqrt(nn)).max() > 1e-3, m   # a unit vector's remainder instead
    assert sides["from V"] >= 100 and sides["unit vector"] >= 20, sides


# ------------------------------------------------------------------------------------------------ ill-posed: what can be asked
@pytest.mark.parametrize("form", HOST_FORMS)
@pytest.mark.parametrize("cid", ILL)
def test_ill_posed_is_still_a_best_fit(host, refs, cid, form):
    """No comparison of R with the reference (a spin about the line, any turn about one point, is free).  A rigid motion,
    centroid onto centroid, and an RMS residual no larger than the optimum's."""
    c, ref, T = uc.BY_ID[cid], refs[cid], host["T"][form][cid]
    check_rigid(T)
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    pmax = float(np.abs(c["P"]).max())
    # float(R) moves a point by at most 3 |p| 2^-24 per coordinate, float(t) by half an ulp; the f64 part as for t above
    slack = 3 * pmax * 2.0 ** -24 + 0.5 * ur.ulp32(t).max() + ur.C * ur.EPS * (1 + 3 * pmax)
    assert np.abs(R @ ref["mu_p"] + t - ref["mu_q"]).max() <= slack
    opt = ur.rms_residual(c["P"], c["Q"], ref["R"], ref["t"])
    got = ur.rms_residual(c["P"], c["Q"], R, t)
    assert got <= opt + np.sqrt(3) * slack, (got, opt)


# ------------------------------------------------------------------------------------------------ the forms against each other
@pytest.mark.parametrize("cid", IDS)
def test_host_forms_agree_bit_for_bit(host, cid):
    """Cold and warm-from-the-identity are the same operations; the C ABI is the same source through another compiler."""
    T, svd = host["T"], host["svd"][cid]
    np.testing.assert_array_equal(T["abi"][cid], T["cold"][cid])
    np.testing.assert_array_equal(T["cold"][cid], T["warm-from-identity"][cid])
    np.testing.assert_array_equal(host["V"]["warm-from-identity"][cid], svd["V3"])   # the V it hands on is the SVD's


@pytest.mark.parametrize("cid", IDS)
def test_jacobi_svd3_is_its_generic_twin(host, cid):
    """jacobi_svd3 against jacobi_svd<3>: the one difference is a reciprocal instead of three divisions in the columns of U
    that come from W (1 ulp of f64 there); s and V equal.  A completed column (rank < 3) is built from those columns by
    two projections and a normalisation: 1 ulp in each of two unit columns cannot move it by more than 8 * 2^-52."""
    r = host["svd"][cid]
    np.testing.assert_array_equal(r["s3"], r["sg"])
    np.testing.assert_array_equal(r["V3"], r["Vg"])
    s = r["s3"]
    U3, Ug = r["U3"].reshape(3, 3), r["Ug"].reshape(3, 3)
    for k in range(3):
        if s[k] > 0 and s[k] > 1e-13 * s[0]:
            assert (np.abs(U3[:, k] - Ug[:, k]) <= np.spacing(np.abs(Ug[:, k]))).all(), k
        else:
            assert np.abs(U3[:, k] - Ug[:, k]).max() <= 8 * ur.EPS, k
    # and both are what they claim: orthogonal factors of sigma
    sig = uc.sigma_as_the_code_does(uc.BY_ID[cid]["sums"])
    V = r["V3"].reshape(3, 3)
    scale = max(np.abs(sig).max(), 1e-300)
    assert np.abs(U3.T @ U3 - np.eye(3)).max() <= 8 * ur.EPS and np.abs(V.T @ V - np.eye(3)).max() <= 16 * ur.EPS
    assert np.abs(U3[:, :3] * s @ V.T - sig).max() <= 1e-13 * scale + 32 * ur.EPS * scale


def test_slow_sequence_warm_start(host):
    """Ten iterations of one alignment closing in, V carried from each to the next: every step within the bound of the
    reference from its pairs, and equal to the cold solve of the same sums within it."""
    seq = uc.slow_sequence()
    S = np.array([s for _, _, s in seq])
    warm, cold = uc.run_runner([(2, uc.IDENT, S), (1, S)])
    for k, (P, Q, _) in enumerate(seq):
        ref = ur.from_pairs(P, Q)
        B = ur.bound(ref)
        Tw, Tc = uc.T_rowmajor(warm["T"][k]), uc.T_rowmajor(cold["T"][k])
        assert (np.abs(Tw.astype(np.float64) - ur.T_of(ref)) <= B).all(), k
        assert (np.abs(Tw.astype(np.float64) - Tc) <= B).all(), k
        check_rigid(Tw)
    np.testing.assert_array_equal(warm["T"][0], cold["T"][0])
    assert np.abs(warm["V"][-1].reshape(3, 3) - np.eye(3)).max() > 0.05   # the start the later steps had was not the identity


def test_measured_ratios_behind_C(host, refs):
    """The two ratios umeyama_ref.C came from, measured again: error / bound-with-C=1.  Neither may have outgrown C / 4."""
    worst_sums = 0.0
    for c in uc.CASES:
        if c["posed"] != "well" or c["exact_zero"]:
            continue
        a, b = refs[c["id"]], ur.from_sums(c["sums"])
        B = ur.bound(a, c["far"], c=1.0)
        dR, dt = np.abs(_hp(b["_R"] - a["_R"])), np.abs(_hp(b["_t"] - a["_t"])).ravel()
        worst_sums = max(worst_sums, (dR / B[:3, :3]).max(), (dt / B[:3, 3]).max())
    worst_host = 0.0
    for c in uc.CASES:
        if c["family"] == "full":
            B = ur.bound(refs[c["id"]], c=1.0)
            err = np.abs(host["T"]["cold"][c["id"]].astype(np.float64) - ur.T_of(refs[c["id"]]))
            worst_host = max(worst_host, (err[:3] / B[:3]).max())
    print("sums vs pairs: %.3f   cold host form, family full: %.3f   C = %.1f" % (worst_sums, worst_host, ur.C))
    assert worst_sums <= ur.C / 4 and worst_host <= ur.C / 4, (worst_sums, worst_host)


def _hp(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


# ------------------------------------------------------------------------------------------------ eig_sym3
def _sym3_cases():
    g = np.random.default_rng(31)
    Qr = np.linalg.qr(g.normal(size=(3, 3)))[0]

    def spectrum(*w):
        A = Qr @ np.diag(w) @ Qr.T
        return (A + A.T) / 2
    return {"diagonal": np.diag([3.0, -1.0, 0.5]), "two-equal": spectrum(2.0, 2.0, 5.0), "three-equal": np.eye(3) * 0.75,
            "rank-1": spectrum(0.0, 0.0, 4.0), "rank-2": spectrum(0.0, 1.5, 4.0), "gap-1e-12": spectrum(1.0, 1.0 + 1e-12, 3.0),
            "tiny-and-huge": spectrum(1e-9, 1.0, 1e6), "general": spectrum(-2.0, 0.3, 1.1)}


@pytest.mark.parametrize("name", sorted(_sym3_cases()))
def test_eig_sym3(name):
    A = _sym3_cases()[name]
    uc.build_runner()
    (r,) = uc.run_runner([(4, A.reshape(1, 9))])
    w, V = r["w"][0], r["v"][0].reshape(3, 3)
    w_ref, _ = ur.eig_sym3(A)
    nA = np.linalg.norm(A, 2)
    assert (np.diff(w) >= 0).all()
    assert np.abs(w - w_ref).max() <= 8 * ur.EPS * nA, np.abs(w - w_ref).max() / (ur.EPS * nA)
    assert np.abs(V.T @ V - np.eye(3)).max() <= 8 * ur.EPS
    assert np.abs(A @ V - V * w).max() <= 16 * ur.EPS * nA   # (no comparison of vectors inside a cluster of equal eigenvalues)


# ------------------------------------------------------------------------------------------------ svd_solve<6>
def _sym6(spectrum, seed=5):
    """A symmetric 6 x 6 and a right-hand side.  A spectrum with zeros in it (NDT's Hessian on a wall: rank 5, on a line:
    rank 3) is built from small integer vectors instead of a rotation, so that the rank is exact in f64."""
    g = np.random.default_rng(seed)
    if 0.0 in spectrum:
        Bv = g.integers(-3, 4, (6, 6)).astype(np.float64)
        A = sum(w * np.outer(Bv[k], Bv[k]) for k, w in enumerate(spectrum))
        return A, g.normal(size=6)
    Qr = np.linalg.qr(g.normal(size=(6, 6)))[0]
    A = Qr @ np.diag(spectrum) @ Qr.T
    return (A + A.T) / 2, g.normal(size=6)


EPS6 = 6 * ur.EPS
SOLVE6 = {"full-rank": [9.0, 5.0, 3.0, 1.0, 0.5, 0.1], "rank-5-wall": [9.0, 5.0, 3.0, 1.0, 0.5, 0.0], "rank-3-line": [9.0, 5.0, 3.0, 0.0, 0.0, 0.0],
          "indefinite": [9.0, -5.0, 3.0, -1.0, 0.5, 0.1], "well-above-rule": [1.0, 0.5, 0.3, 0.2, 0.1, 64 * EPS6],
          "well-below-rule": [1.0, 0.5, 0.3, 0.2, 0.1, EPS6 / 64], "just-above-rule": [1.0, 0.5, 0.3, 0.2, 0.1, 2 * EPS6],
          "just-below-rule": [1.0, 0.5, 0.3, 0.2, 0.1, EPS6 / 2]}


@pytest.mark.parametrize("name", sorted(SOLVE6))
def test_svd_solve6(name):
    """x = pinv(A) b with Eigen's rule (s_i > 6 eps s_max) against the mpmath pseudo-inverse with the same rule.  A singular
    value within a factor 4 of the threshold may fall on either side: the answer must be one of the two, never neither."""
    A, b = _sym6(SOLVE6[name])
    uc.build_runner()
    x_run, s_run = uc.run_runner([(5, A.reshape(1, 36), b.reshape(1, 6)), (6, A.reshape(1, 36))])
    x, s_run = x_run["x"][0], s_run["s"][0]
    x_ref, s, coef, V = ur.pinv_solve6(A, b)
    assert np.abs(s_run - s).max() <= 16 * ur.EPS * s[0]
    thr = EPS6 * s[0]
    near = [k for k in range(6) if thr / 4 < s[k] < thr * 4]
    assert len(near) == (1 if name.startswith("just-") else 0), (name, s, thr)
    # x along each right singular vector of the reference.  Away from the rule: the coefficient (u_k . b) / s_k to the
    # error of an f64 SVD, 64 eps s1 / s_k of itself, or nothing where s_k is dropped; every comparison with an absolute
    # slack of 64 eps |x|, what the largest component of x leaves on the others.
    a = V.T @ x
    slack = 64 * ur.EPS * max(np.abs(x).max(), np.abs(x_ref).max())
    for k in range(6):
        if k in near:
            # the computed s_k is s_k +- a few eps s1, a sixth of itself here: kept (the coefficient within a factor 4,
            # sign and all) or dropped, never neither
            kept = coef[k] != 0 and 0.25 <= a[k] / coef[k] <= 4.0
            assert kept or abs(a[k]) <= slack, (k, a[k], coef[k])
        elif s[k] > thr:
            assert abs(a[k] - coef[k]) <= 64 * ur.EPS * (s[0] / s[k]) * abs(coef[k]) + slack, (k, a[k], coef[k])
        else:
            assert abs(a[k]) <= slack, (k, a[k])
    if not near:
        assert np.abs(x - x_ref).max() <= 64 * ur.EPS * (s[0] / min(v for v in s if v > thr)) * np.abs(x_ref).max() + slack
