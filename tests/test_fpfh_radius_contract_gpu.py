"""The contract of tests/test_cloud_ops_contract_gpu.py for rsreg_cloud_fpfh_radius, on that module's frame and its two contexts:
on success the output keeps its id and its version goes up by exactly 1, the input and the normals keep both, and the output's
n / stride / width / height / is_dense are what include/rsreg.h says; on a refusal the status, the rsreg_last_error text and the
output's version, n and stride are untouched."""
import pytest

import test_cloud_ops_contract_gpu as T

pytestmark = pytest.mark.gpu

RADIUS = 0.025          # the frame's pixels are 0.01 apart: a dozen neighbours or more


@pytest.fixture(scope="module")
def env():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return T.Env()


def _call(e, ctx, inp, out, normals=None, radius=RADIUS):
    return e.L.rsreg_cloud_fpfh_radius(ctx, inp, e.normals if normals is None else normals, radius, out)


def test_success(env):
    out = env.cloud(env.a)
    in_before, normals_before, out_before = env.state(env.inp), env.state(env.normals), env.state(out)
    env.ok(_call(env, env.a.h, env.inp, out))
    (oid, over), shape = env.state(out)
    print("fpfh_radius version", out_before[0][1], "->", over, "shape", shape)
    assert oid == out_before[0][0] and over == out_before[0][1] + 1
    assert env.state(env.inp) == in_before and env.state(env.normals) == normals_before
    assert shape == (T.N, T.FPFH_BYTES, T.W, T.H, 1)
    env.ok(_call(env, env.a.h, env.inp, out))                                  # into a cloud that holds records: once more, by 1
    assert env.state(out) == ((oid, over + 1), shape)
    env.L.rsreg_cloud_destroy(out)


@pytest.mark.parametrize("case", ["null_context", "foreign_input", "foreign_output", "foreign_normals", "radius_zero", "radius_nan"])
def test_refusal(env, case):
    ctx = None if case == "null_context" else env.a.h
    inp = env.foreign if case == "foreign_input" else env.inp
    out = env.foreign if case == "foreign_output" else env.cloud(env.a, env.frame, 32)   # (holds records: n and stride could change)
    normals = env.foreign if case == "foreign_normals" else None
    radius = {"radius_zero": 0.0, "radius_nan": float("nan")}.get(case, RADIUS)
    before = env.state(out)
    env.sentinel()
    rc = _call(env, ctx, inp, out, normals, radius)
    text = env.L.rsreg_last_error(env.a.h).decode()
    print(case, rc, repr(text))
    want = "the radius must be finite and above 0" if case.startswith("radius") else T.SENTINEL
    assert (rc, text) == (T.INV, want)
    after = env.state(out)
    assert after[0] == before[0] and after[1][:2] == before[1][:2]
    if case != "foreign_output":
        env.L.rsreg_cloud_destroy(out)
