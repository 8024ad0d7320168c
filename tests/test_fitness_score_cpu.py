"""CPU side of getFitnessScore: the numpy reference (tests/fitness_ref.py) against an independent brute force, the sharded
helper (sharded_fitness_score) over a real gloo all-reduce with a fake stepper, and the Python surface without a GPU."""
import os
import socket
import sys

import numpy as np
import pytest

import fitness_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -10


def _brute_pcl(pos, tgt, max_range):
    """PCL's loop restated one point at a time: float32 L2_Simple to every finite target, `if (d <= max_range)` in double,
    `fitness_score += d` in double."""
    tgt = [t for t in np.asarray(tgt, np.float32) if np.isfinite(t).all()]
    score, nr = 0.0, 0
    for q in np.asarray(pos, np.float32):
        if not np.isfinite(q).all() or not tgt:
            continue
        best = np.float32(np.inf)
        for t in tgt:
            d = q - t
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            best = min(best, d2)
        if float(best) <= max_range:
            score += float(best)
            nr += 1
    return (score / nr if nr else sys.float_info.max), nr


@pytest.mark.parametrize("kind", ["random", "lattice"])
def test_reference_agrees_with_a_brute_force(kind):
    rng = np.random.default_rng(3)
    if kind == "random":
        tgt = rng.normal(0, 0.5, (300, 3)).astype(np.float32)
        src = rng.normal(0.1, 0.7, (250, 3)).astype(np.float32)
    else:
        tgt = (rng.integers(-40, 40, (300, 3)) * 8 * H).astype(np.float32)
        src = (rng.integers(-400, 400, (250, 3)) * H).astype(np.float32)
    src[5] = np.nan
    src[6, 2] = np.inf
    src[7] = [1e4, -2e3, 7.0]
    tgt[3] = np.nan
    valid = F.finite_rows(src)
    for r in (sys.float_info.max, 0.05, 0.01, 0.0, -1.0):
        want = _brute_pcl(src, tgt, r)
        got = F.fitness(src, tgt, r, valid=valid)
        assert got[1] == want[1]
        if kind == "lattice":
            assert got[0] == want[0]
        else:
            assert got[0] == want[0] or abs(got[0] - want[0]) <= 1e-12 * abs(want[0])
    # the tree path and the brute force give the same bits
    np.testing.assert_array_equal(F.nearest_d2_tree(src, tgt), F.nearest_d2_brute(src, tgt))


def test_tree_path_closes_ties():
    """On a lattice with many equidistant candidates the tree path widens its candidate lists until every row is closed."""
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    tgt = (g * 8 * H).astype(np.float32)
    src = ((g[rng.integers(0, len(g), 2000)] * 8 + rng.choice([-4, 0, 4], (2000, 3))) * H).astype(np.float32)
    np.testing.assert_array_equal(F.nearest_d2_tree(src, tgt, k0=2), F.nearest_d2_brute(src, tgt))


class _FakeStepper:
    def __init__(self, sums):
        self.sums = np.asarray(sums, np.float64)
        self.asked = []

    def fitness_sums(self, max_range):
        self.asked.append(max_range)
        return self.sums


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    import rsreg_amd   # noqa: F401  (the package alias)
    from rsreg_amd import sharded

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(a):
        t = torch.from_numpy(np.array(a, np.float64))
        dist.all_reduce(t)
        return t.numpy()

    blocks = [(3.0, 0.75), (5.0, 1.25)]
    st = _FakeStepper(blocks[rank])
    score, nr = sharded.sharded_fitness_score(st, allreduce, 0.5)
    empty = sharded.sharded_fitness_score(_FakeStepper((0.0, 0.0)), allreduce)
    np.save(os.path.join(out_dir, "r%d.npy" % rank), np.array([score, nr, empty[0], empty[1], st.asked[0]], np.float64))
    dist.destroy_process_group()


def test_sharded_fitness_score_over_gloo(tmp_path):
    torch = pytest.importorskip("torch")
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        score, nr, empty_score, empty_nr, asked = np.load(str(tmp_path / ("r%d.npy" % r)))
        assert nr == 8 and score == 2.0 / 8.0
        assert empty_score == sys.float_info.max and empty_nr == 0
        assert asked == 0.5


def test_sharded_fitness_score_defaults_and_checks():
    sys.path.insert(0, ROOT)
    from rsreg_amd import sharded
    st = _FakeStepper((2.0, 1.0))
    assert sharded.sharded_fitness_score(st, lambda a: a) == (0.5, 2)
    assert st.asked == [sys.float_info.max]
    with pytest.raises(ValueError):
        sharded.sharded_fitness_score(_FakeStepper((1.0, 2.0, 3.0)), lambda a: a)


def test_get_fitness_score_without_a_gpu_raises():
    """Like every other compute call: no CPU fallback, the call raises (and with a GPU, before an align() it raises too)."""
    from rsreg_amd import api, lib
    with pytest.raises(Exception):
        api.IterativeClosestPoint().getFitnessScore()
    with pytest.raises(Exception):
        api.NormalDistributionsTransform().getFitnessScore()
    assert {"rsreg_icp_fitness_score", "rsreg_icp_fitness_sums", "rsreg_ndt_fitness_score"} <= set(lib.EXPORTS)
