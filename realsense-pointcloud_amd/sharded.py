"""One cloud pair registered by N ranks: the source is cut into blocks dealt to the ranks, the target
(and its index) is replicated, and the only exchange per iteration is the sum of the 17
per-block sums (BASELINE configs[3]).  Every rank then runs the same host
Umeyama/SVD on identical numbers, so all ranks hold the same transform without a broadcast.

The reference has no distributed path; this module is new work.  Two transports:
  * native: ``Context.comm_init`` + ``rsreg_icp_align`` all-reduces on the device over RCCL
    (what bench.py uses on a multi-GPU node);
  * step-wise: ``run_sharded_icp`` below drives begin/search/sums/update and leaves the
    all-reduce to a callable (torch.distributed with gloo or nccl, or RCCL via the ctx).
"""
import numpy as np


def shard_range(n, rank, world):
    """Contiguous block [lo, hi) of rank `rank` when n items are cut into `world` blocks."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    return (n * rank) // world, (n * (rank + 1)) // world


def shard_blocks(n, rank, world, block=256):
    """Indices of rank `rank` when n items are cut into blocks of `block` consecutive items and
    the blocks are dealt round-robin.  Same exchange as `shard_range` (the sums do not care which
    points a rank holds), but every rank gets an even sample of the scene: the slow waves of a
    launch (queries on near, densely sampled surfaces) are spread over all ranks instead of
    landing on the one that owns that part of the image."""
    if world < 1 or not (0 <= rank < world) or block < 1:
        raise ValueError("bad rank/world/block")
    idx = np.arange(n, dtype=np.int64)
    return idx[(idx // block) % world == rank]


def filters_on(params):
    """Whether ICP parameters turn a correspondence filter on: rsreg_icp_params, or a stepper's own with `use_reciprocal`."""
    if params is None:
        return False
    recip = getattr(params, "use_reciprocal_correspondences", getattr(params, "use_reciprocal", 0))
    ratio = float(getattr(params, "trim_overlap_ratio", 0.0))
    return bool(recip) or 0.0 < ratio < 1.0


def run_sharded_icp(stepper, allreduce, guess=None, max_steps=100000):
    """Drive one ICP alignment whose sums are combined across ranks.

    stepper   : an object with begin(guess) / search() / sums() / update(sums) / end() — the
                step-wise form of ``api.IterativeClosestPoint`` holding THIS rank's source block.
    allreduce : callable(np.ndarray[17] float64) -> the element-wise sum over all ranks.
    Returns the result of stepper.end().  All ranks take the same number of iterations because
    they evaluate the convergence criteria on the same (global) sums.
    The correspondence filters (reciprocal correspondences, the trimmed rejector) are refused: each rank would filter
    its own block (its own cut, a reciprocal index of its own points), not what one GPU computes.
    """
    if filters_on(getattr(stepper, "params", None)):
        raise ValueError("run_sharded_icp: reciprocal correspondences and the trimmed rejector need the whole source; "
                         "a sharded alignment cannot use them")
    stepper.begin(guess)
    for _ in range(max_steps):
        stepper.search(False) if getattr(stepper, "_quiet_search", False) else stepper.search()
        local = np.ascontiguousarray(stepper.sums(), np.float64)
        total = np.ascontiguousarray(allreduce(local), np.float64)
        _, done = stepper.update(total)
        if done:
            break
    return stepper.end()


def sharded_fitness_score(stepper, allreduce, max_range=None):
    """Registration::getFitnessScore(max_range) of a sharded alignment (after ``run_sharded_icp``): every rank's
    (count, sum of d^2) over its own source block, element-wise summed by ``allreduce`` as the 17 sums are.

    stepper   : an object with fitness_sums(max_range) -> np.ndarray[2] float64 (this rank's count, sum of d^2): the
                ``api.IterativeClosestPoint`` that ran this rank's block (rsreg_icp_fitness_sums, never all-reduced).
    allreduce : callable(np.ndarray[2] float64) -> the element-wise sum over all ranks.
    max_range : compared with the SQUARED distance, as in PCL; None: unbounded (sys.float_info.max).
    Returns (score, records in range); the score is sys.float_info.max when no record of any rank is in range.
    """
    import sys

    if max_range is None:
        max_range = sys.float_info.max
    local = np.ascontiguousarray(stepper.fitness_sums(max_range), np.float64)
    if local.shape != (2,):
        raise ValueError("fitness_sums must return two numbers (count, sum of d^2)")
    total = np.ascontiguousarray(allreduce(local), np.float64)
    count = int(round(float(total[0])))
    return (float(total[1]) / float(total[0]) if total[0] > 0 else sys.float_info.max), count
