"""Model check of the corner / flat selection the HIP kernel performs (a-loam_amd/csrc/registration_kernels.hip,
pick_sector + the second pass of k_ring_features).

The reference sorts every sector by curvature and walks it, skipping points already marked by earlier picks — marks that
spill over sector borders, so its six sectors are inherently sequential (src/scanRegistration.cpp:284-390).  The kernel
runs the six sectors concurrently WITHOUT the incoming marks (iterative arg-max / arg-min instead of a sort) and afterwards
redoes, in order, only the sectors that picked a point the sectors before them had marked.  This file runs that scheme as a
Python model against the literal sequential definition over thousands of random rings — ties in curvature, gaps that cut the
neighbour suppression short, sectors shorter than the suppression reach — so the soundness of the speculation does not rest
on the handful of sweeps the GPU tests see."""
import numpy as np
import pytest

from selection_model import INF, THR, literal, model, pick_sector, pick_sector_regs

F = np.float32


@pytest.mark.parametrize("seed", range(8))
def test_speculative_sector_selection_equals_the_sequential_walk(seed):
    rng = np.random.default_rng(100 + seed)
    for trial in range(250):
        n = int(rng.choice([17, 18, 20, 23, 29, 35, 41, 47, 60, 90, 150, 400]))
        style = trial % 4
        if style == 0:   curv = rng.exponential(0.2, n)
        elif style == 1: curv = rng.choice([0.0, 0.05, 0.1, 0.2, 1.0], n)                   # massive ties, values on the thresholds
        elif style == 2: curv = np.where(rng.random(n) < 0.5, rng.uniform(0.11, 3, n), rng.uniform(0, 0.09, n))
        else:            curv = np.round(rng.exponential(0.3, n), 1)
        curv = curv.astype(np.float32)
        gap = rng.random(n) < rng.choice([0.0, 0.05, 0.3, 0.8])
        la, pa = literal(curv, gap, n)
        lb, pb = model(curv, gap, n)
        assert np.array_equal(la, lb) and pa == pb, (seed, trial, n, curv.tolist(), gap.tolist(), pa, pb)


@pytest.mark.parametrize("W", [16, 32, 64])
def test_register_level_selection_equals_the_sequential_walk(W):
    """The loop the kernel runs (keys with "dead" folded in, integer thresholds, lane-range kills through register kr and its
    neighbours) against the reference's literal walk, with register borders every 16 / 32 / 64 points."""
    rng = np.random.default_rng(700 + W)
    sizes = [17, 23, 41, 90, 150, 400, 700] if W < 64 else [41, 150, 400, 900, 2059]
    for trial in range(120 if W < 64 else 40):
        n = int(rng.choice(sizes))
        style = trial % 4
        if style == 0:   curv = rng.exponential(0.2, n)
        elif style == 1: curv = rng.choice([0.0, 0.05, 0.1, 0.2, 1.0], n)
        elif style == 2: curv = np.where(rng.random(n) < 0.5, rng.uniform(0.11, 3, n), rng.uniform(0, 0.09, n))
        else:            curv = np.round(rng.exponential(0.3, n), 1)
        curv = curv.astype(np.float32)
        gap = rng.random(n) < rng.choice([0.0, 0.05, 0.3, 0.8])
        la, pa = literal(curv, gap, n)
        lb, pb = model(curv, gap, n, lambda *a: pick_sector_regs(*a, W=W, spare=trial % 2))
        assert np.array_equal(la, lb) and pa == pb, (W, trial, n)


def test_curvature_thresholds_as_integer_compares():
    """`(double)c > 0.1` == `THR <= bits(c) <= bits(inf)` and `(double)c < 0.1` == `bits(c) < THR` for every non-negative float."""
    rng = np.random.default_rng(5)
    bits = np.concatenate([np.arange(THR - 4096, THR + 4096), rng.integers(0, 0x7f800000, 200000), [0, 1, INF - 1, INF, INF + 1, 0x7fc00000, 0x7fffffff]]).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        c = bits.view(np.float32).astype(np.float64)
        assert np.array_equal(c > 0.1, (bits >= THR) & (bits <= INF))
        assert np.array_equal(c < 0.1, bits < THR)


def test_reach_from_the_gap_bit_window():
    """k_ring_features keeps "step s -> s + 1 is longer than the threshold" as one bit per step (bit s + 64 of an array whose first
    word and whose steps >= n - 1 read 1) and takes the reach of the neighbour suppression around point i from the 10-bit window
    of steps i - 5 .. i + 4: fw = ctz(window >> 5 | 32), bk = ctz(bitreverse(window << 27) | 32).  Against the literal loops
    (reference src/scanRegistration.cpp:316-341: stop at the first long step, at most 5, inside the ring)."""
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 700))
        gap = rng.random(n) < rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        padded = ((n + 255) // 256) * 256                                  # the kernel ballots whole chunks of 256 steps
        bits = np.ones(64 + padded + 64, np.uint8)
        bits[64:64 + n - 1] = gap[:n - 1]                                  # steps 0 .. n - 2 exist
        words = np.packbits(bits, bitorder="little").view(np.uint32)
        for i in range(n):
            bit = i + 59
            lo, hi = int(words[bit >> 5]), int(words[(bit >> 5) + 1])
            win = (((hi << 32) | lo) >> (bit & 31)) & 0xffffffff           # v_alignbit_b32
            ctz = lambda x: (x & -x).bit_length() - 1
            brev = lambda x: int(format(x & 0xffffffff, "032b")[::-1], 2)
            fw = ctz((win >> 5) | 32)
            bk = ctz(brev((win << 27) & 0xffffffff) | 32)
            fw_ref = bk_ref = 0
            while fw_ref < 5 and i + fw_ref < n - 1 and not gap[i + fw_ref]: fw_ref += 1
            while bk_ref < 5 and i - 1 - bk_ref >= 0 and not gap[i - 1 - bk_ref]: bk_ref += 1
            assert (fw, bk) == (fw_ref, bk_ref), (trial, n, i)
