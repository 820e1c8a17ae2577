"""GPU: lm_conflict_signal (step 04, conflict minimisation) against a plain Python ordered sum, bit for bit, at the sizes where a
one-thread-per-frame kernel with 64-thread workgroups and a pair loop blocked by eight (5000 pairs: whole blocks; 5003: blocks + tail) can
go wrong; the first 96 random cases of G18 (two per weight combination) and one golden stream through the step script on the real
library."""
import numpy as np
import pytest

import segment_conflict_checks as scc

pytestmark = pytest.mark.gpu

UNIVERSE = 400                                   # frames the random pairs live in
SEGMENTS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (37, 1), (100, 63), (1, 64), (129, 65), (143, 257)]       # (first frame, length)
PAIR_COUNTS = [0, 1, 5000, 5003]            # 5003: the blocked pair loop and its tail in one launch


def random_pairs(n_pairs, seed):
    """gaps of 0..60 frames anywhere in the universe (one in five empty: gap_first > gap_last), alive intervals of 1..150 frames
    anywhere (so for most segments a pair is alive in none, a part or all of it), weights with non-terminating binary fractions"""
    rng = np.random.default_rng(seed)
    gap_first = rng.integers(0, UNIVERSE, n_pairs)
    gap_last = gap_first + rng.integers(0, 61, n_pairs)
    empty = rng.random(n_pairs) < 0.2
    gap_last[empty] = gap_first[empty] - rng.integers(1, 5, int(empty.sum()))
    alive_from = rng.integers(0, UNIVERSE, n_pairs)
    alive_until = alive_from + rng.integers(0, 150, n_pairs)
    weight = rng.integers(1, 1000, n_pairs) / 3.0 * (1.0 - rng.integers(0, 500, n_pairs) / 997.0) + 0.1
    return gap_first.astype(np.int32), gap_last.astype(np.int32), alive_from.astype(np.int32), alive_until.astype(np.int32), weight


def ordered_sum(pairs, start, end):
    """what lm_conflict_signal is defined to return (include/lecturemath_amd.h), one `+=` at a time in list order"""
    acc = [0.0] * (end - start + 1)
    for a, b, alive_from, alive_until, w in zip(*(x.tolist() for x in pairs)):
        if alive_from <= end and alive_until >= start:
            for f in range(max(a, start), min(b, end) + 1):
                acc[f - start] += w
    return np.array(acc, np.float64)


@pytest.fixture(scope="module")
def expected():
    """{n_pairs: (pairs, {segment: ordered sum})}, computed once"""
    out = {}
    for n_pairs in PAIR_COUNTS:
        pairs = random_pairs(n_pairs, seed=n_pairs + 5)
        out[n_pairs] = (pairs, {(s, n): ordered_sum(pairs, s, s + n - 1) for s, n in SEGMENTS})
    return out


@pytest.mark.parametrize("n_pairs", PAIR_COUNTS)
def test_conflict_signal_vs_ordered_sum(hip_lib, expected, n_pairs):
    from lecturemath_amd import device
    pairs, sums = expected[n_pairs]
    cs = device.ConflictSignal(pairs, hip_lib)
    for (start, n), want in sums.items():
        got = cs.signal(start, start + n - 1)
        assert got.dtype == np.float64 and got.shape == (n,)
        assert (got.view(np.int64) == want.view(np.int64)).all(), (n_pairs, start, n)
    if n_pairs == 5000:
        want = sums[(143, 257)]
        alive = (pairs[2] <= 399) & (pairs[3] >= 143)
        assert 0 < alive.sum() < n_pairs and (pairs[0] > pairs[1]).sum() > 500          # dead pairs, live pairs, empty gaps
        assert (want != np.round(want)).any() and len(set(want.tolist())) > 100
        # the comparison can tell an ordered sum from a reordered one: the same pairs summed backwards give other bits
        backwards = ordered_sum(tuple(x[::-1] for x in pairs), 143, 399)
        assert (backwards.view(np.int64) != want.view(np.int64)).any() and np.allclose(backwards, want, rtol=1e-12)
    elif n_pairs == 0:
        assert all((w == 0.0).all() for w in sums.values())


def test_first_96_random_cases(hip_lib):
    g = scc.cases()
    assert sorted(tuple(int(v) for v in c) for c in g["combo"][:96]) == sorted(scc.COMBOS * 2)
    scc.check_cases(hip_lib, range(96))


def test_script_on_golden_stream(hip_lib):
    assert scc.check_script_stream(hip_lib, "occluder_return") == 4
