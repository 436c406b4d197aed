"""tests/rng_restatement.py, the statement hv_rng_*_batch_dev are compared with, against three independent witnesses: the oracle's
std::mt19937 (oracle.mt19937_draws), the C++ standard's known answer, and the state array of numpy's legacy-seeded MT19937. Plus
the two properties the device kernels lean on: the phased twist equals the serial one, and advances compose. No GPU."""
import numpy as np
import pytest

import rng_restatement as R

SEEDS = (0, 1, 4649, 5489, 0xffffffff)


@pytest.mark.parametrize("seed", SEEDS)
def test_outputs_equal_the_oracle(oracle, seed):
    want = oracle.mt19937_draws(seed, 2000)
    g = R.Mt19937(seed)
    assert np.array_equal(g.draw(2000), want)
    assert g.pos == R.N and g.mt == R.seed_array(seed)                     # draw left the state alone
    assert [g() for _ in range(2000)] == want.tolist()
    # draw at a position inside the array, across more than one twist
    g = R.Mt19937(seed).advance(700)
    assert np.array_equal(g.draw(1300), oracle.mt19937_draws(seed, 1300, skip=700))


def test_known_answer_of_the_standard():
    g = R.Mt19937(5489).advance(9999)
    assert g() == 4123659995
    assert R.Mt19937().draw(3).tolist() == [3499211612, 581869302, 3890346734]


def _numpy_state(seed, k):
    bg = np.random.MT19937()
    bg._legacy_seeding(seed)
    if k:
        bg.random_raw(k)
    st = bg.state["state"]
    return np.asarray(st["key"], np.uint32), int(st["pos"])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("k", (0, 1, 227, 623, 624, 625, 1248, 2000))
def test_state_equals_numpy_legacy_seeding(seed, k):
    mt, pos = R.Mt19937(seed).advance(k).state()
    key, npos = _numpy_state(seed, k)
    assert pos == npos and (1 <= pos <= R.N)
    assert np.array_equal(mt, key)


@pytest.mark.parametrize("seed", SEEDS)
def test_phased_twist_equals_serial_twist_over_four_twists(seed):
    a = b = R.seed_array(seed)
    for _ in range(4):
        a, b = R.twist_serial(a), R.twist_phased(b)
        assert a == b
    # and as the engine's twist: the same stream
    assert np.array_equal(R.Mt19937(seed, twist=R.twist_phased).draw(4 * R.N), R.Mt19937(seed).draw(4 * R.N))
    assert R.PHASE_BEGIN == (0, R.N - R.M, 2 * (R.N - R.M), R.N - 1)


@pytest.mark.parametrize("a,b", [(0, 0), (0, 5), (5, 0), (1, 623), (623, 1), (624, 624), (200, 2048), (1500, 1500), (226, 1), (453, 171)])
def test_advances_compose(a, b):
    one = R.Mt19937(4649).advance(a + b)
    two = R.Mt19937(4649).advance(a).advance(b)
    assert one.mt == two.mt and one.pos == two.pos
    # an advance by 0 is no change at all, also at pos = 624 (no early twist)
    g = R.Mt19937(4649).advance(a)
    before = (list(g.mt), g.pos)
    assert (g.advance(0).mt, g.pos) == before


def test_consumed_clamps():
    assert R.consumed(-3, 2, 200) == 0 and R.consumed(0, 3, 1500) == 0
    assert R.consumed(7, 2, 200) == 14 and R.consumed(100, 2, 200) == 200 and R.consumed(101, 2, 200) == 200
    assert R.consumed(10 ** 9, 3, 2048) == 2048
