"""Literal restatement of libstdc++'s std::mt19937 = mersenne_twister_engine<uint32_t, 32, 624, 397, 31, 0x9908b0df, 11, 0xffffffff, 7,
0x9d2c5680, 15, 0xefc60000, 18, 1812433253> (bits/random.tcc: seed, _M_gen_rand, operator()) in the stored form of hv_rng
(include/hybvio_hip.h): `mt` is the array of the last twist, `pos` the number of its words already handed out. The engine is lazy:
it twists only when an output needs a word that is not there, so pos is 624 after seeding and 1 .. 624 after any output.

draw(n) and advance(c) are the two device entries (hv_rng_draw_batch_dev leaves the state alone, hv_rng_advance_batch_dev moves
it); twist_phased is the schedule of hybvio_amd/csrc/hv_mt19937.hpp as a separate function: three ranges whose words are computed
from a snapshot (all reads of a phase before its writes), then the last word. Plain Python integers; no GPU."""
import numpy as np

N, M = 624, 397
UPPER, LOWER, MATRIX_A = 0x80000000, 0x7fffffff, 0x9908b0df
MASK = 0xffffffff
PHASE_BEGIN = (0, 227, 454, 623)


def seed_array(seed):
    mt = [seed & MASK]
    for i in range(1, N):
        x = mt[i - 1] ^ (mt[i - 1] >> 30)
        mt.append((1812433253 * x + i) & MASK)
    return mt


def f(cur, nxt):
    y = (cur & UPPER) | (nxt & LOWER)
    return (y >> 1) ^ (MATRIX_A if y & 1 else 0)


def temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9d2c5680
    y ^= (y << 15) & 0xefc60000
    y ^= y >> 18
    return y & MASK


def twist_serial(mt):
    """_M_gen_rand: in place, ascending, so word i sees the new mt[i + M - N] from i = N - M on."""
    mt = list(mt)
    for k in range(N - M):
        mt[k] = mt[k + M] ^ f(mt[k], mt[k + 1])
    for k in range(N - M, N - 1):
        mt[k] = mt[k + M - N] ^ f(mt[k], mt[k + 1])
    mt[N - 1] = mt[M - 1] ^ f(mt[N - 1], mt[0])
    return mt


def twist_phased(mt):
    """The parallel schedule: the words of a phase are all computed from the array as the phase finds it, then all written."""
    mt = list(mt)
    for ph in range(3):
        snap = list(mt)
        for i in range(PHASE_BEGIN[ph], PHASE_BEGIN[ph + 1]):
            mt[i] = snap[(i + M) % N] ^ f(snap[i], snap[i + 1])
    mt[N - 1] = mt[M - 1] ^ f(mt[N - 1], mt[0])
    return mt


class Mt19937:
    """The engine in the form hv_rng stores. twist: the twist function used (serial by default)."""

    def __init__(self, seed=5489, twist=twist_serial):
        self.mt, self.pos, self.twist = seed_array(seed), N, twist

    def copy(self):
        g = Mt19937.__new__(Mt19937)
        g.mt, g.pos, g.twist = list(self.mt), self.pos, self.twist
        return g

    def __call__(self):
        """operator(): one output."""
        if self.pos >= N:
            self.mt, self.pos = self.twist(self.mt), 0
        y = self.mt[self.pos]
        self.pos += 1
        return temper(y)

    def draw(self, n):
        """The next n outputs as uint32; the state is not changed."""
        g = self.copy()
        return np.array([g() for _ in range(n)], np.uint32)

    def advance(self, c):
        """c further calls of operator(). c = 0 changes nothing; after c > 0, pos is in 1 .. 624."""
        for _ in range(c):
            self()
        return self

    def state(self):
        """(mt [624] uint32, pos) as hv_rng holds them."""
        return np.array(self.mt, np.uint32), self.pos


def consumed(count, multiplier, max_draws):
    """The number of outputs hv_rng_advance_batch_dev moves a set by."""
    return min(multiplier * min(max(int(count), 0), max_draws), max_draws)
