// The arithmetic of std::mt19937 = mersenne_twister_engine<uint32_t, 32, 624, 397, 31, 0x9908b0df, 11, 0xffffffff, 7, 0x9d2c5680, 15,
// 0xefc60000, 18, 1812433253> (libstdc++ bits/random.tcc), written once: the seed step, the twist function, the tempering, and the
// schedule that lets 64 lanes run one twist in three phases plus one word (rng.hip). Plain C++: no HIP header, so a
// host compiler alone can build it (tests/cpp/test_mt19937_schedule.cpp).
#pragma once
#include <stdint.h>

#ifndef HV_HD
#if defined(__HIPCC__)
#define HV_HD __host__ __device__ __attribute__((always_inline))
#else
#define HV_HD
#endif
#endif

namespace hv {
namespace mt {

constexpr int N = 624, M = 397;                                  // state words; the word M ahead enters the twist of a word
constexpr uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MATRIX_A = 0x9908b0dfu;

// mt[i] of the seeding from mt[i - 1] (mt[0] = the seed)
HV_HD inline uint32_t seed_step(uint32_t prev, int i) { return 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i; }

// what the twist xors onto the word M ahead: the top bit of one word and the low 31 of the next, times the matrix A
HV_HD inline uint32_t f(uint32_t cur, uint32_t next)
{
    const uint32_t y = (cur & UPPER) | (next & LOWER);
    return (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
}

HV_HD inline uint32_t temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// ---- one twist in parallel ----
// New mt[i] = mt[(i + M) % N] ^ f(mt[i], mt[i + 1]). The serial loop runs i upwards, so word i sees the OLD mt[i], mt[i + 1] and, from
// i = N - M on, the NEW mt[i + M - N]. Three ranges of at most N - M words cut that chain: inside a range every operand is either old
// or was written by an earlier range, so the words of a range are independent once all of them have been read before any is written.
//   phase 0: i in [0, 227)    mt[i + 397] old
//   phase 1: i in [227, 454)  mt[i - 227] written by phase 0
//   phase 2: i in [454, 623)  mt[i - 227] written by phase 1
//   last:    i = 623          mt[396] written by phase 1, mt[0] by phase 0 (the only word whose `next` operand is new)
// mt[i + 1] of the last word of a phase belongs to the next phase and is still old when the phase reads it.
constexpr int PHASES = 3;
constexpr int PHASE_BEGIN[PHASES + 1] = {0, N - M, 2 * (N - M), N - 1};      // 0 | 227 | 454 | 623
static_assert(PHASE_BEGIN[1] == 227 && PHASE_BEGIN[2] == 454 && PHASE_BEGIN[3] == 623, "phase bounds of (624, 397)");
static_assert(PHASE_BEGIN[3] - PHASE_BEGIN[2] <= N - M && 3 * (N - M) >= N - 1, "three ranges of at most N - M words reach word N - 2");

// the new word i < N - 1 from the array as its phase finds it
HV_HD inline uint32_t twist_word(const uint32_t *mt, int i)
{
    const int j = i + M < N ? i + M : i + M - N;
    return mt[j] ^ f(mt[i], mt[i + 1]);
}
// the new word N - 1, after the three phases
HV_HD inline uint32_t twist_last(const uint32_t *mt) { return mt[M - 1] ^ f(mt[N - 1], mt[0]); }

// ---- the lazy, canonical state ----
// pos = words of mt already handed out, 1 .. 624 after any output, 624 after seeding: the engine twists only when an output needs a
// word that is not there. Outputs pos .. pos + n - 1 (counted from the current array's word 0) therefore need this many twists:
HV_HD inline int twists_for(int pos, int n) { return n > 0 ? (pos + n + N - 1) / N - 1 : 0; }

}  // namespace mt
}  // namespace hv
