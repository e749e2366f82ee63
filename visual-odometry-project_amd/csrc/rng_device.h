// NumPy's PCG64 (XSL-RR 128/64) and the sample derivation of Generator.choice(n, 8, replace=False) as host + device
// functions: the fill kernel and the raw-reading hypothesis kernel of the 8-point RANSAC (bootstrap.hip) and the host
// entry points that pin them to NumPy's stream (ransac_host.hip: vo_rng_choice8_from_raw) share this text.
#pragma once
#include <cstdint>

#include "vo_hip.h"

namespace vo_rng {

typedef unsigned __int128 u128;

__host__ __device__ inline u128 make128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }

__host__ __device__ inline u128 pcg_mult() { return make128(2549297995355413924ULL, 4865540595714422341ULL); }

// the state `delta` steps of state <- state * mult + inc further on (the LCG's skip-ahead: O(log delta) 128-bit products)
__host__ __device__ inline u128 pcg_advance(u128 state, u128 inc, uint64_t delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = inc;
  for (int bit = 0; bit < 64 && delta != 0; ++bit) {
    if (delta & 1ull) {
      acc_mult = acc_mult * cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult = cur_mult * cur_mult;
    delta >>= 1;
  }
  return acc_mult * state + acc_plus;
}

// XSL-RR: the 64-bit output of a state (NumPy steps the state first and outputs the new one)
__host__ __device__ inline uint64_t pcg_output(u128 state) {
  const uint64_t v = (uint64_t)(state >> 64) ^ (uint64_t)state;
  const unsigned r = (unsigned)(state >> 122);
  return (v >> r) | (v << ((64u - r) & 63u));
}

// Word p of the generator's 32-bit stream as Generator draws it from *g: a buffered half first, then every 64-bit
// output low half, high half.
__host__ __device__ inline uint32_t pcg_word(const vo_pcg64& g, uint64_t p) {
  const uint64_t off = g.has_uint32 ? 1u : 0u;
  if (p < off) return g.uinteger;
  const uint64_t q = p - off;
  const uint64_t o = pcg_output(pcg_advance(make128(g.state_hi, g.state_lo), make128(g.inc_hi, g.inc_lo), (q >> 1) + 1));
  return (q & 1) ? (uint32_t)(o >> 32) : (uint32_t)o;
}

// *g after `words` 32-bit draws (host and device agree with vo_rng_raw32 / NumPy's next_uint32 on every field)
__host__ __device__ inline void pcg_skip_words(vo_pcg64* g, uint64_t words) {
  if (words == 0) return;
  if (g->has_uint32) {
    g->has_uint32 = 0;
    --words;
    if (words == 0) return;      // (NumPy leaves the spent half in `uinteger`)
  }
  const uint64_t outs = (words + 1) >> 1;
  const u128 s = pcg_advance(make128(g->state_hi, g->state_lo), make128(g->inc_hi, g->inc_lo), outs);
  g->state_hi = (uint64_t)(s >> 64);
  g->state_lo = (uint64_t)s;
  g->uinteger = (uint32_t)(pcg_output(s) >> 32);
  g->has_uint32 = (words & 1) ? 1u : 0u;
}

// NumPy's bounded draw (Lemire, 32-bit) on ONE output of the generator.  `risky` is raised when the draw could have been
// rejected -- the sequential generator might have consumed one more output than a position-based view assumes.
__host__ __device__ inline uint32_t bounded_from_raw(uint32_t raw, uint32_t rng, bool& risky) {
  const uint32_t rex = rng + 1u;
  const uint64_t m = (uint64_t)raw * rex;
  if ((uint32_t)m < rex) risky = true;
  return (uint32_t)(m >> 32);
}

constexpr int CHOICE8_RAWS = 15;      // outputs one sample consumes when none of its draws is rejected

// Generator.choice(pop, 8, replace=False) from the 15 outputs a sample consumes when no draw is rejected: eight bounded
// draws (Floyd, upper ends pop-8 .. pop-1; a value met before is replaced by the upper end) and seven for the shuffle
// (upper ends 7 .. 1).  pop >= 9: at pop = 8 the first draw has range 0 and NumPy consumes no output for it.
// Returns true when one of the draws could have been rejected.  No indexing by a run-time value: the kernel keeps the
// sample in registers.
__host__ __device__ inline bool choice8_from_raw(const uint32_t (&raw)[CHOICE8_RAWS], uint32_t pop, int32_t (&v)[8]) {
  bool risky = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t j = pop - 8u + (uint32_t)k;
    const int32_t val = (int32_t)bounded_from_raw(raw[k], j, risky);
    bool seen = false;
#pragma unroll
    for (int q = 0; q < k; ++q) seen |= (v[q] == val);
    v[k] = seen ? (int32_t)j : val;
  }
#pragma unroll
  for (int i = 7; i >= 1; --i) {
    const int j = (int)bounded_from_raw(raw[8 + (7 - i)], (uint32_t)i, risky);
    int32_t vj = v[0];
#pragma unroll
    for (int q = 1; q <= i; ++q) vj = (j == q) ? v[q] : vj;
    const int32_t vi = v[i];
#pragma unroll
    for (int q = 0; q <= i; ++q)
      if (q == j) v[q] = vi;
    v[i] = vj;
  }
  return risky;
}

}  // namespace vo_rng
