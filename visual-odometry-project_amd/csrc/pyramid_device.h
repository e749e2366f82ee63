// The bordered image pyramid as pyramid.hip builds it and klt.hip reads it: the level table a kernel takes, and where a
// level sits in a sequence's pyramid buffer.
#pragma once
#include "vo_internal.h"

namespace {

constexpr int MAX_LEVELS = 8;

// Every level (level 0 included) is kept with PYR_PAD pixels of reflect-101 border on all
// sides, so the row tracker's blocks -- which reach at most WIN + 4 pixels past an edge, WIN <= 21
// -- are plain in-bounds reads.  prev/next point at the interior origin of each level.
constexpr int PYR_PAD = 32;

struct pyr_t {
  const uint8_t* prev[MAX_LEVELS];
  const uint8_t* next[MAX_LEVELS];
  int H[MAX_LEVELS], W[MAX_LEVELS], pitch[MAX_LEVELS];
  int n_levels;
};

__host__ __device__ inline int pyr_pitch(int W) { return (W + 2 * PYR_PAD + 3) & ~3; }
inline size_t pyr_level_bytes(int H, int W) {
  return ((size_t)(H + 2 * PYR_PAD) * pyr_pitch(W) + 255) & ~size_t(255);
}

__device__ __forceinline__ int reflect101(int c, int n) {
  if (n == 1) return 0;
  while (c < 0 || c >= n) c = (c < 0) ? -c : 2 * (n - 1) - c;
  return c;
}

}  // namespace
