// The observation record of one step (vo_hip.h, "Track ids"): the one definition of its layout.
//
// A record is a run of 8-byte words: a header of two, {n | step, next_id | seq}, then one row of six per feature,
// {id | born, x | y (float bits), state | cand, X, Y, Z (doubles, NaN unless the state is 2)}; "a | b" is a in the low and b
// in the high half of a word.  export_tracks_kernel (pipeline_state.hip) and sl_record_kernel (structure_loop.hip) write it
// through the two writers below; the window joins (window_join_device.h) and the loop's header check read it through the
// accessors.  vo/_pipeline.py (TRACK_HEADER, TRACK_ROW) is the host's view of the same bytes.
#pragma once
#include "state_device.h"

namespace vo_track {

typedef unsigned long long word;

constexpr int HEADER_WORDS = 2;
constexpr int ROW_WORDS = 6;

// 8-byte words of a record of `cap` rows
__host__ __device__ inline size_t record_words(int cap) { return (size_t)HEADER_WORDS + (size_t)ROW_WORDS * (size_t)(cap > 0 ? cap : 0); }

__host__ __device__ inline word pack(int lo, int hi) { return (word)(unsigned)lo | ((word)(unsigned)hi << 32); }
__host__ __device__ inline int lo32(word w) { return (int)(unsigned)(w & 0xffffffffull); }
__host__ __device__ inline int hi32(word w) { return (int)(unsigned)(w >> 32); }

// ---- the header ----
__device__ __forceinline__ int rows(const word* rec, int cap) { return max(0, min(lo32(rec[0]), cap)); }     // n, clamped
__device__ __forceinline__ int step(const word* rec) { return hi32(rec[0]); }
__device__ __forceinline__ int next_id(const word* rec) { return lo32(rec[1]); }

// ---- a row ----
__device__ __forceinline__ const word* row(const word* rec, int r) { return rec + HEADER_WORDS + (size_t)ROW_WORDS * r; }
__device__ __forceinline__ int row_id(const word* row) { return lo32(row[0]); }
__device__ __forceinline__ float row_x(const word* row) { return __int_as_float(lo32(row[1])); }
__device__ __forceinline__ float row_y(const word* row) { return __int_as_float(hi32(row[1])); }
__device__ __forceinline__ int row_state(const word* row) { return lo32(row[2]); }
__device__ __forceinline__ double row_landmark(const word* row, int k) { return __longlong_as_double((long long)row[3 + k]); }

// ---- the writers ----
__device__ __forceinline__ void write_header(word* rec, int n, int step, int next_id, int seq) {
  rec[0] = pack(n, step);
  rec[1] = pack(next_id, seq);
}

// row i from feature i of F; returns the row's id
__device__ __forceinline__ int write_row(word* rec, const vo_feat& F, int i) {
  const int2 id = F.ids[i];
  const float x = F.kp[2 * i], y = F.kp[2 * i + 1];
  const int st = F.state[i], cd = F.cand[i];
  double X[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = F.land[3 * i + k];
  word* row = rec + HEADER_WORDS + (size_t)ROW_WORDS * i;
  row[0] = pack(id.x, id.y);
  row[1] = pack(__float_as_int(x), __float_as_int(y));
  row[2] = pack(st, cd);
#pragma unroll
  for (int k = 0; k < 3; ++k) row[3 + k] = (word)__double_as_longlong(st == 2 ? X[k] : vo_state_dev::dnan());
  return id.x;
}

}  // namespace vo_track
