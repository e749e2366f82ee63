// The window join: the landmarks of the newest of W observation records (track_record_device.h) and their observations in the
// W - 1 older ones, as the arrays vo_window_ba_dev / vo_window_structure_dev take.  window_build_kernel (window_ba.hip) and
// sl_join_kernel (structure_loop.hip) both run vo_window_emit; they differ in how a row of an older record is found.
//
// One workgroup of T threads.  Thread t owns the rows t run .. t run + run - 1 of the newest record (run = ceil(n / T)), counts
// its landmarks and their observations, and an exclusive scan over the T threads (wave scan by shuffles, the wave totals
// through LDS) gives (l, o): how many landmarks and observations lie before its run IN ROW ORDER.  A landmark is kept iff
// l < L_cap and o + c <= M_cap; both grow along the rows, so what is kept is a prefix, and the first landmark left out names
// what cut the list.  The finder is called twice per row (count, then write) instead of its answers being kept in a
// per-thread array: no scratch.
#pragma once
#include "track_record_device.h"

template <int T>
struct vo_window_lds {
  int wl[T / 64], wo[T / 64];     // the waves' landmark / observation counts
  int tot[3];                     // what the join leaves: landmarks kept, observations kept, flags (1: L_cap cut, 2: M_cap cut)
};

// rec_of(s): the record of age s (0: the oldest, W - 1: the newest).  find(s, id, r), s < W - 1: the first row of that record
// that carries `id`, the id of row r of the newest, or -1.  X0 (the window's input once more) and lm_of_row (row of the
// newest record -> its landmark, -1: none) are optional.  All T threads call it; behind it sh.tot is complete for every one
// of them (the caller has not touched sh).
template <int T, class RecOf, class Find>
__device__ __forceinline__ void vo_window_emit(vo_window_lds<T>& sh, int W, int cap, int L_cap, int M_cap, RecOf rec_of, Find find,
                                               int32_t* __restrict__ lm_id, double* __restrict__ X, double* __restrict__ X0,
                                               int32_t* __restrict__ lm_start, int32_t* __restrict__ obs_slot,
                                               double* __restrict__ obs_xy, int32_t* __restrict__ lm_of_row) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const vo_track::word* const newest = rec_of(W - 1);
  const int n_new = vo_track::rows(newest, cap);
  const int run = (n_new + T - 1) / T;
  const int r0 = min(tid * run, n_new), r1 = min(r0 + run, n_new);
  // observations of row r as a landmark, 0 when it is none (the newest record's own row counts as one)
  auto n_obs = [&](int r) {
    const vo_track::word* row = vo_track::row(newest, r);
    if (vo_track::row_state(row) != 2) return 0;
    const double X0 = vo_track::row_landmark(row, 0), X1 = vo_track::row_landmark(row, 1), X2 = vo_track::row_landmark(row, 2);
    if (!(isfinite(X0) && isfinite(X1) && isfinite(X2))) return 0;
    const int id = vo_track::row_id(row);
    int c = 1;
    for (int s = 0; s < W - 1; ++s) c += find(s, id, r) >= 0 ? 1 : 0;
    return c >= 2 ? c : 0;
  };
  int nl = 0, no = 0;
  for (int r = r0; r < r1; ++r) {
    const int c = n_obs(r);
    nl += c > 0 ? 1 : 0;
    no += c;
  }
  // exclusive scan of (nl, no) in thread order
  int il = nl, io = no;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int tl = __shfl_up(il, off), to = __shfl_up(io, off);
    if (lane >= off) {
      il += tl;
      io += to;
    }
  }
  if (lane == 63) {
    sh.wl[wv] = il;
    sh.wo[wv] = io;
  }
  if (tid == 0) sh.tot[0] = sh.tot[1] = sh.tot[2] = 0;
  __syncthreads();
  int l = il - nl, o = io - no;
  for (int w = 0; w < wv; ++w) {
    l += sh.wl[w];
    o += sh.wo[w];
  }
  int kept_l = 0, kept_o = 0, cut = 0;
  for (int r = r0; r < r1; ++r) {
    const int c = n_obs(r);
    int mine = -1;
    if (c > 0) {
      if (l >= L_cap || o + c > M_cap) {
        // the flag names what ended the list: only the first landmark left out sets it (the one before it was kept)
        if (l == 0 || (l - 1 < L_cap && o <= M_cap)) cut |= l >= L_cap ? 1 : 2;
      } else {
        const vo_track::word* row = vo_track::row(newest, r);
        const int id = vo_track::row_id(row);
        lm_id[l] = id;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double v = vo_track::row_landmark(row, k);
          X[3 * (size_t)l + k] = v;
          if (X0) X0[3 * (size_t)l + k] = v;
        }
        lm_start[l] = o;
        lm_start[l + 1] = o + c;                 // (the next landmark writes the same value)
        int k = o;
        for (int s = 0; s < W; ++s) {            // ascending slot
          const int m = s == W - 1 ? r : find(s, id, r);
          if (m < 0) continue;
          const vo_track::word* seen = vo_track::row(rec_of(s), m);
          const float x = vo_track::row_x(seen), y = vo_track::row_y(seen);
          obs_slot[k] = s;
          obs_xy[2 * (size_t)k] = (double)x;
          obs_xy[2 * (size_t)k + 1] = (double)y;
          ++k;
        }
        mine = l;
        ++kept_l;
        kept_o += c;
      }
      ++l;
      o += c;
    }
    if (lm_of_row) lm_of_row[r] = mine;
  }
  if (kept_l) {
    atomicAdd(&sh.tot[0], kept_l);
    atomicAdd(&sh.tot[1], kept_o);
  }
  if (cut) atomicOr(&sh.tot[2], cut);
  __syncthreads();
  if (tid == 0 && sh.tot[0] == 0) lm_start[0] = 0;
}
