// SPDX-License-Identifier: MIT
// Work split of the variable-length message kernels — single definition
// shared by the GPU kernels (p2p_kernels.hip) and plain g++ tests, so
// the CPU tier walks a batch with the very code a wave runs.
//
// Message m has lens[m] bytes and therefore ceil(lens[m] / 4096) chunks
// (the last one may be partial; a zero-length message has none).  Chunks
// are numbered message-major: cstart[m] = sum of the chunk counts of the
// messages before m, cstart[n] = the total.  A wave owns the contiguous
// chunks [c0, c1): it finds the message of c0 with one binary search
// (rocp2p_vl_seek) and from there only steps forward (rocp2p_vl_next).
#pragma once
#ifdef __cplusplus
#include <cstdint>
#else
#include <stdbool.h>
#include <stdint.h>
#endif

#include "p2p_pattern.h"  // ROCP2P_HD

#define ROCP2P_VL_CHUNK 4096u

// chunks of a message of len bytes (no overflow for any len)
ROCP2P_HD uint64_t rocp2p_vl_chunks(uint64_t len) {
  return len / ROCP2P_VL_CHUNK + (len % ROCP2P_VL_CHUNK != 0);
}

// Chunks [c0, c1) of wave number `wave` when `nwaves` waves share
// `total` chunks in equal contiguous runs.  Waves past the end get an
// empty run (c0 == c1 == total).
ROCP2P_HD void rocp2p_vl_run(uint64_t total, uint64_t nwaves, uint64_t wave,
                             uint64_t* c0, uint64_t* c1) {
  const uint64_t run = total / nwaves + (total % nwaves != 0);
  // wave * run cannot overflow: (nwaves - 1) * run < total + nwaves
  uint64_t b = wave * run;
  if (b > total) b = total;
  *c0 = b;
  *c1 = (total - b < run) ? total : b + run;
}

// Where a wave stands: chunk ci of the cpm chunks of message m, which
// is len bytes long.
typedef struct rocp2p_vl_cursor {
  uint64_t m, ci, cpm, len;
} rocp2p_vl_cursor;

// The message that owns chunk c, c < cstart[n]: the one m with
// cstart[m] <= c < cstart[m + 1].  Zero-length messages have
// cstart[m] == cstart[m + 1] and are never the answer.
ROCP2P_HD uint64_t rocp2p_vl_find(const uint64_t* cstart, uint64_t n,
                                  uint64_t c) {
  uint64_t lo = 0, hi = n;  // answer in [lo, hi); cstart[lo] <= c < cstart[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (cstart[mid] <= c)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Put the cursor on chunk c (c < cstart[n]).
ROCP2P_HD void rocp2p_vl_seek(rocp2p_vl_cursor* cur, const uint64_t* cstart,
                              const uint64_t* lens, uint64_t n, uint64_t c) {
  const uint64_t m = rocp2p_vl_find(cstart, n, c);
  const uint64_t first = cstart[m];
  cur->m = m;
  cur->ci = c - first;
  cur->cpm = cstart[m + 1] - first;
  cur->len = lens[m];
}

// Step to the next chunk; only legal while another chunk exists (the
// chunk just done was not cstart[n] - 1), which also bounds the walk
// over zero-length messages.  Returns true when the cursor entered a
// new message.
ROCP2P_HD bool rocp2p_vl_next(rocp2p_vl_cursor* cur, const uint64_t* cstart,
                              const uint64_t* lens) {
  if (++cur->ci < cur->cpm) return false;
  uint64_t m = cur->m + 1;
  uint64_t first = cstart[m], end = cstart[m + 1];
  while (end == first) {  // zero-length: no chunks, nothing to do
    m++;
    end = cstart[m + 1];
  }
  cur->m = m;
  cur->ci = 0;
  cur->cpm = end - first;
  cur->len = lens[m];
  return true;
}
