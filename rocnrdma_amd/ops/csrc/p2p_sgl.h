// SPDX-License-Identifier: MIT
// Geometry of scatter/gather lists — single definition shared by the GPU
// kernels (p2p_kernels.hip) and plain g++ tests, so the CPU tier turns a
// list into work items with the very code the scan kernel runs.
//
// A batch has n messages and S scatter/gather entries (SGEs) in CSR
// form: message m owns the SGEs sge_start[m] .. sge_start[m + 1] - 1
// (sge_start is nondecreasing, sge_start[0] = 0, sge_start[n] = S), SGE
// j is the sge_lens[j] bytes at the outside address sge_addrs[j], and
// the message is their concatenation in list order at region offset
// offs[m].  With P the exclusive byte prefix sum over sge_lens (S + 1
// entries), SGE j of message m
//   - covers the region bytes from offs[m] + P[j] - P[sge_start[m]] on,
//   - has tail = P[sge_start[m + 1]] - P[j + 1] message bytes behind it,
//   - is cut into rocp2p_b_chunks chunks on the granule grid of the side
//     that is written (p2p_bytes.h): the region for a gather, its own
//     address for a scatter.
// The engine's work item is the SGE: to the chunk walk of p2p_varlen.h
// an SGE is a message of its own, and only the digest knows better — a
// CRC piece of SGE j is shifted by tail more bytes and lands in the
// digest of the message that owns j.
#pragma once
#include "p2p_bytes.h"

// Scratch of a batch, in 64-bit words.  Seven arrays, in this order:
// P[S + 1], cstart[S + 1], to[S], from[S], tail[S] (64-bit each) and
// owner[S] (32-bit).  It depends on S only; n is taken so that a later
// layout may use it.
#define ROCP2P_SGL_SCRATCH_WORDS(n, S) \
  ((uint64_t)0 * (n) + 2 * ((uint64_t)(S) + 1) + 3 * (uint64_t)(S) + \
   ((uint64_t)(S) + 1) / 2)

typedef struct rocp2p_sgl_view {
  uint64_t* prefix;  // P: bytes of the SGEs before j; P[S] = all bytes
  uint64_t* cstart;  // chunks of the SGEs before j; cstart[S] = all chunks
  uint64_t* to;      // address SGE j is written at
  uint64_t* from;    // address SGE j is read from
  uint64_t* tail;    // message bytes behind SGE j
  uint32_t* owner;   // the message SGE j belongs to
} rocp2p_sgl_view;

ROCP2P_HD rocp2p_sgl_view rocp2p_sgl_carve(uint64_t* scratch, uint64_t S) {
  rocp2p_sgl_view v;
  v.prefix = scratch;
  v.cstart = v.prefix + S + 1;
  v.to = v.cstart + S + 1;
  v.from = v.to + S;
  v.tail = v.from + S;
  v.owner = reinterpret_cast<uint32_t*>(v.tail + S);
  return v;
}

// The message that owns SGE j, j < sge_start[n]: the one m with
// sge_start[m] <= j < sge_start[m + 1].  Messages without SGEs are never
// the answer.  One binary search; a whole batch is cheaper served by
// rocp2p_sgl_has_sges and a running maximum, see below.
ROCP2P_HD uint64_t rocp2p_sgl_owner(const uint64_t* sge_start, uint64_t n,
                                    uint64_t j) {
  return rocp2p_vl_find(sge_start, n, j);
}

// Does message m own an SGE?  Owners for a whole batch without a search
// per SGE: start from owner[] = 0, let every message that has SGEs write
// owner[sge_start[m]] = m, then take the running maximum over owner[] —
// message numbers grow with the SGE index, and SGE 0 belongs to the
// first message that has any.
ROCP2P_HD bool rocp2p_sgl_has_sges(const uint64_t* sge_start, uint64_t m) {
  return sge_start[m] < sge_start[m + 1];
}

// Everything the engine needs of SGE j, from the finished byte prefix
// sums and owners: fills to[j], from[j] and tail[j] and returns the chunk
// count.  region is the address of the (16-byte aligned) region base.
ROCP2P_HD uint64_t rocp2p_sgl_item(const rocp2p_sgl_view& v, uint64_t region,
                                   const uint64_t* offs,
                                   const uint64_t* sge_start,
                                   const uint64_t* sge_addrs, uint64_t j,
                                   bool gather) {
  const uint64_t m = v.owner[j];
  const uint64_t at = v.prefix[j], next = v.prefix[j + 1];
  const uint64_t inside = region + offs[m] + (at - v.prefix[sge_start[m]]);
  const uint64_t outside = sge_addrs[j];
  const uint64_t to = gather ? inside : outside;
  v.to[j] = to;
  v.from[j] = gather ? outside : inside;
  v.tail[j] = v.prefix[sge_start[m + 1]] - next;
  return rocp2p_b_chunks((uint32_t)to & 15u, next - at);
}
