// SPDX-License-Identifier: MIT
// Geometry of the byte-granular message kernels — single definition
// shared by the GPU kernels (p2p_kernels.hip) and plain g++ tests, so
// the CPU tier cuts, loads, realigns and stores a message with the very
// code a wave runs.
//
// A message of len bytes that is WRITTEN at address dst is cut on the
// grid of naturally aligned 16-byte granules of that side.  With
// skew = dst & 15 the message occupies the bytes [skew, skew + len) of
// the "store stream" that starts at the aligned address dst - skew;
// granule g of the stream is its bytes [16g, 16g + 16) and a chunk is
// 256 granules (4 KiB), so the message has ceil((skew + len) / 4096)
// chunks, none when len == 0.  Only the first and the last granule of a
// message can be partial.  skew == 0 and len % 16 == 0 give exactly the
// chunks and pieces of p2p_varlen.h.
//
// The side that is READ lies s = (src - dst) & 15 bytes further on in
// its own granules: byte p of the store stream is byte p + s of the
// "source stream" that starts at the aligned address src - skew - s, so
// the message occupies [skew + s, skew + s + len) of that stream and
// store granule g is the bytes [s, s + 16) of source granules g, g + 1.
//
// Every access below is naturally aligned for its width and touches
// only bytes inside the range it is given.  Lengths are below 2^63.
#pragma once
#include "p2p_varlen.h"

#define ROCP2P_B_GRAN 16u
#define ROCP2P_B_PER_CHUNK (ROCP2P_VL_CHUNK / ROCP2P_B_GRAN)  // 256

// One granule in registers: the bytes in memory order, little endian.
typedef struct __attribute__((aligned(16))) rocp2p_g16 {
  uint32_t x, y, z, w;
} rocp2p_g16;

// chunks of a message of len bytes stored skew (< 16) bytes into a
// granule: ceil((skew + len) / 4096), 0 for len == 0, no overflow
ROCP2P_HD uint64_t rocp2p_b_chunks(uint32_t skew, uint64_t len) {
  if (!len) return 0;
  const uint64_t tail = len % ROCP2P_VL_CHUNK + skew;  // < 4096 + 16
  return len / ROCP2P_VL_CHUNK +
         (tail + ROCP2P_VL_CHUNK - 1) / ROCP2P_VL_CHUNK;
}

// The bytes [*lo, *hi) of granule g that belong to a message occupying
// [beg, end) of its stream; *lo >= *hi when the granule holds none.
ROCP2P_HD void rocp2p_b_range(uint64_t beg, uint64_t end, uint64_t g,
                              uint32_t* lo, uint32_t* hi) {
  const uint64_t at = g * ROCP2P_B_GRAN;
  *lo = beg > at ? (uint32_t)(beg - at < ROCP2P_B_GRAN ? beg - at
                                                       : ROCP2P_B_GRAN)
                 : 0u;
  *hi = end > at ? (uint32_t)(end - at < ROCP2P_B_GRAN ? end - at
                                                       : ROCP2P_B_GRAN)
                 : 0u;
}

// Is chunk ci full on BOTH sides: all its 256 store granules inside the
// message, and all source granules they are cut from — 257 when s != 0 —
// inside it as well?  Only such a chunk may use whole-granule accesses
// throughout; with s != 0 the first chunk and the chunk(s) holding the
// last 16 - s bytes never are.
ROCP2P_HD bool rocp2p_b_full(uint32_t skew, uint32_t s, uint64_t len,
                             uint64_t ci) {
  const uint64_t p0 = ci * ROCP2P_VL_CHUNK;
  if (p0 < (uint64_t)skew + s) return false;
  return p0 + ROCP2P_VL_CHUNK + (s ? ROCP2P_B_GRAN - s : 0u) <= skew + len;
}

// Width of the access at byte p of a granule when bytes [p, hi) are
// still to do, p < hi <= 16: the widest of 8, 4, 2, 1 that is naturally
// aligned at p and ends at or before hi.  Walking p += width from lo
// tiles [lo, hi) exactly, in at most 7 steps.
ROCP2P_HD uint32_t rocp2p_b_width(uint32_t p, uint32_t hi) {
  uint32_t w = 8;
  while ((p & (w - 1)) || p + w > hi) w >>= 1;
  return w;
}

// Load the bytes [lo, hi) of the granule at gran (16-byte aligned);
// every other byte of the result is 0.  Nothing is loaded when lo >= hi.
ROCP2P_HD rocp2p_g16 rocp2p_b_load(const uint8_t* gran, uint32_t lo,
                                   uint32_t hi) {
  if (lo == 0 && hi == ROCP2P_B_GRAN)
    return *reinterpret_cast<const rocp2p_g16*>(gran);
  uint64_t d0 = 0, d1 = 0;
  for (uint32_t p = lo; p < hi;) {
    const uint32_t w = rocp2p_b_width(p, hi);
    uint64_t v;
    if (w == 8)
      v = *reinterpret_cast<const uint64_t*>(gran + p);
    else if (w == 4)
      v = *reinterpret_cast<const uint32_t*>(gran + p);
    else if (w == 2)
      v = *reinterpret_cast<const uint16_t*>(gran + p);
    else
      v = gran[p];
    if (p < 8)
      d0 |= v << (8 * p);
    else
      d1 |= v << (8 * (p - 8));
    p += w;
  }
  const rocp2p_g16 r = {(uint32_t)d0, (uint32_t)(d0 >> 32), (uint32_t)d1,
                        (uint32_t)(d1 >> 32)};
  return r;
}

// Store the bytes [lo, hi) of v to the granule at gran (16-byte
// aligned): one 16-byte store when that is all of it, otherwise the
// narrow stores of rocp2p_b_width — never a read-modify-write, the
// granule's other bytes may belong to a message another wave owns.
ROCP2P_HD void rocp2p_b_store(uint8_t* gran, uint32_t lo, uint32_t hi,
                              const rocp2p_g16& v) {
  if (lo == 0 && hi == ROCP2P_B_GRAN) {
    *reinterpret_cast<rocp2p_g16*>(gran) = v;
    return;
  }
  const uint64_t d0 = v.x | ((uint64_t)v.y << 32);
  const uint64_t d1 = v.z | ((uint64_t)v.w << 32);
  for (uint32_t p = lo; p < hi;) {
    const uint32_t w = rocp2p_b_width(p, hi);
    const uint64_t x = p < 8 ? d0 >> (8 * p) : d1 >> (8 * (p - 8));
    if (w == 8)
      *reinterpret_cast<uint64_t*>(gran + p) = x;
    else if (w == 4)
      *reinterpret_cast<uint32_t*>(gran + p) = (uint32_t)x;
    else if (w == 2)
      *reinterpret_cast<uint16_t*>(gran + p) = (uint16_t)x;
    else
      gran[p] = (uint8_t)x;
    p += w;
  }
}

// bytes [k, k + 4) of the 8 bytes lo | hi << 32, k = 0..3
ROCP2P_HD uint32_t rocp2p_b_align4(uint32_t lo, uint32_t hi, uint32_t k) {
  return (uint32_t)((lo | ((uint64_t)hi << 32)) >> (8 * k));
}

// Store granule g from the source granules a = g and b = g + 1: the
// bytes [s, s + 16) of a || b, 0 < s < 16.  s is uniform per message,
// so the switch is a scalar branch and every register index is static.
ROCP2P_HD rocp2p_g16 rocp2p_b_realign(const rocp2p_g16& a,
                                      const rocp2p_g16& b, uint32_t s) {
  uint32_t w0, w1, w2, w3, w4;
  switch (s >> 2) {
    case 0: w0 = a.x; w1 = a.y; w2 = a.z; w3 = a.w; w4 = b.x; break;
    case 1: w0 = a.y; w1 = a.z; w2 = a.w; w3 = b.x; w4 = b.y; break;
    case 2: w0 = a.z; w1 = a.w; w2 = b.x; w3 = b.y; w4 = b.z; break;
    default: w0 = a.w; w1 = b.x; w2 = b.y; w3 = b.z; w4 = b.w; break;
  }
  const uint32_t k = s & 3;
  const rocp2p_g16 r = {rocp2p_b_align4(w0, w1, k), rocp2p_b_align4(w1, w2, k),
                        rocp2p_b_align4(w2, w3, k),
                        rocp2p_b_align4(w3, w4, k)};
  return r;
}
