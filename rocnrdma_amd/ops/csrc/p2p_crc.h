// SPDX-License-Identifier: MIT
// GF(2) arithmetic behind the CRC32 digests — single definition shared
// by the GPU kernels (p2p_kernels.hip), the C++ harness and plain g++
// tests.  Polynomials are 32-bit, reflected (zlib convention: bit 31 is
// x^0, bit 0 is x^31), reduced mod P = 0xEDB88320.  Must stay
// bit-identical to crc32_shift/crc32_combine in
// rocnrdma_amd/utils/pattern.py.
//
// The one identity everything rests on (zlib's crc32_combine):
//   crc(A || B) = shift(crc(A), |B|) ^ crc(B),  shift(c, n) = c * x^(8n)
// shift is linear over XOR, so a digest of any byte range is the XOR of
// the independently computed piece CRCs, each shifted by the number of
// bytes that follow the piece.
#pragma once
#ifdef __cplusplus
#include <cstdint>
#else
#include <stdint.h>
#endif

#include "p2p_pattern.h"  // ROCP2P_HD

#define ROCP2P_CRC_POLY 0xEDB88320u
#define ROCP2P_CRC_ONE 0x80000000u  // the polynomial 1 (x^0)
#define ROCP2P_CRC_XPOW_N 64        // table entries: x^(8 * 2^k), k < 64

// The table builders below also run at compile time (C++14 and later):
// the kernels' lookup tables are a constant expression, not run-time
// state.
#if defined(__cplusplus) && __cplusplus >= 201402L
#define ROCP2P_HDC constexpr ROCP2P_HD
#else
#define ROCP2P_HDC ROCP2P_HD
#endif

// a * b mod P.  32 branch-free steps (zlib's multmodp without the
// early exit, so every lane of a wave runs the same instruction count).
ROCP2P_HDC uint32_t rocp2p_crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; i--) {
    p ^= (0u - ((a >> i) & 1u)) & b;
    b = (b >> 1) ^ ((0u - (b & 1u)) & ROCP2P_CRC_POLY);
  }
  return p;
}

// tab[k] = x^(8 * 2^k) mod P, by repeated squaring from x^8.
ROCP2P_HDC void rocp2p_crc_xpow_table(uint32_t tab[ROCP2P_CRC_XPOW_N]) {
  uint32_t p = ROCP2P_CRC_ONE >> 8;  // x^8: one byte
  for (int k = 0; k < ROCP2P_CRC_XPOW_N; k++) {
    tab[k] = p;
    p = rocp2p_crc_mulmod(p, p);
  }
}

// x^(8 * nbytes) mod P, square-and-multiply over the table above.
ROCP2P_HD uint32_t rocp2p_crc_xpow(uint64_t nbytes, const uint32_t* tab) {
  uint32_t p = ROCP2P_CRC_ONE;
  for (int k = 0; nbytes; nbytes >>= 1, k++)
    if (nbytes & 1) p = rocp2p_crc_mulmod(tab[k], p);
  return p;
}

// Byte-sliced powers for hot paths: t8[j][v] = x^(8 * v * 256^j), so
// x^(8 * nbytes) is the product of one entry per non-zero byte of
// nbytes — at most 2 mulmods below 16 MiB instead of one per set bit.
// 8 KiB; built from the x^(8 * 2^k) table.
ROCP2P_HDC void rocp2p_crc_xpow8_table(uint32_t t8[8][256],
                                      const uint32_t* tab) {
  for (int j = 0; j < 8; j++) {
    t8[j][0] = ROCP2P_CRC_ONE;
    for (int v = 1; v < 256; v++)
      t8[j][v] = rocp2p_crc_mulmod(t8[j][v - 1], tab[8 * j]);
  }
}

ROCP2P_HD uint32_t rocp2p_crc_xpow8(uint64_t nbytes,
                                    const uint32_t (*t8)[256]) {
  uint32_t p = t8[0][nbytes & 0xff];
  for (int j = 1; (nbytes >>= 8) != 0; j++)
    if (nbytes & 0xff) p = rocp2p_crc_mulmod(p, t8[j][nbytes & 0xff]);
  return p;
}

// crc * x^(8 * nbytes): what crc(A) contributes to the CRC of a string
// in which nbytes more bytes follow A.
ROCP2P_HD uint32_t rocp2p_crc_shift(uint32_t crc, uint64_t nbytes,
                                    const uint32_t* tab) {
  return rocp2p_crc_mulmod(rocp2p_crc_xpow(nbytes, tab), crc);
}

// crc(A || B) from c1 = crc(A), c2 = crc(B), len2 = |B|.  len2 == 0 is
// the identity on c1 (crc of the empty string is 0).
ROCP2P_HD uint32_t rocp2p_crc_combine(uint32_t c1, uint32_t c2, uint64_t len2,
                                      const uint32_t* tab) {
  return rocp2p_crc_shift(c1, len2, tab) ^ c2;
}

// ---------------------------------------------------------------------
// Lookup tables of the kernels' hot paths, and the two lookups.

typedef uint32_t rocp2p_crc_tab256[256];

// zlib's slicing-by-8: advance the (pre-inverted) crc register over the
// 8 bytes lo | hi << 32.  t = the slice table below.
ROCP2P_HD uint32_t rocp2p_crc_step8(const rocp2p_crc_tab256* t, uint32_t crc,
                                    uint32_t lo, uint32_t hi) {
  uint32_t a = lo ^ crc;
  return t[7][a & 0xff] ^ t[6][(a >> 8) & 0xff] ^ t[5][(a >> 16) & 0xff] ^
         t[4][a >> 24] ^ t[3][hi & 0xff] ^ t[2][(hi >> 8) & 0xff] ^
         t[1][(hi >> 16) & 0xff] ^ t[0][hi >> 24];
}

// Byte-sliced GF(2)-linear operator applied to c: 4 lookups instead of
// a 32-step mulmod.  m = one level of the shift table below.
ROCP2P_HD uint32_t rocp2p_crc_apply(const rocp2p_crc_tab256* m, uint32_t c) {
  return m[0][c & 0xff] ^ m[1][(c >> 8) & 0xff] ^ m[2][(c >> 16) & 0xff] ^
         m[3][c >> 24];
}

#if defined(__cplusplus) && __cplusplus >= 201402L
struct rocp2p_crc_tables {
  uint32_t slice[8][256];     // slicing-by-8
  uint32_t shift[6][4][256];  // shift[k][b][v] = (v << 8b) * x^(8 * 64 * 2^k)
  uint32_t xpow8[8][256];     // rocp2p_crc_xpow8_table
  // Added behind the three above so that none of their offsets moves:
  // shift16[k][b][v] = (v << 8b) * x^(8 * 16 * 2^k), the 16- and 32-byte
  // operators under shift[0] in the inline-ICRC engine's lane tree.
  uint32_t shift16[2][4][256];
};

// One level of a byte-sliced shift operator: m[b][v] = (v << 8b) * p.
constexpr void rocp2p_crc_shift_level(uint32_t m[4][256], uint32_t p) {
  uint32_t bit[32] = {};  // (1 << i) * p; the rest by linearity
  for (int i = 0; i < 32; i++) bit[i] = rocp2p_crc_mulmod(p, 1u << i);
  for (int b = 0; b < 4; b++)
    for (uint32_t v = 0; v < 256; v++) {
      uint32_t s = 0;
      for (int j = 0; j < 8; j++) s ^= (0u - ((v >> j) & 1u)) & bit[8 * b + j];
      m[b][v] = s;
    }
}

// All four, as one constant expression: 48 KiB that depend on nothing
// at run time.
constexpr rocp2p_crc_tables rocp2p_crc_make_tables() {
  rocp2p_crc_tables t = {};
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++)
      c = (c >> 1) ^ ((0u - (c & 1u)) & ROCP2P_CRC_POLY);
    t.slice[0][i] = c;
  }
  for (int s = 1; s < 8; s++)
    for (uint32_t i = 0; i < 256; i++)
      t.slice[s][i] =
          (t.slice[s - 1][i] >> 8) ^ t.slice[0][t.slice[s - 1][i] & 0xff];

  uint32_t xp[ROCP2P_CRC_XPOW_N] = {};
  rocp2p_crc_xpow_table(xp);
  for (int k = 0; k < 6; k++) rocp2p_crc_shift_level(t.shift[k], xp[6 + k]);
  rocp2p_crc_xpow8_table(t.xpow8, xp);
  for (int k = 0; k < 2; k++) rocp2p_crc_shift_level(t.shift16[k], xp[4 + k]);
  return t;
}
#endif  // C++14
