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

// a * b mod P.  32 branch-free steps (zlib's multmodp without the
// early exit, so every lane of a wave runs the same instruction count).
ROCP2P_HD uint32_t rocp2p_crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; i--) {
    p ^= (0u - ((a >> i) & 1u)) & b;
    b = (b >> 1) ^ ((0u - (b & 1u)) & ROCP2P_CRC_POLY);
  }
  return p;
}

// tab[k] = x^(8 * 2^k) mod P, by repeated squaring from x^8.
ROCP2P_HD void rocp2p_crc_xpow_table(uint32_t tab[ROCP2P_CRC_XPOW_N]) {
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
ROCP2P_HD void rocp2p_crc_xpow8_table(uint32_t t8[8][256],
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
