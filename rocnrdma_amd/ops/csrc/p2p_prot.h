// SPDX-License-Identifier: MIT
// Memory protection of the byte-granular message engine — single
// definition shared by the GPU scan kernel (p2p_kernels.hip) and plain
// g++ tests, so the CPU tier judges a batch with the very code the
// kernel runs.
//
// An HCA never trusts a work request: it resolves the request's lkey and
// rkey to registered memory regions (MRs), checks the range and the
// access rights, and completes a request that fails with an error status
// instead of moving a byte.  Here the MR table is R entries of four
// 64-bit words (key, addr, length, access).  access uses the verbs bits
// and 0 marks a free entry.  A key is slot << 8 | tag with slot < R <=
// 2^20, so the lookup is one indexed load: entry key >> 8 must exist, be
// in use and hold exactly this key — the tag makes a stale key fail once
// its slot has been registered again.
//
// A message is offs[m], addrs[m], lens[m] as for the byte-granular
// engine plus keys[m] = lkey << 32 | rkey.  Its verdict is a value of
// enum ibv_wc_status; the first rule that applies wins:
//   1. lens[m] == 0                          -> SUCCESS (keys not read)
//   2. lens[m] < 0                           -> LOC_LEN_ERR
//   3. outside side (addrs[m], lkey): key does not resolve, range not
//      inside the MR, or (scatter) no LOCAL_WRITE   -> LOC_PROT_ERR
//   4. region side (region_base + offs[m], rkey): key does not resolve,
//      range not inside the MR, or no REMOTE_WRITE (gather) /
//      REMOTE_READ (scatter)                 -> REM_ACCESS_ERR
//   5. otherwise                             -> SUCCESS
// With a queue-pair state word the batch is ordered: f is the first
// message whose verdict is not SUCCESS (0 when the word was already set
// on entry), messages before f keep their verdict, f keeps its own, and
// everything behind f — and f itself when the word was set on entry —
// completes with WR_FLUSH_ERR.  A message whose final status is not
// SUCCESS has the effective length 0 and so owns no chunk of the engine.
#pragma once
#include "p2p_bytes.h"

#define ROCP2P_ACCESS_LOCAL_WRITE 1u
#define ROCP2P_ACCESS_REMOTE_WRITE 2u
#define ROCP2P_ACCESS_REMOTE_READ 4u

#define ROCP2P_WC_SUCCESS 0u
#define ROCP2P_WC_LOC_LEN_ERR 1u
#define ROCP2P_WC_LOC_PROT_ERR 4u
#define ROCP2P_WC_WR_FLUSH_ERR 5u
#define ROCP2P_WC_REM_ACCESS_ERR 10u

#define ROCP2P_PROT_MR_WORDS 4u
#define ROCP2P_PROT_MAX_MR (1u << 20)
// "no message failed": above every index of a batch (n < 2^32)
#define ROCP2P_PROT_NO_F 0xffffffffu

// Scratch of a protected launch, in 64-bit words: cstart[n + 1], then
// the effective lengths elen[n].
#define ROCP2P_PROT_SCRATCH_WORDS(n) (2 * (uint64_t)(n) + 1)

// Is [a, a + len) inside [addr, addr + length)?  No sum is formed: a
// range that wraps 2^64 is outside every MR.
ROCP2P_HD bool rocp2p_prot_range_ok(uint64_t a, uint64_t len, uint64_t addr,
                                    uint64_t length) {
  return a >= addr && len <= length && a - addr <= length - len;
}

// Does `key` resolve in the table of nmr entries to an MR that holds
// [a, a + len) and grants every bit of `need`?
ROCP2P_HD bool rocp2p_prot_side_ok(const uint64_t* mrs, uint32_t nmr,
                                   uint32_t key, uint64_t a, uint64_t len,
                                   uint64_t need) {
  const uint32_t slot = key >> 8;
  if (slot >= nmr) return false;
  const uint64_t* e = mrs + (uint64_t)slot * ROCP2P_PROT_MR_WORDS;
  const uint64_t access = e[3];
  if (!access || e[0] != key) return false;
  if (!rocp2p_prot_range_ok(a, len, e[1], e[2])) return false;
  return (access & need) == need;
}

// The verdict of one message, judged on its own.
ROCP2P_HD uint32_t rocp2p_prot_verdict(const uint64_t* mrs, uint32_t nmr,
                                       uint64_t region_base, uint64_t off,
                                       uint64_t addr, uint64_t len,
                                       uint64_t keys, bool gather) {
  if (!len) return ROCP2P_WC_SUCCESS;
  if (len >> 63) return ROCP2P_WC_LOC_LEN_ERR;
  if (!rocp2p_prot_side_ok(mrs, nmr, (uint32_t)(keys >> 32), addr, len,
                           gather ? 0u : ROCP2P_ACCESS_LOCAL_WRITE))
    return ROCP2P_WC_LOC_PROT_ERR;
  // the engine forms region + off the same way, modulo 2^64
  if (!rocp2p_prot_side_ok(mrs, nmr, (uint32_t)keys, region_base + off, len,
                           gather ? ROCP2P_ACCESS_REMOTE_WRITE
                                  : ROCP2P_ACCESS_REMOTE_READ))
    return ROCP2P_WC_REM_ACCESS_ERR;
  return ROCP2P_WC_SUCCESS;
}

// The status message m completes with.  qp: the batch has a queue-pair
// state word, which was set on entry when entry_err; f: the first
// message whose verdict is not SUCCESS, ROCP2P_PROT_NO_F for none.
ROCP2P_HD uint32_t rocp2p_prot_final(uint32_t verdict, uint32_t m, uint32_t f,
                                     bool qp, bool entry_err) {
  if (!qp) return verdict;
  return (entry_err || m > f) ? ROCP2P_WC_WR_FLUSH_ERR : verdict;
}

// What the engine moves of a message of len bytes that completed with
// `status`.
ROCP2P_HD uint64_t rocp2p_prot_elen(uint32_t status, uint64_t len) {
  return status == ROCP2P_WC_SUCCESS ? len : 0;
}
