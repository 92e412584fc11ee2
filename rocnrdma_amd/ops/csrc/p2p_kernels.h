// SPDX-License-Identifier: MIT
// C ABI of the gfx950 payload kernels (implementation: p2p_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

extern "C" {

// No call here needs set-up.  The CRC entry points upload their lookup
// tables (a compile-time constant, p2p_crc.h) to the current device
// before that device's first CRC launch, under a lock: call them, like
// every launch, with the device of `stream` current.

// buf[i] = splitmix64(seed + (i+1)*GOLDEN) for each 8-byte word.
// nbytes % 8 == 0.  HBM-streaming (16 B/lane vector stores).
hipError_t rocp2p_fill(void* buf, uint64_t nbytes, uint64_t seed,
                       hipStream_t stream);

// Recompute the fill pattern and count mismatching words into
// *d_mismatch (device u64, caller zeroes it).
hipError_t rocp2p_verify(const void* buf, uint64_t nbytes, uint64_t seed,
                         unsigned long long* d_mismatch, hipStream_t stream);

// d_out[p] = zlib-compatible CRC32 of 4 KiB page p.  buf 4 KiB-aligned
// length (npages * 4096 bytes).  One wave per page; per-lane 64 B
// segment CRCs combined via GF(2) shift matrices + wave XOR reduce;
// lookup tables staged in LDS.
hipError_t rocp2p_crc32_pages(const void* buf, uint64_t npages,
                              uint32_t* d_out, hipStream_t stream);

// CRC32 digests of caller-supplied payloads, computed in HBM (GF(2)
// helpers: p2p_crc.h).  Stream-ordered, allocate nothing; d_out is
// zeroed on `stream` and accumulated with atomicXor (order-independent,
// so bit-reproducible).
//
// msgs: d_out[m] = zlib crc32 of base[off_m, off_m + msg_bytes), off_m =
// d_offs[m] or m * msg_bytes when d_offs is null.  Same preconditions
// as rocp2p_gather: msg_bytes a non-zero multiple of 16, base and every
// offset 16-byte aligned (host-visible violations: hipErrorInvalidValue).
// region: one digest of any byte length (0 -> 0); buf 16-byte aligned;
// never loads a byte at or beyond buf + nbytes.
// Chunk CRCs never leave the wave that computes them, so neither call
// needs working memory.
// grid_cap: 0 = tuned default; otherwise the maximum number of
// workgroups (16 waves each).  A tuning and testing knob: it makes each
// wave walk a multi-chunk run at test-sized inputs (the default grid
// only does so above 16 MiB).
hipError_t rocp2p_crc32_msgs(const void* base, const uint64_t* d_offs,
                             uint64_t msg_bytes, uint32_t n, uint32_t* d_out,
                             uint32_t grid_cap, hipStream_t stream);
hipError_t rocp2p_crc32_region(const void* buf, uint64_t nbytes,
                               uint32_t* d_out, uint32_t grid_cap,
                               hipStream_t stream);

// Streaming device copy (bandwidth ceiling probe), 16 B/lane.
hipError_t rocp2p_copy(void* dst, const void* src, uint64_t nbytes,
                       hipStream_t stream);
// Nontemporal variant (streamed-once data; see microarch nt rows).
hipError_t rocp2p_copy_nt(void* dst, const void* src, uint64_t nbytes,
                          hipStream_t stream);

// GPU-driven batched message engine (the NIC-WQE analog: one launch
// retires a whole queue of posted messages).  src_addrs/dst_offs are
// device-visible u64 arrays of n entries; every message is msg_bytes
// (16-byte multiple).  gather: host-pinned sources -> HBM region.
// scatter: HBM region -> host-pinned destinations.
hipError_t rocp2p_gather(void* dst_base, const uint64_t* d_dst_offs,
                         const uint64_t* d_src_addrs, uint64_t msg_bytes,
                         uint32_t n, hipStream_t stream);
hipError_t rocp2p_scatter(const void* src_base, const uint64_t* d_src_offs,
                          const uint64_t* d_dst_addrs, uint64_t msg_bytes,
                          uint32_t n, hipStream_t stream);

// The same engine with an inline ICRC: one launch moves the batch and
// leaves d_out[m] = zlib crc32 of message m, taken from the registers
// the bytes pass through — the bytes as they were loaded (over the link
// for gather, from HBM for scatter), not the bytes that landed; the
// receiving memory is proven by rocp2p_crc32_msgs / rocp2p_verify.
// Same descriptors and preconditions as gather/scatter; no byte outside
// [start, start + msg_bytes) of a message is touched on either side.
// Stream-ordered, allocate nothing; d_out (n words) is zeroed on
// `stream`.  grid_cap: 0 = tuned default (128 workgroups of 4 waves, and
// never above the plain engine's cap), otherwise a lower maximum — a
// tuning and testing knob.
hipError_t rocp2p_gather_crc(void* dst_base, const uint64_t* d_dst_offs,
                             const uint64_t* d_src_addrs, uint64_t msg_bytes,
                             uint32_t n, uint32_t* d_out, uint32_t grid_cap,
                             hipStream_t stream);
hipError_t rocp2p_scatter_crc(const void* src_base,
                              const uint64_t* d_src_offs,
                              const uint64_t* d_dst_addrs, uint64_t msg_bytes,
                              uint32_t n, uint32_t* d_out, uint32_t grid_cap,
                              hipStream_t stream);

// Per-message lengths: the same engine, digest and inline ICRC for
// batches in which message m has d_lens[m] bytes (device u64 array of n
// entries; work split and cursor: p2p_varlen.h).  0 is legal, as a
// zero-length RDMA write is: nothing is touched and the digest is 0,
// zlib's crc32(b"").  For the engine the lengths are multiples of 16 and
// offsets/addresses 16-byte aligned, as above; crc32_msgs_v takes any
// byte length and never loads a byte at or past a message's end.  The
// descriptors on the device are trusted like d_offs / d_addrs are.
// Stream-ordered, allocate nothing, no host synchronise: a one-workgroup
// scan kernel writes the chunk prefix sums into d_cstart (n + 1 words of
// caller-provided scratch) and the main kernel follows on the same
// stream.  The host never learns the sum of the lengths.
// max_msg_bytes: an upper bound the caller knows (the slot size), 0 =
// unknown.  It only sizes the grid; results do not depend on it.
// d_out: n digests (zeroed on `stream`); for the engine it may be null:
// no ICRC, no tables staged, no CRC work.
// grid_cap: 0 = the default of the uniform counterpart, otherwise a
// lower maximum number of workgroups.
// hipErrorInvalidValue: null d_cstart, base not 16-byte aligned.
// n == 0 is a no-op.  No byte outside [start, start + len) of any
// message is loaded or stored on either side.
hipError_t rocp2p_gather_v(void* dst_base, const uint64_t* d_dst_offs,
                           const uint64_t* d_src_addrs,
                           const uint64_t* d_lens, uint32_t n,
                           uint64_t max_msg_bytes, uint64_t* d_cstart,
                           uint32_t* d_out, uint32_t grid_cap,
                           hipStream_t stream);
hipError_t rocp2p_scatter_v(const void* src_base, const uint64_t* d_src_offs,
                            const uint64_t* d_dst_addrs,
                            const uint64_t* d_lens, uint32_t n,
                            uint64_t max_msg_bytes, uint64_t* d_cstart,
                            uint32_t* d_out, uint32_t grid_cap,
                            hipStream_t stream);
hipError_t rocp2p_crc32_msgs_v(const void* base, const uint64_t* d_offs,
                               const uint64_t* d_lens, uint32_t n,
                               uint64_t max_msg_bytes, uint64_t* d_cstart,
                               uint32_t* d_out, uint32_t grid_cap,
                               hipStream_t stream);

// Byte-granular messages: the argument lists, errors and guarantees of
// the _v calls above with "16" removed.  d_lens[m] >= 0 is any byte
// count, read from any byte address and written to any byte address;
// the relative misalignment (src - dst) mod 16 is arbitrary per message
// (geometry: p2p_bytes.h).  Only the region base stays 16-byte aligned.
// No byte outside [start, start + len) of any message is loaded or
// stored on either side: full granules move as naturally aligned
// 16-byte accesses, a partial first or last granule as naturally aligned
// 1-, 2-, 4- and 8-byte accesses of exactly its valid bytes, never a
// read-modify-write — neighbouring messages may share a granule.
// Zero-length messages reach no load, store or atomic, their digest is
// 0.  Results do not depend on max_msg_bytes, grid_cap or the grid.
// Stream-ordered, allocate nothing, no host synchronise; d_cstart is
// n + 1 words of scratch.  hipErrorInvalidValue: null d_cstart, base not
// 16-byte aligned.  n == 0 is a no-op.  Aligned multiples of 16 give
// what the _v calls give.
hipError_t rocp2p_gather_b(void* dst_base, const uint64_t* d_dst_offs,
                           const uint64_t* d_src_addrs,
                           const uint64_t* d_lens, uint32_t n,
                           uint64_t max_msg_bytes, uint64_t* d_cstart,
                           uint32_t* d_out, uint32_t grid_cap,
                           hipStream_t stream);
hipError_t rocp2p_scatter_b(const void* src_base, const uint64_t* d_src_offs,
                            const uint64_t* d_dst_addrs,
                            const uint64_t* d_lens, uint32_t n,
                            uint64_t max_msg_bytes, uint64_t* d_cstart,
                            uint32_t* d_out, uint32_t grid_cap,
                            hipStream_t stream);
// d_out[m] = zlib crc32 of base[d_offs[m], d_offs[m] + d_lens[m]), any
// offset, any length.
hipError_t rocp2p_crc32_msgs_b(const void* base, const uint64_t* d_offs,
                               const uint64_t* d_lens, uint32_t n,
                               uint64_t max_msg_bytes, uint64_t* d_cstart,
                               uint32_t* d_out, uint32_t grid_cap,
                               hipStream_t stream);

// Scatter/gather lists: the byte-granular engine for messages that are
// the concatenation of several outside buffers, as a work request's
// sg_list is (geometry and scratch layout: p2p_sgl.h).  The batch has n
// messages and nsge scatter/gather entries (SGEs) in CSR form:
// d_sge_start[n + 1] is nondecreasing from 0 to nsge, message m owns the
// SGEs d_sge_start[m] .. d_sge_start[m + 1] - 1, SGE j is the
// d_sge_lens[j] >= 0 bytes at the outside address d_sge_addrs[j].
// gather_sg writes the SGEs of message m back to back to
// base[d_offs[m], d_offs[m] + L_m), L_m the sum of their lengths;
// scatter_sg cuts that range, in order, over the SGEs.  Any address, any
// offset, any length; the relative misalignment is arbitrary per SGE and
// only the base is 16-byte aligned.  No byte outside an SGE or outside
// the region range of a message is loaded or stored, and partial
// granules are written with narrow stores, never a read-modify-write:
// consecutive SGEs and neighbouring messages may share a granule.  A
// message without SGEs and an SGE of length 0 are legal anywhere and
// reach no load, store or atomic.  SGEs may overlap on the side that is
// read; overlap on the side that is written is undefined.
// d_out: n digests (zeroed on `stream`), or null for no ICRC.  d_out[m]
// is zlib's crc32 of the L_m message bytes however they are cut — what
// the _b calls give for the same bytes as one message; 0 for an empty
// message.  One SGE per message gives what the _b calls give.
// d_scratch: ROCP2P_SGL_SCRATCH_WORDS(n, nsge) 64-bit words.
// max_msg_bytes bounds a whole message (0 = unknown) and grid_cap caps
// the workgroups as above; results depend on neither.  Stream-ordered
// (a one-workgroup scan kernel, then the engine), allocate nothing, no
// host synchronise.  hipErrorInvalidValue: null d_scratch, base not
// 16-byte aligned.  n == 0 is a no-op; nsge == 0 only zeroes d_out.
hipError_t rocp2p_gather_sg(void* dst_base, const uint64_t* d_dst_offs,
                            const uint64_t* d_sge_start,
                            const uint64_t* d_sge_addrs,
                            const uint64_t* d_sge_lens, uint32_t n,
                            uint32_t nsge, uint64_t max_msg_bytes,
                            uint64_t* d_scratch, uint32_t* d_out,
                            uint32_t grid_cap, hipStream_t stream);
hipError_t rocp2p_scatter_sg(const void* src_base, const uint64_t* d_src_offs,
                             const uint64_t* d_sge_start,
                             const uint64_t* d_sge_addrs,
                             const uint64_t* d_sge_lens, uint32_t n,
                             uint32_t nsge, uint64_t max_msg_bytes,
                             uint64_t* d_scratch, uint32_t* d_out,
                             uint32_t grid_cap, hipStream_t stream);

// Memory protection for the byte-granular engine (rules: p2p_prot.h).
// The descriptors of the _b calls plus d_keys[m] = lkey << 32 | rkey and
// an MR table d_mrs of nmr entries {key, addr, length, access} (device,
// 4 words each).  A one-workgroup scan kernel judges every message —
// keys, ranges (wrap-safe), access rights — writes its ibv_wc_status
// into d_status[m] and hands the _b engine an effective length of 0 for
// every message that did not complete with SUCCESS: such a message
// reaches no load, store or atomic and its digest is 0.  No descriptor
// is trusted: an offset, address, length or key of any value gives a
// status, never an access outside an MR.  The table itself is trusted.
// d_qp_state: null = every message is judged on its own.  Otherwise one
// device word, 0 = ready: the first message that fails completes with
// its status, every later one with WR_FLUSH_ERR, and the word is set to
// 1; a word that is non-zero on entry flushes the whole batch.
// d_scratch: ROCP2P_PROT_SCRATCH_WORDS(n) 64-bit words.  d_out: n
// digests or null, max_msg_bytes and grid_cap as for the _b calls.
// Stream-ordered, allocate nothing, no host synchronise.
// hipErrorInvalidValue: null d_scratch, d_status or d_mrs, nmr == 0 or
// nmr > 2^20, base not 16-byte aligned.  n == 0 is a no-op and leaves
// the word alone.  With a table that covers everything and valid keys
// the bytes and digests are those of the _b calls.
hipError_t rocp2p_gather_p(void* dst_base, const uint64_t* d_dst_offs,
                           const uint64_t* d_src_addrs,
                           const uint64_t* d_lens, const uint64_t* d_keys,
                           uint32_t n, const uint64_t* d_mrs, uint32_t nmr,
                           int32_t* d_qp_state, uint64_t max_msg_bytes,
                           uint64_t* d_scratch, int32_t* d_status,
                           uint32_t* d_out, uint32_t grid_cap,
                           hipStream_t stream);
hipError_t rocp2p_scatter_p(const void* src_base, const uint64_t* d_src_offs,
                            const uint64_t* d_dst_addrs,
                            const uint64_t* d_lens, const uint64_t* d_keys,
                            uint32_t n, const uint64_t* d_mrs, uint32_t nmr,
                            int32_t* d_qp_state, uint64_t max_msg_bytes,
                            uint64_t* d_scratch, int32_t* d_status,
                            uint32_t* d_out, uint32_t grid_cap,
                            hipStream_t stream);

}  // extern "C"
