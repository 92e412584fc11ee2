// SPDX-License-Identifier: MIT
//
// p2p_kernels.hip — hand-written gfx950 (CDNA4) payload kernels for the
// GPU-direct RDMA harness: deterministic pattern fill, on-GPU CRC32
// integrity, and a streaming-copy bandwidth probe.  These are the "HIP
// fill/CRC kernel (LDS-staged)" the north star requires: payloads are
// generated AND verified in HBM, so zero-copy RDMA can be proven without
// any host readback.
//
// MI355X design notes:
//  - wave64; all wave-width constants hard-coded 64;
//  - streaming kernels move 16 B/lane/instruction (dwordx4), grid-stride
//    with >> 256 workgroups to fill 8 XCDs;
//  - CRC32: one wave per 4 KiB page, lane l owns bytes [64l, 64l+64);
//    slice-by-8 tables (8 x 256 u32) live in LDS (random-access lookups,
//    exactly what LDS is for); the lanes' segment CRCs are merged by a
//    6-level log tree of byte-sliced GF(2) shift operators (64 B << k),
//    also in LDS.  The algebra and the tables are p2p_crc.h's, checked
//    against zlib in tests/test_crc_digest.py (host) and
//    tests/test_gpu_kernels.py, tests/test_gpu_crc_digest.py (device);
//  - compute ceiling: ~8 table lookups per 8 B per lane; far above the
//    PCIe/NIC rates this harness verifies, far below HBM peak by design
//    (integrity pass, not the timed datapath).

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include "p2p_kernels.h"
#include "p2p_crc.h"
#include "p2p_pattern.h"
#include "p2p_varlen.h"
#include "p2p_bytes.h"
#include "p2p_sgl.h"
#include "p2p_prot.h"

#define WAVE 64u
#define PAGE 4096u
#define SEG 64u  // bytes per lane within a page

#define pattern_word rocp2p_pattern_word

// ---------------------------------------------------------------------
// Streaming-kernel shape (tuned on MI355X, tools/hbm_bench.hip): each
// WAVE owns a contiguous tile of UNROLL x 1 KiB; a lane's UNROLL
// accesses are 64 vectors apart so every instruction stays a fully
// coalesced 1 KiB wave access, with UNROLL independent loads/stores in
// flight per lane.  Nontemporal policy on streamed-once data.
// Measured vs the naive 1-vec grid-stride loop: fill 4.0 -> 5.6 TB/s,
// copy 4.7 -> 5.7 TB/s (r+w).
typedef unsigned long long u64v2_cv __attribute__((ext_vector_type(2)));

// fill: UNROLL=8, nt stores
__global__ void k_fill(uint64_t* __restrict__ buf, uint64_t nwords,
                       uint64_t seed) {
  constexpr int U = 8;
  u64v2_cv* out = reinterpret_cast<u64v2_cv*>(buf);
  uint64_t nvec = nwords / 2;
  uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t nwaves = nthreads / WAVE;
  uint64_t wave = tid / WAVE, lane = tid & (WAVE - 1);
  const uint64_t tile = (uint64_t)WAVE * U;
  uint64_t ntiles = nvec / tile;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    uint64_t base = t * tile + lane;
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint64_t j = base + (uint64_t)WAVE * u;
      u64v2_cv v = {pattern_word(seed, j * 2), pattern_word(seed, j * 2 + 1)};
      __builtin_nontemporal_store(v, &out[j]);
    }
  }
  // vector tail
  for (uint64_t j = ntiles * tile + tid; j < nvec; j += nthreads) {
    u64v2_cv v = {pattern_word(seed, j * 2), pattern_word(seed, j * 2 + 1)};
    __builtin_nontemporal_store(v, &out[j]);
  }
  // odd word tail
  if (blockIdx.x == 0 && threadIdx.x == 0 && (nwords & 1))
    buf[nwords - 1] = pattern_word(seed, nwords - 1);
}

__global__ void k_verify(const uint64_t* __restrict__ buf, uint64_t nwords,
                         uint64_t seed,
                         unsigned long long* __restrict__ mismatch) {
  constexpr int U = 4;
  const u64v2_cv* in = reinterpret_cast<const u64v2_cv*>(buf);
  uint64_t nvec = nwords / 2;
  uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t nwaves = nthreads / WAVE;
  uint64_t wave = tid / WAVE, lane = tid & (WAVE - 1);
  const uint64_t tile = (uint64_t)WAVE * U;
  uint64_t ntiles = nvec / tile;
  uint32_t bad = 0;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    uint64_t base = t * tile + lane;
    u64v2_cv v[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      v[u] = __builtin_nontemporal_load(&in[base + WAVE * u]);
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint64_t j = base + (uint64_t)WAVE * u;
      bad += (v[u].x != pattern_word(seed, j * 2));
      bad += (v[u].y != pattern_word(seed, j * 2 + 1));
    }
  }
  for (uint64_t j = ntiles * tile + tid; j < nvec; j += nthreads) {
    u64v2_cv v = __builtin_nontemporal_load(&in[j]);
    bad += (v.x != pattern_word(seed, j * 2));
    bad += (v.y != pattern_word(seed, j * 2 + 1));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (nwords & 1))
    bad += (buf[nwords - 1] != pattern_word(seed, nwords - 1));
  // wave-reduce then one atomic per wave
  for (unsigned off = WAVE / 2; off; off >>= 1)
    bad += __shfl_xor(bad, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && bad)
    atomicAdd(mismatch, (unsigned long long)bad);
}

// ---------------------------------------------------------------------
// streaming copy (same wave-tile shape; UNROLL=4).  The builtin wants a
// clang vector, not HIP's uint4 class.
typedef unsigned int uint4_cv __attribute__((ext_vector_type(4)));

template <bool NT>
__global__ void k_copy_t(uint4_cv* __restrict__ dst,
                         const uint4_cv* __restrict__ src, uint64_t nvec) {
  constexpr int U = 4;
  uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t nwaves = nthreads / WAVE;
  uint64_t wave = tid / WAVE, lane = tid & (WAVE - 1);
  const uint64_t tile = (uint64_t)WAVE * U;
  uint64_t ntiles = nvec / tile;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    uint64_t base = t * tile + lane;
    uint4_cv v[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      v[u] = NT ? __builtin_nontemporal_load(&src[base + WAVE * u])
                : src[base + WAVE * u];
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (NT)
        __builtin_nontemporal_store(v[u], &dst[base + WAVE * u]);
      else
        dst[base + WAVE * u] = v[u];
    }
  }
  for (uint64_t i = ntiles * tile + tid; i < nvec; i += nthreads)
    dst[i] = src[i];
}

// ---------------------------------------------------------------------
// Batched message engine.  A real HCA retires posted WQEs with its DMA
// hardware regardless of message size; the host-API (hipMemcpyAsync)
// path costs ~10 us per message, capping 4 KB messages near 0.3 GB/s.
// Here one kernel launch retires the whole posted batch: lanes read
// host-pinned staging straight over PCIe (fine-grained zero-copy) and
// store to the HBM region, 16 B/lane, many messages per launch — so the
// small-message lines of the ib_write_bw sweep are PCIe-bound, not
// launch-bound.  msg_bytes is uniform per batch in this kernel and in
// k_msg_engine_crc; batches whose messages carry their own lengths go
// through k_msg_engine_v (below).

// Message m lives at region + offs[m] on one side and at the absolute
// address addrs[m] on the other; GATHER copies addrs -> region, scatter
// the other way.
// vshift: log2(vecs_per_msg) when it is a power of two (uniform branch
// avoids a 64-bit divide per 16-byte vector), else 0xffffffff.
template <bool GATHER>
__global__ void k_msg_engine(uint8_t* __restrict__ region,
                             const uint64_t* __restrict__ offs,
                             const uint64_t* __restrict__ addrs,
                             uint64_t vecs_per_msg, uint64_t total_vecs,
                             uint32_t vshift) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       v < total_vecs; v += stride) {
    uint64_t msg = (vshift != 0xffffffffu) ? (v >> vshift)
                                           : (v / vecs_per_msg);
    uint64_t idx = v - msg * vecs_per_msg;
    uint4* inside = reinterpret_cast<uint4*>(region + offs[msg]);
    uint4* outside = reinterpret_cast<uint4*>(addrs[msg]);
    if (GATHER)
      inside[idx] = outside[idx];
    else
      outside[idx] = inside[idx];
  }
}

// ---------------------------------------------------------------------
// CRC32 (zlib polynomial 0xEDB88320, init/xorout 0xFFFFFFFF)

// slice: slicing-by-8.  shift[k]: byte-sliced GF(2) operator "64 B << k
// follow" (applying a 32x32 GF(2) matrix becomes 4 lookups instead of
// 32 serial dependent steps).  xpow8: x^(8 * v * 256^j) mod P.
// shift16: the 16- and 32-byte operators of k_msg_engine_crc, behind
// the rest so that nothing the older kernels stage has moved.
// Uploaded by crc_tables_ready(), once per device: holding the same
// bytes as constant-initialised data of the code object instead cost
// k_crc32_pages, which stages them 8192 times per GiB, 7-9%
// (docs/PERF.md §2).
__constant__ rocp2p_crc_tables c_crc;

// The 32 KiB a CRC workgroup keeps in LDS.
struct crc_lds {
  uint32_t slice[8][256];
  uint32_t shift[6][4][256];
};

// Stage the slice-by-8 table and the shift operators; ends with the
// barrier that makes them visible to the workgroup.
__device__ __forceinline__ void crc_stage_tables(crc_lds& s) {
  for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
    (&s.slice[0][0])[i] = (&c_crc.slice[0][0])[i];
  for (uint32_t i = threadIdx.x; i < 6 * 4 * 256; i += blockDim.x)
    (&s.shift[0][0][0])[i] = (&c_crc.shift[0][0][0])[i];
  __syncthreads();
}

// zlib crc32 of a 4 KiB chunk, returned in every lane of the wave that
// calls it; seg = this lane's 64-byte segment (4x dwordx4 loads).
__device__ __forceinline__ uint32_t crc_page(const uint8_t* seg, uint32_t lane,
                                             const crc_lds& s) {
  uint4 v0 = reinterpret_cast<const uint4*>(seg)[0];
  uint4 v1 = reinterpret_cast<const uint4*>(seg)[1];
  uint4 v2 = reinterpret_cast<const uint4*>(seg)[2];
  uint4 v3 = reinterpret_cast<const uint4*>(seg)[3];
  uint32_t w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                    v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
  uint32_t crc = 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < 8; i++)
    crc = rocp2p_crc_step8(s.slice, crc, w[2 * i], w[2 * i + 1]);
  crc ^= 0xFFFFFFFFu;

  // Log-tree combine: level k merges adjacent spans of 64B<<k.
  // combine(cL, cR) = shift(cL, span) ^ cR; shift is linear over XOR, so
  // the tree equals the flat XOR-of-shifted-lane-CRCs identity.  The
  // shift operator is UNIFORM per level, and the tree doubles as the
  // wave reduction — every lane ends holding the page CRC.
#pragma unroll
  for (int k = 0; k < 6; k++) {
    uint32_t partner = __shfl_xor(crc, 1u << k, WAVE);
    bool left = ((lane >> k) & 1u) == 0;
    uint32_t cl = left ? crc : partner;
    uint32_t cr = left ? partner : crc;
    crc = rocp2p_crc_apply(s.shift[k], cl) ^ cr;
  }
  return crc;
}

// One wave per 4 KiB page; 4 waves (256 threads) per workgroup.
// Not yet built on crc_stage_tables / crc_page: that form has only
// been measured together with another change that cost this kernel
// 5-8% at 1 GiB (docs/PERF.md §2).
__global__ void __launch_bounds__(256) k_crc32_pages(
    const uint32_t* __restrict__ buf, uint64_t npages,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t s_tab[8][256];
  __shared__ uint32_t s_stab[6][4][256];

  // stage tables into LDS (8 KB slice-by-8 + 24 KB shift operators)
  for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
    (&s_tab[0][0])[i] = (&c_crc.slice[0][0])[i];
  for (uint32_t i = threadIdx.x; i < 6 * 4 * 256; i += blockDim.x)
    (&s_stab[0][0][0])[i] = (&c_crc.shift[0][0][0])[i];
  __syncthreads();

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wave = threadIdx.x / WAVE;  // 0..3
  const uint64_t wave_stride = (uint64_t)gridDim.x * 4;

  for (uint64_t page = blockIdx.x * 4ull + wave; page < npages;
       page += wave_stride) {
    // lane's 64-byte segment as 16 u32 (4x dwordx4 loads)
    const uint32_t* seg =
        buf + page * (PAGE / 4) + lane * (SEG / 4);
    uint4 v0 = reinterpret_cast<const uint4*>(seg)[0];
    uint4 v1 = reinterpret_cast<const uint4*>(seg)[1];
    uint4 v2 = reinterpret_cast<const uint4*>(seg)[2];
    uint4 v3 = reinterpret_cast<const uint4*>(seg)[3];
    uint32_t w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                      v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};

    // zlib crc32 of the 64-byte segment, slicing-by-8 from LDS
    uint32_t crc = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint32_t a = w[2 * i] ^ crc;
      uint32_t b = w[2 * i + 1];
      crc = s_tab[7][a & 0xff] ^ s_tab[6][(a >> 8) & 0xff] ^
            s_tab[5][(a >> 16) & 0xff] ^ s_tab[4][a >> 24] ^
            s_tab[3][b & 0xff] ^ s_tab[2][(b >> 8) & 0xff] ^
            s_tab[1][(b >> 16) & 0xff] ^ s_tab[0][b >> 24];
    }
    crc ^= 0xFFFFFFFFu;

    // uniform log tree, as in crc_page
#pragma unroll
    for (int k = 0; k < 6; k++) {
      uint32_t partner = __shfl_xor(crc, 1u << k, WAVE);
      bool left = ((lane >> k) & 1u) == 0;
      uint32_t cl = left ? crc : partner;
      uint32_t cr = left ? partner : crc;
      crc = s_stab[k][0][cl & 0xff] ^ s_stab[k][1][(cl >> 8) & 0xff] ^
            s_stab[k][2][(cl >> 16) & 0xff] ^ s_stab[k][3][cl >> 24] ^ cr;
    }
    if (lane == 0) out[page] = crc;
  }
}

// ---------------------------------------------------------------------
// CRC32 digests per message / per region (zlib-exact, any content).
//
// Every message is cut into 4 KiB chunks from its own start plus at
// most one partial chunk; chunks are numbered message-major and each
// WAVE owns a contiguous run of them (run length chosen by the
// launcher).  Full chunks go through crc_page (same LDS tables, same
// 32 KB per workgroup).
// Inside a run the wave carries acc = crc(chunks so far of this
// message): acc = shift(acc, 4096) ^ crc(chunk), the 4 KiB shift being
// the level-5 (2 KiB) operator applied twice — 8 LDS lookups, no extra
// table.  When the message or the run ends, acc still has r bytes of
// the message after it and contributes shift(acc, r) to the digest.
// That one variable shift is spread over the wave: lane j < 8 fetches
// x^(8 * byte_j(r) * 256^j) from a byte-sliced power table (8 KiB,
// constant memory), a __shfl_xor product tree over only the levels r
// needs yields x^(8r) in lane 0, one more mulmod applies it — 2
// mulmods per flush below 64 KiB remaining, 3 below 4 GiB, all VALU
// while the kernel is LDS-bound.
// Contributions are XORed into d_out[m] with atomicXor (launcher zeroes
// it); XOR is order-independent so digests are bit-reproducible.  Shares
// of runs that end inside a message are first XORed across the
// workgroup, whose waves own adjacent runs.
//
// The partial chunk (valid < 4096 bytes, any byte count) uses the flat
// identity: lane l owns [64l, min(64l+64, valid)), lanes past the end
// contribute 0, each lane shifts its own CRC by valid - end_l and the
// wave XOR-reduces.  No byte at or beyond the message end is loaded:
// the last partial 16 bytes are fetched with 8/4/2/1-byte loads.

// x^(8*r) in lane 0 (r uniform; other lanes hold partial products).
__device__ __forceinline__ uint32_t crc_xpow_wave(uint64_t r, uint32_t lane) {
  const uint32_t j = lane & 7;  // lanes 8.. mirror 0..7
  uint32_t t = c_crc.xpow8[j][(r >> (8 * j)) & 0xff];
  // level k folds bytes 2^k apart: needed once r has a byte 2^k or above
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (r >> (8u << k))
      t = rocp2p_crc_mulmod(t, __shfl_xor(t, 1u << k, WAVE));
  return t;
}

// Load the nb (0..64) bytes of a lane's segment into w[16], zero padded.
__device__ __forceinline__ void crc_load_partial(const uint8_t* seg,
                                                 uint32_t nb,
                                                 uint32_t w[16]) {
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint8_t* p = seg + 16 * q;
    uint64_t lo = 0, hi = 0;
    if (nb >= 16 * q + 16) {
      uint4 v = *reinterpret_cast<const uint4*>(p);
      lo = v.x | ((uint64_t)v.y << 32);
      hi = v.z | ((uint64_t)v.w << 32);
    } else if (nb > 16 * q) {
      uint32_t rem = nb - 16 * q;  // 1..15: naturally aligned narrow loads
      uint64_t first = 0, rest = 0;
      uint32_t sh = 0;
      if (rem & 8) { first = *reinterpret_cast<const uint64_t*>(p); p += 8; }
      if (rem & 4) { rest = *reinterpret_cast<const uint32_t*>(p); p += 4; sh = 32; }
      if (rem & 2) {
        rest |= (uint64_t)*reinterpret_cast<const uint16_t*>(p) << sh;
        p += 2;
        sh += 16;
      }
      if (rem & 1) rest |= (uint64_t)*p << sh;
      if (rem & 8) { lo = first; hi = rest; } else { lo = rest; }
    }
    w[4 * q] = (uint32_t)lo;
    w[4 * q + 1] = (uint32_t)(lo >> 32);
    w[4 * q + 2] = (uint32_t)hi;
    w[4 * q + 3] = (uint32_t)(hi >> 32);
  }
}

// zlib crc32 of the first nb (0..64) bytes held in w[16]
__device__ __forceinline__ uint32_t crc_bytes64(const rocp2p_crc_tab256* t,
                                                const uint32_t w[16],
                                                uint32_t nb) {
  uint32_t crc = 0xFFFFFFFFu;
  const uint32_t n8 = nb >> 3, rem = nb & 7;
#pragma unroll
  for (uint32_t i = 0; i < 8; i++)
    if (i < n8) crc = rocp2p_crc_step8(t, crc, w[2 * i], w[2 * i + 1]);
  if (rem) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++)
      if (i == n8) { lo = w[2 * i]; hi = w[2 * i + 1]; }
    uint64_t v = lo | ((uint64_t)hi << 32);
    for (uint32_t j = 0; j < rem; j++, v >>= 8)
      crc = t[0][(crc ^ (uint32_t)v) & 0xff] ^ (crc >> 8);
  }
  return crc ^ 0xFFFFFFFFu;
}

// This lane's share of a partial chunk's digest: the chunk's first
// `valid` (1..4095) bytes, seg = this lane's 64-byte segment of it.
__device__ __forceinline__ uint32_t crc_chunk_partial(const crc_lds& s,
                                                      const uint8_t* seg,
                                                      uint32_t valid,
                                                      uint32_t lane) {
  const uint32_t beg = lane * SEG;
  const uint32_t nb = valid > beg ? min(valid - beg, SEG) : 0u;
  uint32_t w[16];
  crc_load_partial(seg, nb, w);
  if (!nb) return 0;
  return rocp2p_crc_mulmod(rocp2p_crc_xpow8(valid - (beg + nb), c_crc.xpow8),
                           crc_bytes64(s.slice, w, nb));
}

// ---------------------------------------------------------------------
// The run walk: the shape every digest kernel and every message engine
// below has, and the pieces of it that k_crc32_msgs, k_msg_engine_v and
// k_crc32_msgs_b share.  (k_msg_engine_crc, k_crc32_msgs_v,
// k_msg_engine_b and k_msg_engine_sg keep their own bodies: on the
// shared ones they measured slower, docs/PERF.md §8.)
// The work items of a batch (messages, or SGEs) are cut
// into 4 KiB chunks, numbered item-major; a wave owns the contiguous
// chunks [c0, c1), finds the item of c0 once and then only steps
// forward.  A kernel supplies
//  - how the run is sized (wave_run::split: from the launcher, or from
//    the chunk total a scan kernel left in device memory),
//  - how the cursor moves (uni_batch, vl_batch: seek and next),
//  - what opening an item means and what one chunk does,
// and, when it digests, carries a crc_run through the walk: acc over the
// full chunks, flush when the item or the run ends, the workgroup merge
// of the shares of runs that ended inside a message.

struct wave_run {
  uint32_t lane, wv, nwv;  // wv: this wave in the workgroup, of nwv
  uint64_t wave, nwaves;   // ... and in the grid
  uint64_t c0, c1;

  // The launcher chose the run length (run > 0).  Waves past the end get
  // an empty run and still join the merge.
  __device__ __forceinline__ void split(uint64_t total, uint64_t run) {
    c0 = wave * run;
    if (c0 > total) c0 = total;
    c1 = (total - c0 < run) ? total : c0 + run;
  }
  // Equal runs over a total only the device knows.
  __device__ __forceinline__ void split(uint64_t total) {
    rocp2p_vl_run(total, nwaves, wave, &c0, &c1);
  }
};

// The wave index is made provably uniform, so the cursor and the
// descriptors it loads live in SGPRs.  nwv = blockDim.x / WAVE, which
// the kernel itself has to read: only in a __global__ function does the
// compiler fold the block size to one scalar load of a kernel argument;
// read in a helper it is a vector load that every wave waits for before
// it knows its run.
__device__ __forceinline__ wave_run wave_run_open(uint32_t nwv) {
  wave_run w;
  w.lane = threadIdx.x & (WAVE - 1);
  w.wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  w.nwv = nwv;
  w.wave = (uint64_t)blockIdx.x * nwv + w.wv;
  w.nwaves = (uint64_t)gridDim.x * nwv;
  w.c0 = w.c1 = 0;
  return w;
}

// Every item has msg_bytes bytes and so cpm = ceil(msg_bytes / 4096)
// chunks: the cursor is a divide and a wrap.
struct uni_batch {
  uint64_t msg_bytes, cpm;
  __device__ __forceinline__ void seek(rocp2p_vl_cursor* cur,
                                       uint64_t c) const {
    cur->m = c / cpm;
    cur->ci = c - cur->m * cpm;
    cur->cpm = cpm;
    cur->len = msg_bytes;
  }
  __device__ __forceinline__ bool next(rocp2p_vl_cursor* cur) const {
    if (++cur->ci < cpm) return false;
    cur->m++;
    cur->ci = 0;
    return true;
  }
};

// Items carry their own lengths; cstart holds the chunk prefix sums a
// scan kernel wrote (p2p_varlen.h).
struct vl_batch {
  const uint64_t* cstart;
  const uint64_t* lens;
  uint64_t n;
  __device__ __forceinline__ void seek(rocp2p_vl_cursor* cur,
                                       uint64_t c) const {
    rocp2p_vl_seek(cur, cstart, lens, n, c);
  }
  __device__ __forceinline__ bool next(rocp2p_vl_cursor* cur) const {
    return rocp2p_vl_next(cur, cstart, lens);
  }
};

// XOR-reduce x over the wave, shift the sum by `tail` more bytes (the
// shift is linear: applied once, to the sum) and XOR it into *digest.
__device__ __forceinline__ void crc_wave_emit(uint32_t x, uint64_t tail,
                                              uint32_t lane,
                                              uint32_t* digest) {
  for (unsigned o = WAVE / 2; o; o >>= 1) x ^= __shfl_xor(x, o, WAVE);
  if (tail) x = rocp2p_crc_mulmod(crc_xpow_wave(tail, lane), x);
  if (lane == 0) atomicXor(digest, x);
}

// Merge the pending shares (runs that ended inside a message) of a
// workgroup's waves.  Adjacent waves own adjacent runs, so in a long
// message the whole workgroup's pending shares target one digest and
// equal targets are adjacent: XOR them and issue one atomic instead of
// one per wave (same-line atomics serialize in L2).  s_pend: 2 * nwv
// words of LDS that are dead by now (the tables' first words); the
// caller has passed the barrier that says so.
__device__ __forceinline__ void crc_merge_pending(uint32_t* s_pend,
                                                  uint32_t lane, uint32_t wv,
                                                  uint32_t nwv, uint32_t pend_f,
                                                  uint32_t pend_m,
                                                  uint32_t* __restrict__ out) {
  if (lane == 0) {
    s_pend[2 * wv] = pend_f;
    s_pend[2 * wv + 1] = pend_m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = s_pend[0], fm = s_pend[1];
    for (uint32_t w = 1; w < nwv; w++) {
      if (s_pend[2 * w + 1] != fm) {
        if (f) atomicXor(&out[fm], f);
        f = 0;
        fm = s_pend[2 * w + 1];
      }
      f ^= s_pend[2 * w];
    }
    if (f) atomicXor(&out[fm], f);
  }
}

// The CRC a wave carries through its run.
struct crc_run {
  uint32_t acc = 0;  // crc of this run's full chunks of the item so far
  // contribution of a run that ends inside a message: merged with the
  // workgroup's other waves (0 contributes nothing)
  uint32_t pend_f = 0, pend_m = 0;

  // acc = crc(chunks so far || one more 4 KiB chunk)
  __device__ __forceinline__ void full_chunk(const crc_lds& t, uint32_t crc) {
    acc = rocp2p_crc_apply(t.shift[5], rocp2p_crc_apply(t.shift[5], acc)) ^
          crc;
  }

  // After every chunk.  acc leaves the wave when the item ends, when the
  // run ends, or when the chunk just done was not a full one (!full: its
  // bytes went straight to the digest and acc does not cover them).
  // `behind`: the message bytes after those acc covers; `key`: the
  // digest they belong to.  A run that ends inside an item parks its
  // share for merge().
  __device__ __forceinline__ void flush(bool item_end, bool run_end, bool full,
                                        uint64_t behind, uint32_t key,
                                        uint32_t lane,
                                        uint32_t* __restrict__ out) {
    if (item_end || run_end || !full) {
      if (acc) {  // a zero CRC contributes nothing wherever it sits
        uint32_t f = acc;
        if (behind) f = rocp2p_crc_mulmod(crc_xpow_wave(behind, lane), acc);
        if (run_end && !item_end) {
          pend_f = f;
          pend_m = key;
        } else if (lane == 0) {
          atomicXor(&out[key], f);
        }
      }
      acc = 0;
    }
  }

  // After the walk, by every wave of the workgroup: the barrier that
  // says the tables are dead, then the merge.
  __device__ __forceinline__ void merge(uint32_t* s_pend, const wave_run& w,
                                        uint32_t* __restrict__ out) const {
    __syncthreads();
    crc_merge_pending(s_pend, w.lane, w.wv, w.nwv, pend_f, pend_m, out);
  }
};

// The digest walk over messages cut from their own start: message m is
// the cur.len bytes at where(m).
template <typename Batch, typename Where>
__device__ __forceinline__ void crc32_msgs_walk(crc_lds& s, const wave_run& w,
                                                const Batch& batch,
                                                Where where,
                                                uint32_t* __restrict__ out) {
  crc_run crc;
  if (w.c0 < w.c1) {
    rocp2p_vl_cursor cur;
    batch.seek(&cur, w.c0);
    const uint8_t* mp = where(cur.m);
    for (uint64_t c = w.c0; c < w.c1; c++) {
      const uint64_t pos = cur.ci * PAGE;
      const uint64_t left = cur.len - pos;  // > 0
      const uint8_t* seg = mp + pos + w.lane * SEG;
      uint64_t done;  // message bytes [.., done) are covered by acc
      if (left >= PAGE) {
        crc.full_chunk(s, crc_page(seg, w.lane, s));
        done = pos + PAGE;
      } else {
        crc_wave_emit(crc_chunk_partial(s, seg, (uint32_t)left, w.lane), 0,
                      w.lane, &out[cur.m]);
        done = pos;  // acc (if any) still has `left` bytes after it
      }
      // a partial chunk is a message's last: the general rule's !full
      // never adds anything here
      crc.flush(cur.ci + 1 == cur.cpm, c + 1 == w.c1, true, cur.len - done,
                (uint32_t)cur.m, w.lane, out);
      if (c + 1 < w.c1 && batch.next(&cur)) mp = where(cur.m);
    }
  }
  crc.merge(&s.slice[0][0], w, out);
}

// One wave per run of `run` consecutive chunks; CRC_DIGEST_WAVES waves
// per workgroup share one copy of the tables.
// Message m starts at base + (offs ? offs[m] : m * msg_bytes); cpm =
// chunks per message = ceil(msg_bytes / 4096); total = n * cpm.
#define CRC_DIGEST_WAVES 16u
__global__ void __launch_bounds__(WAVE * CRC_DIGEST_WAVES) k_crc32_msgs(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ offs,
    uint64_t msg_bytes, uint64_t cpm, uint64_t total, uint64_t run,
    uint32_t* __restrict__ out) {
  __shared__ crc_lds s;
  crc_stage_tables(s);
  wave_run w = wave_run_open(blockDim.x / WAVE);
  w.split(total, run);
  crc32_msgs_walk(
      s, w, uni_batch{msg_bytes, cpm},
      [&](uint64_t m) { return base + (offs ? offs[m] : m * msg_bytes); },
      out);
}

// ---------------------------------------------------------------------
// Message engine with inline ICRC: moves the batch like k_msg_engine and
// digests every message from the registers the bytes pass through, the
// way an HCA checks a packet's ICRC while the data goes by.  The digest
// is of the bytes AS LOADED (over the link for GATHER); what later sits
// in HBM is crc32_messages' business.
//
// Work split, running CRC, end-of-run shift and the workgroup merge are
// the run walk's (above).  What differs from the digest kernels is the
// chunk layout: a lane of a full 4 KiB chunk holds the 16-byte pieces
// l, l+64, l+128, l+192, so every wave load/store is one contiguous
// 1 KiB access — the shape the plain engine's PCIe rate was measured
// with (crc_page's 64 B per lane would make each wave load 64 separate
// 16-byte PCIe reads).  Piece
// q = 64u + l has 1024(3-u) + 16(63-l) bytes of the chunk after it, and
// shifts commute: a lane Horner-folds its four piece CRCs with the
// 1 KiB operator (shift[4]), then one log tree over the lanes with the
// operators 16 B << k (shift16[0..1], shift[0..3]) finishes the chunk.
// A partial chunk (16..4080 bytes, a multiple of 16) neither loads nor
// stores a piece at or past the message end; every valid piece is
// shifted by the bytes that really follow it and the wave XOR-reduces.

// The 40 KiB a workgroup of the inline-ICRC engine keeps in LDS.
struct icrc_lds {
  crc_lds t;
  uint32_t shift16[2][4][256];
};

// crc_stage_tables plus the 16- and 32-byte operators
__device__ __forceinline__ void icrc_stage_tables(icrc_lds& s) {
  for (uint32_t i = threadIdx.x; i < 2 * 4 * 256; i += blockDim.x)
    (&s.shift16[0][0][0])[i] = (&c_crc.shift16[0][0][0])[i];
  crc_stage_tables(s.t);
}

// zlib crc32 of one 16-byte piece
__device__ __forceinline__ uint32_t crc_piece16(const rocp2p_crc_tab256* t,
                                                const uint4& v) {
  uint32_t crc = rocp2p_crc_step8(t, 0xFFFFFFFFu, v.x, v.y);
  return rocp2p_crc_step8(t, crc, v.z, v.w) ^ 0xFFFFFFFFu;
}

// zlib crc32 of a full 4 KiB chunk held the engine's way (lane l: pieces
// l, l+64, l+128, l+192), in every lane.
__device__ __forceinline__ uint32_t icrc_chunk_full(const icrc_lds& s,
                                                    const uint4& v0,
                                                    const uint4& v1,
                                                    const uint4& v2,
                                                    const uint4& v3,
                                                    uint32_t lane) {
  uint32_t crc = crc_piece16(s.t.slice, v0);
  crc = rocp2p_crc_apply(s.t.shift[4], crc) ^ crc_piece16(s.t.slice, v1);
  crc = rocp2p_crc_apply(s.t.shift[4], crc) ^ crc_piece16(s.t.slice, v2);
  crc = rocp2p_crc_apply(s.t.shift[4], crc) ^ crc_piece16(s.t.slice, v3);
  // lane tree: level k merges adjacent spans of 16 B << k
#pragma unroll
  for (int k = 0; k < 6; k++) {
    uint32_t partner = __shfl_xor(crc, 1u << k, WAVE);
    bool is_left = ((lane >> k) & 1u) == 0;
    uint32_t cl = is_left ? crc : partner;
    uint32_t cr = is_left ? partner : crc;
    crc = rocp2p_crc_apply(k < 2 ? s.shift16[k] : s.t.shift[k - 2], cl) ^ cr;
  }
  return crc;
}

// The plain form keeps nothing in LDS.
template <bool ICRC>
struct vl_engine_lds {};
template <>
struct vl_engine_lds<true> {
  icrc_lds t;
};

// The message engine over lengths that are multiples of 16, with (ICRC)
// or without the inline digest: one walk, so both forms move bytes the
// same way — 1 KiB-contiguous wave accesses, lane l holding pieces l,
// l+64, l+128, l+192 of a chunk.  Without ICRC no table is staged and
// no CRC work is done.
#define ICRC_WAVES 4u
template <bool GATHER, bool ICRC, typename Batch>
__device__ __forceinline__ void msg_engine_walk(
    vl_engine_lds<ICRC>& s, const wave_run& w, const Batch& batch,
    uint8_t* __restrict__ region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ addrs, uint32_t* __restrict__ out) {
  const uint32_t lane = w.lane;
  crc_run crc;
  if (w.c0 < w.c1) {
    rocp2p_vl_cursor cur;
    // this message on the side that is read and on the side that is written
    const uint8_t* from = nullptr;
    uint8_t* to = nullptr;
    auto open_msg = [&](uint64_t msg) {
      uint8_t* inside = region + offs[msg];
      uint8_t* outside = reinterpret_cast<uint8_t*>(addrs[msg]);
      from = GATHER ? outside : inside;
      to = GATHER ? inside : outside;
    };
    batch.seek(&cur, w.c0);
    open_msg(cur.m);

    for (uint64_t c = w.c0; c < w.c1; c++) {
      const uint64_t pos = cur.ci * PAGE;
      const uint64_t left = cur.len - pos;  // > 0, a multiple of 16
      const uint4* src = reinterpret_cast<const uint4*>(from + pos);
      uint4* dst = reinterpret_cast<uint4*>(to + pos);
      uint64_t done;  // message bytes [.., done) are covered by acc
      if (left >= PAGE) {
        // four named registers, not an array: the plain form would
        // otherwise get the array promoted to LDS
        const uint4 v0 = src[lane], v1 = src[lane + WAVE];
        const uint4 v2 = src[lane + 2 * WAVE], v3 = src[lane + 3 * WAVE];
        dst[lane] = v0;
        dst[lane + WAVE] = v1;
        dst[lane + 2 * WAVE] = v2;
        dst[lane + 3 * WAVE] = v3;
        if constexpr (ICRC)
          crc.full_chunk(s.t.t, icrc_chunk_full(s.t, v0, v1, v2, v3, lane));
        done = pos + PAGE;
      } else {
        const uint32_t valid = (uint32_t)left;  // 16..4080
        const uint32_t nvec = valid / 16;
        uint32_t x = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
          const uint32_t q = lane + WAVE * u;
          if (q < nvec) {
            uint4 v = src[q];
            dst[q] = v;
            if constexpr (ICRC)
              x ^= rocp2p_crc_mulmod(
                  rocp2p_crc_xpow8(valid - 16 * (q + 1), c_crc.xpow8),
                  crc_piece16(s.t.t.slice, v));
          }
        }
        if constexpr (ICRC) crc_wave_emit(x, 0, lane, &out[cur.m]);
        done = pos;  // acc (if any) still has `valid` bytes after it
      }
      if constexpr (ICRC)
        crc.flush(cur.ci + 1 == cur.cpm, c + 1 == w.c1, true, cur.len - done,
                  (uint32_t)cur.m, lane, out);
      if (c + 1 < w.c1 && batch.next(&cur)) open_msg(cur.m);
    }
  }
  if constexpr (ICRC) crc.merge(&s.t.t.slice[0][0], w, out);
}

// Uniform msg_bytes per batch; run length from the launcher.
template <bool GATHER>
__global__ void __launch_bounds__(WAVE * ICRC_WAVES) k_msg_engine_crc(
    uint8_t* __restrict__ region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ addrs, uint64_t msg_bytes, uint64_t cpm,
    uint64_t total, uint64_t run, uint32_t* __restrict__ out) {
  __shared__ icrc_lds s;
  for (uint32_t i = threadIdx.x; i < 2 * 4 * 256; i += blockDim.x)
    (&s.shift16[0][0][0])[i] = (&c_crc.shift16[0][0][0])[i];
  crc_stage_tables(s.t);

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE, nwv = blockDim.x / WAVE;
  const uint64_t wave = (uint64_t)blockIdx.x * nwv + wv;
  uint64_t c0 = wave * run;
  if (c0 > total) c0 = total;  // idle wave: empty run, still joins the merge
  const uint64_t c1 = (total - c0 < run) ? total : c0 + run;

  uint64_t m = 0, ci = 0;
  // this message on the side that is read and on the side that is written
  const uint8_t* from = nullptr;
  uint8_t* to = nullptr;
  auto open_msg = [&](uint64_t msg) {
    uint8_t* inside = region + offs[msg];
    uint8_t* outside = reinterpret_cast<uint8_t*>(addrs[msg]);
    from = GATHER ? outside : inside;
    to = GATHER ? inside : outside;
  };
  if (c0 < c1) {
    m = c0 / cpm;
    ci = c0 - m * cpm;
    open_msg(m);
  }
  uint32_t acc = 0;  // crc of this run's full chunks of message m so far
  uint32_t pend_f = 0, pend_m = 0;

  for (uint64_t c = c0; c < c1; c++) {
    const uint64_t pos = ci * PAGE;
    const uint64_t left = msg_bytes - pos;  // > 0, a multiple of 16
    const uint4* src = reinterpret_cast<const uint4*>(from + pos);
    uint4* dst = reinterpret_cast<uint4*>(to + pos);
    uint64_t done;  // message bytes [.., done) are covered by acc
    if (left >= PAGE) {
      uint4 v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) v[u] = src[lane + WAVE * u];
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) dst[lane + WAVE * u] = v[u];
      uint32_t crc = crc_piece16(s.t.slice, v[0]);
#pragma unroll
      for (uint32_t u = 1; u < 4; u++)
        crc = rocp2p_crc_apply(s.t.shift[4], crc) ^
              crc_piece16(s.t.slice, v[u]);
      // lane tree: level k merges adjacent spans of 16 B << k
#pragma unroll
      for (int k = 0; k < 6; k++) {
        uint32_t partner = __shfl_xor(crc, 1u << k, WAVE);
        bool is_left = ((lane >> k) & 1u) == 0;
        uint32_t cl = is_left ? crc : partner;
        uint32_t cr = is_left ? partner : crc;
        crc = rocp2p_crc_apply(k < 2 ? s.shift16[k] : s.t.shift[k - 2], cl) ^
              cr;
      }
      acc = rocp2p_crc_apply(s.t.shift[5],
                             rocp2p_crc_apply(s.t.shift[5], acc)) ^ crc;
      done = pos + PAGE;
    } else {
      const uint32_t valid = (uint32_t)left;  // 16..4080
      const uint32_t nvec = valid / 16;
      uint32_t x = 0;
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) {
        const uint32_t q = lane + WAVE * u;
        if (q < nvec) {
          uint4 v = src[q];
          dst[q] = v;
          x ^= rocp2p_crc_mulmod(
              rocp2p_crc_xpow8(valid - 16 * (q + 1), c_crc.xpow8),
              crc_piece16(s.t.slice, v));
        }
      }
      for (unsigned o = WAVE / 2; o; o >>= 1) x ^= __shfl_xor(x, o, WAVE);
      if (lane == 0) atomicXor(&out[m], x);
      done = pos;  // acc (if any) still has `valid` bytes after it
    }
    const bool msg_end = ci + 1 == cpm;
    if (msg_end || c + 1 == c1) {
      if (acc) {  // a zero CRC contributes nothing wherever it sits
        const uint64_t r = msg_bytes - done;
        uint32_t f = acc;
        if (r) f = rocp2p_crc_mulmod(crc_xpow_wave(r, lane), acc);
        if (msg_end) {
          if (lane == 0) atomicXor(&out[m], f);
        } else {
          pend_f = f;
          pend_m = (uint32_t)m;
        }
      }
      acc = 0;
    }
    if (msg_end) {
      m++;
      ci = 0;
      if (c + 1 < c1) open_msg(m);
    } else {
      ci++;
    }
  }

  __syncthreads();  // the tables are dead: their first words hand off
  crc_merge_pending(&s.t.slice[0][0], lane, wv, nwv, pend_f, pend_m, out);
}

// ---------------------------------------------------------------------
// Variable-length batches: every message carries its own byte count
// (lens[m], device memory, 0 allowed), as every verbs work request does.
// The unit of work is still the 4 KiB chunk, numbered message-major, and
// each wave still owns a contiguous run of chunks; what changes is that
// chunks-per-message varies, so "chunk / cpm" is gone.  k_vl_scan first
// writes cstart[m] = chunks before message m and cstart[n] = the total
// (p2p_varlen.h); the main kernels read the total from there — the host
// never learns it — derive their run length from it, find the message of
// their first chunk with ONE binary search of cstart and then only step
// forward.  Zero-length messages have an empty chunk range: the cursor
// steps over them and they never reach a load, a store or an atomic
// (their digest is the 0 the launcher wrote, zlib's crc32(b"")).
// 16-byte and multi-MiB messages side by side cost what their chunks
// cost: a run boundary may fall anywhere, inside a big message or after
// any number of tiny ones.

// A scan of value(0 .. count - 1) by one workgroup of 16 waves; wave w
// owns a contiguous segment of the items (a whole number of 64-item
// tiles, so any count fits and every tile is one coalesced access).
// Pass 1 sums the segment, one barrier hands the 16 sums over, pass 2
// walks the segment tile by tile with a wave scan and a running carry —
// no barrier inside either loop.  PARK keeps the values in out between
// the passes so that value() runs once per item (the same lane owns an
// item in both passes); a value() that is two loads and a shift is
// cheaper run twice.  Sums (MAX false) are exclusive, out[0 .. count]
// with the total last; running maxima (MAX true) are inclusive,
// out[0 .. count).  A PARK scan ends with a barrier — out is complete
// and s_wave free for the scan that follows; a kernel that is one scan
// just ends.
#define VL_SCAN_THREADS 1024u
template <bool MAX, bool PARK, typename T, typename F>
__device__ __forceinline__ void block_scan(F value, uint64_t count, T* out,
                                           T* s_wave) {
  auto op = [](T a, T b) { return MAX ? (a > b ? a : b) : (T)(a + b); };
  const uint32_t lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const uint64_t per = (count + VL_SCAN_THREADS - 1) / VL_SCAN_THREADS * WAVE;
  const uint64_t b = min(wv * per, count);
  const uint64_t e = min(b + per, count);
  T sum = 0;
  for (uint64_t i = b + lane; i < e; i += WAVE) {
    const T k = value(i);
    if (PARK) out[i] = k;
    sum = op(sum, k);
  }
  for (uint32_t o = WAVE / 2; o; o >>= 1)
    sum = op(sum, __shfl_xor(sum, o, WAVE));
  if (lane == 0) s_wave[wv] = sum;
  __syncthreads();
  T at = 0;  // what the items before the tile at hand amount to
  for (uint32_t w = 0; w < wv; w++) at = op(at, s_wave[w]);
  for (uint64_t i0 = b; i0 < e; i0 += WAVE) {  // uniform trip count
    const uint64_t i = i0 + lane;
    const T k = i < e ? (PARK ? out[i] : value(i)) : 0;
    T inc = k;  // inclusive scan over the tile
    for (uint32_t o = 1; o < WAVE; o <<= 1) {
      T v = __shfl_up(inc, o, WAVE);
      if (lane >= o) inc = op(inc, v);
    }
    if (i < e) out[i] = MAX ? op(at, inc) : (T)(at + inc - k);
    at = op(at, __shfl(inc, WAVE - 1, WAVE));
  }
  // the last wave's segment ends at count: its carry is the total
  if (!MAX && threadIdx.x == VL_SCAN_THREADS - 1) out[count] = at;
  if (PARK) __syncthreads();
}

__global__ void __launch_bounds__(VL_SCAN_THREADS) k_vl_scan(
    const uint64_t* __restrict__ lens, uint32_t n,
    uint64_t* __restrict__ cstart) {
  __shared__ uint64_t s_wave[VL_SCAN_THREADS / WAVE];
  block_scan<false, false>(
      [&](uint64_t i) { return rocp2p_vl_chunks(lens[i]); }, n, cstart,
      s_wave);
}

// The message engine for per-message lengths (multiples of 16).
template <bool GATHER, bool ICRC>
__global__ void __launch_bounds__(WAVE * ICRC_WAVES) k_msg_engine_v(
    uint8_t* __restrict__ region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ addrs, const uint64_t* __restrict__ lens,
    const uint64_t* __restrict__ cstart, uint32_t n,
    uint32_t* __restrict__ out) {
  __shared__ vl_engine_lds<ICRC> s;
  if constexpr (ICRC) icrc_stage_tables(s.t);
  wave_run w = wave_run_open(blockDim.x / WAVE);
  w.split(cstart[n]);
  msg_engine_walk<GATHER, ICRC>(s, w, vl_batch{cstart, lens, n}, region, offs,
                                addrs, out);
}

// k_crc32_msgs for per-message lengths (any byte count, 0 included):
// message m is base[offs[m], offs[m] + lens[m]).
__global__ void __launch_bounds__(WAVE * CRC_DIGEST_WAVES) k_crc32_msgs_v(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ lens, const uint64_t* __restrict__ cstart,
    uint32_t n, uint32_t* __restrict__ out) {
  __shared__ crc_lds s;
  crc_stage_tables(s);

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t nwv = blockDim.x / WAVE;
  uint64_t c0, c1;
  rocp2p_vl_run(cstart[n], (uint64_t)gridDim.x * nwv,
                (uint64_t)blockIdx.x * nwv + wv, &c0, &c1);

  rocp2p_vl_cursor cur = {0, 0, 0, 0};
  const uint8_t* mp = base;
  if (c0 < c1) {
    rocp2p_vl_seek(&cur, cstart, lens, n, c0);
    mp = base + offs[cur.m];
  }
  uint32_t acc = 0;  // crc of this run's full chunks of message m so far
  uint32_t pend_f = 0, pend_m = 0;

  for (uint64_t c = c0; c < c1; c++) {
    const uint64_t pos = cur.ci * PAGE;
    const uint64_t left = cur.len - pos;  // > 0
    const uint8_t* seg = mp + pos + lane * SEG;
    uint64_t done;  // message bytes [.., done) are covered by acc
    if (left >= PAGE) {
      acc = rocp2p_crc_apply(s.shift[5], rocp2p_crc_apply(s.shift[5], acc)) ^
            crc_page(seg, lane, s);
      done = pos + PAGE;
    } else {
      const uint32_t valid = (uint32_t)left;  // 1..4095
      const uint32_t beg = lane * SEG;
      const uint32_t nb = valid > beg ? min(valid - beg, SEG) : 0u;
      uint32_t w[16];
      crc_load_partial(seg, nb, w);
      uint32_t x = 0;
      if (nb)
        x = rocp2p_crc_mulmod(
            rocp2p_crc_xpow8(valid - (beg + nb), c_crc.xpow8),
            crc_bytes64(s.slice, w, nb));
      for (unsigned o = WAVE / 2; o; o >>= 1) x ^= __shfl_xor(x, o, WAVE);
      if (lane == 0) atomicXor(&out[cur.m], x);
      done = pos;  // acc (if any) still has `valid` bytes after it
    }
    const bool msg_end = cur.ci + 1 == cur.cpm;
    if (msg_end || c + 1 == c1) {
      if (acc) {  // a zero CRC contributes nothing wherever it sits
        const uint64_t r = cur.len - done;
        uint32_t f = acc;
        if (r) f = rocp2p_crc_mulmod(crc_xpow_wave(r, lane), acc);
        if (msg_end) {
          if (lane == 0) atomicXor(&out[cur.m], f);
        } else {
          pend_f = f;
          pend_m = (uint32_t)cur.m;
        }
      }
      acc = 0;
    }
    if (c + 1 < c1 && rocp2p_vl_next(&cur, cstart, lens))
      mp = base + offs[cur.m];
  }

  __syncthreads();  // the tables are dead: their first words hand off
  crc_merge_pending(&s.slice[0][0], lane, wv, nwv, pend_f, pend_m, out);
}

// ---------------------------------------------------------------------
// Byte-granular batches: lens[m] is any byte count and both addresses of
// a message are any byte address, as an RDMA write's are.  The geometry
// is p2p_bytes.h's: a message is cut on the 16-byte granule grid of the
// side that is WRITTEN, a chunk is 256 of those granules, and the chunk
// count therefore depends on the store-side skew (dst & 15) as well as
// on the length — k_vl_scan_b reads both.  Runs, the one binary search,
// the forward cursor, the running CRC, the end-of-run shift and the
// pending-share merge are the run walk's, unchanged.
//
// The side that is read is loaded as aligned 16-byte granules too and
// realigned in registers by rel = (src - dst) & 15, which is uniform
// per message: rel == 0 is a scalar branch to load-and-store.  Otherwise
// store granule q is cut from source granules q and q + 1; a lane takes
// q + 1 from the next lane, lane 63 from lane 0's next piece, and lane 0
// loads the one granule (256) the chunk needs beyond its own — every
// source granule crosses the link once per chunk, in the same 1 KiB
// contiguous wave loads as before.
//
// A chunk takes whole-granule accesses only if it is full on BOTH sides
// (rocp2p_b_full): with rel != 0 a chunk whose store granules all lie
// inside the message may still be cut from a source granule that holds
// bytes in front of or behind the message.  Every other chunk — at most
// the first one and the last two of a message — takes the same route
// with ranged accesses: a granule is loaded and stored only in the bytes
// [lo, hi) that belong to the message, with naturally aligned 1-, 2-, 4-
// and 8-byte accesses, never a read-modify-write (the rest of the
// granule may be a neighbouring message that another wave is writing).
// A granule outside the message is not touched at all.
//
// ICRC: crc(A || B) = shift(crc(A), |B|) ^ crc(B) holds for any cut, so
// the granule grid serves as well as the 16-bytes-from-the-start grid.
// Full chunks go through icrc_chunk_full on the realigned registers;
// every granule of another chunk contributes the CRC of its valid bytes
// shifted by the message bytes behind them, straight into the digest.
// acc covers full chunks only and is flushed before anything else of
// the message is accounted for.
//
// Scatter/gather lists (geometry: p2p_sgl.h) run on the same walk with
// the SGE as the work item.  A message is the concatenation of its
// SGEs: a gather reads them from anywhere outside and writes them back
// to back into the region, a scatter cuts the contiguous region range
// over them.  A scan kernel (k_sg_scan) turns the lists into what the
// walk takes per item — the address written, the address read, the
// length, the chunk prefix sums — plus the two things only the digest
// needs: the message that owns the SGE and the message bytes behind it
// (its tail).  Consecutive SGEs of a message meet inside a granule of
// the region like neighbouring messages do, which the narrow stores of
// p2p_bytes.h already allow.  A CRC piece of SGE j is shifted by the
// bytes behind it in the SGE and by tail[j] more, and is XORed into
// out[owner[j]]; the pending merge keys on the owner as well (owners
// are nondecreasing in the SGE index, so equal targets stay adjacent).
// A message without SGEs, and an SGE without bytes, own no chunk and
// reach no load, store or atomic.

// k_vl_scan for the byte-granular grid: where[m] is the address (or the
// offset from a 16-byte-aligned base) message m is written at.
__global__ void __launch_bounds__(VL_SCAN_THREADS) k_vl_scan_b(
    const uint64_t* __restrict__ lens, const uint64_t* __restrict__ where,
    uint32_t n, uint64_t* __restrict__ cstart) {
  __shared__ uint64_t s_wave[VL_SCAN_THREADS / WAVE];
  block_scan<false, false>(
      [&](uint64_t i) {
        return rocp2p_b_chunks((uint32_t)where[i] & 15u, lens[i]);
      },
      n, cstart, s_wave);
}

// The granule the next lane holds; lane 63 gets lane 0's.
__device__ __forceinline__ rocp2p_g16 g16_next_lane(const rocp2p_g16& a,
                                                    uint32_t lane) {
  const int from = (int)((lane + 1) & (WAVE - 1));
  const rocp2p_g16 r = {__shfl(a.x, from, WAVE), __shfl(a.y, from, WAVE),
                        __shfl(a.z, from, WAVE), __shfl(a.w, from, WAVE)};
  return r;
}

// The four store granules of a lane (pieces l, l+64, l+128, l+192) from
// its four source granules and e, the chunk's 257th source granule,
// which lane 0 holds.  The successor of piece 64u + 63 is piece
// 64(u + 1), lane 0's next register.
__device__ __forceinline__ void g16_realign4(
    const rocp2p_g16& a0, const rocp2p_g16& a1, const rocp2p_g16& a2,
    const rocp2p_g16& a3, const rocp2p_g16& e, uint32_t rel, uint32_t lane,
    rocp2p_g16& v0, rocp2p_g16& v1, rocp2p_g16& v2, rocp2p_g16& v3) {
  const rocp2p_g16 r0 = g16_next_lane(a0, lane), r1 = g16_next_lane(a1, lane);
  const rocp2p_g16 r2 = g16_next_lane(a2, lane), r3 = g16_next_lane(a3, lane);
  const rocp2p_g16 r4 = g16_next_lane(e, lane);
  // word by word: a ?: of two structs is a select of their addresses
  // and would put them all in scratch
  const bool last = lane == WAVE - 1;
  auto pick = [last](const rocp2p_g16& wrap, const rocp2p_g16& next) {
    const rocp2p_g16 r = {last ? wrap.x : next.x, last ? wrap.y : next.y,
                          last ? wrap.z : next.z, last ? wrap.w : next.w};
    return r;
  };
  v0 = rocp2p_b_realign(a0, pick(r1, r0), rel);
  v1 = rocp2p_b_realign(a1, pick(r2, r1), rel);
  v2 = rocp2p_b_realign(a2, pick(r3, r2), rel);
  v3 = rocp2p_b_realign(a3, pick(r4, r3), rel);
}

// zlib crc32 of the bytes [lo, hi) of a granule, lo < hi
__device__ __forceinline__ uint32_t crc_granule_range(
    const rocp2p_crc_tab256* t, const rocp2p_g16& v, uint32_t lo,
    uint32_t hi) {
  uint64_t d0 = v.x | ((uint64_t)v.y << 32);
  uint64_t d1 = v.z | ((uint64_t)v.w << 32);
  if (lo >= 8) {
    d0 = d1 >> (8 * (lo - 8));
    d1 = 0;
  } else if (lo) {
    d0 = (d0 >> (8 * lo)) | (d1 << (64 - 8 * lo));
    d1 >>= 8 * lo;
  }
  uint32_t rem = hi - lo, crc = 0xFFFFFFFFu;
  if (rem >= 8) {
    crc = rocp2p_crc_step8(t, crc, (uint32_t)d0, (uint32_t)(d0 >> 32));
    d0 = d1;
    rem -= 8;
  }
  if (rem >= 8) {  // all 16 bytes
    crc = rocp2p_crc_step8(t, crc, (uint32_t)d0, (uint32_t)(d0 >> 32));
    rem -= 8;
  }
  for (; rem; rem--, d0 >>= 8)
    crc = t[0][(crc ^ (uint32_t)d0) & 0xff] ^ (crc >> 8);
  return crc ^ 0xFFFFFFFFu;
}

__device__ __forceinline__ uint4 g16_u4(const rocp2p_g16& v) {
  return make_uint4(v.x, v.y, v.z, v.w);
}

// The message engine for any length at any address, with (ICRC) or
// without the inline digest.  Same launch shape, descriptors and scratch
// as k_msg_engine_v; cstart comes from k_vl_scan_b over the side that is
// written.  Without ICRC no table is staged and no CRC work is done.
// Its own body, not a walk shared with k_msg_engine_sg: on a shared body
// the plain gathers of both measured 1.1-1.6% slower (docs/PERF.md §8).
template <bool GATHER, bool ICRC>
__global__ void __launch_bounds__(WAVE * ICRC_WAVES) k_msg_engine_b(
    uint8_t* __restrict__ region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ addrs, const uint64_t* __restrict__ lens,
    const uint64_t* __restrict__ cstart, uint32_t n,
    uint32_t* __restrict__ out) {
  __shared__ vl_engine_lds<ICRC> s;
  if constexpr (ICRC) {
    for (uint32_t i = threadIdx.x; i < 2 * 4 * 256; i += blockDim.x)
      (&s.t.shift16[0][0][0])[i] = (&c_crc.shift16[0][0][0])[i];
    crc_stage_tables(s.t.t);
  }

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t nwv = blockDim.x / WAVE;
  uint64_t c0, c1;
  rocp2p_vl_run(cstart[n], (uint64_t)gridDim.x * nwv,
                (uint64_t)blockIdx.x * nwv + wv, &c0, &c1);

  rocp2p_vl_cursor cur = {0, 0, 0, 0};
  // This message: where its store stream and its source stream start
  // (both 16-byte aligned, p2p_bytes.h), how far into the store stream
  // it begins, and how much further on it lies in the source stream.
  const uint8_t* from0 = nullptr;
  uint8_t* to0 = nullptr;
  uint32_t skew = 0, rel = 0;
  auto open_msg = [&](uint64_t msg) {
    uint8_t* inside = region + offs[msg];
    uint8_t* outside = reinterpret_cast<uint8_t*>(addrs[msg]);
    const uint8_t* from = GATHER ? outside : inside;
    uint8_t* to = GATHER ? inside : outside;
    skew = (uint32_t)reinterpret_cast<uintptr_t>(to) & 15u;
    rel = (uint32_t)(reinterpret_cast<uintptr_t>(from) -
                     reinterpret_cast<uintptr_t>(to)) & 15u;
    to0 = to - skew;
    from0 = from - skew - rel;
  };
  if (c0 < c1) {
    rocp2p_vl_seek(&cur, cstart, lens, n, c0);
    open_msg(cur.m);
  }
  uint32_t acc = 0;  // crc of this run's full chunks of message m so far
  uint32_t pend_f = 0, pend_m = 0;
  const rocp2p_g16 none = {0, 0, 0, 0};

  for (uint64_t c = c0; c < c1; c++) {
    const uint64_t p0 = cur.ci * PAGE;      // of the store stream
    const uint64_t end = skew + cur.len;    // of the message, likewise
    const uint8_t* sp = from0 + p0;
    uint8_t* dp = to0 + p0;
    const bool full = rocp2p_b_full(skew, rel, cur.len, cur.ci);
    // four named registers, not an array: see msg_engine_walk
    rocp2p_g16 v0, v1, v2, v3;
    uint64_t done;  // store-stream bytes [.., done) are covered by acc
    if (full) {
      const rocp2p_g16* src = reinterpret_cast<const rocp2p_g16*>(sp);
      if (rel == 0) {
        v0 = src[lane];
        v1 = src[lane + WAVE];
        v2 = src[lane + 2 * WAVE];
        v3 = src[lane + 3 * WAVE];
      } else {
        const rocp2p_g16 a0 = src[lane], a1 = src[lane + WAVE];
        const rocp2p_g16 a2 = src[lane + 2 * WAVE], a3 = src[lane + 3 * WAVE];
        rocp2p_g16 e = none;
        if (lane == 0) e = src[4 * WAVE];
        g16_realign4(a0, a1, a2, a3, e, rel, lane, v0, v1, v2, v3);
      }
      rocp2p_g16* dst = reinterpret_cast<rocp2p_g16*>(dp);
      dst[lane] = v0;
      dst[lane + WAVE] = v1;
      dst[lane + 2 * WAVE] = v2;
      dst[lane + 3 * WAVE] = v3;
      if constexpr (ICRC)
        acc = rocp2p_crc_apply(s.t.t.shift[5],
                               rocp2p_crc_apply(s.t.t.shift[5], acc)) ^
              icrc_chunk_full(s.t, g16_u4(v0), g16_u4(v1), g16_u4(v2),
                              g16_u4(v3), lane);
      done = p0 + PAGE;
    } else {
      const uint64_t g0 = cur.ci * ROCP2P_B_PER_CHUNK;
      // the message in the source stream
      const uint64_t sbeg = (uint64_t)skew + rel, send = end + rel;
      auto fetch = [&](uint32_t q) {
        uint32_t lo, hi;
        rocp2p_b_range(sbeg, send, g0 + q, &lo, &hi);
        return rocp2p_b_load(sp + ROCP2P_B_GRAN * q, lo, hi);
      };
      if (rel == 0) {
        v0 = fetch(lane);
        v1 = fetch(lane + WAVE);
        v2 = fetch(lane + 2 * WAVE);
        v3 = fetch(lane + 3 * WAVE);
      } else {
        const rocp2p_g16 a0 = fetch(lane), a1 = fetch(lane + WAVE);
        const rocp2p_g16 a2 = fetch(lane + 2 * WAVE);
        const rocp2p_g16 a3 = fetch(lane + 3 * WAVE);
        rocp2p_g16 e = none;
        if (lane == 0) e = fetch(4 * WAVE);
        g16_realign4(a0, a1, a2, a3, e, rel, lane, v0, v1, v2, v3);
      }
      uint32_t x = 0;
      auto put = [&](uint32_t q, const rocp2p_g16& v) {
        uint32_t lo, hi;
        rocp2p_b_range(skew, end, g0 + q, &lo, &hi);
        if (lo < hi) {
          rocp2p_b_store(dp + ROCP2P_B_GRAN * q, lo, hi, v);
          if constexpr (ICRC)
            x ^= rocp2p_crc_mulmod(
                rocp2p_crc_xpow8(end - ((g0 + q) * ROCP2P_B_GRAN + hi),
                                 c_crc.xpow8),
                crc_granule_range(s.t.t.slice, v, lo, hi));
        }
      };
      put(lane, v0);
      put(lane + WAVE, v1);
      put(lane + 2 * WAVE, v2);
      put(lane + 3 * WAVE, v3);
      if constexpr (ICRC) {
        for (unsigned o = WAVE / 2; o; o >>= 1) x ^= __shfl_xor(x, o, WAVE);
        if (lane == 0) atomicXor(&out[cur.m], x);
      }
      done = p0;  // acc (if any) ends where this chunk begins
    }
    if constexpr (ICRC) {
      const bool msg_end = cur.ci + 1 == cur.cpm;
      const bool run_end = c + 1 == c1;
      if (msg_end || run_end || !full) {
        if (acc) {  // a zero CRC contributes nothing wherever it sits
          const uint64_t r = end - done;
          uint32_t f = acc;
          if (r) f = rocp2p_crc_mulmod(crc_xpow_wave(r, lane), acc);
          if (run_end && !msg_end) {
            pend_f = f;
            pend_m = (uint32_t)cur.m;
          } else if (lane == 0) {
            atomicXor(&out[cur.m], f);
          }
        }
        acc = 0;
      }
    }
    if (c + 1 < c1 && rocp2p_vl_next(&cur, cstart, lens)) open_msg(cur.m);
  }

  if constexpr (ICRC) {
    __syncthreads();  // the tables are dead: their first words hand off
    crc_merge_pending(&s.t.t.slice[0][0], lane, wv, nwv, pend_f, pend_m, out);
  }
}

// k_crc32_msgs_v for messages at any byte offset: message m is
// base[offs[m], offs[m] + lens[m]), cut on the granule grid of
// base + offs[m] (base is 16-byte aligned).  Chunks wholly inside the
// message are aligned and go through crc_page; the first and the last
// chunk use the flat identity over the chunk's valid bytes [lo, hi):
// lane l owns [64l, 64l + 64) ∩ [lo, hi), loaded with rocp2p_b_load.
__global__ void __launch_bounds__(WAVE * CRC_DIGEST_WAVES) k_crc32_msgs_b(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ lens, const uint64_t* __restrict__ cstart,
    uint32_t n, uint32_t* __restrict__ out) {
  __shared__ crc_lds s;
  crc_stage_tables(s);
  wave_run w = wave_run_open(blockDim.x / WAVE);
  w.split(cstart[n]);
  const uint32_t lane = w.lane;
  const vl_batch batch = {cstart, lens, n};

  crc_run crc;
  if (w.c0 < w.c1) {
    rocp2p_vl_cursor cur;
    const uint8_t* mp0 = base;  // where the message's stream starts
    uint32_t skew = 0;
    auto open_msg = [&](uint64_t msg) {
      const uint64_t off = offs[msg];
      skew = (uint32_t)off & 15u;
      mp0 = base + (off - skew);
    };
    batch.seek(&cur, w.c0);
    open_msg(cur.m);

    for (uint64_t c = w.c0; c < w.c1; c++) {
      const uint64_t p0 = cur.ci * PAGE;    // of the message's stream
      const uint64_t end = skew + cur.len;  // of the message, likewise
      const uint8_t* seg = mp0 + p0 + lane * SEG;
      const bool full = rocp2p_b_full(skew, 0, cur.len, cur.ci);
      uint64_t done;  // stream bytes [.., done) are covered by acc
      if (full) {
        crc.full_chunk(s, crc_page(seg, lane, s));
        done = p0 + PAGE;
      } else {
        // the chunk's valid bytes, and this lane's [a, b) of its 64
        const uint32_t lo = p0 < skew ? skew : 0u;  // first chunk only
        const uint32_t hi = (uint32_t)min(end - p0, (uint64_t)PAGE);
        const uint32_t beg = lane * SEG;
        const uint32_t a = lo > beg ? min(lo - beg, SEG) : 0u;  // < 16
        const uint32_t b = hi > beg ? min(hi - beg, SEG) : 0u;
        uint32_t x = 0;
        if (a < b) {
          const uint64_t g0 = cur.ci * ROCP2P_B_PER_CHUNK + lane * 4;
          uint64_t d[9];
#pragma unroll
          for (uint32_t q = 0; q < 4; q++) {
            uint32_t glo, ghi;
            rocp2p_b_range(skew, end, g0 + q, &glo, &ghi);
            const rocp2p_g16 v =
                rocp2p_b_load(seg + ROCP2P_B_GRAN * q, glo, ghi);
            d[2 * q] = v.x | ((uint64_t)v.y << 32);
            d[2 * q + 1] = v.z | ((uint64_t)v.w << 32);
          }
          d[8] = 0;
          if (a) {  // bring byte a down to byte 0
            if (a >= 8) {
#pragma unroll
              for (uint32_t i = 0; i < 8; i++) d[i] = d[i + 1];
            }
            const uint32_t sh = 8 * (a & 7);
            if (sh) {
#pragma unroll
              for (uint32_t i = 0; i < 8; i++)
                d[i] = (d[i] >> sh) | (d[i + 1] << (64 - sh));
            }
          }
          uint32_t wd[16];
#pragma unroll
          for (uint32_t i = 0; i < 8; i++) {
            wd[2 * i] = (uint32_t)d[i];
            wd[2 * i + 1] = (uint32_t)(d[i] >> 32);
          }
          x = rocp2p_crc_mulmod(
              rocp2p_crc_xpow8(end - (p0 + beg + b), c_crc.xpow8),
              crc_bytes64(s.slice, wd, b - a));
        }
        crc_wave_emit(x, 0, lane, &out[cur.m]);
        done = p0;  // acc (if any) ends where this chunk begins
      }
      crc.flush(cur.ci + 1 == cur.cpm, c + 1 == w.c1, full, end - done,
                (uint32_t)cur.m, lane, out);
      if (c + 1 < w.c1 && batch.next(&cur)) open_msg(cur.m);
    }
  }
  crc.merge(&s.slice[0][0], w, out);
}

// ---------------------------------------------------------------------
// The scan pass of a scatter/gather batch: one workgroup, one launch.
// Owners first: every message with SGEs writes its number at its first
// SGE and a running maximum spreads it over the others (message numbers
// grow with the SGE index) — no search per SGE.  Then the byte prefix
// sums P, and last every SGE's work item from P (rocp2p_sgl_item) and
// the chunk prefix sums.  nsge > 0.
template <bool GATHER>
__global__ void __launch_bounds__(VL_SCAN_THREADS) k_sg_scan(
    const uint8_t* region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ sge_start,
    const uint64_t* __restrict__ sge_addrs,
    const uint64_t* __restrict__ sge_lens, uint32_t n, uint32_t nsge,
    uint64_t* scratch) {
  __shared__ uint64_t s_wave[VL_SCAN_THREADS / WAVE];
  __shared__ uint32_t s_own[VL_SCAN_THREADS / WAVE];
  const rocp2p_sgl_view v = rocp2p_sgl_carve(scratch, nsge);
  for (uint32_t j = threadIdx.x; j < nsge; j += VL_SCAN_THREADS)
    v.owner[j] = 0;
  __syncthreads();
  for (uint32_t m = threadIdx.x; m < n; m += VL_SCAN_THREADS)
    if (rocp2p_sgl_has_sges(sge_start, m)) v.owner[sge_start[m]] = m;
  __syncthreads();
  block_scan<true, true>([&](uint64_t j) { return v.owner[j]; }, nsge,
                         v.owner, s_own);
  block_scan<false, true>([&](uint64_t j) { return sge_lens[j]; }, nsge,
                          v.prefix, s_wave);
  const uint64_t base = reinterpret_cast<uintptr_t>(region);
  block_scan<false, true>(
      [&](uint64_t j) {
        return rocp2p_sgl_item(v, base, offs, sge_start, sge_addrs, j,
                               GATHER);
      },
      nsge, v.cstart, s_wave);
}

// k_msg_engine_b with the SGE as its work item: the same launch shape,
// run split, cursor and chunk bodies, over the nsge SGEs that k_sg_scan
// laid out in scratch (rocp2p_sgl_view).  The scan has resolved the
// direction (to / from are addresses), so a gather and a scatter are the
// same code here.  Every CRC contribution carries the SGE's tail as a
// further shift and goes to the digest of the owning message; the
// pending merge keys on the owner as well.  Without ICRC no table is
// staged and no CRC work is done.
template <bool ICRC>
__global__ void __launch_bounds__(WAVE * ICRC_WAVES) k_msg_engine_sg(
    const uint64_t* __restrict__ sge_lens, const uint64_t* __restrict__ cstart,
    const uint64_t* __restrict__ sge_to, const uint64_t* __restrict__ sge_from,
    const uint64_t* __restrict__ sge_tail,
    const uint32_t* __restrict__ sge_owner, uint32_t nsge,
    uint32_t* __restrict__ out) {
  __shared__ vl_engine_lds<ICRC> s;
  if constexpr (ICRC) {
    for (uint32_t i = threadIdx.x; i < 2 * 4 * 256; i += blockDim.x)
      (&s.t.shift16[0][0][0])[i] = (&c_crc.shift16[0][0][0])[i];
    crc_stage_tables(s.t.t);
  }

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t nwv = blockDim.x / WAVE;
  uint64_t c0, c1;
  rocp2p_vl_run(cstart[nsge], (uint64_t)gridDim.x * nwv,
                (uint64_t)blockIdx.x * nwv + wv, &c0, &c1);

  rocp2p_vl_cursor cur = {0, 0, 0, 0};  // cur.m is an SGE here
  // This SGE: its store and source streams as in k_msg_engine_b, the
  // message bytes behind it and the message it belongs to.
  const uint8_t* from0 = nullptr;
  uint8_t* to0 = nullptr;
  uint32_t skew = 0, rel = 0, owner = 0;
  uint64_t tail = 0;
  auto open_sge = [&](uint64_t j) {
    const uint64_t to = sge_to[j], from = sge_from[j];
    skew = (uint32_t)to & 15u;
    rel = (uint32_t)(from - to) & 15u;
    to0 = reinterpret_cast<uint8_t*>(to - skew);
    from0 = reinterpret_cast<const uint8_t*>(from - skew - rel);
    if constexpr (ICRC) {
      tail = sge_tail[j];
      owner = sge_owner[j];
    }
  };
  if (c0 < c1) {
    rocp2p_vl_seek(&cur, cstart, sge_lens, nsge, c0);
    open_sge(cur.m);
  }
  uint32_t acc = 0;  // crc of this run's full chunks of SGE cur.m so far
  uint32_t pend_f = 0, pend_m = 0;
  const rocp2p_g16 none = {0, 0, 0, 0};

  for (uint64_t c = c0; c < c1; c++) {
    const uint64_t p0 = cur.ci * PAGE;      // of the store stream
    const uint64_t end = skew + cur.len;    // of the SGE, likewise
    const uint8_t* sp = from0 + p0;
    uint8_t* dp = to0 + p0;
    const bool full = rocp2p_b_full(skew, rel, cur.len, cur.ci);
    // four named registers, not an array: see msg_engine_walk
    rocp2p_g16 v0, v1, v2, v3;
    uint64_t done;  // store-stream bytes [.., done) are covered by acc
    if (full) {
      const rocp2p_g16* src = reinterpret_cast<const rocp2p_g16*>(sp);
      if (rel == 0) {
        v0 = src[lane];
        v1 = src[lane + WAVE];
        v2 = src[lane + 2 * WAVE];
        v3 = src[lane + 3 * WAVE];
      } else {
        const rocp2p_g16 a0 = src[lane], a1 = src[lane + WAVE];
        const rocp2p_g16 a2 = src[lane + 2 * WAVE], a3 = src[lane + 3 * WAVE];
        rocp2p_g16 e = none;
        if (lane == 0) e = src[4 * WAVE];
        g16_realign4(a0, a1, a2, a3, e, rel, lane, v0, v1, v2, v3);
      }
      rocp2p_g16* dst = reinterpret_cast<rocp2p_g16*>(dp);
      dst[lane] = v0;
      dst[lane + WAVE] = v1;
      dst[lane + 2 * WAVE] = v2;
      dst[lane + 3 * WAVE] = v3;
      if constexpr (ICRC)
        acc = rocp2p_crc_apply(s.t.t.shift[5],
                               rocp2p_crc_apply(s.t.t.shift[5], acc)) ^
              icrc_chunk_full(s.t, g16_u4(v0), g16_u4(v1), g16_u4(v2),
                              g16_u4(v3), lane);
      done = p0 + PAGE;
    } else {
      const uint64_t g0 = cur.ci * ROCP2P_B_PER_CHUNK;
      // the SGE in the source stream
      const uint64_t sbeg = (uint64_t)skew + rel, send = end + rel;
      auto fetch = [&](uint32_t q) {
        uint32_t lo, hi;
        rocp2p_b_range(sbeg, send, g0 + q, &lo, &hi);
        return rocp2p_b_load(sp + ROCP2P_B_GRAN * q, lo, hi);
      };
      if (rel == 0) {
        v0 = fetch(lane);
        v1 = fetch(lane + WAVE);
        v2 = fetch(lane + 2 * WAVE);
        v3 = fetch(lane + 3 * WAVE);
      } else {
        const rocp2p_g16 a0 = fetch(lane), a1 = fetch(lane + WAVE);
        const rocp2p_g16 a2 = fetch(lane + 2 * WAVE);
        const rocp2p_g16 a3 = fetch(lane + 3 * WAVE);
        rocp2p_g16 e = none;
        if (lane == 0) e = fetch(4 * WAVE);
        g16_realign4(a0, a1, a2, a3, e, rel, lane, v0, v1, v2, v3);
      }
      uint32_t x = 0;
      auto put = [&](uint32_t q, const rocp2p_g16& v) {
        uint32_t lo, hi;
        rocp2p_b_range(skew, end, g0 + q, &lo, &hi);
        if (lo < hi) {
          rocp2p_b_store(dp + ROCP2P_B_GRAN * q, lo, hi, v);
          if constexpr (ICRC)
            x ^= rocp2p_crc_mulmod(
                rocp2p_crc_xpow8(end - ((g0 + q) * ROCP2P_B_GRAN + hi),
                                 c_crc.xpow8),
                crc_granule_range(s.t.t.slice, v, lo, hi));
        }
      };
      put(lane, v0);
      put(lane + WAVE, v1);
      put(lane + 2 * WAVE, v2);
      put(lane + 3 * WAVE, v3);
      if constexpr (ICRC) {
        for (unsigned o = WAVE / 2; o; o >>= 1) x ^= __shfl_xor(x, o, WAVE);
        // the shift is linear: the tail is applied once, to the sum
        if (tail) x = rocp2p_crc_mulmod(crc_xpow_wave(tail, lane), x);
        if (lane == 0) atomicXor(&out[owner], x);
      }
      done = p0;  // acc (if any) ends where this chunk begins
    }
    if constexpr (ICRC) {
      const bool sge_end = cur.ci + 1 == cur.cpm;
      const bool run_end = c + 1 == c1;
      if (sge_end || run_end || !full) {
        if (acc) {  // a zero CRC contributes nothing wherever it sits
          const uint64_t r = end - done + tail;
          uint32_t f = acc;
          if (r) f = rocp2p_crc_mulmod(crc_xpow_wave(r, lane), acc);
          if (run_end && !sge_end) {
            pend_f = f;
            pend_m = owner;
          } else if (lane == 0) {
            atomicXor(&out[owner], f);
          }
        }
        acc = 0;
      }
    }
    if (c + 1 < c1 && rocp2p_vl_next(&cur, cstart, sge_lens))
      open_sge(cur.m);
  }

  if constexpr (ICRC) {
    __syncthreads();  // the tables are dead: their first words hand off
    crc_merge_pending(&s.t.t.slice[0][0], lane, wv, nwv, pend_f, pend_m, out);
  }
}

// ---------------------------------------------------------------------
// Memory protection (rules: p2p_prot.h).  k_prot_scan is k_vl_scan_b
// with a judge in front of it: one workgroup resolves the keys of every
// message against the MR table, checks both ranges and the access
// rights, and hands the byte-granular engine effective lengths — a
// message that is rejected, or flushed behind a rejected one, has the
// effective length 0, owns no chunk and so reaches no load, store or
// atomic of k_msg_engine_b, which runs unchanged on elen and cstart.
// Wave w judges the segment block_scan gives it, so the verdict parked
// in status[i] is read back by the lane that wrote it.  A table of up to
// PROT_LDS_MRS entries is staged in LDS (every message reads two of
// them); a larger one is read where it lies.  With a queue-pair word the
// first failing message f is the minimum over the whole workgroup: the
// waves' minima meet in LDS at the one barrier between judging and
// scanning.  The word is read by every thread before that barrier and
// written by thread 0 after it.
#define PROT_LDS_MRS 64u
template <bool GATHER>
__global__ void __launch_bounds__(VL_SCAN_THREADS) k_prot_scan(
    const uint8_t* region, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ addrs, const uint64_t* __restrict__ lens,
    const uint64_t* __restrict__ keys, uint32_t n,
    const uint64_t* __restrict__ mrs, uint32_t nmr, int32_t* qp_state,
    int32_t* status, uint64_t* scratch) {
  __shared__ uint64_t s_wave[VL_SCAN_THREADS / WAVE];
  __shared__ uint32_t s_first[VL_SCAN_THREADS / WAVE];
  __shared__ uint64_t s_mr[PROT_LDS_MRS * ROCP2P_PROT_MR_WORDS];
  uint64_t* cstart = scratch;
  uint64_t* elen = scratch + (uint64_t)n + 1;
  const bool qp = qp_state != nullptr;
  const bool entry_err = qp && *qp_state != 0;
  const uint64_t base = reinterpret_cast<uintptr_t>(region);
  const uint32_t lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;

  // block_scan's segments
  const uint64_t per =
      ((uint64_t)n + VL_SCAN_THREADS - 1) / VL_SCAN_THREADS * WAVE;
  const uint64_t b = min(wv * per, (uint64_t)n);
  const uint64_t e = min(b + per, (uint64_t)n);
  uint32_t first = ROCP2P_PROT_NO_F;
  auto judge = [&](const uint64_t* tab) {
    for (uint64_t i = b + lane; i < e; i += WAVE) {
      const uint32_t v = rocp2p_prot_verdict(tab, nmr, base, offs[i], addrs[i],
                                             lens[i], keys[i], GATHER);
      status[i] = (int32_t)v;
      if (v != ROCP2P_WC_SUCCESS && first == ROCP2P_PROT_NO_F)
        first = (uint32_t)i;
    }
  };
  if (nmr <= PROT_LDS_MRS) {
    for (uint32_t i = threadIdx.x; i < nmr * ROCP2P_PROT_MR_WORDS;
         i += VL_SCAN_THREADS)
      s_mr[i] = mrs[i];
    __syncthreads();
    judge(s_mr);
  } else {
    judge(mrs);
  }
  for (uint32_t o = WAVE / 2; o; o >>= 1)
    first = min(first, (uint32_t)__shfl_xor((int)first, o, WAVE));
  if (lane == 0) s_first[wv] = first;
  __syncthreads();
  uint32_t f = ROCP2P_PROT_NO_F;
  for (uint32_t w = 0; w < VL_SCAN_THREADS / WAVE; w++) f = min(f, s_first[w]);
  if (qp && threadIdx.x == 0 && (entry_err || f != ROCP2P_PROT_NO_F))
    *qp_state = 1;

  block_scan<false, true>(
      [&](uint64_t i) {
        const uint32_t st = rocp2p_prot_final((uint32_t)status[i], (uint32_t)i,
                                              f, qp, entry_err);
        const uint64_t el = rocp2p_prot_elen(st, lens[i]);
        status[i] = (int32_t)st;
        elen[i] = el;
        return rocp2p_b_chunks((uint32_t)(GATHER ? offs[i] : addrs[i]) & 15u,
                               el);
      },
      n, cstart, s_wave);
}

// ---------------------------------------------------------------------
// launchers

static inline uint32_t stream_grid(uint64_t items, uint32_t per_block) {
  uint64_t blocks = (items + per_block - 1) / per_block;
  if (blocks > 16384) blocks = 16384;  // tuned: tools/hbm_bench.hip
  if (blocks == 0) blocks = 1;
  return (uint32_t)blocks;
}

extern "C" hipError_t rocp2p_fill(void* buf, uint64_t nbytes, uint64_t seed,
                                  hipStream_t stream) {
  if (nbytes % 8) return hipErrorInvalidValue;
  uint64_t nwords = nbytes / 8;
  uint32_t grid = stream_grid(nwords / 16, 256);
  if (grid > 8192) grid = 8192;  // fill peaks at 8192 WGs (hbm_bench)
  hipLaunchKernelGGL(k_fill, dim3(grid), dim3(256), 0, stream,
                     (uint64_t*)buf, nwords, seed);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_verify(const void* buf, uint64_t nbytes,
                                    uint64_t seed,
                                    unsigned long long* d_mismatch,
                                    hipStream_t stream) {
  if (nbytes % 8) return hipErrorInvalidValue;
  uint64_t nwords = nbytes / 8;
  uint32_t grid = stream_grid(nwords / 8, 256);
  hipLaunchKernelGGL(k_verify, dim3(grid), dim3(256), 0, stream,
                     (const uint64_t*)buf, nwords, seed, d_mismatch);
  return hipGetLastError();
}

template <bool NT>
static hipError_t copy_launch(void* dst, const void* src, uint64_t nbytes,
                              hipStream_t stream) {
  if (nbytes % 16) return hipErrorInvalidValue;
  uint64_t nvec = nbytes / 16;
  uint32_t grid = stream_grid(nvec / 4, 256);
  hipLaunchKernelGGL(k_copy_t<NT>, dim3(grid), dim3(256), 0, stream,
                     (uint4_cv*)dst, (const uint4_cv*)src, nvec);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_copy(void* dst, const void* src, uint64_t nbytes,
                                  hipStream_t stream) {
  return copy_launch<false>(dst, src, nbytes, stream);
}

extern "C" hipError_t rocp2p_copy_nt(void* dst, const void* src,
                                     uint64_t nbytes, hipStream_t stream) {
  return copy_launch<true>(dst, src, nbytes, stream);
}

// The gather/scatter engine is PCIe-bound, not CU-bound: measured on
// MI355X, 512 workgroups (2/CU) already saturate the link and beat the
// full-grid launch by ~4% at 4 KiB (less scheduling churn), while
// leaving 254 of 256 CUs free for whatever else the GPU is running —
// exactly how a NIC coexists with compute.  ROCP2P_GATHER_GRID
// overrides for experiments.
static uint32_t gather_grid_cap() {
  static int cap = -1;
  if (cap < 0) {
    const char* e = getenv("ROCP2P_GATHER_GRID");
    cap = e ? atoi(e) : 0;
    if (cap <= 0) cap = 512;
  }
  return (uint32_t)cap;
}

template <bool GATHER>
static hipError_t msg_engine_launch(void* region, const uint64_t* d_offs,
                                    const uint64_t* d_addrs,
                                    uint64_t msg_bytes, uint32_t n,
                                    hipStream_t stream) {
  if (msg_bytes % 16 || !msg_bytes) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  uint64_t vecs_per_msg = msg_bytes / 16;
  uint64_t total = vecs_per_msg * n;
  uint32_t grid = stream_grid(total, 256);
  if (grid > gather_grid_cap()) grid = gather_grid_cap();
  uint32_t vshift = (vecs_per_msg & (vecs_per_msg - 1))
                        ? 0xffffffffu
                        : (uint32_t)__builtin_ctzll(vecs_per_msg);
  hipLaunchKernelGGL(k_msg_engine<GATHER>, dim3(grid), dim3(256), 0, stream,
                     (uint8_t*)region, d_offs, d_addrs, vecs_per_msg, total,
                     vshift);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_gather(void* dst_base,
                                    const uint64_t* d_dst_offs,
                                    const uint64_t* d_src_addrs,
                                    uint64_t msg_bytes, uint32_t n,
                                    hipStream_t stream) {
  return msg_engine_launch<true>(dst_base, d_dst_offs, d_src_addrs, msg_bytes,
                                 n, stream);
}

extern "C" hipError_t rocp2p_scatter(const void* src_base,
                                     const uint64_t* d_src_offs,
                                     const uint64_t* d_dst_addrs,
                                     uint64_t msg_bytes, uint32_t n,
                                     hipStream_t stream) {
  // the scatter instantiation only reads the region
  return msg_engine_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                  d_dst_addrs, msg_bytes, n, stream);
}

// The tables are a compile-time constant (p2p_crc.h); each device that
// runs a CRC kernel gets its copy before its first launch.  The device
// of `stream` must be current, as for the launch itself.
static hipError_t crc_tables_ready() {
  static constexpr rocp2p_crc_tables tables = rocp2p_crc_make_tables();
  static std::mutex mu;
  static bool ready[64];  // by device ordinal
  int dev;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  if (ready[dev]) return hipSuccess;
  e = hipMemcpyToSymbol(HIP_SYMBOL(c_crc), &tables, sizeof(tables));
  ready[dev] = e == hipSuccess;
  return e;
}

// What every launch that digests does first: the tables, and n zeroed
// digests for the kernels to XOR into.
static hipError_t crc_out_ready(uint32_t* d_out, uint32_t n,
                                hipStream_t stream) {
  hipError_t e = crc_tables_ready();
  if (e != hipSuccess) return e;
  return hipMemsetAsync(d_out, 0, (size_t)n * sizeof(uint32_t), stream);
}

// Workgroup cap of the chunk-walking engines (4-wave workgroups, one
// chunk per wave until the grid is full, longer runs after that).
// The fused forms stay under the plain engine's cap and, measured on
// MI355X, under 128 workgroups: the fused gather loses to its own
// outstanding PCIe reads beyond that (1 MiB-class messages: 49.9 GB/s at
// 512 workgroups, 52.9 at 256, 54.0 at 128, 53.6 at 64; the scatter
// direction does not care).  The plain gather has the same four 16-byte
// PCIe reads per lane in flight and, measured on MI355X, the same
// optimum (4 KiB and 1 MiB messages: 53.0 GB/s at 512 workgroups, 53.5
// at 256, 56.1-56.7 at 128 and 64); only batches known to hold sub-chunk
// messages (0 < max_msg_bytes < 4096), whose waves have few lanes busy,
// do better with the full cap (64 B: 19.6 GB/s at 128, 22.4 at 512).
// The plain scatter does not care from 4 KiB up and wants the full cap
// at 64 B (21.5 at 128, 26.1 at 512).  The byte-granular and the
// scatter/gather engines take the same caps until measurements say
// otherwise (docs/PERF.md).  grid_cap != 0 caps the count further.
#define ICRC_GRID 128u
static uint64_t engine_grid_cap(bool gather, bool icrc, uint64_t max_msg_bytes,
                                uint32_t grid_cap) {
  uint64_t cap = gather_grid_cap();
  const bool small = max_msg_bytes && max_msg_bytes < PAGE;
  if ((icrc || (gather && !small)) && cap > ICRC_GRID) cap = ICRC_GRID;
  if (grid_cap && grid_cap < cap) cap = grid_cap;
  return cap;
}

// Launch an engine's fused form when there are digests to write, its
// plain form otherwise; both take the same arguments.
template <typename K, typename... A>
static hipError_t engine_launch(K fused, K plain, uint32_t* d_out,
                                uint32_t grid, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(d_out ? fused : plain, dim3(grid),
                     dim3(WAVE * ICRC_WAVES), 0, stream, args..., d_out);
  return hipGetLastError();
}

template <bool GATHER>
static hipError_t msg_engine_crc_launch(void* region, const uint64_t* d_offs,
                                        const uint64_t* d_addrs,
                                        uint64_t msg_bytes, uint32_t n,
                                        uint32_t* d_out, uint32_t grid_cap,
                                        hipStream_t stream) {
  if (msg_bytes % 16 || !msg_bytes) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = crc_out_ready(d_out, n, stream);
  if (e != hipSuccess) return e;
  uint64_t cpm = msg_bytes / PAGE + (msg_bytes % PAGE != 0);
  uint64_t total;
  if (__builtin_mul_overflow(cpm, (uint64_t)n, &total))
    return hipErrorInvalidValue;
  const uint64_t W = ICRC_WAVES;
  const uint64_t cap = engine_grid_cap(GATHER, true, 0, grid_cap);
  uint64_t blocks = (total + W - 1) / W;
  if (blocks > cap) blocks = cap;
  uint64_t run = (total + W * blocks - 1) / (W * blocks);
  hipLaunchKernelGGL(k_msg_engine_crc<GATHER>, dim3((uint32_t)blocks),
                     dim3(WAVE * ICRC_WAVES), 0, stream, (uint8_t*)region,
                     d_offs, d_addrs, msg_bytes, cpm, total, run, d_out);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_gather_crc(void* dst_base,
                                        const uint64_t* d_dst_offs,
                                        const uint64_t* d_src_addrs,
                                        uint64_t msg_bytes, uint32_t n,
                                        uint32_t* d_out, uint32_t grid_cap,
                                        hipStream_t stream) {
  return msg_engine_crc_launch<true>(dst_base, d_dst_offs, d_src_addrs,
                                     msg_bytes, n, d_out, grid_cap, stream);
}

extern "C" hipError_t rocp2p_scatter_crc(const void* src_base,
                                         const uint64_t* d_src_offs,
                                         const uint64_t* d_dst_addrs,
                                         uint64_t msg_bytes, uint32_t n,
                                         uint32_t* d_out, uint32_t grid_cap,
                                         hipStream_t stream) {
  // the scatter instantiation only reads the region
  return msg_engine_crc_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                      d_dst_addrs, msg_bytes, n, d_out,
                                      grid_cap, stream);
}

extern "C" hipError_t rocp2p_crc32_pages(const void* buf, uint64_t npages,
                                         uint32_t* d_out, hipStream_t stream) {
  hipError_t e = crc_tables_ready();
  if (e != hipSuccess) return e;
  if (!npages) return hipSuccess;
  uint64_t blocks = (npages + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_crc32_pages, dim3((uint32_t)blocks), dim3(256), 0,
                     stream, (const uint32_t*)buf, npages, d_out);
  return hipGetLastError();
}

// Digest launch shape (measured on MI355X): one chunk per wave up to
// 256 workgroups of 16 waves = 4096 waves = 16 per CU, which already
// saturates the LDS; beyond 16 MiB the grid stays and the runs lengthen,
// so flushes get rarer as the input grows (1 GiB of 1 MiB messages:
// 3.1 TB/s with 8-chunk runs, 3.9 TB/s with 64-chunk runs).  16-wave
// workgroups beat 4- and 8-wave ones by 2-15% from 64 MiB up: one table
// copy per CU and 16 pending shares merged into one atomic.
// grid_cap != 0 caps the workgroup count instead of 256.
static uint64_t digest_grid_cap(uint32_t grid_cap) {
  return grid_cap ? grid_cap : 256;
}

static hipError_t crc32_digest_launch(const void* base,
                                      const uint64_t* d_offs,
                                      uint64_t msg_bytes, uint32_t n,
                                      uint32_t* d_out, uint32_t grid_cap,
                                      hipStream_t stream) {
  hipError_t e = crc_out_ready(d_out, n, stream);
  if (e != hipSuccess) return e;
  if (!msg_bytes) return hipSuccess;  // crc32 of nothing is 0
  uint64_t cpm = msg_bytes / PAGE + (msg_bytes % PAGE != 0);
  uint64_t total;
  if (__builtin_mul_overflow(cpm, (uint64_t)n, &total))
    return hipErrorInvalidValue;
  const uint64_t W = CRC_DIGEST_WAVES;
  const uint64_t cap = digest_grid_cap(grid_cap);
  uint64_t blocks = (total + W - 1) / W;
  if (blocks > cap) blocks = cap;
  uint64_t run = (total + W * blocks - 1) / (W * blocks);
  hipLaunchKernelGGL(k_crc32_msgs, dim3((uint32_t)blocks),
                     dim3(WAVE * CRC_DIGEST_WAVES), 0,
                     stream, (const uint8_t*)base, d_offs, msg_bytes, cpm,
                     total, run, d_out);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_crc32_msgs(const void* base,
                                        const uint64_t* d_offs,
                                        uint64_t msg_bytes, uint32_t n,
                                        uint32_t* d_out, uint32_t grid_cap,
                                        hipStream_t stream) {
  if (msg_bytes % 16 || !msg_bytes || (uintptr_t)base % 16)
    return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  return crc32_digest_launch(base, d_offs, msg_bytes, n, d_out, grid_cap,
                             stream);
}

extern "C" hipError_t rocp2p_crc32_region(const void* buf, uint64_t nbytes,
                                          uint32_t* d_out, uint32_t grid_cap,
                                          hipStream_t stream) {
  if ((uintptr_t)buf % 16) return hipErrorInvalidValue;
  return crc32_digest_launch(buf, nullptr, nbytes, 1, d_out, grid_cap,
                             stream);
}

// ---------------------------------------------------------------------
// Variable-length launchers: the scan, then the main kernel, on one
// stream with no host step in between.  The host knows only an upper
// bound of the chunk total (n messages of at most max_msg_bytes; 0 =
// unknown, take the cap): it sizes the grid and nothing else, the
// kernels take the real total from d_cstart[n].

// Workgroups for at most n messages of at most max_msg_bytes each, plus
// `extra` chunks that cutting the messages up may add.
static uint32_t vl_grid(uint32_t n, uint64_t max_msg_bytes, uint64_t extra,
                        uint64_t waves, uint64_t cap) {
  if (!cap) cap = 1;
  if (!max_msg_bytes) return (uint32_t)cap;
  uint64_t bound;
  if (__builtin_mul_overflow(rocp2p_vl_chunks(max_msg_bytes), (uint64_t)n,
                             &bound) ||
      __builtin_add_overflow(bound, extra, &bound))
    return (uint32_t)cap;
  uint64_t blocks = bound / waves + (bound % waves != 0);
  return (uint32_t)(blocks > cap ? cap : blocks);  // >= 1: n, max > 0
}

static hipError_t vl_scan_launch(const uint64_t* d_lens, uint32_t n,
                                 uint64_t* d_cstart, hipStream_t stream) {
  hipLaunchKernelGGL(k_vl_scan, dim3(1), dim3(VL_SCAN_THREADS), 0, stream,
                     d_lens, n, d_cstart);
  return hipGetLastError();
}

template <bool GATHER>
static hipError_t msg_engine_v_launch(void* region, const uint64_t* d_offs,
                                      const uint64_t* d_addrs,
                                      const uint64_t* d_lens, uint32_t n,
                                      uint64_t max_msg_bytes,
                                      uint64_t* d_cstart, uint32_t* d_out,
                                      uint32_t grid_cap, hipStream_t stream) {
  if (!d_cstart || (uintptr_t)region % 16) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = d_out ? crc_out_ready(d_out, n, stream) : hipSuccess;
  if (e != hipSuccess) return e;
  e = vl_scan_launch(d_lens, n, d_cstart, stream);
  if (e != hipSuccess) return e;
  const uint64_t cap =
      engine_grid_cap(GATHER, d_out != nullptr, max_msg_bytes, grid_cap);
  const uint32_t grid = vl_grid(n, max_msg_bytes, 0, ICRC_WAVES, cap);
  return engine_launch(k_msg_engine_v<GATHER, true>,
                       k_msg_engine_v<GATHER, false>, d_out, grid, stream,
                       (uint8_t*)region, d_offs, d_addrs, d_lens,
                       (const uint64_t*)d_cstart, n);
}

extern "C" hipError_t rocp2p_gather_v(void* dst_base,
                                      const uint64_t* d_dst_offs,
                                      const uint64_t* d_src_addrs,
                                      const uint64_t* d_lens, uint32_t n,
                                      uint64_t max_msg_bytes,
                                      uint64_t* d_cstart, uint32_t* d_out,
                                      uint32_t grid_cap, hipStream_t stream) {
  return msg_engine_v_launch<true>(dst_base, d_dst_offs, d_src_addrs, d_lens,
                                   n, max_msg_bytes, d_cstart, d_out,
                                   grid_cap, stream);
}

extern "C" hipError_t rocp2p_scatter_v(const void* src_base,
                                       const uint64_t* d_src_offs,
                                       const uint64_t* d_dst_addrs,
                                       const uint64_t* d_lens, uint32_t n,
                                       uint64_t max_msg_bytes,
                                       uint64_t* d_cstart, uint32_t* d_out,
                                       uint32_t grid_cap,
                                       hipStream_t stream) {
  // the scatter instantiations only read the region
  return msg_engine_v_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                    d_dst_addrs, d_lens, n, max_msg_bytes,
                                    d_cstart, d_out, grid_cap, stream);
}

extern "C" hipError_t rocp2p_crc32_msgs_v(const void* base,
                                          const uint64_t* d_offs,
                                          const uint64_t* d_lens, uint32_t n,
                                          uint64_t max_msg_bytes,
                                          uint64_t* d_cstart, uint32_t* d_out,
                                          uint32_t grid_cap,
                                          hipStream_t stream) {
  if (!d_cstart || (uintptr_t)base % 16) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = crc_out_ready(d_out, n, stream);
  if (e != hipSuccess) return e;
  e = vl_scan_launch(d_lens, n, d_cstart, stream);
  if (e != hipSuccess) return e;
  const uint32_t grid = vl_grid(n, max_msg_bytes, 0, CRC_DIGEST_WAVES,
                                digest_grid_cap(grid_cap));
  hipLaunchKernelGGL(k_crc32_msgs_v, dim3(grid),
                     dim3(WAVE * CRC_DIGEST_WAVES), 0, stream,
                     (const uint8_t*)base, d_offs, d_lens,
                     (const uint64_t*)d_cstart, n, d_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------
// Byte-granular launchers: those of the variable-length forms with
// k_vl_scan_b over the side that is written.  A skewed message of
// max_msg_bytes may have one chunk more than an aligned one (b_bound);
// like max_msg_bytes itself that only sizes the grid.

static uint64_t b_bound(uint64_t max_msg_bytes) {
  return max_msg_bytes ? max_msg_bytes + PAGE : 0;
}

static hipError_t vl_scan_b_launch(const uint64_t* d_lens,
                                   const uint64_t* d_where, uint32_t n,
                                   uint64_t* d_cstart, hipStream_t stream) {
  hipLaunchKernelGGL(k_vl_scan_b, dim3(1), dim3(VL_SCAN_THREADS), 0, stream,
                     d_lens, d_where, n, d_cstart);
  return hipGetLastError();
}

template <bool GATHER>
static hipError_t msg_engine_b_launch(void* region, const uint64_t* d_offs,
                                      const uint64_t* d_addrs,
                                      const uint64_t* d_lens, uint32_t n,
                                      uint64_t max_msg_bytes,
                                      uint64_t* d_cstart, uint32_t* d_out,
                                      uint32_t grid_cap, hipStream_t stream) {
  if (!d_cstart || (uintptr_t)region % 16) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = d_out ? crc_out_ready(d_out, n, stream) : hipSuccess;
  if (e != hipSuccess) return e;
  // the region base is 16-byte aligned: an offset's low bits are the skew
  e = vl_scan_b_launch(d_lens, GATHER ? d_offs : d_addrs, n, d_cstart,
                       stream);
  if (e != hipSuccess) return e;
  const uint64_t cap =
      engine_grid_cap(GATHER, d_out != nullptr, max_msg_bytes, grid_cap);
  const uint32_t grid =
      vl_grid(n, b_bound(max_msg_bytes), 0, ICRC_WAVES, cap);
  return engine_launch(k_msg_engine_b<GATHER, true>,
                       k_msg_engine_b<GATHER, false>, d_out, grid, stream,
                       (uint8_t*)region, d_offs, d_addrs, d_lens,
                       (const uint64_t*)d_cstart, n);
}

extern "C" hipError_t rocp2p_gather_b(void* dst_base,
                                      const uint64_t* d_dst_offs,
                                      const uint64_t* d_src_addrs,
                                      const uint64_t* d_lens, uint32_t n,
                                      uint64_t max_msg_bytes,
                                      uint64_t* d_cstart, uint32_t* d_out,
                                      uint32_t grid_cap, hipStream_t stream) {
  return msg_engine_b_launch<true>(dst_base, d_dst_offs, d_src_addrs, d_lens,
                                   n, max_msg_bytes, d_cstart, d_out,
                                   grid_cap, stream);
}

extern "C" hipError_t rocp2p_scatter_b(const void* src_base,
                                       const uint64_t* d_src_offs,
                                       const uint64_t* d_dst_addrs,
                                       const uint64_t* d_lens, uint32_t n,
                                       uint64_t max_msg_bytes,
                                       uint64_t* d_cstart, uint32_t* d_out,
                                       uint32_t grid_cap,
                                       hipStream_t stream) {
  // the scatter instantiations only read the region
  return msg_engine_b_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                    d_dst_addrs, d_lens, n, max_msg_bytes,
                                    d_cstart, d_out, grid_cap, stream);
}

extern "C" hipError_t rocp2p_crc32_msgs_b(const void* base,
                                          const uint64_t* d_offs,
                                          const uint64_t* d_lens, uint32_t n,
                                          uint64_t max_msg_bytes,
                                          uint64_t* d_cstart, uint32_t* d_out,
                                          uint32_t grid_cap,
                                          hipStream_t stream) {
  if (!d_cstart || (uintptr_t)base % 16) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = crc_out_ready(d_out, n, stream);
  if (e != hipSuccess) return e;
  e = vl_scan_b_launch(d_lens, d_offs, n, d_cstart, stream);
  if (e != hipSuccess) return e;
  const uint32_t grid = vl_grid(n, b_bound(max_msg_bytes), 0,
                                CRC_DIGEST_WAVES, digest_grid_cap(grid_cap));
  hipLaunchKernelGGL(k_crc32_msgs_b, dim3(grid),
                     dim3(WAVE * CRC_DIGEST_WAVES), 0, stream,
                     (const uint8_t*)base, d_offs, d_lens,
                     (const uint64_t*)d_cstart, n, d_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------
// Scatter/gather launchers: the scan, then the engine, on one stream.
// max_msg_bytes bounds a whole message; cut into its SGEs a message has
// at most two chunks more per SGE than the bytes alone would give (a
// partial first and a partial last one).  That only sizes the grid.

template <bool GATHER>
static hipError_t msg_engine_sg_launch(void* region, const uint64_t* d_offs,
                                       const uint64_t* d_sge_start,
                                       const uint64_t* d_sge_addrs,
                                       const uint64_t* d_sge_lens, uint32_t n,
                                       uint32_t nsge, uint64_t max_msg_bytes,
                                       uint64_t* d_scratch, uint32_t* d_out,
                                       uint32_t grid_cap,
                                       hipStream_t stream) {
  if (!d_scratch || (uintptr_t)region % 16) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = d_out ? crc_out_ready(d_out, n, stream) : hipSuccess;
  if (e != hipSuccess) return e;
  if (!nsge) return hipSuccess;  // n messages without a byte
  hipLaunchKernelGGL(k_sg_scan<GATHER>, dim3(1), dim3(VL_SCAN_THREADS), 0,
                     stream, (const uint8_t*)region, d_offs, d_sge_start,
                     d_sge_addrs, d_sge_lens, n, nsge, d_scratch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const rocp2p_sgl_view v = rocp2p_sgl_carve(d_scratch, nsge);
  const uint64_t cap =
      engine_grid_cap(GATHER, d_out != nullptr, max_msg_bytes, grid_cap);
  const uint32_t grid =
      vl_grid(n, max_msg_bytes, 2 * (uint64_t)nsge, ICRC_WAVES, cap);
  return engine_launch(k_msg_engine_sg<true>, k_msg_engine_sg<false>, d_out,
                       grid, stream, d_sge_lens, (const uint64_t*)v.cstart,
                       (const uint64_t*)v.to, (const uint64_t*)v.from,
                       (const uint64_t*)v.tail, (const uint32_t*)v.owner,
                       nsge);
}

extern "C" hipError_t rocp2p_gather_sg(
    void* dst_base, const uint64_t* d_dst_offs, const uint64_t* d_sge_start,
    const uint64_t* d_sge_addrs, const uint64_t* d_sge_lens, uint32_t n,
    uint32_t nsge, uint64_t max_msg_bytes, uint64_t* d_scratch,
    uint32_t* d_out, uint32_t grid_cap, hipStream_t stream) {
  return msg_engine_sg_launch<true>(dst_base, d_dst_offs, d_sge_start,
                                    d_sge_addrs, d_sge_lens, n, nsge,
                                    max_msg_bytes, d_scratch, d_out, grid_cap,
                                    stream);
}

extern "C" hipError_t rocp2p_scatter_sg(
    const void* src_base, const uint64_t* d_src_offs,
    const uint64_t* d_sge_start, const uint64_t* d_sge_addrs,
    const uint64_t* d_sge_lens, uint32_t n, uint32_t nsge,
    uint64_t max_msg_bytes, uint64_t* d_scratch, uint32_t* d_out,
    uint32_t grid_cap, hipStream_t stream) {
  // the scatter scan only ever puts the region on the side that is read
  return msg_engine_sg_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                     d_sge_start, d_sge_addrs, d_sge_lens, n,
                                     nsge, max_msg_bytes, d_scratch, d_out,
                                     grid_cap, stream);
}

// ---------------------------------------------------------------------
// Protected launchers: k_prot_scan, then the unchanged byte-granular
// engine over the effective lengths, on one stream.  The grid is sized
// as for rocp2p_gather_b; it depends on no verdict.

template <bool GATHER>
static hipError_t msg_engine_p_launch(
    void* region, const uint64_t* d_offs, const uint64_t* d_addrs,
    const uint64_t* d_lens, const uint64_t* d_keys, uint32_t n,
    const uint64_t* d_mrs, uint32_t nmr, int32_t* d_qp_state,
    uint64_t max_msg_bytes, uint64_t* d_scratch, int32_t* d_status,
    uint32_t* d_out, uint32_t grid_cap, hipStream_t stream) {
  if (!d_scratch || !d_status || !d_mrs || !nmr ||
      nmr > ROCP2P_PROT_MAX_MR || (uintptr_t)region % 16)
    return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  hipError_t e = d_out ? crc_out_ready(d_out, n, stream) : hipSuccess;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_prot_scan<GATHER>, dim3(1), dim3(VL_SCAN_THREADS), 0,
                     stream, (const uint8_t*)region, d_offs, d_addrs, d_lens,
                     d_keys, n, d_mrs, nmr, d_qp_state, d_status, d_scratch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t cap =
      engine_grid_cap(GATHER, d_out != nullptr, max_msg_bytes, grid_cap);
  const uint32_t grid =
      vl_grid(n, b_bound(max_msg_bytes), 0, ICRC_WAVES, cap);
  const uint64_t* d_cstart = d_scratch;
  const uint64_t* d_elen = d_scratch + (uint64_t)n + 1;
  return engine_launch(k_msg_engine_b<GATHER, true>,
                       k_msg_engine_b<GATHER, false>, d_out, grid, stream,
                       (uint8_t*)region, d_offs, d_addrs, d_elen, d_cstart, n);
}

extern "C" hipError_t rocp2p_gather_p(
    void* dst_base, const uint64_t* d_dst_offs, const uint64_t* d_src_addrs,
    const uint64_t* d_lens, const uint64_t* d_keys, uint32_t n,
    const uint64_t* d_mrs, uint32_t nmr, int32_t* d_qp_state,
    uint64_t max_msg_bytes, uint64_t* d_scratch, int32_t* d_status,
    uint32_t* d_out, uint32_t grid_cap, hipStream_t stream) {
  return msg_engine_p_launch<true>(dst_base, d_dst_offs, d_src_addrs, d_lens,
                                   d_keys, n, d_mrs, nmr, d_qp_state,
                                   max_msg_bytes, d_scratch, d_status, d_out,
                                   grid_cap, stream);
}

extern "C" hipError_t rocp2p_scatter_p(
    const void* src_base, const uint64_t* d_src_offs,
    const uint64_t* d_dst_addrs, const uint64_t* d_lens,
    const uint64_t* d_keys, uint32_t n, const uint64_t* d_mrs, uint32_t nmr,
    int32_t* d_qp_state, uint64_t max_msg_bytes, uint64_t* d_scratch,
    int32_t* d_status, uint32_t* d_out, uint32_t grid_cap,
    hipStream_t stream) {
  // the scatter instantiations only read the region
  return msg_engine_p_launch<false>(const_cast<void*>(src_base), d_src_offs,
                                    d_dst_addrs, d_lens, d_keys, n, d_mrs,
                                    nmr, d_qp_state, max_msg_bytes, d_scratch,
                                    d_status, d_out, grid_cap, stream);
}
