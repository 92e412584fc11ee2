// SPDX-License-Identifier: MIT
//
// p2p_kernels.hip — hand-written gfx950 (CDNA4) payload kernels for the
// GPU-direct RDMA harness: deterministic pattern fill, on-GPU CRC32
// integrity, and a streaming-copy bandwidth probe.  These are the "HIP
// fill/CRC kernel (LDS-staged)" the north star requires: payloads are
// generated AND verified in HBM, so zero-copy RDMA can be proven without
// any host readback (the reference had no integrity path at all beyond a
// broken single-sg mmap readback — reference: /root/reference/tests/
// amdp2ptest.c:336-395).
//
// MI355X design notes (per /opt/skills/guides/MI355X_MICROARCH.md):
//  - wave64; all wave-width constants hard-coded 64;
//  - streaming kernels move 16 B/lane/instruction (dwordx4), grid-stride
//    with >> 256 workgroups to fill 8 XCDs;
//  - CRC32: one wave per 4 KiB page, lane l owns bytes [64l, 64l+64);
//    slice-by-8 tables (8 x 256 u32) live in LDS (random-access lookups,
//    exactly what LDS is for); each lane's segment CRC is shifted by its
//    tail length with 6 GF(2) 32x32 matrices (M(64B<<k)) also in LDS,
//    then XOR-reduced across the wave with __shfl_xor (combine identity
//    validated against zlib in tests/test_crc.py);
//  - compute ceiling: ~8 table lookups per 8 B per lane; far above the
//    PCIe/NIC rates this harness verifies, far below HBM peak by design
//    (integrity pass, not the timed datapath).

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include "p2p_kernels.h"
#include "p2p_crc.h"
#include "p2p_pattern.h"

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
// launch-bound.  msg_bytes is uniform per batch (transport invariant).

// vshift: log2(vecs_per_msg) when it is a power of two (uniform branch
// avoids a 64-bit divide per 16-byte vector), else 0xffffffff.
__global__ void k_gather(uint8_t* __restrict__ dst_base,
                         const uint64_t* __restrict__ dst_offs,
                         const uint64_t* __restrict__ src_addrs,
                         uint64_t vecs_per_msg, uint64_t total_vecs,
                         uint32_t vshift) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       v < total_vecs; v += stride) {
    uint64_t msg = (vshift != 0xffffffffu) ? (v >> vshift)
                                           : (v / vecs_per_msg);
    uint64_t idx = v - msg * vecs_per_msg;
    const uint4* src = reinterpret_cast<const uint4*>(src_addrs[msg]);
    uint4* dst = reinterpret_cast<uint4*>(dst_base + dst_offs[msg]);
    dst[idx] = src[idx];
  }
}

__global__ void k_scatter(const uint8_t* __restrict__ src_base,
                          const uint64_t* __restrict__ src_offs,
                          const uint64_t* __restrict__ dst_addrs,
                          uint64_t vecs_per_msg, uint64_t total_vecs,
                          uint32_t vshift) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       v < total_vecs; v += stride) {
    uint64_t msg = (vshift != 0xffffffffu) ? (v >> vshift)
                                           : (v / vecs_per_msg);
    uint64_t idx = v - msg * vecs_per_msg;
    const uint4* src =
        reinterpret_cast<const uint4*>(src_base + src_offs[msg]);
    uint4* dst = reinterpret_cast<uint4*>(dst_addrs[msg]);
    dst[idx] = src[idx];
  }
}

// ---------------------------------------------------------------------
// CRC32 (zlib polynomial 0xEDB88320, init/xorout 0xFFFFFFFF)

__constant__ uint32_t c_crc_tab[8][256];   // slice-by-8
// Byte-sliced GF(2) shift operators: c_shift_tab[k][b][v] = M(64B<<k)
// applied to (v << 8b).  Applying a 32x32 GF(2) matrix becomes 4 table
// lookups instead of 32 serial dependent steps.
__constant__ uint32_t c_shift_tab[6][4][256];

static bool g_crc_ready = false;

static void host_make_tables(uint32_t tab[8][256],
                             uint32_t stab[6][4][256]) {
  const uint32_t POLY = 0xEDB88320u;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
    tab[0][i] = c;
  }
  for (int t = 1; t < 8; t++)
    for (uint32_t i = 0; i < 256; i++)
      tab[t][i] = (tab[t - 1][i] >> 8) ^ tab[0][tab[t - 1][i] & 0xff];

  // GF(2) matrices: odd = shift-by-1-bit operator, square to double.
  uint32_t m1[32], m2[32];
  m1[0] = POLY;
  for (int i = 1; i < 32; i++) m1[i] = 1u << (i - 1);
  auto times = [](const uint32_t* m, uint32_t v) {
    uint32_t s = 0;
    for (int i = 0; v; v >>= 1, i++)
      if (v & 1) s ^= m[i];
    return s;
  };
  auto square = [&](const uint32_t* in, uint32_t* out) {
    for (int i = 0; i < 32; i++) out[i] = times(in, in[i]);
  };
  // m1: 1 bit -> square 3x => 8 bits (1 byte)
  square(m1, m2);        // 2 bits
  square(m2, m1);        // 4 bits
  square(m1, m2);        // 8 bits = 1 byte (in m2)
  // 1B -> 64B: square 6 more times
  uint32_t cur[32];
  for (int i = 0; i < 32; i++) cur[i] = m2[i];
  for (int k = 0; k < 6; k++) {
    square(cur, m1);
    for (int i = 0; i < 32; i++) cur[i] = m1[i];
  }  // cur = shift by 64 bytes
  for (int k = 0; k < 6; k++) {
    for (int b = 0; b < 4; b++)
      for (uint32_t v = 0; v < 256; v++)
        stab[k][b][v] = times(cur, v << (8 * b));
    square(cur, m1);
    for (int i = 0; i < 32; i++) cur[i] = m1[i];
  }
}

// One wave per 4 KiB page; 4 waves (256 threads) per workgroup.
__global__ void __launch_bounds__(256) k_crc32_pages(
    const uint32_t* __restrict__ buf, uint64_t npages,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t s_tab[8][256];
  __shared__ uint32_t s_stab[6][4][256];

  // stage tables into LDS (8 KB slice-by-8 + 24 KB shift operators)
  for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
    (&s_tab[0][0])[i] = (&c_crc_tab[0][0])[i];
  for (uint32_t i = threadIdx.x; i < 6 * 4 * 256; i += blockDim.x)
    (&s_stab[0][0][0])[i] = (&c_shift_tab[0][0][0])[i];
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

    // Log-tree combine: level k merges adjacent spans of 64B<<k.
    // combine(cL, cR) = shift(cL, span) ^ cR; shift is linear over
    // XOR, so the tree equals the flat XOR-of-shifted-lane-CRCs
    // identity validated against zlib in tests/test_pattern.py.  The
    // shift matrix is UNIFORM per level (byte-sliced: 4 LDS lookups),
    // and the tree doubles as the wave reduction — every lane ends
    // holding the page CRC.
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
// launcher).  Full chunks reuse the page scheme above (slice-by-8 +
// uniform log tree, same LDS tables, same 32 KB per workgroup).
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

__constant__ uint32_t c_xpow8[8][256];  // x^(8 * v * 256^j) mod P

typedef uint32_t crc_tab256[256];

__device__ __forceinline__ uint32_t crc_step8(const crc_tab256* t,
                                              uint32_t crc, uint32_t lo,
                                              uint32_t hi) {
  uint32_t a = lo ^ crc;
  return t[7][a & 0xff] ^ t[6][(a >> 8) & 0xff] ^ t[5][(a >> 16) & 0xff] ^
         t[4][a >> 24] ^ t[3][hi & 0xff] ^ t[2][(hi >> 8) & 0xff] ^
         t[1][(hi >> 16) & 0xff] ^ t[0][hi >> 24];
}

// byte-sliced GF(2) operator applied to c (4 lookups)
__device__ __forceinline__ uint32_t crc_apply(const crc_tab256* m,
                                              uint32_t c) {
  return m[0][c & 0xff] ^ m[1][(c >> 8) & 0xff] ^ m[2][(c >> 16) & 0xff] ^
         m[3][c >> 24];
}

// x^(8*r) in lane 0 (r uniform; other lanes hold partial products).
__device__ __forceinline__ uint32_t crc_xpow_wave(uint64_t r, uint32_t lane) {
  const uint32_t j = lane & 7;  // lanes 8.. mirror 0..7
  uint32_t t = c_xpow8[j][(r >> (8 * j)) & 0xff];
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
__device__ __forceinline__ uint32_t crc_bytes64(const crc_tab256* t,
                                                const uint32_t w[16],
                                                uint32_t nb) {
  uint32_t crc = 0xFFFFFFFFu;
  const uint32_t n8 = nb >> 3, rem = nb & 7;
#pragma unroll
  for (uint32_t i = 0; i < 8; i++)
    if (i < n8) crc = crc_step8(t, crc, w[2 * i], w[2 * i + 1]);
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

// One wave per run of `run` consecutive chunks; CRC_DIGEST_WAVES waves
// per workgroup share one copy of the tables.
// Message m starts at base + (offs ? offs[m] : m * msg_bytes); cpm =
// chunks per message = ceil(msg_bytes / 4096); total = n * cpm.
#define CRC_DIGEST_WAVES 16u
__global__ void __launch_bounds__(WAVE * CRC_DIGEST_WAVES) k_crc32_msgs(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ offs,
    uint64_t msg_bytes, uint64_t cpm, uint64_t total, uint64_t run,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t s_tab[8][256];
  __shared__ uint32_t s_stab[6][4][256];

  for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
    (&s_tab[0][0])[i] = (&c_crc_tab[0][0])[i];
  for (uint32_t i = threadIdx.x; i < 6 * 4 * 256; i += blockDim.x)
    (&s_stab[0][0][0])[i] = (&c_shift_tab[0][0][0])[i];
  __syncthreads();

  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE, nwv = blockDim.x / WAVE;
  const uint64_t wave = (uint64_t)blockIdx.x * nwv + wv;
  uint64_t c0 = wave * run;
  if (c0 > total) c0 = total;  // idle wave: empty run, still joins the merge
  const uint64_t c1 = (total - c0 < run) ? total : c0 + run;

  uint64_t m = 0, ci = 0;
  const uint8_t* mp = base;
  if (c0 < c1) {
    m = c0 / cpm;
    ci = c0 - m * cpm;
    mp = base + (offs ? offs[m] : m * msg_bytes);
  }
  uint32_t acc = 0;  // crc of this run's full chunks of message m so far
  // contribution of a run that ends inside a message: merged with the
  // workgroup's other waves below (0 contributes nothing)
  uint32_t pend_f = 0, pend_m = 0;

  for (uint64_t c = c0; c < c1; c++) {
    const uint64_t pos = ci * PAGE;
    const uint64_t left = msg_bytes - pos;  // > 0
    const uint8_t* seg = mp + pos + lane * SEG;
    uint64_t done;  // message bytes [.., done) are covered by acc
    if (left >= PAGE) {
      uint4 v0 = reinterpret_cast<const uint4*>(seg)[0];
      uint4 v1 = reinterpret_cast<const uint4*>(seg)[1];
      uint4 v2 = reinterpret_cast<const uint4*>(seg)[2];
      uint4 v3 = reinterpret_cast<const uint4*>(seg)[3];
      uint32_t w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                        v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
      uint32_t crc = 0xFFFFFFFFu;
#pragma unroll
      for (int i = 0; i < 8; i++)
        crc = crc_step8(s_tab, crc, w[2 * i], w[2 * i + 1]);
      crc ^= 0xFFFFFFFFu;
      // uniform log tree, as in k_crc32_pages
#pragma unroll
      for (int k = 0; k < 6; k++) {
        uint32_t partner = __shfl_xor(crc, 1u << k, WAVE);
        bool is_left = ((lane >> k) & 1u) == 0;
        uint32_t cl = is_left ? crc : partner;
        uint32_t cr = is_left ? partner : crc;
        crc = crc_apply(s_stab[k], cl) ^ cr;
      }
      acc = crc_apply(s_stab[5], crc_apply(s_stab[5], acc)) ^ crc;
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
            rocp2p_crc_xpow8(valid - (beg + nb), c_xpow8),
            crc_bytes64(s_tab, w, nb));
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
      if (c + 1 < c1) mp = base + (offs ? offs[m] : m * msg_bytes);
    } else {
      ci++;
    }
  }

  // Adjacent waves own adjacent runs, so in a long message the whole
  // workgroup's pending shares target one digest: XOR them here and
  // issue one atomic instead of one per wave (same-line atomics
  // serialize in L2).  The tables are dead after the barrier; their
  // first words carry the hand-off.
  __syncthreads();
  uint32_t* s_pend = &s_tab[0][0];
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

extern "C" hipError_t rocp2p_copy(void* dst, const void* src, uint64_t nbytes,
                                  hipStream_t stream) {
  if (nbytes % 16) return hipErrorInvalidValue;
  uint64_t nvec = nbytes / 16;
  uint32_t grid = stream_grid(nvec / 4, 256);
  hipLaunchKernelGGL(k_copy_t<false>, dim3(grid), dim3(256), 0, stream,
                     (uint4_cv*)dst, (const uint4_cv*)src, nvec);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_copy_nt(void* dst, const void* src,
                                     uint64_t nbytes, hipStream_t stream) {
  if (nbytes % 16) return hipErrorInvalidValue;
  uint64_t nvec = nbytes / 16;
  uint32_t grid = stream_grid(nvec / 4, 256);
  hipLaunchKernelGGL(k_copy_t<true>, dim3(grid), dim3(256), 0, stream,
                     (uint4_cv*)dst, (const uint4_cv*)src, nvec);
  return hipGetLastError();
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

extern "C" hipError_t rocp2p_gather(void* dst_base,
                                    const uint64_t* d_dst_offs,
                                    const uint64_t* d_src_addrs,
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
  hipLaunchKernelGGL(k_gather, dim3(grid), dim3(256), 0, stream,
                     (uint8_t*)dst_base, d_dst_offs, d_src_addrs,
                     vecs_per_msg, total, vshift);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_scatter(const void* src_base,
                                     const uint64_t* d_src_offs,
                                     const uint64_t* d_dst_addrs,
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
  hipLaunchKernelGGL(k_scatter, dim3(grid), dim3(256), 0, stream,
                     (const uint8_t*)src_base, d_src_offs, d_dst_addrs,
                     vecs_per_msg, total, vshift);
  return hipGetLastError();
}

extern "C" hipError_t rocp2p_crc32_init() {
  if (g_crc_ready) return hipSuccess;
  static uint32_t tab[8][256];
  static uint32_t stab[6][4][256];
  host_make_tables(tab, stab);
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_crc_tab), tab, sizeof(tab));
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(c_shift_tab), stab, sizeof(stab));
  if (e != hipSuccess) return e;
  static uint32_t xtab[ROCP2P_CRC_XPOW_N];
  rocp2p_crc_xpow_table(xtab);
  static uint32_t xtab8[8][256];
  rocp2p_crc_xpow8_table(xtab8, xtab);
  e = hipMemcpyToSymbol(HIP_SYMBOL(c_xpow8), xtab8, sizeof(xtab8));
  if (e != hipSuccess) return e;
  g_crc_ready = true;
  return hipSuccess;
}

extern "C" hipError_t rocp2p_crc32_pages(const void* buf, uint64_t npages,
                                         uint32_t* d_out, hipStream_t stream) {
  hipError_t e = rocp2p_crc32_init();
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
static hipError_t crc32_digest_launch(const void* base,
                                      const uint64_t* d_offs,
                                      uint64_t msg_bytes, uint32_t n,
                                      uint32_t* d_out, uint32_t grid_cap,
                                      hipStream_t stream) {
  hipError_t e = rocp2p_crc32_init();
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d_out, 0, (size_t)n * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  if (!msg_bytes) return hipSuccess;  // crc32 of nothing is 0
  uint64_t cpm = msg_bytes / PAGE + (msg_bytes % PAGE != 0);
  uint64_t total;
  if (__builtin_mul_overflow(cpm, (uint64_t)n, &total))
    return hipErrorInvalidValue;
  const uint64_t W = CRC_DIGEST_WAVES;
  uint64_t cap = grid_cap ? grid_cap : 256;
  uint64_t blocks = (total + W - 1) / W;
  if (blocks > cap) blocks = cap;
  uint64_t run = (total + W * blocks - 1) / (W * blocks);
  hipLaunchKernelGGL(k_crc32_msgs, dim3((uint32_t)blocks),
                     dim3(WAVE * CRC_DIGEST_WAVES), 0,
                     stream, (const uint8_t*)base, d_offs, msg_bytes, cpm,
                     total, run, d_out);
  return hipGetLastError();
}

// Fused design: chunk CRCs never leave the wave, so no scratch.
extern "C" uint64_t rocp2p_crc32_msgs_scratch_bytes(uint64_t msg_bytes,
                                                    uint32_t n) {
  (void)msg_bytes;
  (void)n;
  return 0;
}

extern "C" hipError_t rocp2p_crc32_msgs(const void* base,
                                        const uint64_t* d_offs,
                                        uint64_t msg_bytes, uint32_t n,
                                        uint32_t* d_out, void* d_scratch,
                                        uint32_t grid_cap,
                                        hipStream_t stream) {
  (void)d_scratch;
  if (msg_bytes % 16 || !msg_bytes || (uintptr_t)base % 16)
    return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  return crc32_digest_launch(base, d_offs, msg_bytes, n, d_out, grid_cap,
                             stream);
}

extern "C" hipError_t rocp2p_crc32_region(const void* buf, uint64_t nbytes,
                                          uint32_t* d_out, void* d_scratch,
                                          uint32_t grid_cap,
                                          hipStream_t stream) {
  (void)d_scratch;
  if ((uintptr_t)buf % 16) return hipErrorInvalidValue;
  return crc32_digest_launch(buf, nullptr, nbytes, 1, d_out, grid_cap,
                             stream);
}
