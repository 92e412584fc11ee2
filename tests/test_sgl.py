"""CPU tier for scatter/gather lists: the scan and a wave's walk over a
batch of multi-SGE messages, emulated on the host from the shared
geometry headers, and max_sge > 1 on the fake transport."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Host emulation of k_sg_scan and k_msg_engine_sg.  The work items come
# from p2p_sgl.h (rocp2p_sgl_item over the byte prefix sums, the scratch
# carved by rocp2p_sgl_carve out of exactly ROCP2P_SGL_SCRATCH_WORDS
# words), the walk from p2p_varlen.h and the chunk bodies from
# p2p_bytes.h — the very code a wave runs; a wave's 64 lanes x 4 pieces
# become a loop over 256 granules.  Every SGE lives in an allocation that
# ends exactly where its bytes end, and so does the region: it ends with
# the last message.  An SGE of length 0 points at no memory at all.  The
# yardsticks are memcpy and a bytewise CRC of the whole message.
_WALK_PROG = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "p2p_sgl.h"
#include "p2p_crc.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", \
    __LINE__, #c); return 1; } } while (0)

static constexpr rocp2p_crc_tables T = rocp2p_crc_make_tables();
static const unsigned char CANARY = 0xA5;

// the yardstick: one byte at a time, no table of the headers involved
static uint32_t crc_bytewise(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & 0xEDB88320u);
  }
  return c ^ 0xFFFFFFFFu;
}

static uint32_t crc_table(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) c = T.slice[0][(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// Bytes that start skew bytes into a 16-byte granule and end on the
// allocation's last byte.
struct Buf {
  unsigned char* base = nullptr;  // 16-byte aligned allocation
  unsigned char* msg = nullptr;   // base + skew
  uint32_t skew = 0;
  uint64_t len = 0;
  void make(uint32_t sk, uint64_t n) {
    skew = sk;
    len = n;
    if (!n) {  // nothing may be touched: an address that is no memory
      msg = reinterpret_cast<unsigned char*>((uintptr_t)0x10000 + sk);
      return;
    }
    void* p = nullptr;
    if (posix_memalign(&p, 16, sk + n)) std::abort();
    base = static_cast<unsigned char*>(p);
    msg = base + sk;
    std::memset(base, CANARY, sk + n);
    POISON(base, sk & ~7u);
  }
  int front_intact() const {
    for (uint32_t i = skew & ~7u; i < skew; i++) CHECK(base[i] == CANARY);
    return 0;
  }
  void drop() {
    if (base) {
      UNPOISON(base, skew & ~7u);
      std::free(base);
    }
    base = msg = nullptr;
  }
};

struct Sge { uint64_t len; uint32_t skew; };
typedef std::vector<std::vector<Sge>> Spec;  // per message, its SGEs

struct Batch {
  bool gather = true;
  uint64_t n = 0, S = 0, total = 0;
  std::vector<uint64_t> offs, start, addrs, lens;  // the CSR batch
  std::vector<uint64_t> mlen;                      // L_m
  void* scratch = nullptr;
  rocp2p_sgl_view v;
  Buf region;  // the messages back to back from region.skew on
  std::vector<Buf> sge;
  std::vector<unsigned char> data;  // what the messages carry, in order
  std::vector<uint32_t> want;       // bytewise digests
  std::vector<uint64_t> chunk_sge;  // chunk -> SGE, naive
  ~Batch() {
    region.drop();
    for (auto& b : sge) b.drop();
    std::free(scratch);
  }
};

// Lay the batch out and run the scan the way k_sg_scan does: the byte
// prefix sums and the owners (heads and a running maximum) first, then
// rocp2p_sgl_item per SGE and the chunk prefix sums.  Everything it wrote is checked against a naive derivation.
static int make_batch(Batch& b, const Spec& spec, uint32_t rskew,
                      bool gather) {
  b.gather = gather;
  b.n = spec.size();
  uint64_t bytes = 0;
  for (const auto& m : spec) {
    b.start.push_back(b.S);
    b.offs.push_back(rskew + bytes);
    uint64_t L = 0;
    for (const Sge& e : m) {
      Buf buf;
      buf.make(e.skew, e.len);
      b.sge.push_back(buf);
      b.addrs.push_back((uint64_t)(uintptr_t)buf.msg);
      b.lens.push_back(e.len);
      L += e.len;
      b.S++;
    }
    b.mlen.push_back(L);
    bytes += L;
  }
  b.start.push_back(b.S);
  b.region.make(rskew, bytes);
  b.data.resize(bytes);
  for (auto& x : b.data) x = (unsigned char)rnd();
  uint64_t at = 0;
  for (uint64_t m = 0; m < b.n; m++) {
    b.want.push_back(crc_bytewise(b.data.data() + at, b.mlen[m]));
    at += b.mlen[m];
  }
  const uint64_t region0 = (uint64_t)(uintptr_t)b.region.msg - rskew;
  CHECK(region0 % 16 == 0);

  const uint64_t words = ROCP2P_SGL_SCRATCH_WORDS(b.n, b.S);
  b.scratch = std::malloc(words * 8);
  b.v = rocp2p_sgl_carve(static_cast<uint64_t*>(b.scratch), b.S);
  CHECK((unsigned char*)(b.v.owner + b.S) <=
        (unsigned char*)b.scratch + words * 8);
  uint64_t sum = 0;
  for (uint64_t j = 0; j < b.S; j++) {
    b.v.prefix[j] = sum;
    sum += b.lens[j];
  }
  b.v.prefix[b.S] = sum;
  // owners: heads, then the running maximum
  for (uint64_t j = 0; j < b.S; j++) b.v.owner[j] = 0;
  for (uint64_t m = 0; m < b.n; m++)
    if (rocp2p_sgl_has_sges(b.start.data(), m))
      b.v.owner[b.start[m]] = (uint32_t)m;
  for (uint64_t j = 1; j < b.S; j++)
    if (b.v.owner[j] < b.v.owner[j - 1]) b.v.owner[j] = b.v.owner[j - 1];
  for (uint64_t j = 0; j < b.S; j++) {
    b.v.cstart[j] = b.total;
    const uint64_t k =
        rocp2p_sgl_item(b.v, region0, b.offs.data(), b.start.data(),
                        b.addrs.data(), j, gather);
    for (uint64_t i = 0; i < k; i++) b.chunk_sge.push_back(j);
    b.total += k;
  }
  b.v.cstart[b.S] = b.total;

  // naive: message by message
  uint64_t j = 0, msg_at = 0;
  for (uint64_t m = 0; m < b.n; m++) {
    uint64_t in_msg = 0;
    for (size_t k = 0; k < spec[m].size(); k++, j++) {
      const uint64_t inside = (uint64_t)(uintptr_t)b.region.msg + msg_at + in_msg;
      CHECK(rocp2p_sgl_owner(b.start.data(), b.n, j) == m);
      CHECK(b.v.owner[j] == m);
      CHECK(b.v.to[j] == (gather ? inside : b.addrs[j]));
      CHECK(b.v.from[j] == (gather ? b.addrs[j] : inside));
      in_msg += b.lens[j];
      CHECK(b.v.tail[j] == b.mlen[m] - in_msg);
      CHECK(b.v.cstart[j + 1] - b.v.cstart[j] ==
            rocp2p_b_chunks((uint32_t)b.v.to[j] & 15u, b.lens[j]));
    }
    msg_at += b.mlen[m];
  }
  CHECK(j == b.S);
  return 0;
}

struct Pending { uint32_t f = 0, m = 0; };

// crc of the bytes [lo, hi) of a granule held in registers
static uint32_t crc_range(const rocp2p_g16& v, uint32_t lo, uint32_t hi) {
  unsigned char raw[16];
  std::memcpy(raw, &v, 16);
  return crc_table(raw + lo, hi - lo);
}

// One wave's run [c0, c1), the way k_msg_engine_sg walks it.
static int wave_walk(const Batch& b, uint64_t c0, uint64_t c1,
                     std::vector<uint32_t>& out, std::vector<int>& visits,
                     Pending& pend) {
  rocp2p_vl_cursor cur = {0, 0, 0, 0};
  if (c0 < c1) rocp2p_vl_seek(&cur, b.v.cstart, b.lens.data(), b.S, c0);
  uint32_t acc = 0;
  for (uint64_t c = c0; c < c1; c++) {
    CHECK(cur.m < b.S && cur.m == b.chunk_sge[c]);   // the right SGE
    CHECK(cur.len == b.lens[cur.m] && cur.len > 0);  // never an empty one
    CHECK(b.v.cstart[cur.m] + cur.ci == c);
    visits[c]++;
    const uint64_t to = b.v.to[cur.m], from = b.v.from[cur.m];
    const uint64_t tail = b.v.tail[cur.m];
    const uint32_t owner = b.v.owner[cur.m];
    const uint32_t skew = (uint32_t)to & 15u;
    const uint32_t rel = (uint32_t)(from - to) & 15u;
    CHECK(cur.cpm == rocp2p_b_chunks(skew, cur.len) && cur.ci < cur.cpm);
    const uint64_t p0 = cur.ci * 4096, end = skew + cur.len;
    const unsigned char* sp = reinterpret_cast<const unsigned char*>(
        (uintptr_t)(from - skew - rel + p0));
    unsigned char* dp =
        reinterpret_cast<unsigned char*>((uintptr_t)(to - skew + p0));
    CHECK((uintptr_t)sp % 16 == 0 && (uintptr_t)dp % 16 == 0);
    const bool full = rocp2p_b_full(skew, rel, cur.len, cur.ci);
    const uint64_t g0 = cur.ci * ROCP2P_B_PER_CHUNK;
    const uint64_t sbeg = (uint64_t)skew + rel, send = end + rel;
    const rocp2p_g16 none = {0, 0, 0, 0};
    static rocp2p_g16 a[257], v[256];
    for (uint32_t q = 0; q < 256u + (rel != 0); q++) {
      uint32_t lo = 0, hi = 16;
      if (!full) rocp2p_b_range(sbeg, send, g0 + q, &lo, &hi);
      a[q] = rocp2p_b_load(sp + 16 * q, lo, hi);
    }
    if (!rel) a[256] = none;
    for (uint32_t q = 0; q < 256; q++)
      v[q] = rel ? rocp2p_b_realign(a[q], a[q + 1], rel) : a[q];
    uint64_t done;
    if (full) {
      for (uint32_t q = 0; q < 256; q++)
        rocp2p_b_store(dp + 16 * q, 0, 16, v[q]);
      acc = rocp2p_crc_apply(T.shift[5], rocp2p_crc_apply(T.shift[5], acc)) ^
            crc_table(reinterpret_cast<const unsigned char*>(v), 4096);
      done = p0 + 4096;
    } else {
      uint32_t x = 0;
      for (uint32_t q = 0; q < 256; q++) {
        uint32_t lo, hi;
        rocp2p_b_range(skew, end, g0 + q, &lo, &hi);
        if (lo >= hi) continue;
        rocp2p_b_store(dp + 16 * q, lo, hi, v[q]);
        x ^= rocp2p_crc_mulmod(
            rocp2p_crc_xpow8(end - ((g0 + q) * 16 + hi), T.xpow8),
            crc_range(v[q], lo, hi));
      }
      // the tail shifts the chunk's sum once
      if (tail) x = rocp2p_crc_mulmod(rocp2p_crc_xpow8(tail, T.xpow8), x);
      out[owner] ^= x;
      done = p0;
    }
    const bool sge_end = cur.ci + 1 == cur.cpm, run_end = c + 1 == c1;
    if (sge_end || run_end || !full) {
      if (acc) {
        const uint64_t r = end - done + tail;
        uint32_t f = acc;
        if (r) f = rocp2p_crc_mulmod(rocp2p_crc_xpow8(r, T.xpow8), acc);
        if (run_end && !sge_end) {
          pend.f = f;
          pend.m = owner;
        } else {
          out[owner] ^= f;
        }
      }
      acc = 0;
    }
    if (c + 1 < c1) rocp2p_vl_next(&cur, b.v.cstart, b.lens.data());
  }
  return 0;
}

// the workgroup merge: equal targets are adjacent
static void merge(const std::vector<Pending>& p, std::vector<uint32_t>& out) {
  uint32_t f = p[0].f, fm = p[0].m;
  for (size_t w = 1; w < p.size(); w++) {
    if (p[w].m != fm) {
      if (f) out[fm] ^= f;
      f = 0;
      fm = p[w].m;
    }
    f ^= p[w].f;
  }
  if (f) out[fm] ^= f;
}

// load the sending side with the data, the receiving side with canaries
static void reset(Batch& b) {
  uint64_t at = 0;
  unsigned char* reg = b.region.msg;
  if (b.region.len)
    std::memcpy(reg, b.data.data(), b.region.len);
  for (uint64_t j = 0; j < b.S; j++) {
    if (!b.lens[j]) continue;
    if (b.gather)
      std::memcpy(b.sge[j].msg, b.data.data() + at, b.lens[j]);
    else
      std::memset(b.sge[j].msg, CANARY, b.lens[j]);
    at += b.lens[j];
  }
  if (b.gather && b.region.len) std::memset(reg, CANARY, b.region.len);
}

// a whole launch: runs[w] = [c0, c1) of wave w, wpg waves per workgroup
static int launch(Batch& b,
                  const std::vector<std::pair<uint64_t, uint64_t>>& runs,
                  size_t wpg) {
  reset(b);
  std::vector<uint32_t> out(b.n, 0);
  std::vector<int> visits(b.total, 0);
  for (size_t g = 0; g < runs.size(); g += wpg) {
    std::vector<Pending> pend(wpg);
    for (size_t w = 0; w < wpg && g + w < runs.size(); w++)
      if (wave_walk(b, runs[g + w].first, runs[g + w].second, out, visits,
                    pend[w]))
        return 1;
    merge(pend, out);
  }
  for (uint64_t c = 0; c < b.total; c++) CHECK(visits[c] == 1);
  for (uint64_t m = 0; m < b.n; m++) {
    CHECK(out[m] == b.want[m]);
    if (!b.mlen[m]) CHECK(out[m] == 0);
  }
  // every byte where memcpy would have put it, nothing in front touched
  if (b.region.len) {
    CHECK(!std::memcmp(b.region.msg, b.data.data(), b.region.len));
    if (b.region.front_intact()) return 1;
  }
  uint64_t at = 0;
  for (uint64_t j = 0; j < b.S; j++) {
    if (!b.lens[j]) continue;
    CHECK(!std::memcmp(b.sge[j].msg, b.data.data() + at, b.lens[j]));
    if (b.sge[j].front_intact()) return 1;
    at += b.lens[j];
  }
  return 0;
}

static int derived(Batch& b, uint64_t nwaves, size_t wpg) {
  std::vector<std::pair<uint64_t, uint64_t>> runs(nwaves);
  uint64_t next = 0;
  for (uint64_t w = 0; w < nwaves; w++) {
    rocp2p_vl_run(b.total, nwaves, w, &runs[w].first, &runs[w].second);
    CHECK(runs[w].first == next && runs[w].second >= next);
    next = runs[w].second;
  }
  CHECK(next == b.total);
  return launch(b, runs, wpg);
}

// 1, 3 and 64 waves, in workgroups of 4 and of 1; every == true adds
// every run length from 1 to total + 1 with an idle wave behind
static int check_batch(const Spec& spec, uint32_t rskew, bool every) {
  for (int g = 0; g < 2; g++) {
    Batch b;
    if (make_batch(b, spec, rskew, g == 0)) return 1;
    for (uint64_t nwaves : {1, 3, 64})
      for (size_t wpg : {4, 1})
        if (derived(b, nwaves, wpg)) return 1;
    if (every)
      for (uint64_t run = 1; run <= b.total + 1; run++) {
        std::vector<std::pair<uint64_t, uint64_t>> runs;
        for (uint64_t c0 = 0; c0 < b.total; c0 += run)
          runs.push_back({c0, c0 + run < b.total ? c0 + run : b.total});
        runs.push_back({b.total, b.total});
        if (launch(b, runs, 4)) return 1;
      }
  }
  return 0;
}

int main() {
  CHECK(ROCP2P_SGL_SCRATCH_WORDS(0, 0) == 2 &&
        ROCP2P_SGL_SCRATCH_WORDS(7, 1) == 8 &&
        ROCP2P_SGL_SCRATCH_WORDS(1, 2) == 13);
  // one message of L bytes, cut in every way of the list, at every
  // region skew; SGE k sits at skew (7k + 3) & 15 outside
  const uint64_t L = 3 * 4096 + 2049;
  const std::vector<std::vector<uint64_t>> cuts = {
      {L}, {1, L - 1}, {L - 1, 1}, {15, 17, 4064, L - 4096},
      {4096, 4096, L - 8192}, {0, 4097, 0, 0, L - 4097, 0}};
  for (uint32_t rs = 0; rs < 16; rs++)
    for (const auto& cut : cuts) {
      std::vector<Sge> m;
      uint64_t sum = 0;
      for (size_t k = 0; k < cut.size(); k++) {
        m.push_back({cut[k], (uint32_t)((7 * k + 3) & 15)});
        sum += cut[k];
      }
      CHECK(sum == L);
      if (check_batch({m}, rs, rs == 0 || rs == 5 || rs == 15)) return 1;
    }
  // runs of empty messages and empty SGEs in front, in the middle and at
  // the end; neighbours that meet inside a granule
  const Spec ragged = {
      {}, {}, {{0, 3}}, {{0, 1}, {0, 2}},
      {{5, 9}},
      {{1, 0}, {0, 4}, {30, 15}, {4097, 8}},
      {}, {{0, 0}}, {},
      {{4096, 0}, {4096, 1}, {16, 15}},
      {{3, 13}, {0, 0}, {0, 0}, {8191, 2}, {17, 7}},
      {{0, 5}}, {}, {}};
  for (uint32_t rs : {0u, 9u, 15u})
    if (check_batch(ragged, rs, true)) return 1;
  if (check_batch({{}, {{0, 1}}, {}}, 7, true)) return 1;  // no byte at all
  if (check_batch({}, 0, true)) return 1;                  // no message
  // more messages and SGEs than a wave is wide, seeded
  for (int rep = 0; rep < 6; rep++) {
    const uint64_t pick[] = {0, 0, 1, 3, 15, 16, 17, 33, 48, 4095, 4096, 4097};
    Spec spec(1 + rnd() % 90);
    for (auto& m : spec) {
      m.resize(rnd() % 5);
      for (auto& e : m)
        e = {pick[rnd() % (rep < 3 ? 9 : 12)], (uint32_t)(rnd() % 16)};
    }
    if (check_batch(spec, (uint32_t)(rnd() % 16), false)) return 1;
  }
  std::printf("OK\n");
  return 0;
}
"""


def _build_and_run_walk(tmp_path, extra):
    src = tmp_path / "sgl_walk_check.cpp"
    exe = tmp_path / "sgl_walk_check"
    src.write_text(_WALK_PROG)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra,
         "-I", os.path.join(ROOT, "rocnrdma_amd", "ops", "csrc"),
         str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sgl_walk_copies_every_byte_once_and_digests_match(tmp_path):
    """One message of 3 * 4096 + 2049 bytes in the six cuts, at all 16
    region skews, gathered and scattered by 1, 3 and 64 waves; ragged
    batches with runs of empty messages and SGEs; the scan's output
    against a naive derivation."""
    _build_and_run_walk(tmp_path, [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sgl_walk_under_sanitizers(tmp_path):
    """The same stand-alone program with ASan and UBSan: no byte outside
    an SGE or outside the region's messages is read or written, and the
    scratch is exactly as large as the header says."""
    _build_and_run_walk(tmp_path, ["-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"])


# -- fake transport ----------------------------------------------------------
MSG, REGION = 8192, 128 << 10
K = 3
KNOWN = 0xC3


def _open(direction, region_skew=0, **kw):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction, var_len=True, byte_granular=True,
                       region_skew=region_skew, max_sge=K, **kw)
    rng = np.random.default_rng(23)
    tp.staging[:] = rng.integers(0, 256, tp.staging.shape, dtype=np.uint8)
    tp.region[:] = rng.integers(0, 256, REGION, dtype=np.uint8)
    return tp


def _layout(tp, seed=3):
    """(msgs_per_region, K, 2) disjoint lists: an empty message, a 1-byte
    SGE, a message that fills the slot, SGEs out of slot order."""
    import random

    from rocnrdma_amd.harness.soak import mixed_sges

    room = MSG - tp.region_skew
    sges = mixed_sges(random.Random(seed), tp.msgs_per_region, MSG, K, room,
                      disjoint=True)
    sges[0] = 0
    sges[1] = [(4096, 1), (0, 0), (17, 4000)]
    sges[2] = [(0, room), (0, 0), (0, 0)]
    sges[3] = [(5000, 33), (100, 4097), (4300, 15)]
    return sges


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


@pytest.mark.parametrize("region_skew", [0, 9])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_post_sg_moves_the_concatenation(direction, region_skew):
    tp = _open(direction, region_skew)
    assert tp.supports_sg_list and tp.max_sge == K
    rs, n = region_skew, tp.msgs_per_region
    sges = _layout(tp)
    assert tp.inflight < n  # slots are reused: check as we go
    recv = tp.region if direction == "write" else tp.staging
    recv[...] = KNOWN
    staging0, region0 = tp.staging.copy(), tp.region.copy()
    for i in range(n):
        slot = tp.staging[i % tp.inflight]
        tp.post_sg(i, [tuple(map(int, e)) for e in sges[i]])
        tp.flush()
        ln = int(sges[i, :, 1].sum())
        msg = tp.region[i * MSG:(i + 1) * MSG]
        cat = np.concatenate([slot[o:o + k] for o, k in sges[i]])
        assert (msg[rs:rs + ln] == cat).all()
        if direction == "write":  # slack untouched, in front and behind
            assert (msg[:rs] == KNOWN).all() and (msg[rs + ln:] == KNOWN).all()
        else:
            rest = np.ones(MSG, dtype=bool)
            for o, k in sges[i]:
                rest[o:o + k] = False
            assert (slot[rest] == KNOWN).all()
            slot[:] = KNOWN  # for the message that reuses the slot
    if direction == "write":  # the sending side is only read
        assert (tp.staging == staging0).all()
    else:
        assert (tp.region == region0).all()
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_post_equals_a_one_entry_list(direction):
    a, b, c = _open(direction, 9), _open(direction, 9), _open(direction, 9)
    n = a.msgs_per_region
    lens = np.random.default_rng(6).integers(0, MSG - 8, n)
    sges = np.zeros((n, K, 2), dtype=np.int64)
    sges[:, 0, 1] = lens
    for i in range(n):
        a.post(i, int(lens[i]))
        b.post_sg(i, [(0, int(lens[i]))])
    c.post_many_sg(0, n, sges)
    a.post_many(0, 2)  # None: the most that fits
    b.post_sg(0, [(0, MSG - 9)])
    b.post_sg(1, [(0, MSG - 9)])
    c.post_many(0, 2, MSG - 9)
    for x in (b, c):
        assert (a.region == x.region).all()
        assert (a.staging == x.staging).all()
        x.close()
    a.close()


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("region_skew", [0, 9])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_digest_check_sg(direction, region_skew, icrc):
    tp = _open(direction, region_skew, icrc=icrc)
    sges = _layout(tp)
    assert tp.digest_check_sg(_payload(1), sges) == 0
    assert tp.digest_check_sg(_payload(2), np.zeros_like(sges)) == 0
    if direction == "write":  # sources may overlap
        over = sges.copy()
        over[:, :, 0] = 7
        over[:, :, 1] = np.minimum(over[:, :, 1], 2000)
        assert tp.digest_check_sg(_payload(3), over) == 0

    # negative control: one SGE of one message is dropped on the way
    real = tp.post_sg

    def lossy(i, s):
        s = np.array(s)
        if i == 3:
            s[1] = 0
        real(i, s)

    tp.post_sg = lossy
    assert tp.digest_check_sg(_payload(4), sges) == 1
    # a slack byte right behind the message changes
    def poke(i, s):
        real(i, s)
        if i == 3:
            if direction == "write":
                tp.region[3 * MSG + region_skew + 33 + 4097 + 15] ^= 0xFF
            else:
                tp.staging[3 % tp.inflight][5000 + 33] ^= 0xFF

    tp.post_sg = poke
    assert tp.digest_check_sg(_payload(5), sges) == 1
    tp.post_sg = real
    assert tp.digest_check_sg(_payload(6), sges) == 0
    tp.close()


def test_sg_list_validation():
    kw = dict(msg_bytes=MSG, region_bytes=REGION)
    with pytest.raises(ValueError, match="byte_granular"):
        get_transport("fake", max_sge=2, **kw)
    with pytest.raises(ValueError, match="byte_granular"):
        get_transport("fake", max_sge=2, var_len=True, **kw)
    with pytest.raises(ValueError, match="staging_skew"):
        get_transport("fake", max_sge=2, var_len=True, byte_granular=True,
                      staging_skew=3, **kw)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_sge"):
            get_transport("fake", max_sge=bad, **kw)
    # the default changes nothing, and has no lists
    tp = get_transport("fake", var_len=True, byte_granular=True, **kw)
    assert tp.max_sge == 1
    with pytest.raises(ValueError, match="max_sge"):
        tp.post_sg(0, [(0, 16)])
    tp.close()

    for direction in ("write", "read"):
        tp = _open(direction, 9)
        ok = [(0, 10), (100, 20), (200, 30)]
        tp.post_sg(0, ok)
        tp.post_sg(0, [])
        tp.post_sg(0, [(MSG, 0)])
        tp.post_sg(0, [(MSG - 1, 1)])
        errors = {
            "too many": ok + [(300, 1)],
            "outside": [(MSG - 10, 11)],
            "outside_off": [(MSG + 1, 0)],
            "negative off": [(-1, 4)],
            "negative len": [(0, -4)],
            "non-integer": [(0, 2.5)],
            "not pairs": [(0, 1, 2)],
            "total": [(0, 4096), (4096, 4096 - 8)],  # + skew 9 > MSG
        }
        for what, sges in errors.items():
            with pytest.raises(ValueError):
                tp.post_sg(0, sges)
            arr = np.zeros((2, K, 2), dtype=np.int64)
            if len(sges) <= K and what not in ("non-integer", "not pairs"):
                arr[1, :len(sges)] = sges
                with pytest.raises(ValueError):
                    tp.post_many_sg(0, 2, arr)
        with pytest.raises(ValueError, match="shape"):
            tp.post_many_sg(0, 2, np.zeros((2, K + 1, 2), dtype=np.int64))
        with pytest.raises(ValueError, match="shape"):
            tp.digest_check_sg(_payload(1), np.zeros((2, K, 2), np.int64))
        overlap = [(0, 100), (300, 10), (99, 5)]
        if direction == "read":  # the side that is written
            with pytest.raises(ValueError, match="overlap"):
                tp.post_sg(0, overlap)
            tp.post_sg(0, [(0, 100), (50, 0), (100, 5)])  # empty: no overlap
        else:
            tp.post_sg(0, overlap)
        tp.close()


@pytest.mark.parametrize("name", ["shm", "verbs"])
def test_sg_list_not_implemented_elsewhere(name):
    with pytest.raises(NotImplementedError):
        get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                      host="127.0.0.1", port=1, var_len=True,
                      byte_granular=True, max_sge=2)
    with pytest.raises(NotImplementedError, match="max_sge"):
        get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                      host="127.0.0.1", port=1, max_sge=2)


def test_soak_sg_on_fake():
    import random

    from rocnrdma_amd.harness.soak import mixed_sges, run_soak

    for disjoint in (False, True):
        s = mixed_sges(random.Random(2), 3000, 8192, 3, 8183, disjoint)
        assert s.shape == (3000, 3, 2) and s.dtype == np.int64
        off, ln = s[:, :, 0], s[:, :, 1]
        assert (off >= 0).all() and (ln >= 0).all()
        assert (off + ln <= 8192).all() and ln.sum(axis=1).max() == 8183
        assert (ln.sum(axis=1) == 0).any() and (ln == 1).any()
        assert ((ln > 0).sum(axis=1) == 3).any()
    with pytest.raises(ValueError, match="byte_granular"):
        run_soak("fake", secs=0.1, mixed=True, sg=3)
    with pytest.raises(ValueError, match="sg"):
        run_soak("fake", secs=0.1, mixed=True, byte_granular=True, sg=1)
    for icrc in (False, True):
        stats = run_soak("fake", secs=0.3, region_bytes=1 << 20, seed=5,
                         mixed=True, byte_granular=True, icrc=icrc, sg=3)
        assert stats["cycles"] > 0 and stats["failures"] == 0
        assert 0 < stats["bytes"]
