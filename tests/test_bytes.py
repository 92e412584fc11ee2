"""CPU tier for byte-granular messages: a wave's walk over a batch of
messages of any length at any address, emulated on the host from the
shared geometry header (source loads, realignment, stores, digests), and
byte_granular=True on the fake transport."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Host emulation of k_msg_engine_b and k_crc32_msgs_b.  The chunk count,
# the fast-path test, the per-granule byte ranges, the ranged loads and
# stores and the realignment are p2p_bytes.h's, the very code a wave
# runs; a wave's 64 lanes x 4 pieces become a loop over 256 granules and
# the lane shuffle an index + 1.  Every message's source and destination
# live in allocations that end exactly where the message ends and start
# on the granule the message starts in; the bytes in front of the
# message are poisoned as far as ASan's 8-byte shadow allows, and the
# rest of them (at most 7) are covered by the exhaustive check of the
# access decomposition (rocp2p_b_width) and, on the written side, by
# canaries.
_WALK_PROG = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "p2p_bytes.h"
#include "p2p_crc.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

// A buffer whose message starts skew bytes into a 16-byte granule and
// ends on the allocation's last byte.
struct Buf {
  unsigned char* base = nullptr;  // 16-byte aligned allocation
  unsigned char* msg = nullptr;   // base + skew
  uint32_t skew = 0;
  uint64_t len = 0;
  void make(uint32_t sk, uint64_t n, bool random) {
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
    for (uint32_t i = 0; i < sk; i++) base[i] = CANARY;
    for (uint64_t i = 0; i < n; i++)
      msg[i] = random ? (unsigned char)rnd() : CANARY;
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

struct Batch {
  std::vector<uint64_t> lens, cstart;  // cstart: n + 1, the scan
  std::vector<Buf> src, dst;
  std::vector<uint32_t> want;   // bytewise digests
  std::vector<uint64_t> owner;  // chunk -> message, naive
  uint64_t total = 0;
  ~Batch() {
    for (auto& b : src) b.drop();
    for (auto& b : dst) b.drop();
  }
};

struct Spec { uint64_t len; uint32_t sskew, dskew; };

static void make_batch(Batch& b, const std::vector<Spec>& specs) {
  for (const Spec& s : specs) {
    b.lens.push_back(s.len);
    b.cstart.push_back(b.total);
    const uint64_t k = rocp2p_b_chunks(s.dskew, s.len);
    for (uint64_t i = 0; i < k; i++) b.owner.push_back(b.src.size());
    b.total += k;
    Buf in, out;
    in.make(s.sskew, s.len, true);
    out.make(s.dskew, s.len, false);
    b.want.push_back(crc_bytewise(s.len ? in.msg : nullptr, s.len));
    b.src.push_back(in);
    b.dst.push_back(out);
  }
  b.cstart.push_back(b.total);
}

struct Pending { uint32_t f = 0, m = 0; };

// crc of the bytes [lo, hi) of a granule held in registers
static uint32_t crc_range(const rocp2p_g16& v, uint32_t lo, uint32_t hi) {
  unsigned char raw[16];
  std::memcpy(raw, &v, 16);
  return crc_table(raw + lo, hi - lo);
}

// One wave's run [c0, c1), the way the kernels walk it.  digest_only:
// k_crc32_msgs_b over the landed bytes (reads dst, stores nothing).
static int wave_walk(const Batch& b, bool digest_only, uint64_t c0,
                     uint64_t c1, std::vector<uint32_t>& out,
                     std::vector<int>& visits, Pending& pend) {
  const uint64_t n = b.lens.size();
  rocp2p_vl_cursor cur = {0, 0, 0, 0};
  if (c0 < c1) rocp2p_vl_seek(&cur, b.cstart.data(), b.lens.data(), n, c0);
  uint32_t acc = 0;
  for (uint64_t c = c0; c < c1; c++) {
    CHECK(cur.m < n && cur.m == b.owner[c]);         // the right message
    CHECK(cur.len == b.lens[cur.m] && cur.len > 0);  // never a zero-length
    CHECK(b.cstart[cur.m] + cur.ci == c);
    visits[c]++;
    const uintptr_t to = (uintptr_t)b.dst[cur.m].msg;
    const uintptr_t from = digest_only ? to : (uintptr_t)b.src[cur.m].msg;
    const uint32_t skew = (uint32_t)to & 15u;
    const uint32_t rel = (uint32_t)(from - to) & 15u;
    CHECK(cur.cpm == rocp2p_b_chunks(skew, cur.len) && cur.ci < cur.cpm);
    const uint64_t p0 = cur.ci * 4096, end = skew + cur.len;
    const unsigned char* sp =
        reinterpret_cast<const unsigned char*>(from - skew - rel + p0);
    unsigned char* dp = reinterpret_cast<unsigned char*>(to - skew + p0);
    CHECK((uintptr_t)sp % 16 == 0 && (uintptr_t)dp % 16 == 0);
    const bool full = rocp2p_b_full(skew, rel, cur.len, cur.ci);
    const uint64_t g0 = cur.ci * ROCP2P_B_PER_CHUNK;
    const uint64_t sbeg = (uint64_t)skew + rel, send = end + rel;
    const rocp2p_g16 none = {0, 0, 0, 0};
    static rocp2p_g16 a[257], v[256];
    // source granules: each loaded once, the 257th only when rel != 0
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
      if (!digest_only)
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
        if (!digest_only) rocp2p_b_store(dp + 16 * q, lo, hi, v[q]);
        x ^= rocp2p_crc_mulmod(
            rocp2p_crc_xpow8(end - ((g0 + q) * 16 + hi), T.xpow8),
            crc_range(v[q], lo, hi));
      }
      out[cur.m] ^= x;
      done = p0;
    }
    const bool msg_end = cur.ci + 1 == cur.cpm, run_end = c + 1 == c1;
    if (msg_end || run_end || !full) {
      if (acc) {
        const uint64_t r = end - done;
        uint32_t f = acc;
        if (r) f = rocp2p_crc_mulmod(rocp2p_crc_xpow8(r, T.xpow8), acc);
        if (run_end && !msg_end) {
          pend.f = f;
          pend.m = (uint32_t)cur.m;
        } else {
          out[cur.m] ^= f;
        }
      }
      acc = 0;
    }
    if (c + 1 < c1) rocp2p_vl_next(&cur, b.cstart.data(), b.lens.data());
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

// a whole launch: runs[w] = [c0, c1) of wave w, wpg waves per workgroup
static int launch(Batch& b, bool digest_only,
                  const std::vector<std::pair<uint64_t, uint64_t>>& runs,
                  size_t wpg) {
  const size_t n = b.lens.size();
  if (!digest_only)
    for (size_t m = 0; m < n; m++)
      if (b.lens[m]) std::memset(b.dst[m].msg, CANARY, b.lens[m]);
  std::vector<uint32_t> out(n, 0);
  std::vector<int> visits(b.total, 0);
  for (size_t g = 0; g < runs.size(); g += wpg) {
    std::vector<Pending> pend(wpg);
    for (size_t w = 0; w < wpg && g + w < runs.size(); w++)
      if (wave_walk(b, digest_only, runs[g + w].first, runs[g + w].second,
                    out, visits, pend[w]))
        return 1;
    merge(pend, out);
  }
  for (uint64_t c = 0; c < b.total; c++) CHECK(visits[c] == 1);
  for (size_t m = 0; m < n; m++) {
    CHECK(out[m] == b.want[m]);
    if (!b.lens[m]) CHECK(out[m] == 0);
    if (b.lens[m]) {  // every byte copied, nothing in front touched
      CHECK(!std::memcmp(b.dst[m].msg, b.src[m].msg, b.lens[m]));
      if (b.dst[m].front_intact() || b.src[m].front_intact()) return 1;
    }
  }
  return 0;
}

static int check_batch(const std::vector<Spec>& specs,
                       std::initializer_list<size_t> wpgs) {
  Batch b;
  make_batch(b, specs);
  for (size_t wpg : wpgs) {
    // every run length from 1 to total + 1, with an idle wave behind
    for (uint64_t run = 1; run <= b.total + 1; run++) {
      std::vector<std::pair<uint64_t, uint64_t>> runs;
      for (uint64_t c0 = 0; c0 < b.total; c0 += run)
        runs.push_back({c0, c0 + run < b.total ? c0 + run : b.total});
      runs.push_back({b.total, b.total});
      if (launch(b, false, runs, wpg) || launch(b, true, runs, wpg)) return 1;
    }
    // and the runs the kernels derive themselves, for every wave count
    for (uint64_t nwaves = 1; nwaves <= b.total + 2; nwaves++) {
      std::vector<std::pair<uint64_t, uint64_t>> runs(nwaves);
      uint64_t next = 0;
      for (uint64_t w = 0; w < nwaves; w++) {
        rocp2p_vl_run(b.total, nwaves, w, &runs[w].first, &runs[w].second);
        CHECK(runs[w].first == next && runs[w].second >= next);
        next = runs[w].second;
      }
      CHECK(next == b.total);
      if (launch(b, false, runs, wpg) || launch(b, true, runs, wpg)) return 1;
    }
  }
  return 0;
}

int main() {
  // the geometry on its own
  CHECK(rocp2p_b_chunks(0, 0) == 0 && rocp2p_b_chunks(15, 0) == 0 &&
        rocp2p_b_chunks(15, 1) == 1 && rocp2p_b_chunks(1, 4095) == 1 &&
        rocp2p_b_chunks(1, 4096) == 2 && rocp2p_b_chunks(15, 8177) == 2 &&
        rocp2p_b_chunks(15, 8178) == 3 &&
        rocp2p_b_chunks(15, ~0ull) == (1ull << 52) + 1);
  for (uint64_t len = 0; len <= 5 * 4096; len += 16)
    CHECK(rocp2p_b_chunks(0, len) == rocp2p_vl_chunks(len));
  for (uint64_t len : {(1ull << 40), (1ull << 63) + 4096, ~0ull - 15})
    CHECK(rocp2p_b_chunks(0, len) == rocp2p_vl_chunks(len));
  for (uint32_t skew = 0; skew < 16; skew++)
    for (uint64_t len = 1; len < 3 * 4096 + 40; len++)
      CHECK(rocp2p_b_chunks(skew, len) == (skew + len + 4095) / 4096);
  // the accesses of a partial granule: naturally aligned, and a tiling
  // of exactly [lo, hi)
  for (uint32_t lo = 0; lo < 16; lo++)
    for (uint32_t hi = lo + 1; hi <= 16; hi++) {
      uint32_t p = lo, steps = 0;
      while (p < hi) {
        const uint32_t w = rocp2p_b_width(p, hi);
        CHECK((w == 1 || w == 2 || w == 4 || w == 8) && p % w == 0 &&
              p + w <= hi);
        p += w;
        steps++;
      }
      CHECK(p == hi && steps <= 7);
    }

  const uint64_t small[] = {0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 33, 255};
  const uint64_t large[] = {4079, 4081, 4095, 4096, 4097, 4111, 4113, 8193};
  for (uint32_t ss = 0; ss < 16; ss++)
    for (uint32_t ds = 0; ds < 16; ds++) {
      std::vector<Spec> a, b;
      for (uint64_t len : small) a.push_back({len, ss, ds});
      for (uint64_t len : large) b.push_back({len, ss, ds});
      const bool all = (ss == 0 && ds == 0) || (ss == 3 && ds == 11) ||
                       (ss == 15 && ds == 1) || (ss == 9 && ds == 9);
      if (all ? check_batch(a, {1, 4, 16}) || check_batch(b, {1, 4, 16})
              : check_batch(a, {4}) || check_batch(b, {4}))
        return 1;
    }
  // every message at its own pair of skews, zero lengths in between, a
  // message of many chunks
  const uint64_t pick[] = {0, 0, 1, 3, 16, 33, 1023, 4080, 4095, 4096,
                           4097, 4113, 8191, 3 * 4096 + 2049, 20001};
  for (int rep = 0; rep < 10; rep++) {
    std::vector<Spec> specs(1 + rnd() % 12);
    for (auto& s : specs)
      s = {pick[rnd() % (sizeof(pick) / sizeof(pick[0]))],
           (uint32_t)(rnd() % 16), (uint32_t)(rnd() % 16)};
    if (check_batch(specs, {1, 4, 16})) return 1;
  }
  std::vector<Spec> gap(72, Spec{0, 5, 9});  // longer than a wave is wide
  gap.front() = {4113, 3, 11};
  gap.back() = {47, 11, 3};
  if (check_batch(gap, {4})) return 1;
  if (check_batch({{0, 1, 2}, {0, 0, 0}, {0, 15, 15}}, {1, 4})) return 1;
  std::printf("OK\n");
  return 0;
}
"""


def _build_and_run_walk(tmp_path, extra):
    src = tmp_path / "bytes_walk_check.cpp"
    exe = tmp_path / "bytes_walk_check"
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
def test_walk_copies_every_byte_once_and_digests_match(tmp_path):
    """Every (src skew, dst skew) in 16 x 16 with the lengths 0, 1, 2, 3,
    7, 8, 15, 16, 17, 31, 33, 255, 4079, 4081, 4095, 4096, 4097, 4111,
    4113, 8193; every run length and every derived wave count; the chunk
    count equals rocp2p_vl_chunks for aligned multiples of 16."""
    _build_and_run_walk(tmp_path, [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_walk_under_sanitizers(tmp_path):
    """The same stand-alone program with ASan and UBSan: no byte outside
    a message is read or written, every access is naturally aligned."""
    _build_and_run_walk(tmp_path, ["-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"])


# -- fake transport ----------------------------------------------------------
MSG, REGION = 8192, 128 << 10
KNOWN = 0xC3
SKEWS = [(0, 0), (5, 0), (0, 9), (5, 9)]  # (region_skew, staging_skew)


def _open(direction, skews=(0, 0), **kw):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction, var_len=True, byte_granular=True,
                       region_skew=skews[0], staging_skew=skews[1], **kw)
    rng = np.random.default_rng(21)
    tp.staging[:] = rng.integers(0, 256, tp.staging.shape, dtype=np.uint8)
    tp.region[:] = rng.integers(0, 256, REGION, dtype=np.uint8)
    return tp


def _lens(tp, seed=9):
    n, cap = tp.msgs_per_region, tp.max_nbytes
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 3, 17, 4095, 4097, cap - 1, cap],
                      n).astype(np.int64)
    lens[:4] = [0, 1, cap, 4097]
    return lens


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


@pytest.mark.parametrize("skews", SKEWS)
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_byte_granular_moves_only_nbytes(direction, skews):
    tp = _open(direction, skews)
    assert tp.byte_granular and tp.supports_byte_granular
    assert tp.max_nbytes == MSG - max(skews)
    rs, ss = skews
    n = tp.msgs_per_region
    lens = _lens(tp)
    recv = tp.region if direction == "write" else tp.staging
    recv[...] = KNOWN
    staging0, region0 = tp.staging.copy(), tp.region.copy()
    assert tp.inflight < n  # slots are reused: check as we go
    for i in range(n):
        tp.post(i, int(lens[i]))
        tp.flush()
        ln, slot = int(lens[i]), tp.staging[i % tp.inflight]
        msg = tp.region[i * MSG:(i + 1) * MSG]
        assert (msg[rs:rs + ln] == slot[ss:ss + ln]).all()
        if direction == "write":  # slack untouched, in front and behind
            assert (msg[:rs] == KNOWN).all()
            assert (msg[rs + ln:] == KNOWN).all()
        else:
            assert (slot[:ss] == KNOWN).all()
            assert (slot[ss + ln:] == KNOWN).all()
            slot[:] = KNOWN  # for the message that reuses the slot
    if direction == "write":  # the sending side is only read
        assert (tp.staging == staging0).all()
    else:
        assert (tp.region == region0).all()
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_post_and_post_many_agree(direction):
    a, b = _open(direction, (5, 9)), _open(direction, (5, 9))
    n = a.msgs_per_region
    lens = _lens(a, seed=4)
    for i in range(n):
        a.post(i, int(lens[i]))
    a.flush()
    b.post_many(0, n, lens)
    b.flush()
    assert (a.region == b.region).all() and (a.staging == b.staging).all()
    # a scalar for all, and None = the most that fits behind the skews
    a.post_many(0, n, 37)
    for i in range(n):
        b.post(i, 37)
    a.post_many(0, 3)
    for i in range(3):
        b.post(i, MSG - 9)
    assert (a.region == b.region).all() and (a.staging == b.staging).all()
    a.close()
    b.close()


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("skews", SKEWS)
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_byte_granular_digest_check(direction, skews, icrc):
    tp = _open(direction, skews, icrc=icrc)
    lens = _lens(tp)
    assert tp.digest_check(_payload(1), lens) == 0
    assert tp.digest_check(_payload(2)) == 0  # None: the most that fits
    assert tp.digest_check(_payload(3), np.zeros_like(lens)) == 0

    real_post = tp.post
    victim = 3  # lens[3] == 4097
    skew = skews[0] if direction == "write" else skews[1]
    recv = ((lambda: tp.region[victim * MSG:(victim + 1) * MSG])
            if direction == "write"
            else (lambda: tp.staging[victim % tp.inflight]))

    def poke(at, mask):
        def post(i, nbytes=None):
            real_post(i, nbytes)
            if i == victim:
                recv()[at] ^= mask
        return post

    # the last payload byte of one message flipped on its way
    if not (icrc and direction == "write"):
        # (write with icrc compares the inline digest, taken as loaded:
        # a byte changed after landing is crc32_messages_bytes' to find)
        tp.post = poke(skew + 4096, 1)
        assert tp.digest_check(_payload(4), lens) == 1
    # the slack byte right behind the message, and the one right in front
    tp.post = poke(skew + 4097, 0xFF)
    assert tp.digest_check(_payload(5), lens) == 1
    if skew:
        tp.post = poke(skew - 1, 0xFF)
        assert tp.digest_check(_payload(6), lens) == 1
    tp.post = real_post
    assert tp.digest_check(_payload(7), lens) == 0
    tp.close()


def test_fake_byte_granular_icrc_write_sees_link_corruption():
    tp = _open("write", (5, 9), icrc=True)
    lens = _lens(tp)
    real_post = tp.post

    def post(i, nbytes=None):
        if i == 3:  # after the sender digested the slot, before the move
            tp.staging[3 % tp.inflight][9 + 4096] ^= 1
        real_post(i, nbytes)

    tp.post = post
    assert tp.digest_check(_payload(8), lens) == 1
    tp.close()


def test_byte_granular_validation():
    kw = dict(msg_bytes=MSG, region_bytes=REGION)
    with pytest.raises(ValueError, match="var_len"):
        get_transport("fake", byte_granular=True, **kw)
    for name in ("region_skew", "staging_skew"):
        with pytest.raises(ValueError, match="byte_granular"):
            get_transport("fake", var_len=True, **{name: 3}, **kw)
        for bad in (-1, 16, 2.5):
            with pytest.raises(ValueError, match=name):
                get_transport("fake", var_len=True, byte_granular=True,
                              **{name: bad}, **kw)
    tp = _open("write", (5, 9))
    for bad in (-1, MSG - 8, MSG, 2.5):  # nbytes + skew > msg_bytes
        with pytest.raises(ValueError):
            tp.post(0, bad)
        with pytest.raises(ValueError):
            tp.post_many(0, 2, np.array([1, bad]))
    with pytest.raises(ValueError):
        tp.digest_check(_payload(1), np.full(tp.msgs_per_region, MSG - 8))
    tp.post(0, MSG - 9)
    with pytest.raises(NotImplementedError, match="length"):
        tp.stamp()
    with pytest.raises(NotImplementedError, match="skew"):
        tp.integrity_check(seed=1)
    tp.close()
    tp = _open("write")  # no skew: whole slots fit
    tp.post(0, MSG)
    assert tp.integrity_check(seed=77) == 0
    tp.close()


def test_multiples_of_16_still_required_without_byte_granular():
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       var_len=True)
    assert tp.byte_granular is False and tp.max_nbytes == MSG
    with pytest.raises(ValueError, match="16"):
        tp.post(0, 17)
    tp.close()


@pytest.mark.parametrize("name", ["shm", "verbs"])
def test_byte_granular_not_implemented_elsewhere(name):
    with pytest.raises(NotImplementedError, match="byte_granular"):
        get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                      host="127.0.0.1", port=1, var_len=True,
                      byte_granular=True)


def test_soak_mixed_bytes_on_fake():
    import random

    from rocnrdma_amd.harness.soak import mixed_lens, run_soak

    lens = mixed_lens(random.Random(1), 4000, 65529, 1)
    assert lens.dtype == np.int64 and (lens % 16 != 0).any()
    assert lens.min() == 0 and lens.max() == 65529
    for v in (0, 1, 65529, 4095, 4096, 4097):
        assert (lens == v).sum() > 0
    # the default unit is what it was
    assert (mixed_lens(random.Random(1), 400, 65536)
            == mixed_lens(random.Random(1), 400, 65536, 16)).all()
    with pytest.raises(ValueError, match="mixed"):
        run_soak("fake", secs=0.1, byte_granular=True)
    for icrc in (False, True):
        stats = run_soak("fake", secs=0.3, region_bytes=1 << 20, seed=5,
                         mixed=True, byte_granular=True, icrc=icrc)
        assert stats["cycles"] > 0 and stats["failures"] == 0
        assert 0 < stats["bytes"]
