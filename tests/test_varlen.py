"""CPU tier for variable-length messages: the kernels' walk over a batch
emulated on the host from the shared headers, the zlib yardstick for
scattered unequal messages, and var_len=True on the fake transport."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport
from rocnrdma_amd.utils import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Host emulation of k_msg_engine_v / k_crc32_msgs_v: the scan, the run of
# every wave (rocp2p_vl_run), one seek per wave, the forward walk, the
# running CRC with its end-of-run shift, and the workgroup merge of the
# pending shares.  Every message lives in its own exactly-sized
# allocation, so ASan sees any byte read past a message's end.
_WALK_PROG = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "p2p_crc.h"
#include "p2p_varlen.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", \
    __LINE__, #c); return 1; } } while (0)

static constexpr rocp2p_crc_tables T = rocp2p_crc_make_tables();

// the yardstick: one byte at a time, no table of the headers involved
static uint32_t crc_bytewise(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & 0xEDB88320u);
  }
  return c ^ 0xFFFFFFFFu;
}

// crc of one chunk (full or partial) from the slice table
static uint32_t crc_chunk(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) c = T.slice[0][(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

struct Batch {
  std::vector<uint64_t> lens, cstart;           // cstart: n + 1, the scan
  std::vector<std::unique_ptr<unsigned char[]>> data;  // exactly lens[m]
  std::vector<uint32_t> want;                   // bytewise digests
  std::vector<uint64_t> owner;                  // chunk -> message, naive
  uint64_t total = 0;
};

static Batch make_batch(const std::vector<uint64_t>& lens) {
  Batch b;
  b.lens = lens;
  for (uint64_t len : lens) {
    b.cstart.push_back(b.total);
    uint64_t k = rocp2p_vl_chunks(len);
    for (uint64_t i = 0; i < k; i++) b.owner.push_back(b.data.size());
    b.total += k;
    std::unique_ptr<unsigned char[]> p(len ? new unsigned char[len] : nullptr);
    for (uint64_t i = 0; i < len; i++) p[i] = (unsigned char)rnd();
    b.want.push_back(crc_bytewise(p.get(), len));
    b.data.push_back(std::move(p));
  }
  b.cstart.push_back(b.total);
  return b;
}

struct Pending { uint32_t f = 0, m = 0; };

// One wave's run [c0, c1), the way the kernels walk it.
static int wave_walk(const Batch& b, uint64_t c0, uint64_t c1,
                     std::vector<uint32_t>& out, std::vector<int>& visits,
                     Pending& pend) {
  const uint64_t n = b.lens.size();
  rocp2p_vl_cursor cur = {0, 0, 0, 0};
  if (c0 < c1) rocp2p_vl_seek(&cur, b.cstart.data(), b.lens.data(), n, c0);
  uint32_t acc = 0;
  for (uint64_t c = c0; c < c1; c++) {
    CHECK(cur.m < n && cur.m == b.owner[c]);           // the right message
    CHECK(cur.len == b.lens[cur.m] && cur.len > 0);    // never a zero-length
    CHECK(b.cstart[cur.m] + cur.ci == c);
    CHECK(cur.cpm == rocp2p_vl_chunks(cur.len) && cur.ci < cur.cpm);
    visits[c]++;
    const uint64_t pos = cur.ci * 4096, left = cur.len - pos;
    const unsigned char* p = b.data[cur.m].get() + pos;
    uint64_t done;
    if (left >= 4096) {
      acc = rocp2p_crc_apply(T.shift[5], rocp2p_crc_apply(T.shift[5], acc)) ^
            crc_chunk(p, 4096);
      done = pos + 4096;
    } else {
      out[cur.m] ^= crc_chunk(p, left);  // never reads p[left]
      done = pos;
    }
    const bool msg_end = cur.ci + 1 == cur.cpm;
    if (msg_end || c + 1 == c1) {
      if (acc) {
        const uint64_t r = cur.len - done;
        uint32_t f = acc;
        if (r) f = rocp2p_crc_mulmod(rocp2p_crc_xpow8(r, T.xpow8), acc);
        if (msg_end) {
          out[cur.m] ^= f;
        } else {
          pend.f = f;
          pend.m = (uint32_t)cur.m;
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
static int launch(const Batch& b,
                  const std::vector<std::pair<uint64_t, uint64_t>>& runs,
                  size_t wpg) {
  std::vector<uint32_t> out(b.lens.size(), 0);
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
  for (size_t m = 0; m < b.lens.size(); m++) {
    CHECK(out[m] == b.want[m]);
    if (!b.lens[m]) CHECK(out[m] == 0);
  }
  return 0;
}

static int check_batch(const std::vector<uint64_t>& lens) {
  const Batch b = make_batch(lens);
  // the search on its own, every chunk
  for (uint64_t c = 0; c < b.total; c++)
    CHECK(rocp2p_vl_find(b.cstart.data(), lens.size(), c) == b.owner[c]);
  for (size_t wpg : {1, 4, 16}) {
    // every run length from 1 to total + 1, with an idle wave behind
    for (uint64_t run = 1; run <= b.total + 1; run++) {
      std::vector<std::pair<uint64_t, uint64_t>> runs;
      for (uint64_t c0 = 0; c0 < b.total; c0 += run)
        runs.push_back({c0, c0 + run < b.total ? c0 + run : b.total});
      runs.push_back({b.total, b.total});
      if (launch(b, runs, wpg)) return 1;
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
      if (launch(b, runs, wpg)) return 1;
    }
  }
  return 0;
}

int main() {
  CHECK(rocp2p_vl_chunks(0) == 0 && rocp2p_vl_chunks(1) == 1 &&
        rocp2p_vl_chunks(4096) == 1 && rocp2p_vl_chunks(4097) == 2 &&
        rocp2p_vl_chunks(~0ull) == (1ull << 52));
  const uint64_t pick[] = {0, 0, 1, 15, 16, 48, 4080, 4095, 4096, 4097,
                           4112, 8192, 3 * 4096 + 2048, 20000};
  const std::vector<std::vector<uint64_t>> fixed = {
      {16}, {0}, {4096}, {4097}, {3 * 4096},       // n = 1
      {0, 0, 0, 0, 0},                             // nothing at all
      {0, 0, 8192, 16, 0, 0, 0, 4097, 64, 0, 0},   // zeros front/middle/end
      {0, 5000}, {5000, 0}, {16, 0, 16},
      {3 * 4096 + 2048, 16, 0, 3 * 4096 + 2048, 4096, 3 * 4096 + 2048},
  };
  for (const auto& lens : fixed)
    if (check_batch(lens)) return 1;
  for (int rep = 0; rep < 12; rep++) {
    std::vector<uint64_t> lens(1 + rnd() % 12);
    for (auto& l : lens) l = pick[rnd() % (sizeof(pick) / sizeof(pick[0]))];
    if (check_batch(lens)) return 1;
  }
  // a run of zero-length messages longer than a wave is wide
  std::vector<uint64_t> gap(72, 0);
  gap.front() = 4112;
  gap.back() = 48;
  if (check_batch(gap)) return 1;
  std::printf("OK\n");
  return 0;
}
"""


def _build_and_run_walk(tmp_path, extra):
    src = tmp_path / "varlen_walk_check.cpp"
    exe = tmp_path / "varlen_walk_check"
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
def test_walk_visits_every_chunk_once_and_digests_match(tmp_path):
    _build_and_run_walk(tmp_path, [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_walk_under_sanitizers(tmp_path):
    """The same stand-alone program with ASan and UBSan: no byte at or
    past a message's end is read, no descriptor past the scan's end."""
    _build_and_run_walk(tmp_path, ["-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"])


def test_crc32_messages_v_reference():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 40000, dtype=np.uint8)
    offs = [16, 0, 20000, 39999, 40000, 4096, 100]
    lens = [4097, 0, 20000, 1, 0, 4096, 15]
    got = pattern.crc32_messages_v_reference(data, offs, lens)
    assert got.dtype == np.uint32 and got.shape == (len(offs),)
    raw = data.tobytes()
    for o, ln, g in zip(offs, lens, got):
        assert int(g) == zlib.crc32(raw[o:o + ln])
    assert got[1] == 0 and got[4] == 0  # crc32(b"") is 0
    # uniform lengths: the fixed-length yardstick
    assert (pattern.crc32_messages_v_reference(
        data[:32768], range(0, 32768, 4096), [4096] * 8)
        == pattern.crc32_messages_reference(data[:32768], 4096)).all()
    with pytest.raises(AssertionError):
        pattern.crc32_messages_v_reference(data, [39999], [2])


# -- fake transport ----------------------------------------------------------
MSG, REGION = 8192, 128 << 10
KNOWN = 0xC3


def _open(direction, **kw):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction, var_len=True, **kw)
    rng = np.random.default_rng(21)
    tp.staging[:] = rng.integers(0, 256, tp.staging.shape, dtype=np.uint8)
    tp.region[:] = rng.integers(0, 256, REGION, dtype=np.uint8)
    return tp


def _lens(n, seed=9):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 16, 48, 4080, 4096, 4112, MSG], n).astype(np.int64)
    lens[:4] = [0, 16, MSG, 4112]
    return lens


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_var_len_moves_only_nbytes(direction):
    tp = _open(direction)
    assert tp.var_len and tp.supports_var_len
    n = tp.msgs_per_region
    lens = _lens(n)
    recv = tp.region if direction == "write" else tp.staging
    recv[...] = KNOWN
    staging0, region0 = tp.staging.copy(), tp.region.copy()
    assert tp.inflight < n  # slots are reused: check as we go
    for i in range(n):
        tp.post(i, int(lens[i]))
        tp.flush()
        ln, slot = int(lens[i]), tp.staging[i % tp.inflight]
        msg = tp.region[i * MSG:(i + 1) * MSG]
        if direction == "write":
            assert (msg[:ln] == slot[:ln]).all()
            assert (msg[ln:] == KNOWN).all()  # slack untouched
        else:
            assert (slot[:ln] == msg[:ln]).all()
            assert (slot[ln:] == KNOWN).all()
            slot[:] = KNOWN  # for the message that reuses the slot
    # the sending side is only read
    if direction == "write":
        assert (tp.staging == staging0).all()
    else:
        assert (tp.region == region0).all()
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_post_and_post_many_agree(direction):
    a, b = _open(direction), _open(direction)
    n = a.msgs_per_region
    lens = _lens(n, seed=4)
    for i in range(n):
        a.post(i, int(lens[i]))
    a.flush()
    b.post_many(0, n, lens)
    b.flush()
    assert (a.region == b.region).all() and (a.staging == b.staging).all()
    # a scalar for all, and None = full slots
    a.post_many(0, n, 48)
    for i in range(n):
        b.post(i, 48)
    a.post_many(0, 3)
    for i in range(3):
        b.post(i, MSG)
    assert (a.region == b.region).all() and (a.staging == b.staging).all()
    a.close()
    b.close()


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_var_len_digest_check(direction, icrc):
    tp = _open(direction, icrc=icrc)
    lens = _lens(tp.msgs_per_region)
    assert tp.digest_check(_payload(1), lens) == 0
    assert tp.digest_check(_payload(2)) == 0  # None: full slots
    assert tp.digest_check(_payload(3), np.zeros_like(lens)) == 0

    # one byte of one message flipped on its way
    real_post = tp.post
    victim = 3  # lens[3] == 4112
    recv = ((lambda: tp.region[victim * MSG:(victim + 1) * MSG])
            if direction == "write"
            else (lambda: tp.staging[victim % tp.inflight]))

    def flip_payload(i, nbytes=None):
        real_post(i, nbytes)
        if i == victim:
            recv()[5] ^= 1

    tp.post = flip_payload
    if not (icrc and direction == "write"):
        # (write with icrc compares the inline digest, taken as loaded:
        # a byte changed after landing is crc32_messages_v's to find)
        assert tp.digest_check(_payload(4), lens) == 1

    # one slack byte of the receiver overwritten
    def hit_slack(i, nbytes=None):
        real_post(i, nbytes)
        if i == victim:
            recv()[int(lens[victim]) + 7] ^= 0xFF

    tp.post = hit_slack
    assert tp.digest_check(_payload(5), lens) == 1
    tp.post = real_post
    assert tp.digest_check(_payload(6), lens) == 0
    tp.close()


def test_fake_var_len_icrc_write_sees_link_corruption():
    tp = _open("write", icrc=True)
    lens = _lens(tp.msgs_per_region)
    real_post = tp.post

    def post(i, nbytes=None):
        if i == 3:  # after the sender digested the slot, before the move
            tp.staging[3 % tp.inflight][5] ^= 1
        real_post(i, nbytes)

    tp.post = post
    assert tp.digest_check(_payload(7), lens) == 1
    tp.close()


def test_var_len_validation():
    tp = _open("write")
    for bad in (-16, 8, MSG + 16, 17):
        with pytest.raises(ValueError):
            tp.post(0, bad)
        with pytest.raises(ValueError):
            tp.post_many(0, 2, bad)
        with pytest.raises(ValueError):
            tp.post_many(0, 2, np.array([16, bad]))
    with pytest.raises(ValueError):
        tp.post_many(0, 3, np.array([16, 16]))  # not n entries
    with pytest.raises(ValueError):
        tp.post_many(0, 2, np.array([16.0, 32.0]))
    with pytest.raises(ValueError):
        tp.digest_check(_payload(1), np.array([16]))
    with pytest.raises(NotImplementedError, match="length"):
        tp.stamp()
    tp.close()
    tp = _open("write", icrc=True)
    with pytest.raises(NotImplementedError, match="length"):
        tp.stamp()
    tp.close()


def test_nbytes_needs_var_len():
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION)
    assert tp.var_len is False
    with pytest.raises(ValueError, match="var_len"):
        tp.post(0, 16)
    with pytest.raises(ValueError, match="var_len"):
        tp.post_many(0, 2, 16)
    with pytest.raises(ValueError, match="var_len"):
        tp.digest_check(_payload(1), np.full(tp.msgs_per_region, 16))
    tp.post(0)
    tp.post_many(0, 2)
    assert tp.digest_check(_payload(1)) == 0
    tp.close()


@pytest.mark.parametrize("name", ["shm", "verbs"])
def test_var_len_not_implemented_elsewhere(name):
    with pytest.raises(NotImplementedError, match="var_len"):
        get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                      host="127.0.0.1", port=1, var_len=True)


def test_integrity_check_through_var_len():
    for direction in ("write", "read"):
        tp = _open(direction)
        assert tp.var_len  # full slots through the variable-length path
        assert tp.integrity_check(seed=77) == 0
        tp.close()


def test_soak_mixed_on_fake():
    from rocnrdma_amd.harness.soak import SIZES, mixed_lens, run_soak

    import random

    lens = mixed_lens(random.Random(1), 4000, 65536)
    assert lens.dtype == np.int64 and (lens % 16 == 0).all()
    assert lens.min() == 0 and lens.max() == 65536
    for v in (0, 16, 65536, 4096 - 16, 4096, 4096 + 16):
        assert (lens == v).sum() > 0
    assert (mixed_lens(random.Random(1), 4000, 65536) == lens).all()

    stats = run_soak("fake", secs=0.3, region_bytes=1 << 20, seed=5,
                     mixed=True)
    assert stats["cycles"] > 0 and stats["failures"] == 0
    # bytes actually moved: less than full slots would have been
    assert 0 < stats["bytes"] < stats["msgs"] * max(SIZES)
    stats = run_soak("fake", secs=0.2, region_bytes=1 << 20, seed=6,
                     mixed=True, icrc=True)
    assert stats["cycles"] > 0 and stats["failures"] == 0
