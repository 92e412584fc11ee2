"""CPU tier for the inline ICRC: the fused engine's chunk algebra
emulated on the host from the shared header, the guarantee that the
tables the older kernels stage did not move, and the transports'
stamp / icrc_stats logic on the fake transport."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Host emulation of k_msg_engine_crc: 64 lanes, lane l of a full 4 KiB
# chunk holds the 16-byte pieces l, l+64, l+128, l+192.
_ENGINE_PROG = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "p2p_crc.h"

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", \
    __LINE__, #c); return 1; } } while (0)

static constexpr rocp2p_crc_tables T = rocp2p_crc_make_tables();

// the yardstick: one byte at a time, no table of the header involved
static uint32_t crc_bytewise(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & 0xEDB88320u);
  }
  return c ^ 0xFFFFFFFFu;
}

static uint32_t piece16(const unsigned char* p) {
  uint32_t w[4];
  std::memcpy(w, p, 16);
  uint32_t c = rocp2p_crc_step8(T.slice, 0xFFFFFFFFu, w[0], w[1]);
  return rocp2p_crc_step8(T.slice, c, w[2], w[3]) ^ 0xFFFFFFFFu;
}

// operator "16 B << k follow": the two new levels, then shift[0..3]
static const rocp2p_crc_tab256* lane_op(int k) {
  return k < 2 ? T.shift16[k] : T.shift[k - 2];
}

// full chunk: per-lane Horner with the 1 KiB operator, then the lane tree
static uint32_t chunk_full(const unsigned char* p) {
  uint32_t lane[64];
  for (int l = 0; l < 64; l++) {
    uint32_t c = piece16(p + 16 * l);
    for (int u = 1; u < 4; u++)
      c = rocp2p_crc_apply(T.shift[4], c) ^ piece16(p + 16 * (l + 64 * u));
    lane[l] = c;
  }
  for (int k = 0; k < 6; k++) {
    uint32_t next[64];
    for (int l = 0; l < 64; l++) {
      uint32_t partner = lane[l ^ (1 << k)];
      bool left = ((l >> k) & 1) == 0;
      uint32_t cl = left ? lane[l] : partner, cr = left ? partner : lane[l];
      next[l] = rocp2p_crc_apply(lane_op(k), cl) ^ cr;
    }
    std::memcpy(lane, next, sizeof(lane));
  }
  for (int l = 1; l < 64; l++)
    if (lane[l] != lane[0]) return ~lane[0];  // every lane must agree
  return lane[0];
}

// partial chunk: pieces past the end contribute 0 and are never read
static uint32_t chunk_partial(const unsigned char* p, uint32_t valid) {
  uint32_t nvec = valid / 16, x = 0;
  for (uint32_t l = 0; l < 64; l++)
    for (uint32_t u = 0; u < 4; u++) {
      uint32_t q = l + 64 * u;
      if (q < nvec)
        x ^= rocp2p_crc_mulmod(rocp2p_crc_xpow8(valid - 16 * (q + 1), T.xpow8),
                               piece16(p + 16 * q));
    }
  return x;
}

// a message the way one wave walks it: running CRC over the full
// chunks, the partial chunk flat, the variable shift at the end
static uint32_t message(const unsigned char* p, size_t n) {
  uint32_t acc = 0, out = 0;
  size_t pos = 0;
  for (; n - pos >= 4096; pos += 4096)
    acc = rocp2p_crc_apply(T.shift[5], rocp2p_crc_apply(T.shift[5], acc)) ^
          chunk_full(p + pos);
  if (pos < n) out ^= chunk_partial(p + pos, (uint32_t)(n - pos));
  return out ^
         rocp2p_crc_mulmod(rocp2p_crc_xpow8(n - pos, T.xpow8), acc);
}

int main() {
  // the tables the older kernels stage must not have moved or changed:
  // offsets, sizes and zlib CRC32 of each block as they were before
  // shift16 was added
  CHECK(offsetof(rocp2p_crc_tables, slice) == 0);
  CHECK(offsetof(rocp2p_crc_tables, shift) == 8192);
  CHECK(offsetof(rocp2p_crc_tables, xpow8) == 32768);
  CHECK(offsetof(rocp2p_crc_tables, shift16) == 40960);
  CHECK(sizeof(T.slice) == 8192 && sizeof(T.shift) == 24576 &&
        sizeof(T.xpow8) == 8192 && sizeof(T.shift16) == 8192);
  CHECK(sizeof(T) == 49152);
  CHECK(crc_bytewise((const unsigned char*)T.slice, sizeof(T.slice)) ==
        0x1a76768fu);
  CHECK(crc_bytewise((const unsigned char*)T.shift, sizeof(T.shift)) ==
        0xe416ad3cu);
  CHECK(crc_bytewise((const unsigned char*)T.xpow8, sizeof(T.xpow8)) ==
        0x080790cau);

  // exactly as many bytes as each case may touch: ASan sees any read
  // past a partial chunk's end
  const size_t sizes[] = {4096, 16, 48, 1024, 4080, 3 * 4096,
                          3 * 4096 + 2048};
  for (size_t n : sizes)
    for (int rep = 0; rep < 4; rep++) {
      std::vector<unsigned char> buf(n);
      for (auto& b : buf) b = (unsigned char)rnd();
      if (n == 4096) CHECK(chunk_full(buf.data()) == crc_bytewise(buf.data(), n));
      if (n < 4096)
        CHECK(chunk_partial(buf.data(), (uint32_t)n) ==
              crc_bytewise(buf.data(), n));
      CHECK(message(buf.data(), n) == crc_bytewise(buf.data(), n));
    }
  // the new operators on their own: append 16 and 32 bytes
  for (int k = 0; k < 2; k++)
    for (int i = 0; i < 50; i++) {
      size_t nb = (size_t)16 << k, na = rnd() % 300;
      std::vector<unsigned char> buf(na + nb);
      for (auto& b : buf) b = (unsigned char)rnd();
      CHECK((rocp2p_crc_apply(T.shift16[k], crc_bytewise(buf.data(), na)) ^
             crc_bytewise(buf.data() + na, nb)) ==
            crc_bytewise(buf.data(), na + nb));
    }
  std::printf("OK\n");
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_engine_algebra_and_unchanged_tables(tmp_path):
    src = tmp_path / "icrc_engine_check.cpp"
    exe = tmp_path / "icrc_engine_check"
    src.write_text(_ENGINE_PROG)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "rocnrdma_amd", "ops", "csrc"),
         str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK"


# -- transports ------------------------------------------------------------
MSG, REGION = 4096, 64 << 10
ROUNDS = 3


def _open(direction):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction, icrc=True)
    rng = np.random.default_rng(11)
    tp.staging[:] = rng.integers(0, 256, tp.staging.shape, dtype=np.uint8)
    tp.region[:] = rng.integers(0, 256, REGION, dtype=np.uint8)
    return tp


def _post_rounds(tp):
    posted = 0
    for _ in range(ROUNDS):
        tp.post_many(posted, tp.msgs_per_region)
        posted += tp.msgs_per_region
    tp.flush()
    return posted


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_icrc_clean_corrupt_restamp(direction):
    tp = _open(direction)
    # before the first stamp: moved, nothing to compare with
    tp.post_many(0, 5)
    tp.flush()
    assert tp.icrc_stats() == {"checked": 0, "bad": 0}

    tp.stamp()
    posted = _post_rounds(tp)
    assert tp.icrc_stats() == {"checked": posted, "bad": 0}

    # one byte of the sender goes bad after the stamp
    if direction == "write":
        tp.staging[3][5] ^= 1
        hits = sum(1 for i in range(posted) if i % tp.inflight == 3)
    else:
        tp.region[3 * MSG + 5] ^= 1
        hits = sum(1 for i in range(posted) if i % tp.msgs_per_region == 3)
    assert hits > 0
    _post_rounds(tp)
    assert tp.icrc_stats() == {"checked": 2 * posted, "bad": hits}

    # stamping again accepts the sender as it is now
    tp.stamp()
    _post_rounds(tp)
    assert tp.icrc_stats() == {"checked": 3 * posted, "bad": hits}
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_icrc_digest_check(direction):
    tp = _open(direction)
    tp.stamp()
    payload = np.random.default_rng(5).integers(0, 256, REGION,
                                                dtype=np.uint8)
    assert tp.digest_check(payload) == 0
    # digest_check rewrote the sender: its stale stamp must not count
    assert tp.icrc_stats() == {"checked": 0, "bad": 0}
    tp.close()


def test_fake_icrc_digest_check_counts_link_corruption():
    """A byte that changes between the sender's digest and the move is
    what the inline digest exists to catch."""
    tp = _open("write")
    real_post = tp.post

    def post(i):
        if i == 3:
            tp.staging[3 % tp.inflight][5] ^= 1
        real_post(i)

    tp.post = post
    payload = np.random.default_rng(6).integers(0, 256, REGION,
                                                dtype=np.uint8)
    assert tp.digest_check(payload) == 1
    tp.close()


def test_icrc_is_opt_in():
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION)
    assert tp.icrc is False
    with pytest.raises(NotImplementedError):
        tp.stamp()
    with pytest.raises(NotImplementedError):
        tp.icrc_stats()
    tp.close()


@pytest.mark.parametrize("name", ["shm", "verbs"])
def test_icrc_not_implemented_elsewhere(name):
    with pytest.raises(NotImplementedError, match="icrc"):
        get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                      host="127.0.0.1", port=1, icrc=True)


def test_sweep_and_soak_icrc_on_fake():
    from rocnrdma_amd.harness.soak import run_soak
    from rocnrdma_amd.harness.sweep import run_sweep

    rows = run_sweep("fake", region_bytes=1 << 20, sizes=[4096, 65536],
                     target_secs=0.05, icrc=True)
    assert len(rows) == 4
    for r in rows:
        assert r["icrc_checked"] >= r["msgs"] > 0 and r["icrc_bad"] == 0
    plain = run_sweep("fake", region_bytes=1 << 20, sizes=[4096],
                      directions=("write",), target_secs=0.05)
    assert "icrc_checked" not in plain[0]

    stats = run_soak("fake", secs=0.2, region_bytes=1 << 20, seed=5,
                     icrc=True)
    assert stats["cycles"] > 0 and stats["failures"] == 0
    assert stats["icrc_checked"] > 0 and stats["icrc_bad"] == 0
    assert "icrc_checked" not in run_soak("fake", secs=0.0)
