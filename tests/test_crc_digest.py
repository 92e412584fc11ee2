"""CPU tier for the CRC32 digests: the GF(2) combine algebra (Python
references and the shared C++ header) against zlib, and the transports'
payload-agnostic digest_check."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport
from rocnrdma_amd.transport.base import Transport
from rocnrdma_amd.utils import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = [0, 1, 15, 16, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 48,
           12345, 70000]


@pytest.fixture(scope="module")
def blob():
    return np.random.default_rng(2024).integers(
        0, 256, 70000, dtype=np.uint8).tobytes()


def test_combine_matches_zlib_at_random_splits(blob):
    rng = np.random.default_rng(7)
    for _ in range(40):
        n = int(rng.integers(0, len(blob) + 1))
        k = int(rng.integers(0, n + 1))
        a, b = blob[:k], blob[k:n]
        assert pattern.crc32_combine(
            zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(blob[:n])


@pytest.mark.parametrize("chunk", [64, 1000, 4096])
@pytest.mark.parametrize("length", LENGTHS)
def test_flat_fold_of_chunk_crcs(blob, length, chunk):
    """XOR over chunks of shift(crc(chunk), bytes after the chunk) — the
    identity the digest kernel accumulates with atomicXor."""
    data = blob[:length]
    acc = 0
    for s in range(0, length, chunk):
        e = min(s + chunk, length)
        acc ^= pattern.crc32_shift(zlib.crc32(data[s:e]), length - e)
    assert acc == zlib.crc32(data)


def test_shift_zero_is_identity():
    for c in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert pattern.crc32_shift(c, 0) == c
        assert pattern.crc32_combine(c, 0, 0) == c


def test_shift_is_additive_for_64bit_lengths():
    a = 2 ** 33 + 5
    b = 2 ** 32 + 7 * 4096 + 16
    for c in (1, 0x80000000, 0xCBF43926):
        assert pattern.crc32_shift(c, a + b) == pattern.crc32_shift(
            pattern.crc32_shift(c, a), b)


@pytest.mark.parametrize("msg", [16, 1000, 4096 + 16])
def test_messages_reference_matches_slices(blob, msg):
    n = 11
    data = np.frombuffer(blob[:16 * 7 + n * msg], dtype=np.uint8)
    got = pattern.crc32_messages_reference(data[:n * msg], msg)
    assert got.dtype == np.uint32 and got.shape == (n,)
    for m in range(n):
        assert got[m] == zlib.crc32(blob[m * msg:(m + 1) * msg])
    perm = np.random.default_rng(3).permutation(n)
    offs = 16 * 7 + perm * msg
    got = pattern.crc32_messages_reference(data, msg, offs)
    for m in range(n):
        o = int(offs[m])
        assert got[m] == zlib.crc32(blob[o:o + msg])


def test_message_digests_fold_to_region_crc(blob):
    msg, n = 4096 + 16, 13
    data = blob[:n * msg]
    acc = 0
    for d in pattern.crc32_messages_reference(
            np.frombuffer(data, dtype=np.uint8), msg):
        acc = pattern.crc32_combine(acc, int(d), msg)
    assert acc == zlib.crc32(data)


# -- transports ------------------------------------------------------------
MSG, REGION = 4096, 64 << 10


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_digest_check_clean(direction):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction)
    assert tp.digest_check(_payload(1)) == 0
    assert tp.digest_check(_payload(2)) == 0
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_digest_check_counts_one_corrupt_message(direction):
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION,
                       direction=direction)
    real_post = tp.post

    def post(i):
        real_post(i)
        if i == 3:  # one byte of one message goes bad after delivery
            if direction == "write":
                tp.region[3 * MSG + 5] ^= 1
            else:
                tp.staging[3 % tp.inflight][5] ^= 1

    tp.post = post
    assert tp.digest_check(_payload(3)) == 1
    tp.close()


def test_fake_digest_check_rejects_wrong_payload():
    tp = get_transport("fake", msg_bytes=MSG, region_bytes=REGION)
    with pytest.raises(ValueError):
        tp.digest_check(np.zeros(REGION - 1, dtype=np.uint8))
    with pytest.raises(ValueError):
        tp.digest_check(np.zeros(REGION // 4, dtype=np.uint32))


def test_digest_check_default_raises():
    class Bare(Transport):
        name = "bare"

        def post(self, i):
            pass

        def flush(self):
            pass

        def integrity_check(self, seed):
            return 0

    tp = Bare(MSG, REGION)
    with pytest.raises(NotImplementedError, match="bare"):
        tp.digest_check(_payload(4))


def test_soak_crc_audit_on_fake():
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("fake", secs=0.2, region_bytes=1 << 20, seed=5,
                     audit="crc")
    assert stats["cycles"] > 0 and stats["failures"] == 0
    with pytest.raises(ValueError):
        run_soak("fake", secs=0.0, audit="md5")


# -- the shared header, as plain C++ against zlib's own combine ------------
_HEADER_PROG = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "p2p_crc.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 11;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", \
    __LINE__, #c); return 1; } } while (0)

// The kernels hold this as constant-initialised device data, so it has
// to stay a constant expression: one entry of each table known from
// zlib (crc_table[0][1], x^8, x2n_table[9] = x^512).
static constexpr rocp2p_crc_tables T = rocp2p_crc_make_tables();
static_assert(T.slice[0][1] == 0x77073096u, "slice-by-8 table");
static_assert(T.xpow8[0][1] == 0x00800000u, "byte-sliced power table");
static_assert(T.shift[0][3][0x80] == 0x88d14467u, "shift operators");

// "combine" mode: zlib's own crc32_combine64 at fixed inputs, one line
// "c1 c2 len2 result" each, for the Python combine to be compared with.
static int print_combines() {
  const uint64_t lens[] = {(1ull << 24) + 5, (1ull << 32) + 28688,
                           (1ull << 33) + 5};
  const uint32_t cs[][2] = {{0x00000001u, 0u},          {0x80000000u, 0u},
                            {0xCBF43926u, 0u},          {0xCBF43926u, 0xDEADBEEFu},
                            {0xFFFFFFFFu, 0x12345678u}, {0x0BADF00Du, 0xFFFFFFFFu}};
  for (uint64_t n : lens)
    for (const auto& c : cs)
      std::printf("%u %u %llu %u\n", c[0], c[1], (unsigned long long)n,
                  (uint32_t)crc32_combine64(c[0], c[1], (z_off64_t)n));
  return 0;
}

int main(int argc, char**) {
  if (argc > 1) return print_combines();
  uint32_t tab[ROCP2P_CRC_XPOW_N];
  rocp2p_crc_xpow_table(tab);
  CHECK(tab[0] == 0x00800000u);
  static uint32_t t8[8][256];
  rocp2p_crc_xpow8_table(t8, tab);
  std::vector<unsigned char> buf(70000);
  for (auto& b : buf) b = (unsigned char)rnd();

  // mulmod: 1 is neutral, commutative, distributes over XOR
  for (int i = 0; i < 200; i++) {
    uint32_t a = (uint32_t)rnd(), b = (uint32_t)rnd(), c = (uint32_t)rnd();
    CHECK(rocp2p_crc_mulmod(ROCP2P_CRC_ONE, a) == a);
    CHECK(rocp2p_crc_mulmod(a, b) == rocp2p_crc_mulmod(b, a));
    CHECK(rocp2p_crc_mulmod(a, b ^ c) ==
          (rocp2p_crc_mulmod(a, b) ^ rocp2p_crc_mulmod(a, c)));
  }
  // shift == zlib's combine with an empty-CRC right side, any length
  const uint64_t lens[] = {0, 1, 15, 16, 63, 64, 65, 4095, 4096, 4097,
                           12336, 12345, 70000, (1ull << 32) + 28688,
                           (1ull << 33) + 5, (1ull << 40) + 123};
  for (uint64_t n : lens)
    for (int i = 0; i < 8; i++) {
      uint32_t c = (uint32_t)rnd();
      CHECK(rocp2p_crc_shift(c, n, tab) ==
            (uint32_t)crc32_combine64(c, 0, (z_off64_t)n));
      CHECK(rocp2p_crc_mulmod(rocp2p_crc_xpow(n, tab), c) ==
            rocp2p_crc_shift(c, n, tab));
      CHECK(rocp2p_crc_xpow8(n, t8) == rocp2p_crc_xpow(n, tab));
      uint64_t wide = rnd() * 0x9E3779B97F4A7C15ull;  // all 8 bytes live
      CHECK(rocp2p_crc_xpow8(wide, t8) == rocp2p_crc_xpow(wide, tab));
    }
  // combine against crc32() of the concatenation and zlib's combine
  for (int i = 0; i < 300; i++) {
    size_t n = rnd() % (buf.size() + 1), k = n ? rnd() % (n + 1) : 0;
    uint32_t ca = (uint32_t)crc32(0, buf.data(), (uInt)k);
    uint32_t cb = (uint32_t)crc32(0, buf.data() + k, (uInt)(n - k));
    uint32_t whole = (uint32_t)crc32(0, buf.data(), (uInt)n);
    CHECK(rocp2p_crc_combine(ca, cb, n - k, tab) == whole);
    CHECK(rocp2p_crc_combine(ca, cb, n - k, tab) ==
          (uint32_t)crc32_combine(ca, cb, (z_off_t)(n - k)));
    CHECK(rocp2p_crc_combine(ca, 0, 0, tab) == ca);
  }
  // the kernels' tables: the run-time builders agree with the constant
  CHECK(std::memcmp(t8, T.xpow8, sizeof(t8)) == 0);
  // slice-by-8 over a 64-byte block, the way a lane walks its segment
  for (int i = 0; i < 200; i++) {
    const unsigned char* p = buf.data() + rnd() % (buf.size() - 64);
    uint32_t w[16];
    std::memcpy(w, p, 64);
    uint32_t crc = 0xFFFFFFFFu;
    for (int j = 0; j < 8; j++)
      crc = rocp2p_crc_step8(T.slice, crc, w[2 * j], w[2 * j + 1]);
    CHECK((crc ^ 0xFFFFFFFFu) == (uint32_t)crc32(0, p, 64));
  }
  // shift[k] appends 64 << k bytes: one level of the kernels' log tree
  for (int k = 0; k < 6; k++)
    for (int i = 0; i < 50; i++) {
      size_t nb = (size_t)64 << k, na = rnd() % 5000;
      const unsigned char* a = buf.data() + rnd() % (buf.size() - na - nb);
      uint32_t ca = (uint32_t)crc32(0, a, (uInt)na);
      uint32_t cb = (uint32_t)crc32(0, a + na, (uInt)nb);
      CHECK((rocp2p_crc_apply(T.shift[k], ca) ^ cb) ==
            (uint32_t)crc32(0, a, (uInt)(na + nb)));
    }
  std::printf("OK\n");
  return 0;
}
"""


def _build_header_prog(tmp_path):
    src = tmp_path / "crc_header_check.cpp"
    exe = tmp_path / "crc_header_check"
    src.write_text(_HEADER_PROG)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-D_LARGEFILE64_SOURCE", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "rocnrdma_amd", "ops", "csrc"),
         str(src), "-lz", "-o", str(exe)],
        check=True, capture_output=True, text=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_crc_header_against_zlib(tmp_path):
    exe = _build_header_prog(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK"


# -- lengths past 4 GiB, and the periodic reference of the wide GPU tier ---
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_python_combine_matches_zlib_combine64_past_4gib(tmp_path):
    """pattern.crc32_combine / crc32_shift at second-part lengths that do
    not fit in memory, against zlib's crc32_combine64 (printed by the C
    program above for fixed inputs)."""
    exe = _build_header_prog(tmp_path)
    r = subprocess.run([str(exe), "combine"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(rows) == 18
    assert {n for _, _, n, _ in rows} == {2 ** 24 + 5, 2 ** 32 + 28688,
                                          2 ** 33 + 5}
    for c1, c2, n, want in rows:
        assert pattern.crc32_combine(c1, c2, n) == want
        if c2 == 0:
            assert pattern.crc32_shift(c1, n) == want


def test_repeat_matches_zlib(blob):
    for n in (0, 1, 17, 1000):
        for times in (0, 1, 2, 3, 7, 16, 33):
            x = blob[100:100 + n]
            assert pattern.crc32_repeat(zlib.crc32(x), n, times) == zlib.crc32(
                x * times)


@pytest.mark.parametrize("period", [1, 48, 1009])
def test_periodic_reference_matches_materialised_bytes(blob, period):
    """crc32_periodic_reference against plain zlib on the bytes themselves:
    ranges inside one period, across one boundary, and over one and
    several whole periods, from every kind of phase."""
    block = np.frombuffer(blob[:period], dtype=np.uint8)
    stream = blob[:period] * 16
    pairs = [(s, n) for s in (0, 1, period - 1, period, period + 5,
                              3 * period + period // 2)
             for n in (0, 1, period - 1, period, period + 1, 2 * period,
                       5 * period + 3, 7 * period)]
    assert len(pairs) == 48
    for s, n in pairs:
        assert s + n <= len(stream)
        assert pattern.crc32_periodic_reference(block, s, n) == zlib.crc32(
            stream[s:s + n]), (s, n)
    with pytest.raises(ValueError):
        pattern.crc32_periodic_reference(block[:0], 0, 1)
    with pytest.raises(ValueError):
        pattern.crc32_periodic_reference(block, -1, 1)
