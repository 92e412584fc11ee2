"""CPU reference implementations of the GPU payload kernels.

Bit-identical to rocnrdma_amd/ops/csrc/p2p_kernels.hip — the GPU
numerics tests compare the HIP kernels against these.
"""
from __future__ import annotations

import zlib

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)

PAGE = 4096


def splitmix64_words(seed: int, start: int, count: int) -> np.ndarray:
    """Pattern words i in [start, start+count): mix(seed + (i+1)*GOLDEN)."""
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        x = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + i * _GOLDEN
        x = (x ^ (x >> np.uint64(30))) * _M1
        x = (x ^ (x >> np.uint64(27))) * _M2
        return x ^ (x >> np.uint64(31))


def fill_reference(nbytes: int, seed: int) -> np.ndarray:
    """The full pattern buffer as uint8 (nbytes % 8 == 0)."""
    assert nbytes % 8 == 0
    words = splitmix64_words(seed, 0, nbytes // 8)
    return words.view(np.uint8)


def crc32_pages_reference(data: bytes | np.ndarray) -> np.ndarray:
    """zlib.crc32 of each 4 KiB page, as uint32 array."""
    buf = np.asarray(data, dtype=np.uint8).tobytes()
    assert len(buf) % PAGE == 0
    return np.array(
        [zlib.crc32(buf[i : i + PAGE]) for i in range(0, len(buf), PAGE)],
        dtype=np.uint32,
    )


# -- CRC32 digest algebra (mirrors rocnrdma_amd/ops/csrc/p2p_crc.h) ----
# Polynomials are 32-bit, reflected (bit 31 = x^0), mod P = 0xEDB88320.
# zlib.crc32 exists in Python but zlib's crc32_combine is not exposed.
_CRC_POLY = 0xEDB88320
_CRC_ONE = 0x80000000


def _crc_mulmod(a: int, b: int) -> int:
    """a * b mod P."""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (_CRC_POLY if b & 1 else 0)
    return p


def _crc_xpow_table() -> list[int]:
    tab, p = [], _CRC_ONE >> 8  # x^8: one byte
    for _ in range(64):
        tab.append(p)
        p = _crc_mulmod(p, p)
    return tab


_CRC_XPOW = _crc_xpow_table()  # x^(8 * 2^k)


def crc32_shift(crc: int, nbytes: int) -> int:
    """crc * x^(8*nbytes): what crc(A) contributes to the CRC of a string
    in which nbytes more bytes follow A (nbytes < 2**64)."""
    if not 0 <= nbytes < 1 << 64:
        raise ValueError("nbytes out of range")
    p, k = _CRC_ONE, 0
    while nbytes:
        if nbytes & 1:
            p = _crc_mulmod(_CRC_XPOW[k], p)
        nbytes >>= 1
        k += 1
    return _crc_mulmod(p, crc & 0xFFFFFFFF)


def crc32_combine(c1: int, c2: int, len2: int) -> int:
    """crc(A || B) from c1 = crc(A), c2 = crc(B), len2 = len(B)."""
    return crc32_shift(c1, len2) ^ (c2 & 0xFFFFFFFF)


def crc32_repeat(crc: int, nbytes: int, times: int) -> int:
    """crc(X * times) from crc = crc(X) and nbytes = len(X), by
    square-and-multiply over crc32_combine (times >= 0)."""
    if times < 0 or nbytes < 0:
        raise ValueError("negative count")
    out = 0  # crc of the empty string
    while times:
        if times & 1:
            out = crc32_combine(out, crc, nbytes)
        crc = crc32_combine(crc, crc, nbytes)
        nbytes *= 2
        times >>= 1
    return out


def crc32_periodic_reference(block: bytes | np.ndarray, start: int,
                             length: int) -> int:
    """zlib.crc32 of the `length` bytes from byte `start` of the endless
    repetition of `block`, without materialising them: zlib on one whole
    block rotated to the phase of `start` and on one partial block,
    joined with crc32_repeat / crc32_combine.  Exact for any length below
    2**64; the GPU tests' reference for multi-GiB periodic buffers."""
    blk = np.asarray(block, dtype=np.uint8).tobytes()
    period = len(blk)
    if period == 0 or start < 0 or length < 0:
        raise ValueError("empty block or negative range")
    phase = start % period
    whole, rest = divmod(length, period)

    def take(n):  # the n <= period bytes from the phase on
        head = blk[phase : phase + n]
        return head + blk[: n - len(head)]

    crc = crc32_repeat(zlib.crc32(take(period)), period, whole) if whole else 0
    return crc32_combine(crc, zlib.crc32(take(rest)), rest)


def crc32_messages_reference(data: bytes | np.ndarray, msg_bytes: int,
                             offs=None) -> np.ndarray:
    """zlib.crc32 of each msg_bytes message, as uint32 array: message m
    is data[offs[m] : offs[m] + msg_bytes], back to back without offs."""
    buf = np.asarray(data, dtype=np.uint8).tobytes()
    if offs is None:
        assert len(buf) % msg_bytes == 0
        offs = range(0, len(buf), msg_bytes)
    out = []
    for o in offs:
        o = int(o)
        assert 0 <= o and o + msg_bytes <= len(buf)
        out.append(zlib.crc32(buf[o : o + msg_bytes]))
    return np.array(out, dtype=np.uint32)


def crc32_messages_v_reference(data: bytes | np.ndarray, offs,
                               lens) -> np.ndarray:
    """zlib.crc32 of data[offs[m] : offs[m] + lens[m]] for every m, as
    uint32 array (a zero-length message digests to 0)."""
    buf = np.asarray(data, dtype=np.uint8).tobytes()
    assert len(offs) == len(lens)
    out = []
    for o, ln in zip(offs, lens):
        o, ln = int(o), int(ln)
        assert 0 <= o and 0 <= ln and o + ln <= len(buf)
        out.append(zlib.crc32(buf[o : o + ln]))
    return np.array(out, dtype=np.uint32)
