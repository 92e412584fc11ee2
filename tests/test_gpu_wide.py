"""GPU tests: the wide tier — offsets, lengths and CRC shifts at and past
the 4 GiB boundary.  Regions of 2**32 bytes and more, messages longer
than 2**32 bytes and descriptors whose offsets do not fit in 32 bits go
through every digest kernel, every message engine and the streaming
kernels, against zlib and a numpy model.

The large HBM tensors are repetitions of one random block of
B = 16 * 65539 bytes.  B is an odd multiple of 16, so no power of two is
a multiple of B: an access displaced by 2**32 (or by any power of two
from 32 up) lands on another phase of the block, reads other bytes and
cannot hide behind the period.  The reference for any byte range is
pattern.crc32_periodic_reference — zlib on one block, joined by the
combine algebra — so nothing here pushes gigabytes through the host.

Every range a launch touches is computed and asserted in bounds on the
host before the launch; every access lies inside a tensor the test owns.
A case frees what it allocated; with the shared `wide` tensor the module
holds at most about 14 GiB at once."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

B = 16 * 65539                         # the period, 1 048 624 bytes
T = 1 << 32                            # the boundary
L = T + (1 << 26) + 4096 + 5           # bytes of `wide`
RB = T + (1 << 20)                     # bytes of a gather region
LONG = T + (1 << 24) + 16              # one message of more than 4 GiB
NEED = 14 << 30                        # HBM the module may hold at once
CANARY = 0xA5
PAD = 64
OUTSIDE = 128 << 10                    # pinned bytes on the outside


@pytest.fixture(scope="module")
def ops():
    import rocnrdma_amd.ops as ops

    return ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def block():
    assert T % B and (1 << 33) % B and B % 16 == 0 and (B // 16) % 2
    return np.random.default_rng(20240229).integers(0, 256, B, dtype=np.uint8)


@pytest.fixture(scope="module")
def wide(dev, block):
    """block repeated to L bytes in HBM; shared and never written."""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < NEED:
        pytest.skip(f"the wide tier needs {NEED >> 30} GiB of free HBM, "
                    f"the device has {free >> 30}")
    t = torch.from_numpy(block).to(dev).repeat(-(-L // B))[:L]
    assert t.numel() == L and t.data_ptr() % 16 == 0 and t.is_contiguous()
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ref(block):
    """zlib.crc32 of wide[start : start + length], computed once per range."""
    from rocnrdma_amd.utils import pattern

    seen = {}

    def crc(start, length):
        assert 0 <= start and 0 <= length and start + length <= L
        key = (start, length)
        if key not in seen:
            seen[key] = pattern.crc32_periodic_reference(block, start, length)
        return seen[key]

    return crc


@pytest.fixture(scope="module")
def host_src():
    """One pinned random buffer, shared and never written."""
    t = torch.empty(OUTSIDE, dtype=torch.uint8, pin_memory=True)
    assert t.data_ptr() % 16 == 0
    t.numpy()[:] = np.random.default_rng(97).integers(0, 256, OUTSIDE,
                                                      dtype=np.uint8)
    return t


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev64(a, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)


def _wide_bytes(block, start, length):
    """wide[start : start + length] from the periodic model, on the host."""
    return block[(start + np.arange(length, dtype=np.int64)) % B]


def _equal(a, b, step=1 << 28):
    """torch.equal in slices, so that no multi-GiB temporary is made."""
    assert a.shape == b.shape and a.dim() == 1
    return all(torch.equal(a[i:i + step], b[i:i + step])
               for i in range(0, a.numel(), step))


def _all_canary(t):
    return bool((t == CANARY).all().item())


# -- 1. region digest across the shift tree ----------------------------------
REGION_SIZES = [(1 << 24) - 16, (1 << 24) + 4097, T - 16, T, T + 4097, L]
REGION_CASES = [(n, 0) for n in REGION_SIZES] + [(T + 4097, 1), (L, 1)]


@pytest.mark.parametrize("n,grid_cap", REGION_CASES)
def test_region_digest(ops, wide, ref, n, grid_cap):
    """ops.crc32 with up to L bytes behind a flush: xpow8[3] from 16 MiB
    on, xpow8[4] and the third level of crc_xpow_wave's tree from 4 GiB
    on — in some sixty waves at once at L, whose default runs are about
    1 MiB."""
    assert n <= L
    assert ops.crc32(wide[:n], grid_cap=grid_cap) == ref(0, n)


# -- 2. per-message digests with long messages -------------------------------
# two overlapping messages of more than 4 GiB (a digest only reads) and
# short neighbours on and around the boundary
V_OFFS = [0, 48, 64, T - 16, T - 4096, T - (1 << 24)]
V_LENS = [LONG + 4097, LONG, 0, 17, 4097, (1 << 24) + 33]
B_OFFS = [5, 48 + 11, 77, T - 9, T - 4090, T - (1 << 24) + 7]
B_LENS = V_LENS
# (max_msg_bytes, grid_cap): unknown, wrong and small (its grid is one
# workgroup as well), exact; grid_cap 1 makes the hint irrelevant
HINTS = [(0, 0), (4096, 0), (max(V_LENS), 0), (max(V_LENS), 1), (0, 1)]


@pytest.mark.parametrize("grid_cap", [0, 1])
def test_long_messages_uniform(ops, dev, wide, ref, grid_cap):
    offs = [0, 48]
    assert all(o % 16 == 0 and o + LONG <= L for o in offs)
    got = ops.crc32_messages(wide, LONG, _dev64(offs, dev), grid_cap=grid_cap)
    assert _u32(got).tolist() == [ref(o, LONG) for o in offs]


@pytest.mark.parametrize("hint,grid_cap", HINTS)
def test_long_messages_varlen(ops, dev, wide, ref, hint, grid_cap):
    assert all(o % 16 == 0 and o + n <= L for o, n in zip(V_OFFS, V_LENS))
    got = ops.crc32_messages_v(wide, _dev64(V_OFFS, dev), _dev64(V_LENS, dev),
                               max_msg_bytes=hint, grid_cap=grid_cap)
    assert _u32(got).tolist() == [ref(o, n) for o, n in zip(V_OFFS, V_LENS)]


@pytest.mark.parametrize("hint,grid_cap", HINTS)
def test_long_messages_bytes(ops, dev, wide, ref, hint, grid_cap):
    assert all(o + n <= L for o, n in zip(B_OFFS, B_LENS))
    got = ops.crc32_messages_bytes(wide, _dev64(B_OFFS, dev),
                                   _dev64(B_LENS, dev), max_msg_bytes=hint,
                                   grid_cap=grid_cap)
    assert _u32(got).tolist() == [ref(o, n) for o, n in zip(B_OFFS, B_LENS)]


# -- 3. contiguous uniform digest past 4 GiB ---------------------------------
MSG = 65536
N_MSGS = T // MSG + 64  # m * MSG crosses 2**32 at m = 65536


def _sample(n, pivot, seed, total=200):
    """The first and the last 8 items, every one within 4 of the pivot
    and a seeded random rest."""
    pick = set(range(8)) | set(range(n - 8, n))
    pick |= set(range(pivot - 4, pivot + 5))
    rng = np.random.default_rng(seed)
    while len(pick) < total:
        pick.add(int(rng.integers(0, n)))
    return sorted(pick)


def _check_sampled(got, idx, item_bytes, ref, dev):
    got = _u32(got[_dev64(idx, dev)])
    want = np.array([ref(i * item_bytes, item_bytes) for i in idx],
                    dtype=np.uint32)
    assert (got == want).all()
    # an item read 2**32 bytes early or late is an item of another phase:
    # no two phases of the sample may share a digest
    by_phase = {(i * item_bytes) % B: int(g) for i, g in zip(idx, got)}
    assert len(set(by_phase.values())) == len(by_phase) > 150


def test_uniform_messages_past_4gib(ops, dev, wide, ref):
    assert N_MSGS * MSG > T and N_MSGS * MSG <= L
    got = ops.crc32_messages(wide[:N_MSGS * MSG], MSG)
    assert got.shape == (N_MSGS,)
    _check_sampled(got, _sample(N_MSGS, T // MSG, 5), MSG, ref, dev)


def test_pages_past_4gib(ops, dev, wide, ref):
    npages = N_MSGS * MSG // 4096
    got = ops.crc32_pages(wide[:N_MSGS * MSG])
    assert got.shape == (npages,)
    _check_sampled(got, _sample(npages, T // 4096, 6), 4096, ref, dev)


# -- 4. offsets beyond 4 GiB in every engine ---------------------------------
KINDS = ["uniform", "v", "bytes", "sg"]


def _batches(kind, size):
    """[(msg_bytes or None, [(region offset, length), ...]), ...] for a
    region of `size` bytes: a message low in the region, one ending
    exactly at 2**32, one starting there, one at 2**32 + odd, one ending
    on the region's last byte — and, in a batch of its own because it
    overlaps the two at the boundary, one straddling 2**32 from
    2**32 - 2049 - skew.  The aligned engines take multiples of 16, so
    their "odd" is an odd number of granules and their last message ends
    on the region's last whole granule."""
    if kind in ("bytes", "sg"):
        a = [(3, 4113), (65536 + 9, 16), (T - 12289, 12289), (T, 4097),
             (T + 65537, 33), (size - 8191, 8191), (T + (1 << 19) + 7, 47),
             ((1 << 20) + 15, 12287)]
        b = [(T - 2049 - 13, 8191), (131072 + 1, 1),
             (T + (1 << 18) + 5, 4095), ((1 << 21) + 8, 17)]
        return [(None, a), (None, b)]
    end = size & ~15
    if kind == "v":
        a = [(0, 4112), (65536, 16), (T - 12288, 12288), (T, 4096),
             (T + 65552, 48), (end - 8192, 8192), (T + (1 << 19), 2064),
             (1 << 20, 12272)]
        b = [(T - 2049 - 15, 8192), (131072, 16), (T + (1 << 18), 4080),
             (1 << 21, 32)]
        return [(None, a), (None, b)]
    out = []
    for mb in (16, 4112, 12288):
        a = [0, 65536, T - mb, T, T + 65552, end - mb, T + (1 << 19)]
        b = [131072, T + (1 << 18)] + ([T - 2049 - 15] if mb > 2064 else [])
        out += [(mb, [(o, mb) for o in a]), (mb, [(o, mb) for o in b])]
    return out


def _plan(kind, msgs, size):
    """Lay a batch out on the outside: [(region offset, [(outside offset,
    length), ...])] with one entry per SGE (one SGE per message unless
    kind is "sg"), every SGE in a slot of its own with at least 16 canary
    bytes between slots.  The byte-granular kinds get a different skew on
    either side of most messages.  Asserts every range in bounds."""
    bytewise = kind in ("bytes", "sg")
    cuts = []
    for m, (off, ln) in enumerate(msgs):
        assert 0 <= off and off + ln <= size
        assert bytewise or (off % 16 == 0 and ln % 16 == 0 and ln > 0)
        if kind != "sg":
            parts = [ln]
        elif off < T < off + ln:  # one SGE ends exactly at the boundary
            parts = [T - off, (off + ln - T) // 3, 0]
            parts.append(ln - sum(parts))
        elif ln >= 3:
            parts = [ln // 3, 0, ln // 3]
            parts.append(ln - sum(parts))
        else:
            parts = [ln]
        assert sum(parts) == ln and min(parts) >= 0
        cuts.append((off, parts))
    # slots in reverse SGE order, so a gather really gathers
    at, where = PAD, {}
    for m in reversed(range(len(cuts))):
        for j in reversed(range(len(cuts[m][1]))):
            sl = cuts[m][1][j]
            skew = (3 + 5 * (m + j)) % 16 if bytewise else 0
            at = (at + 15) // 16 * 16 + skew
            where[m, j] = at
            at += sl + 16
    assert at + PAD <= OUTSIDE
    return [(off, [(where[m, j], sl) for j, sl in enumerate(parts)])
            for m, (off, parts) in enumerate(cuts)]


def _launch(ops, gather, kind, crc, region, plan, base, mb, dev):
    """One engine launch for a planned batch; `base` is the address of the
    outside buffer.  Returns the digests or None."""
    offs = _dev64([off for off, _ in plan], dev)
    if kind == "sg":
        fn = ops.gather_sg_ if gather else ops.scatter_sg_
        start = np.cumsum([0] + [len(sges) for _, sges in plan])
        flat = [s for _, sges in plan for s in sges]
        return fn(region, offs, _dev64(start, dev),
                  _dev64([base + oo for oo, _ in flat], dev),
                  _dev64([sl for _, sl in flat], dev), crc=crc)
    addrs = _dev64([base + sges[0][0] for _, sges in plan], dev)
    if kind == "uniform":
        if crc:
            fn = ops.gather_crc_ if gather else ops.scatter_crc_
        else:
            fn = ops.gather_ if gather else ops.scatter_
        return fn(region, offs, addrs, mb)
    fn = {("v", True): ops.gather_v_, ("v", False): ops.scatter_v_,
          ("bytes", True): ops.gather_bytes_,
          ("bytes", False): ops.scatter_bytes_}[kind, gather]
    return fn(region, offs, addrs, _dev64([sges[0][1] for _, sges in plan],
                                          dev), crc=crc)


def _sides_of_boundary(plan):
    """Does a message of the plan have an SGE wholly below 2**32 and one
    wholly at or above it?"""
    for off, sges in plan:
        p, below, above = off, False, False
        for _, sl in sges:
            below |= sl > 0 and p + sl <= T
            above |= sl > 0 and p >= T
            p += sl
        if below and above:
            return True
    return False


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_beyond_4gib(ops, dev, wide, host_src, kind, crc):
    """Pinned sources into a canary-filled region of 2**32 + 2**20 bytes:
    a store whose offset lost its upper bits lands in the low 4 GiB of the
    same tensor and breaks a canary there."""
    src = host_src.numpy()
    src_gpu = host_src.to(dev)
    region = torch.full((RB,), CANARY, dtype=torch.uint8, device=dev)
    expected = torch.full((RB,), CANARY, dtype=torch.uint8, device=dev)
    both_sides = False
    for mb, msgs in _batches(kind, RB):
        plan = _plan(kind, msgs, RB)
        both_sides |= _sides_of_boundary(plan)
        got = _launch(ops, True, kind, crc, region, plan,
                      host_src.data_ptr(), mb, dev)
        want = []
        for off, sges in plan:
            p, c = off, 0
            for oo, sl in sges:
                expected[p:p + sl] = src_gpu[oo:oo + sl]
                c = zlib.crc32(src[oo:oo + sl].tobytes(), c)
                p += sl
            want.append(c)
        assert _equal(region, expected)
        if crc:
            assert _u32(got).tolist() == want
        else:
            assert got is None
    assert both_sides or kind != "sg"
    del region, expected, src_gpu
    torch.cuda.empty_cache()


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_scatter_beyond_4gib(ops, dev, wide, block, ref, kind, crc):
    """From `wide`, read-only, into a canary-filled pinned buffer: byte for
    byte the periodic model, and a load displaced by 2**32 reads another
    phase of the block."""
    both_sides = False
    for mb, msgs in _batches(kind, L):
        plan = _plan(kind, msgs, L)
        both_sides |= _sides_of_boundary(plan)
        want = np.full(OUTSIDE, CANARY, dtype=np.uint8)
        for off, sges in plan:
            p = off
            for oo, sl in sges:
                want[oo:oo + sl] = _wide_bytes(block, p, sl)
                p += sl
        dst = torch.empty(OUTSIDE, dtype=torch.uint8, pin_memory=True)
        assert dst.data_ptr() % 16 == 0
        dst.fill_(CANARY)
        got = _launch(ops, False, kind, crc, wide, plan, dst.data_ptr(), mb,
                      dev)
        torch.cuda.synchronize(dev)
        assert (dst.numpy() == want).all()
        if crc:
            assert _u32(got).tolist() == [
                ref(off, sum(sl for _, sl in sges)) for off, sges in plan]
        else:
            assert got is None
    assert both_sides or kind != "sg"
    assert ops.crc32(wide) == ref(0, L)  # the region was only read


# -- 5. long messages through the ICRC engines, HBM to HBM -------------------
LONG_ENGINES = ["gather_crc", "gather_v", "gather_bytes", "scatter_bytes"]


@pytest.mark.parametrize("grid_cap", [0, 1])
@pytest.mark.parametrize("engine", LONG_ENGINES)
def test_long_message_icrc(ops, dev, wide, ref, engine, grid_cap):
    """One message of more than 4 GiB from `wide` into a second HBM tensor
    (the outside address of a message is a flat address: device memory
    serves as well as pinned memory).  The byte engine moves 5 bytes more,
    from skew 3 to skew 11."""
    bytewise = engine.endswith("bytes")
    ln = LONG + 5 if bytewise else LONG
    so, do = (PAD + 3, PAD + 11) if bytewise else (PAD, PAD)
    assert so + ln <= L
    dst = torch.full((do + ln + PAD,), CANARY, dtype=torch.uint8, device=dev)
    assert dst.data_ptr() % 16 == 0
    d_ln = _dev64([ln], dev)
    if engine == "scatter_bytes":  # the region is the side that is read
        got = ops.scatter_bytes_(wide, _dev64([so], dev),
                                 _dev64([dst.data_ptr() + do], dev), d_ln,
                                 crc=True, grid_cap=grid_cap)
    else:
        offs, addrs = _dev64([do], dev), _dev64([wide.data_ptr() + so], dev)
        if engine == "gather_crc":
            got = ops.gather_crc_(dst, offs, addrs, ln, grid_cap=grid_cap)
        else:
            fn = ops.gather_bytes_ if bytewise else ops.gather_v_
            got = fn(dst, offs, addrs, d_ln, crc=True, grid_cap=grid_cap)
    assert _u32(got).tolist() == [ref(so, ln)]
    assert _equal(dst[do:do + ln], wide[so:so + ln])
    assert _all_canary(dst[:do]) and _all_canary(dst[do + ln:])
    del dst
    torch.cuda.empty_cache()


WIN = (1 << 26) + 7
NSGE = 70


@pytest.mark.parametrize("grid_cap", [0, 1])
def test_long_message_sg_icrc(ops, dev, wide, ref, grid_cap):
    """One message of 70 SGEs that all read the same window of `wide`,
    then a short message: the byte prefix crosses 2**32 and the tails run
    from more than 4 GiB down to 0."""
    from rocnrdma_amd.utils import pattern

    wo = T - (1 << 25) + 5  # the window straddles the boundary
    so, sn = 17, 4097       # the short message
    off0 = 9
    off1 = off0 + NSGE * WIN  # back to back: they share a granule
    assert wo + WIN <= L and so + sn <= L
    assert (NSGE - 1) * WIN > T  # the first SGE's tail is above 4 GiB
    size = off1 + sn + PAD
    region = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    assert region.data_ptr() % 16 == 0
    base = wide.data_ptr()
    got = ops.gather_sg_(region, _dev64([off0, off1], dev),
                         _dev64([0, NSGE, NSGE + 1], dev),
                         _dev64([base + wo] * NSGE + [base + so], dev),
                         _dev64([WIN] * NSGE + [sn], dev), crc=True,
                         grid_cap=grid_cap)
    assert _u32(got).tolist() == [
        pattern.crc32_repeat(ref(wo, WIN), WIN, NSGE), ref(so, sn)]
    window = wide[wo:wo + WIN]
    for j in range(NSGE):
        at = off0 + j * WIN
        assert torch.equal(region[at:at + WIN], window), j
    assert torch.equal(region[off1:off1 + sn], wide[so:so + sn])
    assert _all_canary(region[:off0]) and _all_canary(region[off1 + sn:])
    del region, window
    torch.cuda.empty_cache()


# -- 6. streaming kernels ----------------------------------------------------
def test_streaming_kernels_past_4gib(ops, dev, wide):
    from rocnrdma_amd.utils import pattern

    nbytes, seed = T + 4096 + 8, 0x5EED
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed)
    assert ops.verify(buf, seed) == 0
    for start in (0, T - 2048, nbytes - 4096):
        words = buf[start:start + 4096].cpu().numpy().view(np.uint64)
        assert (words == pattern.splitmix64_words(seed, start // 8,
                                                  512)).all()
    buf[T + 1234] ^= 1
    assert ops.verify(buf, seed) == 1
    buf[T + 1234] ^= 1
    assert ops.verify(buf, seed) == 0
    # the copies take multiples of 16 bytes: all but the last word
    src = buf[:nbytes - 8]
    dst = torch.full((nbytes - 8,), CANARY, dtype=torch.uint8, device=dev)
    ops.copy_(dst, src)
    assert _equal(dst, src)
    dst.fill_(CANARY)
    ops.copy_nt_(dst, src)
    assert _equal(dst, src)
    assert ops.verify(buf, seed) == 0  # the source is as it was
    del buf, src, dst
    torch.cuda.empty_cache()
