"""GPU tests: scatter/gather lists — messages that are the concatenation
of several outside buffers — in the message engine (ops.gather_sg_ /
scatter_sg_, with and without the inline ICRC) against a numpy model,
zlib and the byte-granular engines; and max_sge > 1 on the sdma
transport and the soak."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

CANARY = 0xA5
PAD = 64              # canary bytes around everything that is written
HOST_BYTES = 3 << 20  # covers every batch below
L_CUT = 3 * 4096 + 2049
CUTS = [
    [L_CUT],
    [1, L_CUT - 1],
    [L_CUT - 1, 1],
    [15, 17, 4064, L_CUT - 4096],
    [4096, 4096, L_CUT - 8192],
    [0, 4097, 0, 0, L_CUT - 4097, 0],
]
# tests/test_gpu_bytes.py's length set
LEN_SET = [0, 1, 3, 16, 33, 1023, 4080, 4095, 4096, 4097, 4113, 8191,
           3 * 4096 + 2049, 65537]
RAGGED_COUNTS = [0, 1, 2, 7, 0, 0, 3, 30, 1, 0]
RAGGED_LENS = [0, 1, 3, 15, 16, 17, 33, 4095, 4096, 4097, 8191]
BIG = (1 << 20) + 81


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def host():
    """One pinned random buffer, shared and never written."""
    t = torch.empty(HOST_BYTES, dtype=torch.uint8, pin_memory=True)
    assert t.data_ptr() % 16 == 0
    t.numpy()[:] = np.random.default_rng(83).integers(
        0, 256, HOST_BYTES, dtype=np.uint8)
    return t


@pytest.fixture(scope="module")
def hbm_src(dev, host):
    """The same random bytes in HBM: the scatter cases' region."""
    return host.to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def _packed(lens, base, seed=None):
    """Byte offsets of ranges packed back to back from `base`, in order
    or (seed) in a permuted order: neighbours then share granules."""
    lens = _i64(lens)
    if seed is None:
        return base + np.cumsum(lens) - lens
    perm = np.random.default_rng(seed).permutation(len(lens))
    offs = np.empty(len(lens), dtype=np.int64)
    offs[perm] = base + np.cumsum(lens[perm]) - lens[perm]
    return offs


class Batch:
    """A batch in CSR form, in byte offsets: message m at region offset
    offs[m] owns counts[m] SGEs; SGE j is sge_lens[j] bytes at offset
    sge_at[j] of the outside buffer."""

    def __init__(self, counts, sge_lens, offs, sge_at):
        self.counts, self.sge_lens = _i64(counts), _i64(sge_lens)
        self.offs, self.sge_at = _i64(offs), _i64(sge_at)
        self.n, self.nsge = len(self.counts), len(self.sge_lens)
        self.start = np.concatenate([[0], np.cumsum(self.counts)]).astype(
            np.int64)
        assert self.start[-1] == self.nsge == len(self.sge_at)
        assert len(self.offs) == self.n and (self.sge_lens >= 0).all()
        self.msg_lens = _i64([self.sge_lens[a:b].sum() for a, b in
                              zip(self.start[:-1], self.start[1:])])

    def device(self, dev, outside_ptr):
        return (torch.from_numpy(self.offs).to(dev),
                torch.from_numpy(self.start).to(dev),
                torch.from_numpy(outside_ptr + self.sge_at).to(dev),
                torch.from_numpy(self.sge_lens).to(dev))

    def flat(self):
        """The same bytes as one gather_bytes_ / scatter_bytes_ message
        per SGE: (region offsets, outside offsets, lens), host-made."""
        inside = np.empty(self.nsge, dtype=np.int64)
        for m in range(self.n):
            a, b = self.start[m], self.start[m + 1]
            ln = self.sge_lens[a:b]
            inside[a:b] = self.offs[m] + np.cumsum(ln) - ln
        return inside, self.sge_at, self.sge_lens


def _model_gather(b, src, size):
    """(expected region, zlib digests): canaries everywhere but the
    messages; asserts every range in bounds."""
    want = np.full(size, CANARY, dtype=np.uint8)
    crcs = np.empty(b.n, dtype=np.uint32)
    for m in range(b.n):
        parts = []
        for j in range(b.start[m], b.start[m + 1]):
            at, ln = b.sge_at[j], b.sge_lens[j]
            assert 0 <= at and at + ln <= src.size
            parts.append(src[at:at + ln])
        msg = np.concatenate(parts) if parts else np.empty(0, np.uint8)
        assert msg.size == b.msg_lens[m]
        assert 0 <= b.offs[m] and b.offs[m] + msg.size <= size - PAD
        want[b.offs[m]:b.offs[m] + msg.size] = msg
        crcs[m] = zlib.crc32(msg.tobytes())
    return want, crcs


def _model_scatter(b, src, size):
    """(expected outside buffer, zlib digests)."""
    want = np.full(size, CANARY, dtype=np.uint8)
    crcs = np.empty(b.n, dtype=np.uint32)
    taken = np.zeros(size, dtype=bool)
    for m in range(b.n):
        off, ln = b.offs[m], b.msg_lens[m]
        assert 0 <= off and off + ln <= src.size
        msg = src[off:off + ln]
        crcs[m] = zlib.crc32(msg.tobytes())
        pos = 0
        for j in range(b.start[m], b.start[m + 1]):
            at, k = b.sge_at[j], b.sge_lens[j]
            # (an SGE without bytes may point anywhere: it is not touched)
            assert k == 0 or (0 <= at and at + k <= size)
            assert not taken[at:at + k].any()  # the written side: disjoint
            taken[at:at + k] = True
            want[at:at + k] = msg[pos:pos + k]
            pos += k
        assert pos == ln
    return want, crcs


def _gather(src, dev, b, **kw):
    """Gather from the pinned tensor src into a canary-filled region,
    twice; bytes, canaries and (crc=True) digests against numpy and zlib.
    Returns (region bytes, digests or None)."""
    import rocnrdma_amd.ops as ops

    size = (int((b.offs + b.msg_lens).max()) if b.n else 0) + PAD
    # the model first: it also proves every range in bounds
    want, crcs = _model_gather(b, src.numpy(), size)
    args = b.device(dev, src.data_ptr())
    region = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    got = ops.gather_sg_(region, *args, **kw)
    first = region.clone()
    again = ops.gather_sg_(region, *args, **kw)
    assert (region.cpu().numpy() == want).all()
    assert torch.equal(first, region)
    if kw.get("crc"):
        assert got.dtype == torch.int32 and got.shape == (b.n,)
        assert got.device == region.device
        assert (_u32(got) == crcs).all()
        assert torch.equal(got, again)  # no stale scratch or accumulator
        return want, _u32(got)
    assert got is None and again is None
    return want, None


def _scatter(hbm_src, dev, b, size, **kw):
    """Scatter from the random HBM tensor into a canary-filled pinned
    buffer of exactly `size` bytes, twice."""
    import rocnrdma_amd.ops as ops

    src = hbm_src.cpu().numpy()
    want, crcs = _model_scatter(b, src, size)

    def run():
        dst = torch.empty(max(size, 1), dtype=torch.uint8, pin_memory=True)
        assert dst.data_ptr() % 16 == 0
        dst.fill_(CANARY)
        out = ops.scatter_sg_(hbm_src, *b.device(dev, dst.data_ptr()), **kw)
        torch.cuda.synchronize(dev)
        return dst.numpy()[:size].copy(), out

    dst, got = run()
    dst2, again = run()
    assert (dst == want).all() and (dst2 == want).all()
    assert (hbm_src.cpu().numpy() == src).all()  # the region is only read
    if kw.get("crc"):
        assert got.dtype == torch.int32 and got.shape == (b.n,)
        assert (_u32(got) == crcs).all()
        assert torch.equal(got, again)
        return want, _u32(got)
    assert got is None and again is None
    return want, None


# -- one message, cut in every way ------------------------------------------
STRIDE = (L_CUT + 2 * PAD + 15) // 16 * 16  # one SGE's own padded area


def _cut_at(cut):
    """SGE k in its own area, at skew (7k + 3) & 15."""
    return _i64([k * STRIDE + PAD + ((7 * k + 3) & 15)
                 for k in range(len(cut))])


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("rskew", [0, 5, 15])
def test_gather_cuts(host, dev, rskew, crc):
    msg = host.numpy()[77:77 + L_CUT]
    regions, digests = [], []
    for cut in CUTS:
        at = _cut_at(cut)
        src = torch.empty(len(cut) * STRIDE, dtype=torch.uint8,
                          pin_memory=True)
        src.fill_(CANARY)
        pos = 0
        for a, k in zip(at, cut):
            src.numpy()[a:a + k] = msg[pos:pos + k]
            pos += k
        b = Batch([len(cut)], cut, [PAD + rskew], at)
        region, dig = _gather(src, dev, b, crc=crc)
        regions.append(region)
        digests.append(dig)
    assert all((r == regions[0]).all() for r in regions)
    if crc:
        assert all(d[0] == zlib.crc32(msg.tobytes()) for d in digests)


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("rskew", [0, 5, 15])
def test_scatter_cuts(hbm_src, dev, rskew, crc):
    off = 16 * 9 + rskew
    whole = zlib.crc32(hbm_src[off:off + L_CUT].cpu().numpy().tobytes())
    for cut in CUTS:
        at = _cut_at(cut)
        b = Batch([len(cut)], cut, [off], at)
        # the buffer ends with the last SGE that has bytes
        size = int((at + _i64(cut))[_i64(cut) > 0].max())
        _, dig = _scatter(hbm_src, dev, b, size, crc=crc)
        if crc:
            assert dig[0] == whole


# -- ragged batches -----------------------------------------------------------
def _ragged(counts, choices, seed, region_base, out_base):
    """Messages back to back in the region in a permuted order, SGEs back
    to back outside in another: disjoint on both sides."""
    rng = np.random.default_rng(seed)
    counts = _i64(counts)
    lens = rng.choice(choices, int(counts.sum())).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)])
    msg_lens = [lens[a:b].sum() for a, b in zip(start[:-1], start[1:])]
    return Batch(counts, lens, _packed(msg_lens, region_base, seed=seed + 1),
                 _packed(lens, out_base, seed=seed + 2))


def _both(host, hbm_src, dev, b, **kw):
    """Gather and scatter the batch, crc off and on; the bytes must not
    depend on crc.  Returns the gathered region and both digest sets."""
    size = int((b.sge_at + b.sge_lens).max()) if b.nsge else 0
    g_plain, _ = _gather(host, dev, b, **kw)
    g_fused, g_dig = _gather(host, dev, b, crc=True, **kw)
    assert (g_plain == g_fused).all()
    s_plain, _ = _scatter(hbm_src, dev, b, size, **kw)
    s_fused, s_dig = _scatter(hbm_src, dev, b, size, crc=True, **kw)
    assert (s_plain == s_fused).all()
    empty = b.msg_lens == 0
    assert (g_dig[empty] == 0).all() and (s_dig[empty] == 0).all()
    return g_plain, g_dig, s_dig


def test_ragged_batch(host, hbm_src, dev):
    b = _ragged(RAGGED_COUNTS, RAGGED_LENS, 11, PAD + 11, 16 * 5 + 3)
    assert (b.sge_lens == 0).any() and (b.sge_lens > 4096).any()
    _both(host, hbm_src, dev, b)
    _both(host, hbm_src, dev, b, grid_cap=1)


def test_scan_tiles(host, hbm_src, dev):
    """More messages and more SGEs than the scan has threads: several
    tiles per wave, runs of empty messages and SGEs throughout."""
    counts = np.arange(1500) % 4
    b = _ragged(counts, np.arange(49), 13, PAD + 7, 16 * 3 + 9)
    assert b.n == 1500 and b.nsge == 2250
    _both(host, hbm_src, dev, b)


def test_empty_runs_at_the_ends(host, hbm_src, dev):
    """Empty messages and empty SGEs first, last and in between; a batch
    without any SGE only zeroes the digests."""
    import rocnrdma_amd.ops as ops

    b = Batch([0, 0, 2, 3, 0, 1, 0, 0], [0, 0, 0, 4097, 0, 33],
              [3, 3, 3, PAD + 1, 0, PAD + 4200, 9, 9],
              [5, 5, 5, 16 * 4 + 7, 1, 16 * 300 + 1])
    _both(host, hbm_src, dev, b)
    _both(host, hbm_src, dev, Batch([0, 0, 0], [], [1, 2, 3], []))
    _both(host, hbm_src, dev, Batch([1, 2], [0, 0, 0], [1, 2], [7, 8, 9]))
    # n == 0 is a no-op
    none = torch.empty(0, dtype=torch.int64, device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    region = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    out = ops.gather_sg_(region, none, zero, none, none, crc=True)
    assert out.shape == (0,) and (region == CANARY).all()


# -- long messages, every grid -------------------------------------------------
def test_long_messages_do_not_depend_on_the_grid(host, hbm_src, dev):
    lens = [BIG, 4097, 65537, 17, 8191, 1, 4095]
    b = Batch([3, 1, 3], lens, _packed([sum(lens[:3]), 17, sum(lens[4:])],
                                       PAD + 11),
              # 9 bytes more between neighbours: mutually misaligned
              _i64(_packed(lens, 16 * 5 + 3)) + 9 * np.arange(len(lens)))
    assert len(set((b.sge_at[:3] % 16).tolist())) == 3
    exact = int(b.msg_lens.max())
    base = _both(host, hbm_src, dev, b)
    for grid_cap in (0, 1, 3):
        for hint in (0, exact):
            got = _both(host, hbm_src, dev, b, grid_cap=grid_cap,
                        max_msg_bytes=hint)
            assert all((x == y).all() for x, y in zip(got, base))


# -- equivalences -----------------------------------------------------------
def test_one_sge_per_message_equals_the_byte_engine(host, hbm_src, dev):
    import rocnrdma_amd.ops as ops

    lens = np.random.default_rng(5).choice(LEN_SET, 37).astype(np.int64)
    lens[:len(LEN_SET)] = LEN_SET
    inside, outside = _packed(lens, PAD + 11, seed=1), _packed(lens, 83)
    b = Batch(np.ones(len(lens)), lens, inside, outside)
    d = [torch.from_numpy(x).to(dev) for x in (inside, lens)]
    size = int((outside + lens).max())
    for crc in (False, True):
        new, d_new = _gather(host, dev, b, crc=crc)
        region = torch.full((len(new),), CANARY, dtype=torch.uint8,
                            device=dev)
        d_old = ops.gather_bytes_(
            region, d[0], torch.from_numpy(host.data_ptr() + outside).to(dev),
            d[1], crc=crc)
        assert (region.cpu().numpy() == new).all()
        assert crc is False or (_u32(d_old) == d_new).all()

        new, d_new = _scatter(hbm_src, dev, b, size, crc=crc)
        dst = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        dst.fill_(CANARY)
        d_old = ops.scatter_bytes_(
            hbm_src, d[0], torch.from_numpy(dst.data_ptr() + outside).to(dev),
            d[1], crc=crc)
        torch.cuda.synchronize(dev)
        assert (dst.numpy() == new).all()
        assert crc is False or (_u32(d_old) == d_new).all()


def test_ragged_batch_equals_its_flattening(host, dev):
    """What a user had to do before: one gather_bytes_ message per SGE
    with region offsets made on the host."""
    import rocnrdma_amd.ops as ops

    b = _ragged(RAGGED_COUNTS, RAGGED_LENS, 11, PAD + 11, 16 * 5 + 3)
    want, _ = _gather(host, dev, b)
    inside, outside, lens = b.flat()
    region = torch.full((len(want),), CANARY, dtype=torch.uint8, device=dev)
    ops.gather_bytes_(region, torch.from_numpy(inside).to(dev),
                      torch.from_numpy(host.data_ptr() + outside).to(dev),
                      torch.from_numpy(lens).to(dev))
    assert (region.cpu().numpy() == want).all()


def test_shared_sources(host, dev):
    """SGEs of different messages, and of one message, read the same
    outside range."""
    b = Batch([2, 3, 1], [4097, 33, 33, 4097, 4097, 4097],
              _packed([4130, 4130 + 4097, 4097], PAD + 5),
              [16 * 6 + 3, 16 * 2 + 1, 16 * 2 + 1, 16 * 6 + 3, 16 * 6 + 3,
               16 * 6 + 5])
    for crc in (False, True):
        _gather(host, dev, b, crc=crc)


# -- argument errors -----------------------------------------------------------
@pytest.mark.parametrize("name", ["gather_sg_", "scatter_sg_"])
def test_argument_errors_raise_before_any_launch(host, dev, name):
    import rocnrdma_amd.ops as ops

    fn = getattr(ops, name)
    region = torch.full((8192 + 16,), CANARY, dtype=torch.uint8, device=dev)
    dst = torch.empty(8192, dtype=torch.uint8, pin_memory=True)
    dst.fill_(CANARY)
    good = dict(
        offs=torch.tensor([16, 4096 + 16], device=dev),
        sge_start=torch.tensor([0, 2, 3], device=dev),
        sge_addrs=torch.tensor([0, 100, 4096], device=dev) + dst.data_ptr(),
        sge_lens=torch.tensor([100, 33, 4000], device=dev))
    wide = torch.arange(8, device=dev)
    bad = {
        "dtype": dict(offs=good["offs"].to(torch.int32)),
        "dtype_lens": dict(sge_lens=good["sge_lens"].to(torch.int32)),
        "device": dict(sge_addrs=good["sge_addrs"].cpu()),
        "device_start": dict(sge_start=good["sge_start"].cpu()),
        "non_contiguous": dict(sge_lens=wide[::3]),
        "non_contiguous_offs": dict(
            offs=torch.stack([good["offs"]] * 2, 1)[:, 0]),
        "sge_start_numel": dict(sge_start=torch.tensor([0, 3], device=dev)),
        "sge_start_long": dict(sge_start=torch.tensor([0, 1, 2, 3],
                                                      device=dev)),
        "addrs_vs_lens": dict(sge_addrs=good["sge_addrs"][:2].clone()),
        "negative_hint": dict(max_msg_bytes=-1),
        "negative_grid_cap": dict(grid_cap=-1),
    }
    for what, change in bad.items():
        kw = {**good, **change}
        with pytest.raises((RuntimeError, TypeError)):
            fn(region, kw.pop("offs"), kw.pop("sge_start"),
               kw.pop("sge_addrs"), kw.pop("sge_lens"), crc=True, **kw)
        torch.cuda.synchronize(dev)
        assert (region == CANARY).all(), what
        assert (dst.numpy() == CANARY).all(), what
    with pytest.raises(RuntimeError, match="aligned"):
        fn(region[1:], good["offs"], good["sge_start"], good["sge_addrs"],
           good["sge_lens"])
    with pytest.raises(RuntimeError):
        fn(region.cpu(), good["offs"], good["sge_start"], good["sge_addrs"],
           good["sge_lens"])
    torch.cuda.synchronize(dev)
    assert (region == CANARY).all() and (dst.numpy() == CANARY).all()
    # and the arguments they were derived from are accepted
    out = fn(region, good["offs"], good["sge_start"], good["sge_addrs"],
             good["sge_lens"], crc=True)
    want = [zlib.crc32(bytes([CANARY]) * k) for k in (133, 4000)]
    assert (_u32(out) == want).all()


# -- the sdma transport --------------------------------------------------------
MSG, REGION, K = 8192, 64 << 10, 3


def _layout(region_skew, n, seed=3):
    """(n, K, 2) disjoint lists, seeded, with an empty message, a 1-byte
    SGE, a message that fills the slot and SGEs out of slot order."""
    import random

    from rocnrdma_amd.harness.soak import mixed_sges

    room = MSG - region_skew
    sges = mixed_sges(random.Random(seed), n, MSG, K, room, disjoint=True)
    sges[0] = 0
    sges[1] = [(4096, 1), (0, 0), (17, 4000)]
    sges[2] = [(0, room), (0, 0), (0, 0)]
    sges[3] = [(5000, 33), (100, 4097), (4300, 15)]
    return sges


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("region_skew", [0, 9])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_digest_check_sg(dev, direction, region_skew, icrc):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=MSG, region_bytes=REGION,
                       device=dev, direction=direction, inflight=4,
                       var_len=True, byte_granular=True,
                       region_skew=region_skew, max_sge=K, icrc=icrc)
    assert tp.engine == "kernel" and tp.supports_sg_list
    assert tp.inflight == 4 < tp.msgs_per_region  # slots are reused
    sges = _layout(region_skew, tp.msgs_per_region)
    rng = np.random.default_rng(31)
    for _ in range(2):  # twice: nothing stale in the ring or the scratch
        payload = rng.integers(0, 256, REGION, dtype=np.uint8)
        assert tp.digest_check_sg(payload, sges) == 0
    assert tp.digest_check_sg(payload, np.zeros_like(sges)) == 0
    # post(i, nbytes) is post_sg(i, [(0, nbytes)]) here
    lens = np.array([0, 1, 4097, MSG - region_skew] * 2, dtype=np.int64)
    assert tp.digest_check(payload, lens) == 0
    tp.close()


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_digest_check_sg_counts_corruption(dev, direction, icrc):
    """The negative controls of digest_check_sg: one payload byte or one
    receiver slack byte of one message goes bad around the last flush,
    and exactly that message is counted."""
    import torch

    from rocnrdma_amd.transport import get_transport

    rs = 9
    tp = get_transport("sdma", msg_bytes=MSG, region_bytes=REGION,
                       device=dev, direction=direction, inflight=4,
                       var_len=True, byte_granular=True, region_skew=rs,
                       max_sge=K, icrc=icrc)
    n = tp.msgs_per_region
    bursts = -(-n // tp.inflight)
    assert bursts == 2  # slots are reused
    victim = n - 1  # of the last burst: its slot still holds it at the end
    sges = _layout(rs, n)
    sges[victim] = sges[3]  # non-empty, out of slot order, free slot bytes
    total = int(sges[victim, :, 1].sum())
    slot = tp.staging[victim % tp.inflight]
    write = direction == "write"
    real_flush = tp.flush
    calls = [0]

    def wrap(before, after):
        calls[0] = 0

        def flush():
            last = calls[0] + 1 == bursts
            if last and before:
                before()
            real_flush()
            calls[0] += 1
            if last and after:
                after()
        tp.flush = flush

    def payload(seed):
        return np.random.default_rng(seed).integers(0, 256, REGION,
                                                    dtype=np.uint8)

    # (a) one byte inside an SGE flipped: write — in the slot after the
    # sender digested it, before the engine loads it (what the inline
    # digest sees too); read — in the slot after it landed
    def flip():
        slot[100 + 7] ^= 1

    wrap(flip, None) if write else wrap(None, flip)
    assert tp.digest_check_sg(payload(1), sges) == 1
    assert calls[0] == bursts

    # (b) one slack byte of the receiver changed after the transfer: right
    # behind the message and right in front of it (write), outside every
    # SGE of the slot (read)
    def poke(at):
        def after():
            if write:
                tp.region[victim * MSG + at] ^= 0xFF
                torch.cuda.synchronize(dev)
            else:
                slot[50] ^= 0xFF
        return after

    for at in (rs + total, rs - 1) if write else (None,):
        wrap(None, poke(at))
        assert tp.digest_check_sg(payload(2), sges) == 1
        assert calls[0] == bursts

    # (c) the real flush again: clean
    tp.flush = real_flush
    assert tp.digest_check_sg(payload(3), sges) == 0
    tp.close()


def test_sdma_sg_needs_the_kernel_engine():
    from rocnrdma_amd.transport import get_transport

    with pytest.raises(ValueError, match="kernel engine"):
        get_transport("sdma", msg_bytes=MSG, region_bytes=REGION,
                      engine="stream", byte_granular=True, max_sge=2)


@pytest.mark.parametrize("icrc", [False, True])
def test_soak_sg_short(dev, icrc):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=0.5, region_bytes=4 << 20, seed=9,
                     device=dev, mixed=True, byte_granular=True, icrc=icrc,
                     sg=3)
    assert stats["cycles"] > 0 and stats["failures"] == 0
    assert stats["bytes"] > 0
