"""GPU tests: byte-granular messages — any length at any address — in the
message engine (ops.gather_bytes_ / scatter_bytes_, with and without the
inline ICRC) and in the landed-bytes digest (ops.crc32_messages_bytes),
against a numpy model, zlib and the variable-length engines; and
byte_granular=True on the sdma transport and the soak."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

PAIR_LENS = [1, 15, 17, 4095, 4097]
LEN_SET = [0, 1, 3, 16, 33, 1023, 4080, 4095, 4096, 4097, 4113, 8191,
           3 * 4096 + 2049, 65537]
COUNTS = [1, 5, 37]
CANARY = 0xA5
BIG = (1 << 20) + 81
HOST_BYTES = 6 << 20  # covers every batch below
PAD = 64              # canary bytes around a batch or a slot


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def host():
    """One pinned random buffer, shared and never written."""
    t = torch.empty(HOST_BYTES, dtype=torch.uint8, pin_memory=True)
    assert t.data_ptr() % 16 == 0
    t.numpy()[:] = np.random.default_rng(79).integers(
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
    """Byte offsets of messages packed back to back from `base`, in order
    or (seed) in a permuted order: neighbours then share granules."""
    lens = _i64(lens)
    if seed is None:
        return base + np.cumsum(lens) - lens
    perm = np.random.default_rng(seed).permutation(len(lens))
    offs = np.empty(len(lens), dtype=np.int64)
    offs[perm] = base + np.cumsum(lens[perm]) - lens[perm]
    return offs


def _model(src, lens, read_at, write_at, size):
    """(expected written side, zlib digests) for canaries everywhere but
    the messages."""
    want = np.full(size, CANARY, dtype=np.uint8)
    crcs = np.empty(len(lens), dtype=np.uint32)
    for m in range(len(lens)):
        assert read_at[m] >= 0 and write_at[m] >= 0
        assert write_at[m] + lens[m] <= size
        s = src[read_at[m]:read_at[m] + lens[m]]
        assert s.size == lens[m]
        want[write_at[m]:write_at[m] + lens[m]] = s
        crcs[m] = zlib.crc32(s.tobytes())
    return want, crcs


def _gather(host, dev, lens, inside, outside, fn=None, **kw):
    """Gather into a canary-filled region, twice; bytes, canaries and
    (crc=True) digests against numpy and zlib.  Returns (region bytes,
    digests or None)."""
    import rocnrdma_amd.ops as ops

    fn = fn or ops.gather_bytes_
    lens, inside, outside = _i64(lens), _i64(inside), _i64(outside)
    n = len(lens)
    size = (int((inside + lens).max()) if n else 0) + PAD
    # the model first: it also proves every range in bounds
    want, crcs = _model(host.numpy(), lens, outside, inside, size)
    d_offs = torch.from_numpy(inside).to(dev)
    d_addrs = torch.from_numpy(host.data_ptr() + outside).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)

    region = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    got = fn(region, d_offs, d_addrs, d_lens, **kw)
    first = region.clone()
    again = fn(region, d_offs, d_addrs, d_lens, **kw)

    assert (region.cpu().numpy() == want).all()
    assert torch.equal(first, region)
    if kw.get("crc"):
        assert got.dtype == torch.int32 and got.shape == (n,)
        assert got.device == region.device
        assert (_u32(got) == crcs).all()
        assert torch.equal(got, again)  # no stale scratch or accumulator
        return want, _u32(got)
    assert got is None and again is None
    return want, None


def _scatter(hbm_src, dev, lens, inside, outside, size, fn=None, **kw):
    """Scatter from the random HBM tensor into a canary-filled pinned
    buffer of exactly `size` bytes, twice."""
    import rocnrdma_amd.ops as ops

    fn = fn or ops.scatter_bytes_
    src = hbm_src.cpu().numpy()
    lens, inside, outside = _i64(lens), _i64(inside), _i64(outside)
    n = len(lens)
    # the model first: it also proves every range in bounds
    want, crcs = _model(src, lens, inside, outside, size)
    d_offs = torch.from_numpy(inside).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)

    def run():
        dst = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        assert dst.data_ptr() % 16 == 0
        dst.fill_(CANARY)
        d_addrs = torch.from_numpy(dst.data_ptr() + outside).to(dev)
        out = fn(hbm_src, d_offs, d_addrs, d_lens, **kw)
        torch.cuda.synchronize(dev)
        return dst.numpy().copy(), out

    dst, got = run()
    dst2, again = run()
    assert (dst == want).all() and (dst2 == want).all()
    assert (hbm_src.cpu().numpy() == src).all()  # the region is only read
    if kw.get("crc"):
        assert got.dtype == torch.int32 and got.shape == (n,)
        assert (_u32(got) == crcs).all()
        assert torch.equal(got, again)
        return want, _u32(got)
    assert got is None and again is None
    return want, None


# -- every pair of skews ------------------------------------------------------
SLOT = 4096 + 2 * PAD  # a message of up to 4097 bytes at skew < 16, padded


def _pairs():
    """Every (src skew, dst skew) for every length of PAIR_LENS: 1280
    messages, each in its own canary-padded slot on the written side."""
    lens, read_at, write_at = [], [], []
    k = 0
    for ln in PAIR_LENS:
        for ss in range(16):
            for ds in range(16):
                lens.append(ln)
                read_at.append(k * SLOT + 32 + ss)
                write_at.append(k * SLOT + 32 + ds)
                k += 1
    assert k == 1280 and k * SLOT <= HOST_BYTES
    return _i64(lens), _i64(read_at), _i64(write_at)


@pytest.mark.parametrize("crc", [False, True])
def test_gather_every_skew_pair(host, dev, crc):
    lens, read_at, write_at = _pairs()
    _gather(host, dev, lens, write_at, read_at, crc=crc)


@pytest.mark.parametrize("crc", [False, True])
def test_scatter_every_skew_pair(hbm_src, dev, crc):
    lens, read_at, write_at = _pairs()
    _scatter(hbm_src, dev, lens, read_at, write_at, 1280 * SLOT, crc=crc)


# -- mixed batches, packed at byte granularity --------------------------------
def _mixed(n, seed=None):
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    return rng.choice(LEN_SET, n).astype(np.int64)


def _gather_packed(host, dev, lens, **kw):
    """Sources in order from an odd address, destinations permuted and
    back to back from another odd offset."""
    return _gather(host, dev, lens, _packed(lens, PAD + 11, seed=1),
                   _packed(lens, 16 * 5 + 3), **kw)


def _scatter_packed(hbm_src, dev, lens, **kw):
    """Likewise; the last message ends on the pinned buffer's last byte."""
    total = int(_i64(lens).sum())
    return _scatter(hbm_src, dev, lens, _packed(lens, 16 * 7 + 9),
                    _packed(lens, PAD + 5, seed=2), PAD + 5 + total, **kw)


@pytest.mark.parametrize("n", COUNTS)
def test_gather_mixed(host, dev, n):
    lens = _mixed(n)
    plain, _ = _gather_packed(host, dev, lens)
    fused, _ = _gather_packed(host, dev, lens, crc=True)
    assert (plain == fused).all()  # crc on and off leave identical bytes


@pytest.mark.parametrize("n", COUNTS)
def test_scatter_mixed(hbm_src, dev, n):
    lens = _mixed(n)
    plain, _ = _scatter_packed(hbm_src, dev, lens)
    fused, _ = _scatter_packed(hbm_src, dev, lens, crc=True)
    assert (plain == fused).all()


@pytest.mark.parametrize("grid_cap", [1, 2])
def test_runs_that_end_inside_messages(host, hbm_src, dev, grid_cap):
    """4 or 8 waves over some 530 chunks: run boundaries inside the big
    messages and inside the first and last chunk of skewed ones, pending
    shares of different messages in one workgroup."""
    lens = _i64([BIG, 17, 0, 8191, BIG, 4097, 4095, 1])
    # the first message reads at skew 3 and writes at skew 11
    read_at, write_at = _packed(lens, 16 * 5 + 3), _packed(lens, PAD + 11)
    plain, _ = _gather(host, dev, lens, write_at, read_at, grid_cap=grid_cap)
    fused, _ = _gather(host, dev, lens, write_at, read_at, crc=True,
                       grid_cap=grid_cap)
    assert (plain == fused).all()
    size = int(write_at[-1] + lens[-1])
    plain, _ = _scatter(hbm_src, dev, lens, read_at, write_at, size,
                        grid_cap=grid_cap)
    fused, _ = _scatter(hbm_src, dev, lens, read_at, write_at, size,
                        crc=True, grid_cap=grid_cap)
    assert (plain == fused).all()


ZERO_BATCHES = {
    "all_zero": [0] * 5,
    "zero_first_and_last": [0, 4113, 17, 0],
    # the cursor steps over more than a wave's worth of empty messages
    "long_gap": [4113] + [0] * 70 + [47],
}


@pytest.mark.parametrize("name", list(ZERO_BATCHES))
def test_zero_length_messages(host, hbm_src, dev, name):
    lens = ZERO_BATCHES[name]
    for crc in (False, True):
        for grid_cap in (0, 1):
            _, dig = _gather_packed(host, dev, lens, crc=crc,
                                    grid_cap=grid_cap)
            _, dig2 = _scatter_packed(hbm_src, dev, lens, crc=crc,
                                      grid_cap=grid_cap)
            if crc:
                zero = np.asarray(lens) == 0
                assert (dig[zero] == 0).all() and (dig2[zero] == 0).all()


def test_max_msg_bytes_is_only_a_hint(host, hbm_src, dev):
    lens = _mixed(37)
    for fn, buf in ((_gather_packed, host), (_scatter_packed, hbm_src)):
        base, dig = fn(buf, dev, lens, crc=True)
        for hint in (1, 16, 65537):
            got, d = fn(buf, dev, lens, crc=True, max_msg_bytes=hint)
            assert (got == base).all() and (d == dig).all()
            got, _ = fn(buf, dev, lens, max_msg_bytes=hint)
            assert (got == base).all()


def test_aligned_multiples_of_16_equal_the_varlen_engine(host, hbm_src, dev):
    import rocnrdma_amd.ops as ops

    lens = np.random.default_rng(4).choice(
        [0, 16, 48, 1024, 4080, 4096, 4112, 8192, 3 * 4096 + 2048, 65536],
        37).astype(np.int64)
    inside, outside = _packed(lens, 16 * 7, seed=3), _packed(lens, 16 * 5)
    for crc in (False, True):
        new, d_new = _gather(host, dev, lens, inside, outside, crc=crc)
        old, d_old = _gather(host, dev, lens, inside, outside,
                             fn=ops.gather_v_, crc=crc)
        assert (new == old).all()
        assert crc is False or (d_new == d_old).all()
        size = int((outside + lens).max())
        new, d_new = _scatter(hbm_src, dev, lens, inside, outside, size,
                              crc=crc)
        old, d_old = _scatter(hbm_src, dev, lens, inside, outside, size,
                              fn=ops.scatter_v_, crc=crc)
        assert (new == old).all()
        assert crc is False or (d_new == d_old).all()


# -- the landed-bytes digest ------------------------------------------------
@pytest.mark.parametrize("grid_cap", [0, 1])
def test_crc32_messages_bytes(hbm_src, dev, grid_cap):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    src = hbm_src.cpu().numpy()
    # every skew for each length, each message at its own odd offset
    per = [1, 15, 17, 4095, 4097, 0, 33, 8191]
    lens = _i64([ln for ln in per for _ in range(16)])
    offs = _i64([k * 8240 + 16 + (k % 16) for k in range(len(lens))])
    batches = [(lens, offs)]
    for n in COUNTS:  # packed: neighbours share granules
        ml = _mixed(n)
        batches.append((ml, _packed(ml, 16 * 7 + 9, seed=5)))
    big = _i64([BIG, 17, 0, BIG, 4097, 65537])
    batches.append((big, _packed(big, 7)))
    batches.append((_i64([0] * 5), _i64([3] * 5)))
    for lens, offs in batches:
        d_offs = torch.from_numpy(offs).to(dev)
        d_lens = torch.from_numpy(lens).to(dev)
        want = pattern.crc32_messages_v_reference(src, offs, lens)
        # a wrong hint, none, and the exact one
        for hint in (16, 0, int(max(lens.max(), 1))):
            got = ops.crc32_messages_bytes(hbm_src, d_offs, d_lens,
                                           max_msg_bytes=hint,
                                           grid_cap=grid_cap)
            assert got.dtype == torch.int32 and got.shape == (len(lens),)
            assert (_u32(got) == want).all()

    # the last message ends on the tensor's last byte
    lens = _i64([4097, 1, 15])
    offs = _packed(lens, 5)
    buf = hbm_src[:int(offs[-1] + lens[-1])]
    got = ops.crc32_messages_bytes(buf, torch.from_numpy(offs).to(dev),
                                   torch.from_numpy(lens).to(dev),
                                   grid_cap=grid_cap)
    assert (_u32(got) == pattern.crc32_messages_v_reference(
        src[:buf.numel()], offs, lens)).all()


def test_rejects_bad_input(host, dev):
    import rocnrdma_amd.ops as ops

    region = torch.zeros(4096 + 16, dtype=torch.uint8, device=dev)
    offs = torch.full((1,), 3, dtype=torch.int64, device=dev)
    lens = torch.full((1,), 17, dtype=torch.int64, device=dev)
    addrs = torch.full((1,), host.data_ptr() + 5, dtype=torch.int64,
                       device=dev)
    two = torch.cat([lens, lens])
    for fn in (ops.gather_bytes_, ops.scatter_bytes_):
        for crc in (False, True):
            with pytest.raises(RuntimeError, match="int64 on GPU"):
                fn(region, offs, addrs, lens.cpu(), crc=crc)
            with pytest.raises(RuntimeError, match="int64 on GPU"):
                fn(region, offs, addrs, lens.to(torch.int32), crc=crc)
            with pytest.raises(RuntimeError, match="contiguous"):
                fn(region, offs, addrs, torch.cat([two, two])[::2], crc=crc)
            with pytest.raises(RuntimeError, match="n mismatch"):
                fn(region, offs, addrs, two, crc=crc)
            with pytest.raises(RuntimeError, match="n mismatch"):
                fn(region, offs, torch.cat([addrs, addrs]), lens, crc=crc)
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                fn(region[1:], offs, addrs, lens, crc=crc)
            with pytest.raises(RuntimeError, match="grid_cap"):
                fn(region, offs, addrs, lens, crc=crc, grid_cap=-1)
            with pytest.raises(RuntimeError, match="grid_cap"):
                fn(region, offs, addrs, lens, crc=crc, grid_cap=1 << 32)
            with pytest.raises(RuntimeError, match="max_msg_bytes"):
                fn(region, offs, addrs, lens, crc=crc, max_msg_bytes=-1)
            with pytest.raises(RuntimeError, match="on GPU"):
                fn(region.cpu(), offs, addrs, lens, crc=crc)
            none = fn(region, offs[:0], addrs[:0], lens[:0], crc=crc)
            if crc:
                assert none.shape == (0,) and none.dtype == torch.int32
            else:
                assert none is None
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages_bytes(region, offs, lens.cpu())
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages_bytes(region, offs.to(torch.int32), lens)
    with pytest.raises(RuntimeError, match="n mismatch"):
        ops.crc32_messages_bytes(region, offs, two)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.crc32_messages_bytes(region[1:], offs, lens)
    with pytest.raises(RuntimeError, match="grid_cap"):
        ops.crc32_messages_bytes(region, offs, lens, grid_cap=-1)
    with pytest.raises(RuntimeError, match="max_msg_bytes"):
        ops.crc32_messages_bytes(region, offs, lens, max_msg_bytes=-1)
    none = ops.crc32_messages_bytes(region, offs[:0], lens[:0])
    assert none.shape == (0,) and none.dtype == torch.int32


# -- sdma transport ---------------------------------------------------------
REGION = 1 << 20
VICTIM = 3
SKEWS = [(0, 0), (5, 0), (0, 9), (5, 9)]  # (region_skew, staging_skew)


def _open(dev, msg, direction, icrc, skews, region=REGION):
    from rocnrdma_amd.transport import get_transport

    return get_transport("sdma", msg_bytes=msg, region_bytes=region,
                         device=dev, direction=direction, engine="kernel",
                         icrc=icrc, var_len=True, byte_granular=True,
                         region_skew=skews[0], staging_skew=skews[1])


def _payload(seed, region=REGION):
    return np.random.default_rng(seed).integers(0, 256, region,
                                                dtype=np.uint8)


def _slot_lens(n, cap, seed=12):
    lens = np.random.default_rng(seed).integers(0, cap + 1, n,
                                                dtype=np.int64)
    lens[:4] = [0, 1, cap, 37]  # lens[VICTIM] = 37: bytes and slack
    return lens


@pytest.mark.parametrize("skews", SKEWS)
@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_byte_granular_digest_check(dev, direction, icrc, skews):
    msg = 4096
    tp = _open(dev, msg, direction, icrc, skews)
    assert tp.byte_granular and tp.max_nbytes == msg - max(skews)
    n = tp.msgs_per_region
    lens = _slot_lens(n, tp.max_nbytes)
    assert tp.digest_check(_payload(1), lens) == 0
    assert tp.digest_check(_payload(2)) == 0  # the most that fits
    with pytest.raises(NotImplementedError, match="length"):
        tp.stamp()
    if skews == (0, 0):  # whole slots through the byte path
        assert tp.integrity_check(seed=5) == 0
    else:
        with pytest.raises(NotImplementedError, match="skew"):
            tp.integrity_check(seed=5)

    bursts = -(-n // tp.inflight)
    real_flush = tp.flush
    calls = [0]
    slot = tp.staging[VICTIM % tp.inflight]
    rs, ss = skews
    ln = int(lens[VICTIM])

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

    # the last byte of one message flipped: write — in the slot after the
    # sender digested it, before the engine loads it; read — in the slot
    # after it landed
    def flip():
        slot[ss + ln - 1] ^= 1

    wrap(flip, None) if direction == "write" else wrap(None, flip)
    assert tp.digest_check(_payload(3), lens) == 1
    assert calls[0] == bursts

    # one slack byte of the receiver changed after the transfer: right
    # behind the message, and right in front of it
    def poke(at):
        def slack():
            if direction == "write":
                tp.region[VICTIM * msg + at] ^= 0xFF
                torch.cuda.synchronize(dev)
            else:
                slot[at] ^= 0xFF
        return slack

    skew = rs if direction == "write" else ss
    wrap(None, poke(skew + ln))
    assert tp.digest_check(_payload(4), lens) == 1
    if skew:
        wrap(None, poke(skew - 1))
        assert tp.digest_check(_payload(5), lens) == 1
    tp.flush = real_flush
    assert tp.digest_check(_payload(6), lens) == 0
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
@pytest.mark.parametrize("msg", [4096, 65536])
def test_sdma_byte_granular_moves_only_nbytes(dev, msg, direction):
    rs, ss = 5, 9
    tp = _open(dev, msg, direction, False, (rs, ss))
    n = tp.msgs_per_region
    assert tp.inflight == n
    lens = _slot_lens(n, tp.max_nbytes, seed=3)
    rng = np.random.default_rng(8)
    stage = rng.integers(0, 256, n * msg, dtype=np.uint8)
    reg = rng.integers(0, 256, REGION, dtype=np.uint8)
    tp.staging_flat.numpy()[:] = stage
    tp.region.copy_(torch.from_numpy(reg))
    torch.cuda.synchronize(dev)

    # post() and post_many() fill the same ring
    tp.post_many(0, n, lens)
    ring = tp._desc_np[:, :n].copy()
    tp.flush()
    for i in range(n):
        tp.post(i, int(lens[i]))
    assert (tp._desc_np[:, :n] == ring).all()
    tp.flush()

    at = np.arange(msg)[None, :]
    s2, r2 = stage.reshape(n, msg), reg.reshape(n, msg)
    got_s = tp.staging_flat.numpy().reshape(n, msg)
    got_r = tp.region.cpu().numpy().reshape(n, msg)
    if direction == "write":
        moved = (at >= rs) & (at < rs + lens[:, None])
        want = r2.copy()
        for i in range(n):
            want[i, rs:rs + lens[i]] = s2[i, ss:ss + lens[i]]
        assert (got_s == s2).all()
        assert (got_r == want).all()
        assert (got_r[~moved] == r2[~moved]).all()
    else:
        moved = (at >= ss) & (at < ss + lens[:, None])
        want = s2.copy()
        for i in range(n):
            want[i, ss:ss + lens[i]] = r2[i, rs:rs + lens[i]]
        assert (got_r == r2).all()
        assert (got_s == want).all()
        assert (got_s[~moved] == s2[~moved]).all()
    with pytest.raises(ValueError):
        tp.post_many(0, 2, np.array([1, msg - 8]))
    tp.close()


def test_sdma_byte_granular_validation(dev):
    from rocnrdma_amd.transport import get_transport

    kw = dict(msg_bytes=4096, region_bytes=REGION, device=dev,
              engine="kernel")
    with pytest.raises(ValueError, match="var_len"):
        get_transport("sdma", byte_granular=True, **kw)
    with pytest.raises(ValueError, match="byte_granular"):
        get_transport("sdma", var_len=True, region_skew=3, **kw)
    with pytest.raises(ValueError, match="staging_skew"):
        get_transport("sdma", var_len=True, byte_granular=True,
                      staging_skew=16, **kw)
    tp = get_transport("sdma", var_len=True, **kw)
    with pytest.raises(ValueError, match="16"):
        tp.post(0, 17)  # still multiples of 16 without the option
    tp.close()


def test_soak_mixed_bytes(dev):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=2.0, region_bytes=16 << 20, device=dev,
                     mixed=True, byte_granular=True)
    assert stats["cycles"] > 0
    assert stats["failures"] == 0
    assert 0 < stats["bytes"]
