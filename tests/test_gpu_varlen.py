"""GPU tests: per-message lengths in the message engine (ops.gather_v_ /
scatter_v_, with and without the inline ICRC) and in the landed-bytes
digest (ops.crc32_messages_v), against a numpy model, zlib and the
uniform engines; and var_len=True on the sdma transport and the soak."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

LEN_SET = [0, 16, 48, 64, 1024, 4080, 4096, 4112, 8192, 3 * 4096 + 2048,
           65536]
COUNTS = [1, 5, 37]
HOST_BASE = 16 * 5    # 16-aligned, not 4096-aligned
REGION_BASE = 16 * 7  # likewise, inside the canary-filled region
CANARY = 0xA5
BIG = (1 << 20) + 80
HOST_BYTES = 6 << 20  # covers every batch below from HOST_BASE


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def host():
    """One pinned random buffer, shared and never written."""
    t = torch.empty(HOST_BYTES, dtype=torch.uint8, pin_memory=True)
    t.numpy()[:] = np.random.default_rng(78).integers(
        0, 256, HOST_BYTES, dtype=np.uint8)
    return t


@pytest.fixture(scope="module")
def hbm_src(dev, host):
    """The same random bytes in HBM: the scatter cases' region."""
    return host.to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _mixed(n, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    return rng.choice(LEN_SET, n).astype(np.int64)


def _layout(lens, seed):
    """Messages packed back to back on both sides: in a permuted order
    inside the region, in order outside."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    perm = np.random.default_rng(seed).permutation(n)
    inside = np.empty(n, dtype=np.int64)
    inside[perm] = REGION_BASE + np.cumsum(lens[perm]) - lens[perm]
    outside = HOST_BASE + np.cumsum(lens) - lens
    assert HOST_BASE + int(lens.sum()) <= HOST_BYTES
    return lens, inside, outside


def _gather(host, dev, lens, seed=1, **kw):
    """gather_v_ into a canary-filled region, twice; checks bytes,
    canaries and (crc=True) digests against numpy and zlib.  Returns
    (region bytes, digests or None)."""
    import rocnrdma_amd.ops as ops

    hnp = host.numpy()
    lens, inside, outside = _layout(lens, seed)
    n, size = len(lens), REGION_BASE + int(lens.sum()) + 16 * 9
    d_offs = torch.from_numpy(inside).to(dev)
    d_addrs = torch.from_numpy(host.data_ptr() + outside).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)

    region = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    got = ops.gather_v_(region, d_offs, d_addrs, d_lens, **kw)
    first = region.clone()
    again = ops.gather_v_(region, d_offs, d_addrs, d_lens, **kw)

    want = np.full(size, CANARY, dtype=np.uint8)  # canary outside the msgs
    crcs = np.empty(n, dtype=np.uint32)
    for m in range(n):
        src = hnp[outside[m]:outside[m] + lens[m]]
        want[inside[m]:inside[m] + lens[m]] = src
        crcs[m] = zlib.crc32(src.tobytes())
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


def _scatter(hbm_src, dev, lens, seed=2, **kw):
    """scatter_v_ from the random HBM tensor into a canary-filled pinned
    buffer whose last message ends on the buffer's last byte."""
    import rocnrdma_amd.ops as ops

    src = hbm_src.cpu().numpy()
    lens, inside, outside = _layout(lens, seed)
    n, size = len(lens), HOST_BASE + int(lens.sum())
    d_offs = torch.from_numpy(inside).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)

    def run():
        dst = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        dst.fill_(CANARY)
        d_addrs = torch.from_numpy(dst.data_ptr() + outside).to(dev)
        out = ops.scatter_v_(hbm_src, d_offs, d_addrs, d_lens, **kw)
        torch.cuda.synchronize(dev)
        return dst.numpy().copy(), out

    dst, got = run()
    dst2, again = run()
    want = np.full(size, CANARY, dtype=np.uint8)
    crcs = np.empty(n, dtype=np.uint32)
    for m in range(n):
        s = src[inside[m]:inside[m] + lens[m]]
        want[outside[m]:outside[m] + lens[m]] = s
        crcs[m] = zlib.crc32(s.tobytes())
    assert (dst == want).all() and (dst2 == want).all()
    assert (hbm_src.cpu().numpy() == src).all()  # the region is only read
    if kw.get("crc"):
        assert got.dtype == torch.int32 and got.shape == (n,)
        assert (_u32(got) == crcs).all()
        assert torch.equal(got, again)
        return want, _u32(got)
    assert got is None and again is None
    return want, None


# -- the engine -------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_gather_mixed(host, dev, n):
    lens = _mixed(n)
    plain, _ = _gather(host, dev, lens)
    fused, _ = _gather(host, dev, lens, crc=True)
    assert (plain == fused).all()  # crc on and off leave identical bytes


@pytest.mark.parametrize("n", COUNTS)
def test_scatter_mixed(hbm_src, dev, n):
    lens = _mixed(n)
    plain, _ = _scatter(hbm_src, dev, lens)
    fused, _ = _scatter(hbm_src, dev, lens, crc=True)
    assert (plain == fused).all()


@pytest.mark.parametrize("msg", [16, 4096, 4112])
def test_uniform_lengths_equal_the_uniform_engines(host, hbm_src, dev, msg):
    import rocnrdma_amd.ops as ops

    n = 37
    lens, inside, outside = _layout(np.full(n, msg), msg)
    d_offs = torch.from_numpy(inside).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)
    size = REGION_BASE + n * msg + 16 * 9

    # gather
    d_addrs = torch.from_numpy(host.data_ptr() + outside).to(dev)

    def fresh():
        return torch.full((size,), CANARY, dtype=torch.uint8, device=dev)

    r_old, r_new, r_oldp, r_newp = fresh(), fresh(), fresh(), fresh()
    old = ops.gather_crc_(r_old, d_offs, d_addrs, msg)
    new = ops.gather_v_(r_new, d_offs, d_addrs, d_lens, crc=True)
    ops.gather_(r_oldp, d_offs, d_addrs, msg)
    assert ops.gather_v_(r_newp, d_offs, d_addrs, d_lens) is None
    assert torch.equal(old, new)
    assert torch.equal(r_old, r_new) and torch.equal(r_oldp, r_newp)
    assert torch.equal(r_old, r_oldp)

    # scatter
    hsize = HOST_BASE + n * msg

    def run(fn):
        dst = torch.empty(hsize, dtype=torch.uint8, pin_memory=True)
        dst.fill_(CANARY)
        addrs = torch.from_numpy(dst.data_ptr() + outside).to(dev)
        out = fn(addrs)
        torch.cuda.synchronize(dev)
        return dst, out

    d_old, old = run(lambda a: ops.scatter_crc_(hbm_src, d_offs, a, msg))
    d_new, new = run(lambda a: ops.scatter_v_(hbm_src, d_offs, a, d_lens,
                                              crc=True))
    d_oldp, _ = run(lambda a: ops.scatter_(hbm_src, d_offs, a, msg))
    d_newp, _ = run(lambda a: ops.scatter_v_(hbm_src, d_offs, a, d_lens))
    assert torch.equal(old, new)
    assert torch.equal(d_old, d_new) and torch.equal(d_oldp, d_newp)
    assert torch.equal(d_old, d_oldp)


ZERO_BATCHES = {
    "all_zero": [0] * 5,
    "zero_first_and_last": [0, 4112, 16, 0],
    # the cursor steps over more than a wave's worth of empty messages
    "long_gap": [4112] + [0] * 70 + [48],
}


@pytest.mark.parametrize("name", list(ZERO_BATCHES))
def test_zero_length_messages(host, hbm_src, dev, name):
    lens = ZERO_BATCHES[name]
    for crc in (False, True):
        for grid_cap in (0, 1):
            _, dig = _gather(host, dev, lens, crc=crc, grid_cap=grid_cap)
            _, dig2 = _scatter(hbm_src, dev, lens, crc=crc,
                               grid_cap=grid_cap)
            if crc:
                zero = np.asarray(lens) == 0
                assert (dig[zero] == 0).all() and (dig2[zero] == 0).all()


@pytest.mark.parametrize("grid_cap", [1, 2])
def test_runs_that_end_inside_messages(host, hbm_src, dev, grid_cap):
    """4 or 8 waves over 3 x 257 + 2 chunks: run boundaries inside the
    big messages, pending shares of different messages in one workgroup,
    tiny messages sharing a run."""
    lens = [BIG, 16, 0, BIG, 4096, BIG]
    plain, _ = _gather(host, dev, lens, grid_cap=grid_cap)
    fused, _ = _gather(host, dev, lens, crc=True, grid_cap=grid_cap)
    assert (plain == fused).all()
    plain, _ = _scatter(hbm_src, dev, lens, grid_cap=grid_cap)
    fused, _ = _scatter(hbm_src, dev, lens, crc=True, grid_cap=grid_cap)
    assert (plain == fused).all()


def test_scan_wider_than_its_workgroup(host, dev):
    lens = np.tile([16, 0, 32, 4112], 1250)  # n = 5000
    _gather(host, dev, lens, crc=True)
    _gather(host, dev, lens)


def test_max_msg_bytes_is_only_a_hint(host, hbm_src, dev):
    lens = _mixed(37)
    for fn, buf in ((_gather, host), (_scatter, hbm_src)):
        base, dig = fn(buf, dev, lens, crc=True)
        for hint in (16, 65536):
            got, d = fn(buf, dev, lens, crc=True, max_msg_bytes=hint)
            assert (got == base).all() and (d == dig).all()
            got, _ = fn(buf, dev, lens, max_msg_bytes=hint)
            assert (got == base).all()


# -- the landed-bytes digest ------------------------------------------------
@pytest.mark.parametrize("grid_cap", [0, 1])
def test_crc32_messages_v(hbm_src, dev, grid_cap):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    src = hbm_src.cpu().numpy()
    batches = [_mixed(37), _mixed(5), _mixed(1),
               [BIG, 16, 0, BIG, 4096, BIG], [0] * 5,
               [4112] + [0] * 70 + [48]]
    for lens in batches:
        lens, inside, _ = _layout(lens, 5)
        d_offs = torch.from_numpy(inside).to(dev)
        d_lens = torch.from_numpy(lens).to(dev)
        want = pattern.crc32_messages_v_reference(src, inside, lens)
        for hint in (0, 16, int(max(lens.max(), 16))):
            got = ops.crc32_messages_v(hbm_src, d_offs, d_lens,
                                       max_msg_bytes=hint,
                                       grid_cap=grid_cap)
            assert got.dtype == torch.int32 and got.shape == (len(lens),)
            assert (_u32(got) == want).all()

    # odd byte lengths at 16-aligned offsets, the last message ending on
    # the tensor's last byte
    lens = np.array([1, 15, 17, 4095, 4097, 0, 4097, 17], dtype=np.int64)
    offs = np.cumsum((lens + 15) // 16 * 16) - (lens + 15) // 16 * 16 + 48
    buf = hbm_src[:int(offs[-1] + lens[-1])]
    want = pattern.crc32_messages_v_reference(src[:buf.numel()], offs, lens)
    got = ops.crc32_messages_v(buf, torch.from_numpy(offs).to(dev),
                               torch.from_numpy(lens).to(dev),
                               grid_cap=grid_cap)
    assert (_u32(got) == want).all()


def test_scan_wider_than_its_workgroup_digest(hbm_src, dev):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    lens, inside, _ = _layout(np.tile([16, 0, 32, 4112], 1250), 6)
    got = ops.crc32_messages_v(hbm_src, torch.from_numpy(inside).to(dev),
                               torch.from_numpy(lens).to(dev))
    assert (_u32(got) == pattern.crc32_messages_v_reference(
        hbm_src.cpu().numpy(), inside, lens)).all()


def test_rejects_bad_input(host, dev):
    import rocnrdma_amd.ops as ops

    region = torch.zeros(4096 + 16, dtype=torch.uint8, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    lens = torch.full((1,), 16, dtype=torch.int64, device=dev)
    addrs = torch.full((1,), host.data_ptr(), dtype=torch.int64, device=dev)
    two = torch.cat([lens, lens])
    for fn in (ops.gather_v_, ops.scatter_v_):
        for crc in (False, True):
            with pytest.raises(RuntimeError, match="int64 on GPU"):
                fn(region, offs, addrs, lens.cpu(), crc=crc)
            with pytest.raises(RuntimeError, match="int64 on GPU"):
                fn(region, offs, addrs, lens.to(torch.int32), crc=crc)
            with pytest.raises(RuntimeError, match="n mismatch"):
                fn(region, offs, addrs, two, crc=crc)
            with pytest.raises(RuntimeError, match="n mismatch"):
                fn(region, offs, torch.cat([addrs, addrs]), lens, crc=crc)
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                fn(region[1:], offs, addrs, lens, crc=crc)
            with pytest.raises(RuntimeError, match="grid_cap"):
                fn(region, offs, addrs, lens, crc=crc, grid_cap=-1)
            none = fn(region, offs[:0], addrs[:0], lens[:0], crc=crc)
            if crc:
                assert none.shape == (0,) and none.dtype == torch.int32
            else:
                assert none is None
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages_v(region, offs, lens.cpu())
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages_v(region, offs.to(torch.int32), lens)
    with pytest.raises(RuntimeError, match="n mismatch"):
        ops.crc32_messages_v(region, offs, two)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.crc32_messages_v(region[1:], offs, lens)
    none = ops.crc32_messages_v(region, offs[:0], lens[:0])
    assert none.shape == (0,) and none.dtype == torch.int32


# -- sdma transport ---------------------------------------------------------
REGION = 2 << 20
VICTIM = 3


def _open(dev, msg, direction, icrc):
    from rocnrdma_amd.transport import get_transport

    return get_transport("sdma", msg_bytes=msg, region_bytes=REGION,
                         device=dev, direction=direction, engine="kernel",
                         icrc=icrc, var_len=True)


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


def _slot_lens(n, msg, seed=12):
    rng = np.random.default_rng(seed)
    pool = [v for v in (0, 16, 48, 4080, 4096, 4112, msg - 16, msg)
            if v <= msg]
    lens = rng.choice(pool, n).astype(np.int64)
    lens[:4] = [0, 16, msg, 48]  # lens[VICTIM] = 48: bytes and slack
    return lens


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
@pytest.mark.parametrize("msg", [4096, 65536])
def test_sdma_var_len_digest_check(dev, msg, direction, icrc):
    tp = _open(dev, msg, direction, icrc)
    assert tp.var_len
    n = tp.msgs_per_region
    lens = _slot_lens(n, msg)
    assert tp.digest_check(_payload(1), lens) == 0
    assert tp.digest_check(_payload(2)) == 0  # full slots
    if direction == "write":
        # only the first lens[j] bytes landed, and they are the payload's
        got = tp.region.cpu().numpy().reshape(n, msg)
        pay = _payload(2).reshape(n, msg)
        assert (got == pay).all()
    with pytest.raises(NotImplementedError, match="length"):
        tp.stamp()
    assert tp.integrity_check(seed=5) == 0

    bursts = -(-n // tp.inflight)
    real_flush = tp.flush
    calls = [0]
    slot = tp.staging[VICTIM % tp.inflight]

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

    # one byte of one message flipped: write — in the slot after the
    # sender digested it, before the engine loads it; read — in the slot
    # after it landed
    def flip():
        slot[5] ^= 1

    wrap(flip, None) if direction == "write" else wrap(None, flip)
    assert tp.digest_check(_payload(3), lens) == 1
    assert calls[0] == bursts

    # one slack byte of the receiver changed after the transfer
    def slack():
        at = int(lens[VICTIM]) + 7
        if direction == "write":
            tp.region[VICTIM * msg + at] ^= 0xFF
            torch.cuda.synchronize(dev)
        else:
            slot[at] ^= 0xFF

    wrap(None, slack)
    assert tp.digest_check(_payload(4), lens) == 1
    tp.flush = real_flush
    assert tp.digest_check(_payload(5), lens) == 0
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_var_len_moves_only_nbytes(dev, direction):
    msg = 4096
    tp = _open(dev, msg, direction, False)
    n = tp.msgs_per_region
    assert tp.inflight == n
    lens = _slot_lens(n, msg, seed=3)
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

    keep = np.arange(msg)[None, :] >= lens[:, None]  # the slack
    s2, r2 = stage.reshape(n, msg), reg.reshape(n, msg)
    got_s = tp.staging_flat.numpy().reshape(n, msg)
    got_r = tp.region.cpu().numpy().reshape(n, msg)
    if direction == "write":
        assert (got_s == s2).all()
        assert (got_r == np.where(keep, r2, s2)).all()
    else:
        assert (got_r == r2).all()
        assert (got_s == np.where(keep, s2, r2)).all()
    with pytest.raises(ValueError):
        tp.post_many(0, 2, np.array([16, msg + 16]))
    tp.close()


@pytest.mark.parametrize("engine,msg", [("stream", 65536), ("auto", 8 << 20)])
def test_var_len_needs_the_kernel_engine(dev, engine, msg):
    from rocnrdma_amd.transport import get_transport

    with pytest.raises(ValueError, match="kernel engine"):
        get_transport("sdma", msg_bytes=msg, region_bytes=16 << 20,
                      device=dev, engine=engine, var_len=True)


def test_sdma_nbytes_needs_var_len(dev):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=4096, region_bytes=REGION,
                       device=dev, engine="kernel")
    with pytest.raises(ValueError, match="var_len"):
        tp.post(0, 16)
    with pytest.raises(ValueError, match="var_len"):
        tp.post_many(0, 2, 16)
    tp.close()


def test_soak_mixed(dev):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=2.0, region_bytes=16 << 20, device=dev,
                     mixed=True)
    assert stats["cycles"] > 0
    assert stats["failures"] == 0
    assert 0 < stats["bytes"]
