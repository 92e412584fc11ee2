"""GPU tests: the message engine with inline ICRC (ops.gather_crc_ /
scatter_crc_) against zlib and against the plain engine, and the sdma
transport's stamp / icrc_stats / digest_check on top of it."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

MSG_SIZES = [16, 48, 64, 1024, 4080, 4096, 4112, 8192, 3 * 4096 + 2048,
             65536]
COUNTS = [1, 5, 37]
HOST_BASE = 16 * 5    # 16-aligned, not 4096-aligned
REGION_BASE = 16 * 7  # likewise, inside the canary-filled region
CANARY = 0xA5
BIG_MSG = (1 << 20) + 80
HOST_BYTES = 256 + max(37 * 65536, 3 * BIG_MSG)  # covers both bases


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def host():
    """One pinned random buffer, shared and never written by the gather
    cases (scatter cases use their own destination)."""
    t = torch.empty(HOST_BYTES, dtype=torch.uint8, pin_memory=True)
    t.numpy()[:] = np.random.default_rng(77).integers(
        0, 256, HOST_BYTES, dtype=np.uint8)
    return t


@pytest.fixture(scope="module")
def hbm_src(dev, host):
    """The same random bytes in HBM: the scatter cases' region."""
    return host.to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _layout(msg, n, seed):
    """Permuted region offsets and in-order outside offsets."""
    perm = np.random.default_rng(seed).permutation(n).astype(np.int64)
    return REGION_BASE + perm * msg, HOST_BASE + np.arange(
        n, dtype=np.int64) * msg


def _check_gather(host, dev, msg, n, grid_cap=0):
    import rocnrdma_amd.ops as ops

    hnp = host.numpy()
    inside, outside = _layout(msg, n, msg + n)
    size = REGION_BASE + n * msg + 16 * 9
    d_offs = torch.from_numpy(inside).to(dev)
    d_addrs = torch.from_numpy(host.data_ptr() + outside).to(dev)

    region = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    got = ops.gather_crc_(region, d_offs, d_addrs, msg, grid_cap=grid_cap)
    again = ops.gather_crc_(region, d_offs, d_addrs, msg, grid_cap=grid_cap)
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert got.device == region.device

    want = np.full(size, CANARY, dtype=np.uint8)  # canary outside the msgs
    crcs = np.empty(n, dtype=np.uint32)
    for m in range(n):
        src = hnp[outside[m]:outside[m] + msg]
        want[inside[m]:inside[m] + msg] = src
        crcs[m] = zlib.crc32(src.tobytes())
    assert (region.cpu().numpy() == want).all()
    assert (_u32(got) == crcs).all()
    assert torch.equal(got, again)  # no stale accumulator

    plain = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    ops.gather_(plain, d_offs, d_addrs, msg)
    assert torch.equal(plain, region)


def _check_scatter(hbm_src, dev, msg, n, grid_cap=0):
    import rocnrdma_amd.ops as ops

    src = hbm_src.cpu().numpy()
    # the region side: permuted messages of the random HBM tensor; the
    # outside: a canary-filled pinned buffer whose last message ends on
    # the buffer's last byte
    inside, _ = _layout(msg, n, 3 * msg + n)
    size = HOST_BASE + n * msg
    outside = HOST_BASE + np.arange(n, dtype=np.int64) * msg
    d_offs = torch.from_numpy(inside).to(dev)

    def run(engine, **kw):
        dst = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        dst.fill_(CANARY)
        d_addrs = torch.from_numpy(dst.data_ptr() + outside).to(dev)
        out = engine(hbm_src, d_offs, d_addrs, msg, **kw)
        torch.cuda.synchronize(dev)
        return dst, out

    dst, got = run(ops.scatter_crc_, grid_cap=grid_cap)
    _, again = run(ops.scatter_crc_, grid_cap=grid_cap)
    want = np.full(size, CANARY, dtype=np.uint8)
    crcs = np.empty(n, dtype=np.uint32)
    for m in range(n):
        s = src[inside[m]:inside[m] + msg]
        want[outside[m]:outside[m] + msg] = s
        crcs[m] = zlib.crc32(s.tobytes())
    assert (dst.numpy() == want).all()
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert (_u32(got) == crcs).all()
    assert torch.equal(got, again)
    assert (hbm_src.cpu().numpy() == src).all()  # the region is only read

    plain, _ = run(ops.scatter_)
    assert torch.equal(plain, dst)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("msg", MSG_SIZES)
def test_gather_crc(host, dev, msg, n):
    _check_gather(host, dev, msg, n)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("msg", MSG_SIZES)
def test_scatter_crc(hbm_src, dev, msg, n):
    _check_scatter(hbm_src, dev, msg, n)


@pytest.mark.parametrize("grid_cap", [1, 2])
def test_runs_that_end_inside_a_message(host, hbm_src, dev, grid_cap):
    """3 messages of 257 chunks over 4 or 8 waves: every run boundary
    falls inside a message, and the shares meet in the workgroup merge."""
    _check_gather(host, dev, BIG_MSG, 3, grid_cap=grid_cap)
    _check_scatter(hbm_src, dev, BIG_MSG, 3, grid_cap=grid_cap)


def test_engine_rejects_bad_input(host, dev):
    import rocnrdma_amd.ops as ops

    region = torch.zeros(4096, dtype=torch.uint8, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    addrs = torch.full((1,), host.data_ptr(), dtype=torch.int64, device=dev)
    for fn in (ops.gather_crc_, ops.scatter_crc_):
        with pytest.raises(RuntimeError):
            fn(region, offs, addrs, 24)
        with pytest.raises(RuntimeError):
            fn(region, offs, addrs, 0)
        with pytest.raises(RuntimeError, match="int64 on GPU"):
            fn(region, offs.cpu(), addrs, 16)
        with pytest.raises(RuntimeError, match="n mismatch"):
            fn(region, offs, torch.cat([addrs, addrs]), 16)
        none = fn(region, offs[:0], addrs[:0], 16)
        assert none.shape == (0,) and none.dtype == torch.int32


# -- sdma transport --------------------------------------------------------
REGION = 2 << 20
ROUNDS = 3


def _open(dev, msg, direction, **kw):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=msg, region_bytes=REGION,
                       device=dev, direction=direction, engine="kernel",
                       icrc=True, **kw)
    rng = np.random.default_rng(msg)
    tp.staging_flat.numpy()[:] = rng.integers(
        0, 256, tp.staging_flat.numel(), dtype=np.uint8)
    tp.region.copy_(torch.from_numpy(
        rng.integers(0, 256, REGION, dtype=np.uint8)))
    torch.cuda.synchronize(dev)
    return tp


def _post_rounds(tp):
    posted = 0
    for _ in range(ROUNDS):
        tp.post_many(posted, tp.msgs_per_region)
        posted += tp.msgs_per_region
    tp.flush()
    return posted


@pytest.mark.parametrize("direction", ["write", "read"])
@pytest.mark.parametrize("msg", [4096, 65536])
def test_sdma_icrc_clean_corrupt_restamp(dev, msg, direction):
    tp = _open(dev, msg, direction)
    tp.post_many(0, 5)  # before the first stamp: moved, not compared
    tp.post(5)
    tp.flush()
    assert tp.icrc_stats() == {"checked": 0, "bad": 0}

    tp.stamp()
    posted = _post_rounds(tp)
    tp.post(0)  # the scalar path fills the same WQE field
    assert tp.icrc_stats() == {"checked": posted + 1, "bad": 0}

    # one byte of the sender goes bad after the stamp
    if direction == "write":
        tp.staging[3][5] ^= 1
        hits = sum(1 for i in range(posted) if i % tp.inflight == 3)
    else:
        tp.region[3 * msg + 5] ^= 1
        torch.cuda.synchronize(dev)
        hits = sum(1 for i in range(posted) if i % tp.msgs_per_region == 3)
    assert hits > 0
    _post_rounds(tp)
    assert tp.icrc_stats() == {"checked": 2 * posted + 1, "bad": hits}

    tp.stamp()  # accepts the sender as it is now
    _post_rounds(tp)
    assert tp.icrc_stats() == {"checked": 3 * posted + 1, "bad": hits}
    tp.close()


def _payload(seed):
    return np.random.default_rng(seed).integers(0, 256, REGION,
                                                dtype=np.uint8)


@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_icrc_digest_check_clean(dev, direction):
    tp = _open(dev, 65536, direction)
    assert tp.digest_check(_payload(1)) == 0
    # and the bytes did land: the separate HBM-side pass agrees
    if direction == "write":
        import rocnrdma_amd.ops as ops
        from rocnrdma_amd.utils import pattern

        assert (_u32(ops.crc32_messages(tp.region, 65536)) ==
                pattern.crc32_messages_reference(_payload(1), 65536)).all()
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_icrc_digest_check_counts_one_corrupt_message(dev, direction):
    """One byte flipped from a wrapped flush(), as for the plain
    digest_check.  read: in the staging slot after the final flush, seen
    by the host-side zlib.  write: in the staging slot just before the
    final flush moves it — after the sender digested it; the inline
    digest is of the bytes as loaded, so this is the corruption it can
    see (bytes changed in HBM after landing are crc32_messages' to
    find)."""
    msg = 65536
    tp = _open(dev, msg, direction)
    bursts = -(-tp.msgs_per_region // tp.inflight)
    real_flush = tp.flush
    calls = [0]

    def flush():
        last = calls[0] + 1 == bursts
        if last and direction == "write":
            tp.staging[3 % tp.inflight][5] ^= 1
        real_flush()
        calls[0] += 1
        if last and direction == "read":
            tp.staging[3 % tp.inflight][5] ^= 1

    tp.flush = flush
    assert tp.digest_check(_payload(2)) == 1
    assert calls[0] == bursts
    tp.flush = real_flush
    tp.close()


@pytest.mark.parametrize("engine,msg", [("stream", 65536), ("auto", 8 << 20)])
def test_icrc_needs_the_kernel_engine(dev, engine, msg):
    from rocnrdma_amd.transport import get_transport

    with pytest.raises(ValueError, match="kernel engine"):
        get_transport("sdma", msg_bytes=msg, region_bytes=16 << 20,
                      device=dev, engine=engine, icrc=True)


def test_soak_icrc(dev):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=2.0, region_bytes=16 << 20, device=dev,
                     icrc=True)
    assert stats["cycles"] > 0
    assert stats["failures"] == 0
    assert stats["icrc_checked"] > 0 and stats["icrc_bad"] == 0
