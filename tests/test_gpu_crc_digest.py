"""GPU tests: on-GPU CRC32 digests per message and per region against
zlib on host bytes, and the sdma transport's digest_check."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

PAGE = 4096
REGION_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097,
                  5 * PAGE + 16, 17 * PAGE + 1000]
MSG_SIZES = [16, 64, PAGE, PAGE + 16, 2 * PAGE, 3 * PAGE + 2048, 65536]
COUNTS = [1, 5, 37]
SCATTER_BASE = 16 * 7  # 16-aligned, not 4096-aligned


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def big(dev):
    """One random HBM tensor and its host copy, shared and never written:
    every case digests a slice of it, so a load past a slice's end reads
    other random bytes and changes the answer."""
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    t = torch.randint(0, 256, (SCATTER_BASE + 37 * 65536 + 64,),
                      dtype=torch.uint8, device=dev, generator=g)
    return t, t.cpu().numpy()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("length", REGION_LENGTHS)
def test_crc32_region_matches_zlib(big, length):
    import rocnrdma_amd.ops as ops

    t, host = big
    got = ops.crc32(t[16:16 + length])
    assert got == zlib.crc32(host[16:16 + length].tobytes())


def test_crc32_region_rejects_bad_input(big):
    import rocnrdma_amd.ops as ops

    t, host = big
    with pytest.raises(RuntimeError, match="aligned"):
        ops.crc32(t[8:8 + 4096])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.crc32(t[0:8192:2])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.crc32(torch.from_numpy(host[:4096].copy()))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("msg", MSG_SIZES)
def test_crc32_messages_contiguous(big, msg, n):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    t, host = big
    got = ops.crc32_messages(t[16:16 + n * msg], msg)
    again = ops.crc32_messages(t[16:16 + n * msg], msg)
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert got.device == t.device
    ref = pattern.crc32_messages_reference(host[16:16 + n * msg], msg)
    assert (_u32(got) == ref).all()
    assert torch.equal(got, again)  # no stale accumulator


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("msg", MSG_SIZES)
def test_crc32_messages_scattered(big, msg, n):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    t, host = big
    perm = np.random.default_rng(msg + n).permutation(n)
    offs = SCATTER_BASE + perm.astype(np.int64) * msg
    d_offs = torch.from_numpy(offs).to(t.device)
    got = ops.crc32_messages(t, msg, d_offs)
    again = ops.crc32_messages(t, msg, d_offs)
    ref = pattern.crc32_messages_reference(host, msg, offs)
    assert (_u32(got) == ref).all()
    assert torch.equal(got, again)


def test_crc32_messages_edge_inputs(big):
    import rocnrdma_amd.ops as ops

    t, _ = big
    empty = ops.crc32_messages(t[16:16], 4096)
    assert empty.shape == (0,) and empty.dtype == torch.int32
    none = ops.crc32_messages(
        t, 4096, torch.empty(0, dtype=torch.int64, device=t.device))
    assert none.shape == (0,)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.crc32_messages(t[16:16 + 4 * 24], 24)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.crc32_messages(t[16:16 + 4096], 0)
    with pytest.raises(RuntimeError, match="multiple of msg_bytes"):
        ops.crc32_messages(t[16:16 + 4096 + 16], 4096)
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages(t, 4096, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int64 on GPU"):
        ops.crc32_messages(
            t, 4096, torch.zeros(2, dtype=torch.int32, device=t.device))
    with pytest.raises(RuntimeError, match="aligned"):
        ops.crc32_messages(t[8:8 + 4096], 4096)


@pytest.mark.parametrize("grid_cap", [1, 3])
def test_grid_cap_multi_chunk_runs(big, grid_cap):
    """A capped grid makes every wave walk a run of several chunks that
    crosses message boundaries — the path the default grid only takes on
    inputs of tens of MiB."""
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    t, host = big
    length = 17 * PAGE + 1000
    assert ops.crc32(t[16:16 + length], grid_cap=grid_cap) == zlib.crc32(
        host[16:16 + length].tobytes())

    msg, n = 3 * PAGE + 2048, 37
    perm = np.random.default_rng(grid_cap).permutation(n)
    offs = SCATTER_BASE + perm.astype(np.int64) * msg
    got = ops.crc32_messages(t, msg, torch.from_numpy(offs).to(t.device),
                             grid_cap=grid_cap)
    assert (_u32(got) == pattern.crc32_messages_reference(
        host, msg, offs)).all()
    got = ops.crc32_messages(t[16:16 + n * msg], msg, grid_cap=grid_cap)
    assert (_u32(got) == pattern.crc32_messages_reference(
        host[16:16 + n * msg], msg)).all()
    # 16-chunk messages: run lengths that do not divide the message
    msg = 65536
    got = ops.crc32_messages(t[16:16 + n * msg], msg, grid_cap=grid_cap)
    assert (_u32(got) == pattern.crc32_messages_reference(
        host[16:16 + n * msg], msg)).all()


def test_crc32_messages_agrees_with_page_kernel(big):
    import rocnrdma_amd.ops as ops

    t, _ = big
    buf = t[4096:4096 + 257 * PAGE]
    assert torch.equal(ops.crc32_messages(buf, PAGE), ops.crc32_pages(buf))


# -- sdma transport --------------------------------------------------------
def _payload(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes,
                                                dtype=np.uint8)


@pytest.mark.parametrize("engine", ["kernel", "stream"])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_digest_check_clean(dev, direction, engine):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=65536, region_bytes=1 << 20,
                       device=dev, direction=direction, engine=engine)
    assert tp.digest_check(_payload(1 << 20, 1)) == 0
    tp.close()


@pytest.mark.parametrize("engine", ["kernel", "stream"])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_digest_check_counts_one_corrupt_message(dev, direction,
                                                      engine):
    from rocnrdma_amd.transport import get_transport

    msg = 65536
    tp = get_transport("sdma", msg_bytes=msg, region_bytes=1 << 20,
                       device=dev, direction=direction, engine=engine)
    bursts = -(-tp.msgs_per_region // tp.inflight)
    real_flush = tp.flush
    calls = [0]

    def flush():
        real_flush()
        calls[0] += 1
        if calls[0] == bursts:  # after the final flush of the transfer
            if direction == "write":
                tp.region[3 * msg + 5] ^= 1
            else:
                tp.staging[3 % tp.inflight][5] ^= 1

    tp.flush = flush
    assert tp.digest_check(_payload(1 << 20, 2)) == 1
    assert calls[0] == bursts
    tp.flush = real_flush
    tp.close()


def test_sdma_digest_check_4kb_messages(dev):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=4096, region_bytes=1 << 20,
                       device=dev, engine="kernel")
    assert tp.digest_check(_payload(1 << 20, 3)) == 0
    tp.close()


def test_soak_crc_audit(dev):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=2.0, region_bytes=16 << 20, audit="crc",
                     device=dev)
    assert stats["cycles"] > 0
    assert stats["failures"] == 0
