"""GPU numerics tests: hand-written gfx950 kernels vs CPU references
(numpy splitmix64, zlib CRC32)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def test_extension_is_native(dev):
    import rocnrdma_amd.ops as ops

    # on a GPU box the native extension must be present — no fallback
    assert ops.have_ext()
    assert "_p2p_ext" in str(ops._p2p_ext.__file__)


@pytest.mark.parametrize("nbytes", [4096, 1 << 20, (1 << 22) + 8])
def test_fill_matches_reference(dev, nbytes):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed=321)
    got = buf.cpu().numpy()
    ref = pattern.fill_reference(nbytes, 321)
    assert (got == ref).all()


# -- the wave-tile split shared by fill / verify / copy --------------------
# fill works in tiles of 8 KiB per wave, verify and copy in tiles of
# 4 KiB; what is left after the last whole tile goes one 16-byte vector
# per thread, and fill/verify end with an odd 8-byte word.
GUARD = 64


@pytest.mark.parametrize("nbytes", [8, 16, 24, 8184, 8192, 8216])
def test_fill_tails(dev, nbytes):
    """No vector at all, the odd word alone, and one tile -/+ a tail."""
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8,
                     device=dev)
    ops.fill_(buf[GUARD:GUARD + nbytes], seed=77)
    got = buf.cpu().numpy()
    assert (got[GUARD:GUARD + nbytes] == pattern.fill_reference(nbytes, 77)).all()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + nbytes:] == 0xA5).all()


def test_verify_tail_word(dev):
    import rocnrdma_amd.ops as ops

    buf = torch.empty(8216, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed=78)
    assert ops.verify(buf, seed=78) == 0
    buf[8216 - 3] ^= 0x10  # one bit of the odd last word
    assert ops.verify(buf, seed=78) == 1


@pytest.fixture(scope="module")
def noise(dev):
    """256 MiB + 8 KiB of random bytes, shared and never written."""
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    return torch.randint(0, 256, ((256 << 20) + 8192,), dtype=torch.uint8,
                         device=dev, generator=g)


@pytest.mark.parametrize("op", ["copy_", "copy_nt_"])
@pytest.mark.parametrize("nbytes", [16, 4080, 4096, 4112])
def test_copy_tails(dev, noise, op, nbytes):
    import rocnrdma_amd.ops as ops

    src = noise[4096 + 48:4096 + 48 + nbytes]
    buf = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8,
                     device=dev)
    getattr(ops, op)(buf[GUARD:GUARD + nbytes], src)
    torch.cuda.synchronize()
    assert torch.equal(buf[GUARD:GUARD + nbytes], src)
    assert (buf[:GUARD] == 0x5A).all() and (buf[GUARD + nbytes:] == 0x5A).all()


# Past 256 MiB the grid caps are reached and a wave takes a second tile:
# the only size at which the tile stride loop iterates.
STRIDE_FILL = (256 << 20) + 8216
STRIDE_COPY = (256 << 20) + 4112


def test_fill_verify_stride_loop(dev):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    buf = torch.empty(STRIDE_FILL, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed=9)
    ref = torch.from_numpy(pattern.fill_reference(STRIDE_FILL, 9)).to(dev)
    assert torch.equal(buf, ref)
    assert ops.verify(buf, seed=9) == 0
    buf[STRIDE_FILL - 5000] ^= 0x04  # in the second tile of wave 0
    assert ops.verify(buf, seed=9) == 1


@pytest.mark.parametrize("op", ["copy_", "copy_nt_"])
def test_copy_stride_loop(dev, noise, op):
    import rocnrdma_amd.ops as ops

    src = noise[:STRIDE_COPY]
    dst = torch.zeros_like(src)
    getattr(ops, op)(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_verify_counts_corruption(dev):
    import rocnrdma_amd.ops as ops

    buf = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed=11)
    assert ops.verify(buf, seed=11) == 0
    assert ops.verify(buf, seed=12) > 0
    buf[777] ^= 0x01  # flip one bit -> exactly one bad word
    assert ops.verify(buf, seed=11) == 1


def test_crc32_matches_zlib_on_random_data(dev):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    npages = 257  # odd count: exercises grid-stride tail
    data = torch.randint(0, 256, (npages * 4096,), dtype=torch.uint8,
                         device=dev)
    crcs = ops.crc32_pages(data).cpu().numpy().view(np.uint32)
    ref = pattern.crc32_pages_reference(data.cpu().numpy())
    assert (crcs == ref).all()


def test_crc32_large(dev):
    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    nbytes = 64 << 20
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ops.fill_(buf, seed=5)
    crcs = ops.crc32_pages(buf).cpu().numpy().view(np.uint32)
    ref = pattern.crc32_pages_reference(pattern.fill_reference(nbytes, 5))
    assert (crcs == ref).all()


def test_copy_kernel(dev):
    import rocnrdma_amd.ops as ops

    src = torch.randint(0, 256, (8 << 20,), dtype=torch.uint8, device=dev)
    dst = torch.zeros_like(src)
    ops.copy_(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_copy_nt_kernel(dev):
    import rocnrdma_amd.ops as ops

    src = torch.randint(0, 256, (8 << 20,), dtype=torch.uint8, device=dev)
    dst = torch.zeros_like(src)
    ops.copy_nt_(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


@pytest.mark.parametrize("engine", ["stream", "kernel"])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_transport_integrity(dev, direction, engine):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=1 << 20, region_bytes=32 << 20,
                       device=dev, direction=direction, engine=engine)
    assert tp.integrity_check(seed=1234) == 0
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_transport_4kb_messages(dev, direction):
    from rocnrdma_amd.transport import get_transport

    tp = get_transport("sdma", msg_bytes=4096, region_bytes=1 << 20,
                       device=dev, direction=direction)
    assert tp.engine == "kernel"
    assert tp.inflight == 256  # full region fits the WQE ring
    assert tp.integrity_check(seed=77) == 0
    tp.close()


# 48 B = 3 vectors per message: not a power of two, so the kernel
# divides instead of shifting
@pytest.mark.parametrize("msg", [48, 8192])
def test_gather_kernel_matches_reference(dev, msg):
    """Direct gather_ use: scattered host-pinned slots -> chosen HBM
    offsets, compared against a CPU-composed reference."""
    import rocnrdma_amd.ops as ops

    n = 37
    staging = torch.randint(0, 256, (n * msg,), dtype=torch.uint8,
                            pin_memory=True)
    region = torch.zeros(n * msg, dtype=torch.uint8, device=dev)
    perm = torch.randperm(n)
    dst_offs = (perm * msg).to(dtype=torch.int64, device=dev)
    src_addrs = torch.tensor(
        [staging.data_ptr() + i * msg for i in range(n)],
        dtype=torch.int64, device=dev)
    ops.gather_(region, dst_offs, src_addrs, msg)
    torch.cuda.synchronize()
    got = region.cpu()
    for i in range(n):
        off = int(perm[i]) * msg
        assert torch.equal(got[off:off + msg], staging[i * msg:(i + 1) * msg])


@pytest.mark.parametrize("msg", [48, 8192])
def test_scatter_kernel_matches_reference(dev, msg):
    """Direct scatter_ use: chosen HBM offsets -> host-pinned slots."""
    import rocnrdma_amd.ops as ops

    n = 37
    region = torch.randint(0, 256, (n * msg,), dtype=torch.uint8, device=dev)
    staging = torch.zeros(n * msg, dtype=torch.uint8, pin_memory=True)
    perm = torch.randperm(n)
    src_offs = (perm * msg).to(dtype=torch.int64, device=dev)
    dst_addrs = torch.tensor(
        [staging.data_ptr() + i * msg for i in range(n)],
        dtype=torch.int64, device=dev)
    ops.scatter_(region, src_offs, dst_addrs, msg)
    torch.cuda.synchronize()
    want = region.cpu()
    for i in range(n):
        off = int(perm[i]) * msg
        assert torch.equal(staging[i * msg:(i + 1) * msg], want[off:off + msg])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_kernels_run_on_the_tensors_device():
    """Tensors on cuda:1 while cuda:0 is current, after cuda:0 has already
    run a CRC kernel: launch, tables and outputs follow the tensor."""
    import zlib

    import rocnrdma_amd.ops as ops
    from rocnrdma_amd.utils import pattern

    d0, d1 = torch.device("cuda", 0), torch.device("cuda", 1)
    torch.cuda.set_device(d0)
    first = torch.randint(0, 256, (4 * 4096,), dtype=torch.uint8, device=d0)
    assert (ops.crc32_pages(first).cpu().numpy().view(np.uint32) ==
            pattern.crc32_pages_reference(first.cpu().numpy())).all()

    buf = torch.empty(1 << 20, dtype=torch.uint8, device=d1)
    ops.fill_(buf, seed=21)
    assert (buf.cpu().numpy() == pattern.fill_reference(1 << 20, 21)).all()
    assert ops.verify(buf, seed=21) == 0

    data = torch.randint(0, 256, (257 * 4096,), dtype=torch.uint8, device=d1)
    host = data.cpu().numpy()
    crcs = ops.crc32_pages(data)
    assert crcs.device == d1
    assert (crcs.cpu().numpy().view(np.uint32) ==
            pattern.crc32_pages_reference(host)).all()
    n = 17 * 4096 + 1000
    assert ops.crc32(data[:n]) == zlib.crc32(host[:n].tobytes())
    assert torch.cuda.current_device() == 0


def test_smoke_entry():
    import __graft_entry__ as ge

    ge.smoke()


def test_dmabuf_export(dev):
    """The kernel-module-free MR path's GPU half: an HBM range exports
    as a dmabuf fd (what ibv_reg_dmabuf_mr consumes on HCA hosts)."""
    import os

    import rocnrdma_amd.ops as ops

    buf = torch.empty(8 << 20, dtype=torch.uint8, device=dev)
    fd = ops.dmabuf_fd(buf)
    assert fd >= 0
    st = os.fstat(fd)
    assert st is not None
    os.close(fd)


def test_soak_gpu_short(dev):
    from rocnrdma_amd.harness.soak import run_soak

    stats = run_soak("sdma", secs=5.0, region_bytes=64 << 20, seed=3,
                     device=dev)
    assert stats["cycles"] > 0
    assert stats["failures"] == 0


def test_p2p_matrix_runs(dev):
    from rocnrdma_amd.harness.xgmi_check import p2p_matrix

    rows = p2p_matrix(mb=64, iters=3)
    assert len(rows) >= 1  # 1 GPU -> self copy row
    assert all(r["gbps"] > 50 for r in rows)
