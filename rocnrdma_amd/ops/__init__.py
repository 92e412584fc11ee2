"""gfx950 payload kernels (fill / verify / CRC32 / copy).

The native extension is mandatory on GPU: if torch sees a device but the
extension is missing, every entry point raises — no silent eager
fallback (CPU references for tests live in rocnrdma_amd.utils.pattern).
"""
from __future__ import annotations

import torch

try:
    from . import _p2p_ext  # built in-tree by setup.py (gfx950)
except ImportError:  # pragma: no cover - exercised only on broken installs
    _p2p_ext = None


def have_ext() -> bool:
    return _p2p_ext is not None


def _require():
    if _p2p_ext is None:
        raise RuntimeError(
            "rocnrdma_amd.ops._p2p_ext is not built. Run "
            "`python __graft_entry__.py build` (PYTORCH_ROCM_ARCH=gfx950). "
            "The GPU path never falls back to eager."
        )
    return _p2p_ext


def fill_(buf: torch.Tensor, seed: int) -> None:
    """In-place splitmix64 pattern fill (word i = mix(seed+(i+1)*PHI))."""
    _require().fill_(buf, seed)


def verify(buf: torch.Tensor, seed: int) -> int:
    """Count 8-byte words deviating from the fill pattern (on-GPU)."""
    return _require().verify(buf, seed)


def crc32_pages(buf: torch.Tensor) -> torch.Tensor:
    """zlib-compatible CRC32 of each 4 KiB page; int32 tensor on GPU."""
    return _require().crc32_pages(buf)


def crc32_messages(region: torch.Tensor, msg_bytes: int,
                   offs: torch.Tensor | None = None, *,
                   grid_cap: int = 0) -> torch.Tensor:
    """zlib-compatible CRC32 of each msg_bytes message; int32 tensor[n] on
    GPU, no sync (view as uint32 for zlib's values).

    Without offs the region is n = nbytes // msg_bytes back-to-back
    messages; with offs (contiguous int64 GPU tensor, 16-byte-aligned byte
    offsets as for gather_) message m starts at offs[m].  msg_bytes is a
    non-zero multiple of 16.  grid_cap caps the workgroup count (0 = tuned
    default) — a tuning and testing knob."""
    return _require().crc32_messages(region, msg_bytes, offs, grid_cap)


def crc32(buf: torch.Tensor, *, grid_cap: int = 0) -> int:
    """zlib.crc32 of the whole buffer (any byte length, 16-byte-aligned
    base), computed in HBM; only the 4-byte digest crosses to the host."""
    return _require().crc32(buf, grid_cap)


def copy_(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Streaming 16 B/lane device copy (bandwidth ceiling probe)."""
    _require().copy_(dst, src)


def copy_nt_(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Nontemporal streaming copy (streamed-once data stays out of L2)."""
    _require().copy_nt_(dst, src)


def gather_(region: torch.Tensor, dst_offs: torch.Tensor,
            src_addrs: torch.Tensor, msg_bytes: int) -> None:
    """Batched message engine: host-pinned sources -> HBM region offsets
    (one launch retires the whole batch — the NIC-WQE analog)."""
    _require().gather_(region, dst_offs, src_addrs, msg_bytes)


def scatter_(region: torch.Tensor, src_offs: torch.Tensor,
             dst_addrs: torch.Tensor, msg_bytes: int) -> None:
    """Batched message engine: HBM region offsets -> host-pinned dests."""
    _require().scatter_(region, src_offs, dst_addrs, msg_bytes)


def gather_crc_(region: torch.Tensor, dst_offs: torch.Tensor,
                src_addrs: torch.Tensor, msg_bytes: int, *,
                grid_cap: int = 0) -> torch.Tensor:
    """gather_ with an inline ICRC: the same launch moves the batch and
    returns zlib's CRC32 of every message as it was loaded over the link
    (int32 tensor[n] on the region's device, no sync; view as uint32).
    grid_cap caps the workgroup count below the engine's own cap (0 =
    default) — a tuning and testing knob."""
    return _require().gather_crc_(region, dst_offs, src_addrs, msg_bytes,
                                  grid_cap)


def scatter_crc_(region: torch.Tensor, src_offs: torch.Tensor,
                 dst_addrs: torch.Tensor, msg_bytes: int, *,
                 grid_cap: int = 0) -> torch.Tensor:
    """scatter_ with an inline ICRC: digests are of the HBM bytes as they
    were loaded on their way to the host-pinned destinations."""
    return _require().scatter_crc_(region, src_offs, dst_addrs, msg_bytes,
                                   grid_cap)


def gather_v_(region: torch.Tensor, dst_offs: torch.Tensor,
              src_addrs: torch.Tensor, lens: torch.Tensor, *,
              max_msg_bytes: int = 0, crc: bool = False,
              grid_cap: int = 0) -> torch.Tensor | None:
    """gather_ for a batch whose messages carry their own lengths: lens
    is a contiguous int64 GPU tensor[n] of byte counts, multiples of 16,
    0 allowed (nothing moved, digest 0).  Returns None, or with crc=True
    the inline ICRC as gather_crc_ does (int32 tensor[n], no sync).
    max_msg_bytes is an upper bound of the lengths if the caller knows
    one (0 = unknown); it only sizes the grid, results do not depend on
    it.  grid_cap as for gather_crc_."""
    return _require().gather_v_(region, dst_offs, src_addrs, lens,
                                max_msg_bytes, crc, grid_cap)


def scatter_v_(region: torch.Tensor, src_offs: torch.Tensor,
               dst_addrs: torch.Tensor, lens: torch.Tensor, *,
               max_msg_bytes: int = 0, crc: bool = False,
               grid_cap: int = 0) -> torch.Tensor | None:
    """scatter_ for per-message lengths; see gather_v_."""
    return _require().scatter_v_(region, src_offs, dst_addrs, lens,
                                 max_msg_bytes, crc, grid_cap)


def crc32_messages_v(region: torch.Tensor, offs: torch.Tensor,
                     lens: torch.Tensor, *, max_msg_bytes: int = 0,
                     grid_cap: int = 0) -> torch.Tensor:
    """zlib-compatible CRC32 of region[offs[m] : offs[m] + lens[m]] for
    every m; int32 tensor[n] on GPU, no sync.  offs are 16-byte aligned,
    lens are any byte counts (0 -> 0).  max_msg_bytes and grid_cap as
    for gather_v_."""
    return _require().crc32_messages_v(region, offs, lens, max_msg_bytes,
                                       grid_cap)


def gather_bytes_(region: torch.Tensor, dst_offs: torch.Tensor,
                  src_addrs: torch.Tensor, lens: torch.Tensor, *,
                  max_msg_bytes: int = 0, crc: bool = False,
                  grid_cap: int = 0) -> torch.Tensor | None:
    """gather_v_ for byte-granular messages: lens[m] >= 0 is any byte
    count, read from any byte address src_addrs[m] and written to any
    byte offset dst_offs[m]; the relative misalignment (src - dst) mod 16
    is arbitrary per message.  Only the region's base stays 16-byte
    aligned.  No byte outside [start, start + len) of any message is
    loaded or stored on either side (partial granules are written with
    narrow stores of exactly their valid bytes, never read-modify-write,
    so neighbours may share a granule); zero-length messages reach no
    load, store or atomic and their digest is 0.  Keyword arguments and
    result as for gather_v_; aligned multiples of 16 give what gather_v_
    gives."""
    return _require().gather_bytes_(region, dst_offs, src_addrs, lens,
                                    max_msg_bytes, crc, grid_cap)


def scatter_bytes_(region: torch.Tensor, src_offs: torch.Tensor,
                   dst_addrs: torch.Tensor, lens: torch.Tensor, *,
                   max_msg_bytes: int = 0, crc: bool = False,
                   grid_cap: int = 0) -> torch.Tensor | None:
    """scatter_v_ for byte-granular messages; see gather_bytes_."""
    return _require().scatter_bytes_(region, src_offs, dst_addrs, lens,
                                     max_msg_bytes, crc, grid_cap)


def crc32_messages_bytes(region: torch.Tensor, offs: torch.Tensor,
                         lens: torch.Tensor, *, max_msg_bytes: int = 0,
                         grid_cap: int = 0) -> torch.Tensor:
    """crc32_messages_v for offsets of any alignment: zlib's CRC32 of
    region[offs[m] : offs[m] + lens[m]] for every m, no byte outside a
    message loaded; int32 tensor[n] on GPU, no sync."""
    return _require().crc32_messages_bytes(region, offs, lens,
                                           max_msg_bytes, grid_cap)


def gather_sg_(region: torch.Tensor, offs: torch.Tensor,
               sge_start: torch.Tensor, sge_addrs: torch.Tensor,
               sge_lens: torch.Tensor, *, max_msg_bytes: int = 0,
               crc: bool = False, grid_cap: int = 0) -> torch.Tensor | None:
    """gather_bytes_ for messages with a scatter/gather list, as a work
    request's sg_list: the batch has n messages and S entries (SGEs) in
    CSR form.  sge_start is int64[n + 1], nondecreasing from 0 to S;
    message m owns the SGEs sge_start[m] .. sge_start[m + 1] - 1, SGE j
    is the sge_lens[j] >= 0 bytes at the byte address sge_addrs[j]
    (int64[S] each), and the message — their concatenation in list
    order, L_m bytes — is written to region[offs[m] : offs[m] + L_m].
    All four are contiguous int64 tensors on the region's device.  Any
    address, offset and length; the misalignment is arbitrary per SGE
    and only the region's base stays 16-byte aligned.  No byte outside
    an SGE or outside a message's region range is loaded or stored
    (narrow stores, never read-modify-write: consecutive SGEs and
    neighbouring messages may share a granule).  Messages without SGEs
    and SGEs of length 0 are legal anywhere and touch nothing.  SGEs may
    overlap where they are read; overlap where they are written is
    undefined.  With crc=True the result is zlib's CRC32 of every whole
    message (int32 tensor[n], no sync; 0 for an empty one), however it
    is cut — what gather_bytes_ returns for the same bytes as one
    message; one SGE per message gives what gather_bytes_ gives.
    max_msg_bytes bounds a whole message (0 = unknown) and only sizes
    the grid; grid_cap as for gather_crc_.  Stream-ordered, no host
    synchronise; the offsets are taken on the device."""
    return _require().gather_sg_(region, offs, sge_start, sge_addrs,
                                 sge_lens, max_msg_bytes, crc, grid_cap)


def scatter_sg_(region: torch.Tensor, offs: torch.Tensor,
                sge_start: torch.Tensor, sge_addrs: torch.Tensor,
                sge_lens: torch.Tensor, *, max_msg_bytes: int = 0,
                crc: bool = False, grid_cap: int = 0) -> torch.Tensor | None:
    """scatter_bytes_ for messages with a scatter/gather list:
    region[offs[m] : offs[m] + L_m] is cut, in list order, over the SGEs
    of message m; see gather_sg_."""
    return _require().scatter_sg_(region, offs, sge_start, sge_addrs,
                                  sge_lens, max_msg_bytes, crc, grid_cap)

# enum ibv_wc_status, as far as the protected engines produce it, and the
# verbs access bits of an MR-table entry
WC_SUCCESS = 0
WC_LOC_LEN_ERR = 1
WC_LOC_PROT_ERR = 4
WC_WR_FLUSH_ERR = 5
WC_REM_ACCESS_ERR = 10
ACCESS_LOCAL_WRITE = 1
ACCESS_REMOTE_WRITE = 2
ACCESS_REMOTE_READ = 4


def gather_prot_(region: torch.Tensor, dst_offs: torch.Tensor,
                 src_addrs: torch.Tensor, lens: torch.Tensor,
                 keys: torch.Tensor, mrs: torch.Tensor, *,
                 qp_state: torch.Tensor | None = None,
                 max_msg_bytes: int = 0, crc: bool = False,
                 grid_cap: int = 0):
    """gather_bytes_ behind memory protection, as an HCA checks a work
    request before it moves a byte.  keys[m] = lkey << 32 | rkey (int64
    [n], utils.prot.pack_keys); mrs is the MR table, contiguous int64
    [R, 4] on the region's device with rows (key, addr, length, access):
    a key is slot << 8 | tag and must sit in row `slot` with access != 0,
    access holds the ACCESS_* bits.  Per message, first rule wins: lens
    == 0 -> WC_SUCCESS (keys not read); lens < 0 -> WC_LOC_LEN_ERR; the
    outside range [src_addrs, +lens) not inside the MR of lkey ->
    WC_LOC_PROT_ERR; the region range [region + dst_offs, +lens) not
    inside the MR of rkey, or that MR without ACCESS_REMOTE_WRITE ->
    WC_REM_ACCESS_ERR.  No descriptor value is trusted: a message that
    does not complete with WC_SUCCESS moves nothing and its digest is 0.

    qp_state (int32 [1] on the device, 0 = ready) orders the batch like a
    queue pair: the first failing message completes with its own status,
    every later one with WC_WR_FLUSH_ERR, and the word is set to 1; a
    word that is non-zero on entry flushes the whole batch.  Without it
    every message is judged on its own.

    Returns (status, digests): int32 [n] each, digests None unless
    crc=True; no sync.  With a table that covers everything, valid keys
    and qp_state=None the bytes and digests are bit for bit those of
    gather_bytes_ and every status is 0.  max_msg_bytes and grid_cap as
    for gather_bytes_."""
    return _require().gather_prot_(region, dst_offs, src_addrs, lens, keys,
                                   mrs, qp_state, max_msg_bytes, crc,
                                   grid_cap)


def scatter_prot_(region: torch.Tensor, src_offs: torch.Tensor,
                  dst_addrs: torch.Tensor, lens: torch.Tensor,
                  keys: torch.Tensor, mrs: torch.Tensor, *,
                  qp_state: torch.Tensor | None = None,
                  max_msg_bytes: int = 0, crc: bool = False,
                  grid_cap: int = 0):
    """scatter_bytes_ behind memory protection; see gather_prot_.  The
    outside MR (lkey) is written and needs ACCESS_LOCAL_WRITE, the region
    MR (rkey) is read and needs ACCESS_REMOTE_READ."""
    return _require().scatter_prot_(region, src_offs, dst_addrs, lens, keys,
                                    mrs, qp_state, max_msg_bytes, crc,
                                    grid_cap)


def dmabuf_fd(buf: torch.Tensor) -> int:
    """Export an HBM tensor as a dmabuf fd (ibv_reg_dmabuf_mr's GPU
    half). Caller must os.close() the fd."""
    return _require().dmabuf_fd(buf)
