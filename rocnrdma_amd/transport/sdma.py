"""SDMA/PCIe transport: the BAR data path on a GPU-only box.

An HCA doing RDMA WRITE into GPU HBM is a PCIe bus master writing into
the GPU's BAR aperture; on a box without an HCA the measurable
equivalent of that path is moving data between host-pinned memory and
HBM across the same PCIe Gen5 x16 link (~63 GB/s spec).
One transport instance = one "QP" analog on one GPU.

Two engines, mirroring how a NIC actually retires work:

- "stream": hipMemcpyAsync per message on HIP streams (SDMA engines)
  taken round-robin by destination (stream_index), so copies into one
  destination stay in post order.  ~10 us host cost per message — fine
  >= 8 MiB, hopeless at 4 KiB (measured 0.3 GB/s).
- "kernel": doorbell semantics.  post() appends a WQE (two u64 writes
  into a pinned descriptor ring); flush() rings the doorbell — one
  gather/scatter kernel launch retires the whole batch, lanes reading
  host-pinned staging directly over PCIe (fine-grained zero-copy).
  Small-message bandwidth becomes PCIe-bound instead of launch-bound.

"auto" picks kernel below 8 MiB messages (measured crossover).  Integrity is proven on-GPU
(verify/CRC kernels) — zero host readback for write direction.

icrc=True (kernel engine only) swaps in the fused engine
(ops.gather_crc_/scatter_crc_): the launch that moves a batch also
digests every message, and the digests are compared with the stamped
expectations on the same stream — each WQE carries a third word for
that — into two device counters.  No host readback, no extra sync.

var_len=True (kernel engine only) gives every WQE a length word and
retires the ring with ops.gather_v_/scatter_v_ (crc=icrc): msg_bytes is
the slot size, each message moves only the bytes its post asked for.

byte_granular=True (on top of var_len) retires the same ring with
ops.gather_bytes_/scatter_bytes_: any byte count, and region_skew /
staging_skew move every region offset and staging address of the ring
by a constant, so the rows stay what they were.

max_sge=K > 1 (on top of byte_granular, staging_skew == 0) gives every
WQE a fixed K SGE fields (address, length) next to its region offset, as
a hardware WQE has: a list with fewer SGEs leaves the others at length
0, so the CSR row starts are the constant arange(inflight + 1) * K, built
once on the device.  flush() retires the ring with one
ops.gather_sg_/scatter_sg_ launch (crc=icrc) on the flush stream.

protected=True (on top of byte_granular, max_sge == 1) gives every WQE a
key word (lkey << 32 | rkey) and retires the ring with
ops.gather_prot_/scatter_prot_ (crc=icrc): the MR table lives in pinned
memory and is copied to the device at the next flush after it changed,
the queue-pair state word and the {"ok", "errors", "flushed"} counters
live on the device and are updated on the flush stream.
"""
from __future__ import annotations

import torch

from .base import Transport

_KERNEL_THRESHOLD = 8 << 20
_STAGING_TARGET = 64 << 20  # pinned staging budget for small messages

# Rows of the WQE ring.  The optional rows follow in this order: the
# message's byte count (var_len), then its keys (protected), then what
# the inline digest is compared with (icrc): the expected CRC32 of the
# slot (write), or the region message whose stamp stays on the device
# (read).
ROW_OFF, ROW_ADDR = 0, 1  # region offset, staging address


def stream_index(i: int, inflight: int, msgs_per_region: int,
                 direction: str, num_streams: int) -> int:
    """The HIP stream the stream engine copies message i on: chosen by
    the destination (the staging slot of a read, the region message of a
    write), so that two copies into one destination share a stream and
    keep post order (Transport's destination rule).  Equal to
    i % num_streams wherever num_streams divides the modulus."""
    dest = i % inflight if direction == "read" else i % msgs_per_region
    return dest % num_streams


class SdmaTransport(Transport):
    name = "sdma"
    supports_icrc = True
    supports_var_len = True
    supports_byte_granular = True
    supports_sg_list = True
    supports_protection = True

    def __init__(self, msg_bytes: int, region_bytes: int, device=None,
                 num_streams: int = 2, engine: str = "auto",
                 inflight: int | None = None, **kw):
        if not torch.cuda.is_available():
            raise RuntimeError("sdma transport requires a GPU")
        if engine == "auto":
            engine = "kernel" if msg_bytes < _KERNEL_THRESHOLD else "stream"
        self.engine = engine
        if kw.get("icrc") and engine != "kernel":
            raise ValueError(
                "icrc=True needs the kernel engine: the stream engine "
                "(explicit, or picked by auto for messages of 8 MiB and "
                "up) moves data with hipMemcpyAsync, where no kernel "
                "sees the bytes to digest them")
        if kw.get("var_len") and engine != "kernel":
            raise ValueError(
                "var_len=True needs the kernel engine: only its WQEs "
                "carry a length; the stream engine (explicit, or picked "
                "by auto for slots of 8 MiB and up) copies whole slots")
        if kw.get("max_sge", 1) != 1 and engine != "kernel":
            raise ValueError(
                "max_sge > 1 needs the kernel engine: only its WQEs carry "
                "a scatter/gather list; the stream engine (explicit, or "
                "picked by auto for slots of 8 MiB and up) copies whole "
                "slots")
        if kw.get("protected") and engine != "kernel":
            raise ValueError(
                "protected=True needs the kernel engine: only its WQEs "
                "carry keys and only a kernel can judge them; the stream "
                "engine (explicit, or picked by auto for slots of 8 MiB "
                "and up) copies whole slots")
        if inflight in (None, 0):
            if engine == "kernel":
                inflight = max(8, min(region_bytes // msg_bytes,
                                      _STAGING_TARGET // msg_bytes, 16384))
            else:
                inflight = 8
        super().__init__(msg_bytes, region_bytes, inflight=inflight, **kw)
        self.device = torch.device(device or "cuda")
        with torch.cuda.device(self.device):
            self.streams = [torch.cuda.Stream(self.device)
                            for _ in range(max(1, num_streams))]
        # one contiguous pinned staging area, sliced into slots
        self.staging_flat = torch.empty(self.inflight * msg_bytes,
                                        dtype=torch.uint8, pin_memory=True)
        self.staging = [
            self.staging_flat[i * msg_bytes:(i + 1) * msg_bytes]
            for i in range(self.inflight)
        ]
        self.region = torch.zeros(region_bytes, dtype=torch.uint8,
                                  device=self.device)
        if self.engine == "kernel":
            import numpy as np

            base = self.staging_flat.data_ptr() + self.staging_skew
            self._slot_addr = [base + i * msg_bytes
                               for i in range(self.inflight)]
            self._slot_addr_np = np.array(self._slot_addr, dtype=np.int64)
            # WQE ring: ROW_OFF, ROW_ADDR, then the optional rows
            rows = 2
            self._row_len = self._row_exp = self._row_key = None
            if self.var_len:
                self._row_len, rows = rows, rows + 1
            if self.protected:
                self._row_key, rows = rows, rows + 1
            if self.icrc:
                self._row_exp, rows = rows, rows + 1
            self._desc_pin = torch.empty((rows, self.inflight),
                                         dtype=torch.int64, pin_memory=True)
            self._desc_np = self._desc_pin.numpy()
            self._desc_dev = torch.empty((rows, self.inflight),
                                         dtype=torch.int64,
                                         device=self.device)
            self._pending = 0
            if self.max_sge > 1:
                # the SGE fields of the ring: [address | length][WQE][SGE]
                K = self.max_sge
                self._sg_pin = torch.zeros((2, self.inflight, K),
                                           dtype=torch.int64, pin_memory=True)
                self._sg_np = self._sg_pin.numpy()
                self._sg_dev = torch.empty((2, self.inflight * K),
                                           dtype=torch.int64,
                                           device=self.device)
                self._sg_start = torch.arange(
                    self.inflight + 1, dtype=torch.int64,
                    device=self.device) * K
                torch.cuda.synchronize(self.device)
        if self.protected:
            self._mr_pin = torch.zeros((self.max_mr, 4), dtype=torch.int64,
                                       pin_memory=True)
            self._mr_dev = torch.zeros((self.max_mr, 4), dtype=torch.int64,
                                       device=self.device)
            self._prot_open(self._mr_pin.numpy(), self.region.data_ptr(),
                            self.staging_flat.data_ptr(),
                            self.inflight * msg_bytes)
            self._qp_dev = torch.zeros(1, dtype=torch.int32,
                                       device=self.device)
            # ok, errors, flushed
            self._prot_dev = torch.zeros(3, dtype=torch.int64,
                                         device=self.device)
            self._last_status = None  # of the last flushed batch
            self._sink = None  # statuses of a running check, post order
            self._last_digests = None
            torch.cuda.synchronize(self.device)
        if self.icrc:
            self._stamped = False
            self._exp_slot_np = None  # write: int32-wrapped CRC per slot
            self._exp_dev = None      # read: int32 CRC per region message
            self._icrc_dev = torch.zeros(2, dtype=torch.int64,
                                         device=self.device)  # checked, bad
            self._last_digests = None  # of the last flushed batch
            # the counters were zeroed on the caller's stream; flush()
            # updates them on its own
            torch.cuda.synchronize(self.device)

    # -- data plane ----------------------------------------------------
    def post(self, i: int, nbytes: int | None = None, *, rkey=None,
             lkey=None) -> None:
        keys = None
        if self.protected or rkey is not None or lkey is not None:
            keys = self._keys(rkey, lkey, 1)
        if self.max_sge > 1:
            return self.post_sg(i, [(0, self._len1(nbytes))])
        if nbytes is not None or self.var_len:
            nbytes = self._len1(nbytes)
        off = (i % self.msgs_per_region) * self.msg_bytes + self.region_skew
        slot = i % self.inflight
        if self.engine == "kernel":
            if self._pending >= self.inflight:
                self.flush()
            k = self._pending
            self._desc_np[ROW_OFF, k] = off
            self._desc_np[ROW_ADDR, k] = self._slot_addr[slot]
            if self.var_len:
                self._desc_np[self._row_len, k] = nbytes
            if keys is not None:
                self._desc_np[self._row_key, k] = keys[0]
            if self.icrc and self._stamped:
                self._desc_np[self._row_exp, k] = (
                    self._exp_slot_np[slot] if self.direction == "write"
                    else i % self.msgs_per_region)
            self._pending = k + 1
            return
        stream = self.streams[stream_index(
            i, self.inflight, self.msgs_per_region, self.direction,
            len(self.streams))]
        dst = self.region[off:off + self.msg_bytes]
        with torch.cuda.stream(stream):
            if self.direction == "write":
                dst.copy_(self.staging[slot], non_blocking=True)
            else:
                self.staging[slot].copy_(dst, non_blocking=True)

    def post_many(self, start: int, n: int, nbytes=None, *, rkey=None,
                  lkey=None) -> None:
        """Vectorized WQE writes (numpy) — the posting loop itself must
        not bound small-message rates (a verbs app posts in C; measured:
        scalar python post() capped 4 KiB at ~10 GB/s)."""
        if self.engine != "kernel":
            return super().post_many(start, n, nbytes, rkey=rkey, lkey=lkey)
        import numpy as np

        keys = None
        if self.protected or rkey is not None or lkey is not None:
            keys = self._keys(rkey, lkey, n)

        if self.max_sge > 1:  # one SGE each: the slot's first nbytes
            sges = np.zeros((n, self.max_sge, 2), dtype=np.int64)
            sges[:, 0, 1] = self._lens(nbytes, n)
            return self.post_many_sg(start, n, sges)
        lens = None
        if nbytes is not None or self.var_len:
            lens = self._lens(nbytes, n)  # one vectorized check
        done = 0
        while done < n:
            if self._pending >= self.inflight:
                self.flush()
            k = self._pending
            take = min(n - done, self.inflight - k)
            idx = np.arange(start + done, start + done + take,
                            dtype=np.int64)
            self._desc_np[ROW_OFF, k:k + take] = \
                (idx % self.msgs_per_region) * self.msg_bytes + \
                self.region_skew
            self._desc_np[ROW_ADDR, k:k + take] = \
                self._slot_addr_np[idx % self.inflight]
            if lens is not None:
                self._desc_np[self._row_len, k:k + take] = \
                    lens[done:done + take]
            if keys is not None:
                self._desc_np[self._row_key, k:k + take] = \
                    keys[done:done + take]
            if self.icrc and self._stamped:
                self._desc_np[self._row_exp, k:k + take] = (
                    self._exp_slot_np[idx % self.inflight]
                    if self.direction == "write"
                    else idx % self.msgs_per_region)
            self._pending = k + take
            done += take

    def post_sg(self, i: int, sges) -> None:
        self.post_many_sg(i, 1, self._sges(sges)[None])

    def post_many_sg(self, start: int, n: int, sges) -> None:
        """Vectorized WQE writes for scatter/gather lists: the region
        offset row as in post_many, and the K SGE fields per WQE."""
        import numpy as np

        sges = self._sges(sges, n)  # one vectorized check
        done = 0
        while done < n:
            if self._pending >= self.inflight:
                self.flush()
            k = self._pending
            take = min(n - done, self.inflight - k)
            idx = np.arange(start + done, start + done + take,
                            dtype=np.int64)
            self._desc_np[ROW_OFF, k:k + take] = \
                (idx % self.msgs_per_region) * self.msg_bytes + \
                self.region_skew
            part = sges[done:done + take]
            self._sg_np[0, k:k + take] = \
                self._slot_addr_np[idx % self.inflight][:, None] + \
                part[:, :, 0]
            self._sg_np[1, k:k + take] = part[:, :, 1]
            self._pending = k + take
            done += take

    def flush(self) -> None:
        if self.engine == "kernel":
            n = self._pending
            if n:
                from .. import ops

                self._pending = 0
                stream = self.streams[0]
                with torch.cuda.stream(stream):
                    self._desc_dev[:, :n].copy_(self._desc_pin[:, :n],
                                                non_blocking=True)
                    if self.max_sge > 1:
                        self._flush_sg(n)
                    elif self.protected:
                        self._flush_prot(n)
                    elif self.var_len:
                        self._flush_var_len(n)
                    elif self.icrc:
                        self._flush_icrc(n)
                    elif self.direction == "write":
                        ops.gather_(self.region, self._desc_dev[ROW_OFF, :n],
                                    self._desc_dev[ROW_ADDR, :n],
                                    self.msg_bytes)
                    else:
                        ops.scatter_(self.region, self._desc_dev[ROW_OFF, :n],
                                     self._desc_dev[ROW_ADDR, :n],
                                     self.msg_bytes)
            self.streams[0].synchronize()
            return
        for s in self.streams:
            s.synchronize()

    def _flush_icrc(self, n: int) -> None:
        """Fused engine + compare, on the current (flush) stream."""
        from .. import ops

        engine = (ops.gather_crc_ if self.direction == "write"
                  else ops.scatter_crc_)
        dig = engine(self.region, self._desc_dev[ROW_OFF, :n],
                     self._desc_dev[ROW_ADDR, :n], self.msg_bytes)
        self._last_digests = dig
        if not self._stamped:
            return
        field = self._desc_dev[self._row_exp, :n]
        exp = field if self.direction == "write" else self._exp_dev[field]
        self._icrc_dev[0].add_(n)
        self._icrc_dev[1].add_((dig != exp).sum())

    def _flush_var_len(self, n: int) -> None:
        """One variable-length engine launch for the ring, on the current
        (flush) stream; with icrc the digests of the batch are kept."""
        from .. import ops

        if self.byte_granular:
            engine = (ops.gather_bytes_ if self.direction == "write"
                      else ops.scatter_bytes_)
        else:
            engine = (ops.gather_v_ if self.direction == "write"
                      else ops.scatter_v_)
        dig = engine(self.region, self._desc_dev[ROW_OFF, :n],
                     self._desc_dev[ROW_ADDR, :n],
                     self._desc_dev[self._row_len, :n],
                     max_msg_bytes=self.msg_bytes, crc=self.icrc)
        if self.icrc:
            self._last_digests = dig

    def _flush_prot(self, n: int) -> None:
        """One protected engine launch for the ring, on the current
        (flush) stream: the MR table first if it changed, then the
        launch against the transport's queue-pair word; the statuses of
        the batch are kept and counted on the same stream."""
        from .. import ops

        if self._mr_dirty:
            self._mr_dev.copy_(self._mr_pin, non_blocking=True)
            self._mr_dirty = False
        engine = (ops.gather_prot_ if self.direction == "write"
                  else ops.scatter_prot_)
        st, dig = engine(self.region, self._desc_dev[ROW_OFF, :n],
                         self._desc_dev[ROW_ADDR, :n],
                         self._desc_dev[self._row_len, :n],
                         self._desc_dev[self._row_key, :n], self._mr_dev,
                         qp_state=self._qp_dev, max_msg_bytes=self.msg_bytes,
                         crc=self.icrc)
        self._last_status = st
        if self.icrc:
            self._last_digests = dig
        ok = (st == ops.WC_SUCCESS).sum()
        flushed = (st == ops.WC_WR_FLUSH_ERR).sum()
        self._prot_dev[0].add_(ok)
        self._prot_dev[1].add_(n - ok - flushed)
        self._prot_dev[2].add_(flushed)
        if self._sink is not None:
            self._sink.append(st)

    def completions(self):
        import numpy as np

        self._need_protected()
        if self._last_status is None:
            return np.zeros(0, dtype=np.int32)
        return self._last_status.cpu().numpy()

    def prot_stats(self) -> dict:
        self._need_protected()
        self.flush()
        ok, errors, flushed = self._prot_dev.tolist()
        return {"ok": ok, "errors": errors, "flushed": flushed}

    def qp_in_error(self) -> bool:
        self._need_protected()
        self.flush()
        return bool(self._qp_dev.item())

    def reset_qp(self) -> None:
        self._need_protected()
        self.flush()
        with torch.cuda.stream(self.streams[0]):
            self._qp_dev.zero_()
        self.streams[0].synchronize()

    def _flush_sg(self, n: int) -> None:
        """One scatter/gather engine launch for the ring, on the current
        (flush) stream; with icrc the digests of the batch are kept."""
        from .. import ops

        nsge = n * self.max_sge
        self._sg_dev[:, :nsge].copy_(
            self._sg_pin.view(2, -1)[:, :nsge], non_blocking=True)
        engine = (ops.gather_sg_ if self.direction == "write"
                  else ops.scatter_sg_)
        dig = engine(self.region, self._desc_dev[ROW_OFF, :n],
                     self._sg_start[:n + 1], self._sg_dev[0, :nsge],
                     self._sg_dev[1, :nsge], max_msg_bytes=self.msg_bytes,
                     crc=self.icrc)
        if self.icrc:
            self._last_digests = dig
        # (the pinned SGE fields may be rewritten once flush() has
        # synchronised, as the rest of the ring)

    def stamp(self) -> None:
        if not self.icrc or self.var_len:
            return super().stamp()
        import zlib

        import numpy as np

        from .. import ops

        self.flush()
        if self.direction == "write":
            crcs = np.array([zlib.crc32(s.numpy()) for s in self.staging],
                            dtype=np.uint32)
            # as the int32 the engine returns, widened to the WQE word
            self._exp_slot_np = crcs.view(np.int32).astype(np.int64)
        else:
            self._exp_dev = ops.crc32_messages(self.region, self.msg_bytes)
            # taken on the caller's stream; flush() works on its own
            torch.cuda.synchronize(self.device)
        self._stamped = True

    def icrc_stats(self) -> dict:
        if not self.icrc:
            return super().icrc_stats()
        self.flush()
        checked, bad = self._icrc_dev.tolist()
        return {"checked": checked, "bad": bad}

    # -- integrity plane: what the checks of the base class work on -----
    @property
    def _slots(self):
        return self.staging_flat.numpy().reshape(self.inflight,
                                                 self.msg_bytes)

    def _region_set(self, arr) -> None:
        self.region.copy_(torch.from_numpy(arr))
        torch.cuda.synchronize(self.device)

    def _region_fill(self, byte: int) -> None:
        self.region.fill_(byte)
        torch.cuda.synchronize(self.device)

    def _region_get(self):
        return self.region.cpu().numpy()

    def _region_digests(self, offs, lens, bound: int):
        """One launch over the region, so only 4 bytes per message ever
        cross back — no payload readback: crc32_messages for the whole
        slots of a transport without var_len, crc32_messages_v with it,
        crc32_messages_bytes with byte_granular."""
        import numpy as np

        from .. import ops

        if not self.var_len:
            got = ops.crc32_messages(self.region, self.msg_bytes)
        else:
            crc_v = (ops.crc32_messages_bytes if self.byte_granular
                     else ops.crc32_messages_v)
            got = crc_v(self.region, torch.from_numpy(offs).to(self.device),
                        torch.from_numpy(lens).to(self.device),
                        max_msg_bytes=bound)
        return got.cpu().numpy().view(np.uint32)

    def _region_pattern(self, seed: int) -> None:
        from .. import ops

        ops.fill_(self.region, seed)
        torch.cuda.synchronize(self.device)

    def _region_mismatches(self, seed: int) -> int:
        from .. import ops

        # on-GPU verification — no host readback
        return int(ops.verify(self.region, seed))

    def _gather_host(self, batches):
        return torch.cat(batches).cpu().numpy()

    def close(self) -> None:
        self.flush()
