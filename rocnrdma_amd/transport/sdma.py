"""SDMA/PCIe transport: the BAR data path on a GPU-only box.

An HCA doing RDMA WRITE into GPU HBM is a PCIe bus master writing into
the GPU's BAR aperture; on a box without an HCA the measurable
equivalent of that path is moving data between host-pinned memory and
HBM across the same PCIe Gen5 x16 link (~63 GB/s spec).
One transport instance = one "QP" analog on one GPU.

Two engines, mirroring how a NIC actually retires work:

- "stream": hipMemcpyAsync per message on round-robin HIP streams (SDMA
  engines).  ~10 us host cost per message — fine >= 8 MiB, hopeless at
  4 KiB (measured 0.3 GB/s).
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

from ..utils import pattern
from .base import Transport

_KERNEL_THRESHOLD = 8 << 20
_STAGING_TARGET = 64 << 20  # pinned staging budget for small messages

# Rows of the WQE ring.  The optional rows follow in this order: the
# message's byte count (var_len), then its keys (protected), then what
# the inline digest is compared with (icrc): the expected CRC32 of the
# slot (write), or the region message whose stamp stays on the device
# (read).
ROW_OFF, ROW_ADDR = 0, 1  # region offset, staging address
_KNOWN = 0x5A  # what digest_check(payload, lens) leaves in the slack


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
        stream = self.streams[i % len(self.streams)]
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

    def _rejected(self, run):
        """run() a check's posts and flushes; the boolean array of its
        messages, in post order, that did not complete with SUCCESS
        (nothing is rejected without protected=True)."""
        if not self.protected:
            return run(), False
        self.flush()
        self._sink = []
        try:
            res = run()
            self.flush()
            st = torch.cat(self._sink).cpu().numpy()
        finally:
            self._sink = None
        return res, st != 0

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

    # -- integrity plane ----------------------------------------------
    def integrity_check(self, seed: int) -> int:
        bad, rejected = self._rejected(lambda: self._integrity_check(seed))
        return bad + int(rejected.sum() if self.protected else 0)

    def _integrity_check(self, seed: int) -> int:
        from .. import ops

        self._no_pattern_with_skew()
        if self.icrc:
            self._stamped = False  # the sender is rewritten below
        ref = pattern.fill_reference(self.region_bytes, seed)
        ref_t = torch.from_numpy(ref.copy())
        if self.direction == "write":
            i = 0
            while i < self.msgs_per_region:
                burst = min(self.inflight, self.msgs_per_region - i)
                for j in range(i, i + burst):
                    off = j * self.msg_bytes
                    self.staging[j % self.inflight].copy_(
                        ref_t[off:off + self.msg_bytes])
                    self.post(j)
                self.flush()  # slots reused next burst: must complete
                i += burst
            # on-GPU verification — no host readback
            return int(ops.verify(self.region, seed))
        # read: pattern HBM with the fill kernel, pull to host, check there
        ops.fill_(self.region, seed)
        torch.cuda.synchronize(self.device)
        bad = 0
        i = 0
        while i < self.msgs_per_region:
            burst = min(self.inflight, self.msgs_per_region - i)
            for j in range(i, i + burst):
                self.post(j)
            self.flush()
            for j in range(i, i + burst):
                off = j * self.msg_bytes
                got = self.staging[j % self.inflight].numpy()
                want = ref[off:off + self.msg_bytes]
                bad += int((got.view("u8") != want.view("u8")).sum())
            i += burst
        return bad

    def digest_check(self, payload, lens=None) -> int:
        """Per-message CRC32 of arbitrary content, sender vs receiver.
        The HBM side is digested by one crc32_messages launch, so only
        4 bytes per message ever cross back — no payload readback."""
        import zlib

        import numpy as np

        from .. import ops

        pay = self._payload_bytes(payload)
        pay_t = torch.from_numpy(pay)
        n, msg = self.msgs_per_region, self.msg_bytes
        if self.var_len or lens is not None:
            lens = self._lens(lens, n)
            bad, rejected = self._rejected(
                lambda: self._digest_check_var_len(pay_t, lens))
            return int((bad | rejected).sum())
        if self.icrc:
            return self._digest_check_icrc(pay_t)
        if self.direction == "write":
            sent = np.empty(n, dtype=np.uint32)
            i = 0
            while i < n:
                burst = min(self.inflight, n - i)
                for j in range(i, i + burst):
                    slot = self.staging[j % self.inflight]
                    slot.copy_(pay_t[j * msg:(j + 1) * msg])
                    sent[j] = zlib.crc32(slot.numpy())
                    self.post(j)
                self.flush()  # slots reused next burst: must complete
                i += burst
            got = ops.crc32_messages(self.region, msg)
            return int(np.count_nonzero(
                got.cpu().numpy().view(np.uint32) != sent))
        # read: load HBM with the payload, digest it there, pull to host
        self.region.copy_(pay_t)
        sent = ops.crc32_messages(self.region, msg)
        torch.cuda.synchronize(self.device)
        sent = sent.cpu().numpy().view(np.uint32)
        bad = 0
        i = 0
        while i < n:
            burst = min(self.inflight, n - i)
            for j in range(i, i + burst):
                self.post(j)
            self.flush()
            for j in range(i, i + burst):
                got = zlib.crc32(self.staging[j % self.inflight].numpy())
                bad += int(got != int(sent[j]))
            i += burst
        return bad

    def _digest_check_icrc(self, pay_t) -> int:
        """digest_check with the HBM-side digests taken by the fused
        engine while it moves each burst — no second pass over the
        region.  The host side is digested with zlib as before."""
        import zlib

        import numpy as np

        n, msg = self.msgs_per_region, self.msg_bytes
        write = self.direction == "write"
        self._stamped = False  # the sender is rewritten below
        if not write:
            self.region.copy_(pay_t)
            torch.cuda.synchronize(self.device)
        host = np.empty(n, dtype=np.uint32)
        inline = []
        i = 0
        while i < n:
            burst = min(self.inflight, n - i)
            for j in range(i, i + burst):
                if write:
                    slot = self.staging[j % self.inflight]
                    slot.copy_(pay_t[j * msg:(j + 1) * msg])
                    host[j] = zlib.crc32(slot.numpy())
                self.post(j)
            self.flush()  # slots reused next burst: must complete
            inline.append(self._last_digests)
            if not write:
                for j in range(i, i + burst):
                    host[j] = zlib.crc32(
                        self.staging[j % self.inflight].numpy())
            i += burst
        got = torch.cat(inline).cpu().numpy().view(np.uint32)
        return int(np.count_nonzero(got != host))

    def _digest_check_var_len(self, pay_t, lens) -> int:
        """digest_check for per-message lengths.  HBM-side digests: the
        fused engine's (icrc) or one crc32_messages_v launch; host side:
        zlib.  The receiver starts as _KNOWN everywhere and its slack
        ranges must still hold it: in HBM a second crc32_messages_v over
        the slack ranges against the digest of that many _KNOWN bytes,
        on the host numpy.  With byte_granular the messages sit at the
        skews, the launches are crc32_messages_bytes and the slack is
        the slot in front of and behind the message.  Returns the
        boolean array of bad messages."""
        import zlib

        import numpy as np

        from .. import ops

        n, msg = self.msgs_per_region, self.msg_bytes
        ss, rs = self.staging_skew, self.region_skew
        crc_v = (ops.crc32_messages_bytes if self.byte_granular
                 else ops.crc32_messages_v)
        write = self.direction == "write"
        if self.icrc:
            self._stamped = False
        offs = np.arange(n, dtype=np.int64) * msg
        d_offs = torch.from_numpy(offs + rs).to(self.device)
        d_lens = torch.from_numpy(lens).to(self.device)
        if write:
            self.region.fill_(_KNOWN)
        elif rs:
            reg = pay_t.numpy().copy()
            for j in range(n):
                reg[j * msg + rs:j * msg + rs + lens[j]] = \
                    pay_t.numpy()[j * msg:j * msg + lens[j]]
            self.region.copy_(torch.from_numpy(reg))
        else:
            self.region.copy_(pay_t)
        torch.cuda.synchronize(self.device)
        host = np.empty(n, dtype=np.uint32)
        bad = np.zeros(n, dtype=bool)
        inline = []
        i = 0
        while i < n:
            burst = min(self.inflight, n - i)
            if not write:
                self.staging_flat[:burst * msg].fill_(_KNOWN)
            else:
                for j in range(i, i + burst):
                    slot = self.staging[j % self.inflight]
                    slot.copy_(pay_t[j * msg:(j + 1) * msg])
                    if ss:
                        slot[ss:ss + lens[j]].copy_(
                            pay_t[j * msg:j * msg + lens[j]])
                    host[j] = zlib.crc32(slot.numpy()[ss:ss + lens[j]])
            self.post_many(i, burst, lens[i:i + burst])
            self.flush()  # slots reused next burst: must complete
            if self.icrc:
                inline.append(self._last_digests)
            if not write:
                for j in range(i, i + burst):
                    slot = self.staging[j % self.inflight].numpy()
                    host[j] = zlib.crc32(slot[ss:ss + lens[j]])
                    bad[j] = bool((slot[:ss] != _KNOWN).any() or
                                  (slot[ss + lens[j]:] != _KNOWN).any())
            i += burst
        if self.icrc:
            hbm = torch.cat(inline)
        else:
            hbm = crc_v(self.region, d_offs, d_lens, max_msg_bytes=msg)
        if write:
            behind = msg - rs - lens
            slack = crc_v(self.region, d_offs + d_lens, msg - rs - d_lens,
                          max_msg_bytes=msg)
            known = {int(k): zlib.crc32(bytes([_KNOWN]) * int(k))
                     for k in np.unique(behind)}
            want = np.array([known[int(k)] for k in behind],
                            dtype=np.uint32)
            bad |= slack.cpu().numpy().view(np.uint32) != want
            if rs:
                front = crc_v(self.region, d_offs - rs,
                              torch.full_like(d_lens, rs), max_msg_bytes=16)
                bad |= (front.cpu().numpy().view(np.uint32)
                        != zlib.crc32(bytes([_KNOWN]) * rs))
        bad |= hbm.cpu().numpy().view(np.uint32) != host
        return bad

    def digest_check_sg(self, payload, sges) -> int:
        """digest_check for scatter/gather traffic (see the base class).
        HBM-side digests: the fused engine's (icrc) or one
        crc32_messages_bytes launch over the region ranges; host side:
        zlib over the concatenated SGE ranges of the slot.  The slack in
        HBM is digested as in digest_check(payload, lens), the slack of a
        slot is inspected with numpy."""
        import zlib

        import numpy as np

        from .. import ops

        pay = self._payload_bytes(payload)
        pay_t = torch.from_numpy(pay)
        n, msg, rs = self.msgs_per_region, self.msg_bytes, self.region_skew
        sges = self._sges(sges, n)
        lens = sges[:, :, 1].sum(axis=1)
        write = self.direction == "write"
        if self.icrc:
            self._stamped = False
        d_offs = torch.from_numpy(
            np.arange(n, dtype=np.int64) * msg + rs).to(self.device)
        d_lens = torch.from_numpy(lens).to(self.device)
        if write:
            self.region.fill_(_KNOWN)
        else:  # the first L_j payload bytes of the slot, at the skew
            reg = pay.copy()
            for j in range(n):
                reg[j * msg + rs:j * msg + rs + lens[j]] = \
                    pay[j * msg:j * msg + lens[j]]
            self.region.copy_(torch.from_numpy(reg))
        torch.cuda.synchronize(self.device)

        def pieces(slot, j):
            return np.concatenate([slot[o:o + k] for o, k in sges[j]])

        host = np.empty(n, dtype=np.uint32)
        bad = np.zeros(n, dtype=bool)
        inline = []
        i = 0
        while i < n:
            burst = min(self.inflight, n - i)
            if write:
                for j in range(i, i + burst):
                    slot = self.staging[j % self.inflight]
                    slot.copy_(pay_t[j * msg:(j + 1) * msg])
                    host[j] = zlib.crc32(pieces(slot.numpy(), j))
            else:
                self.staging_flat[:burst * msg].fill_(_KNOWN)
            self.post_many_sg(i, burst, sges[i:i + burst])
            self.flush()  # slots reused next burst: must complete
            if self.icrc:
                inline.append(self._last_digests)
            if not write:
                for j in range(i, i + burst):
                    slot = self.staging[j % self.inflight].numpy()
                    host[j] = zlib.crc32(pieces(slot, j))
                    rest = np.ones(msg, dtype=bool)
                    for o, k in sges[j]:
                        rest[o:o + k] = False
                    bad[j] = bool((slot[rest] != _KNOWN).any())
            i += burst
        crc_b = ops.crc32_messages_bytes
        if self.icrc:
            hbm = torch.cat(inline)
        else:
            hbm = crc_b(self.region, d_offs, d_lens, max_msg_bytes=msg)
        if write:
            behind = msg - rs - lens
            slack = crc_b(self.region, d_offs + d_lens, msg - rs - d_lens,
                          max_msg_bytes=msg)
            known = {int(k): zlib.crc32(bytes([_KNOWN]) * int(k))
                     for k in np.unique(behind)}
            want = np.array([known[int(k)] for k in behind],
                            dtype=np.uint32)
            bad |= slack.cpu().numpy().view(np.uint32) != want
            if rs:
                front = crc_b(self.region, d_offs - rs,
                              torch.full_like(d_lens, rs), max_msg_bytes=16)
                bad |= (front.cpu().numpy().view(np.uint32)
                        != zlib.crc32(bytes([_KNOWN]) * rs))
        bad |= hbm.cpu().numpy().view(np.uint32) != host
        return int(bad.sum())

    def close(self) -> None:
        self.flush()
