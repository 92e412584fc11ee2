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
"""
from __future__ import annotations

import torch

from ..utils import pattern
from .base import Transport

_KERNEL_THRESHOLD = 8 << 20
_STAGING_TARGET = 64 << 20  # pinned staging budget for small messages


class SdmaTransport(Transport):
    name = "sdma"

    def __init__(self, msg_bytes: int, region_bytes: int, device=None,
                 num_streams: int = 2, engine: str = "auto",
                 inflight: int | None = None, **kw):
        if not torch.cuda.is_available():
            raise RuntimeError("sdma transport requires a GPU")
        if engine == "auto":
            engine = "kernel" if msg_bytes < _KERNEL_THRESHOLD else "stream"
        self.engine = engine
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

            base = self.staging_flat.data_ptr()
            self._slot_addr = [base + i * msg_bytes
                               for i in range(self.inflight)]
            self._slot_addr_np = np.array(self._slot_addr, dtype=np.int64)
            # WQE ring: [0] = region offset, [1] = staging address
            self._desc_pin = torch.empty((2, self.inflight),
                                         dtype=torch.int64, pin_memory=True)
            self._desc_np = self._desc_pin.numpy()
            self._desc_dev = torch.empty((2, self.inflight),
                                         dtype=torch.int64,
                                         device=self.device)
            self._pending = 0

    # -- data plane ----------------------------------------------------
    def post(self, i: int) -> None:
        off = (i % self.msgs_per_region) * self.msg_bytes
        slot = i % self.inflight
        if self.engine == "kernel":
            if self._pending >= self.inflight:
                self.flush()
            k = self._pending
            self._desc_np[0, k] = off
            self._desc_np[1, k] = self._slot_addr[slot]
            self._pending = k + 1
            return
        stream = self.streams[i % len(self.streams)]
        dst = self.region[off:off + self.msg_bytes]
        with torch.cuda.stream(stream):
            if self.direction == "write":
                dst.copy_(self.staging[slot], non_blocking=True)
            else:
                self.staging[slot].copy_(dst, non_blocking=True)

    def post_many(self, start: int, n: int) -> None:
        """Vectorized WQE writes (numpy) — the posting loop itself must
        not bound small-message rates (a verbs app posts in C; measured:
        scalar python post() capped 4 KiB at ~10 GB/s)."""
        if self.engine != "kernel":
            return super().post_many(start, n)
        import numpy as np

        done = 0
        while done < n:
            if self._pending >= self.inflight:
                self.flush()
            k = self._pending
            take = min(n - done, self.inflight - k)
            idx = np.arange(start + done, start + done + take,
                            dtype=np.int64)
            self._desc_np[0, k:k + take] = \
                (idx % self.msgs_per_region) * self.msg_bytes
            self._desc_np[1, k:k + take] = \
                self._slot_addr_np[idx % self.inflight]
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
                    if self.direction == "write":
                        ops.gather_(self.region, self._desc_dev[0, :n],
                                    self._desc_dev[1, :n], self.msg_bytes)
                    else:
                        ops.scatter_(self.region, self._desc_dev[0, :n],
                                     self._desc_dev[1, :n], self.msg_bytes)
            self.streams[0].synchronize()
            return
        for s in self.streams:
            s.synchronize()

    # -- integrity plane ----------------------------------------------
    def integrity_check(self, seed: int) -> int:
        from .. import ops

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

    def digest_check(self, payload) -> int:
        """Per-message CRC32 of arbitrary content, sender vs receiver.
        The HBM side is digested by one crc32_messages launch, so only
        4 bytes per message ever cross back — no payload readback."""
        import zlib

        import numpy as np

        from .. import ops

        pay = self._payload_bytes(payload)
        pay_t = torch.from_numpy(pay)
        n, msg = self.msgs_per_region, self.msg_bytes
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

    def close(self) -> None:
        self.flush()
