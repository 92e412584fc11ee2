"""Transport interface: one-sided RDMA-write/read semantics.

A transport owns a *source* staging side and a *destination* region (the
"registered MR").  `post(i)` enqueues message i (size msg_bytes) toward
the destination at offset (i % msgs_per_region) * msg_bytes; `flush()`
waits for all outstanding messages — mirroring
ibv_post_send(IBV_WR_RDMA_WRITE) + CQ polling.  For `direction="read"`
the roles flip (region -> staging), mirroring RDMA READ.

`integrity_check()` proves the data path end to end: it moves the whole
region with deterministic per-message payloads and verifies the receiving
side (on-GPU via the CRC/verify kernels when the receiver is HBM) —
never inside a timed section.  `digest_check(payload)` does the same for
caller-supplied content: per-message CRC32 digests taken at the sender
and at the receiver are compared, like a NIC's per-message ICRC.

`icrc=True` (opt-in, backends that support it) checks the measured
traffic itself: `stamp()` records the CRC32 the sending side holds per
staging slot (write) or per region message (read), every message moved
afterwards is digested while it is moved and compared with its stamp,
and `icrc_stats()` reads the running {"checked", "bad"} counters.  The
inline digest is of the bytes as the engine loaded them; what landed in
the receiving memory is still proven by integrity_check/digest_check.
"""
from __future__ import annotations

import abc


class Transport(abc.ABC):
    name = "base"
    supports_icrc = False

    def __init__(self, msg_bytes: int, region_bytes: int,
                 inflight: int | None = 8, direction: str = "write",
                 icrc: bool = False, **_):
        if icrc and not self.supports_icrc:
            raise NotImplementedError(
                f"{self.name} transport does not implement icrc=True")
        if region_bytes % msg_bytes:
            raise ValueError("region must be a multiple of msg size")
        if direction not in ("write", "read"):
            raise ValueError(direction)
        if not inflight:
            inflight = 8
        self.msg_bytes = msg_bytes
        self.region_bytes = region_bytes
        self.inflight = max(1, min(inflight, region_bytes // msg_bytes))
        self.direction = direction
        self.icrc = bool(icrc)

    # -- data plane ----------------------------------------------------
    @abc.abstractmethod
    def post(self, i: int) -> None:
        """Enqueue message i (non-blocking where the backend allows)."""

    @abc.abstractmethod
    def flush(self) -> None:
        """Complete every outstanding message."""

    def post_many(self, start: int, n: int) -> None:
        """Enqueue messages start..start+n-1 (backends may vectorize the
        WQE writes; semantics identical to n post() calls)."""
        for i in range(start, start + n):
            self.post(i)

    # -- integrity plane (never timed) ---------------------------------
    @abc.abstractmethod
    def integrity_check(self, seed: int) -> int:
        """Move the whole region with pattern payloads; return mismatching
        8-byte words at the receiver (0 = intact)."""

    def digest_check(self, payload) -> int:
        """Payload-agnostic check: move the whole region carrying
        `payload` (any uint8 array of region_bytes, arbitrary content) in
        the same bursts as integrity_check; return the number of MESSAGES
        whose receiver CRC32 digest differs from the sender's (0 =
        intact).  Optional: backends without it raise."""
        raise NotImplementedError(
            f"{self.name} transport does not implement digest_check")

    # -- inline ICRC (icrc=True only) ----------------------------------
    def stamp(self) -> None:
        """Record the expected CRC32 of what the sending side holds now
        (staging slots for write, region messages for read).  Messages
        posted from here on are compared with it while they move; call
        it again after changing the sender's content.  integrity_check
        and digest_check rewrite the sender and drop the stamp."""
        raise NotImplementedError(
            f"{self.name} transport was not opened with icrc=True")

    def icrc_stats(self) -> dict:
        """{"checked": messages compared with their stamp so far,
        "bad": how many of them differed}."""
        raise NotImplementedError(
            f"{self.name} transport was not opened with icrc=True")

    def _payload_bytes(self, payload):
        """payload as a flat contiguous uint8 numpy array of region_bytes."""
        import numpy as np

        arr = np.ascontiguousarray(payload)
        if arr.dtype != np.uint8 or arr.size != self.region_bytes:
            raise ValueError(
                f"payload must be uint8 of {self.region_bytes} bytes")
        return arr.reshape(-1)

    def close(self) -> None:  # optional
        pass

    @property
    def msgs_per_region(self) -> int:
        return self.region_bytes // self.msg_bytes
