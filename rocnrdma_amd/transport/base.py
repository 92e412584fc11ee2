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

`var_len=True` (opt-in, backends that support it) lets every post carry
its own byte count, as every verbs work request does: `msg_bytes`
becomes the slot size, message i still goes to region offset
(i % msgs_per_region) * msg_bytes and staging slot i % inflight, and
`post(i, nbytes)` / `post_many(start, n, nbytes)` move only the first
nbytes (0 <= nbytes <= msg_bytes, a multiple of 16) of the slot and of
the region message; the rest of both is untouched.
`digest_check(payload, lens)` audits such traffic, slack included.

`byte_granular=True` (opt-in on top of var_len=True, backends that
support it) removes the "16": nbytes may be any integer in range, and
the constructor arguments `region_skew` / `staging_skew` (each in
[0, 16), constant per transport) start message i that many bytes into
its region message and into its staging slot, so that the two sides may
be misaligned against each other by any amount.  nbytes + skew <=
msg_bytes holds on both sides; nbytes=None means the most that fits.
Only nbytes bytes move; the whole rest of the slot, in front of and
behind the message, is slack that digest_check(payload, lens) audits.
"""
from __future__ import annotations

import abc


class Transport(abc.ABC):
    name = "base"
    supports_icrc = False
    supports_var_len = False
    supports_byte_granular = False

    def __init__(self, msg_bytes: int, region_bytes: int,
                 inflight: int | None = 8, direction: str = "write",
                 icrc: bool = False, var_len: bool = False,
                 byte_granular: bool = False, region_skew: int = 0,
                 staging_skew: int = 0, **_):
        if icrc and not self.supports_icrc:
            raise NotImplementedError(
                f"{self.name} transport does not implement icrc=True")
        if byte_granular and not self.supports_byte_granular:
            raise NotImplementedError(
                f"{self.name} transport does not implement "
                "byte_granular=True")
        if var_len and not self.supports_var_len:
            raise NotImplementedError(
                f"{self.name} transport does not implement var_len=True")
        if byte_granular and not var_len:
            raise ValueError("byte_granular=True needs var_len=True: only "
                             "a post that carries its own byte count can "
                             "carry an odd one")
        for what, skew in (("region_skew", region_skew),
                           ("staging_skew", staging_skew)):
            if int(skew) != skew or not 0 <= skew < 16:
                raise ValueError(f"{what} must be an integer in [0, 16)")
            if skew and not byte_granular:
                raise ValueError(f"{what} needs byte_granular=True")
        if max(region_skew, staging_skew) >= msg_bytes:
            raise ValueError("skew leaves no room in a slot of msg_bytes")
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
        self.var_len = bool(var_len)
        self.byte_granular = bool(byte_granular)
        self.region_skew = int(region_skew)
        self.staging_skew = int(staging_skew)
        # the longest message a slot holds behind the larger skew
        self.max_nbytes = msg_bytes - max(self.region_skew,
                                          self.staging_skew)

    # -- data plane ----------------------------------------------------
    @abc.abstractmethod
    def post(self, i: int, nbytes: int | None = None) -> None:
        """Enqueue message i (non-blocking where the backend allows).
        nbytes (var_len=True only): this message's byte count, None =
        msg_bytes."""

    @abc.abstractmethod
    def flush(self) -> None:
        """Complete every outstanding message."""

    def post_many(self, start: int, n: int, nbytes=None) -> None:
        """Enqueue messages start..start+n-1 (backends may vectorize the
        WQE writes; semantics identical to n post() calls).  nbytes
        (var_len=True only): one byte count for all, or an integer array
        of n."""
        if nbytes is None:
            for i in range(start, start + n):
                self.post(i)
            return
        lens = self._lens(nbytes, n)
        for k in range(n):
            self.post(start + k, int(lens[k]))

    def _lens(self, nbytes, n: int):
        """nbytes of n posts as a validated int64 array (None = full
        slots): 0 <= nbytes <= msg_bytes, multiples of 16.  With
        byte_granular any integer 0 <= nbytes <= max_nbytes (msg_bytes
        less the larger skew; None = max_nbytes)."""
        import numpy as np

        if not self.var_len:
            raise ValueError(
                f"nbytes needs a transport opened with var_len=True "
                f"(this {self.name} transport moves msg_bytes per message)")
        if nbytes is None:
            return np.full(n, self.max_nbytes, dtype=np.int64)
        arr = np.asarray(nbytes)
        if arr.dtype.kind not in "iu":
            raise ValueError("nbytes must be integers")
        if arr.ndim == 0:
            arr = np.full(n, arr)
        elif arr.shape != (n,):
            raise ValueError(f"nbytes must be a scalar or {n} entries")
        if arr.dtype.kind == "u" and arr.size and int(arr.max()) > self.msg_bytes:
            raise ValueError("nbytes above msg_bytes")
        arr = arr.astype(np.int64)
        if self.byte_granular:
            if ((arr < 0) | (arr > self.max_nbytes)).any():
                raise ValueError(
                    f"nbytes must be in [0, {self.max_nbytes}] (msg_bytes "
                    "less the larger skew)")
            return arr
        if ((arr < 0) | (arr > self.msg_bytes) | (arr % 16 != 0)).any():
            raise ValueError(
                f"nbytes must be multiples of 16 in [0, {self.msg_bytes}]")
        return arr

    def _len1(self, nbytes) -> int:
        """_lens for one post, without numpy."""
        if nbytes is None:
            return self.max_nbytes
        if not self.var_len:
            self._lens(nbytes, 1)  # raises
        ln = int(nbytes)
        if self.byte_granular:
            if ln != nbytes or not 0 <= ln <= self.max_nbytes:
                raise ValueError(
                    f"nbytes must be in [0, {self.max_nbytes}] (msg_bytes "
                    "less the larger skew)")
            return ln
        if ln != nbytes or not 0 <= ln <= self.msg_bytes or ln % 16:
            raise ValueError(
                f"nbytes must be a multiple of 16 in [0, {self.msg_bytes}]")
        return ln

    # -- integrity plane (never timed) ---------------------------------
    @abc.abstractmethod
    def integrity_check(self, seed: int) -> int:
        """Move the whole region with pattern payloads; return mismatching
        8-byte words at the receiver (0 = intact)."""

    def digest_check(self, payload, lens=None) -> int:
        """Payload-agnostic check: move the whole region carrying
        `payload` (any uint8 array of region_bytes, arbitrary content) in
        the same bursts as integrity_check; return the number of MESSAGES
        whose receiver CRC32 digest differs from the sender's (0 =
        intact).  Optional: backends without it raise.

        lens (var_len=True only): message j carries payload[j * msg_bytes
        : j * msg_bytes + lens[j]]; None = full slots.  The receiving
        side is set to a known byte first and every slack range
        [j * msg_bytes + lens[j], (j + 1) * msg_bytes) must still hold
        it afterwards: a message is bad if its digest differs or its
        slack changed.  With byte_granular the sender holds those bytes
        at its skew and the slack is the whole slot outside
        [skew, skew + lens[j]), in front of and behind the message."""
        raise NotImplementedError(
            f"{self.name} transport does not implement digest_check")

    # -- inline ICRC (icrc=True only) ----------------------------------
    def stamp(self) -> None:
        """Record the expected CRC32 of what the sending side holds now
        (staging slots for write, region messages for read).  Messages
        posted from here on are compared with it while they move; call
        it again after changing the sender's content.  integrity_check
        and digest_check rewrite the sender and drop the stamp."""
        self._no_stamp_with_var_len()
        raise NotImplementedError(
            f"{self.name} transport was not opened with icrc=True")

    def icrc_stats(self) -> dict:
        """{"checked": messages compared with their stamp so far,
        "bad": how many of them differed}."""
        raise NotImplementedError(
            f"{self.name} transport was not opened with icrc=True")

    def _no_stamp_with_var_len(self) -> None:
        if self.var_len:
            raise NotImplementedError(
                "stamp() is not available with var_len=True: a stamp is "
                "one digest per slot (or region message), taken before "
                "the posts, and cannot know the length a later post will "
                "carry; icrc=True still serves digest_check(payload, lens)")

    def _no_pattern_with_skew(self) -> None:
        if self.region_skew or self.staging_skew:
            raise NotImplementedError(
                "integrity_check moves whole slots of the fill pattern; a "
                "transport with a skew is audited with "
                "digest_check(payload, lens)")

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
