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

`max_sge=K` with K > 1 (opt-in on top of byte_granular=True with
staging_skew == 0, backends that support it) gives every post a
scatter/gather list, as a work request's sg_list: `post_sg(i, sges)`
takes up to K pairs (slot_off, nbytes), SGE k being the bytes
[slot_off, slot_off + nbytes) of staging slot i % inflight.  The message
is their concatenation in list order and sits at region offset
(i % msgs_per_region) * msg_bytes + region_skew.  A write gathers the
SGEs into that range, a read scatters the range over them (the SGEs of a
read may not overlap: they are written).  `post(i, nbytes)` is
`post_sg(i, [(0, nbytes)])` there, `post_many_sg(start, n, sges)` posts
n lists at once and `digest_check_sg(payload, sges)` audits such
traffic, the slack on the receiving side included.

`protected=True` (opt-in on top of byte_granular=True with max_sge == 1,
backends that support it) puts memory protection in front of every
message, as an HCA resolves lkey and rkey before it moves a byte.  The
transport registers two default MRs at open — the region
(REMOTE_READ | REMOTE_WRITE, `region_key`) and the staging area
(LOCAL_WRITE, `staging_key`) —, `reg_mr(side, offset, length, access)`
registers a window of either side and returns its key, `dereg_mr(key)`
frees it (the slot's next key carries another tag, so the old key is
stale).  `post(i, nbytes, rkey=..., lkey=...)` and `post_many` take the
keys a message is checked with (None = the default keys); the host does
not check ranges against MRs, the engine does.  Each message completes
with an `ibv_wc_status` value: `completions()` returns those of the last
flushed batch in post order, `prot_stats()` the running {"ok", "errors",
"flushed"} counts.  The transport is one queue pair: the first message
that fails puts it in the error state, everything posted behind it is
flushed (WR_FLUSH_ERR, no byte moved) until `reset_qp()`;
`qp_in_error()` reads the state.  digest_check and integrity_check run
through the protected engine with the default keys and count a message
that did not complete with SUCCESS as bad.
"""
from __future__ import annotations

import abc

KNOWN = 0x5A  # what digest_check(payload, lens) leaves in the slack


def _known_crc32(lens):
    """zlib's CRC32 of lens[m] KNOWN bytes for every m (uint32 numpy),
    computed once per distinct length."""
    import zlib

    import numpy as np

    crc = {int(k): zlib.crc32(bytes([KNOWN]) * int(k))
           for k in np.unique(lens)}
    return np.array([crc[int(k)] for k in lens], dtype=np.uint32)


class Transport(abc.ABC):
    """The ring contract, for every backend and every mode
    (tests/test_ring.py states it once more as a model and replays
    scripts against it):

    - Posts apply in post order.  Message i works on staging slot
      i % inflight and on region message i % msgs_per_region; the two
      moduli are independent.
    - The ring holds `inflight` posts.  A post into a full ring retires
      the ring first, exactly as flush() would; post_many(start, n) and
      post_many_sg are n posts, so they retire as often as they fill the
      ring, and a scalar post and a vectorized one fill the same ring.
    - flush() retires the pending posts: one batch.  flush() with nothing
      pending changes nothing, the last batch included.  stamp(),
      icrc_stats(), prot_stats(), qp_in_error(), reset_qp() and close()
      retire the ring as flush() does.
    - "Last batch" is the posts of the most recent retirement that had
      any, whether flush() or a full ring caused it, in post order:
      `_last_digests` (icrc) holds their inline digests, completions()
      (protected) their statuses.  After post_many(start, n); flush()
      with n > inflight that is the tail of the n posts, not all of them.
      Counters (icrc_stats, prot_stats) run over every retired post.
    - The destination rule: between two retirements no two posts may
      have the same destination — the staging slot for a read, the
      region message for a write —, and the sender's memory may not
      change between a post and the retirement that moves it.  The
      messages of one batch move concurrently (ops.gather_sg_ says so
      for the kernel), so the result of breaking the rule is undefined.
      Backends that move every post on its own (fake, sdma's stream
      engine) keep post order per destination anyway.
    """

    name = "base"
    supports_icrc = False
    supports_var_len = False
    supports_byte_granular = False
    supports_sg_list = False
    supports_protection = False

    def __init__(self, msg_bytes: int, region_bytes: int,
                 inflight: int | None = 8, direction: str = "write",
                 icrc: bool = False, var_len: bool = False,
                 byte_granular: bool = False, region_skew: int = 0,
                 staging_skew: int = 0, max_sge: int = 1,
                 protected: bool = False, max_mr: int = 16, **_):
        if protected and not self.supports_protection:
            raise NotImplementedError(
                f"{self.name} transport does not implement protected=True")
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
        if int(max_sge) != max_sge or max_sge < 1:
            raise ValueError("max_sge must be an integer >= 1")
        if max_sge > 1 and not self.supports_sg_list:
            raise NotImplementedError(
                f"{self.name} transport does not implement max_sge > 1")
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
        if max_sge > 1 and not byte_granular:
            raise ValueError("max_sge > 1 needs byte_granular=True: the "
                             "SGEs of a message have any length and meet "
                             "at any byte")
        if max_sge > 1 and staging_skew:
            raise ValueError("max_sge > 1 needs staging_skew == 0: every "
                             "SGE carries its own offset into the slot")
        if max(region_skew, staging_skew) >= msg_bytes:
            raise ValueError("skew leaves no room in a slot of msg_bytes")
        if protected and not byte_granular:
            raise ValueError("protected=True needs byte_granular=True: the "
                             "protected engine is the byte-granular one")
        if protected and max_sge > 1:
            raise ValueError("protected=True needs max_sge == 1: keys per "
                             "SGE are not implemented")
        if protected and (int(max_mr) != max_mr or
                          not 2 <= max_mr <= 1 << 20):
            raise ValueError("max_mr must be an integer in [2, 2^20]")
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
        self.max_sge = int(max_sge)
        self.protected = bool(protected)
        self.max_mr = int(max_mr)
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

    def post_many(self, start: int, n: int, nbytes=None, *, rkey=None,
                  lkey=None) -> None:
        """Enqueue messages start..start+n-1 (backends may vectorize the
        WQE writes; semantics identical to n post() calls).  nbytes
        (var_len=True only): one byte count for all, or an integer array
        of n.  rkey / lkey (protected=True only): one key for all, or an
        array of n; None = the default keys."""
        if rkey is not None or lkey is not None:
            keys = self._keys(rkey, lkey, n)
            lens = self._lens(nbytes, n)
            for k in range(n):
                self.post(start + k, int(lens[k]),
                          rkey=int(keys[k]) & 0xFFFFFFFF,
                          lkey=int(keys[k]) >> 32)
            return
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

    # -- memory protection (protected=True only) -----------------------
    def _prot_open(self, table, region_base: int, staging_base: int,
                   staging_bytes: int) -> None:
        """Start the MR table (a zeroed int64 array [max_mr, 4] the
        backend owns) with the two default MRs."""
        from ..utils import prot

        self._mr = table
        self._mr_tag = [0] * self.max_mr
        self._mr_dirty = True
        self._mr_sides = {"region": (region_base, self.region_bytes),
                          "staging": (staging_base, staging_bytes)}
        self.region_key = self.reg_mr(
            "region", 0, self.region_bytes,
            prot.ACCESS_REMOTE_READ | prot.ACCESS_REMOTE_WRITE)
        self.staging_key = self.reg_mr("staging", 0, staging_bytes,
                                       prot.ACCESS_LOCAL_WRITE)

    def _need_protected(self) -> None:
        if not self.protected:
            raise ValueError(
                f"this {self.name} transport was not opened with "
                "protected=True: it has no MR table and its posts carry "
                "no keys")

    def reg_mr(self, side: str, offset: int, length: int, access: int) -> int:
        """Register bytes [offset, offset + length) of the region
        (side="region") or of the staging area (side="staging") with the
        verbs access bits `access`; returns the key.  ValueError: a range
        outside that side, access == 0, a full table."""
        from ..utils import prot

        self._need_protected()
        if side not in self._mr_sides:
            raise ValueError('side must be "region" or "staging"')
        base, size = self._mr_sides[side]
        if (int(offset) != offset or int(length) != length or offset < 0
                or length < 0 or offset + length > size):
            raise ValueError(f"MR range outside the {side}")
        if int(access) != access or not 0 < access < 8:
            raise ValueError("access must be a non-empty set of the "
                             "LOCAL_WRITE, REMOTE_WRITE, REMOTE_READ bits")
        free = [r for r in range(self.max_mr) if self._mr[r, 3] == 0]
        if not free:
            raise ValueError(f"MR table full (max_mr = {self.max_mr})")
        slot = free[0]
        self._mr_tag[slot] = (self._mr_tag[slot] + 1) & 0xFF
        key = prot.make_key(slot, self._mr_tag[slot])
        self._mr[slot] = (key, base + int(offset), int(length), int(access))
        self._mr_dirty = True
        return key

    def dereg_mr(self, key: int) -> None:
        """Free the MR `key` names.  ValueError: no such MR."""
        self._need_protected()
        slot = int(key) >> 8
        if not (0 <= slot < self.max_mr and self._mr[slot, 3] != 0
                and self._mr[slot, 0] == key):
            raise ValueError(f"unknown MR key {key!r}")
        self._mr[slot] = 0
        self._mr_dirty = True

    def _keys(self, rkey, lkey, n: int):
        """The keys of n posts as an int64 array of lkey << 32 | rkey
        (None = the default key of that side)."""
        import numpy as np

        self._need_protected()
        cols = []
        for what, k, default in (("lkey", lkey, self.staging_key),
                                 ("rkey", rkey, self.region_key)):
            arr = np.asarray(default if k is None else k)
            if arr.dtype.kind not in "iu":
                raise ValueError(f"{what} must be integers")
            if arr.ndim == 0:
                arr = np.full(n, arr)
            elif arr.shape != (n,):
                raise ValueError(f"{what} must be a scalar or {n} entries")
            arr = arr.astype(np.int64)
            if ((arr < 0) | (arr >> 32 != 0)).any():
                raise ValueError(f"{what} must fit 32 bits")
            cols.append(arr)
        return (cols[0] << 32) | cols[1]

    def prot_expected(self, start: int, n: int, nbytes=None, *, rkey=None,
                      lkey=None, qp_state=0):
        """What the rules give for post_many(start, n, nbytes, rkey=...,
        lkey=...) against the MR table as it stands and a queue pair in
        state qp_state: (status, elens, qp_state_out) of
        utils.prot.prot_reference.  The model, not the engine."""
        import numpy as np

        from ..utils import prot

        keys = self._keys(rkey, lkey, n)
        lens = self._lens(nbytes, n)
        idx = np.arange(start, start + n, dtype=np.int64)
        offs = (idx % self.msgs_per_region) * self.msg_bytes + \
            self.region_skew
        addrs = (self._mr_sides["staging"][0] + self.staging_skew
                 + (idx % self.inflight) * self.msg_bytes)
        return prot.prot_reference(
            np.array(self._mr), self._mr_sides["region"][0], offs, addrs,
            lens, keys, self.direction == "write", qp_state=qp_state)

    def completions(self):
        """The ibv_wc_status of every message of the last flushed batch,
        in post order (int32 numpy array)."""
        self._need_protected()
        raise NotImplementedError

    def prot_stats(self) -> dict:
        """{"ok": messages completed with SUCCESS so far, "errors": with
        an error status of their own, "flushed": with WR_FLUSH_ERR}."""
        self._need_protected()
        raise NotImplementedError

    def qp_in_error(self) -> bool:
        """Has a message failed since open / the last reset_qp()?"""
        self._need_protected()
        raise NotImplementedError

    def reset_qp(self) -> None:
        """Leave the error state: messages posted from here on move."""
        self._need_protected()
        raise NotImplementedError

    # -- scatter/gather lists (max_sge > 1 only) -----------------------
    def post_sg(self, i: int, sges) -> None:
        """Enqueue message i as the concatenation of the staging-slot
        ranges sges: a sequence of at most max_sge pairs (slot_off,
        nbytes).  ValueError: too many SGEs, a range outside the slot, a
        negative or non-integer value, a total that does not fit behind
        region_skew, or (direction="read") SGEs that overlap."""
        self._sges(sges)
        raise NotImplementedError(
            f"{self.name} transport does not implement post_sg")

    def post_many_sg(self, start: int, n: int, sges) -> None:
        """Enqueue messages start..start+n-1 with the lists sges: an
        integer array of shape (n, max_sge, 2), unused entries of length
        0.  Semantics identical to n post_sg() calls."""
        arr = self._sges(sges, n)
        for k in range(n):
            self.post_sg(start + k, arr[k])

    def _sges(self, sges, n: int | None = None):
        """The lists of n posts (None: of one post, with at most max_sge
        entries) as a validated int64 array of shape (n, max_sge, 2) —
        (max_sge, 2) for one post —, unused entries (0, 0)."""
        import numpy as np

        if self.max_sge <= 1:
            raise ValueError(
                f"scatter/gather lists need a transport opened with "
                f"max_sge > 1 (this {self.name} transport posts one range "
                "per message)")
        K, msg = self.max_sge, self.msg_bytes
        try:
            arr = np.asarray(sges)
        except ValueError:
            raise ValueError("sges must be pairs (slot_off, nbytes)")
        if arr.size == 0 and n is None:
            arr = np.zeros((0, 2), dtype=np.int64)
        if arr.dtype.kind not in "iu":
            raise ValueError("sges must be integers")
        if n is None:
            if arr.ndim != 2 or arr.shape[1] != 2:
                raise ValueError("sges must be pairs (slot_off, nbytes)")
            if arr.shape[0] > K:
                raise ValueError(f"more than max_sge = {K} SGEs")
            full = np.zeros((1, K, 2), dtype=np.int64)
            full[0, :arr.shape[0]] = arr
            arr = full
        elif arr.shape != (n, K, 2):
            raise ValueError(f"sges must have shape ({n}, {K}, 2)")
        if arr.dtype.kind == "u" and arr.size and int(arr.max()) > msg:
            raise ValueError("an SGE outside the slot")
        arr = arr.astype(np.int64)
        off, ln = arr[..., 0], arr[..., 1]
        if (off < 0).any() or (ln < 0).any():
            raise ValueError("negative SGE offset or length")
        if (off + ln > msg).any():
            raise ValueError("an SGE outside the slot of msg_bytes")
        if (ln.sum(axis=1) + self.region_skew > msg).any():
            raise ValueError(
                f"a message of more than {msg - self.region_skew} bytes "
                "(msg_bytes less region_skew)")
        if self.direction == "read" and K > 1:
            # the SGEs of a read are written: sorted by offset, each must
            # end before the next one with bytes begins
            o = np.where(ln > 0, off, msg)  # empty ones last, out of the way
            order = np.argsort(o, axis=1, kind="stable")
            o = np.take_along_axis(o, order, axis=1)
            e = o + np.take_along_axis(ln, order, axis=1)
            if (e[:, :-1] > o[:, 1:]).any():
                raise ValueError("the SGEs of a read may not overlap")
        return arr[0] if n is None else arr

    def digest_check_sg(self, payload, sges) -> int:
        """digest_check for scatter/gather traffic: sges has shape
        (msgs_per_region, max_sge, 2).  Write: slot j is loaded with
        payload[j * msg_bytes : (j + 1) * msg_bytes], the receiver must
        hold the concatenation of the SGE ranges at its region_skew (HBM
        digests against host zlib) and the slack in front of and behind
        the message must still hold the known byte.  Read: the region
        message holds the first L_j payload bytes of its slot at
        region_skew, the slot is pre-filled with the known byte, and
        afterwards the SGE ranges must carry the pieces in order and
        every other slot byte must still be known.  Returns the number
        of bad messages."""
        pay = self._payload_bytes(payload)
        n = self.msgs_per_region
        sges = self._sges(sges, n)
        return int(self._audit(
            pay, sges, True,
            lambda i, b: self.post_many_sg(i, b, sges[i:i + b])).sum())

    # -- integrity plane (never timed) ---------------------------------
    # What a backend supplies to the checks below; one that supplies
    # none has post() and flush() only and overrides integrity_check.
    #   _slots                  the staging area as one host numpy view
    #                           (inflight, msg_bytes)
    #   _region_set(arr)        load the region from a host uint8 array
    #   _region_fill(byte)      set every region byte
    #   _region_get()           the region as a host uint8 array
    #   _region_digests(offs, lens, bound)
    #                           CRC32 of region[offs[m] : offs[m] + lens[m]]
    #                           for every m as uint32 numpy; lens <= bound
    #   _region_pattern(seed)   load the region with the fill pattern
    #   _region_mismatches(seed)
    #                           8-byte region words that differ from it
    #   _gather_host(batches)   the per-batch arrays flush() left (statuses
    #                           in _sink, digests in _last_digests), joined
    #                           into one host numpy array
    # and two attributes its flush() keeps: _last_digests (icrc: the
    # inline digests of the batch just flushed) and _sink (protected: when
    # it is a list, the statuses of every flushed batch are appended).
    def _no_checks(self, *_):
        raise NotImplementedError(
            f"{self.name} transport does not implement digest_check")

    _slots = property(_no_checks)
    _region_set = _region_fill = _region_get = _region_digests = _no_checks
    _region_pattern = _region_mismatches = _gather_host = _no_checks

    def _bursts(self):
        """(first message, count) of every burst of a walk over the
        region: the slots are reused, so a burst must complete before the
        next one loads them."""
        n = self.msgs_per_region
        for i in range(0, n, self.inflight):
            yield i, min(self.inflight, n - i)

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
            st = self._gather_host(self._sink)
        finally:
            self._sink = None
        return res, st != 0

    def integrity_check(self, seed: int) -> int:
        """Move the whole region with pattern payloads; return mismatching
        8-byte words at the receiver (0 = intact)."""
        import numpy as np

        from ..utils import pattern

        self._no_pattern_with_skew()
        if self.icrc:
            self._stamped = False  # the sender is rewritten below
        msg, slots = self.msg_bytes, self._slots
        ref = pattern.fill_reference(self.region_bytes, seed).reshape(-1, msg)
        write = self.direction == "write"

        def run():
            if not write:
                self._region_pattern(seed)
            bad = 0
            for i, burst in self._bursts():
                for j in range(i, i + burst):
                    if write:
                        slots[j % self.inflight] = ref[j]
                    self.post(j)
                self.flush()
                if not write:
                    for j in range(i, i + burst):
                        bad += int(np.count_nonzero(
                            slots[j % self.inflight].view(np.uint64)
                            != ref[j].view(np.uint64)))
            return self._region_mismatches(seed) if write else bad

        bad, rejected = self._rejected(run)
        return bad + int(np.sum(rejected))

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
        import numpy as np

        pay = self._payload_bytes(payload)
        n = self.msgs_per_region
        if self.var_len or lens is not None:
            lens = self._lens(lens, n)
            at = self.staging_skew

            def post(i, b):
                self.post_many(i, b, lens[i:i + b])
        else:  # whole slots: nothing of the receiver is slack
            lens, at, post = np.full(n, self.msg_bytes), 0, self.post_many
        pieces = np.stack([np.full(n, at), lens], axis=1)[:, None, :]
        return int(self._audit(pay, pieces, self.var_len, post).sum())

    def _audit(self, pay, pieces, slack: bool, post):
        """The one statement of digest_check and digest_check_sg.  Message
        j is the concatenation of the staging-slot ranges pieces[j] — an
        (n, K, 2) array of (slot_off, nbytes) — and sits in the region at
        j * msg_bytes + region_skew; post(i, b) posts messages i..i+b-1.
        Per burst: load and digest the sender slots (write) or set the
        slots to KNOWN (read, slack), post, flush() once, keep the inline
        digests (icrc), digest and inspect the received slots (read).  The
        far side is digested by the engine while it moves (icrc) or by
        _region_digests afterwards, so only 4 bytes per message come back
        from it.  With slack the receiver starts as KNOWN everywhere and
        every byte outside the message must still hold it: in a slot a
        compare, in the region the digest of the range against the CRC32
        of that many KNOWN bytes.  Returns the boolean array of bad
        messages: a digest differs, the slack changed, or (protected) the
        message did not complete with SUCCESS."""
        import zlib

        import numpy as np

        n, msg, ring = self.msgs_per_region, self.msg_bytes, self.inflight
        ss, rs = self.staging_skew, self.region_skew
        write = self.direction == "write"
        slots = self._slots
        lens = pieces[:, :, 1].sum(axis=1)
        offs = np.arange(n, dtype=np.int64) * msg + rs
        if self.icrc:
            self._stamped = False  # the sender is rewritten below
        if not write:  # the first L_j payload bytes of the slot, at the skew
            reg = pay.copy() if rs else pay
            for j in range(n if rs else 0):
                reg[offs[j]:offs[j] + lens[j]] = \
                    pay[j * msg:j * msg + lens[j]]
            self._region_set(reg)
        elif slack:
            self._region_fill(KNOWN)

        def digest(j):  # zlib over the concatenated pieces of the slot
            crc = 0
            for o, k in pieces[j]:
                crc = zlib.crc32(slots[j % ring][o:o + k], crc)
            return crc

        host = np.empty(n, dtype=np.uint32)
        bad = np.zeros(n, dtype=bool)
        inline = []

        def run():
            for i, burst in self._bursts():
                if write:
                    for j in range(i, i + burst):
                        slot = slots[j % ring]
                        slot[:] = pay[j * msg:(j + 1) * msg]
                        if ss:
                            slot[ss:ss + lens[j]] = \
                                pay[j * msg:j * msg + lens[j]]
                        host[j] = digest(j)
                elif slack:
                    slots[:burst] = KNOWN
                post(i, burst)
                self.flush()
                if self.icrc:
                    inline.append(self._last_digests)
                if not write:
                    for j in range(i, i + burst):
                        host[j] = digest(j)
                        if slack:
                            rest = np.ones(msg, dtype=bool)
                            for o, k in pieces[j]:
                                rest[o:o + k] = False
                            bad[j] = (slots[j % ring][rest] != KNOWN).any()

        _, rejected = self._rejected(run)
        if self.icrc:
            far = self._gather_host(inline).view(np.uint32)
        else:
            far = self._region_digests(offs, lens, msg)
        bad |= far != host
        if write and slack:
            behind = msg - rs - lens
            front = np.full(n, rs, dtype=np.int64)
            bad |= (self._region_digests(offs + lens, behind, msg)
                    != _known_crc32(behind))
            if rs:
                bad |= (self._region_digests(offs - rs, front, 16)
                        != _known_crc32(front))
        return bad | rejected

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
