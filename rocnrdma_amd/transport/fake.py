"""CPU loopback transport: BASELINE config 1 ("host-malloc ibv_reg_mr +
ib_write_bw loopback") without hardware.  Used by the CPU test tier and
as the bench fallback where no GPU/HCA exists."""
from __future__ import annotations

import zlib

import numpy as np

from ..utils import pattern
from .base import Transport


class FakeTransport(Transport):
    name = "fake"
    supports_icrc = True  # zlib on the host: the sdma logic, CPU tier
    supports_var_len = True
    supports_byte_granular = True
    supports_sg_list = True  # numpy and zlib: the sdma logic, CPU tier
    supports_protection = True  # utils.prot: the sdma logic, CPU tier
    KNOWN = 0x5A  # what digest_check(payload, lens) leaves in the slack

    def __init__(self, msg_bytes: int, region_bytes: int, **kw):
        super().__init__(msg_bytes, region_bytes, **kw)
        self.staging = np.zeros((self.inflight, msg_bytes), dtype=np.uint8)
        self.region = np.zeros(region_bytes, dtype=np.uint8)
        if self.icrc:
            self._expected = None  # per slot (write) / per message (read)
            self._checked = self._bad = 0
            self._inline = None  # digests of a running digest_check
        if self.protected:
            # the "addresses" the MRs and the posts speak of are those of
            # the two numpy buffers; one ring of `inflight` posts per batch
            self._prot_open(np.zeros((self.max_mr, 4), dtype=np.int64),
                            self.region.ctypes.data,
                            self.staging.ctypes.data,
                            self.inflight * msg_bytes)
            self._qp = 0
            self._batch = []  # statuses of the posts since the last flush
            self._last = np.zeros(0, dtype=np.int32)
            self._stats = {"ok": 0, "errors": 0, "flushed": 0}
            self._sink = None  # statuses of a running check, post order

    def post(self, i: int, nbytes: int | None = None, *, rkey=None,
             lkey=None) -> None:
        ln = self._len1(nbytes)
        ss = self.staging_skew
        slot = self.staging[i % self.inflight][ss : ss + ln]
        off = (i % self.msgs_per_region) * self.msg_bytes + self.region_skew
        dst = self.region[off : off + ln]
        if self.protected or rkey is not None or lkey is not None:
            if not self._judge(i, off, ln, self._keys(rkey, lkey, 1)):
                return
        if self.icrc:
            self._digest(i, slot if self.direction == "write" else dst)
        if self.direction == "write":
            dst[:] = slot
        else:
            slot[:] = dst

    def post_sg(self, i: int, sges) -> None:
        sges = self._sges(sges)
        slot = self.staging[i % self.inflight]
        total = int(sges[:, 1].sum())
        off = (i % self.msgs_per_region) * self.msg_bytes + self.region_skew
        dst = self.region[off : off + total]
        if self.direction == "write":
            msg = np.concatenate([slot[o : o + k] for o, k in sges])
            if self.icrc:
                self._digest(i, msg)
            dst[:] = msg
            return
        if self.icrc:
            self._digest(i, dst)
        pos = 0
        for o, k in sges:
            slot[o : o + k] = dst[pos : pos + k]
            pos += k

    def _digest(self, i: int, src) -> None:
        """The inline ICRC: digest the bytes being moved, compare with
        the stamp if there is one."""
        crc = zlib.crc32(src.tobytes())
        if self._inline is not None:
            self._inline.append(crc)
        if self._expected is not None:
            k = (i % self.inflight if self.direction == "write"
                 else i % self.msgs_per_region)
            self._checked += 1
            self._bad += int(crc != int(self._expected[k]))

    def _judge(self, i: int, off: int, ln: int, keys) -> bool:
        """The protected engine's verdict on one post, taken when it is
        posted (this backend moves data in post()); False = nothing
        moves.  The ring is flushed when it is full, as sdma's is."""
        from ..utils import prot

        if len(self._batch) >= self.inflight:
            self.flush()
        addr = (self.staging.ctypes.data
                + (i % self.inflight) * self.msg_bytes + self.staging_skew)
        st, _, self._qp = prot.prot_reference(
            self._mr, self.region.ctypes.data, [off], [addr], [ln], keys,
            self.direction == "write", qp_state=self._qp)
        self._batch.append(int(st[0]))
        if st[0] != prot.WC_SUCCESS and self.icrc \
                and self._inline is not None:
            self._inline.append(0)  # what the engine leaves for it
        return st[0] == prot.WC_SUCCESS

    def flush(self) -> None:  # synchronous backend
        if self.protected and self._batch:
            from ..utils import prot

            st = np.array(self._batch, dtype=np.int32)
            self._batch = []
            self._last = st
            self._stats["ok"] += int((st == prot.WC_SUCCESS).sum())
            self._stats["flushed"] += int((st == prot.WC_WR_FLUSH_ERR).sum())
            self._stats["errors"] += int(
                ((st != prot.WC_SUCCESS) & (st != prot.WC_WR_FLUSH_ERR)).sum())
            if self._sink is not None:
                self._sink.append(st)

    def completions(self):
        self._need_protected()
        return self._last.copy()

    def prot_stats(self) -> dict:
        self._need_protected()
        self.flush()
        return dict(self._stats)

    def qp_in_error(self) -> bool:
        self._need_protected()
        return self._qp != 0

    def reset_qp(self) -> None:
        self._need_protected()
        self.flush()
        self._qp = 0

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
            st = (np.concatenate(self._sink) if self._sink
                  else np.zeros(0, dtype=np.int32))
        finally:
            self._sink = None
        return res, st != 0

    def stamp(self) -> None:
        if not self.icrc or self.var_len:
            return super().stamp()
        if self.direction == "write":
            self._expected = np.array(
                [zlib.crc32(s.tobytes()) for s in self.staging], np.uint32)
        else:
            self._expected = pattern.crc32_messages_reference(
                self.region, self.msg_bytes)

    def icrc_stats(self) -> dict:
        if not self.icrc:
            return super().icrc_stats()
        return {"checked": self._checked, "bad": self._bad}

    def integrity_check(self, seed: int) -> int:
        bad, rejected = self._rejected(lambda: self._integrity_check(seed))
        return bad + int(np.sum(rejected))

    def _integrity_check(self, seed: int) -> int:
        self._no_pattern_with_skew()
        if self.icrc:
            self._expected = None  # the sender is rewritten below
        ref = pattern.fill_reference(self.region_bytes, seed)
        if self.direction == "write":
            for i in range(self.msgs_per_region):
                off = i * self.msg_bytes
                self.staging[i % self.inflight][:] = ref[off : off + self.msg_bytes]
                self.post(i)
            self.flush()
            got = self.region
            return int(
                np.count_nonzero(
                    got.view(np.uint64) != ref.view(np.uint64)))
        # read: pattern the region, pull into staging slot by slot
        self.region[:] = ref
        bad = 0
        for i in range(self.msgs_per_region):
            self.post(i)
            self.flush()
            off = i * self.msg_bytes
            bad += int(
                np.count_nonzero(
                    self.staging[i % self.inflight].view(np.uint64)
                    != ref[off : off + self.msg_bytes].view(np.uint64)))
        return bad

    def digest_check(self, payload, lens=None) -> int:
        pay = self._payload_bytes(payload)
        n, msg = self.msgs_per_region, self.msg_bytes
        if self.var_len or lens is not None:
            lens = self._lens(lens, n)
            bad, rejected = self._rejected(
                lambda: self._digest_check_var(pay, lens))
            return int((bad | rejected).sum())
        if self.icrc:
            # the region-side digests come from the inline ICRC of the
            # transfer itself, not from a second pass over the region
            self._expected = None
            self._inline = []
        try:
            if self.direction == "write":
                sent = []
                for i in range(n):
                    slot = self.staging[i % self.inflight]
                    slot[:] = pay[i * msg : (i + 1) * msg]
                    sent.append(zlib.crc32(slot.tobytes()))
                    self.post(i)
                self.flush()
                if self.icrc:
                    got = np.array(self._inline, np.uint32)
                else:
                    got = pattern.crc32_messages_reference(self.region, msg)
                return int(np.count_nonzero(got != np.array(sent, np.uint32)))
            # read: load the region, digest it, pull slot by slot
            self.region[:] = pay
            if not self.icrc:
                sent = pattern.crc32_messages_reference(self.region, msg)
            bad = 0
            for i in range(n):
                self.post(i)
                self.flush()
                got = zlib.crc32(self.staging[i % self.inflight].tobytes())
                want = self._inline[i] if self.icrc else int(sent[i])
                bad += int(got != want)
            return bad
        finally:
            if self.icrc:
                self._inline = None

    def _digest_check_var(self, pay, lens) -> int:
        """digest_check for per-message lengths: digests of the lens[j]
        bytes at the skew (0 unless byte_granular), and the receiver's
        slack — the slot outside the message — must keep KNOWN.  Returns
        the boolean array of bad messages."""
        n, msg = self.msgs_per_region, self.msg_bytes
        ss, rs = self.staging_skew, self.region_skew
        write = self.direction == "write"
        if self.icrc:
            self._expected = None
            self._inline = []
        try:
            bad = np.zeros(n, dtype=bool)
            if write:
                self.region[:] = self.KNOWN
                sent = np.empty(n, dtype=np.uint32)
                for i in range(n):
                    slot = self.staging[i % self.inflight]
                    slot[:] = pay[i * msg : (i + 1) * msg]
                    slot[ss : ss + lens[i]] = pay[i * msg : i * msg + lens[i]]
                    sent[i] = zlib.crc32(slot[ss : ss + lens[i]].tobytes())
                    self.post(i, int(lens[i]))
                self.flush()
                offs = np.arange(n, dtype=np.int64) * msg + rs
                if self.icrc:
                    got = np.array(self._inline, np.uint32)
                else:
                    got = pattern.crc32_messages_v_reference(
                        self.region, offs, lens)
                bad |= got != sent
                for i in range(n):
                    slot = self.region[i * msg : (i + 1) * msg]
                    bad[i] |= bool((slot[:rs] != self.KNOWN).any() or
                                   (slot[rs + lens[i]:] != self.KNOWN).any())
                return bad
            # read: load the region, pull every message into a slot that
            # holds KNOWN, digest and inspect the slot
            self.region[:] = pay
            if rs:
                for i in range(n):
                    self.region[i * msg + rs : i * msg + rs + lens[i]] = \
                        pay[i * msg : i * msg + lens[i]]
            for i in range(n):
                slot = self.staging[i % self.inflight]
                slot[:] = self.KNOWN
                self.post(i, int(lens[i]))
                self.flush()
                ln = int(lens[i])
                got = zlib.crc32(slot[ss : ss + ln].tobytes())
                want = (self._inline[i] if self.icrc else
                        zlib.crc32(pay[i * msg : i * msg + ln].tobytes()))
                bad[i] = (got != want or
                          bool((slot[:ss] != self.KNOWN).any()) or
                          bool((slot[ss + ln:] != self.KNOWN).any()))
            return bad
        finally:
            if self.icrc:
                self._inline = None

    def digest_check_sg(self, payload, sges) -> int:
        pay = self._payload_bytes(payload)
        n, msg, rs = self.msgs_per_region, self.msg_bytes, self.region_skew
        sges = self._sges(sges, n)
        lens = sges[:, :, 1].sum(axis=1)
        write = self.direction == "write"
        if self.icrc:
            self._expected = None
            self._inline = []
        try:
            bad = np.zeros(n, dtype=bool)
            if write:
                self.region[:] = self.KNOWN
            else:  # the first L_j payload bytes of the slot, at the skew
                self.region[:] = pay
                for i in range(n):
                    self.region[i * msg + rs : i * msg + rs + lens[i]] = \
                        pay[i * msg : i * msg + lens[i]]
            for i in range(n):
                slot = self.staging[i % self.inflight]
                slot[:] = pay[i * msg : (i + 1) * msg] if write else self.KNOWN
                self.post_sg(i, sges[i])
                self.flush()
                ln = int(lens[i])
                pieces = np.concatenate([slot[o : o + k] for o, k in sges[i]])
                host = zlib.crc32(pieces.tobytes())
                if write:
                    there = self.region[i * msg : (i + 1) * msg]
                    got = (self._inline[i] if self.icrc else
                           zlib.crc32(there[rs : rs + ln].tobytes()))
                    bad[i] = (got != host or
                              bool((there[:rs] != self.KNOWN).any()) or
                              bool((there[rs + ln:] != self.KNOWN).any()))
                else:
                    want = (self._inline[i] if self.icrc else
                            zlib.crc32(pay[i * msg : i * msg + ln].tobytes()))
                    rest = np.ones(msg, dtype=bool)
                    for o, k in sges[i]:
                        rest[o : o + k] = False
                    bad[i] = (host != want or
                              bool((slot[rest] != self.KNOWN).any()))
            return int(bad.sum())
        finally:
            if self.icrc:
                self._inline = None
