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
    # every mode sdma has, moved with numpy, digested with zlib and judged
    # with utils.prot; the checks are the base class's, as sdma's are
    supports_icrc = True
    supports_var_len = True
    supports_byte_granular = True
    supports_sg_list = True
    supports_protection = True

    def __init__(self, msg_bytes: int, region_bytes: int, **kw):
        super().__init__(msg_bytes, region_bytes, **kw)
        self.staging = np.zeros((self.inflight, msg_bytes), dtype=np.uint8)
        self.region = np.zeros(region_bytes, dtype=np.uint8)
        self._pending = 0  # posts since the last retirement, <= inflight
        if self.icrc:
            self._stamped = False
            self._expected = None  # per slot (write) / per message (read)
            self._checked = self._bad = 0
            self._inline = []  # digests of the pending posts
            self._last_digests = None  # of the last flushed batch
        if self.protected:
            # the "addresses" the MRs and the posts speak of are those of
            # the two numpy buffers
            self._prot_open(np.zeros((self.max_mr, 4), dtype=np.int64),
                            self.region.ctypes.data,
                            self.staging.ctypes.data,
                            self.inflight * msg_bytes)
            self._qp = 0
            self._batch = []  # statuses of the pending posts
            self._last = np.zeros(0, dtype=np.int32)
            self._stats = {"ok": 0, "errors": 0, "flushed": 0}
            self._sink = None  # statuses of a running check, post order

    def post(self, i: int, nbytes: int | None = None, *, rkey=None,
             lkey=None) -> None:
        ln = self._len1(nbytes)
        self._ring()
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
        self._ring()
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

    def _ring(self) -> None:
        """Take one entry of the ring for a post (this backend moves the
        data in post(), the ring only decides what a batch is): a post
        into a full ring retires it first, as sdma's does."""
        if self._pending >= self.inflight:
            self.flush()
        self._pending += 1

    def _digest(self, i: int, src) -> None:
        """The inline ICRC: digest the bytes being moved, compare with
        the stamp if there is one."""
        crc = zlib.crc32(src.tobytes())
        self._inline.append(crc)
        if self._stamped:
            k = (i % self.inflight if self.direction == "write"
                 else i % self.msgs_per_region)
            self._checked += 1
            self._bad += int(crc != int(self._expected[k]))

    def _judge(self, i: int, off: int, ln: int, keys) -> bool:
        """The protected engine's verdict on one post, taken when it is
        posted (this backend moves data in post()); False = nothing
        moves."""
        from ..utils import prot

        addr = (self.staging.ctypes.data
                + (i % self.inflight) * self.msg_bytes + self.staging_skew)
        st, _, self._qp = prot.prot_reference(
            self._mr, self.region.ctypes.data, [off], [addr], [ln], keys,
            self.direction == "write", qp_state=self._qp)
        self._batch.append(int(st[0]))
        if st[0] != prot.WC_SUCCESS and self.icrc:
            self._inline.append(0)  # what the engine leaves for it
        return st[0] == prot.WC_SUCCESS

    def flush(self) -> None:  # synchronous backend
        if not self._pending:  # nothing to retire: the last batch stays
            return
        self._pending = 0
        if self.icrc:
            self._last_digests = np.array(self._inline, dtype=np.uint32)
            self._inline = []
        if self.protected:
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
        self.flush()
        return self._qp != 0

    def reset_qp(self) -> None:
        self._need_protected()
        self.flush()
        self._qp = 0

    def stamp(self) -> None:
        if not self.icrc or self.var_len:
            return super().stamp()
        self.flush()
        if self.direction == "write":
            self._expected = np.array(
                [zlib.crc32(s.tobytes()) for s in self.staging], np.uint32)
        else:
            self._expected = pattern.crc32_messages_reference(
                self.region, self.msg_bytes)
        self._stamped = True

    def icrc_stats(self) -> dict:
        if not self.icrc:
            return super().icrc_stats()
        self.flush()
        return {"checked": self._checked, "bad": self._bad}

    # -- integrity plane: what the checks of the base class work on -----
    @property
    def _slots(self):
        return self.staging

    def _region_set(self, arr) -> None:
        self.region[:] = arr

    _region_fill = _region_set  # numpy broadcasts the byte

    def _region_get(self):
        return self.region

    def _region_digests(self, offs, lens, bound: int):
        return pattern.crc32_messages_v_reference(self.region, offs, lens)

    def _region_pattern(self, seed: int) -> None:
        self.region[:] = pattern.fill_reference(self.region_bytes, seed)

    def _region_mismatches(self, seed: int) -> int:
        ref = pattern.fill_reference(self.region_bytes, seed)
        return int(np.count_nonzero(
            self.region.view(np.uint64) != ref.view(np.uint64)))

    def _gather_host(self, batches):
        return (np.concatenate(batches) if batches
                else np.zeros(0, dtype=np.int32))
