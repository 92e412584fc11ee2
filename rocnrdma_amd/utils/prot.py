"""Reference model of the protected message engines: MR keys, bounds,
access rights, completion status and queue-pair flush semantics.

Pure numpy and Python integers, written from the rules (docs/API.md,
"Memory protection") and not from the shared header: it is the oracle for
the CPU emulation of the scan kernel and for the GPU tier, and the fake
transport judges its posts with it.

An MR table is R rows (key, addr, length, access); access holds the
verbs bits and 0 marks a free row.  A key is slot << 8 | tag, slot < R.
"""
from __future__ import annotations

import numpy as np

WC_SUCCESS = 0
WC_LOC_LEN_ERR = 1
WC_LOC_PROT_ERR = 4
WC_WR_FLUSH_ERR = 5
WC_REM_ACCESS_ERR = 10

ACCESS_LOCAL_WRITE = 1
ACCESS_REMOTE_WRITE = 2
ACCESS_REMOTE_READ = 4

MAX_MR = 1 << 20
_M64 = (1 << 64) - 1


def make_key(slot: int, tag: int) -> int:
    """The key of MR-table row `slot` with the 8-bit `tag`."""
    if not 0 <= slot < MAX_MR:
        raise ValueError("slot must be in [0, 2^20)")
    if not 0 <= tag < 256:
        raise ValueError("tag must be in [0, 256)")
    return slot << 8 | tag


def pack_keys(lkey, rkey):
    """keys = lkey << 32 | rkey as int64 (scalars or arrays; the usual
    broadcasting).  Keys are below 2^28, so the word is non-negative."""
    lk = np.asarray(lkey, dtype=np.int64)
    rk = np.asarray(rkey, dtype=np.int64)
    if ((lk < 0) | (lk >> 32 != 0) | (rk < 0) | (rk >> 32 != 0)).any():
        raise ValueError("a key must fit 32 bits")
    out = (lk << 32) | rk
    return out if out.ndim else np.int64(out)


def _u64_list(x) -> list:
    """64-bit words of any signedness as non-negative Python integers."""
    return [int(v) & _M64 for v in np.asarray(x).reshape(-1).tolist()]


def _resolves(table, key: int, start: int, length: int, need: int) -> bool:
    """Does `key` name a row in use that holds exactly this key, contains
    [start, start + length) and grants every bit of `need`?  Exact
    integer arithmetic: a range that runs past 2^64 is in no MR."""
    slot = key >> 8
    if slot >= len(table):
        return False
    k, addr, size, access = table[slot]
    if access == 0 or k != key:
        return False
    if start < addr or start + length > addr + size:
        return False
    return access & need == need


def prot_reference(mrs, region_base, offs, addrs, lens, keys, gather,
                   qp_state=None):
    """(status, elens, qp_state_out) of one batch.

    status: int32 [n], values of enum ibv_wc_status.  elens: int64 [n],
    lens where status is WC_SUCCESS and 0 elsewhere.  qp_state: None =
    every message is judged on its own and qp_state_out is None;
    otherwise the word on entry (0 = ready) and qp_state_out the word
    afterwards."""
    tab = np.asarray(mrs).reshape(-1, 4)
    table = [tuple(int(v) & _M64 for v in row) for row in tab.tolist()]
    offs, addrs, keys = _u64_list(offs), _u64_list(addrs), _u64_list(keys)
    lens_s = [int(v) for v in np.asarray(lens).reshape(-1).tolist()]
    n = len(lens_s)
    if not (len(offs) == len(addrs) == len(keys) == n):
        raise ValueError("n mismatch")
    base = int(region_base) & _M64
    status = np.zeros(n, dtype=np.int32)
    for m in range(n):
        ln = lens_s[m]
        if ln >= 1 << 63:  # an unsigned view of a negative length
            ln -= 1 << 64
        if ln == 0:
            continue
        if ln < 0:
            status[m] = WC_LOC_LEN_ERR
            continue
        lkey, rkey = keys[m] >> 32, keys[m] & 0xFFFFFFFF
        if not _resolves(table, lkey, addrs[m], ln,
                         0 if gather else ACCESS_LOCAL_WRITE):
            status[m] = WC_LOC_PROT_ERR
            continue
        inside = (base + offs[m]) & _M64  # where the engine's pointer lands
        if not _resolves(table, rkey, inside, ln,
                         ACCESS_REMOTE_WRITE if gather
                         else ACCESS_REMOTE_READ):
            status[m] = WC_REM_ACCESS_ERR
    qp_out = None
    if qp_state is not None:
        qp_out = int(qp_state)
        failed = np.flatnonzero(status)
        if qp_out != 0:
            status[:] = WC_WR_FLUSH_ERR
            if n:
                qp_out = 1
        elif failed.size:
            status[failed[0] + 1:] = WC_WR_FLUSH_ERR
            qp_out = 1
    elens = np.where(status == WC_SUCCESS,
                     np.asarray(lens).reshape(-1).astype(np.int64), 0)
    return status, elens.astype(np.int64), qp_out
