"""Soak / stress: randomized message sizes, directions and burst
shapes against one region, with periodic full CRC audits — the
stability tier for production deployment (run for minutes/hours on a
deploy candidate; the GPU test tier runs a short bounded pass).

CLI: python -m rocnrdma_amd.harness.soak [--secs 30] [--transport auto]
                                         [--audit pattern|crc] [--mixed]
                                         [--bytes] [--sg K] [--prot]
Exit nonzero on any integrity failure.
"""
from __future__ import annotations

import argparse
import random
import time

SIZES = [4 << 10, 16 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20]


def mixed_lens(rng: random.Random, n: int, msg: int, unit: int = 16):
    """n seeded message lengths for a slot of msg bytes: multiples of 16
    in [0, msg], with mass on 0, 16, msg and just around the 4096-byte
    chunk boundaries, where the engine changes path.  unit=1 (--bytes)
    draws from all byte counts instead, with the mass on 0, 1, msg and
    one byte either side of the boundaries."""
    import numpy as np

    g = np.random.default_rng(rng.getrandbits(32))
    lens = g.integers(0, msg // unit + 1, n, dtype=np.int64) * unit
    kind = g.random(n)
    lens[kind < 0.10] = 0
    lens[(kind >= 0.10) & (kind < 0.20)] = unit
    lens[(kind >= 0.20) & (kind < 0.35)] = msg
    edge = (kind >= 0.35) & (kind < 0.55)
    near = (g.integers(1, max(msg // 4096, 1) + 1, n, dtype=np.int64) * 4096
            + g.integers(-1, 2, n, dtype=np.int64) * unit)
    lens[edge] = np.clip(near, 0, msg)[edge]
    return lens


def mixed_sges(rng: random.Random, n: int, msg: int, max_sge: int,
               room: int, disjoint: bool):
    """n seeded scatter/gather lists for a slot of msg bytes, as an
    int64 array (n, max_sge, 2) of (slot_off, nbytes): every list has a
    seeded number of SGEs in [0, max_sge] (the others stay at length 0,
    anywhere in the list), their lengths are a seeded cut of a
    mixed_lens total of at most room bytes — so empty and 1-byte SGEs
    and whole-slot messages all occur — and their offsets are seeded:
    disjoint ranges in a shuffled order of the slot (what a read needs),
    or anywhere in the slot, overlaps included."""
    import numpy as np

    g = np.random.default_rng(rng.getrandbits(32))
    total = mixed_lens(rng, n, room, 1)
    sges = np.zeros((n, max_sge, 2), dtype=np.int64)
    for i in range(n):
        used = np.sort(g.permutation(max_sge)[:g.integers(0, max_sge + 1)])
        if not used.size:
            continue
        cuts = np.sort(g.integers(0, total[i] + 1, used.size - 1))
        if used.size > 1 and g.random() < 0.3:
            cuts[0] = min(1, total[i])  # a 1-byte SGE in front
            cuts.sort()
        lens = np.diff(np.concatenate([[0], cuts, [total[i]]]))
        sges[i, used, 1] = lens
        if disjoint:
            # spread the free bytes of the slot over the gaps, then lay
            # the SGEs out in a shuffled order
            order = g.permutation(used.size)
            gaps = np.diff(np.concatenate(
                [[0], np.sort(g.integers(0, msg - total[i] + 1, used.size))]))
            at = np.cumsum(gaps + np.concatenate([[0], lens[order][:-1]]))
            sges[i, used[order], 0] = at
        else:
            sges[i, used, 0] = g.integers(0, msg - lens + 1)
    return sges


def run_soak(transport: str = "auto", secs: float = 10.0,
             region_bytes: int = 256 << 20, seed: int = 1234,
             device=None, metrics=None, audit: str = "pattern",
             icrc: bool = False, mixed: bool = False,
             byte_granular: bool = False, sg: int = 0,
             prot: bool = False) -> dict:
    """audit="pattern": splitmix64 pattern + integrity_check (default).
    audit="crc": a seeded random payload per cycle through digest_check
    (per-message CRC32, content-independent).
    icrc=True: the burst phase runs on a patterned, stamped sender with
    every message's CRC32 checked inline; a cycle with a bad message is
    a failure, and the stats gain icrc_checked / icrc_bad.
    mixed=True: every cycle opens the transport with var_len=True at a
    slot size from SIZES, posts its bursts with seeded random lengths
    (mixed_lens) and audits with digest_check(payload, lens), slack
    included; msgs and bytes count what was actually moved.  A stamp
    cannot serve variable lengths, so with icrc=True the inline digests
    are used by the audit only.
    byte_granular=True (needs mixed): the transport is opened with
    byte_granular=True and a seeded region_skew / staging_skew per cycle,
    and the lengths are drawn from all byte counts that fit.
    sg=K > 1 (needs byte_granular): the transport is opened with
    max_sge=K and staging_skew 0, every post carries a seeded
    scatter/gather list (mixed_sges) and the audit is
    digest_check_sg(payload, sges).
    prot=True (needs byte_granular, not sg): the transport is opened with
    protected=True; every cycle registers a seeded window MR and posts
    bursts in which a seeded minority of the messages use the window key
    outside its range, a deregistered key or a key without the needed
    right.  completions() is compared with the model
    (utils.prot.prot_reference), rejected and flushed messages must have
    left the known byte in place and accepted ones must have landed;
    reset_qp() runs between bursts and the audit follows with the
    default keys."""
    from rocnrdma_amd.harness.sweep import pattern_sender
    from rocnrdma_amd.transport import get_transport

    if audit not in ("pattern", "crc"):
        raise ValueError(f"audit must be 'pattern' or 'crc', not {audit!r}")
    if byte_granular and not mixed:
        raise ValueError("byte_granular=True needs mixed=True")

    if sg and sg < 2:
        raise ValueError("sg must be 0 (off) or a max_sge of at least 2")
    if sg and not byte_granular:
        raise ValueError("sg needs mixed=True and byte_granular=True")

    if prot and (not byte_granular or sg):
        raise ValueError("prot needs mixed=True and byte_granular=True, "
                         "and no sg")

    if metrics is None:
        from rocnrdma_amd.utils.metrics import TransferMetrics

        metrics = TransferMetrics(port=None)
    rng = random.Random(seed)
    t_end = time.monotonic() + secs
    stats = {"cycles": 0, "msgs": 0, "bytes": 0, "audits": 0,
             "failures": 0}
    extra = {}
    if icrc:
        extra["icrc"] = True
        stats.update(icrc_checked=0, icrc_bad=0)
    if mixed:
        extra["var_len"] = True
    if prot:
        extra["protected"] = True
        stats.update(prot_rejected=0, prot_flushed=0)
    while time.monotonic() < t_end:
        msg = rng.choice(SIZES)
        direction = rng.choice(["write", "read"])
        region = max(region_bytes // msg, 1) * msg
        if byte_granular:
            extra.update(byte_granular=True, region_skew=rng.randrange(16),
                         staging_skew=rng.randrange(16))
        if sg:
            extra.update(max_sge=sg, staging_skew=0)
        tp = get_transport(transport, msg_bytes=msg, region_bytes=region,
                           direction=direction, device=device, **extra)
        try:
            if mixed:
                if prot:
                    moved, msgs, bad = _prot_cycle(tp, rng, region, stats)
                else:
                    moved, msgs, bad = _mixed_cycle(tp, rng, region)
                stats["audits"] += 1
                if bad:
                    stats["failures"] += 1
                stats["msgs"] += msgs
                stats["bytes"] += moved
                stats["cycles"] += 1
                metrics.observe_bytes(direction, moved, msgs)
                metrics.observe_audit(ok=bad == 0)
                continue
            if icrc:
                pattern_sender(tp, seed=rng.getrandbits(32))
                tp.stamp()
            # a few random bursts (bandwidth phase; content irrelevant
            # unless stamped)
            posted = 0
            for _ in range(rng.randint(1, 4)):
                burst = rng.randint(1, max(2, tp.inflight))
                tp.post_many(posted, burst)
                posted += burst
                tp.flush()
            if icrc:
                st = tp.icrc_stats()
                stats["icrc_checked"] += st["checked"]
                stats["icrc_bad"] += st["bad"]
                if st["bad"]:
                    stats["failures"] += 1
            # audit: full-region transfer + receiver verify
            if audit == "crc":
                import numpy as np

                payload = np.random.default_rng(
                    rng.getrandbits(32)).integers(
                        0, 256, region, dtype=np.uint8)
                bad = tp.digest_check(payload)
            else:
                bad = tp.integrity_check(seed=rng.getrandbits(32))
            stats["audits"] += 1
            if bad:
                stats["failures"] += 1
            moved = (posted + tp.msgs_per_region) * msg
            stats["msgs"] += posted + tp.msgs_per_region
            stats["bytes"] += moved
            stats["cycles"] += 1
            metrics.observe_bytes(direction, moved,
                                  posted + tp.msgs_per_region)
            metrics.observe_audit(ok=bad == 0)
        finally:
            tp.close()
    return stats


def _mixed_cycle(tp, rng: random.Random, region: int):
    """One mixed-length cycle on an open var_len transport: (bytes
    moved, messages moved, bad messages of the audit)."""
    import numpy as np

    if tp.max_sge > 1:
        return _sg_cycle(tp, rng, region)
    unit = 1 if tp.byte_granular else 16
    moved = posted = 0
    for _ in range(rng.randint(1, 4)):
        burst = rng.randint(1, max(2, tp.inflight))
        lens = mixed_lens(rng, burst, tp.max_nbytes, unit)
        tp.post_many(posted, burst, lens)
        posted += burst
        moved += int(lens.sum())
        tp.flush()
    payload = np.random.default_rng(rng.getrandbits(32)).integers(
        0, 256, region, dtype=np.uint8)
    lens = mixed_lens(rng, tp.msgs_per_region, tp.max_nbytes, unit)
    bad = tp.digest_check(payload, lens)
    return (moved + int(lens.sum()), posted + tp.msgs_per_region, bad)


_PROT_KNOWN = 0x3C  # what a receiver holds before a protected burst


def _prot_cycle(tp, rng: random.Random, region: int, stats: dict):
    """One cycle of hostile traffic on an open protected transport:
    (bytes moved, messages moved, bad messages).  Bad: a completion that
    differs from the model's, a rejected or flushed message whose
    receiver lost the known byte, an accepted one that did not land, and
    whatever the closing audit finds."""
    import numpy as np

    from rocnrdma_amd.utils import prot as P

    msg, mpr, inflight = tp.msg_bytes, tp.msgs_per_region, tp.inflight
    rs, ss = tp.region_skew, tp.staging_skew
    write = tp.direction == "write"
    staging = tp._slots
    g = np.random.default_rng(rng.getrandbits(32))
    # the window: a run of whole region messages, every right granted
    w0 = rng.randrange(mpr)
    w1 = rng.randint(w0 + 1, mpr)
    window = tp.reg_mr("region", w0 * msg, (w1 - w0) * msg,
                       P.ACCESS_REMOTE_READ | P.ACCESS_REMOTE_WRITE)
    weak = tp.reg_mr("region", 0, region,  # the right this direction lacks
                     P.ACCESS_REMOTE_READ if write else P.ACCESS_REMOTE_WRITE)
    stale = tp.reg_mr("region", 0, region,
                      P.ACCESS_REMOTE_READ | P.ACCESS_REMOTE_WRITE)
    tp.dereg_mr(stale)
    moved = posted = bad = 0
    for _ in range(rng.randint(1, 4)):
        burst = min(rng.randint(1, max(2, inflight)), inflight)
        lens = mixed_lens(rng, burst, tp.max_nbytes, 1)
        idx = np.arange(posted, posted + burst)
        rkeys = np.full(burst, tp.region_key, dtype=np.int64)
        hostile = g.random(burst) < min(0.25, 2.0 / burst)
        rkeys[hostile] = g.choice([window, weak, stale], int(hostile.sum()))
        friendly = ~hostile & (g.random(burst) < 0.3)
        rkeys[friendly] = window  # in range or not: the model knows
        # sender random, receiver known
        data = g.integers(0, 256, (burst, msg), dtype=np.uint8)
        reg = np.full(region, _PROT_KNOWN, dtype=np.uint8)
        slots, rmsg = idx % inflight, idx % mpr
        if write:
            staging[slots] = data
        else:
            staging[slots] = _PROT_KNOWN
            for k in range(burst):
                reg[rmsg[k] * msg:(rmsg[k] + 1) * msg] = data[k]
        tp._region_set(reg)
        want, elens, _ = tp.prot_expected(posted, burst, lens, rkey=rkeys)
        tp.post_many(posted, burst, lens, rkey=rkeys)
        tp.flush()
        got = tp.completions()
        mism = np.zeros(burst, dtype=bool)
        if got.shape != want.shape:
            mism[:] = True
        else:
            mism |= got != want
        reg = tp._region_get()
        for k in range(burst):
            ln = int(elens[k])
            there = reg[rmsg[k] * msg:(rmsg[k] + 1) * msg]
            slot = staging[slots[k]]
            recv, sent = ((there, slot[ss:ss + ln]) if write
                          else (slot, there[rs:rs + ln]))
            at = rs if write else ss
            mism[k] |= bool((recv[:at] != _PROT_KNOWN).any() or
                            (recv[at:at + ln] != sent).any() or
                            (recv[at + ln:] != _PROT_KNOWN).any())
        bad += int(mism.sum())
        stats["prot_rejected"] += int(
            ((want != P.WC_SUCCESS) & (want != P.WC_WR_FLUSH_ERR)).sum())
        stats["prot_flushed"] += int((want == P.WC_WR_FLUSH_ERR).sum())
        moved += int(elens.sum())
        posted += burst
        tp.reset_qp()
    tp.dereg_mr(window)
    tp.dereg_mr(weak)
    payload = g.integers(0, 256, region, dtype=np.uint8)
    lens = mixed_lens(rng, mpr, tp.max_nbytes, 1)
    bad += tp.digest_check(payload, lens)
    return (moved + int(lens.sum()), posted + mpr, bad)


def _sg_cycle(tp, rng: random.Random, region: int):
    """_mixed_cycle with a seeded scatter/gather list per message."""
    import numpy as np

    room = tp.msg_bytes - tp.region_skew
    disjoint = tp.direction == "read"  # the side that is written
    moved = posted = 0
    for _ in range(rng.randint(1, 4)):
        burst = rng.randint(1, max(2, tp.inflight))
        sges = mixed_sges(rng, burst, tp.msg_bytes, tp.max_sge, room,
                          disjoint)
        tp.post_many_sg(posted, burst, sges)
        posted += burst
        moved += int(sges[:, :, 1].sum())
        tp.flush()
    payload = np.random.default_rng(rng.getrandbits(32)).integers(
        0, 256, region, dtype=np.uint8)
    sges = mixed_sges(rng, tp.msgs_per_region, tp.msg_bytes, tp.max_sge,
                      room, disjoint)
    bad = tp.digest_check_sg(payload, sges)
    return (moved + int(sges[:, :, 1].sum()), posted + tp.msgs_per_region,
            bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--secs", type=float, default=30.0)
    ap.add_argument("--transport", default="auto")
    ap.add_argument("--region-bytes", type=int, default=256 << 20)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--audit", choices=["pattern", "crc"],
                    default="pattern",
                    help="pattern: splitmix64 + verify; crc: random "
                         "payload + per-message CRC32 digests")
    ap.add_argument("--icrc", action="store_true",
                    help="run the burst phase stamped, every message's "
                         "CRC32 checked inline")
    ap.add_argument("--mixed", action="store_true",
                    help="variable-length traffic: var_len transport, "
                         "seeded random lengths per message, audited "
                         "with digest_check(payload, lens)")
    ap.add_argument("--bytes", action="store_true", dest="byte_granular",
                    help="with --mixed: byte-granular traffic, lengths "
                         "from all byte counts (not multiples of 16) at a "
                         "random skew per side")
    ap.add_argument("--sg", type=int, default=0, metavar="K",
                    help="with --mixed --bytes: scatter/gather traffic, "
                         "up to K SGEs per message in seeded layouts, "
                         "audited with digest_check_sg")
    ap.add_argument("--prot", action="store_true",
                    help="with --mixed --bytes: protected traffic, a "
                         "seeded minority of the messages with keys that "
                         "must be rejected; completions are compared with "
                         "the model and rejected messages must move nothing")
    ap.add_argument("--metrics-port", type=int, default=0,
                    help="expose Prometheus metrics on this port")
    args = ap.parse_args()
    from rocnrdma_amd.utils.metrics import TransferMetrics

    metrics = TransferMetrics(port=args.metrics_port or None)
    stats = run_soak(args.transport, args.secs, args.region_bytes,
                     args.seed, metrics=metrics, audit=args.audit,
                     icrc=args.icrc, mixed=args.mixed,
                     byte_granular=args.byte_granular, sg=args.sg,
                     prot=args.prot)
    print(stats)
    raise SystemExit(1 if stats["failures"] else 0)


if __name__ == "__main__":
    main()
