#!/usr/bin/env python3
"""Scatter/gather-list engine against the byte-granular engine, one GPU.

Method as in tools/varlen_bench.py (whose measure() and fmt() this tool
uses): one process; every timing is a pair of device events around a
window of launches that ends in a synchronise; every shape is warmed up
first; the variants of a shape alternate inside each repeat; min /
median / max over the repeats.  Batch sizes are the sdma transport's.

1. one SGE per message through gather_sg_/scatter_sg_ against
   gather_bytes_/scatter_bytes_ on the same batches, crc off and on; the
   _bytes_ form is measured three times, the spread of its three medians
   is the noise;
2. header plus payload (64 B + 4 KiB, 64 B + 64 KiB) as two SGEs per
   message against the same bytes flattened into 2n gather_bytes_ /
   scatter_bytes_ messages with host-made offsets (which yields no
   whole-message digest);
3. one 1 MiB message cut into 1, 4 and 30 SGEs.

Usage: python tools/sgl_bench.py [--out profiles/sgl_1gpu.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rocnrdma_amd.ops as ops  # noqa: E402
from tools.varlen_bench import (MAX_BATCH, REPEATS, SIZES, STAGING,  # noqa: E402
                                batch_of, fmt, measure, time_ms)

HEADER = 64


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sgl_1gpu.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sgl_bench needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def dev64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    say(f"# tools/sgl_bench.py on {torch.cuda.get_device_name(dev)}; GB/s = "
        f"1e9 bytes/s moved (one direction), median [min .. max] of "
        f"{REPEATS} repeats, device events")
    slack = 2 << 20
    staging = torch.empty(STAGING + slack, dtype=torch.uint8, pin_memory=True)
    staging.numpy()[:] = np.random.default_rng(1).integers(
        0, 256, staging.numel(), dtype=np.uint8)
    region = torch.zeros(STAGING + slack, dtype=torch.uint8, device=dev)
    base = staging.data_ptr()
    assert base % 16 == 0 and region.data_ptr() % 16 == 0

    def flat(offs, addrs, lens, cap):
        """The four _bytes_ variants of one batch."""
        out = {}
        for name, fn in (("gather", ops.gather_bytes_),
                         ("scatter", ops.scatter_bytes_)):
            out[name] = lambda fn=fn: fn(region, offs, addrs, lens,
                                         max_msg_bytes=cap)
            out[name + "(crc)"] = lambda fn=fn: fn(
                region, offs, addrs, lens, max_msg_bytes=cap, crc=True)
        return out

    def lists(offs, start, addrs, lens, cap):
        """The four _sg_ variants of one batch."""
        out = {}
        for name, fn in (("gather", ops.gather_sg_),
                         ("scatter", ops.scatter_sg_)):
            out[name] = lambda fn=fn: fn(region, offs, start, addrs, lens,
                                         max_msg_bytes=cap)
            out[name + "(crc)"] = lambda fn=fn: fn(
                region, offs, start, addrs, lens, max_msg_bytes=cap,
                crc=True)
        return out

    # -- 1. one SGE per message ------------------------------------------
    say()
    say("## 1. one SGE per message: gather_sg_/scatter_sg_ against "
        "gather_bytes_/scatter_bytes_")
    say("_bytes_ is measured three times (a, b, c); noise = spread of its "
        "three medians; ratio = sg / median of the three")
    say(f"{'msg':>8} {'batch':>6} {'variant':<14} {'_bytes_ a/b/c GB/s':<26} "
        f"{'noise':>6} {'sg GB/s':>10}  {'[min .. max]':<20} ratio")
    for msg in SIZES:
        n = batch_of(msg)
        offs = dev64(np.arange(n) * msg)
        addrs = dev64(base + np.arange(n) * msg)
        lens = dev64(np.full(n, msg))
        old = flat(offs, addrs, lens, msg)
        new = lists(offs, dev64(np.arange(n + 1)), addrs, lens, msg)
        assert torch.equal(old["gather(crc)"](), new["gather(crc)"]())
        variants = {}
        for k in old:
            for rep in "abc":
                variants[f"{k}/b{rep}"] = old[k]
            variants[f"{k}/sg"] = new[k]
        rates = measure(variants, n * msg)
        for k in old:
            meds = [statistics.median(rates[f"{k}/b{rep}"]) for rep in "abc"]
            noise = max(meds) - min(meds)
            r = rates[f"{k}/sg"]
            ratio = statistics.median(r) / statistics.median(meds)
            say(f"{msg:>8} {n:>6} {k:<14} "
                f"{meds[0]:8.2f} {meds[1]:8.2f} {meds[2]:8.2f} "
                f"{noise:6.2f} {fmt(r)} {ratio:5.3f}")

    # what the scans cost: an all-zero batch through both
    n = MAX_BATCH
    offs, addrs = dev64(np.arange(n) * 64), dev64(base + np.arange(n) * 64)
    zeros, start = dev64(np.zeros(n)), dev64(np.arange(n + 1))
    for name, call in (
            ("gather_bytes_", lambda: ops.gather_bytes_(
                region, offs, addrs, zeros, max_msg_bytes=64)),
            ("gather_sg_", lambda: ops.gather_sg_(
                region, offs, start, addrs, zeros, max_msg_bytes=64))):
        call()
        torch.cuda.synchronize()
        t = [time_ms(call, 200) for _ in range(REPEATS)]
        say(f"scan + empty engine launch, {name}, n = {n} zero-length "
            f"messages of one SGE: {statistics.median(t) * 1e3:.1f} us per "
            f"call [{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")

    # -- 2. header + payload ---------------------------------------------
    say()
    say(f"## 2. header + payload: {HEADER} B + payload as two SGEs per "
        "message against the same bytes as 2n _bytes_ messages")
    say("headers and payloads come from two separate outside arrays and "
        "land back to back in the region; only the sg form returns a "
        "digest of the whole message")
    say(f"{'payload':>8} {'batch':>6} {'variant':<14} {'flat GB/s':>9}  "
        f"{'[min .. max]':<20} {'sg GB/s':>9}  {'[min .. max]':<20} ratio")
    for payload in (4 << 10, 64 << 10):
        whole = HEADER + payload
        n = batch_of(whole)
        assert n * whole <= STAGING
        k = np.arange(n)
        hdr_at = base + k * HEADER               # a header array in front
        pay_at = base + n * HEADER + k * payload  # the payloads behind it
        msg_at = k * whole
        f_offs = np.stack([msg_at, msg_at + HEADER], 1).reshape(-1)
        f_addrs = np.stack([hdr_at, pay_at], 1).reshape(-1)
        f_lens = np.tile([HEADER, payload], n)
        old = flat(dev64(f_offs), dev64(f_addrs), dev64(f_lens), payload)
        new = lists(dev64(msg_at), dev64(2 * np.arange(n + 1)),
                    dev64(f_addrs), dev64(f_lens), whole)
        variants = {}
        for name in old:
            variants[name + "/flat"] = old[name]
            variants[name + "/sg"] = new[name]
        rates = measure(variants, n * whole)
        for name in old:
            a, b = rates[name + "/flat"], rates[name + "/sg"]
            say(f"{payload:>8} {n:>6} {name:<14} {fmt(a)} {fmt(b)} "
                f"{statistics.median(b) / statistics.median(a):5.3f}")

    # -- 3. one long message, cut -------------------------------------------
    say()
    say("## 3. one 1 MiB message cut into 1, 4 and 30 SGEs (batch of "
        f"{batch_of(1 << 20)} such messages)")
    say(f"{'SGEs':>5} {'variant':<14} {'GB/s':>8}  {'[min .. max]':<20}")
    msg = 1 << 20
    n = batch_of(msg)
    for cuts in (1, 4, 30):
        edges = np.linspace(0, msg, cuts + 1).astype(np.int64)
        piece = np.diff(edges)
        at = (np.arange(n)[:, None] * msg + edges[None, :-1]).reshape(-1)
        new = lists(dev64(np.arange(n) * msg), dev64(cuts * np.arange(n + 1)),
                    dev64(base + at), dev64(np.tile(piece, n)), msg)
        rates = measure(new, n * msg)
        for name in new:
            say(f"{cuts:>5} {name:<14} {fmt(rates[name])}")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
