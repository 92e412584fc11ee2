#!/usr/bin/env python3
"""What memory protection costs: gather_prot_ / scatter_prot_ with every
message valid against gather_bytes_ / scatter_bytes_, one GPU.

One process; every timing is a pair of device events around ITERS
launches that end in a synchronise; every shape is warmed up first; the
variants of a shape are alternated inside each repeat, so drift hits
them alike; REPEATS repeats show the spread (min / median / max).

1. all messages valid: 16384 messages of 64 B, 4 KiB and 64 KiB and 1024
   messages of 1 MiB, both directions, a table of R = 2 and of R = 1024
   MRs (the second is read from global memory, not staged in LDS), the
   queue-pair word off and on.  The unprotected engine is measured three
   times (a, b, c); the spread of its three medians is the noise.
2. the scan kernels with nothing behind them: 16384 messages whose
   engine launch finds no chunk — zero lengths through gather_bytes_
   (k_vl_scan_b; the judge would return at once for these), and 64-byte
   messages that are all rejected for a stale rkey through gather_prot_
   (k_prot_scan resolves both keys and checks the outside range of
   every message).  The kernels' own times come from a kernel trace of
   `--trace S [--table R]`, which only issues launches: gather_bytes_
   and gather_prot_ (table of R MRs, no queue-pair word) alternating on
   shape S of section 1, as section 1 does, so that each scan finds the
   caches as the engine before it left them.

Usage: python tools/prot_bench.py [--out profiles/prot_1gpu.txt]
       rocprofv3 --kernel-trace --stats -d DIR -- \\
           python tools/prot_bench.py --trace 2 --table 1024
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
from rocnrdma_amd.utils import prot  # noqa: E402

REPEATS = 5
SHAPES = [(16384, 64), (16384, 4 << 10), (16384, 64 << 10), (1024, 1 << 20)]
TABLES = [2, 1024]


def time_ms(fn, iters: int) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(variants: dict, target_ms: float = 100.0) -> dict:
    """{name: [ms per call, per repeat]}; variants alternate inside a
    repeat."""
    iters = {}
    for name, fn in variants.items():  # warm-up, and size the window
        fn()
        torch.cuda.synchronize()
        one = max(time_ms(fn, 3), 1e-3)
        iters[name] = max(3, min(5000, int(target_ms / one)))
    times = {name: [] for name in variants}
    for _ in range(REPEATS):
        for name, fn in variants.items():
            times[name].append(time_ms(fn, iters[name]))
    return times


def table(R: int, region, staging, dev):
    """R MRs: row 0 the region, row 1 the staging buffer, the others
    small windows of the region nobody uses."""
    t = np.zeros((R, 4), dtype=np.int64)
    t[:, 0] = (np.arange(R) << 8) | 1
    t[:, 1] = region.data_ptr() + (np.arange(R) % 64) * 4096
    t[:, 2] = 4096
    t[:, 3] = prot.ACCESS_REMOTE_READ
    t[0, 1:] = (region.data_ptr(), region.numel(),
                prot.ACCESS_REMOTE_READ | prot.ACCESS_REMOTE_WRITE)
    t[1, 1:] = (staging.data_ptr(), staging.numel(),
                prot.ACCESS_LOCAL_WRITE)
    return torch.from_numpy(t).to(dev)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prot_1gpu.txt")
    ap.add_argument("--trace", type=int, default=None, metavar="S",
                    choices=range(len(SHAPES)),
                    help="no timing: alternating launches of the plain and "
                         "the protected gather on shape S, for a kernel "
                         "trace")
    ap.add_argument("--table", type=int, default=2, choices=TABLES,
                    help="with --trace: the size of the MR table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prot_bench needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def dev64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    size = max(n * msg for n, msg in SHAPES)
    staging = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    staging.zero_()
    region = torch.zeros(size, dtype=torch.uint8, device=dev)
    base = staging.data_ptr()
    assert base % 16 == 0 and region.data_ptr() % 16 == 0
    tables = {R: table(R, region, staging, dev) for R in TABLES}
    good = int(prot.pack_keys(prot.make_key(1, 1), prot.make_key(0, 1)))
    stale = int(prot.pack_keys(prot.make_key(1, 1), prot.make_key(0, 2)))
    qp = torch.zeros(1, dtype=torch.int32, device=dev)

    def variants_of(n, msg, which):
        offs = dev64(np.arange(n) * msg)
        addrs = dev64(base + np.arange(n) * msg)
        lens = dev64(np.full(n, msg))
        keys = dev64(np.full(n, good))
        plain, guarded = ((ops.gather_bytes_, ops.gather_prot_)
                          if which == "gather"
                          else (ops.scatter_bytes_, ops.scatter_prot_))
        v = {}
        for rep in "abc":
            v[f"bytes/{rep}"] = lambda: plain(region, offs, addrs, lens,
                                              max_msg_bytes=msg)
        for R in TABLES:
            v[f"prot R={R}"] = lambda R=R: guarded(
                region, offs, addrs, lens, keys, tables[R],
                max_msg_bytes=msg)
            v[f"prot R={R} qp"] = lambda R=R: guarded(
                region, offs, addrs, lens, keys, tables[R], qp_state=qp,
                max_msg_bytes=msg)
        st, _ = guarded(region, offs, addrs, lens, keys, tables[2],
                        qp_state=qp, max_msg_bytes=msg)
        assert not st.any() and int(qp.item()) == 0
        return v

    if args.trace is not None:
        n, msg = SHAPES[args.trace]
        v = variants_of(n, msg, "gather")
        for _ in range(20):
            v["bytes/a"]()
            v[f"prot R={args.table}"]()
        torch.cuda.synchronize()
        return 0

    say(f"# tools/prot_bench.py on {torch.cuda.get_device_name(dev)}; "
        f"us per call and GB/s = 1e9 bytes/s moved (one direction), median "
        f"[min .. max] of {REPEATS} repeats, device events")
    say()
    say("## 1. all messages valid: gather_prot_/scatter_prot_ against "
        "gather_bytes_/scatter_bytes_")
    say("bytes is measured three times (a, b, c); noise = spread of its "
        "three medians; extra = median - median of the three")
    say(f"{'n':>6} {'msg':>8} {'variant':<22} {'us/call':>10}  "
        f"{'[min .. max]':<24} {'GB/s':>8} {'extra us':>9} ratio")
    for n, msg in SHAPES:
        for which in ("gather", "scatter"):
            times = measure(variants_of(n, msg, which))
            meds = [statistics.median(times[f"bytes/{r}"]) for r in "abc"]
            ref = statistics.median(meds)
            say(f"{n:>6} {msg:>8} {which + ' bytes a/b/c':<22} "
                f"{meds[0] * 1e3:10.1f} {meds[1] * 1e3:10.1f} "
                f"{meds[2] * 1e3:10.1f}  noise "
                f"{(max(meds) - min(meds)) * 1e3:.1f} us  "
                f"{n * msg / ref / 1e6:8.2f} GB/s")
            for name, t in times.items():
                if name.startswith("bytes"):
                    continue
                med = statistics.median(t)
                say(f"{n:>6} {msg:>8} {which + ' ' + name:<22} "
                    f"{med * 1e3:10.1f}  [{min(t) * 1e3:9.1f} .. "
                    f"{max(t) * 1e3:9.1f}] {n * msg / med / 1e6:8.2f} "
                    f"{(med - ref) * 1e3:9.1f} {ref / med:5.3f}")

    say()
    say("## 2. the scans with an engine launch that finds no chunk, "
        "n = 16384")
    n = 16384
    offs, addrs = dev64(np.arange(n) * 64), dev64(base + np.arange(n) * 64)
    zeros, lens = dev64(np.zeros(n)), dev64(np.full(n, 64))
    bad = dev64(np.full(n, stale))
    calls = {"k_vl_scan_b (zero lengths, gather_bytes_)":
             lambda: ops.gather_bytes_(region, offs, addrs, zeros,
                                       max_msg_bytes=64)}
    for R in TABLES:
        calls[f"k_prot_scan (all rejected, R={R})"] = lambda R=R: \
            ops.gather_prot_(region, offs, addrs, lens, bad, tables[R],
                             max_msg_bytes=64)
        calls[f"k_prot_scan (all rejected, R={R}, qp)"] = lambda R=R: (
            qp.zero_(), ops.gather_prot_(region, offs, addrs, lens, bad,
                                         tables[R], qp_state=qp,
                                         max_msg_bytes=64))
    st, _ = ops.gather_prot_(region, offs, addrs, lens, bad, tables[2])
    assert (st == prot.WC_REM_ACCESS_ERR).all()
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        t = [time_ms(fn, 200) for _ in range(REPEATS)]
        say(f"{name:<44} {statistics.median(t) * 1e3:7.1f} us per call "
            f"[{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")
    say("(the qp rows include one memset of the word per call)")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
