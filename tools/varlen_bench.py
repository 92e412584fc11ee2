#!/usr/bin/env python3
"""Variable-length message engine against the uniform engines, one GPU.

One process; every timing is a pair of device events around ITERS
launches that end in a synchronise; every shape is warmed up first; the
variants of a shape are alternated inside each repeat, so drift hits
them alike; REPEATS repeats show the spread (min / median / max).

1. uniform lengths through gather_v_/scatter_v_ (crc off and on)
   against gather_/scatter_/gather_crc_/scatter_crc_, at the batch
   sizes the sdma transport uses for a 1 GiB region;
2. a mixed batch (1/3 each of 64 B, 4 KiB, 1 MiB by count) against the
   byte-weighted expectation from the three uniform rates;
3. crc32_messages_v against crc32_messages, 1 MiB messages, 1 GiB.

--bytes measures the byte-granular path instead (gather_bytes_ /
scatter_bytes_ / crc32_messages_bytes):

4. co-aligned: aligned multiples of 16 through the byte path against
   gather_v_/scatter_v_ on the same batches; the _v form is measured
   three times, the spread of its three medians is the noise;
5. skewed: the same sizes plus one byte at each --skew SRC,DST (default
   5,5: store skew only, and 3,11: the source realigned as well);
6. crc32_messages_bytes against crc32_messages_v, 1 MiB messages,
   1 GiB, at offset skew 0 and 7.

Usage: python tools/varlen_bench.py [--out profiles/varlen_1gpu.txt]
       python tools/varlen_bench.py --bytes [--skew 5,5 --skew 3,11]
                                    [--out profiles/bytes_1gpu.txt]
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

REPEATS = 5
SIZES = [64, 4 << 10, 64 << 10, 1 << 20]
STAGING = 64 << 20  # the sdma transport's pinned staging budget
MAX_BATCH = 16384   # and its ring size


def batch_of(msg: int) -> int:
    return max(8, min(STAGING // msg, MAX_BATCH))


def time_ms(fn, iters: int) -> float:
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(variants: dict, nbytes: int, target_ms: float = 100.0) -> dict:
    """{name: [GB/s per repeat]}; variants alternate inside a repeat."""
    iters = {}
    for name, fn in variants.items():  # warm-up, and size the window
        fn()
        torch.cuda.synchronize()
        one = max(time_ms(fn, 3), 1e-3)
        iters[name] = max(3, min(5000, int(target_ms / one)))
    rates = {name: [] for name in variants}
    for _ in range(REPEATS):
        for name, fn in variants.items():
            ms = time_ms(fn, iters[name])
            rates[name].append(nbytes / ms / 1e6)
    return rates


def fmt(r) -> str:
    return (f"{statistics.median(r):8.2f}  [{min(r):7.2f} .. {max(r):7.2f}]")


def bytes_sections(say, dev, skews) -> None:
    """Sections 4-6: the byte-granular path."""
    slack = 2 << 20  # room for the skewed layouts
    staging = torch.empty(STAGING + slack, dtype=torch.uint8,
                          pin_memory=True)
    staging.numpy()[:] = np.random.default_rng(1).integers(
        0, 256, staging.numel(), dtype=np.uint8)
    region = torch.zeros(STAGING + slack, dtype=torch.uint8, device=dev)
    base = staging.data_ptr()
    assert base % 16 == 0 and region.data_ptr() % 16 == 0

    def dev64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    def engines(offs, addrs, lens, cap, which):
        g, sc = ((ops.gather_v_, ops.scatter_v_) if which == "v"
                 else (ops.gather_bytes_, ops.scatter_bytes_))
        return {
            "gather": lambda: g(region, offs, addrs, lens,
                                max_msg_bytes=cap),
            "gather(crc)": lambda: g(region, offs, addrs, lens,
                                     max_msg_bytes=cap, crc=True),
            "scatter": lambda: sc(region, offs, addrs, lens,
                                  max_msg_bytes=cap),
            "scatter(crc)": lambda: sc(region, offs, addrs, lens,
                                       max_msg_bytes=cap, crc=True),
        }

    say()
    say("## 4. co-aligned multiples of 16: gather_bytes_/scatter_bytes_ "
        "against gather_v_/scatter_v_")
    say("_v is measured three times (a, b, c); noise = spread of its "
        "three medians; ratio = bytes / median of the three")
    say(f"{'msg':>8} {'batch':>6} {'variant':<14} {'_v a/b/c GB/s':<26} "
        f"{'noise':>6} {'bytes GB/s':>10}  {'[min .. max]':<20} ratio")
    for msg in SIZES:
        n = batch_of(msg)
        offs = dev64(np.arange(n) * msg)
        addrs = dev64(base + np.arange(n) * msg)
        lens = dev64(np.full(n, msg))
        old = engines(offs, addrs, lens, msg, "v")
        new = engines(offs, addrs, lens, msg, "bytes")
        variants = {}
        for k in old:
            for rep in "abc":
                variants[f"{k}/v{rep}"] = old[k]
            variants[f"{k}/bytes"] = new[k]
        rates = measure(variants, n * msg)
        for k in old:
            meds = [statistics.median(rates[f"{k}/v{rep}"]) for rep in "abc"]
            noise = max(meds) - min(meds)
            r = rates[f"{k}/bytes"]
            ratio = statistics.median(r) / statistics.median(meds)
            say(f"{msg:>8} {n:>6} {k:<14} "
                f"{meds[0]:8.2f} {meds[1]:8.2f} {meds[2]:8.2f} "
                f"{noise:6.2f} {fmt(r)} {ratio:5.3f}")

    # what the two-input scan costs: an all-zero batch through both
    n = MAX_BATCH
    offs, addrs = dev64(np.arange(n) * 64), dev64(base + np.arange(n) * 64)
    zeros = dev64(np.zeros(n))
    for name, fn in (("gather_v_", ops.gather_v_),
                     ("gather_bytes_", ops.gather_bytes_)):
        def call(fn=fn):
            fn(region, offs, addrs, zeros, max_msg_bytes=64)
        call()
        torch.cuda.synchronize()
        t = [time_ms(call, 200) for _ in range(REPEATS)]
        say(f"scan + empty engine launch, {name}, n = {n} zero-length "
            f"messages: {statistics.median(t) * 1e3:.1f} us per call "
            f"[{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")

    say()
    say("## 5. skewed: msg + 1 bytes, source at SRC and destination at "
        "DST bytes past a 16-byte boundary")
    say(f"{'skew':>6} {'msg':>8} {'batch':>6} {'variant':<14} {'GB/s':>8}  "
        f"{'[min .. max]':<20}")
    for src_skew, dst_skew in skews:
        for msg in SIZES:
            ln = msg + 1
            n = batch_of(msg)
            stride = (ln + 15) // 16 * 16 + 16
            assert n * stride + 16 <= STAGING + slack
            inside = np.arange(n) * stride
            # gather writes the region, scatter the staging buffer: give
            # each direction SRC on the side it reads, DST on the other
            for which, o_sk, a_sk in (("gather", dst_skew, src_skew),
                                      ("scatter", src_skew, dst_skew)):
                fns = engines(dev64(inside + o_sk),
                              dev64(base + inside + a_sk),
                              dev64(np.full(n, ln)), ln, "bytes")
                variants = {k: f for k, f in fns.items()
                            if k.startswith(which)}
                rates = measure(variants, n * ln)
                for k in variants:
                    say(f"{src_skew:>3},{dst_skew:<2} {ln:>8} {n:>6} "
                        f"{k:<14} {fmt(rates[k])}")

    say()
    say("## 6. crc32_messages_bytes / crc32_messages_v, 1 MiB messages, "
        "1 GiB")
    del region
    big = torch.empty((1 << 30) + 16, dtype=torch.uint8, device=dev)
    ops.fill_(big[:1 << 30], 7)
    msg, n = 1 << 20, 1 << 10
    lens = dev64(np.full(n, msg))
    offs0, offs7 = dev64(np.arange(n) * msg), dev64(np.arange(n) * msg + 7)
    variants = {
        "crc32_messages_v": lambda: ops.crc32_messages_v(
            big, offs0, lens, max_msg_bytes=msg),
        "bytes, skew 0": lambda: ops.crc32_messages_bytes(
            big, offs0, lens, max_msg_bytes=msg),
        "bytes, skew 7": lambda: ops.crc32_messages_bytes(
            big, offs7, lens, max_msg_bytes=msg),
    }
    assert torch.equal(variants["crc32_messages_v"](),
                       variants["bytes, skew 0"]())
    rates = measure(variants, 1 << 30)
    ref = statistics.median(rates["crc32_messages_v"])
    for name in variants:
        say(f"{name:<18} {fmt(rates[name])}  "
            f"ratio {statistics.median(rates[name]) / ref:5.3f}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bytes", action="store_true",
                    help="measure the byte-granular path (sections 4-6)")
    ap.add_argument("--skew", action="append", default=None,
                    metavar="SRC,DST",
                    help="with --bytes: a (source, destination) skew pair "
                         "for section 5; repeatable")
    args = ap.parse_args()
    if args.out is None:
        args.out = ("profiles/bytes_1gpu.txt" if args.bytes
                    else "profiles/varlen_1gpu.txt")
    skews = [tuple(int(v) for v in s.split(","))
             for s in (args.skew or ["5,5", "3,11"])]
    if any(len(p) != 2 or not all(0 <= v < 16 for v in p) for p in skews):
        ap.error("--skew takes SRC,DST with both in [0, 16)")
    assert torch.cuda.is_available(), "varlen_bench needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.bytes:
        say(f"# tools/varlen_bench.py --bytes on "
            f"{torch.cuda.get_device_name(dev)}; GB/s = 1e9 bytes/s moved "
            f"(one direction), median [min .. max] of {REPEATS} repeats, "
            f"device events")
        bytes_sections(say, dev, skews)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return 0

    say(f"# tools/varlen_bench.py on {torch.cuda.get_device_name(dev)}; "
        f"GB/s = 1e9 bytes/s moved (one direction), median "
        f"[min .. max] of {REPEATS} repeats, device events")
    staging = torch.empty(STAGING + (2 << 20), dtype=torch.uint8,
                          pin_memory=True)
    staging.numpy()[:] = np.random.default_rng(1).integers(
        0, 256, staging.numel(), dtype=np.uint8)
    region = torch.zeros(STAGING + (2 << 20), dtype=torch.uint8, device=dev)
    base = staging.data_ptr()

    def dev64(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)

    # -- 1. uniform lengths ---------------------------------------------
    say()
    say("## 1. uniform lengths: new path / existing engine")
    say(f"{'msg':>8} {'batch':>6} {'variant':<22} {'GB/s':>8}  "
        f"{'[min .. max]':<20} ratio")
    uniform_v = {}  # (direction, msg) -> median GB/s of the plain _v form
    for msg in SIZES:
        n = batch_of(msg)
        offs = dev64(np.arange(n) * msg)
        addrs = dev64(base + np.arange(n) * msg)
        lens = dev64(np.full(n, msg))
        variants = {
            "gather_": lambda: ops.gather_(region, offs, addrs, msg),
            "gather_v_": lambda: ops.gather_v_(
                region, offs, addrs, lens, max_msg_bytes=msg),
            "gather_crc_": lambda: ops.gather_crc_(region, offs, addrs, msg),
            "gather_v_(crc)": lambda: ops.gather_v_(
                region, offs, addrs, lens, max_msg_bytes=msg, crc=True),
            "scatter_": lambda: ops.scatter_(region, offs, addrs, msg),
            "scatter_v_": lambda: ops.scatter_v_(
                region, offs, addrs, lens, max_msg_bytes=msg),
            "scatter_crc_": lambda: ops.scatter_crc_(region, offs, addrs,
                                                     msg),
            "scatter_v_(crc)": lambda: ops.scatter_v_(
                region, offs, addrs, lens, max_msg_bytes=msg, crc=True),
        }
        rates = measure(variants, n * msg)
        names = list(variants)
        for old, new in zip(names[0::2], names[1::2]):
            ratio = statistics.median(rates[new]) / statistics.median(
                rates[old])
            say(f"{msg:>8} {n:>6} {old:<22} {fmt(rates[old])}")
            say(f"{msg:>8} {n:>6} {new:<22} {fmt(rates[new])} "
                f"{ratio:5.3f}")
        uniform_v["gather", msg] = statistics.median(rates["gather_v_"])
        uniform_v["scatter", msg] = statistics.median(rates["scatter_v_"])
        uniform_v["gather_crc", msg] = statistics.median(
            rates["gather_v_(crc)"])
        uniform_v["scatter_crc", msg] = statistics.median(
            rates["scatter_v_(crc)"])

    # what the scan and an empty main kernel cost: an all-zero batch
    n = MAX_BATCH
    offs, addrs = dev64(np.arange(n) * 64), dev64(base + np.arange(n) * 64)
    zeros = dev64(np.zeros(n))
    ops.gather_v_(region, offs, addrs, zeros, max_msg_bytes=64)
    torch.cuda.synchronize()
    t = [time_ms(lambda: ops.gather_v_(region, offs, addrs, zeros,
                                       max_msg_bytes=64), 200)
         for _ in range(REPEATS)]
    say(f"scan + empty engine launch, n = {n} zero-length messages: "
        f"{statistics.median(t) * 1e3:.1f} us per call "
        f"[{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")
    t = [time_ms(lambda: ops.gather_(region, offs[:1], addrs[:1], 16), 200)
         for _ in range(REPEATS)]
    say(f"for scale, gather_ of one 16-byte message: "
        f"{statistics.median(t) * 1e3:.1f} us per call "
        f"[{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]")

    # -- 2. mixed batch -------------------------------------------------
    say()
    say("## 2. mixed batch: 1/3 each of 64 B, 4 KiB, 1 MiB by count")
    kinds = [64, 4 << 10, 1 << 20]
    n = 63
    lens_np = np.array(kinds * (n // 3), dtype=np.int64)
    np.random.default_rng(2).shuffle(lens_np)
    starts = np.cumsum(lens_np) - lens_np
    total = int(lens_np.sum())
    offs, addrs, lens = dev64(starts), dev64(base + starts), dev64(lens_np)
    variants = {
        "gather_v_": lambda: ops.gather_v_(
            region, offs, addrs, lens, max_msg_bytes=1 << 20),
        "gather_v_(crc)": lambda: ops.gather_v_(
            region, offs, addrs, lens, max_msg_bytes=1 << 20, crc=True),
        "scatter_v_": lambda: ops.scatter_v_(
            region, offs, addrs, lens, max_msg_bytes=1 << 20),
        "scatter_v_(crc)": lambda: ops.scatter_v_(
            region, offs, addrs, lens, max_msg_bytes=1 << 20, crc=True),
    }
    rates = measure(variants, total)
    keys = {"gather_v_": "gather", "gather_v_(crc)": "gather_crc",
            "scatter_v_": "scatter", "scatter_v_(crc)": "scatter_crc"}
    say(f"n = {n}, {total} bytes per batch; expectation = bytes / "
        f"sum(bytes_k / uniform rate_k) from section 1's _v rates")
    for name in variants:
        t_exp = sum((n // 3) * k / uniform_v[keys[name], k] for k in kinds)
        exp = total / t_exp
        got = statistics.median(rates[name])
        say(f"{name:<18} {fmt(rates[name])}  expected {exp:7.2f}  "
            f"achieved/expected {got / exp:5.3f}")

    # -- 3. landed-bytes digest ------------------------------------------
    say()
    say("## 3. crc32_messages_v / crc32_messages, 1 MiB messages, 1 GiB")
    del region
    big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    ops.fill_(big, 7)
    msg, n = 1 << 20, 1 << 10
    offs, lens = dev64(np.arange(n) * msg), dev64(np.full(n, msg))
    variants = {
        "crc32_messages": lambda: ops.crc32_messages(big, msg),
        "crc32_messages_v": lambda: ops.crc32_messages_v(
            big, offs, lens, max_msg_bytes=msg),
    }
    assert torch.equal(variants["crc32_messages"](),
                       variants["crc32_messages_v"]())
    rates = measure(variants, 1 << 30)
    ratio = (statistics.median(rates["crc32_messages_v"]) /
             statistics.median(rates["crc32_messages"]))
    for name in variants:
        say(f"{name:<18} {fmt(rates[name])}")
    say(f"ratio {ratio:5.3f}")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
