#!/usr/bin/env python3
"""Flagship bench: aggregate RDMA-write bandwidth into GPU HBM.

Measures the BASELINE.json metric ("ib_write_bw GB/s NIC<->GPU-HBM ...")
on the best transport the box offers: real IB verbs when an HCA exists,
otherwise the SDMA PCIe-BAR path (same bus and BAR window an HCA would
master; transport recorded in config), `fake` on CPU-only boxes.

One rank per GPU ("one QP per MI355X").  A step posts `--msgs-per-step`
messages of `--msg-bytes` into a `--region-bytes` HBM region and
completes them.  Timed region: exactly K steps bracketed by
barrier + torch.cuda.synchronize on both sides; value is the whole-job
aggregate GB/s (sum of bytes over all ranks / max elapsed over ranks).

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the result line.  `--full` adds everything else,
outside the timed region: the payload-integrity proof (on-GPU
pattern/CRC kernels; a failure exits 2) and the 4 KiB / 1 MiB points
the metric names (`config.msg_sweep_gbps`).

`--dump-outputs DIR` writes what the last timed step left at the
receiver (the HBM region for writes, the staging slots for reads) as
DIR/<name>.npy, float32.  Inputs are a fixed pattern, so two builds run
with the same arguments can be compared output for output.

Launch (driver contract):
  python bench.py --gpus 1 --steps 20 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W
"""
from __future__ import annotations

import argparse
import json
import os
import time

METRIC = ("ib_write_bw GB/s NIC<->GPU-HBM at 4KB/1MB/64MB msg; "
          "1/2/4/8 MI355X aggregate")

# --dump-outputs: payload bytes kept per array (x4 on disk as float32,
# so one array stays at 32 MiB); larger arrays are sampled in chunks
_DUMP_BUDGET = 8 << 20
_DUMP_CHUNK = 4096
_DUMP_SEED = 0xD0BB5


def verbs_ok() -> bool:
    """A usable verbs stack: libibverbs + >=1 IB device + the built
    native harness (ROCNR_FORCE_VERBS=1 forces it for the fake-verbs
    CI tier)."""
    if os.environ.get("ROCNR_FORCE_VERBS") == "1":
        return True
    from rocnrdma_amd.transport.verbs import harness_binary, verbs_available

    return verbs_available() and harness_binary() is not None


def choose_transport(has_gpu: bool, verbs: bool) -> str:
    """--transport auto order: verbs — the BASELINE
    metric's real data plane (ibv_reg_mr + RDMA write, reference
    README.md:67) — then sdma (same PCIe/BAR path an HCA masters),
    then fake."""
    if verbs:
        return "verbs"
    return "sdma" if has_gpu else "fake"


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--msg-bytes", type=int, default=64 << 20,
                   help="message size (headline: 64 MiB)")
    p.add_argument("--region-bytes", type=int, default=1 << 30,
                   help="registered-region size per GPU (config 2: 1 GiB)")
    p.add_argument("--msgs-per-step", type=int, default=0,
                   help="0 = one full region pass per step")
    p.add_argument("--transport", default="auto",
                   choices=["auto", "fake", "sdma", "verbs"])
    p.add_argument("--verbs-mr", default="auto",
                   choices=["auto", "peer", "dmabuf", "host"],
                   help="verbs MR mode (auto: peer on GPU — the bridge "
                        "path — else host)")
    p.add_argument("--direction", default="write",
                   choices=["write", "read"])
    p.add_argument("--inflight", type=int, default=0,
                   help="0 = transport-chosen (kernel engine sizes its "
                        "WQE ring for ~64 MiB of pinned staging)")
    p.add_argument("--streams", type=int, default=2)
    p.add_argument("--skip-integrity", action="store_true")
    p.add_argument("--json-out", default="")
    p.add_argument("--full", action="store_true",
                   help="also run what the headline figure does not need "
                        "(outside the timed region): the integrity proof "
                        "and the 4 KiB / 1 MiB message-size points")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="write what the last timed step left at the "
                        "receiver as DIR/<name>.npy (float32)")
    return p.parse_args()


def dump_sample_chunks(nbytes: int):
    """Which _DUMP_CHUNK-byte chunks of an nbytes array --dump-outputs
    keeps: None = the whole array (it fits the budget), else a sorted
    index array that depends only on nbytes (fixed seed), so two runs
    with the same arguments sample the same bytes."""
    if nbytes <= _DUMP_BUDGET:
        return None
    import numpy as np

    from rocnrdma_amd.utils import pattern

    n_chunks = nbytes // _DUMP_CHUNK
    want = _DUMP_BUDGET // _DUMP_CHUNK
    picks = pattern.splitmix64_words(_DUMP_SEED, 0, want) % np.uint64(n_chunks)
    return np.unique(picks).astype(np.int64)


def dump_array(out_dir: str, name: str, buf) -> None:
    """Write a flat uint8 buffer (numpy array, or torch tensor on any
    device) as out_dir/name.npy in float32 — shape (nbytes,) when it fits
    the budget, else (chunks, _DUMP_CHUNK) for the sampled chunks."""
    import numpy as np

    is_np = isinstance(buf, np.ndarray)
    flat = buf.reshape(-1)
    idx = dump_sample_chunks(flat.shape[0])
    if idx is not None:
        n_chunks = flat.shape[0] // _DUMP_CHUNK
        rows = flat[:n_chunks * _DUMP_CHUNK].reshape(n_chunks, _DUMP_CHUNK)
        if is_np:
            flat = rows[idx]
        else:
            import torch

            flat = rows.index_select(
                0, torch.from_numpy(idx).to(rows.device))
    host = flat if is_np else flat.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), host.astype(np.float32))


def dump_outputs(out_dir: str, tp, direction: str, rank: int) -> None:
    """The arrays a caller of the timed path receives: the destination
    region after one-sided writes, the staging slots after reads."""
    suffix = f"_rank{rank}" if rank else ""
    if direction == "write":
        dump_array(out_dir, "region" + suffix, tp.region)
    else:
        staging = getattr(tp, "staging_flat", None)
        if staging is None:
            staging = tp.staging
        dump_array(out_dir, "staging" + suffix, staging)


def main():
    args = parse_args()
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist_mod.init_process_group("gloo", rank=rank, world_size=world)
        dist = dist_mod

    has_gpu = torch.cuda.is_available()
    device = None
    numa = None
    if has_gpu:
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
        device = torch.device("cuda", local_rank % torch.cuda.device_count())
        # pin the posting loop + pinned staging to the GPU's NUMA node
        from rocnrdma_amd.utils import topology

        numa = topology.bind_rank_near_gpu(device.index)

        # the gfx950 extension carries the message engine and the
        # integrity/CRC kernels: load it before anything is set up, so a
        # GPU run without it fails here instead of measuring a tree
        # whose native half is missing
        import rocnrdma_amd.ops as ops

        if not ops.have_ext():
            raise SystemExit(
                "rocnrdma_amd.ops._p2p_ext is not built "
                "(python __graft_entry__.py build)")

    from rocnrdma_amd.transport import get_transport

    # fake transport on CPU boxes gets a small region so CI stays fast
    region = args.region_bytes
    tname = args.transport
    if tname == "auto":
        tname = choose_transport(has_gpu, verbs_ok())
    if tname == "fake" and args.region_bytes > (64 << 20):
        region = min(region, 256 << 20)
    if tname == "verbs" and not has_gpu and args.region_bytes > (64 << 20):
        region = min(region, 256 << 20)   # CPU fake-verbs tier
    msg = min(args.msg_bytes, region)

    if tname == "verbs":
        if args.dump_outputs:
            # the region lives in the native harness process, which has
            # no way to hand it back; refuse rather than dump nothing
            raise SystemExit(
                "--dump-outputs is not available on the verbs transport "
                "(use --transport sdma or fake)")
        return run_verbs(args, msg, region, rank, world, has_gpu, device,
                         numa, dist)

    tp = get_transport(tname, msg_bytes=msg, region_bytes=region,
                       inflight=args.inflight, direction=args.direction,
                       device=device, num_streams=args.streams)

    msgs_per_step = args.msgs_per_step or tp.msgs_per_region
    bytes_per_step = msgs_per_step * msg

    def barrier():
        if dist is not None:
            dist.barrier()

    def gpu_sync():
        if has_gpu:
            torch.cuda.synchronize(device)

    def step(base):
        tp.post_many(base, msgs_per_step)
        tp.flush()

    # synthetic random payloads: pattern every staging slot before the
    # timed region (PCIe is data-agnostic, but the measurement should
    # not depend on that)
    if hasattr(tp, "staging"):
        from rocnrdma_amd.utils import pattern as _pat

        for si, slot in enumerate(tp.staging):
            words = _pat.splitmix64_words(0xDA7A + rank, si * 8192,
                                          msg // 8)
            try:
                import numpy as _np

                slot_np = slot.numpy() if hasattr(slot, "numpy") else slot
                slot_np.view(_np.uint64)[:] = words
            except (TypeError, ValueError):
                break

    # warmup (also first-touch of staging and region)
    for s in range(args.warmup):
        step(s * msgs_per_step)

    barrier()
    gpu_sync()
    t0 = time.perf_counter()
    for s in range(args.steps):
        step(s * msgs_per_step)
    gpu_sync()
    t1 = time.perf_counter()
    barrier()

    elapsed = t1 - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # before the integrity pass, which re-patterns the whole region
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, tp, args.direction, rank)

    integrity = "skipped"
    if args.full and not args.skip_integrity:
        bad = tp.integrity_check(seed=0xC0FFEE + rank)
        integrity = "ok" if bad == 0 else f"FAILED:{bad}"

    # --full: the metric names 4KB/1MB/64MB — attach quick per-GPU points
    # for the other two sizes (outside the timed region; single-rank runs
    # only — the scaling runs keep the headline size)
    msg_sweep = None
    if (args.full and world == 1 and tp.name in ("sdma", "fake")
            and not args.msgs_per_step):
        from rocnrdma_amd.harness.sweep import run_point
        from rocnrdma_amd.transport import get_transport as _gt

        msg_sweep = {}
        for other in (4096, 1 << 20):
            if other == msg:
                continue
            stp = _gt(tp.name, msg_bytes=other,
                      region_bytes=max(region // other, 1) * other,
                      direction=args.direction, device=device)
            try:
                msg_sweep[str(other)] = run_point(
                    stp, target_secs=0.3)["gbps"]
            finally:
                stp.close()

    total_bytes = bytes_per_step * args.steps * world
    value = total_bytes / elapsed / 1e9
    if msg_sweep is not None:
        msg_sweep[str(msg)] = round(value, 3)

    tp.close()
    emit_result(args, rank, world, has_gpu, value=value, elapsed=elapsed,
                msgs_per_step=msgs_per_step, msg=msg, region=region,
                transport=tp.name, integrity=integrity, numa=numa,
                msg_sweep=msg_sweep, dist=dist)


def emit_result(args, rank, world, has_gpu, *, value, elapsed,
                msgs_per_step, msg, region, transport, integrity, numa,
                msg_sweep, dist, mr=None):
    result = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "GB/s",
        "n_gpus": world if has_gpu else args.gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,  # reference publishes no numbers
        "dtype": "uint8",
        "data": "synthetic",
        "config": {
            "model": "rdma-write-bandwidth",
            "global_batch": msgs_per_step * world,
            "seq_len": msg,
            "parallelism": f"1qp-per-gpu x{world}",
            "transport": transport,
            "direction": args.direction,
            "msg_bytes": msg,
            "region_bytes": region,
            "inflight": args.inflight,
            "streams": args.streams,
            "integrity": integrity,
            "numa_bound": numa,
            "msg_sweep_gbps": msg_sweep,
        },
    }
    if mr is not None:
        result["config"]["verbs_mr"] = mr
    if rank == 0:
        line = json.dumps(result)
        print(line)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    if dist is not None:
        dist.destroy_process_group()
    if integrity.startswith("FAILED"):
        raise SystemExit(2)


def run_verbs(args, msg, region, rank, world, has_gpu, device, numa, dist):
    """The BASELINE metric's real data plane: one native harness run
    per rank ("one QP per MI355X") through ibv_reg_mr on the region
    (peer MR = the rocp2p bridge path) + chained one-sided RDMA WRs.
    The harness times exactly K steps after W warmup steps inside the
    native plane; ranks barrier around the run and aggregate as
    sum(bytes) / max(elapsed), same as the python paths."""
    import torch
    from rocnrdma_amd.transport.verbs import run_harness_steps

    dev_idx = device.index if device is not None else 0

    # Pick the MR mode BEFORE the ranks synchronize: peer (the bridge
    # path, the product under test) is preferred on GPU boxes, but a
    # box with an HCA and no rocp2p.ko loaded should still measure the
    # NIC<->HBM metric through the module-free dmabuf path rather than
    # fail.  A 1-step probe run per candidate keeps every rank on the
    # same number of barrier calls.
    if args.verbs_mr != "auto":
        candidates = [args.verbs_mr]
    elif has_gpu:
        candidates = ["peer", "dmabuf"]
    else:
        candidates = ["host"]
    mr = None
    probe_err = ""
    for cand in candidates:
        if len(candidates) == 1:
            mr = cand
            break
        try:
            run_harness_steps(msg_bytes=min(msg, 1 << 20),
                              region_bytes=min(region, 16 << 20),
                              steps=1, warmup=0,
                              direction=args.direction, mr=cand,
                              device_index=dev_idx, timeout=120)
            mr = cand
            break
        except RuntimeError as e:
            probe_err = str(e)
            print(f"# verbs mr={cand} unavailable: {probe_err}",
                  flush=True)
    if mr is None:
        raise RuntimeError(
            f"no usable verbs MR mode (last error: {probe_err})")

    if dist is not None:
        dist.barrier()
    rec = run_harness_steps(msg_bytes=msg, region_bytes=region,
                            steps=args.steps, warmup=args.warmup,
                            direction=args.direction, mr=mr,
                            device_index=dev_idx, seed=0xC0FFEE + rank,
                            integrity=args.full)
    if dist is not None:
        dist.barrier()

    elapsed = float(rec["secs"])
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    msgs_per_step = int(rec["msgs"]) // max(args.steps, 1)
    total_bytes = int(rec["msgs"]) * msg * world
    value = total_bytes / elapsed / 1e9
    integrity = rec.get("integrity", "skipped")

    # --full: metric names 4KB/1MB/64MB — quick per-GPU points outside
    # the timed region (single-rank runs only, like the sdma path)
    msg_sweep = None
    if args.full and world == 1:
        msg_sweep = {}
        for other in (4096, 1 << 20):
            if other == msg:
                continue
            sweep_region = max(min(region, 64 << 20) // other, 1) * other
            r2 = run_harness_steps(msg_bytes=other,
                                   region_bytes=sweep_region,
                                   steps=1, warmup=1,
                                   direction=args.direction, mr=mr,
                                   device_index=dev_idx)
            msg_sweep[str(other)] = round(float(r2["gbps"]), 3)
        msg_sweep[str(msg)] = round(value, 3)

    emit_result(args, rank, world, has_gpu, value=value, elapsed=elapsed,
                msgs_per_step=msgs_per_step, msg=msg, region=region,
                transport="verbs", integrity=integrity, numa=numa,
                msg_sweep=msg_sweep, dist=dist, mr=mr)


if __name__ == "__main__":
    main()
