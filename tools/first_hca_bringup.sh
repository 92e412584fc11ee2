#!/bin/bash
# first_hca_bringup.sh — the documented bring-up sequence
# (docs/RUNBOOK.md) as one executable pass for the first HCA-equipped
# box.  Stops at the first failing layer so the failure localizes.
#
#   tools/first_hca_bringup.sh [--dry-run] [--skip-modules]
#
# --dry-run: print and sanity-check every step without touching the
#            system (CI-exercised; no root, no hardware needed).
# --skip-modules: assume rocp2p.ko/rocp2p_probe.ko already loaded.
set -u
DRY=0
SKIP_MODULES=0
for a in "$@"; do
    case "$a" in
        --dry-run) DRY=1 ;;
        --skip-modules) SKIP_MODULES=1 ;;
        *) echo "unknown arg: $a" >&2; exit 2 ;;
    esac
done

HERE=$(cd "$(dirname "$0")/.." && pwd)
step() { echo; echo "== $1 =="; }
run() {
    echo "+ $*"
    [ "$DRY" = 1 ] && return 0
    "$@"
}

step "0. toolchain / artifacts present"
for f in "$HERE/harness/build/rocp2p_bw" "$HERE/tools/abi_probe.sh" \
         "$HERE/module/bridge/Makefile"; do
    [ -e "$f" ] || { echo "missing $f — run: python __graft_entry__.py build"; exit 1; }
done
echo "ok"

step "1. classify the installed ABI trees (drift switches)"
run bash "$HERE/tools/abi_probe.sh" || [ "$DRY" = 1 ] || {
    echo "NOTE: probe could not find system trees; kbuild will use the"
    echo "vendored contracts — acceptable for compile, risky for load."; }

if [ "$SKIP_MODULES" = 0 ]; then
    step "2. build + load the modules (root)"
    run make -C "$HERE/module" KDIR="/lib/modules/$(uname -r)/build"
    run insmod "$HERE/module/bridge/rocp2p.ko"
    run insmod "$HERE/module/probe/rocp2p_probe.ko"
fi

step "3. registration liveness (the #1 field failure)"
run bash "$HERE/tools/liveness.sh"

step "4. layer isolation, inside out (each must pass before the next)"
run "$HERE/build/tools/rocp2p_probe_cli" selftest 256
run "$HERE/harness/build/rocp2p_bw" --transport verbs --mr host \
    --msg 65536 --region 67108864 --secs 1 --json
run "$HERE/harness/build/rocp2p_bw" --transport verbs --mr dmabuf \
    --msg 1048576 --region 268435456 --secs 1 --json
run "$HERE/harness/build/rocp2p_bw" --transport verbs --mr peer \
    --msg 1048576 --region 268435456 --secs 1 --json

step "5. small-message chain sweep (find the doorbell knee; PERF.md §4)"
for c in 1 2 4 8 16 32 64; do
    run "$HERE/harness/build/rocp2p_bw" --transport verbs --mr peer \
        --msg 4096 --region 268435456 --secs 1 --chain "$c" --json
done

step "6. the metric (bench contract; auto now selects verbs)"
run python3 "$HERE/bench.py" --gpus 1 --steps 20 --warmup 5 --full

step "DONE"
echo "Compare step-6 output against profiles/ (PCIe envelope 50-57"
echo "GB/s) and the NIC line rate; an HCA below its line rate with"
echo "active_regs>0 is a fabric/NIC issue, not a bridge issue."
