"""CPU tier for memory protection: the scan kernel's judging, first-
failure search, flush, effective lengths and chunk prefix sums, emulated
on the host from the shared header (p2p_prot.h) and compared with the
numpy model (utils.prot.prot_reference), and protected=True on the fake
transport."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rocnrdma_amd.transport import get_transport
from rocnrdma_amd.utils import prot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1

# Host emulation of k_prot_scan.  The verdict, the final status and the
# effective length are p2p_prot.h's and the chunk count p2p_bytes.h's,
# the very code the kernel runs; the workgroup becomes W waves of 64
# lanes that own block_scan's segments, the wave reduction a loop over
# the lanes' minima, the LDS hand-over an array of W words and the scan a
# running sum.  Batches come from a file the test writes, results go to
# stdout; nothing here knows an expected value.
_SCAN_PROG = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "p2p_prot.h"

struct Case {
  uint64_t n, nmr, base;
  int gather, has_qp;
  int32_t qp;
  std::vector<uint64_t> mrs, offs, addrs, lens, keys;
};

static bool read_case(FILE* f, Case& c) {
  if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %d %d %d %" SCNu64, &c.n,
                  &c.nmr, &c.gather, &c.has_qp, &c.qp, &c.base) != 6)
    return false;
  c.mrs.resize(4 * c.nmr);
  for (auto& w : c.mrs)
    if (std::fscanf(f, "%" SCNu64, &w) != 1) std::abort();
  c.offs.resize(c.n); c.addrs.resize(c.n); c.lens.resize(c.n);
  c.keys.resize(c.n);
  for (uint64_t i = 0; i < c.n; i++)
    if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64,
                    &c.offs[i], &c.addrs[i], &c.lens[i], &c.keys[i]) != 4)
      std::abort();
  return true;
}

static void scan(Case& c, uint32_t W) {
  const uint32_t n = (uint32_t)c.n, threads = W * 64;
  // exactly sized: the sanitizers see an index past any of them
  std::vector<int32_t> status(n);
  std::vector<uint64_t> scratch(ROCP2P_PROT_SCRATCH_WORDS(n));
  uint64_t* cstart = scratch.data();
  uint64_t* elen = scratch.data() + (uint64_t)n + 1;
  int32_t* qp_state = c.has_qp ? &c.qp : nullptr;
  const bool qp = qp_state != nullptr;
  const bool entry_err = qp && *qp_state != 0;
  const uint64_t per = ((uint64_t)n + threads - 1) / threads * 64;
  std::vector<uint32_t> s_first(W);
  for (uint32_t wv = 0; wv < W; wv++) {
    const uint64_t b = wv * per < n ? wv * per : n;
    const uint64_t e = b + per < n ? b + per : n;
    uint32_t wave_first = ROCP2P_PROT_NO_F;
    for (uint32_t lane = 0; lane < 64; lane++) {
      uint32_t first = ROCP2P_PROT_NO_F;
      for (uint64_t i = b + lane; i < e; i += 64) {
        const uint32_t v = rocp2p_prot_verdict(
            c.mrs.data(), (uint32_t)c.nmr, c.base, c.offs[i], c.addrs[i],
            c.lens[i], c.keys[i], c.gather != 0);
        status[i] = (int32_t)v;
        if (v != ROCP2P_WC_SUCCESS && first == ROCP2P_PROT_NO_F)
          first = (uint32_t)i;
      }
      if (first < wave_first) wave_first = first;  // the shuffle tree
    }
    s_first[wv] = wave_first;
  }
  uint32_t f = ROCP2P_PROT_NO_F;
  for (uint32_t w = 0; w < W; w++)
    if (s_first[w] < f) f = s_first[w];
  if (qp && (entry_err || f != ROCP2P_PROT_NO_F)) *qp_state = 1;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t st =
        rocp2p_prot_final((uint32_t)status[i], i, f, qp, entry_err);
    const uint64_t el = rocp2p_prot_elen(st, c.lens[i]);
    status[i] = (int32_t)st;
    elen[i] = el;
    cstart[i] = at;
    at += rocp2p_b_chunks(
        (uint32_t)(c.gather ? c.offs[i] : c.addrs[i]) & 15u, el);
  }
  cstart[n] = at;
  std::printf("%d %" PRIu64 "\n", c.has_qp ? c.qp : -1, cstart[n]);
  for (uint32_t i = 0; i < n; i++)
    std::printf("%d %" PRIu64 " %" PRIu64 "\n", status[i], elen[i],
                cstart[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const uint32_t W = (uint32_t)std::atoi(argv[2]);
  Case c;
  while (read_case(f, c)) scan(c, W);
  std::fclose(f);
  return 0;
}
"""

RR, RW, LW = (prot.ACCESS_REMOTE_READ, prot.ACCESS_REMOTE_WRITE,
              prot.ACCESS_LOCAL_WRITE)
BASE = 0x7F0000001000  # region base, 16-byte aligned
OUT = 0x560000000000   # where the outside buffers lie
TOP = (1 << 64) - 4096


def _table():
    """Eight MRs; R = 9 with one free row whose old key is still there."""
    rows = [
        (prot.make_key(0, 1), BASE + 4096, 8192, RR | RW),  # region, middle
        (prot.make_key(1, 7), OUT + 4096, 8192, LW),        # outside
        (prot.make_key(2, 3), BASE + 4096, 8192, 0),        # free row
        (prot.make_key(3, 9), OUT + 4096, 8192, RR),        # outside, no LW
        (prot.make_key(4, 2), BASE + 4096, 8192, RR),       # region, read only
        (prot.make_key(5, 2), BASE + 4096, 8192, RW),       # ... write only
        (prot.make_key(6, 1), TOP, 4096, LW),               # ends at 2^64
        (prot.make_key(7, 1), TOP, 4095, LW),               # ends at 2^64 - 1
        (prot.make_key(8, 255), BASE, 1 << 20, RR | RW | LW),
    ]
    return np.array(rows, dtype=np.uint64)


def _rule_messages():
    """(off, addr, len, lkey, rkey) for every rule and every edge."""
    k = _table()[:, 0].tolist()
    R, O = k[0], k[1]
    o0, a0 = 4096, OUT + 4096  # first byte of both MRs
    return [
        (o0, a0, 100, O, R),                      # valid
        (o0, a0, 8192, O, R),                     # the whole MR
        (0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF),        # empty, garbage keys
        (M64, M64, 0, 0, 0),                      # empty, garbage all over
        (o0, a0, M64, O, R),                      # length -1
        (o0, a0, 1 << 63, O, R),                  # the sign bit alone
        (o0, a0, (1 << 63) + 5, 0xFFFFFFFF, R),   # ... beats a bad lkey
        # outside side: keys
        (o0, a0, 16, O ^ 1, R),                   # stale tag
        (o0, a0, 16, k[2], R),                    # free slot, key still there
        (o0, a0, 16, prot.make_key(9, 1), R),     # slot == R
        (o0, a0, 16, prot.make_key(1000, 7), R),  # slot far beyond
        (o0, a0, 16, 0xFFFFFFFF, R),              # 32 bits of garbage
        # outside side: both ends of the MR
        (o0, a0 + 8191, 1, O, R),                 # the last byte
        (o0, a0 + 8192, 1, O, R),                 # one byte past
        (o0, a0 - 1, 1, O, R),                    # one byte before
        (o0, a0 - 1, 2, O, R),                    # straddles the start
        (o0, a0 + 8191, 2, O, R),                 # straddles the end
        (o0, a0 + 1, 8192, O, R),                 # as long as the MR, shifted
        (o0, a0, 8193, O, R),                     # one byte too long
        # outside side: 2^64
        (o0, (1 << 64) - 16, 32, k[6], R),        # wraps; MR ends at 2^64
        (o0, (1 << 64) - 16, 32, k[7], R),        # wraps; MR ends just below
        (o0, (1 << 64) - 16, 16, k[6], R),        # fits to the last byte
        (o0, (1 << 64) - 16, 16, k[7], R),        # one byte past that MR
        (o0, (1 << 64) - 16, 15, k[7], R),
        # outside side: rights (a scatter writes it)
        (o0, a0, 16, k[3], R),
        # region side: keys and ends
        (o0, a0, 16, O, R ^ 2),
        (o0, a0, 16, O, k[2]),
        (o0, a0, 16, O, prot.make_key(9, 1)),
        (o0 + 8191, a0, 1, O, R),
        (o0 + 8192, a0, 1, O, R),
        (o0 - 1, a0, 1, O, R),
        (o0 + 8191, a0, 2, O, R),
        (o0, a0, 8193, O, R),
        (M64 - BASE + 1 + 4096 + BASE, a0, 16, O, R),  # offset wraps to o0
        ((-BASE) & M64, a0, 16, O, R),            # region + off == 0
        # region side: rights
        (o0, a0, 16, O, k[4]),
        (o0, a0, 16, O, k[5]),
        # both sides bad: the local error is reported
        (o0 + 8192, a0 + 8192, 1, O, R),
        # the catch-all MR on both sides
        (0, BASE + 512, 64, k[8], k[8]),
        (1 << 20, BASE, 1, k[8], k[8]),
    ]


def _case(msgs, mrs, gather, qp=None, base=BASE):
    m = np.array([[int(v) & M64 for v in row] for row in msgs],
                 dtype=np.uint64).reshape(-1, 5)
    keys = (m[:, 3] << np.uint64(32)) | (m[:, 4] & np.uint64(0xFFFFFFFF))
    return dict(mrs=np.asarray(mrs, dtype=np.uint64), base=base,
                offs=m[:, 0], addrs=m[:, 1], lens=m[:, 2], keys=keys,
                gather=gather, qp=qp)


def _f_cases():
    """Ordered batches: the first failure at 0, 63, 64, in another wave's
    segment, at n - 1 and absent, more failures behind it, zero-length
    messages around it, and the word already set on entry."""
    k = _table()[:, 0].tolist()
    R, O = int(k[0]), int(k[1])
    good = (4096 + 5, OUT + 4096 + 9, 4097, O, R)
    bad_l = (4096, OUT, 16, O, R)
    bad_r = (0, OUT + 4096, 16, O, R)
    empty = (0, 0, 0, 0xFFFFFFFF, 0)
    out = []
    # n = 200: W = 3 gives segments of 128, W = 1 one of 256
    # n = 2500: W = 16 gives segments of 192, W = 3 of 896
    for n in (1, 64, 65, 200, 2500):
        spots = [(), (0,), (n - 1,)]
        for f in (63, 64, 130, 150, 191, 192, 200, 900, 2000):
            if f < n - 1:
                spots += [(f,), (f, f + 1), (f, n - 1)]
        if n > 150:
            spots += [(150, 3), (129, 127), (193, 190, 191)]
        for where in spots:
            msgs = [good] * n
            for j, w in enumerate(where):
                msgs[w] = bad_r if j % 2 else bad_l
            if n > 4:
                msgs[1] = empty
                msgs[n - 2] = empty
            for gather in (True, False):
                out.append(_case(msgs, _table(), gather, qp=0))
                out.append(_case(msgs, _table(), gather, qp=None))
            out.append(_case(msgs, _table(), True, qp=1))
            out.append(_case(msgs, _table(), False, qp=-3))
    return out


def _random_cases(seed, count):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        R = int(g.choice([1, 2, 5, 64, 65, 300]))
        mrs = np.zeros((R, 4), dtype=np.uint64)
        for s in range(R):
            mrs[s] = (prot.make_key(s, int(g.integers(256))),
                      (BASE if g.random() < 0.5 else OUT)
                      + int(g.integers(0, 64)) * 64,
                      int(g.integers(1, 64)) * 64,
                      int(g.integers(0, 8)))
        n = int(g.choice([1, 2, 63, 64, 65, 129, 700]))
        msgs = []
        for _ in range(n):
            def side():
                s = int(g.integers(0, R + 1))
                key = prot.make_key(s, 0) | (int(mrs[s, 0]) & 0xFF
                                             if s < R else 1)
                if g.random() < 0.1:
                    key ^= 1
                at = (int(mrs[s, 1]) if s < R else OUT) + int(
                    g.integers(-2, 3))
                return key, at, (int(mrs[s, 2]) if s < R else 64)
            lk, a, la = side()
            rk, r, lr = side()
            ln = int(g.choice([0, 1, min(la, lr) - 2, min(la, lr),
                               min(la, lr) + 1, -1]))
            msgs.append(((r - BASE) & M64, a & M64, ln & M64, lk, rk))
        qp = [None, 0, 0, 1][int(g.integers(4))]
        out.append(_case(msgs, mrs, bool(g.integers(2)), qp=qp))
    return out


def _all_cases():
    cases = []
    for gather in (True, False):
        for qp in (None, 0):
            cases.append(_case(_rule_messages(), _table(), gather, qp=qp))
        # every rule as a batch of its own, ordered: f = 0 or absent
        for msg in _rule_messages():
            cases.append(_case([msg], _table(), gather, qp=0))
    cases += _f_cases()
    cases += _random_cases(11, 120)
    return cases


def _expected(c):
    st, el, qp = prot.prot_reference(c["mrs"], c["base"], c["offs"],
                                     c["addrs"], c["lens"], c["keys"],
                                     c["gather"], qp_state=c["qp"])
    where = c["offs"] if c["gather"] else c["addrs"]
    skew = (where & np.uint64(15)).astype(np.int64)
    chunks = np.where(el > 0, (skew + el + 4095) // 4096, 0)
    cstart = np.concatenate([[0], np.cumsum(chunks)])
    return st, el, cstart, qp


def _write_cases(path, cases):
    with open(path, "w") as f:
        for c in cases:
            qp = c["qp"]
            f.write(f"{len(c['lens'])} {len(c['mrs'])} {int(c['gather'])} "
                    f"{int(qp is not None)} {0 if qp is None else qp} "
                    f"{c['base']}\n")
            for row in c["mrs"].tolist():
                f.write(" ".join(str(v) for v in row) + "\n")
            for row in zip(c["offs"].tolist(), c["addrs"].tolist(),
                           c["lens"].tolist(), c["keys"].tolist()):
                f.write(" ".join(str(v) for v in row) + "\n")


def _run_scan(tmp_path, extra, waves, cases, header_dir=None, prog=None):
    """Build the emulation, run it with `waves` waves over `cases`;
    returns per case (status, elens, cstart, qp_out)."""
    src = tmp_path / "prot_scan_check.cpp"
    exe = tmp_path / "prot_scan_check"
    src.write_text(prog or _SCAN_PROG)
    inc = header_dir or os.path.join(ROOT, "rocnrdma_amd", "ops", "csrc")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra,
         "-I", inc, str(src), "-o", str(exe)],
        check=True, capture_output=True, text=True)
    inp = tmp_path / "cases.txt"
    _write_cases(inp, cases)
    r = subprocess.run([str(exe), str(inp), str(waves)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    tok = r.stdout.split()
    pos, out = 0, []
    for c in cases:
        n = len(c["lens"])
        qp, total = int(tok[pos]), int(tok[pos + 1])
        body = np.array(tok[pos + 2:pos + 2 + 3 * n],
                        dtype=np.uint64).reshape(n, 3)
        pos += 2 + 3 * n
        cstart = np.concatenate([body[:, 2], [total]]).astype(np.int64)
        out.append((body[:, 0].astype(np.int32), body[:, 1].astype(np.int64),
                    cstart, qp if c["qp"] is not None else None))
    assert pos == len(tok)
    return out


def _compare(cases, got):
    for j, (c, g) in enumerate(zip(cases, got)):
        st, el, cstart, qp = _expected(c)
        what = f"case {j} (n={len(st)}, gather={c['gather']}, qp={c['qp']})"
        assert (g[0] == st).all(), (what, np.flatnonzero(g[0] != st)[:5],
                                    g[0][:8], st[:8])
        assert (g[1] == el).all(), what
        assert (g[2] == cstart).all(), what
        assert g[3] == qp, what


def test_model_rules_by_hand():
    """The oracle itself, against statuses worked out by hand from the
    rules for every rule message, both directions."""
    S, LEN, LOC, REM = (prot.WC_SUCCESS, prot.WC_LOC_LEN_ERR,
                        prot.WC_LOC_PROT_ERR, prot.WC_REM_ACCESS_ERR)
    gather = [S, S, S, S, LEN, LEN, LEN,
              LOC, LOC, LOC, LOC, LOC,
              S, LOC, LOC, LOC, LOC, LOC, LOC,
              LOC, LOC, S, LOC, S,
              S,  # a gather only reads the outside MR
              REM, REM, REM, S, REM, REM, REM, LOC,  # 8193 fails outside first
              S, REM,
              REM, S,  # read only / write only
              LOC,
              S, REM]
    scatter = list(gather)
    scatter[24] = LOC        # no LOCAL_WRITE
    scatter[35], scatter[36] = S, REM
    # the MRs at the top of the address space grant LOCAL_WRITE only and
    # the catch-all grants everything: unchanged
    for want, g in ((gather, True), (scatter, False)):
        c = _case(_rule_messages(), _table(), g)
        st, el, qp = prot.prot_reference(c["mrs"], c["base"], c["offs"],
                                         c["addrs"], c["lens"], c["keys"], g)
        assert st.tolist() == want
        assert qp is None
        lens = c["lens"].astype(np.int64)
        assert (el == np.where(st == 0, lens, 0)).all()
    # ordered: everything behind the first failure (index 4) is flushed
    c = _case(_rule_messages(), _table(), True)
    st, el, qp = prot.prot_reference(c["mrs"], c["base"], c["offs"],
                                     c["addrs"], c["lens"], c["keys"], True,
                                     qp_state=0)
    assert st[:5].tolist() == [S, S, S, S, LEN] and qp == 1
    assert (st[5:] == prot.WC_WR_FLUSH_ERR).all() and not el[4:].any()
    st, el, qp = prot.prot_reference(c["mrs"], c["base"], c["offs"][:4],
                                     c["addrs"][:4], c["lens"][:4],
                                     c["keys"][:4], True, qp_state=0)
    assert not st.any() and qp == 0
    st, el, qp = prot.prot_reference(c["mrs"], c["base"], c["offs"][:4],
                                     c["addrs"][:4], c["lens"][:4],
                                     c["keys"][:4], True, qp_state=7)
    assert (st == prot.WC_WR_FLUSH_ERR).all() and qp == 1 and not el.any()


def test_keys():
    assert prot.make_key(0, 0) == 0 and prot.make_key(3, 5) == 0x305
    assert prot.make_key((1 << 20) - 1, 255) == (1 << 28) - 1
    for bad in ((-1, 0), (1 << 20, 0), (0, 256), (0, -1)):
        with pytest.raises(ValueError):
            prot.make_key(*bad)
    assert int(prot.pack_keys(0x305, 0x102)) == (0x305 << 32) | 0x102
    k = prot.pack_keys(np.array([1, 2]), 7)
    assert k.dtype == np.int64 and k.tolist() == [(1 << 32) | 7, (2 << 32) | 7]
    with pytest.raises(ValueError):
        prot.pack_keys(1 << 32, 0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("waves", [1, 3, 16])
def test_scan_emulation_matches_model(tmp_path, waves):
    """Every rule of the verdict, both ends of an MR, 2^64, the sign bit,
    stale tag / free slot / slot >= R, empty messages with garbage keys,
    f at 0, 63, 64, in another wave's segment, at n - 1 and absent, the
    word set on entry, effective lengths and cstart."""
    cases = _all_cases()
    _compare(cases, _run_scan(tmp_path, [], waves, cases))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_scan_emulation_under_sanitizers(tmp_path):
    """The same stand-alone program with ASan and UBSan: status, cstart
    and elen are exactly sized, no index leaves them and nothing
    overflows on the way."""
    cases = _all_cases()
    _compare(cases, _run_scan(
        tmp_path, ["-fsanitize=address,undefined",
                   "-fno-sanitize-recover=undefined"], 16, cases))


# -- fake transport ----------------------------------------------------------
MSG, REGION = 8192, 128 << 10  # 16 region messages, 8 staging slots
KNOWN = 0xC3
S, LOC, FLUSH, REM = (prot.WC_SUCCESS, prot.WC_LOC_PROT_ERR,
                      prot.WC_WR_FLUSH_ERR, prot.WC_REM_ACCESS_ERR)


def _open(direction="write", name="fake", **kw):
    kw.setdefault("region_skew", 5)
    kw.setdefault("staging_skew", 9)
    tp = get_transport(name, msg_bytes=MSG, region_bytes=REGION,
                       direction=direction, var_len=True, byte_granular=True,
                       protected=True, **kw)
    return tp


def _views(tp):
    """(region as numpy, staging [inflight, msg] as numpy, set_region)."""
    return tp._region_get, tp._slots, tp._region_fill


def check_post_and_post_many_agree(name, direction, **kw):
    a, b = _open(direction, name, **kw), _open(direction, name, **kw)
    n = a.msgs_per_region
    lens = np.random.default_rng(3).choice([0, 1, 17, 4097, MSG - 9], n)
    rng = np.random.default_rng(5)
    for tp in (a, b):
        region, staging, set_region = _views(tp)
        staging[:] = np.random.default_rng(8).integers(
            0, 256, staging.shape, dtype=np.uint8)
        set_region(KNOWN)
    wa = a.reg_mr("region", 0, 4 * MSG, RR | RW)
    wb = b.reg_mr("region", 0, 4 * MSG, RR | RW)
    assert wa == wb
    rkeys = np.where(rng.random(n) < 0.5, wa, a.region_key)
    rkeys[:6] = wa  # 0..3 inside the window, 4 is the first one outside
    want, _, _ = a.prot_expected(0, n, lens, rkey=rkeys)
    assert want[:4].tolist() == [S] * 4 and want[4] in (S, REM)
    got_a = []
    for i in range(n):
        a.post(i, int(lens[i]), rkey=int(rkeys[i]))
        if (i + 1) % a.inflight == 0:
            a.flush()
            got_a.append(a.completions())
    b.post_many(0, n, lens, rkey=rkeys)  # flushes its ring when it is full
    b.flush()
    got_b_tail = b.completions()
    got_a = np.concatenate(got_a)
    assert (got_a == want).all()
    assert (got_b_tail == want[-len(got_b_tail):]).all()
    assert (_views(a)[0]() == _views(b)[0]()).all()
    assert (_views(a)[1] == _views(b)[1]).all()
    assert a.prot_stats() == b.prot_stats()
    assert a.qp_in_error() == b.qp_in_error() == bool(want.any())
    a.close()
    b.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_post_and_post_many_agree(direction):
    check_post_and_post_many_agree("fake", direction)


def check_reg_dereg_and_tags(name, direction, **kw):
    tp = _open(direction, name, max_mr=4, **kw)
    assert tp.protected and tp.supports_protection
    assert tp.region_key != tp.staging_key
    w = tp.reg_mr("region", MSG, MSG, RR | RW)
    w2 = tp.reg_mr("staging", 0, MSG, LW)
    with pytest.raises(ValueError, match="full"):
        tp.reg_mr("region", 0, 16, RR)
    for bad in (("region", REGION - 15, 16, RR), ("region", -1, 16, RR),
                ("staging", 0, tp.inflight * MSG + 1, LW),
                ("region", 0, 16, 0), ("region", 0, 16, 8),
                ("elsewhere", 0, 16, RR)):
        with pytest.raises(ValueError):
            tp.reg_mr(*bad)
    for i, rkey, lkey, want in ((1, w, None, S), (2, w, None, REM),
                                (0, None, w2, S), (1, None, w2, LOC),
                                (1, w, w2, LOC), (0, w, w2, REM),
                                (0, w2, w, LOC)):  # the sides swapped
        tp.post(i, 64, rkey=rkey, lkey=lkey)
        tp.flush()
        assert tp.completions().tolist() == [want], (i, rkey, lkey)
        assert tp.qp_in_error() == (want != S)
        tp.reset_qp()
        assert not tp.qp_in_error()
    # a freed slot is reused under another tag: the old key is stale
    tp.dereg_mr(w)
    with pytest.raises(ValueError, match="unknown"):
        tp.dereg_mr(w)
    with pytest.raises(ValueError, match="unknown"):
        tp.dereg_mr(12345 << 8)
    tp.post(1, 64, rkey=w)
    tp.flush()
    assert tp.completions().tolist() == [REM]
    tp.reset_qp()
    w3 = tp.reg_mr("region", MSG, MSG, RR | RW)
    assert w3 >> 8 == w >> 8 and w3 != w
    tp.post_many(1, 1, 64, rkey=np.array([w]))
    tp.flush()
    assert tp.completions().tolist() == [REM]
    tp.reset_qp()
    tp.post(1, 64, rkey=w3)
    tp.flush()
    assert tp.completions().tolist() == [S]
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_reg_dereg_and_tags(direction):
    check_reg_dereg_and_tags("fake", direction)


def check_error_flushes_across_ring(name, direction, **kw):
    """A failing post puts the queue pair in error; everything behind it
    is flushed and moves nothing, across the automatic flush of a full
    ring, until reset_qp()."""
    tp = _open(direction, name, **kw)
    region, staging, set_region = _views(tp)
    n, ring = tp.msgs_per_region, tp.inflight
    assert n == 2 * ring
    rs, ss = tp.region_skew, tp.staging_skew
    write = direction == "write"
    w = tp.reg_mr("region", 0, 3 * MSG, RR | RW)
    data = np.random.default_rng(2).integers(0, 256, (n, MSG), dtype=np.uint8)

    def load():
        if write:
            staging[:] = data[:ring]  # slot j serves messages j and j + ring
            set_region(KNOWN)
        else:
            staging[:] = KNOWN
            tp._region_set(data.reshape(-1))

    def landed(i, ln):
        there = region()[i * MSG:(i + 1) * MSG]
        slot = staging[i % ring]
        recv, sent, at = ((there, slot[ss:ss + ln], rs) if write
                          else (slot, there[rs:rs + ln], ss))
        if (recv == KNOWN).all():
            return False
        assert (recv[:at] == KNOWN).all() and (recv[at + ln:] == KNOWN).all()
        assert (recv[at:at + ln] == sent).all()
        return True

    load()
    rkeys = np.full(n, w)  # messages 0..2 are inside the window
    tp.post_many(0, n, 100, rkey=rkeys)  # the ring flushes after `ring`
    first = tp.completions()
    assert first.tolist() == [S, S, S, REM] + [FLUSH] * (ring - 4)
    tp.flush()
    assert tp.completions().tolist() == [FLUSH] * ring
    assert tp.qp_in_error()
    if write:
        assert [landed(i, 100) for i in range(n)] == \
            [True] * 3 + [False] * (n - 3)
    else:  # slots are shared by i and i + ring; neither moved from 3 on
        assert [landed(i, 100) for i in range(ring)] == \
            [True] * 3 + [False] * (ring - 3)
    assert tp.prot_stats() == {"ok": 3, "errors": 1, "flushed": n - 4}
    # still in error: valid default-key posts are flushed too
    load()
    tp.post_many(0, 4, 100)
    tp.flush()
    assert tp.completions().tolist() == [FLUSH] * 4
    assert not any(landed(i, 100) for i in range(4))
    assert tp.prot_stats() == {"ok": 3, "errors": 1, "flushed": n}
    tp.reset_qp()
    assert not tp.qp_in_error()
    tp.post_many(0, 4, 100)
    tp.flush()
    assert tp.completions().tolist() == [S] * 4
    assert all(landed(i, 100) for i in range(4))
    assert tp.prot_stats() == {"ok": 7, "errors": 1, "flushed": n}
    tp.close()


@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_error_flushes_across_ring(direction):
    check_error_flushes_across_ring("fake", direction)


def check_digest_and_integrity(name, direction, **kw):
    tp = _open(direction, name, **kw)
    n = tp.msgs_per_region
    pay = np.random.default_rng(6).integers(0, 256, REGION, dtype=np.uint8)
    lens = np.random.default_rng(7).choice([0, 1, 4097, MSG - 9], n)
    lens[:4] = [0, 1, MSG - 9, 4097]
    assert tp.digest_check(pay, lens) == 0
    assert tp.digest_check(pay) == 0
    assert not tp.qp_in_error()
    # without its default staging MR every message with bytes is rejected
    # or flushed, and counted as bad; the empty ones in front still pass
    tp.dereg_mr(tp.staging_key)
    assert tp.digest_check(pay, lens) == n - 1
    assert tp.qp_in_error()
    tp.close()
    tp = _open(direction, name, region_skew=0, staging_skew=0, **kw)
    assert tp.integrity_check(seed=31) == 0
    tp.dereg_mr(tp.region_key)
    assert tp.integrity_check(seed=32) >= n
    tp.close()


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_fake_digest_check_counts_rejected_as_bad(direction, icrc):
    check_digest_and_integrity("fake", direction, icrc=icrc)


def test_protected_validation():
    kw = dict(msg_bytes=MSG, region_bytes=REGION)
    with pytest.raises(ValueError, match="byte_granular"):
        get_transport("fake", var_len=True, protected=True, **kw)
    with pytest.raises(ValueError, match="max_sge"):
        get_transport("fake", var_len=True, byte_granular=True, max_sge=2,
                      protected=True, **kw)
    for bad in (1, 2.5, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_mr"):
            get_transport("fake", var_len=True, byte_granular=True,
                          protected=True, max_mr=bad, **kw)
    for name in ("shm", "verbs"):
        with pytest.raises(NotImplementedError, match="protected"):
            get_transport(name, host="127.0.0.1", port=1, var_len=True,
                          byte_granular=True, protected=True, **kw)
    # keys need a protected transport; so does everything else
    tp = get_transport("fake", var_len=True, byte_granular=True, **kw)
    assert tp.protected is False
    with pytest.raises(ValueError, match="protected"):
        tp.post(0, 16, rkey=1)
    with pytest.raises(ValueError, match="protected"):
        tp.post_many(0, 2, 16, lkey=np.array([1, 1]))
    for call in (lambda: tp.reg_mr("region", 0, 16, RR),
                 lambda: tp.dereg_mr(1), tp.completions, tp.prot_stats,
                 tp.qp_in_error, tp.reset_qp):
        with pytest.raises(ValueError, match="protected"):
            call()
    tp.post(0, 16)  # and nothing else has changed
    tp.close()
    tp = _open()
    with pytest.raises(ValueError):
        tp.post_many(0, 2, 16, rkey=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        tp.post(0, 16, rkey=1 << 32)
    with pytest.raises(ValueError):
        tp.post(0, 16, lkey=-1)
    with pytest.raises(ValueError):
        tp.post(0, 16, rkey=1.5)
    with pytest.raises(ValueError):  # the host checks of nbytes stay
        tp.post(0, MSG, rkey=tp.region_key)
    assert tp.completions().size == 0
    tp.close()


def test_soak_prot_on_fake():
    from rocnrdma_amd.harness.soak import run_soak

    with pytest.raises(ValueError, match="prot"):
        run_soak("fake", secs=0.1, mixed=True, prot=True)
    with pytest.raises(ValueError, match="prot"):
        run_soak("fake", secs=0.1, mixed=True, byte_granular=True, sg=2,
                 prot=True)
    for icrc in (False, True):
        stats = run_soak("fake", secs=0.3, region_bytes=1 << 20, seed=5,
                         mixed=True, byte_granular=True, prot=True, icrc=icrc)
        assert stats["cycles"] > 0 and stats["failures"] == 0
        assert stats["prot_rejected"] > 0 and stats["prot_flushed"] > 0
        assert 0 < stats["bytes"]


def test_gpu_tier_batches_hold_every_status():
    """The seeded batches of tests/test_gpu_prot.py, judged here by the
    model: SUCCESS, LOC_PROT_ERR and REM_ACCESS_ERR each occur, SUCCESS
    is between a quarter and three quarters of the non-empty messages
    from 63 messages up, and every range lies inside the arena (Batch
    asserts it).  The queue-pair batches fail where they are meant to."""
    pytest.importorskip("torch")
    from tests import test_gpu_prot as G

    for R in G.R_SET:
        for gather in (True, False):
            for n in G.N_SET:
                G.assert_mix(G.independent_batches(n, R, gather), n)
    for gather in (True, False):
        for f in (0, 63, 64, 4160, G.QP_N - 1, None):
            st, el, qp = G._qp_batch(gather, f).judge(0)
            if f is None:
                assert not st.any() and qp == 0
                continue
            assert not st[:f].any() and st[f] == REM and qp == 1
            assert (st[f + 1:] == FLUSH).all() and not el[f:].any()
            if f == 4160:  # on its own it fails in three waves' segments
                alone = G._qp_batch(gather, f).judge()[0]
                assert set(np.flatnonzero(alone)) == {
                    f, f + 5000, f + 30000}
