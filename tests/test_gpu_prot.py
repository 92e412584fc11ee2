"""GPU tests: memory protection in front of the byte-granular engine
(ops.gather_prot_ / scatter_prot_) against the numpy model
(utils.prot.prot_reference) plus a numpy / zlib model of the bytes, and
protected=True on the sdma transport and the soak.

Safety rule of this module: every address and length handed to the GPU,
accepted or rejected, lies inside memory the test owns (the runners
assert it before they launch).  An MR covers the middle of a larger
canary-filled buffer and "out of range" means outside the MR but inside
the buffer, so a wrong verdict shows as a changed canary or a wrong
status, never as a fault.  Negative lengths and ranges that wrap 2^64
are the CPU tier's (tests/test_prot.py): the verdict code is shared."""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rocnrdma_amd.utils import prot  # noqa: E402

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

# the length set and the skew pairs of tests/test_gpu_bytes.py
PAIR_LENS = [1, 15, 17, 4095, 4097]
LEN_SET = [0, 1, 3, 16, 33, 1023, 4080, 4095, 4096, 4097, 4113, 8191,
           3 * 4096 + 2049, 65537]
PROT_LENS = [ln for ln in LEN_SET if ln <= 4113]
CANARY = 0xA5
PAD = 64
RR, RW, LW = (prot.ACCESS_REMOTE_READ, prot.ACCESS_REMOTE_WRITE,
              prot.ACCESS_LOCAL_WRITE)
ALL = RR | RW | LW
S, LOC, FLUSH, REM = (prot.WC_SUCCESS, prot.WC_LOC_PROT_ERR,
                      prot.WC_WR_FLUSH_ERR, prot.WC_REM_ACCESS_ERR)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# -- one arena: the outside area, then the region ---------------------------
# Both sides of a message live in one device allocation, so that a table
# of a single MR can hold both.  The area that is read holds random
# bytes, the area that is written canaries.
class Batch:
    """Descriptors relative to the arena, an MR table relative to it,
    and what the models say."""

    def __init__(self, gather, area, out_at, reg_at, lens, keys, mrs):
        self.gather, self.area = gather, int(area)
        self.out_at, self.reg_at = _i64(out_at), _i64(reg_at)
        self.lens, self.keys = _i64(lens), _i64(keys)
        self.mrs = _i64(mrs).reshape(-1, 4)  # addr relative to the arena
        self.n = len(self.lens)
        # the safety rule: every range inside the area it belongs to
        for at in (self.out_at, self.reg_at):
            assert (at >= 0).all() and (self.lens >= 0).all()
            assert (at + self.lens <= self.area).all()
        assert self.area % 16 == 0

    @property
    def size(self):  # PAD | outside | PAD | region | PAD
        return 3 * PAD + 2 * self.area

    @property
    def out_base(self):
        return PAD

    @property
    def reg_base(self):
        return 2 * PAD + self.area

    def table(self, arena_addr):
        t = self.mrs.copy()
        t[:, 1] += arena_addr
        return t

    @functools.lru_cache(maxsize=None)
    def source(self):
        return np.random.default_rng(self.n + 7).integers(
            0, 256, self.size, dtype=np.uint8)

    def fresh(self):
        """The arena before a launch."""
        a = self.source().copy()
        lo = self.reg_base if self.gather else self.out_base
        a[:PAD] = CANARY
        a[lo - PAD:lo + self.area + PAD] = CANARY
        a[-PAD:] = CANARY
        return a

    @functools.lru_cache(maxsize=None)
    def judge(self, qp=None):
        """(status, elens, qp_out) by the model; the addresses are taken
        with the arena at 1 << 40 (a verdict does not depend on it)."""
        base = 1 << 40
        return prot.prot_reference(
            self.table(base), base + self.reg_base, self.reg_at,
            base + self.out_base + self.out_at, self.lens, self.keys,
            self.gather, qp_state=qp)

    @functools.lru_cache(maxsize=None)
    def expect(self, qp=None):
        """(status, arena afterwards, digests, qp_out) by the models."""
        st, el, qp_out = self.judge(qp)
        arena = self.fresh()
        crcs = np.zeros(self.n, dtype=np.uint32)
        src_at = (self.out_base + self.out_at if self.gather
                  else self.reg_base + self.reg_at)
        dst_at = (self.reg_base + self.reg_at if self.gather
                  else self.out_base + self.out_at)
        src = self.source()
        for m in np.flatnonzero(el):
            s = src[src_at[m]:src_at[m] + el[m]]
            arena[dst_at[m]:dst_at[m] + el[m]] = s
            crcs[m] = zlib.crc32(s.tobytes())
        return st, arena, crcs, qp_out


def _launch(b, dev, arena, qp=None, crc=True, grid_cap=0):
    import rocnrdma_amd.ops as ops

    assert arena.data_ptr() % 16 == 0 and arena.numel() == b.size
    region = arena[b.reg_base:]
    d = lambda a: torch.from_numpy(_i64(a)).to(dev)  # noqa: E731
    fn = ops.gather_prot_ if b.gather else ops.scatter_prot_
    return fn(region, d(b.reg_at),
              d(arena.data_ptr() + b.out_base + b.out_at), d(b.lens),
              d(b.keys), d(b.table(arena.data_ptr())), qp_state=qp, crc=crc,
              max_msg_bytes=int(b.lens.max()) if b.n else 0,
              grid_cap=grid_cap)


def _check(b, dev, qp_entry=None, crc=True, grid_cap=0):
    """Launch twice on the same tensors; status, landed bytes, canaries
    and digests against the models, and both launches alike."""
    st_w, arena_w, crc_w, qp_w = b.expect(qp_entry)
    arena = torch.from_numpy(b.fresh()).to(dev)
    outs = []
    for _ in range(2):
        qp = (None if qp_entry is None else
              torch.full((1,), qp_entry, dtype=torch.int32, device=dev))
        st, dig = _launch(b, dev, arena, qp=qp, crc=crc, grid_cap=grid_cap)
        assert st.dtype == torch.int32 and st.shape == (b.n,)
        assert (st.cpu().numpy() == st_w).all()
        assert (arena.cpu().numpy() == arena_w).all()
        if qp is not None:
            assert int(qp.item()) == qp_w
        if crc:
            assert dig.dtype == torch.int32 and dig.shape == (b.n,)
            assert (_u32(dig) == crc_w).all()
        else:
            assert dig is None
        outs.append((st, dig))
    assert torch.equal(outs[0][0], outs[1][0])  # no stale scratch
    assert crc is False or torch.equal(outs[0][1], outs[1][1])
    return st_w


# -- the seeded generator of hostile batches --------------------------------
def _lens(g, n):
    """Lengths up to 4113; large batches are mostly short messages so
    that 65537 of them stay a few MiB."""
    big = g.choice(PROT_LENS, n)
    if n <= 1025:
        return big.astype(np.int64)
    small = g.integers(0, 41, n)
    return np.where(g.random(n) < 0.04, big, small).astype(np.int64)


def _place(g, lens):
    """Every message in its own range, a seeded gap of 0..19 bytes in
    front of it: any skew, neighbours share granules."""
    step = lens + g.integers(0, 20, len(lens))
    at = np.cumsum(step) - lens
    return at, int(at[-1] + lens[-1])


@functools.lru_cache(maxsize=None)
def hostile_batch(n, R, gather, seed=0):
    """n messages against a table of R MRs.  R == 1: one MR with every
    right from the middle of the outside area to the middle of the
    region.  R >= 2: even rows are windows of the outside area, odd rows
    windows of the region, each from somewhere in the first fifth to
    somewhere in the last fifth; from row 2 on a tenth of the rows is
    free and a tenth lacks a right.  A message takes a row of the right
    kind for nine tenths of its keys and any row otherwise; a twentieth
    of the keys carries a stale tag, a thirtieth a slot >= R.
    n == 1: one non-empty message in the middle of both areas with the
    keys of rows 0 and 1, which hold it; seed 1 makes its lkey stale,
    seed 2 its rkey."""
    g = np.random.default_rng(1000 * R + 10 * n + gather + 7919 * seed)
    lens = _lens(g, n)
    out_at, used_o = _place(g, lens)
    reg_at, used_r = _place(g, lens)
    area = (max(used_o, used_r) + 64) // 16 * 16
    if n == 1:
        lens[0] = PROT_LENS[1 + int(g.integers(len(PROT_LENS) - 1))]
        area = 3 * 4224
        out_at, reg_at = out_at + area // 3, reg_at + area // 3
    out_base, reg_base = PAD, 2 * PAD + area
    mrs = np.zeros((R, 4), dtype=np.int64)
    tags = g.integers(0, 256, R)
    mrs[:, 0] = (np.arange(R) << 8) | tags
    if R == 1:
        lo = out_base + area // 4
        hi = reg_base + 3 * area // 4
        mrs[0, 1:] = (lo, hi - lo, ALL)
        lk = rk = np.zeros(n, dtype=np.int64)
    else:
        kind = np.arange(R) % 2  # 0: outside, 1: region
        lo = g.integers(0, area // 5 + 1, R)
        hi = area - g.integers(0, area // 5 + 1, R)
        mrs[:, 1] = np.where(kind == 0, out_base, reg_base) + lo
        mrs[:, 2] = hi - lo
        fate = g.random(R)
        fate[:2] = 1.0
        weak_o = g.choice([RR, RW, RR | RW], R)  # no LOCAL_WRITE
        weak_r = g.choice([RR, RW, LW], R)       # lacks one remote right
        mrs[:, 3] = np.where(fate < 0.1, 0,
                             np.where(fate < 0.2,
                                      np.where(kind == 0, weak_o, weak_r),
                                      np.where(kind == 0, LW | RR,
                                               RR | RW)))
        n_out, n_reg = (R + 1) // 2, R // 2

        def pick(count, first):
            right = 2 * g.integers(0, count, n) + first
            return np.where(g.random(n) < 0.9, right, g.integers(0, R, n))
        lk, rk = pick(n_out, 0), pick(n_reg, 1)

    def key_of(slot):
        key = mrs[slot, 0].copy()
        u = g.random(n)
        key = np.where(u < 0.05, key ^ 1, key)
        return np.where((u >= 0.05) & (u < 0.083),
                        ((R + g.integers(0, 3, n)) << 8) | 1, key)
    keys = prot.pack_keys(key_of(lk), key_of(rk))
    if n == 1:
        rows = (0, 0) if R == 1 else (0, 1)
        keys = prot.pack_keys(mrs[rows[0], 0] ^ (seed == 1),
                              mrs[rows[1], 0] ^ (seed == 2)).reshape(1)
    return Batch(bool(gather), area, out_at, reg_at, lens, keys, mrs)


def status_mix(st, lens):
    """(SUCCESS share of the non-empty messages, the set of statuses)."""
    busy = lens > 0
    share = float((st[busy] == S).sum()) / max(int(busy.sum()), 1)
    return share, set(st.tolist())


N_SET = [1, 63, 64, 65, 1024, 1025, 65537]
R_SET = [1, 2, 64, 4097]
# n == 1 cannot hold three statuses: three single-message batches per R
# and direction (valid, stale lkey, stale rkey) hold them between them


def independent_batches(n, R, gather):
    if n > 1:
        return [hostile_batch(n, R, gather)]
    return [hostile_batch(1, R, gather, seed) for seed in (0, 1, 2)]


def assert_mix(batches, n):
    """What the issue asks of the generator, on the model's output."""
    seen = set()
    for b in batches:
        st = b.judge()[0]
        share, kinds = status_mix(st, b.lens)
        seen |= kinds
        if n >= 63:
            assert 0.25 <= share <= 0.75, (n, share)
        assert FLUSH not in kinds
    assert {S, LOC, REM} <= seen, (n, seen)


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "scatter"])
@pytest.mark.parametrize("R", R_SET)
@pytest.mark.parametrize("n", N_SET)
def test_independent_mode(dev, n, R, gather):
    batches = independent_batches(n, R, gather)
    assert_mix(batches, n)
    for b in batches:
        _check(b, dev)
    if n == 1025:  # no digests asked for: the same bytes and statuses
        _check(batches[0], dev, crc=False)
        _check(batches[0], dev, grid_cap=1)


# -- equivalence with the unprotected engine --------------------------------
HOST_BYTES = 6 << 20
SLOT = 4096 + 2 * PAD


@pytest.fixture(scope="module")
def host():
    t = torch.empty(HOST_BYTES, dtype=torch.uint8, pin_memory=True)
    assert t.data_ptr() % 16 == 0
    t.numpy()[:] = np.random.default_rng(79).integers(
        0, 256, HOST_BYTES, dtype=np.uint8)
    return t


@pytest.fixture(scope="module")
def hbm_src(dev, host):
    return host.to(dev)


def _pairs():
    lens, read_at, write_at = [], [], []
    k = 0
    for ln in PAIR_LENS:
        for ss in range(16):
            for ds in range(16):
                lens.append(ln)
                read_at.append(k * SLOT + 32 + ss)
                write_at.append(k * SLOT + 32 + ds)
                k += 1
    return _i64(lens), _i64(read_at), _i64(write_at)


def _packed(lens, base, seed=None):
    lens = _i64(lens)
    if seed is None:
        return base + np.cumsum(lens) - lens
    perm = np.random.default_rng(seed).permutation(len(lens))
    offs = np.empty(len(lens), dtype=np.int64)
    offs[perm] = base + np.cumsum(lens[perm]) - lens[perm]
    return offs


def _equiv_batches():
    lens, read_at, write_at = _pairs()
    yield lens, read_at, write_at
    for n in (1, 5, 37):
        ml = np.random.default_rng(2000 + n).choice(LEN_SET, n)
        ml = ml.astype(np.int64)
        yield ml, _packed(ml, 16 * 5 + 3), _packed(ml, PAD + 11, seed=1)


@pytest.mark.parametrize("grid_cap", [0, 1])
@pytest.mark.parametrize("crc", [False, True])
def test_valid_keys_equal_the_bytes_engine(host, hbm_src, dev, crc, grid_cap):
    """A table that covers everything, valid keys, no queue-pair word:
    statuses all 0, bytes and digests bit for bit gather_bytes_ /
    scatter_bytes_."""
    import rocnrdma_amd.ops as ops

    kw = dict(crc=crc, grid_cap=grid_cap)
    for lens, read_at, write_at in _equiv_batches():
        n = len(lens)
        size = int((write_at + lens).max()) + PAD
        assert int((read_at + lens).max()) <= HOST_BYTES
        d_lens = torch.from_numpy(lens).to(dev)
        keys = torch.from_numpy(np.full(
            n, int(prot.pack_keys(prot.make_key(1, 9), prot.make_key(0, 3))),
            dtype=np.int64)).to(dev)

        def table(reg, out):
            return torch.tensor(
                [[prot.make_key(0, 3), reg.data_ptr(), reg.numel(), RR | RW],
                 [prot.make_key(1, 9), out.data_ptr(), out.numel(), LW]],
                dtype=torch.int64, device=dev)
        # gather: pinned host -> canary region
        d_offs = torch.from_numpy(write_at).to(dev)
        d_addrs = torch.from_numpy(host.data_ptr() + read_at).to(dev)
        a = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
        b = a.clone()
        want = ops.gather_bytes_(a, d_offs, d_addrs, d_lens, **kw)
        st, got = ops.gather_prot_(b, d_offs, d_addrs, d_lens, keys,
                                   table(b, host), **kw)
        assert not st.any() and torch.equal(a, b)
        assert (got is None and want is None) if not crc \
            else torch.equal(got, want)
        # scatter: random region -> canary pinned buffers
        d_offs = torch.from_numpy(read_at).to(dev)
        dst = [torch.empty(size, dtype=torch.uint8, pin_memory=True)
               for _ in range(2)]
        for t in dst:
            t.fill_(CANARY)
        d_addrs = [torch.from_numpy(t.data_ptr() + write_at).to(dev)
                   for t in dst]
        want = ops.scatter_bytes_(hbm_src, d_offs, d_addrs[0], d_lens, **kw)
        st, got = ops.scatter_prot_(hbm_src, d_offs, d_addrs[1], d_lens,
                                    keys, table(hbm_src, dst[1]), **kw)
        torch.cuda.synchronize(dev)
        assert not st.any() and torch.equal(dst[0], dst[1])
        assert (got is None and want is None) if not crc \
            else torch.equal(got, want)


# -- queue-pair mode --------------------------------------------------------
QP_N = 65537  # block_scan's segments are 4160 messages long


@functools.lru_cache(maxsize=None)
def _qp_batch(gather, f, n=QP_N):
    """All valid but message f (a stale rkey) and, well behind it in
    other waves' segments, two more failures that must come out flushed.
    f None: all valid."""
    g = np.random.default_rng(5 + gather)
    lens = _lens(g, n)
    lens[[0, 63, 64, 4160 % n, n - 1]] = 33  # none of the f's is empty
    out_at, used_o = _place(g, lens)
    reg_at, used_r = _place(g, lens)
    area = (max(used_o, used_r) + 64) // 16 * 16
    out_base, reg_base = PAD, 2 * PAD + area
    # the MRs: the used part of either area; one region byte short for
    # the key that fails
    mrs = _i64([[prot.make_key(0, 1), out_base, used_o, LW | RR],
                [prot.make_key(1, 2), reg_base, used_r, RR | RW],
                [prot.make_key(2, 3), reg_base + 1, used_r - 2, RR | RW]])
    rk = np.full(n, prot.make_key(1, 2), dtype=np.int64)
    lk = np.full(n, prot.make_key(0, 1), dtype=np.int64)
    if f is not None:
        rk[f] = prot.make_key(2, 3) ^ 1  # stale
        for later in (f + 5000, f + 30000):
            if later < n:
                lk[later] = prot.make_key(1, 2)  # the wrong side's MR
    return Batch(bool(gather), area, out_at, reg_at, lens,
                 prot.pack_keys(lk, rk), mrs)


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "scatter"])
@pytest.mark.parametrize("f", [0, 63, 64, 4160, QP_N - 1, None])
def test_qp_mode_flushes_behind_the_first_failure(dev, gather, f):
    b = _qp_batch(gather, f)
    st = _check(b, dev, qp_entry=0)
    # the model itself: nothing at or behind f completes with SUCCESS
    if f is None:
        assert not st.any() and b.expect(0)[3] == 0
        return
    assert not st[:f].any() and st[f] == REM
    assert (st[f + 1:] == FLUSH).all() and b.expect(0)[3] == 1
    moved = np.flatnonzero(b.expect(0)[1] != b.fresh())
    dst0 = (b.reg_base + b.reg_at if gather else b.out_base + b.out_at)[f]
    assert not moved.size or moved.max() < dst0


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "scatter"])
def test_qp_word_in_error_flushes_a_valid_batch(dev, gather):
    bad, good = _qp_batch(gather, 64, n=1025), _qp_batch(gather, None, n=1025)
    arena = torch.from_numpy(bad.fresh()).to(dev)
    qp = torch.zeros(1, dtype=torch.int32, device=dev)
    st, _ = _launch(bad, dev, arena, qp=qp)
    assert (st.cpu().numpy() == bad.expect(0)[0]).all()
    assert int(qp.item()) == 1
    # a second, all-valid batch on the same word: flushed, nothing moves
    arena = torch.from_numpy(good.fresh()).to(dev)
    st, dig = _launch(good, dev, arena, qp=qp)
    assert (st == FLUSH).all() and not dig.any() and int(qp.item()) == 1
    assert (arena.cpu().numpy() == good.fresh()).all()
    assert (st.cpu().numpy() == good.expect(1)[0]).all()
    qp.zero_()
    st, dig = _launch(good, dev, arena, qp=qp)
    assert not st.any() and int(qp.item()) == 0
    assert (arena.cpu().numpy() == good.expect(0)[1]).all()
    assert (_u32(dig) == good.expect(0)[2]).all()


def test_empty_batch_leaves_the_word_alone(dev):
    import rocnrdma_amd.ops as ops

    region = torch.full((256,), CANARY, dtype=torch.uint8, device=dev)
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    mrs = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    qp = torch.full((1,), 7, dtype=torch.int32, device=dev)
    st, dig = ops.gather_prot_(region, e, e, e, e, mrs, qp_state=qp, crc=True)
    assert st.shape == (0,) and dig.shape == (0,) and int(qp.item()) == 7
    assert (region == CANARY).all()


# -- access rights ----------------------------------------------------------
def test_access_rights(dev):
    """One message per launch through MRs that grant one right each."""
    area = 4096
    out_base, reg_base = PAD, 2 * PAD + area
    rows = [(out_base + 512, 2048, LW), (out_base + 512, 2048, RR),
            (reg_base + 512, 2048, RR | RW), (reg_base + 512, 2048, RR),
            (reg_base + 512, 2048, RW)]
    mrs = _i64([[prot.make_key(s, 5), a, ln, acc]
                for s, (a, ln, acc) in enumerate(rows)])
    key = lambda s: prot.make_key(s, 5)  # noqa: E731
    cases = [  # gather?, lkey row, rkey row, status
        (True, 0, 2, S), (False, 0, 2, S),
        (True, 0, 3, REM),   # a gather writes the region: needs REMOTE_WRITE
        (True, 0, 4, S),
        (False, 0, 4, REM),  # a scatter reads the region: needs REMOTE_READ
        (False, 0, 3, S),
        (False, 1, 2, LOC),  # a scatter writes outside: needs LOCAL_WRITE
        (True, 1, 2, S),     # a gather only reads it
    ]
    for gather, lrow, rrow, want in cases:
        b = Batch(gather, area, [700, 600], [900, 1000], [100, 0],
                  prot.pack_keys([key(lrow)] * 2, [key(rrow)] * 2), mrs)
        st = _check(b, dev)
        assert st.tolist() == [want, S], (gather, lrow, rrow)
        st = _check(b, dev, qp_entry=0)
        assert st.tolist() == [want, S if want == S else FLUSH]


# -- host-visible argument errors -------------------------------------------
def test_argument_errors_raise_before_any_launch(dev):
    import rocnrdma_amd.ops as ops

    region = torch.full((4096,), CANARY, dtype=torch.uint8, device=dev)
    v = torch.zeros(4, dtype=torch.int64, device=dev)
    mrs = torch.zeros((2, 4), dtype=torch.int64, device=dev)
    qp = torch.zeros(1, dtype=torch.int32, device=dev)
    ok = dict(region=region, dst_offs=v, src_addrs=v, lens=v, keys=v, mrs=mrs)

    def call(**over):
        kw = {**ok, **over}
        return ops.gather_prot_(kw.pop("region"), kw.pop("dst_offs"),
                                kw.pop("src_addrs"), kw.pop("lens"),
                                kw.pop("keys"), kw.pop("mrs"), **kw)
    assert not call()[0].any()
    bad = [dict(keys=v[:3]), dict(lens=v[:3]), dict(keys=v.cpu()),
           dict(keys=v.to(torch.int32)), dict(mrs=mrs.cpu()),
           dict(mrs=mrs.reshape(-1)), dict(mrs=mrs[:, :3]),
           dict(mrs=mrs[:0]), dict(mrs=mrs.to(torch.int32)),
           dict(mrs=torch.zeros((2, 8), dtype=torch.int64,
                                device=dev)[:, :4]),
           dict(qp_state=qp.to(torch.int64)), dict(qp_state=qp.cpu()),
           dict(qp_state=torch.zeros(2, dtype=torch.int32, device=dev)),
           dict(qp_state=torch.zeros((1, 1), dtype=torch.int32, device=dev)),
           dict(region=region[1:]), dict(grid_cap=-1),
           dict(max_msg_bytes=-1)]
    for over in bad:
        with pytest.raises(RuntimeError):
            call(**over)
    with pytest.raises(RuntimeError, match="n mismatch"):
        call(keys=v[:3])
    with pytest.raises(RuntimeError):
        ops.scatter_prot_(region, v, v, v, v[:2], mrs)
    assert (region == CANARY).all() and int(qp.item()) == 0


# -- the sdma transport -----------------------------------------------------
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_post_and_post_many_agree(direction):
    from tests.test_prot import check_post_and_post_many_agree

    check_post_and_post_many_agree("sdma", direction, inflight=8)


@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_reg_dereg_and_tags(direction):
    from tests.test_prot import check_reg_dereg_and_tags

    check_reg_dereg_and_tags("sdma", direction, inflight=8)


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_error_flushes_across_ring(direction, icrc):
    from tests.test_prot import check_error_flushes_across_ring

    check_error_flushes_across_ring("sdma", direction, inflight=8, icrc=icrc)


@pytest.mark.parametrize("icrc", [False, True])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_sdma_digest_and_integrity_check(direction, icrc):
    from tests.test_prot import check_digest_and_integrity

    check_digest_and_integrity("sdma", direction, inflight=8, icrc=icrc)


def test_sdma_protected_validation():
    from rocnrdma_amd.transport import get_transport

    kw = dict(msg_bytes=8192, region_bytes=128 << 10, var_len=True,
              byte_granular=True, protected=True)
    with pytest.raises(ValueError, match="kernel engine"):
        get_transport("sdma", engine="stream", **kw)
    tp = get_transport("sdma", **kw)
    assert tp.protected and tp.supports_protection
    assert tp.completions().size == 0 and not tp.qp_in_error()
    assert tp.prot_stats() == {"ok": 0, "errors": 0, "flushed": 0}
    tp.close()
    tp = get_transport("sdma", msg_bytes=8192, region_bytes=128 << 10,
                       var_len=True, byte_granular=True)
    with pytest.raises(ValueError, match="protected"):
        tp.post(0, 16, rkey=1)
    with pytest.raises(ValueError, match="protected"):
        tp.post_many(0, 2, 16, rkey=1)
    tp.close()


def test_soak_prot_bounded():
    from rocnrdma_amd.harness.soak import run_soak

    for icrc in (False, True):
        stats = run_soak("sdma", secs=1.0, region_bytes=16 << 20, seed=11,
                         mixed=True, byte_granular=True, prot=True, icrc=icrc)
        assert stats["cycles"] > 0 and stats["failures"] == 0
        assert stats["prot_rejected"] > 0 and stats["prot_flushed"] > 0
