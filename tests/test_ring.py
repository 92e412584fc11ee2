"""The transports' ring semantics against a model (CPU tier: `fake`).

The contract is in rocnrdma_amd/transport/base.py (class Transport).
`RingModel` states it once more in plain numpy, zlib and Python
integers, `make_script` draws scripts of scalar and vectorized posts,
flushes, stamps and sender corruptions over a ring that divides neither
the region nor the counts posted, and `check_ring_replay` plays a script
on a transport and on the model: digests and statuses of every batch,
the counters, and at the end every byte of the region and of the slots
(both start as random bytes, so every untouched byte is a canary).
tests/test_gpu_ring.py plays the same scripts on sdma.  Every comparison
is exact.

The model takes nothing from rocnrdma_amd.transport: the player opens a
transport, the model only ever sees integers and its own arrays."""
import zlib

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

# -- geometries: the smallest at which the ring can go wrong ----------------
# A: two 4 KiB chunks per message; the ring divides neither the region's
#    message count nor the counts drawn
GEOM_A = dict(msg_bytes=8192, msgs_per_region=11, inflight=4)
# B: bench's step shape — one post_many over a ring much smaller than the
#    region, from a start that is no multiple of anything: 16 refills, a wrap
GEOM_B = dict(msg_bytes=4096, msgs_per_region=257, inflight=48)
B_START, B_COUNT = 7, 3 * 257 + 5

# mode -> what the transport is opened with
MODES = {
    "plain": {},
    "icrc": dict(icrc=True),
    "var_len": dict(var_len=True),
    "var_len_icrc": dict(var_len=True, icrc=True),
    "bytes": dict(var_len=True, byte_granular=True, region_skew=5,
                  staging_skew=9),
    "bytes_icrc": dict(var_len=True, byte_granular=True, region_skew=5,
                       staging_skew=9, icrc=True),
    "sg": dict(var_len=True, byte_granular=True, region_skew=3, max_sge=3),
    "sg_icrc": dict(var_len=True, byte_granular=True, region_skew=3,
                    max_sge=3, icrc=True),
    "protected": dict(var_len=True, byte_granular=True, region_skew=5,
                      staging_skew=9, protected=True),
}
DIRECTIONS = ["write", "read"]
WINDOW_MSGS = 5  # the protected mode's window MR: region messages 0..4


# -- the model --------------------------------------------------------------
class RingModel:
    """One transport's memory, ring and counters.  A post is (i, pieces):
    pieces are the (slot_off, nbytes) ranges of staging slot i % inflight
    whose concatenation is the message; it sits in the region at
    (i % msgs_per_region) * msg_bytes + region_skew."""

    def __init__(self, msg_bytes, msgs_per_region, inflight, direction,
                 region_skew=0, ordered=False):
        assert direction in ("write", "read")
        self.msg = int(msg_bytes)
        self.n_msgs = int(msgs_per_region)
        self.inflight = max(1, min(int(inflight), self.n_msgs))
        self.write = direction == "write"
        self.region_skew = int(region_skew)
        # ordered: the backend keeps post order per destination, so a
        # script may repeat one between two retirements
        self.ordered = ordered
        self.region = np.zeros(self.msg * self.n_msgs, dtype=np.uint8)
        self.slots = np.zeros((self.inflight, self.msg), dtype=np.uint8)
        self.pending = 0
        self.batch = []        # digests of the pending posts
        self.dests = set()     # their destinations
        self.last = None       # digests of the last batch
        self.retired = 0       # batches retired so far
        self.posts = 0
        self.expected = None   # the stamp
        self.checked = self.bad = 0

    def dest(self, i):
        return i % self.n_msgs if self.write else i % self.inflight

    def post(self, i, pieces):
        if self.pending == self.inflight:
            self.flush()
        d = self.dest(i)
        # the destination rule: a condition of every script, not a tolerance
        assert self.ordered or d not in self.dests, \
            f"script posts destination {d} twice in one batch"
        self.dests.add(d)
        slot = self.slots[i % self.inflight]
        total = sum(k for _, k in pieces)
        off = (i % self.n_msgs) * self.msg + self.region_skew
        assert off + total <= (i % self.n_msgs + 1) * self.msg
        there = self.region[off:off + total]
        if self.write:
            data = np.concatenate(
                [slot[o:o + k] for o, k in pieces] +
                [np.zeros(0, dtype=np.uint8)])
            there[:] = data
        else:
            data = there.copy()
            at = 0
            for o, k in pieces:
                assert o + k <= self.msg
                slot[o:o + k] = data[at:at + k]
                at += k
        crc = zlib.crc32(data.tobytes()) if total else 0
        self.batch.append(crc)
        if self.expected is not None:
            self.checked += 1
            self.bad += crc != self.expected[
                i % self.inflight if self.write else i % self.n_msgs]
        self.pending += 1
        self.posts += 1

    def flush(self):
        """True if there was anything to retire."""
        if not self.pending:
            return False
        self.last = np.array(self.batch, dtype=np.uint32)
        self.batch, self.dests, self.pending = [], set(), 0
        self.retired += 1
        return True

    def sender(self):
        return self.slots if self.write else self.region.reshape(-1, self.msg)

    def stamp(self):
        assert not self.pending
        self.expected = [zlib.crc32(m.tobytes()) for m in self.sender()]

    def corrupt_sender(self, where):
        # never between a post and the flush that retires it
        assert not self.pending
        self.sender()[where, 1] ^= 0x40


# -- scripts ----------------------------------------------------------------
def _edge_lengths(mode, msg, max_nbytes):
    if mode.startswith("var_len"):
        edges = [0, 16, 4096, 4112, msg]
    else:
        edges = [0, 1, 17, 4095, 4097, max_nbytes]
    return [e for e in edges if e <= max_nbytes]


def _draw_pieces(rng, mode, msg, kw):
    """The pieces of one message of `mode`."""
    rs, ss = kw.get("region_skew", 0), kw.get("staging_skew", 0)
    if mode in ("plain", "icrc"):
        return [(0, msg)]
    if "max_sge" not in kw:
        edges = _edge_lengths(mode, msg, msg - max(rs, ss))
        return [(ss, int(rng.choice(edges)))]
    room = msg - rs
    if rng.random() < 0.1:  # one SGE at the front: what post(i, nbytes) is
        return [(0, int(rng.integers(0, room + 1)))]
    lens = []
    for _ in range(int(rng.integers(0, kw["max_sge"] + 1))):
        small = [0, 1, 17, 4095, 4097]
        k = int(rng.choice(small) if rng.random() < 0.5
                else rng.integers(0, room + 1))
        k = min(k, room - sum(lens))
        lens.append(k)
    # disjoint ranges of the slot, in a list order of their own
    gaps = rng.multinomial(msg - sum(lens), np.ones(len(lens) + 1) /
                           (len(lens) + 1))
    order = rng.permutation(len(lens))
    pieces, at = [None] * len(lens), 0
    for pos, which in enumerate(order):
        at += int(gaps[pos])
        pieces[which] = (at, lens[which])
        at += lens[which]
    return pieces


def make_script(seed, mode, direction, msg_bytes, msgs_per_region, inflight,
                ops=40, ordered=False):
    """About `ops` operations.  Unless `ordered`, an explicit flush goes in
    front of every post whose destination the batch already holds (ring-full
    retirements counted), splitting a post_many where it has to."""
    kw = MODES[mode]
    rng = np.random.default_rng([seed, sorted(MODES).index(mode),
                                 int(direction == "read")])
    inflight = max(1, min(inflight, msgs_per_region))
    script, state = [], dict(pending=0, dests=set())

    def flush():
        script.append(("flush",))
        state.update(pending=0, dests=set())

    def posts(start, n, pieces, many):
        run_from = 0
        for k in range(n):
            i = start + k
            if state["pending"] == inflight:
                state.update(pending=0, dests=set())
            d = (i % msgs_per_region if direction == "write"
                 else i % inflight)
            if d in state["dests"] and not ordered:
                emit(start + run_from, pieces[run_from:k], many)
                run_from = k
                flush()
            state["dests"].add(d)
            state["pending"] += 1
        emit(start + run_from, pieces[run_from:], many)

    def emit(start, pieces, many):
        if not pieces:
            return
        if many:
            script.append(("post_many", start, len(pieces), pieces))
        else:
            assert len(pieces) == 1
            script.append(("post", start, pieces[0]))

    nxt = int(rng.integers(0, 10_000))
    stamps = mode == "icrc"
    while len(script) < ops:
        r = rng.random()
        if rng.random() < 0.2:
            nxt = int(rng.integers(0, 10_000))
        if r < 0.45:
            n = int(rng.integers(1, 3 * inflight + 1))
            posts(nxt, n, [_draw_pieces(rng, mode, msg_bytes, kw)
                           for _ in range(n)], True)
            nxt += n
        elif r < 0.8:
            posts(nxt, 1, [_draw_pieces(rng, mode, msg_bytes, kw)], False)
            nxt += 1
        elif r < 0.92 or not stamps:
            flush()
            if rng.random() < 0.3:
                flush()  # an empty one
        elif r < 0.96:
            flush()
            script.append(("stamp",))
        else:
            flush()
            n_senders = inflight if direction == "write" else msgs_per_region
            script.append(("corrupt_sender", int(rng.integers(0, n_senders))))
    flush()
    return script


def stamped_script(direction, msgs_per_region, inflight, start, count):
    """Stamped icrc in three phases of the same region passes (one
    post_many each): clean, one sender byte flipped (slot 3 / region
    message 3), stamped again.  Returns (phases, bad): the scripts and,
    per pass, how many of its messages the flipped byte is in — the posts
    with i % inflight == 3 for a write, i % msgs_per_region == 3 for a
    read."""
    modulus = inflight if direction == "write" else msgs_per_region
    assert modulus > 3
    passes = [(start, count), (start + count, count)]
    pieces = None  # whole slots
    run = [op for s, n in passes
           for op in (("post_many", s, n, pieces), ("flush",))]
    hits = [sum(i % modulus == 3 for i in range(s, s + n))
            for s, n in passes]
    phases = [[("stamp",)] + run,
              [("corrupt_sender", 3)] + run,
              [("stamp",)] + run]
    return phases, hits


# -- the player -------------------------------------------------------------
class Replay:
    """A transport and its model, side by side."""

    def __init__(self, name, mode, direction, seed, msg_bytes,
                 msgs_per_region, inflight, ordered=False, **open_kw):
        from rocnrdma_amd.transport import get_transport

        self.mode, self.kw = mode, MODES[mode]
        self.tp = tp = get_transport(
            name, msg_bytes=msg_bytes,
            region_bytes=msg_bytes * msgs_per_region, inflight=inflight,
            direction=direction, **self.kw, **open_kw)
        self.model = m = RingModel(
            msg_bytes, msgs_per_region, inflight, direction,
            region_skew=self.kw.get("region_skew", 0), ordered=ordered)
        assert tp.inflight == m.inflight
        rng = np.random.default_rng([seed, 77])
        m.region[:] = rng.integers(0, 256, m.region.shape, dtype=np.uint8)
        m.slots[:] = rng.integers(0, 256, m.slots.shape, dtype=np.uint8)
        tp._region_set(m.region.copy())
        tp._slots[:] = m.slots
        self.icrc = bool(self.kw.get("icrc"))
        self.protected = bool(self.kw.get("protected"))
        self.sg = "max_sge" in self.kw
        self.seen = 0  # model batches compared so far
        if self.protected:
            from rocnrdma_amd.utils import prot

            self.window = tp.reg_mr(
                "region", 0, min(WINDOW_MSGS, msgs_per_region) * msg_bytes,
                prot.ACCESS_REMOTE_READ | prot.ACCESS_REMOTE_WRITE)

    def _rkey(self, i):
        """Every other message inside the window goes through its MR."""
        inside = i % self.model.n_msgs < WINDOW_MSGS
        return self.window if inside and i % 2 else self.tp.region_key

    def _post(self, i, pieces):
        tp = self.tp
        if self.sg:
            if len(pieces) == 1 and pieces[0][0] == 0 and i % 2:
                tp.post(i, pieces[0][1])
            else:
                tp.post_sg(i, pieces)
        elif self.protected:
            tp.post(i, pieces[0][1], rkey=self._rkey(i))
        elif self.kw.get("var_len"):
            tp.post(i, pieces[0][1])
        else:
            tp.post(i)

    def _post_many(self, start, n, pieces):
        tp = self.tp
        if self.sg:
            arr = np.zeros((n, self.kw["max_sge"], 2), dtype=np.int64)
            for k, p in enumerate(pieces):
                arr[k, :len(p)] = np.array(p, dtype=np.int64).reshape(-1, 2)
            tp.post_many_sg(start, n, arr)
            return
        if not self.kw.get("var_len"):
            tp.post_many(start, n)
            return
        lens = np.array([p[0][1] for p in pieces], dtype=np.int64)
        if self.protected:
            rkeys = np.array([self._rkey(start + k) for k in range(n)])
            tp.post_many(start, n, lens, rkey=rkeys)
        else:
            tp.post_many(start, n, lens)

    def _check_last_batch(self, what):
        """The last batch as the transport published it, whenever the
        model says one was retired — by this flush or by a full ring —,
        and after a flush that retired nothing: it must have stayed."""
        tp, m = self.tp, self.model
        if self.icrc:
            if m.last is None:
                assert tp._last_digests is None, what
            else:
                got = tp._gather_host([tp._last_digests]).view(np.uint32)
                assert np.array_equal(got, m.last), (what, got, m.last)
        if self.protected and m.last is not None:
            got = tp.completions()
            assert got.tolist() == [0] * len(m.last), (what, got)  # SUCCESS
        self.seen = m.retired

    def play(self, script):
        tp, m = self.tp, self.model
        whole = [(0, m.msg)]
        for step, op in enumerate(script):
            what = (step, op[:3])
            if op[0] == "post":
                _, i, pieces = op
                m.post(i, pieces)
                self._post(i, pieces)
            elif op[0] == "post_many":
                _, start, n, pieces = op
                pieces = pieces or [whole] * n
                for k in range(n):
                    m.post(start + k, pieces[k])
                self._post_many(start, n, pieces)
            elif op[0] == "flush":
                m.flush()
                tp.flush()
                self._check_last_batch(what)
            elif op[0] == "stamp":
                m.stamp()
                tp.stamp()
            elif op[0] == "corrupt_sender":
                m.corrupt_sender(op[1])
                if m.write:
                    tp._slots[op[1], 1] ^= 0x40
                else:
                    tp._region_set(m.region.copy())
            else:
                raise ValueError(op)
            if m.retired != self.seen and m.pending:
                # a full ring retired inside this op and more was posted
                # behind it: the pending posts are not yet "last batch"
                self._check_last_batch(what)

    def check_stats(self):
        """The counters; reading them retires the ring."""
        tp, m = self.tp, self.model
        if self.icrc:
            m.flush()
            assert tp.icrc_stats() == {"checked": m.checked, "bad": m.bad}
            self._check_last_batch("icrc_stats")
        if self.protected:
            m.flush()
            assert tp.prot_stats() == {"ok": m.posts, "errors": 0,
                                       "flushed": 0}
            assert not tp.qp_in_error()
            self._check_last_batch("prot_stats")

    def check_memory(self):
        tp, m = self.tp, self.model
        assert not m.pending
        tp.flush()
        region, slots = np.asarray(tp._region_get()), np.asarray(tp._slots)
        bad = np.flatnonzero(region != m.region)
        assert not bad.size, \
            f"region differs at {bad[:8]} ({bad.size} bytes), message " \
            f"{bad[0] // m.msg}"
        bad = np.argwhere(slots != m.slots)
        assert not bad.size, \
            f"slots differ at {bad[:8].tolist()} ({len(bad)} bytes)"

    def close(self):
        self.tp.close()


def check_ring_replay(name, mode, direction, seed, msg_bytes,
                      msgs_per_region, inflight, script=None, ordered=False,
                      **open_kw):
    """Play the seed's script (or `script`) on transport `name` opened in
    `mode` and on the model; compare everything the contract speaks of."""
    if script is None:
        script = make_script(seed, mode, direction, msg_bytes,
                             msgs_per_region, inflight, ordered=ordered)
    rp = Replay(name, mode, direction, seed, msg_bytes, msgs_per_region,
                inflight, ordered=ordered, **open_kw)
    try:
        rp.play(script)
        rp.check_stats()
        rp.check_memory()
    finally:
        rp.close()
    return rp.model


def check_stamped_replay(name, direction, seed, msg_bytes, msgs_per_region,
                         inflight, start, count, **open_kw):
    """Stamped icrc: checked / bad against the model after each phase,
    and against the count of posts the flipped byte is in."""
    phases, hits = stamped_script(direction, msgs_per_region, inflight,
                                  start, count)
    rp = Replay(name, "icrc", direction, seed, msg_bytes, msgs_per_region,
                inflight, **open_kw)
    try:
        want_bad = [0, sum(hits), sum(hits)]
        for k, script in enumerate(phases):
            rp.play(script)
            rp.check_stats()
            m = rp.model
            assert (m.checked, m.bad) == (2 * count * (k + 1), want_bad[k])
        rp.check_memory()
    finally:
        rp.close()
    return hits


# -- CPU tests ----------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("mode", list(MODES))
def test_fake_ring_replay(mode, direction, seed):
    check_ring_replay("fake", mode, direction, seed, **GEOM_A)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_fake_ring_replay_bench_shape(direction):
    script = [("post_many", B_START, B_COUNT, None), ("flush",)]
    m = check_ring_replay("fake", "plain", direction, 0, script=script,
                          **GEOM_B)
    assert m.retired == -(-B_COUNT // GEOM_B["inflight"]) == 17


@pytest.mark.parametrize("geom", [GEOM_A, GEOM_B], ids=["A", "B"])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_fake_stamped_icrc(direction, geom):
    start, count = ((B_START, B_COUNT) if geom is GEOM_B
                    else (7, 3 * geom["msgs_per_region"] + 5))
    hits = check_stamped_replay("fake", direction, 0, start=start,
                                count=count, **geom)
    # the ring does not divide the region, so the two directions count
    # differently: that the two moduli are not mixed up is the point
    other = stamped_script(
        "read" if direction == "write" else "write",
        geom["msgs_per_region"], geom["inflight"], start, count)[1]
    assert sum(hits) != sum(other)


def test_scripts_exercise_the_ring():
    """The generator's scripts are not vacuous: over the seeds the tests
    use, rings retire because they are full, scalar and vectorized posts
    meet in one batch, flushes find the ring empty, and in the icrc mode
    stamps and corruptions occur."""
    seen = set()
    for mode in MODES:
        for direction in DIRECTIONS:
            for seed in range(2):
                script = make_script(seed, mode, direction, **GEOM_A)
                assert 40 <= len(script) <= 60
                pending, kinds = 0, set()
                for op in script:
                    seen.add(op[0])
                    if op[0] == "flush":
                        if not pending:
                            seen.add("empty flush")
                        pending, kinds = 0, set()
                    if op[0] not in ("post", "post_many"):
                        continue
                    n = 1 if op[0] == "post" else op[2]
                    for _ in range(n):
                        if pending == GEOM_A["inflight"]:
                            seen.add("refill")
                            pending, kinds = 0, set()
                        pending += 1
                        kinds.add(op[0])
                        if len(kinds) == 2:
                            seen.add("mixed batch")
                    if n % GEOM_A["inflight"]:
                        seen.add("count does not divide")
    assert seen >= {"post", "post_many", "flush", "empty flush", "stamp",
                    "corrupt_sender", "refill", "mixed batch",
                    "count does not divide"}


def test_model_asserts_the_destination_rule():
    m = RingModel(64, 11, 4, "write")
    m.post(0, [(0, 64)])
    with pytest.raises(AssertionError, match="twice"):
        m.post(11, [(0, 64)])
    m = RingModel(64, 11, 4, "read")
    for i in range(4):
        m.post(i, [(0, 64)])
    m.post(4, [(0, 64)])  # slot 0 again, but the full ring retired first
    with pytest.raises(AssertionError, match="twice"):
        m.post(8, [(0, 64)])
    with pytest.raises(AssertionError):
        m.corrupt_sender(0)  # a post is pending


def test_stream_index_is_by_destination():
    """The stream engine's stream: by destination, so that two copies
    into one destination share a stream; and for bench's default (2
    streams, 8 slots, an even message count) still i % 2, so its timing
    is what it was."""
    pytest.importorskip("torch")
    from rocnrdma_amd.transport.sdma import stream_index

    for direction in DIRECTIONS:
        for n_msgs in (16, 256, 1 << 20):
            assert all(stream_index(i, 8, n_msgs, direction, 2) == i % 2
                       for i in range(5000))
        for streams in (2, 3):
            by_dest = {}
            for i in range(5000):
                d = i % 4 if direction == "read" else i % 11
                s = stream_index(i, 4, 11, direction, streams)
                assert by_dest.setdefault(d, s) == s and 0 <= s < streams


@given(st.sampled_from(["plain", "bytes", "sg"]), st.sampled_from(DIRECTIONS),
       st.integers(0, 2**32 - 1), st.sampled_from([64, 4112, 8192]),
       st.integers(1, 13), st.integers(1, 9))
@settings(max_examples=60, deadline=None,
          suppress_health_check=[HealthCheck.too_slow])
def test_fake_ring_replay_any_geometry(mode, direction, seed, msg, n_msgs,
                                       inflight):
    check_ring_replay("fake", mode, direction, seed, msg_bytes=msg,
                      msgs_per_region=n_msgs, inflight=inflight)
