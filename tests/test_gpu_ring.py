"""GPU tests: the sdma transport's WQE ring against the model of
tests/test_ring.py — `_pending`, the column of a post, the refill inside
post(), post_many() and post_many_sg(), the per-mode rows — over a ring
that divides neither the region nor the counts posted, with scalar and
vectorized posts mixed, in every mode and both directions; bench's step
shape (one post_many over a ring much smaller than the region); stamped
icrc where the write-side and read-side counts differ; and the stream
engine, whose copies into one destination must keep post order.

Safety rule of this module: the scripts pass the transports' own
validation (_lens, _sges) and the protected mode's keys are all valid,
so every address handed to the GPU lies inside the region or the staging
area the transport owns.  Fixed seeds; every comparison is exact."""
import pytest

torch = pytest.importorskip("torch")

from tests.test_ring import (B_COUNT, B_START, DIRECTIONS, GEOM_A,  # noqa: E402
                             GEOM_B, MODES, check_ring_replay,
                             check_stamped_replay)

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("mode", list(MODES))
def test_sdma_ring_replay(mode, direction, seed):
    check_ring_replay("sdma", mode, direction, seed, engine="kernel",
                      **GEOM_A)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_sdma_ring_replay_bench_shape(direction):
    script = [("post_many", B_START, B_COUNT, None), ("flush",)]
    m = check_ring_replay("sdma", "plain", direction, 0, script=script,
                          engine="kernel", **GEOM_B)
    assert m.retired == 17  # 16 refills inside the call, then the flush


@pytest.mark.parametrize("geom", [GEOM_A, GEOM_B], ids=["A", "B"])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_sdma_stamped_icrc(direction, geom):
    start, count = ((B_START, B_COUNT) if geom is GEOM_B
                    else (7, 3 * geom["msgs_per_region"] + 5))
    check_stamped_replay("sdma", direction, 0, start=start, count=count,
                         engine="kernel", **geom)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("num_streams", [3, 2])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_sdma_stream_engine_keeps_order_per_destination(direction,
                                                        num_streams, seed):
    """The stream engine has no ring; its scripts repeat destinations
    without a flush in between, and the last post must win: copies into
    one destination share a stream (sdma.stream_index).  With 3 streams
    over 4 slots or 11 region messages, i % 3 would put them on
    different streams, unordered — a race, which need not show on every
    run."""
    check_ring_replay("sdma", "plain", direction, seed, ordered=True,
                      engine="stream", num_streams=num_streams, **GEOM_A)
