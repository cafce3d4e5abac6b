"""
Strahler order, Shreve magnitude and stream links on the MI355X (``StreamOrder``,
``DemToStreamOrder``, ``hdem_streamorder_u8[_dev]``): every result bit for bit against the
per-cell references of tests/test_streamorder.py and through the local equations, on random
acyclic codes with the three forms of the stream set, on constructed networks with known
answers (a binary tree across tile seams, a comb of 300 junctions, a star, donor triples),
the links as pour points of ``Watersheds``, the chain from a DEM, and the refusals, each an
ordinary error return in bounded time.
"""
import ctypes

import numpy as np
import pytest

import hdem_synth
import hydrodem_amd as hd
from hydrodem_amd import backend, streamorder
from test_flowacc import acc_kahn, random_acyclic_codes
from test_streamorder import (E, N, S, W_, binary_tree, comb, link_ends, link_stops,
                              order_holds, order_kahn, star, stream_donors, stream_of, triple)

pytestmark = pytest.mark.gpu

ALL = ("order", "magnitude", "link")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    yield


def run(codes, streams=None, threshold=None, want=ALL):
    outs, stats = streamorder.streamorder(np.ascontiguousarray(codes, dtype=np.uint8), streams,
                                          threshold, want)
    assert set(outs) == set(want)
    for name in want:
        assert outs[name].dtype == (np.uint8 if name == "order" else np.uint32)
    return outs, stats


def check(codes, outs, stats, stream):
    """Bit for bit against the per-cell peel, through the local equations, and the counters."""
    order, mag = order_kahn(codes, stream)
    assert np.array_equal(outs["order"], order)
    assert np.array_equal(outs["magnitude"], mag)
    assert np.array_equal(outs["link"], link_ends(codes, stream))
    assert order_holds(codes, stream, outs["order"], outs["magnitude"], outs["link"])
    nin = stream_donors(codes, stream)
    assert stats["stream_cells"] == int(stream.sum())
    assert stats["heads"] == int((stream & (nin == 0)).sum())
    assert stats["junctions"] == int((stream & (nin >= 2)).sum())
    assert stats["links"] == int(link_stops(codes, stream).sum())
    assert stats["max_order"] == int(order.max())
    assert stats["tile_h"] == 64 and stats["tile_w"] == 64


# ---------------------------------------------------------------------------
# random acyclic codes, the three forms of the stream set
# ---------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 130), (130, 1), (64, 64), (65, 63), (70, 90), (129, 200), (257, 130)]


@pytest.fixture(scope="module")
def cases():
    """Codes and their accumulation per (shape, ramp), made once."""
    made = {}

    def get(shape, ramp):
        if (shape, ramp) not in made:
            codes = random_acyclic_codes(*shape, seed=shape[0] * 1000 + shape[1], ramp=ramp)
            made[shape, ramp] = codes, acc_kahn(codes).astype(np.uint32)
        return made[shape, ramp]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ramp", [False, True], ids=["flat", "ramp"])
@pytest.mark.parametrize("kind", ["all", "acc", "mask"])
def test_random_acyclic_codes_match_the_per_cell_peel(cases, shape, ramp, kind):
    codes, acc = cases(shape, ramp)
    if kind == "all":
        streams, threshold = None, None
    elif kind == "acc":
        streams, threshold = acc, 4
    else:
        # 60 % of the cells: stream cells drain into others, and links restart below them
        streams, threshold = np.random.default_rng(shape[1]).random(shape) < 0.6, None
    outs, stats = run(codes, streams, threshold)
    check(codes, outs, stats, stream_of(codes, streams, threshold))


def test_the_forms_of_a_stream_set_host_and_device_and_two_runs_are_identical(cases):
    codes, acc = cases((257, 130), True)
    stream = acc >= 4
    a, _ = run(codes, acc, 4)
    for streams in (stream, stream.astype(np.uint8) * 7):
        b, _ = run(codes, streams)
        assert all(a[k].tobytes() == b[k].tobytes() for k in ALL)
    c, _ = run(codes, acc, 4)
    assert all(a[k].tobytes() == c[k].tobytes() for k in ALL)
    f = hd.StreamOrder(acc, threshold=4, keep_partial_results=True)
    assert np.array_equal(f.apply(codes), a["order"]) and f.order.dtype == np.uint8
    assert np.array_equal(f.magnitude, a["magnitude"]) and np.array_equal(f.links, a["link"])
    g = hd.StreamOrder(acc, threshold=4, method="shreve")
    got = g.apply(codes)
    assert got.dtype == np.uint32 and np.array_equal(got, a["magnitude"])
    assert g.order is None and g.magnitude is None and g.links is None
    with backend.DeviceRaster.from_host(codes, dtype=np.uint8) as dc, \
            backend.DeviceRaster.from_host(acc, dtype=np.uint32) as dacc:
        dev = hd.StreamOrder(dacc, threshold=4, keep_partial_results=True)
        out = dev.apply_device(dc)
        with dev.order, dev.magnitude, dev.links:
            assert out is dev.order and backend.is_device_raster(dev.links)
            assert dev.order.dtype == np.uint8 and dev.links.dtype == np.uint32
            assert all(a[k].tobytes() == r.to_host().tobytes()
                       for k, r in zip(ALL, (dev.order, dev.magnitude, dev.links)))
        # one output at a time, a host mask for device codes
        for method, key in (("strahler", "order"), ("shreve", "magnitude")):
            h = hd.StreamOrder(stream, method=method)
            with h.apply_device(dc) as out:
                assert np.array_equal(out.to_host(), a[key]) and h.links is None
        links, _ = streamorder.streamorder_dev(dc, dacc, 4, "link")
        with links["link"] as raster:
            assert np.array_equal(raster.to_host(), a["link"])


# ---------------------------------------------------------------------------
# constructed networks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("every_cell", [False, True], ids=["mask", "every_cell"])
def test_a_perfect_binary_tree_across_tile_seams(every_cell):
    codes, mask, root = binary_tree()
    assert codes.shape == (160, 256) and root == (93, 103)
    outs, stats = run(codes, None if every_cell else mask)
    stream = np.ones(codes.shape, bool) if every_cell else mask
    check(codes, outs, stats, stream)
    assert (outs["order"][root], outs["magnitude"][root]) == (7, 64)
    assert [int(((outs["order"] == k) & mask).sum()) for k in range(1, 8)] == [64] * 6 + [1]
    assert np.unique(outs["link"][mask]).size == 127
    assert stats["max_order"] == 7 and stats["max_hops"] == 6
    if not every_cell:
        assert (stats["links"], stats["heads"], stats["junctions"]) == (127, 64, 63)
        assert not outs["order"][~mask].any() and not outs["link"][~mask].any()
    else:
        assert (outs["order"][~mask] == 1).all() and stats["junctions"] == 63


def test_a_comb_of_three_hundred_junctions():
    codes = comb()
    outs, stats = run(codes)
    check(codes, outs, stats, np.ones(codes.shape, bool))
    assert (outs["order"][1] == 2).all() and (outs["order"][[0, 2]] == 1).all()
    assert outs["magnitude"][1, 299] == 600
    assert stats["links"] == 900 and stats["junctions"] == 300 and stats["heads"] == 600
    assert 1 <= stats["max_hops"] <= 300                 # a chain of 300 hops across five tiles


def test_a_star_and_the_donor_triples():
    codes = star()
    outs, stats = run(codes)
    check(codes, outs, stats, np.ones((3, 3), bool))
    assert (outs["order"][1, 1], outs["magnitude"][1, 1]) == (2, 8)
    for third in (2, 3):
        codes, at = triple(third)
        for streams in (None, codes != 0):
            stream = stream_of(codes, streams)
            if streams is not None:
                stream[at] = streams[at] = True
            outs, stats = run(codes, streams)
            check(codes, outs, stats, stream)
            assert outs["order"][at] == 3


# ---------------------------------------------------------------------------
# links
# ---------------------------------------------------------------------------
def test_links_are_pour_points_that_give_one_catchment_per_link(cases):
    codes, acc = cases((129, 200), True)
    stream = acc >= 4
    outs, _ = run(codes, acc, 4)
    link, stops = outs["link"], link_stops(codes, stream)
    flat = np.arange(codes.size).reshape(codes.shape)
    # 1 + the flat index of the link's last cell, constant along the link, and it changes
    # exactly where a link ends
    assert np.array_equal(link[stops], flat[stops] + 1)
    assert (link[stream] > 0).all() and stops.ravel()[link[stream] - 1].all()
    from test_flowacc import receivers
    rec = receivers(codes).reshape(codes.shape)
    inner = stream & ~stops
    assert np.array_equal(link[inner], link.ravel()[rec[inner]])
    below = stops & (rec >= 0)
    assert (link[below] != link.ravel()[rec[below]]).all()
    # the ids at the link ends go straight in as a seeds raster
    labels = hd.Watersheds(pour_points=np.where(stops, link, 0)).apply(codes)
    assert np.array_equal(labels[stream], link[stream])


# ---------------------------------------------------------------------------
# terrain: the chain from a DEM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flats", ["keep", "resolve"])
def test_the_chain_from_a_dem_matches_the_peel_on_its_own_codes(flats):
    z = hdem_synth.synth_dem(512, 512)
    chain = hd.DemToStreamOrder(threshold=100, flats=flats, keep_partial_results=True)
    got = chain.apply(z)
    assert got is chain.order and got.dtype == np.uint8
    assert chain.codes.dtype == np.uint8 and chain.accumulation.dtype == np.uint32
    stream = chain.accumulation >= 100
    order, mag = order_kahn(chain.codes, stream)
    assert np.array_equal(got, order) and np.array_equal(chain.magnitude, mag)
    assert order_holds(chain.codes, stream, got, chain.magnitude, chain.links)
    st = chain.stats["StreamOrder"]
    assert st["max_order"] == int(order.max()) >= 3
    assert st["heads"] == int((stream & (stream_donors(chain.codes, stream) == 0)).sum()) > 10
    assert set(chain.stats) == {"SinkFill", "FlowAccumulation", "StreamOrder"} | \
        ({"ResolveFlats"} if flats == "resolve" else set())
    plain = hd.DemToStreamOrder(threshold=100, flats=flats, method="shreve")
    assert np.array_equal(plain.apply(z), mag) and plain.codes is None and plain.links is None
    with backend.DeviceRaster.from_host(z) as dz:
        with plain.apply_device(dz) as out:
            assert backend.is_device_raster(out) and np.array_equal(out.to_host(), mag)


def test_profiling_times_the_phases():
    ctx = backend.context()
    ctx.profile(True)
    try:
        f = hd.StreamOrder()
        f.apply(random_acyclic_codes(300, 300, seed=5, ramp=True))
    finally:
        ctx.profile(False)
    assert f.stats["ms_nodes"] > 0 and f.stats["ms_walk"] > 0 and f.stats["ms_gather"] > 0
    f.apply(np.full((3, 5), S, np.uint8))
    assert f.stats["ms_nodes"] == 0 and f.stats["max_order"] == 1


# ---------------------------------------------------------------------------
# refusals: each returns, and the context stays usable
# ---------------------------------------------------------------------------
def still_works():
    outs, _ = run(np.full((3, 5), S, np.uint8))
    assert (outs["order"] == 1).all() and np.array_equal(outs["magnitude"][:, 0], [1, 1, 1])
    assert np.array_equal(outs["link"][:, 2], [13, 13, 13])


def loop(shape=(70, 70), y=30, x=62):
    """A 4-cell loop that lies across a tile seam."""
    codes = np.zeros(shape, np.uint8)
    codes[y, x], codes[y, x + 1], codes[y + 1, x + 1], codes[y + 1, x] = E, S, W_, N
    return codes


def test_a_stream_loop_alone_is_refused():
    codes = loop()
    for streams in (codes != 0, None):
        with pytest.raises(ValueError, match="flow directions form a cycle"):
            run(codes, streams)
    still_works()


def test_a_stream_loop_with_a_tributary_is_refused():
    codes = loop()
    codes[30, 50:62] = E                                 # joins the loop at (30, 62)
    for streams in (codes != 0, None):
        with pytest.raises(ValueError, match="flow directions form a cycle: 1 stream junctions"):
            run(codes, streams)
    still_works()


def test_a_loop_off_the_streams_is_refused():
    codes = loop()
    codes[5, 5:20] = E
    streams = np.zeros(codes.shape, bool)
    streams[5, 5:20] = True
    with pytest.raises(ValueError, match="flow directions form a cycle"):
        run(codes, streams)
    still_works()


@pytest.mark.parametrize("bad", [3, 255])
def test_invalid_bytes_raise(bad):
    codes = np.full((50, 70), E, np.uint8)
    codes[20, 33] = bad
    with pytest.raises(ValueError, match="invalid D8 code in 1 cells"):
        run(codes)
    still_works()


def test_argument_combinations_are_refused_by_the_library():
    ctx = backend.context()
    lib = ctx.lib
    codes = np.full((4, 6), E, np.uint8)
    out = np.zeros((4, 6), np.uint8)
    st = backend._StreamOrderStats()                # pylint: disable=protected-access
    args = (ctx.handle, codes.ctypes.data, 4, 6)
    none = (None, backend.FT_STREAMS_NONE, 0)
    for fn in (lib.hdem_streamorder_u8, lib.hdem_streamorder_u8_dev):
        assert fn(*args, *none, None, None, None, 0, None) == backend.BAD_ARG
        assert b"no output wanted" in lib.hdem_last_error()
    assert lib.hdem_streamorder_u8(*args, *none, out.ctypes.data, None, None, 1, None) == \
        backend.BAD_ARG
    assert b"flags" in lib.hdem_last_error()
    for streams, kind, threshold, says in ((codes.ctypes.data, 0, 0, b"must be null"),
                                           (None, 1, 0, b"mask is null"),
                                           (codes.ctypes.data, 1, 2, b"no threshold"),
                                           (codes.ctypes.data, 2, 0, b"threshold >= 1"),
                                           (None, 7, 0, b"unknown stream kind")):
        assert lib.hdem_streamorder_u8(*args, streams, kind, threshold, out.ctypes.data, None,
                                       None, 0, None) == backend.BAD_ARG
        assert says in lib.hdem_last_error()
    st.struct_size = 3
    assert lib.hdem_streamorder_u8(*args, *none, out.ctypes.data, None, None, 0,
                                   ctypes.byref(st)) == backend.BAD_ARG
    assert b"hdem_streamorder_stats.struct_size is 3" in lib.hdem_last_error()
    # a shorter struct is filled as far as it goes
    st = backend._StreamOrderStats()                # pylint: disable=protected-access
    st.struct_size, st.max_hops = 40, -7
    assert lib.hdem_streamorder_u8(*args, *none, out.ctypes.data, None, None, 0,
                                   ctypes.byref(st)) == backend.OK
    assert st.struct_size == 40 and st.heads == 4 and st.links == 4 and st.max_hops == -7
    assert (out == 1).all()
    still_works()


def test_more_than_2_to_the_32_cells_is_rejected_before_any_allocation():
    ctx = backend.context()
    fake = ctypes.c_void_p(256)          # never dereferenced: the size check comes first
    for fn in (ctx.lib.hdem_streamorder_u8_dev, ctx.lib.hdem_streamorder_u8):
        rc = fn(ctx.handle, fake, 65536, 65536, None, 0, 0, fake, fake, fake, 0, None)
        assert rc == backend.BAD_ARG
        assert b"2^32" in ctx.lib.hdem_last_error()
    still_works()
