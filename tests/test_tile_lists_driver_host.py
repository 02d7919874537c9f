"""CPU: the host protocol between a view's tile lists and its compositing (rasterizer/rasterize.py: the `TileLists`
record, `_finish_for` -- the second half of every device-sized list build -- and `composite_lists`, the forward
driver both rasterize ops share).  Pure Python: the compositing callables and the pinned count are fakes that log their
calls, the lists are strings, and `build_tile_lists` is replaced by a function that returns what the case needs."""
import pytest
import torch

from rasterizer import rasterize as R

XYS = torch.zeros(4, 2)   # (the driver only reads its device, for the tile flags of a two-round walk)
H, W = 40, 70             # 3 x 5 tiles of 16 px
TWO = ("two", "bins2", 1024)
DET = ("order", "cum_sorted", "slots")


class Pending:
    def __init__(self, count):
        self.count, self.reads = count, 0

    def resolve(self):
        self.reads += 1
        return self.count


class Calls:
    """composite / round1 / round2 of a caller: every call is logged, outputs name the lists they came from."""

    def __init__(self):
        self.log = []

    def composite(self, ids, bins):
        self.log.append(("composite", ids, bins))
        return ("walked", ids, bins)

    def round1(self, ids, bins1, flags):
        self.log.append(("round1", ids, bins1, flags.clone()))
        flags += 1  # (as the kernel marks finished tiles)

    def round2(self, ids, aux):
        self.log.append(("round2", ids, aux))
        return ("two rounds", ids, aux)

    @property
    def names(self):
        return [c[0] for c in self.log]


def drive(monkeypatch, build, calls, fuse=None, rounds=True):
    seen = {}

    def fake_build(xys, depths, radii, conics, num_tiles_hit, opacity, img_height, img_width, block_width, round1=None,
                   fuse=None):
        seen.update(round1=round1, fuse=fuse, size=(img_height, img_width, block_width))
        return build(round1)

    monkeypatch.setattr(R, "build_tile_lists", fake_build)
    out = R.composite_lists(XYS, None, None, None, None, None, H, W, 16, calls.composite,
                            calls.round1 if rounds else None, calls.round2 if rounds else None, fuse)
    assert seen["size"] == (H, W, 16) and seen["fuse"] is fuse and (seen["round1"] is None) == (not rounds)
    return out


def device_sized(count, capacity, lists, rebuilt=None, on_overflow=None):
    """-> (finish, log): `_finish_for` over fakes; `log` records note / remember / rebuild / on_overflow."""
    log = []
    pending = Pending(count)

    def rebuild(n):
        log.append(("rebuild", n))
        return rebuilt

    def overflowed():
        log.append(("on_overflow",))
        on_overflow()

    finish = R._finish_for(pending, capacity, lists, rebuild, overflowed if on_overflow else None,
                           note=lambda n: log.append(("note", n)), remember=lambda rec: log.append(("remember", rec)))
    return finish, log


def test_the_record_keeps_its_field_order_and_knows_two_segment_lists():
    rec = R.TileLists(7, "ids", "bins", TWO)
    assert tuple(rec) == (7, "ids", "bins", TWO) and rec[0] == 7 and rec[2] == "bins" and rec[3][0] == "two"
    assert rec.two and not R.TileLists(7, "ids", "bins").two and not R.TileLists(7, "ids", "bins", DET).two
    assert R.TileLists(7, "ids", "bins").aux is None
    assert not hasattr(R, "last_list_aux") and not hasattr(R, "_tls")


def test_count_known_is_a_single_walk(monkeypatch):
    calls = Calls()
    lists = R.TileLists(500, "ids", "bins", None)
    got, outputs = drive(monkeypatch, lambda round1: (lists, None), calls)
    assert got is lists and outputs == ("walked", "ids", "bins") and calls.names == ["composite"]


def test_device_sized_lists_that_fit_are_walked_once_and_remembered(monkeypatch):
    calls = Calls()
    lists = R.TileLists(None, "ids", "bins", DET)
    finish, log = device_sized(900, 1000, lists)
    before = dict(R.counters)
    got, outputs = drive(monkeypatch, lambda round1: (lists, finish), calls)
    assert got == R.TileLists(900, "ids", "bins", DET) and outputs == ("walked", "ids", "bins")
    assert calls.names == ["composite"]
    assert log == [("note", 900), ("remember", got)] and R.counters == before
    finish, log = device_sized(1000, 1000, lists)  # exactly full is not an overflow
    assert finish() == (R.TileLists(1000, "ids", "bins", DET), False) and [e[0] for e in log] == ["note", "remember"]


def test_device_sized_lists_that_overflow_are_built_again_and_walked_again(monkeypatch):
    calls = Calls()
    lists = R.TileLists(None, "ids0", "bins0", None)
    again = R.TileLists(1500, "ids1", "bins1", DET)
    ran = []
    finish, log = device_sized(1500, 1000, lists, rebuilt=again, on_overflow=lambda: ran.append(True))
    before = dict(R.counters)
    got, outputs = drive(monkeypatch, lambda round1: (lists, finish), calls)
    assert got is again and got.aux == DET and outputs == ("walked", "ids1", "bins1")
    assert calls.log == [("composite", "ids0", "bins0"), ("composite", "ids1", "bins1")]
    assert log == [("note", 1500), ("on_overflow",), ("rebuild", 1500)] and ran == [True]  # (`rebuild` remembers its own)
    changed = {k: R.counters[k] - before[k] for k in before if R.counters[k] != before[k]}
    assert changed == {"list_rebuilds": 1}


def test_overflow_of_the_one_call_build_drops_its_outputs(monkeypatch):
    """`fuse.outputs` of lists that were cut short must not survive: the overflow hook clears them, the driver walks
    the rebuilt lists."""
    calls = Calls()
    fuse = R.FusedForward(None, None, H, W, False, None)
    lists = R.TileLists(None, "ids0", "bins0", None)
    again = R.TileLists(1500, "ids1", "bins1", None)
    finish, _ = device_sized(1500, 1000, lists, rebuilt=again, on_overflow=lambda: setattr(fuse, "outputs", None))

    def build(round1):
        fuse.outputs = ("composited by the build",)
        return lists, finish

    got, outputs = drive(monkeypatch, build, calls, fuse=fuse)
    assert got is again and outputs == ("walked", "ids1", "bins1") and fuse.outputs is None
    assert calls.log == [("composite", "ids1", "bins1")]


def test_outputs_of_the_list_building_call_are_not_composited_again(monkeypatch):
    calls = Calls()
    fuse = R.FusedForward(None, None, H, W, False, None)
    lists = R.TileLists(None, "ids", "bins", None)
    finish, log = device_sized(900, 1000, lists)

    def build(round1):
        fuse.outputs = ("composited by the build",)
        return lists, finish

    got, outputs = drive(monkeypatch, build, calls, fuse=fuse)
    assert outputs == ("composited by the build",) and calls.log == [] and got.num_intersects == 900
    assert log[-1] == ("remember", got)


def test_two_round_lists_whose_first_round_ran_in_the_build_take_round_two_only(monkeypatch):
    calls = Calls()
    lists = R.TileLists(None, "ids", "bins1", TWO)
    done = lists._replace(num_intersects=800)

    def build(round1):
        round1("ids", "bins1", torch.zeros(15, dtype=torch.int32))
        return lists, lambda: (done, False)

    got, outputs = drive(monkeypatch, build, calls)
    assert got is done and outputs == ("two rounds", "ids", TWO) and calls.names == ["round1", "round2"]


@pytest.mark.parametrize("speculative", [False, True])
def test_two_round_lists_from_the_cache_take_both_rounds_with_fresh_flags(monkeypatch, speculative):
    calls = Calls()
    cached = R.TileLists(800, "ids", "bins1", TWO)
    if speculative:  # (the cache's "verify" route: walked first, the inputs' equality checked behind the walk)
        build = lambda round1: (cached._replace(num_intersects=None), lambda: (cached, False))
    else:
        build = lambda round1: (cached, None)
    for _ in range(2):  # (the second view's flags are its own: round 1 of the first has marked its tiles)
        got, outputs = drive(monkeypatch, build, calls)
        assert got is cached and outputs == ("two rounds", "ids", TWO)
    assert calls.names == ["round1", "round2"] * 2
    for call in (calls.log[0], calls.log[2]):
        flags = call[3]
        assert call[:3] == ("round1", "ids", "bins1")
        assert flags.dtype == torch.int32 and flags.shape == (15,) and not flags.any()


def test_an_empty_view_composites_nothing(monkeypatch):
    calls = Calls()
    empty = R.TileLists(0, None, None, None)
    assert drive(monkeypatch, lambda round1: (empty, None), calls) == (empty, None)
    lists = R.TileLists(None, "ids", "bins", None)  # device-sized: walked before the count says there was nothing
    finish, _ = device_sized(0, 1000, lists)
    got, outputs = drive(monkeypatch, lambda round1: (lists, finish), calls)
    assert got.num_intersects == 0 and outputs is None and calls.names == ["composite"]


def test_a_single_round_view_behind_a_two_round_view_has_no_aux(monkeypatch):
    """What travelled through per-thread state until the record carried it: the `aux` a view walks is the one its own
    lists came with, whatever the view before it left."""
    calls = Calls()
    deep = R.TileLists(800, "ids", "bins1", TWO)
    got, _ = drive(monkeypatch, lambda round1: (deep, None), calls)
    assert got.two
    shallow = R.TileLists(None, "ids_s", "bins_s", None)
    finish, _ = device_sized(90, 1000, shallow)
    got, outputs = drive(monkeypatch, lambda round1: (shallow, finish), calls)
    assert got.aux is None and not got.two and outputs == ("walked", "ids_s", "bins_s")
    assert calls.names == ["round1", "round2", "composite"]
    got, outputs = drive(monkeypatch, lambda round1: (shallow._replace(num_intersects=90), None), calls, rounds=False)
    assert got.aux is None and calls.names[-1] == "composite"
