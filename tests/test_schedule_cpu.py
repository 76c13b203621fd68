"""The host-side pieces of the segment schedule (vla_adapter_amd/schedule.py) that need no GPU."""
from vla_adapter_amd.schedule import Segment, chunks


def test_chunks_cover_the_layers_with_the_given_sizes():
    assert chunks(24, [4] * 5 + [2, 1, 1]) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 22), (22, 23), (23, 24)]
    assert chunks(5, [1]) == [(i, i + 1) for i in range(5)]
    assert chunks(10, [4]) == [(0, 4), (4, 8), (8, 10)]                 # the last size repeats and is clipped
    assert chunks(3, [1, 2, 4, 7]) == [(0, 1), (1, 3)]
    assert chunks(0, [4]) == []


def test_segment_is_positional():
    """tools/*_timeline.py read seg[2] (wait), seg[3] (signal) and seg[4] (ranges)."""
    fn = object()
    sg = Segment("H", fn, ("f", 0))
    assert tuple(sg) == ("H", fn, ("f", 0), None, None)
    assert (sg[0], sg[1], sg[2], sg[3], sg[4]) == (sg.stream, sg.fn, sg.wait, sg.signal, sg.ranges)
