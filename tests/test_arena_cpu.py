"""The arena helper's own tests, on CPU tensors (tests/arena.py)."""
import pytest
import torch

from tests.arena import MIN_MARGIN, Arena, assert_bits_equal

BF = torch.bfloat16

# (name, shape, strides): a 2-D window, a batched one whose batch stride is no multiple of the row stride, a row-group window
VIEWS = [
    ("2d", (5, 24), (40, 1)),
    ("batched", (3, 5, 24), (5 * 40 + 8, 40, 1)),
    ("row_group", (2, 4, 16), (9 * 24, 24, 1)),        # [B, row0:, D]: 4 live rows of 9 per sequence
]
IDS = [v[0] for v in VIEWS]


def overrun(a: Arena, shape, strides, first=0):
    """What a kernel with a wrong extent does: a view of the same arena from element `first` (may be negative) with another shape."""
    es = a.esize
    start = a.offset + first * es
    span = (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * es
    return a.buf[start:start + span].view(a.dtype).as_strided(shape, strides)


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
@pytest.mark.parametrize("dtype,align", [(BF, 2), (BF, 16), (torch.float32, 4), (torch.uint8, 1), (torch.uint8, 16)])
def test_view_geometry_and_margin(name, shape, strides, dtype, align):
    a = Arena(shape, dtype, strides=strides, align=align)
    assert tuple(a.view.shape) == shape and tuple(a.view.stride()) == strides and a.view.dtype == dtype
    p = a.view.data_ptr()
    assert p % align == 0 and p % (2 * align) != 0, "first element at exactly the requested alignment"
    before, after = a.margins()
    assert a.span_bytes == (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * a.esize
    assert before >= max(MIN_MARGIN, a.span_bytes) and after >= max(MIN_MARGIN, a.span_bytes)
    assert p - a.buf.data_ptr() == before and before + a.span_bytes + after == a.buf.numel()


def test_margin_grows_with_the_view():
    a = Arena((3, 1 << 20), torch.uint8, strides=((1 << 20) + 16, 1))          # spans 3 MiB
    assert a.span_bytes > 3 * MIN_MARGIN - 64 and min(a.margins()) >= a.span_bytes


def test_poison_values():
    for dt in (BF, torch.float32):
        a = Arena((2, 8), dt, strides=(16, 1), data=torch.ones(2, 8, dtype=dt))
        everything = a.buf.view(dt)
        assert int(torch.isnan(everything).sum()) == everything.numel() - 16, "everything but the declared elements is NaN"
        assert torch.isnan(overrun(a, (2, 16), (16, 1))[:, 8:]).all(), "the stride gap is poisoned"
    a = Arena((4,), torch.uint8)
    assert (a.buf == 0x7F).all()
    a = Arena((4,), torch.uint8, poison=1, data=torch.zeros(4, dtype=torch.uint8))       # a mask case that uses 0
    assert int((a.buf == 1).sum()) == a.buf.numel() - 4
    a = Arena((4,), torch.int64, poison=7)
    assert (a.buf.view(torch.int64) == 7).all()
    with pytest.raises(ValueError):
        Arena((4,), torch.int32)                        # integer poison is the case's choice


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
def test_writes_inside_the_extent_are_not_flagged(name, shape, strides):
    a = Arena(shape, BF, strides=strides, align=16, data=torch.zeros(shape, dtype=BF))
    a.assert_outside_intact()
    a.assert_unchanged()
    a.view.copy_(torch.randn(shape).to(BF))             # every declared element, first and last of every row included
    a.view[..., -1] = float("nan")
    a.assert_outside_intact()
    with pytest.raises(AssertionError, match="input arena was written"):
        a.assert_unchanged()


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
def test_flags_one_element_past_a_rows_end(name, shape, strides):
    a = Arena(shape, BF, strides=strides, data=torch.zeros(shape, dtype=BF))
    wide = overrun(a, shape[:-1] + (shape[-1] + 1,), strides)
    idx = tuple(n // 2 for n in shape[:-1]) + (shape[-1],)
    wide[idx] = 1.0
    with pytest.raises(AssertionError, match="stride gap"):
        a.assert_outside_intact()


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
def test_flags_one_element_in_the_stride_gap(name, shape, strides):
    a = Arena(shape, BF, strides=strides, data=torch.zeros(shape, dtype=BF))
    wide = overrun(a, shape[:-1] + (strides[-2],), strides)
    idx = tuple(0 for _ in shape[:-1]) + (strides[-2] - 1,)       # the last gap element of the first row
    wide[idx] = 1.0
    with pytest.raises(AssertionError, match="stride gap"):
        a.assert_outside_intact()


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
def test_flags_one_row_past_the_last(name, shape, strides):
    a = Arena(shape, BF, strides=strides, data=torch.zeros(shape, dtype=BF))
    tall = overrun(a, shape[:-2] + (shape[-2] + 1, shape[-1]), strides)
    tall[..., shape[-2], :] = 1.0                       # row `rows` of every batch / group: between the groups, and past the last
    with pytest.raises(AssertionError, match="PAST the last element"):
        a.assert_outside_intact()
    if len(shape) == 3:                                 # the same row of the FIRST group alone lies between two groups
        b = Arena(shape, BF, strides=strides, data=torch.zeros(shape, dtype=BF))
        overrun(b, shape[:-2] + (shape[-2] + 1, shape[-1]), strides)[0, shape[-2], :] = 1.0
        with pytest.raises(AssertionError, match="stride gap"):
            b.assert_outside_intact()


@pytest.mark.parametrize("name,shape,strides", VIEWS, ids=IDS)
def test_flags_one_element_before_the_first(name, shape, strides):
    a = Arena(shape, BF, strides=strides, data=torch.zeros(shape, dtype=BF))
    overrun(a, (1,), (1,), first=-1)[0] = 1.0
    with pytest.raises(AssertionError, match="2 bytes BEFORE the first element"):
        a.assert_outside_intact()


def test_checks_compare_bits_not_values():
    a = Arena((2, 8), torch.float32, strides=(12, 1), data=torch.zeros(2, 8))
    gap = overrun(a, (2, 12), (12, 1))
    gap[0, 9] = float("nan")                            # the same NaN the poison is: same bits, not a write the checker can see
    a.assert_outside_intact()
    gap.view(torch.int32)[0, 9] = 0x7FC00001            # another NaN payload: float comparison could not tell, the bits do
    with pytest.raises(AssertionError):
        a.assert_outside_intact()
    x = torch.tensor([0.0, float("nan")])
    assert_bits_equal(x, x.clone())
    with pytest.raises(AssertionError):
        assert_bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


def test_set_records_a_new_state():
    a = Arena((3, 8), BF, strides=(16, 1))
    a.view.fill_(1.0)
    with pytest.raises(AssertionError):
        a.assert_unchanged()
    a.set(torch.full((3, 8), 2.0, dtype=BF))
    a.assert_unchanged()
    assert a.ptr(1, 2) == a.view.data_ptr() + (16 + 2) * 2
