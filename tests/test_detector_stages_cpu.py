"""The two host-side decisions of ``StreamDetector.step`` and the subscript view of ``_FrameContext``,
without a device and without loading the library: when may a frame be uploaded ahead, and when may an uploaded frame be
trusted.  The second rule has been wrong before (an edited tensor, a new tensor at a recycled address)."""
import numpy as np
import pytest
import torch

from centertrack_amd import _lib
from centertrack_amd.detector import _FrameContext, _frame_source, _prefetchable

SHAPE = (1, 3, 2, 2)
# every name bench.py, tools/determinism.py, tools/tie_report.py and the GPU tests read by subscript
READ_FROM_OUTSIDE = ('plan', 'decoder', 'graph', 'partial', 'merged', 'host_rows', 'loop', 'launched', 'loop_stream', 'args',
                     'counts', 'frames', 'slot', 'nslots', 'raw')
CALLED_FROM_OUTSIDE = ('device_frame', 'pre_stage')      # (methods: read by subscript and called, never in __slots__)


def frame():
    return torch.arange(12, dtype=torch.float32).reshape(SHAPE)


def strided():
    t = torch.zeros((1, 3, 2, 4))[..., 1:3]
    assert tuple(t.shape) == SHAPE and not t.is_contiguous()
    return t


def test_prefetchable_takes_a_contiguous_float32_host_tensor_of_the_frames_shape():
    assert _prefetchable(frame(), SHAPE) is True
    assert _prefetchable(frame(), torch.Size(SHAPE)) is True          # (the native path passes ``images.shape``)


@pytest.mark.parametrize('what,bad', [('none', None), ('numpy', np.zeros(SHAPE, np.float32)),
                                      ('float64', torch.zeros(SHAPE, dtype=torch.float64)), ('strided', strided()),
                                      ('shape', torch.zeros((1, 3, 2, 3))), ('batch', torch.zeros((2, 3, 2, 2)))])
def test_prefetchable_refuses(what, bad):
    assert not _prefetchable(bad, SHAPE)


def test_frame_source_trusts_an_upload_of_this_object_at_this_version_into_this_slot_only():
    t = frame()
    assert _frame_source(t, (t, t._version, 1), 1) == _lib.CT_FRAME_UPLOADED
    assert _frame_source(t, None, 1) == _lib.CT_FRAME_HOST
    assert _frame_source(t, (t, t._version, 2), 1) == _lib.CT_FRAME_HOST         # the right tensor, recorded for another slot
    other = t.clone()
    assert torch.equal(other, t)
    assert _frame_source(other, (t, t._version, 1), 1) == _lib.CT_FRAME_HOST     # an equal-valued other tensor
    record = (t, t._version, 1)
    t.add_(0)                                                                    # same values, edited in place since
    assert t._version != record[1]
    assert _frame_source(t, record, 1) == _lib.CT_FRAME_HOST


@pytest.mark.parametrize('images', [strided(), frame().double(), frame().to(torch.uint8)])
def test_frame_source_copies_in_place_what_is_no_contiguous_float32_tensor(images):
    t = frame()
    assert _frame_source(images, None, 0) == _lib.CT_FRAME_IN_PLACE
    assert _frame_source(images, (t, t._version, 0), 0) == _lib.CT_FRAME_IN_PLACE     # an upload record exists: of another frame


def test_the_four_frame_kinds_are_distinct():
    assert len({_lib.CT_FRAME_UPLOADED, _lib.CT_FRAME_HOST, _lib.CT_FRAME_DEVICE, _lib.CT_FRAME_IN_PLACE}) == 4


def test_context_declares_every_field_read_from_outside():
    assert not set(READ_FROM_OUTSIDE) - set(_FrameContext.__slots__)
    assert len(set(_FrameContext.__slots__)) == len(_FrameContext.__slots__)
    for name in CALLED_FROM_OUTSIDE:
        assert callable(getattr(_FrameContext, name)) and name not in _FrameContext.__slots__


def test_context_subscript_and_get_return_the_attributes():
    ctx = _FrameContext.__new__(_FrameContext)            # (the real constructor needs a device)
    assert not hasattr(ctx, '__dict__')
    with pytest.raises(AttributeError):                   # no field can be added later
        ctx.not_a_field = 1
    marks = {name: object() for name in READ_FROM_OUTSIDE}
    for name, mark in marks.items():
        setattr(ctx, name, mark)
    for name, mark in marks.items():
        assert ctx[name] is mark and ctx.get(name) is mark and ctx.get(name, 7) is mark
    ctx.partial = None
    assert ctx['partial'] is None and ctx.get('partial') is None and ctx.get('partial', 7) is None
    for name in CALLED_FROM_OUTSIDE:
        assert ctx[name] == getattr(ctx, name) and ctx.get(name) == getattr(ctx, name)      # the bound method
    for name in ('not_a_field', 'close', '__slots__'):
        with pytest.raises(KeyError):
            ctx[name]
        assert ctx.get(name) is None and ctx.get(name, 7) == 7
