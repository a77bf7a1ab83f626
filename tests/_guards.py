"""Caller buffers of the forward GPU tests (tests/test_hip_conv_forward.py, tests/test_hip_dcn_forward.py): an input is read from
a channel slice of a NaN-filled wider NHWC buffer, an output is written into a NaN-filled slice between guard channels; ``take``
checks that the guards still stand and that every element of the slice was written."""
import torch

NAN, GUARD = float('nan'), 7.0


def slice_of(t_nchw, device, c0=4, tail=4):
    """``t`` as the channel slice [c0, c0 + C) of a wider NHWC buffer whose other channels are NaN"""
    from centertrack_amd import ops
    N, Cc, H, W = t_nchw.shape
    buf = torch.full((N, H, W, c0 + (Cc + 3) // 4 * 4 + tail), NAN)
    buf[..., c0:c0 + Cc] = t_nchw.permute(0, 2, 3, 1)
    return ops.View(buf.to(device), c0, Cc)


def guarded(N, H, W, Cc, device, c0=4, tail=4):
    """a NaN-filled output slice between guard channels of 7.0"""
    from centertrack_amd import ops
    buf = torch.full((N, H, W, c0 + (Cc + 3) // 4 * 4 + tail), GUARD)
    buf[..., c0:c0 + Cc] = NAN
    return ops.View(buf.to(device), c0, Cc)


def guards_intact(v):
    buf = v.buf.cpu()
    return bool((buf[..., :v.c0] == GUARD).all()) and bool((buf[..., v.c0 + v.C:] == GUARD).all())


def take(v, what):
    """the slice as NCHW on the CPU, after checking that the guards still hold 7.0 and no NaN is left inside"""
    assert guards_intact(v), '%s: wrote outside its slice' % what
    y = v.buf.cpu()[..., v.c0:v.c0 + v.C].permute(0, 3, 1, 2).contiguous()
    assert not bool(torch.isnan(y).any()), '%s: %d elements never written (or NaN read)' % (what, int(torch.isnan(y).sum()))
    return y


def untouched(v, what):
    """the guards hold and the slice is still all NaN: nothing wrote this view"""
    assert guards_intact(v), '%s: wrote outside its slice' % what
    y = v.buf.cpu()[..., v.c0:v.c0 + v.C]
    assert bool(torch.isnan(y).all()), '%s: %d elements written into a view the launch does not produce' % (what, int((~torch.isnan(y)).sum()))
