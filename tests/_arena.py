"""Device-side caller buffers for the near-limit GPU tests (tests/test_hip_limits.py).  ``tests/_guards.py`` builds and checks its
buffers on the host, which is too slow at 2 GiB; here a view lies inside one device allocation (an ``Arena``) that is filled with a
sentinel, a NaN payload no arithmetic produces (as in tests/test_hip_optim.py), with FRONT = 2 GiB of sentinel in front of the
view's first byte and BACK = 4 GiB behind its last.  An offset that is wrong by a sign or by a 32-bit wrap therefore lands in
memory the test owns and shows up as a changed sentinel.  ``check`` counts, in chunks and on the device, the words outside the
channel slice that no longer hold the sentinel; ``take`` also counts the words inside an output slice that still do, and copies
only the slice itself to the host.  No host copy of anything but the slice is ever made."""
import torch

from _limits import extent_bytes

SENTINEL = 0x7FC0BEEF                          # a NaN payload no arithmetic produces
FRONT, BACK = 2 ** 31, 2 ** 32                 # bytes of sentinel in front of the view's first byte / behind its last
CHUNK = 1 << 26                                # words compared at a time (256 MiB; the comparison's mask is 64 MiB)


class Arena(object):
    """one allocation: FRONT bytes of sentinel, the NHWC buffer [N, H, W, ld] whose channels [0, C) are the view, BACK bytes of
    sentinel.  ``view`` is an ``ops.View`` of it."""

    def __init__(self, N, H, W, Cc, ld, device):
        from centertrack_amd import ops
        assert ld >= Cc and ld % 4 == 0
        self.shape, self.C, self.ld = (N, H, W), Cc, ld
        self.px = N * H * W
        self.lo = FRONT // 4
        self.hi = self.lo + self.px * ld
        self.words = torch.full((self.hi + BACK // 4,), SENTINEL, dtype=torch.int32, device=device)
        self.view = ops.View(self.words[self.lo:self.hi].view(torch.float32).view(N, H, W, ld), 0, Cc)
        assert self.view.ptr == self.words.data_ptr() + FRONT
        self.extent = extent_bytes(self.px, ld, Cc)

    def bytes(self):
        return self.words.numel() * 4

    def fill(self, t_nchw):
        """the tensor (NCHW, on any device) into the channel slice; the rest of every pixel keeps the sentinel"""
        N, Cc, H, W = t_nchw.shape
        assert (N, H, W) == self.shape and Cc == self.C
        self.view.buf[..., :Cc] = t_nchw.permute(0, 2, 3, 1).to(self.words.device, torch.float32)
        return self

    def outside_changed(self):
        """how many words outside the channel slice no longer hold the sentinel (counted on the device, one number comes back)"""
        bad = torch.zeros((), dtype=torch.int64, device=self.words.device)
        for a, b in ((0, self.lo), (self.hi, self.words.numel())):
            for s in range(a, b, CHUNK):
                bad += (self.words[s:min(b, s + CHUNK)] != SENTINEL).sum()
        rows = self.words[self.lo:self.hi].view(self.px, self.ld)
        step = max(1, CHUNK // self.ld)
        for s in range(0, self.px, step):
            bad += (rows[s:s + step, self.C:] != SENTINEL).sum()
        return int(bad)

    def check(self, what):
        n = self.outside_changed()
        assert n == 0, '%s: %d words outside the channel slice changed (pitch %d, extent %d bytes)' % (what, n, self.ld, self.extent)

    def take_device(self, what):
        """an output: nothing outside the slice changed, every element inside was written -> the slice as a strided [N, H, W, C]
        view on the device (no copy)"""
        self.check(what)
        rows = self.words[self.lo:self.hi].view(self.px, self.ld)
        step = max(1, CHUNK // self.C)
        left = sum((rows[s:s + step, :self.C] == SENTINEL).sum() for s in range(0, self.px, step))
        assert int(left) == 0, '%s: %d elements never written' % (what, int(left))
        return self.view.buf[..., :self.C]

    def take(self, what):
        """``take_device``, then the slice alone as NCHW on the CPU"""
        return self.take_device(what).contiguous().cpu().permute(0, 3, 1, 2).contiguous()

    def free(self):
        self.view = self.words = None
