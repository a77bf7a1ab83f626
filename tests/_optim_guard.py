"""Shared by tests/test_optim_guard_cpu.py and tests/test_hip_optim_guard.py: the gradients of the
norm tests, torch's own ``clip_grad_norm_`` + optimizer trajectories on the CPU (computed once per configuration), and the
fields of ``ct_optim_guard``."""
import functools

import numpy as np
import torch

import _optim as T

U53 = 2.0 ** -53                                # the unit roundoff of a double
GUARD_FIELDS = ('sumsq', 'norm', 'norm_sum', 'norm_max', 'nonfinite', 'steps', 'skipped', 'clipped', 'nonfinite_steps',
                'coef', 'skip')
BIG = 2049 * T.CHUNK + 3                        # more chunks than the grid cap of 2048: the strided walk, a ragged end
MAGNITUDES = (1e-20, 1e-6, 1.0, 1e4, 1e30)
# T.data()'s gradients have a norm of about 5.9e5 (tensor 6: 4096 values of 1e4).  Times 4 against max_norm = 1e6 the
# coefficient is about 0.42 and the clipped gradients are 1.7 times the unclipped ones: the 1e-20 tensor's exp_avg_sq
# stays as many float32 denormal steps above zero as in tests/test_hip_optim.py, where the bound was set
CLIP_SCALE, CLIP_MAX_NORM = 4.0, 1e6


@functools.lru_cache(maxsize=None)
def norm_grads(seed=31):
    """float32 gradients for T.SIZES + T.VIEW_SIZES + [BIG]: tensor i of the first twelve has the magnitude
    MAGNITUDES[i % 5], every seventh element is an exact zero, tensor 2 is all zeros; the big tensor is of magnitude 1"""
    rs = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(T.SIZES + T.VIEW_SIZES):
        g = (rs.randn(n) * MAGNITUDES[i % len(MAGNITUDES)]).astype(np.float32)
        g[::7] = 0.0
        if i == 2:
            g[:] = 0.0
        out.append(g)
    out.append(rs.standard_normal(BIG).astype(np.float32))
    return out


def sumsq64(g):
    """numpy's float64 sum of squares (pairwise: another order than the kernel's)"""
    return float((g.astype(np.float64) ** 2).sum())


def clip_(tensors, max_norm):
    """torch's own clipping, single-tensor form; returns the total norm it found (a 0-dim tensor)"""
    return torch.nn.utils.clip_grad_norm_(tensors, max_norm, foreach=False)


@functools.lru_cache(maxsize=None)
def torch_clipped_trajectory(kind, wd, dtype, max_norm=CLIP_MAX_NORM, scale=CLIP_SCALE):
    """``clip_grad_norm_(max_norm)`` then torch's single-tensor optimizer on the CPU in ``dtype`` over ``T.data()`` (its
    gradients times ``scale``): (the snapshot after every step, the total norm of every step as a float)"""
    params, grads = T.data()
    tensors = [torch.tensor(p, dtype=dtype).requires_grad_() for p in params]
    opt = T.torch_class(kind)(T.groups(tensors, kind, wd), foreach=False)
    traj, norms = [], []
    for row in grads:
        for t, g in zip(tensors, row):
            t.grad = None if g is None else torch.tensor(g * np.float32(scale), dtype=dtype)
        norms.append(float(clip_(tensors, max_norm)))
        opt.step()
        traj.append(T.snapshot(opt, tensors, kind))
    return traj, norms
