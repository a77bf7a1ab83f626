"""Shared by tests/test_optim_cpu.py and tests/test_hip_optim.py: the tensor list, the seeded data, torch's own CPU
trajectories (computed once per configuration) and the project's error bound."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CHUNK = 4096                                   # CT_OPTIM_CHUNK (checked against the header in test_optim_cpu.py)
# below / at / above 4 elements and a chunk, several chunks with a ragged end, more than one round of 16-byte lanes
SIZES = [1, 2, 27, 64, 512, 4095, 4096, 4097, 3 * CHUNK + 5, 70001]
VIEW_SIZES = [1030, 27]                        # the two parameters that are views at 4-byte-aligned offsets
STEPS = 5
LRS = (1e-2, 2e-2)                             # group 0: the first five tensors; group 1: the rest and the views
SKIP = {3: (1, 3)}                             # tensor 3 has no gradient on steps 2 and 4 (counted from 1)
HYPER = {'adam': dict(betas=(0.9, 0.999), eps=1e-8), 'sgd': dict(momentum=0.9)}
STATE_KEYS = {'adam': ('exp_avg', 'exp_avg_sq'), 'sgd': ('momentum_buffer',)}


def dlaseg_sizes():
    """the element counts of the 243 parameter tensors of DLASeg(34, MOT heads)"""
    from test_dlaseg_cpu import HEAD_CONVS, HEADS, Opt
    from centertrack_amd.dla_seg import DLASeg
    return [p.numel() for p in DLASeg(34, HEADS, HEAD_CONVS, Opt()).parameters()]


@functools.lru_cache(maxsize=None)
def data(seed=20):
    """(initial parameters, gradients[step][tensor] or None) as float32 numpy arrays for SIZES + VIEW_SIZES.  Across the
    tensors the gradients hold exact zeros (tensor 2 wholly, every seventh element elsewhere) and the magnitudes 1e-6
    (tensor 4), 1, 1e4 (tensor 6) and 1e-20 (tensor 1)."""
    rs = np.random.RandomState(seed)
    sizes = SIZES + VIEW_SIZES
    scale = {1: 1e-20, 2: 0.0, 4: 1e-6, 6: 1e4}
    params = [rs.randn(n).astype(np.float32) for n in sizes]
    grads = []
    for step in range(STEPS):
        row = []
        for i, n in enumerate(sizes):
            if step in SKIP.get(i, ()):
                row.append(None)
                continue
            g = (rs.randn(n) * scale.get(i, 1.0)).astype(np.float32)
            g[::7] = 0.0
            row.append(g)
        grads.append(row)
    return params, grads


def groups(tensors, kind, wd):
    kw = dict(HYPER[kind], weight_decay=wd)
    return [dict(params=tensors[:5], lr=LRS[0], **kw), dict(params=tensors[5:], lr=LRS[1], **kw)]


def torch_class(kind):
    return torch.optim.Adam if kind == 'adam' else torch.optim.SGD


def snapshot(opt, tensors, kind):
    """[(p, state tensors...) per tensor] as float64 numpy arrays (None where the state does not exist yet)"""
    out = []
    for p in tensors:
        st = opt.state.get(p, {})
        out.append([p.detach().cpu().double().numpy().copy()]
                   + [st[k].detach().cpu().double().numpy().copy() if st.get(k) is not None else None
                      for k in STATE_KEYS[kind]])
    return out


@functools.lru_cache(maxsize=None)
def torch_trajectory(kind, wd, dtype):
    """torch's own single-tensor optimizer on the CPU in ``dtype`` over data(): the snapshot after every step"""
    params, grads = data()
    tensors = [torch.tensor(p, dtype=dtype).requires_grad_() for p in params]
    opt = torch_class(kind)(groups(tensors, kind, wd), foreach=False)
    traj = []
    for row in grads:
        for t, g in zip(tensors, row):
            t.grad = None if g is None else torch.tensor(g, dtype=dtype)
        opt.step()
        traj.append(snapshot(opt, tensors, kind))
    return traj


def bound(ref64, ref32):
    """the project's bound for one tensor: 4 max(e32, 2^-23) max|ref|, e32 = the error of torch's own float32 CPU
    trajectory against float64 on the same data, relative to max|ref|"""
    top = float(np.abs(ref64).max())
    e32 = float(np.abs(ref32 - ref64).max())
    return 4.0 * max(e32, 2.0 ** -23 * top)


def check_against(got, ref64, ref32, what, worst):
    """``got`` (float64 array) within the bound; records the largest error / bound ratio in ``worst[0]``"""
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ref64).max())
    b = bound(ref64, ref32)
    if b == 0.0:
        assert err == 0.0, (what, err)
        return
    worst[0] = max(worst[0], err / b)
    assert err <= b, '%s: error %.3e above the bound %.3e' % (what, err, b)
