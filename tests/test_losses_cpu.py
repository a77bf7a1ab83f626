"""CPU: the float64 mirror of the training loss (tests/_loss_ref.py) reproduces the reference's own numbers
(tests/golden/losses.npz, from tests/golden/make_loss_golden.py); the loss entry points of the C ABI reject bad
descriptors before any launch; the ctypes descriptors have the header's layout."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _loss_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CASES, load_case = R.CASES, R.load_case


def test_golden_file_is_small_and_holds_the_three_cases(golden_dir):
    path = os.path.join(golden_dir, 'losses.npz')
    assert os.path.getsize(path) < 256 * 1024
    a, b, c = (load_case(golden_dir, n) for n in CASES)
    assert a['heads'] == list(R.ALL_HEADS) and a['out']['hm'].shape == (2, 10, 8, 12) and a['batch']['ind'].shape == (2, 16)
    ind, cat, mask = a['batch']['ind'], a['batch']['cat'], a['batch']['mask']
    assert mask.sum(1).tolist() == [11, 5]
    assert ind[0, 2] == ind[0, 3] == ind[0, 4] and cat[0, 2] == cat[0, 3] != cat[0, 4]
    assert 0 in ind[0, :11].tolist() and 95 in ind[0, :11].tolist()
    assert b['heads'] == ['hm', 'hm_hp', 'hps', 'hp_offset', 'reg', 'wh']
    assert b['batch']['hp_ind'].shape[1] == b['batch']['ind'].shape[1] * 17
    assert c['heads'] == ['hm', 'reg', 'wh', 'tracking', 'ltrb_amodal']
    assert all(float(v.abs().sum()) == 0 for k, v in c['batch'].items() if k.endswith('mask'))
    for case in (a, b, c):
        assert all(v.dtype in (torch.float32, torch.int64) for v in list(case['out'].values()) + list(case['batch'].values()))


@pytest.mark.parametrize('name', CASES)
def test_mirror_reproduces_the_reference_in_float64(golden_dir, name):
    """1e-12 relative on every loss and on every gradient (max error over gradient max)"""
    g = load_case(golden_dir, name)
    got = R.losses_and_grads(g['out'], g['batch'], g['heads'], torch.float64)
    for h in g['heads']:
        loss, grad = got[h]
        want = float(g['loss'][h])
        assert abs(float(loss) - want) <= 1e-12 * max(abs(want), 1e-300) or want == float(loss), (h, float(loss), want)
        assert R.err(grad, g['grad'][h]) <= 1e-12, h
    tot, _ = R.generic_loss([{h: g['out'][h].double() for h in g['heads']}],
                            {k: (v.double() if v.is_floating_point() else v) for k, v in g['batch'].items()},
                            g['heads'], R.Opt(g['heads']).weights)
    want = sum((0.1 if h == 'wh' else 1.0) * float(g['loss'][h]) for h in g['heads'])
    assert abs(float(tot) - want) <= 1e-12 * abs(want)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_hip_losses_scale.py: what the GPU tests rely on, checked without a GPU

def _float32_mirror_is_inside_the_bounds(want, e32, heads, terms):
    """the float32 composition of the same formulas passes the check the kernels are held to: its own errors are finite
    and below the cap of 1e-3 at which ``bound`` stops following e32"""
    for h in heads:
        assert e32[h][0] <= R.bound(e32[h][0], terms[h]), (h, 'loss', e32[h][0])
        assert e32[h][1] <= R.bound(e32[h][1], 1), (h, 'grad', e32[h][1])
        assert float(want[h][1].abs().max()) > 0, h


def test_scale_inputs_every_partial_carries_more_than_twice_the_tolerance():
    out, batch = R.scale_batch()
    B, C, H, W, M = R.SCALE
    n = out['hm'].numel()
    assert tuple(out['hm'].shape) == (B, C, H, W) and n == 4259840 and R.CAP == 4194304 and R.CAP < n and n % R.TRIP
    want, e32 = R.truth_and_e32('scale', out, batch, ('hm',))
    _float32_mirror_is_inside_the_bounds(want, e32, ('hm',), {'hm': n})
    tol = min(R.bound(e32['hm'][0], n), R.SHARE_TOL)
    assert e32['hm'][0] <= tol
    for vec in (True, False):
        shares = R.scale_shares(vec)
        print('loss scale cpu %s path: shares min %.3e max %.3e, e32 loss %.3e grad %.3e, tolerance %.3e'
              % ('float4' if vec else 'scalar', float(shares.min()), float(shares.max()), e32['hm'][0], e32['hm'][1], tol))
        assert shares.shape == (R.MAX_PARTIALS,) and 0.99 < float(shares.sum()) < 1      # (the positives are the rest)
        assert tol < 0.5 * float(shares.min())
        # the project bound alone would not do: it is as large as a whole share
        assert R.bound(e32['hm'][0], n) > 0.5 * float(shares.min())


def test_scale_probes_miss_the_positives_and_carry_the_whole_negative_sum():
    out, batch, probes = R.probe_batch()
    B, C, H, W, M = R.SCALE
    n, S = out['hm'].numel(), R.TRIP
    assert probes == [0, 3, 4, n - 1, n - 4, n - 5, S - 1, S, S + 1, 3 * S - 1, 3 * S, n // 2]
    assert len(set(probes)) == 12 and all(0 <= p < n for p in probes)
    pos = R.positive_elements(batch, out['hm'].shape)
    assert len(pos) == len(set(pos)) == int(batch['mask'].sum()) == 17 and not set(pos) & set(probes)
    assert int((batch['hm'] == 0).sum()) == 12 and int((batch['hm'] == 1).sum()) == n - 12
    want, e32 = R.truth_and_e32('probes', out, batch, ('hm',))
    K = len(probes) + B * M
    _float32_mirror_is_inside_the_bounds(want, e32, ('hm',), {'hm': K})
    g = want['hm'][1].reshape(-1)
    live = torch.zeros(n, dtype=torch.bool)
    live[probes + pos] = True
    assert float(g[~live].abs().max()) == 0.0 and bool((g[probes] != 0).all())          # no probe sits in the clamp
    # every probe is a visible part of the loss: losing or doubling one moves it by far more than the bound
    x, mask = out['hm'].double().reshape(-1)[probes], float(batch['mask'].sum())
    p = torch.sigmoid(x)
    each = -(torch.log(1 - p) * p ** 2) / mask / float(want['hm'][0])
    print('loss probes cpu: smallest probe share of the loss %.3e, bound %.3e' % (float(each.min()), R.bound(e32['hm'][0], K)))
    assert float(each.min()) > 1e-3 > 100 * R.bound(e32['hm'][0], K) and len(set(each.tolist())) == 12


def test_slot_limit_and_fifteen_head_inputs():
    out, batch, heads = R.slot_limit_batch()
    assert heads == ('hm', 'reg', 'hm_hp', 'hp_offset') and tuple(out['hm_hp'].shape) == (2, 16, 16, 24)
    assert batch['hp_ind'].shape == (2, R.MAX_SLOTS) and int(batch['hp_ind'].max()) < 16 * 24
    # every position is named by many slots of either image
    for b in (0, 1):
        live = batch['hp_ind'][b][batch['hm_hp_mask'][b] > 0]
        assert live.numel() > 5000 and torch.bincount(live, minlength=384).min() >= 4
        assert int((batch['hp_ind'][b] == 0).sum()) > 2000            # the masked slots all name position 0
    want, e32 = R.truth_and_e32('slots', out, batch, heads)
    M = {'hm': 512, 'reg': 512, 'hm_hp': R.MAX_SLOTS, 'hp_offset': R.MAX_SLOTS}
    _float32_mirror_is_inside_the_bounds(want, e32, heads, {h: R.terms(h, out[h].shape, M[h]) for h in heads})
    from centertrack_amd import losses
    out, batch = R.fifteen_batch()
    assert sorted(R.FIFTEEN) == sorted(losses.KNOWN_HEADS) and list(out) == list(R.FIFTEEN)
    assert tuple(out['ltrb'].shape) == (2, 4, 8, 12) and tuple(out['hps'].shape) == (2, 34, 8, 12)
    assert batch['hps'].shape == batch['hps_mask'].shape == (2, 8, 34) and batch['hp_ind'].shape == (2, 8 * 17)
    want, e32 = R.truth_and_e32('fifteen', out, batch, R.FIFTEEN)
    terms = {h: R.terms(h, out[h].shape, 8 * 17 if h in ('hm_hp', 'hp_offset') else 8) for h in R.FIFTEEN}
    _float32_mirror_is_inside_the_bounds(want, e32, R.FIFTEEN, terms)


# ---------------------------------------------------------------------------------------------------------------------
# host-side validation (no GPU: nothing is launched for a rejected descriptor)

@pytest.fixture(scope='module')
def lib():
    from centertrack_amd import _lib
    return _lib.load()


def _desc(nheads=1, kind=1, C=2, M=4, B=1, H=4, W=4):
    from centertrack_amd import _lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    heads = (_lib.LossHead * nheads)()
    for h in heads:
        h.kind, h.logits, h.C, h.target, h.mask, h.ind, h.cat, h.M, h.grad = kind, p, C, p, p, p, p, M, p
    d = _lib.LossDesc()
    d.B, d.H, d.W, d.heads, d.nheads = B, H, W, heads, nheads
    d.loss = d.grad_loss = d.workspace = p
    d.workspace_bytes = 4096 * 4
    return d, heads, buf


def _rejected(lib, d, code, text):
    for fn in (lib.ct_generic_loss_forward, lib.ct_generic_loss_backward):
        assert fn(ctypes.byref(d), None) == code
        assert text in lib.ct_last_error(), lib.ct_last_error()


def test_loss_entry_points_validate_before_any_launch(lib):
    from centertrack_amd import _lib
    ARG, WS = _lib.CT_ERR_ARG, _lib.CT_ERR_WORKSPACE
    for fn in (lib.ct_generic_loss_forward, lib.ct_generic_loss_backward):
        assert fn(None, None) == ARG and b'null descriptor' in lib.ct_last_error()
    assert lib.ct_generic_loss_workspace_bytes(None) == 0
    d, heads, _ = _desc()
    d.heads = None
    _rejected(lib, d, ARG, b'null head array')
    d, heads, _ = _desc()
    d.nheads = 0
    _rejected(lib, d, ARG, b'nheads')
    d, heads, _ = _desc(nheads=_lib.CT_LOSS_MAX_HEADS)
    d.nheads = _lib.CT_LOSS_MAX_HEADS + 1
    _rejected(lib, d, ARG, b'nheads')
    for field in ('logits', 'target', 'mask', 'ind'):
        d, heads, _ = _desc()
        setattr(heads[0], field, None)
        _rejected(lib, d, ARG, b'null')
    d, heads, _ = _desc()
    d.loss = None
    assert lib.ct_generic_loss_forward(ctypes.byref(d), None) == ARG and b'null loss' in lib.ct_last_error()
    d.grad_loss = None
    assert lib.ct_generic_loss_backward(ctypes.byref(d), None) == ARG and b'null grad_loss' in lib.ct_last_error()
    for kind in (-1, 5, 77):
        d, heads, _ = _desc(kind=kind)
        _rejected(lib, d, ARG, b'unknown kind')
    for field in ('C', 'M'):
        for v in (0, -3):
            d, heads, _ = _desc()
            setattr(heads[0], field, v)
            _rejected(lib, d, ARG, b'must be positive')
    for field in ('B', 'H', 'W'):
        for v in (0, -1):
            d, heads, _ = _desc()
            setattr(d, field, v)
            _rejected(lib, d, ARG, b'must be positive')
            assert lib.ct_generic_loss_workspace_bytes(ctypes.byref(d)) == 0
    d, heads, _ = _desc(kind=_lib.CT_LOSS_FOCAL)
    heads[0].cat = None
    _rejected(lib, d, ARG, b'focal head needs cat')
    d, heads, _ = _desc(kind=_lib.CT_LOSS_ROT, C=4)
    _rejected(lib, d, ARG, b'C = 8')
    d, heads, _ = _desc(kind=_lib.CT_LOSS_ROT, C=8)
    heads[0].cat = None
    _rejected(lib, d, ARG, b'rotbin')
    d, heads, _ = _desc()
    heads[0].M = _lib.CT_LOSS_MAX_SLOTS + 1
    _rejected(lib, d, ARG, b'CT_LOSS_MAX_SLOTS')
    # the workspace: the query is positive for a good descriptor and grows with the partials of a focal head
    d, heads, _ = _desc(kind=_lib.CT_LOSS_FOCAL, C=3, H=64, W=64, B=2)
    need = lib.ct_generic_loss_workspace_bytes(ctypes.byref(d))
    small, _h, _ = _desc()
    assert need > lib.ct_generic_loss_workspace_bytes(ctypes.byref(small)) > 0
    d.workspace_bytes = need - 4
    _rejected(lib, d, WS, b'workspace')
    d.workspace_bytes, d.workspace = need, None
    _rejected(lib, d, WS, b'workspace')


def test_loss_descriptors_match_the_header_layout(tmp_path):
    """as tests/test_cabi.py does for the other descriptors: sizes and field offsets from a C compiler"""
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    checks = {'ct_loss_head': (_lib.LossHead, [n for n, _ in _lib.LossHead._fields_]),
              'ct_loss_desc': (_lib.LossDesc, [n for n, _ in _lib.LossDesc._fields_])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {']
    for cname, (_, fields) in checks.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for name in ('CT_LOSS_FOCAL', 'CT_LOSS_L1', 'CT_LOSS_L1_DEPTH', 'CT_LOSS_BCE', 'CT_LOSS_ROT', 'CT_LOSS_MAX_HEADS',
                 'CT_LOSS_MAX_SLOTS'):
        lines.append('printf("%s %%d\\n", %s);' % (name, name))
    lines += ['return 0; }']
    src = tmp_path / 'lay.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'lay'
    r = subprocess.run([gcc, '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, (cls, fields) in checks.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in fields:
            assert int(got['%s.%s' % (cname, f)]) == getattr(cls, f).offset, '%s.%s' % (cname, f)
    for name in ('CT_LOSS_FOCAL', 'CT_LOSS_L1', 'CT_LOSS_L1_DEPTH', 'CT_LOSS_BCE', 'CT_LOSS_ROT', 'CT_LOSS_MAX_HEADS',
                 'CT_LOSS_MAX_SLOTS'):
        assert int(got[name]) == getattr(_lib, name)


def test_cpu_tensors_raise_cterror():
    from centertrack_amd import _lib, losses
    out, batch = R.make_batch(1, 1, 4, 4, 2, ('hm', 'reg'), 2)
    with pytest.raises(_lib.CTError):
        losses.GenericLoss(R.Opt(('hm', 'reg')))([out], batch)
    with pytest.raises(_lib.CTError):
        losses.RegWeightedL1Loss()(out['reg'], batch['reg_mask'], batch['ind'], batch['reg'])
