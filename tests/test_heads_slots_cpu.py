"""CPU: what the slot-heads GPU tests (tests/test_hip_heads_slots.py) rest on.  The truth they use -- the reference's dense
heads read at the slots -- has the gradients of the pipeline the module runs (gather, matmul, ReLU, matmul, fold); the
owner-order restatement of ct_slot_fold has one owner per cell; the fixtures flip no ReLU unit in float32; the two C entry
points reject bad descriptors; the module's parameters do not depend on the flag."""
import ctypes
from collections import OrderedDict

import pytest
import torch

import _heads_slots as S


@pytest.mark.parametrize('combo', S.COMBOS, ids=S.combo_id)
def test_dense_heads_at_the_slots_have_the_gradients_of_the_slot_pipeline(combo):
    fx = S.fixture(combo)
    slot, _ = S.split(fx['heads'])
    want = S.autograd(fx, torch.float64, slot)
    got = S.slot_pipeline(fx, torch.float64)

    def close(name, a, b):
        scale = max(float(b.abs().max()), 1.0)
        assert float((a - b).abs().max()) <= 1e-12 * scale, (name, float((a - b).abs().max()), scale)
    close('x', got['x'], want['x'])
    for h in slot:
        for k in ('out', 'w0', 'b0', 'w2', 'b2'):
            close('%s %s' % (k, h), got[k][h], want[k][h])


@pytest.mark.parametrize('case', list(S.CASES))
def test_the_fold_in_owner_order_has_one_owner_per_cell_and_the_sum_of_index_add(case):
    (B, H, W, M), ind = S.CASES[case]
    g = torch.Generator().manual_seed(5)
    P = torch.randn((B, M, 9, 8), generator=g)
    gx = torch.randn((B, H, W, 8), generator=g)
    got, owner, count = S.fold_owner_order(P, ind, gx)
    assert torch.equal(owner, S.lowest_covering_slot(ind, H, W))
    untouched = owner < 0
    assert torch.equal(got[untouched], gx[untouched])
    v = S.valid_of(ind, H, W)
    if not bool(v.any()):
        assert bool(untouched.all())
        return
    assert int(count.max()) >= (2 if M > 1 else 1)
    f64 = S.fold_index_add(P.double(), ind, gx.double())
    f32 = S.fold_index_add(P, ind, gx)
    K = int(count.max()) + 1
    assert S.err(got, f64) <= S.bound(S.err(f32, f64), K)


@pytest.mark.parametrize('combo', S.COMBOS, ids=S.combo_id)
def test_float32_flips_no_hidden_unit(combo):
    """a condition of the fixtures, not a measurement: dyadic x, w0, b0 make the pre-activation exact"""
    _, t64, t32 = S.truth(combo)
    flips = sum(int(((t32['pre'][h] > 0) != (t64['pre'][h] > 0)).sum()) for h in t64['pre'])
    assert flips == 0
    for h in t64['pre']:
        assert torch.equal(t32['pre'][h].double(), t64['pre'][h])


def test_the_entry_points_reject_bad_descriptors_without_a_gpu():
    from centertrack_amd import _lib, build
    build.build()
    l = _lib.load()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16

    def good():
        d = _lib.SlotDesc()
        d.map, d.N, d.H, d.W, d.C, d.ld = base, 1, 4, 4, 64, 64
        d.ind, d.M = base, 3
        d.rows, d.ldr = base, 576
        return d

    def bad(**kw):
        d = good()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = [('null', None), ('null', bad(map=None)), ('null', bad(ind=None)), ('null', bad(rows=None)),
             ('shape', bad(N=0)), ('shape', bad(H=-1)), ('shape', bad(W=0)), ('shape', bad(C=0)),
             ('M=', bad(M=0)), ('M=', bad(M=-3)),
             ('pitch', bad(ld=60)), ('pitch', bad(ldr=572)),
             ('aligned', bad(map=base + 4)), ('aligned', bad(rows=base + 8)), ('aligned', bad(ind=base + 4)),
             ('aligned', bad(ld=66)), ('aligned', bad(ldr=578)), ('multiple of 4', bad(C=6, ld=8)),
             ('2 GiB', bad(N=2048, H=128, W=128)), ('2 GiB', bad(N=1024, M=1024))]
    for entry in (l.ct_slot_gather, l.ct_slot_fold):
        for word, d in cases:
            rc = entry(ctypes.byref(d) if d is not None else None, None)
            assert rc == _lib.CT_ERR_ARG, (word, rc)
            assert word.encode() in l.ct_last_error(), (word, l.ct_last_error())


def test_the_ctypes_descriptor_matches_the_header_layout(tmp_path):
    import os
    import shutil
    import subprocess
    from centertrack_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    fields = [f for f, _ in _lib.SlotDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "centertrack_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ct_slot_desc));']
    lines += ['printf("%s %%zu\\n", offsetof(ct_slot_desc, %s));' % (f, f) for f in fields] + ['return 0; }']
    src, exe = tmp_path / 'lay.c', tmp_path / 'lay'
    src.write_text('\n'.join(lines))
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    r = subprocess.run([gcc, '-std=c99', '-I' + os.path.join(root, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.SlotDesc)
    for f in fields:
        assert int(got[f]) == getattr(_lib.SlotDesc, f).offset, f


@pytest.mark.parametrize('hs', list(S.HEAD_SETS))
def test_the_module_keeps_its_parameters_and_splits_the_heads(hs):
    from centertrack_amd import heads as HD
    heads = S.HEAD_SETS[hs]
    torch.manual_seed(0)
    dense = HD.FusedHeads(heads, 256)
    torch.manual_seed(0)
    slots = HD.FusedHeads(heads, 256, slot_heads=True)
    a, b = dense.state_dict(), slots.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k           # names, shapes and initialisation
    slots.load_state_dict(a)
    dense.load_state_dict(b)
    assert tuple(HD.SLOT_HEADS) == S.SLOT_HEADS
    assert dense.slot_head_names() == ()
    want = {'mot': ('reg', 'wh', 'tracking', 'ltrb_amodal'),
            'nusc': ('reg', 'wh', 'tracking', 'dep', 'rot', 'dim', 'amodel_offset', 'nuscenes_att', 'velocity'),
            'pose': ('hps',)}[hs]
    assert slots.slot_head_names() == want
    assert [h for h in heads if h not in want] == S.split(heads)[1]


def test_a_cpu_tensor_raises():
    from centertrack_amd import _lib
    from centertrack_amd import heads as HD
    m = HD.FusedHeads(OrderedDict([('hm', 1), ('wh', 2)]), 256, slot_heads=True)
    ind = torch.zeros((1, 4), dtype=torch.int64)
    with pytest.raises(_lib.CTError):
        m(torch.zeros(1, 64, 4, 4), ind)
    with pytest.raises(_lib.CTError):
        m.forward_nhwc(torch.zeros(1, 4, 4, 64), ind)
