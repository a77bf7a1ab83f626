"""CPU: the checkpoint-like weight family of tests/_ckpt_weights.py -- its conditions on the float64 oracle for every case of
tests/test_hip_ckpt_weights.py, determinism and key set, and the reason for the family and for its bar: wrong float32 oracles
(mutants) that the bound ``min(1e-3, 10 * max(e32, 2^-23 sqrt(4608)))`` catches under these weights, that
``atol = rtol = 1e-3`` lets through, and that the benign weights of ``make_synthetic_state_dict`` cannot see at all."""
import pytest
import torch

import _ckpt_weights as C
from _dcn_bwd import err

# (head set, shape, seed, head_conv) of every checkpoint-like case of tests/test_hip_ckpt_weights.py
PLAN_CASES = [(h, s, 317, 256) for h in ('mot', 'nusc', 'pose') for s in C.SHAPES] + [('mot', (1, 64, 96), 317, 64)]
TRAIN_CASES = [('mot4', s, 5200, 256) for s in C.SHAPES]
CASES = PLAN_CASES + TRAIN_CASES


def case_id(c):
    return '%s-%s-seed%d-hc%d' % (c[0], 'x'.join(str(v) for v in c[1]), c[2], c[3])


def test_the_cases_use_the_listed_seeds():
    assert {c[2] for c in CASES} == set(C.SEEDS) and {c[1] for c in CASES} == set(C.SHAPES)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_conditions(case):
    name, shape, seed, hc = case
    sd, inputs, t64, t32, offsets, e32 = C.truth('ckpt', name, shape, seed, hc)
    rows = C.conditions(sd, t64, offsets, e32)
    print(case_id(case), C.summary(rows))
    assert len(offsets) == 16 and not C.failed(rows), C.failed(rows)
    # the cap holds for every compared tensor, not only for the feature map; hm is spread, not saturated
    assert max(e32.values()) <= C.E32_CAP, max(e32.items(), key=lambda kv: kv[1])
    score = torch.sigmoid(t64['head hm'])
    print('   hm scores %.3f .. %.3f, %.2f of them in (0.01, 0.99)' % (
        float(score.min()), float(score.max()), float(((score > 0.01) & (score < 0.99)).double().mean())))
    assert float(((score > 0.01) & (score < 0.99)).double().mean()) >= 0.9 and float(score.max() - score.min()) >= 0.3


@pytest.mark.parametrize('name,hc', [('mot', 256), ('pose', 64)])
def test_deterministic_with_the_synthetic_key_set(name, hc):
    from centertrack_amd import weights as W
    heads = C.head_sets()[name]
    a = C.checkpoint_like_state_dict(heads, 317, hc)
    C._trunk_cache.clear()                                              # the second draw starts from nothing
    b = C.checkpoint_like_state_dict(heads, 317, hc)
    ref = W.make_synthetic_state_dict(heads, seed=317, head_conv=hc)
    assert list(a) == list(ref) == list(b)
    for k in ref:
        assert a[k].shape == ref[k].shape and a[k].dtype == ref[k].dtype and torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k
    other = C.checkpoint_like_state_dict(heads, 318, hc)
    assert not torch.equal(other['base.level2.tree1.bn1.weight'], a['base.level2.tree1.bn1.weight'])
    # the trunk is the same under every head set
    c = C.checkpoint_like_state_dict(C.head_sets()['nusc'], 317, hc)
    assert all(torch.equal(a[k], c[k]) for k in a if k.split('.')[0] in C.FAMILIES)


def test_training_calibration_keeps_the_offsets_of_a_training_step_in_range():
    """under batch statistics an activation has the scale of gamma, four decades wide, not that of the folded scale: with the
    offsets calibrated on the running statistics a training step at 2 x 64 x 64 throws every sample of the 4 x 4 and 2 x 2
    maps out of the image and those DeformConv nodes are constant.  ``training=True`` calibrates under batch statistics."""
    from centertrack_amd import weights as W
    name, shape, seed, hc = TRAIN_CASES[1]
    inputs = W.synthetic_inputs(*shape, seed=seed)
    off = C.training_offsets(C.checkpoint_like_state_dict(C.head_sets()[name], seed, hc, training=True), inputs)
    for p, o in off.items():
        print('%-24s std %.2f px, max %.1f px, outside %.2f' % (p, o['std'], o['max'], o['outside']))
        assert 1.0 <= o['std'] <= 4.0 and o['max'] <= 12.0 and 0.01 <= o['outside'] <= 0.9, (p, o)
    wild = C.training_offsets(C.checkpoint_like_state_dict(C.head_sets()[name], seed, hc), inputs)
    assert max(o['outside'] for o in wild.values()) > 0.99
    # the two draws differ in the offset convs alone
    a, b = (C.checkpoint_like_state_dict(C.head_sets()[name], seed, hc, training=t) for t in (False, True))
    assert all(torch.equal(a[k], b[k]) for k in a if 'conv_offset_mask' not in k)


MUTANT_CASE = ('mot', (1, 64, 96), 317)
OUTPUTS = ['feature', 'head hm', 'head reg', 'head wh', 'head tracking', 'head ltrb_amodal']


def _mutant_rows(family):
    name, shape, seed = MUTANT_CASE
    sd, inputs, t64, t32, offsets, e32 = C.truth(family, name, shape, seed)
    heads = C.head_sets()[name]
    rows = []
    for m in C.mutants(sd):
        if m.kind in ('zero_gamma_1e-3', 'no_eps') and m.idx is None:
            rows.append((m, None, None, None))                           # nothing to apply it to
            continue
        got, _ = C.oracle_run(sd, inputs, heads, torch.float32, m)
        ratio = max(err(got[k], t64[k]) / C.bound(e32[k]) for k in OUTPUTS)
        old = all(C.old_bar_passes(got[k], t32[k]) for k in OUTPUTS)
        same = all(torch.equal(got[k], t32[k]) for k in OUTPUTS)
        rows.append((m, ratio, old, same))
    return rows


def _table(title, rows):
    lines = [title, '  %-52s %12s  %s' % ('mutant', 'err / bound', 'atol = rtol = 1e-3')]
    for m, ratio, old, same in rows:
        if ratio is None:
            lines.append('  %-52s %12s  %s' % (m, '-', 'not applicable: no such channel'))
        else:
            lines.append('  %-52s %12.3g  %s' % (m, ratio, 'bitwise the oracle' if same else 'passes' if old else 'catches it too'))
    return '\n'.join(lines)


def test_the_bound_discriminates():
    """every mutant exceeds the new bound on the feature map or a head; the table says which of them the old bar let through"""
    rows = _mutant_rows('ckpt')
    print(_table('checkpoint-like weights, %s %s seed %d' % MUTANT_CASE, rows))
    assert len(rows) == 6 and any(old for _, _, old, _ in rows)
    for m, ratio, old, same in rows:
        assert ratio is not None and ratio > 1.0, (m, ratio)
    # the clean float32 oracle itself sits at 1 / M of the bound or below
    name, shape, seed = MUTANT_CASE
    e32 = C.truth('ckpt', name, shape, seed)[5]
    assert all(e32[k] / C.bound(e32[k]) <= 1.0 / C.M for k in OUTPUTS)


def test_the_benign_weights_cannot_see_the_sign_and_zero_mutants():
    """under ``make_synthetic_state_dict`` gamma lies in [0.5, 1.5]: |gamma| is gamma, bit for bit, and no channel has a zero
    gamma to put 1e-3 into, nor an all-zero filter whose output eps alone decides.  That is the reason for the new family."""
    rows = {m.kind: (m, ratio, old, same) for m, ratio, old, same in _mutant_rows('benign:0.01')}
    print(_table('benign weights, %s %s seed %d' % MUTANT_CASE, list(rows.values())))
    assert rows['abs_gamma'][3] is True
    assert rows['zero_gamma_1e-3'][1] is None and rows['no_eps'][1] is None
    sd = C.truth('benign:0.01', *MUTANT_CASE)[0]
    assert all(not z and not d for z, d in C.zeroed(sd).values())
    assert all(float(v.min()) >= 0.5 for k, v in sd.items() if k.endswith(('bn1.weight', 'bn2.weight', 'bn.weight', 'actf.0.weight')))
