"""Golden vectors of the training loss from the reference's own ``trainer.GenericLoss`` (build container only, like
make_golden.py): tests/golden/losses.npz.

Per case: the inputs as float32 values, the reference's per-head losses and logit gradients computed in float64 from
those values, and the reference's own float32 error against them (``e32``: relative loss error, gradient max-error over
gradient max).  The file is written with fixed zip timestamps, so a second run reproduces it byte for byte.

    python tests/golden/make_loss_golden.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_import  # noqa: E402

ref_import.install()

import torch  # noqa: E402
from trainer import GenericLoss  # noqa: E402  (the reference's)

import _loss_ref as R  # noqa: E402  (input generation only)


def case_a():
    """B = 2, 8 x 12, M = 16, 10 classes, 11 and 5 objects; three slots share one ind, two of them one cat; ind 0 and
    H*W - 1 present; logits scaled by 3 -- all eleven heads"""
    out, batch = R.make_batch(11, 2, 8, 12, 16, R.ALL_HEADS, 10, valid=[11, 5], scale=3.0)
    ind, cat = batch['ind'], batch['cat']
    ind[0, 0], ind[0, 1] = 0, 95
    ind[0, 2] = ind[0, 3] = ind[0, 4] = 41
    cat[0, 2] = cat[0, 3] = 6
    cat[0, 4] = 2
    ind[1, 0], ind[1, 1] = 95, 0
    hm = batch['hm']
    for b, n in ((0, 11), (1, 5)):
        for m in range(n):
            hm[b, cat[b, m], ind[b, m] // 12, ind[b, m] % 12] = 1
    return out, batch, R.ALL_HEADS


def case_b():
    """pose: hm, hm_hp, hps, hp_offset, reg, wh with hp_ind of length M * 17"""
    heads = ('hm', 'hm_hp', 'hps', 'hp_offset', 'reg', 'wh')
    out, batch = R.make_batch(12, 2, 6, 8, 4, heads, 1, valid=[3, 2], scale=2.0)
    return out, batch, heads


def case_c():
    """the MOT heads with every mask zero: the num_pos == 0 branch and the 1e-4 denominators"""
    heads = ('hm', 'reg', 'wh', 'tracking', 'ltrb_amodal')
    out, batch = R.make_batch(13, 2, 8, 12, 16, heads, 1, valid=[0, 0], scale=3.0)
    return out, batch, heads


def reference(out, batch, heads, dtype):
    """the reference's GenericLoss per head in ``dtype`` -> {head: (loss, d loss / d logits)}"""
    opt = R.Opt(heads)
    crit = GenericLoss(opt)
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    leaves = {h: out[h].to(dtype).requires_grad_() for h in heads}
    # (the reference transforms hm / hm_hp / dep in place: hand it non-leaf copies)
    _, stats = crit([{h: leaves[h] * 1 for h in heads}], b)
    return {h: (stats[h].detach(), torch.autograd.grad(stats[h], leaves[h], retain_graph=True)[0]) for h in heads}


def main():
    torch.set_num_threads(1)
    arrays = {}
    for name, make in (('A', case_a), ('B', case_b), ('C', case_c)):
        out, batch, heads = make()
        arrays['%s/heads' % name] = np.array(','.join(heads))
        for h in heads:
            arrays['%s/out/%s' % (name, h)] = out[h].numpy()
        for k, v in batch.items():
            arrays['%s/batch/%s' % (name, k)] = v.numpy()
        r64, r32 = reference(out, batch, heads, torch.float64), reference(out, batch, heads, torch.float32)
        for h in heads:
            l64, g64 = r64[h]
            l32, g32 = r32[h]
            arrays['%s/loss/%s' % (name, h)] = l64.numpy()
            arrays['%s/grad/%s' % (name, h)] = g64.numpy()
            e_loss = abs(float(l32) - float(l64)) / max(abs(float(l64)), 1e-300)
            gmax = float(g64.abs().max())
            e_grad = float((g32.double() - g64).abs().max()) / (gmax if gmax > 0 else 1.0)
            arrays['%s/e32_loss/%s' % (name, h)] = np.float64(e_loss)
            arrays['%s/e32_grad/%s' % (name, h)] = np.float64(e_grad)
            print('%s %-14s loss %.9g  e32 loss %.2e grad %.2e' % (name, h, float(l64), e_loss, e_grad))
    path = os.path.join(HERE, 'losses.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
