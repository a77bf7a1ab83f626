"""Golden vectors of the training loss on NON-FINITE logits from the reference's own ``trainer.GenericLoss`` (build container
only, like make_loss_golden.py): tests/golden/losses_nonfinite.npz.

One batch (tests/_nonfinite.py: ``loss_base``) and, per plant of ``loss_plants`` (one logit replaced by NaN, +Inf or -Inf), the
reference's per-head losses and the logit gradient of the planted head, computed in float64 from the float32 inputs.  The other
heads' gradients do not depend on the plant.  Written with fixed zip timestamps: a second run reproduces the file byte for byte.

    python tests/golden/make_loss_nonfinite_golden.py
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

import _nonfinite as NF  # noqa: E402  (input generation only)
from make_loss_golden import reference  # noqa: E402


def main():
    torch.set_num_threads(1)
    out, batch = NF.loss_base()
    heads = NF.LOSS_HEADS
    arrays = {}
    for h in heads:
        arrays['base/out/%s' % h] = out[h].numpy()
    for k, v in batch.items():
        arrays['base/batch/%s' % k] = v.numpy()
    names = []
    for name, head, flat, v in NF.loss_plants():
        o, b, _ = NF.loss_case(name)
        r64 = reference(o, b, heads, torch.float64)
        names.append(name)
        for h in heads:
            arrays['%s/loss/%s' % (name, h)] = r64[h][0].numpy()
        g = r64[head][1].contiguous()
        arrays['%s/grad' % name] = g.numpy()
        print('%-24s %-13s loss %-12.9g non-finite gradient elements %d, at the plant %s' % (
            name, head, float(r64[head][0]), int((~torch.isfinite(g)).sum()), float(g.view(-1)[flat])))
    arrays['cases'] = np.array(','.join(names))
    path = os.path.join(HERE, 'losses_nonfinite.npz')
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
