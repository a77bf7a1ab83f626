#!/usr/bin/env python
"""Write tests/golden/dlaseg_keys.json: [[key, shape], ...] of the state dict of the REFERENCE's own ``DLASeg`` (heads hm 1, reg 2,
wh 2, tracking 2; ``pre_img`` and ``pre_hm``; head_conv 256), in its order.  Run in the build container only (needs the reference checkout):

    python tests/golden/make_dlaseg_keys.py

tests/test_dlaseg_cpu.py holds ``centertrack_amd.dla_seg.DLASeg`` against the list."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()

HEADS = {'hm': 1, 'reg': 2, 'wh': 2, 'tracking': 2}


def main():
    from opts import opts
    from model.networks.dla import DLASeg
    o = opts().parse(['tracking', '--dataset', 'fake', '--load_model', 'x', '--gpus', '-1', '--num_classes', '1', '--pre_hm'])
    opt = opts().update_dataset_info_and_set_heads(o, ref_import.FakeDataset)
    assert dict(opt.heads) == HEADS, opt.heads
    assert opt.pre_img and opt.pre_hm
    model = DLASeg(34, opt.heads, opt.head_conv, opt)
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(HERE, 'dlaseg_keys.json'), 'w') as f:
        json.dump(keys, f, indent=0)
        f.write('\n')
    print('dlaseg_keys.json: %d keys' % len(keys))


if __name__ == '__main__':
    main()
