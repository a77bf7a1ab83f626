"""Records tests/golden/plan_launches.json: the structure of the launch plan DLASegHIP builds for every configuration
of tests/test_hip_plan_structure.py (launch names, plan signature, outputs, sparse heads, conv and fused-heads
descriptors).  Needs an MI355X (a plan allocates its buffers on the device).  Run it on the tree whose plans are the
truth -- it was recorded on the one-function plan builder, before that was split into stages.

    python tests/golden/make_plan_golden.py [output.json]
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

os.environ['CENTERTRACK_AUTOTUNE'] = '0'         # fixed DCN knobs, algo 0: read at every plan build

import test_hip_plan_structure as T  # noqa: E402
from centertrack_amd import model as M  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, T.GOLDEN_FILE)
    device = torch.device('cuda:0')
    rec = {}
    for cfg in T.CONFIGS:
        M.FUSE_PROJ = cfg['fuse_proj']
        rec[cfg['name']] = T.summarize(*T.build_plan(cfg, device))
        print('%-20s %d launches' % (cfg['name'], len(rec[cfg['name']]['launches'])))
    with open(out, 'w') as f:
        f.write('{\n%s\n}\n' % ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(rec[k], sort_keys=True)) for k in sorted(rec)))


if __name__ == '__main__':
    main()
