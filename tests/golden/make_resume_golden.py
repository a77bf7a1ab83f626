"""Golden results of the resume branch of the reference's own ``load_model`` (src/lib/model/model.py:73-90; build
container only, like make_golden.py): tests/golden/resume.json.

A tiny model and a two-group Adam with state from one step; per case a checkpoint of some epoch, with or without its
``'optimizer'`` entry, loaded with ``opt.resume`` on or off against ``opt.lr_step``.  Recorded: what ``load_model``
returned as ``start_epoch``, every group's ``lr`` afterwards as ``float.hex`` (the reference multiplies by 0.1 once per
passed step, which is not ``lr * 0.1 ** k`` in floating point), and whether the optimizer's state was left alone.

    python tests/golden/make_resume_golden.py
"""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

ref_import.install()

import torch  # noqa: E402
from model.model import load_model  # noqa: E402  (the reference's)

LR = 1.25e-4
GROUP_LRS = (LR, 5e-4)
EPOCHS = (0, 59, 60, 61, 120)
LR_STEPS = ([60], [60, 120])


def tiny():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    optimizer = torch.optim.Adam([{'params': model[0].parameters(), 'lr': GROUP_LRS[0]},
                                  {'params': model[1].parameters(), 'lr': GROUP_LRS[1]}])
    model(torch.ones(4, 3)).sum().backward()
    optimizer.step()
    return model, optimizer


def state_bits(optimizer):
    return [[k, v.tolist()] for st in optimizer.state_dict()['state'].values() for k, v in sorted(st.items())]


def main():
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for epoch in EPOCHS:
            for lr_step in LR_STEPS:
                for has_opt in (True, False):
                    for resume in (True, False):
                        model, optimizer = tiny()
                        ckpt = {'epoch': epoch, 'state_dict': model.state_dict()}
                        if has_opt:
                            ckpt['optimizer'] = optimizer.state_dict()
                        path = os.path.join(tmp, 'ckpt.pth')
                        torch.save(ckpt, path)
                        before = state_bits(optimizer)
                        opt = types.SimpleNamespace(resume=resume, lr=LR, lr_step=lr_step, reset_hm=False, reuse_hm=False)
                        m, o, start = load_model(model, path, opt, optimizer)
                        assert m is model and o is optimizer
                        cases.append({'epoch': epoch, 'lr_step': lr_step, 'optimizer_in_checkpoint': has_opt,
                                      'resume': resume, 'start_epoch': int(start),
                                      'lr': [float(g['lr']).hex() for g in optimizer.param_groups],
                                      'state_untouched': state_bits(optimizer) == before})
    out = {'lr': LR, 'group_lrs': list(GROUP_LRS), 'cases': cases}
    with open(os.path.join(HERE, 'resume.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %d cases' % len(cases))


if __name__ == '__main__':
    main()
