"""The reference's training loop (src/lib/trainer.py:89-189) around this package's modules, without its per-iteration host
waits.

``Trainer(opt, model, optimizer)`` with ``set_device``, ``train`` / ``val`` / ``run_epoch`` returning the reference's
``(ret, results)``: ``ret[l]`` the batch-size-weighted average of ``loss_stats[l].mean()`` for ``'tot'`` and every head
with ``opt.weights[l] > 0``, and ``ret['time']`` in minutes.  The reference reads every loss statistic back with
``.item()`` on every iteration; here the sums stay on the device -- float64, ``sum += val * n`` in the reference's order, so
the averages are the ``AverageMeter``'s to the bit -- and the host reads them every ``opt.print_iter`` iterations (when
> 0) and once at the end of the epoch.  The model is any ``model(image, pre_img, pre_hm) -> [ {head: logits} ]`` of this
package (``dla_seg.DLASeg``, ``heads.HeadFinetuner``), the loss is ``losses.GenericLoss``, the optimizer either
``centertrack_amd.optim``'s or torch's.

``opt.max_grad_norm`` / ``opt.skip_nonfinite`` (both optional attributes) switch on the optimizer's device-side guard
(``optim.Adam.guard``).  With a guard on, the ``print_iter`` line carries the epoch's mean gradient
norm, the closing line the number of skipped steps as well, and ``ret`` gains ``'grad_norm'`` and ``'skipped'``; they
come in the same device read as the loss sums, so the loop waits no more often.  With the guard off nothing changes.

More than one GPU: one process per GPU under torchrun, each with a full replica.  With a process
group active (``parallel.init_from_env``), ``set_device`` broadcasts rank 0's module and calls ``optimizer.distribute()``,
after which every ``step()`` averages the gradients over the ranks with one all-reduce; ``set_device(gpus, ..)`` accepts
``len(gpus) > 1`` when it equals the group's world size, ``device`` being this rank's.  The loss sums and the sample count
are added over the ranks at the reads above (no additional read), so ``ret`` is the global average and equal on every
rank; rank 0 prints; after a train epoch the buffers (the BatchNorm running statistics) are broadcast from rank 0, so its
checkpoint holds what ``DataParallel`` keeps.  BatchNorm stays per replica by default, and the caller shards the data
(``DistributedSampler``, ``batch_size / world`` samples per rank).

``opt.sync_bn`` (an optional attribute): with a process group active ``set_device`` marks the model
with ``parallel.sync_batchnorm``, after which every training-mode BatchNorm takes its statistics over the batches of all
ranks, forward and backward, as ``torch.nn.SyncBatchNorm`` does.  The running statistics are then the same bits on every
rank, so the broadcast of rank 0's buffers after a train epoch is skipped; ``check_in_sync()`` compares parameters and
buffers across the ranks on request.

Not covered: single-process ``DataParallel`` (``chunk_sizes`` is ignored), gradient accumulation, overlapping the
collectives with the backward, ``opt.debug > 0`` (the reference's drawing), the progress bar (a plain line is printed instead).
"""
import time

import torch

from . import dcn_v2, parallel
from ._lib import CTError
from .losses import GenericLoss
from .optim import guard_options

LOSS_ORDER = ('hm', 'wh', 'reg', 'ltrb', 'hps', 'hm_hp', 'hp_offset', 'dep', 'dim', 'rot', 'amodel_offset', 'ltrb_amodal',
              'tracking', 'nuscenes_att', 'velocity')


class ModelWithLoss(torch.nn.Module):
    """the reference's ``ModleWithLoss``: ``forward(batch) -> (outputs[-1], loss, loss_stats)``"""

    def __init__(self, model, loss):
        super().__init__()
        self.model = model
        self.loss = loss

    def forward(self, batch):
        pre_img = batch['pre_img'] if 'pre_img' in batch else None
        pre_hm = batch['pre_hm'] if 'pre_hm' in batch else None
        if getattr(self.model, 'slot_heads', False):              # (heads.FusedHeads: regression heads at batch['ind'] only)
            outputs = self.model(batch['image'], pre_img, pre_hm, batch['ind'])
        else:
            outputs = self.model(batch['image'], pre_img, pre_hm)
        loss, loss_stats = self.loss(outputs, batch)
        return outputs[-1], loss, loss_stats


class Trainer(object):
    def __init__(self, opt, model, optimizer=None):
        self._refuse_debug(opt)
        self.opt = opt
        self.optimizer = optimizer
        max_norm, skip_nonfinite = guard_options(opt)
        if optimizer is not None and (max_norm is not None or skip_nonfinite):
            if not hasattr(optimizer, 'guard'):
                raise CTError('centertrack_amd.trainer.Trainer: opt.max_grad_norm / opt.skip_nonfinite need an optimizer of '
                              'centertrack_amd.optim (got %s)' % type(optimizer).__name__)
            optimizer.guard(max_norm, skip_nonfinite)
        self.loss_stats, self.loss = self._get_losses(opt)
        self.model_with_loss = ModelWithLoss(model, self.loss)
        self.device = getattr(opt, 'device', None)

    @staticmethod
    def _refuse_debug(opt):
        if getattr(opt, 'debug', 0) > 0:
            raise CTError('centertrack_amd.trainer.Trainer: opt.debug = %r is not supported (the reference draws its '
                          'detections there)' % (opt.debug,))

    def set_device(self, gpus, chunk_sizes, device):
        world = parallel.world_size()
        if len(gpus) > 1 and not parallel.group_active():
            raise CTError('centertrack_amd.trainer.Trainer runs on one GPU per process (gpus = %s): single-process '
                          'DataParallel is not covered; start one process per GPU with torchrun and call '
                          'parallel.init_from_env() first' % (list(gpus),))
        if len(gpus) > 1 and len(gpus) != world:
            raise CTError('centertrack_amd.trainer.Trainer: gpus = %s inside a process group of %d ranks (one rank per GPU)'
                          % (list(gpus), world))
        if world > 1 and self.optimizer is not None and not hasattr(self.optimizer, 'distribute'):
            raise CTError('centertrack_amd.trainer.Trainer: training on %d ranks needs an optimizer of '
                          'centertrack_amd.optim (got %s, which does not exchange gradients)'
                          % (world, type(self.optimizer).__name__))
        self.device = device
        self.model_with_loss = self.model_with_loss.to(device)
        if self.optimizer is not None:
            for state in self.optimizer.state.values():
                for k, v in state.items():
                    if isinstance(v, torch.Tensor):
                        state[k] = v.to(device=device, non_blocking=True)
        if parallel.group_active():                          # one replica per rank: start from rank 0's, exchange gradients
            parallel.broadcast_module(self.model_with_loss, src=0)
            if hasattr(self.optimizer, 'distribute'):
                self.optimizer.distribute()
            if getattr(self.opt, 'sync_bn', False):          # BatchNorm statistics over the batches of all ranks
                parallel.sync_batchnorm(self.model_with_loss.model)

    def sync_bn(self):
        """is the model's BatchNorm synchronised: ``opt.sync_bn`` with a process group active"""
        return bool(getattr(self.opt, 'sync_bn', False)) and parallel.group_active()

    def check_in_sync(self):
        """Compare the replicas on request: the parameters (``optimizer.check_in_sync``) and the buffers -- the BatchNorm
        running statistics and counters -- of every rank against rank 0's; raises on EVERY rank, naming the ranks that
        differ.  A read that WAITS.  The buffers agree after a train epoch (the broadcast) or, with ``opt.sync_bn``, always."""
        if hasattr(self.optimizer, 'check_in_sync'):
            self.optimizer.check_in_sync()
        try:
            parallel.check_buffers_in_sync(self.model_with_loss)
        except RuntimeError as e:
            raise CTError(str(e))

    def _get_losses(self, opt):
        loss_states = ['tot'] + [k for k in LOSS_ORDER if k in opt.heads]
        return loss_states, GenericLoss(opt)

    def run_epoch(self, phase, epoch, data_loader):
        opt = self.opt
        self._refuse_debug(opt)
        train = phase == 'train'
        if train and self.optimizer is None:
            raise CTError('centertrack_amd.trainer.Trainer: the train phase needs an optimizer')
        model_with_loss = self.model_with_loss
        if train:
            model_with_loss.train()
        else:
            model_with_loss.eval()
            torch.cuda.empty_cache()
        device = self.device
        results = {}
        names = [l for l in self.loss_stats if l == 'tot' or opt.weights[l] > 0]
        num_iters = len(data_loader) if opt.num_iters < 0 else opt.num_iters
        print_iter = getattr(opt, 'print_iter', 0)
        title = '{}/{}'.format(getattr(opt, 'task', ''), getattr(opt, 'exp_id', ''))
        sums, count, done = None, 0, 0
        start = time.time()
        # the optimizer's guard, when it is on: its running counters at the start of the epoch, on the device
        counters = getattr(self.optimizer, 'guard_counters', None) if train else None
        guarded = counters is not None and getattr(self.optimizer, '_guard', None) is not None
        base = counters() if guarded else None
        # one process per GPU: the sums and the count are added over the ranks at every read, and rank 0 prints
        spread = parallel.group_active()
        chatty = not spread or torch.distributed.get_rank() == 0

        def line(host_sums, count, guard=None, closing=False):
            text = '{}| {}: [{}][{}/{}]|Tot: {:.1f}s '.format(title, phase, epoch, done, num_iters, time.time() - start)
            for l, s in zip(names, host_sums):
                text += '|{} {:.4f} '.format(l, s / count if count else 0.0)
            if guard is not None:
                text += '|grad_norm {:.4f} '.format(guard[0])
                if closing:
                    text += '|skipped {} '.format(guard[1])
            return text

        def over_ranks():
            """the loss sums with the sample count behind them, added over the ranks (a device tensor under nccl)"""
            mine = sums if sums is not None else torch.zeros(len(names), dtype=torch.float64, device=device)
            return parallel.reduce_sums(torch.cat([mine, torch.tensor([count], dtype=torch.float64, device=mine.device)]))

        def read():
            """the loss sums of this epoch in ONE device read: (sums, count) -- over all ranks when there are several"""
            if spread:
                host = over_ranks().cpu().tolist()
                return host[:-1], int(host[-1])
            return (sums.cpu().tolist() if sums is not None else [0.0] * len(names)), count

        def read_guarded():
            """the loss sums and the guard's counters of this epoch in ONE device read: (sums, count, (mean norm, skipped));
            the counters come from the averaged gradient and are the same on every rank"""
            cur = counters()
            if cur is None or sums is None:
                return read() + ((0.0, 0),)
            cur = cur if base is None else cur - base
            if spread:
                host = torch.cat([over_ranks().to(cur.device), cur]).cpu().tolist()
                host_sums, n = host[:len(names)], int(host[len(names)])
            else:
                host = torch.cat([sums, cur]).cpu().tolist()
                host_sums, n = host[:len(names)], count
            norm_sum, steps, skipped, _, nonfinite_steps = host[-5:]
            finite = steps - nonfinite_steps
            return host_sums, n, (norm_sum / finite if finite else 0.0, int(skipped))

        with dcn_v2.trainable(train or dcn_v2.is_trainable()):
            for iter_id, batch in enumerate(data_loader):
                if iter_id >= num_iters:
                    break
                for k in batch:
                    if k != 'meta':
                        batch[k] = batch[k].to(device=device, non_blocking=True)
                output, loss, loss_stats = model_with_loss(batch)
                loss = loss.mean()
                if train:
                    self.optimizer.zero_grad()
                    loss.backward()
                    self.optimizer.step()
                # AverageMeter.update(val, n) for every statistic at once, on the device: sum += val * n in double
                n = batch['image'].size(0)
                vals = torch.stack([loss_stats[l].detach().mean().double() for l in names])
                sums = vals * n if sums is None else sums + vals * n
                count += n
                done = iter_id + 1
                if print_iter > 0 and iter_id % print_iter == 0:
                    text = line(*(read_guarded() if guarded else read()))  # the only per-iteration read, on request
                    if chatty:
                        print(text)
                del output, loss, loss_stats
        guard = None
        if guarded:
            host_sums, total, guard = read_guarded()
        else:
            host_sums, total = read()                                     # waits for the epoch's last launch
        ret = {l: (s / total if total else 0) for l, s in zip(names, host_sums)}
        if guarded:
            ret['grad_norm'], ret['skipped'] = guard
        ret['time'] = (time.time() - start) / 60.
        if chatty:
            print(line(host_sums, total, guard, closing=True))
        if train and spread and not self.sync_bn():
            # rank 0's checkpoint holds what DataParallel keeps: replica 0's running statistics.  (Under synchronised BatchNorm
            # every rank moved its buffers with the same merged statistics: they are equal already.  That rests on EVERY
            # BatchNorm of the model going through ``_train.bn_statistics`` under ``dcn_v2.trainable()`` on every rank, which
            # the train phase above guarantees for this package's modules; a BatchNorm that runs on torch instead -- the stems
            # of a first width other than 16 -- keeps per-rank statistics, and ``check_in_sync()`` is how to find out.)
            parallel.broadcast_module(model_with_loss, src=0, parameters=False)
        return ret, results

    def val(self, epoch, data_loader):
        return self.run_epoch('val', epoch, data_loader)

    def train(self, epoch, data_loader):
        return self.run_epoch('train', epoch, data_loader)
