"""The optimizer step on the device: ``Adam`` and ``SGD`` as drop-ins for ``torch.optim.Adam`` /
``torch.optim.SGD`` -- the reference's two optimizers (src/main.py:17-26) -- whose ``step()`` updates every tensor of the
optimizer with ONE launch of ``ct_optim_step`` (csrc/optim.hip).

Both subclass the torch class and override ``step`` only: ``param_groups``, ``defaults``, ``zero_grad``,
``add_param_group``, ``state_dict`` / ``load_state_dict`` and the reference's ``param_group['lr'] = lr`` schedule are
torch's own, and the state is what torch creates (``step`` a float32 scalar tensor on the CPU, ``exp_avg``,
``exp_avg_sq`` / ``momentum_buffer``), so a checkpoint's ``'optimizer'`` entry crosses both ways.

``step()`` packs one record per tensor that has a gradient (``pack``) into a pinned block of the ``_staging`` ring,
enqueues one asynchronous copy and one launch on the current stream and records the block's event: no host wait.  The
bias corrections are formed on the host in double from each tensor's own integer step, as torch's non-capturable path
forms them; a parameter whose ``.grad`` is ``None`` is skipped and its step does not advance.  A ``step`` tensor found
on a device (``Trainer.set_device`` after ``load_state_dict``) is brought back to the CPU once: that one read waits.

No CPU fallback: parameters, gradients and state must be CUDA float32 contiguous dense tensors, and ``amsgrad``,
``maximize``, ``capturable``, ``differentiable``, ``decoupled_weight_decay``, ``nesterov``, ``dampening != 0`` and a
tensor ``lr`` are refused with ``CTError``.  ``foreach`` / ``fused`` choose between torch's implementations and mean
nothing here.

The guarded step: ``optimizer.guard(max_norm=..., skip_nonfinite=...)`` puts ``ct_optim_norms`` in
front of the update -- the global gradient norm, ``clip_grad_norm_``'s coefficient and a skip decision for gradients that
are not finite, all of which stay on the device -- and ``grad_stats()`` reads them back on request.

Data-parallel training: ``optimizer.distribute(group=None)`` puts ``ct_optim_pack_grads`` -- one launch
that gathers every gradient, scaled by 1 / world, into one flat buffer -- and ONE all-reduce of that buffer in front of the
unguarded or guarded step, which reads the averaged gradient through the same table.  ``reduced_grads()`` hands the
averaged gradients out, ``check_in_sync()`` compares the replicas on request.
"""
import numpy as np
import torch

from . import _lib, _staging
from ._lib import CTError

CHUNK = _lib.CT_OPTIM_CHUNK                      # elements a workgroup updates per round (csrc/optim.hip)
MAX_TENSORS = _lib.CT_OPTIM_MAX_TENSORS
KINDS = {'adam': _lib.CT_OPTIM_ADAM, 'sgd': _lib.CT_OPTIM_SGD}
# ct_optim_rec of include/centertrack_hip.h
REC = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('numel', '<i8'),
                ('s', '<f4', (_lib.CT_OPTIM_SCALARS,)), ('first', '<i4'), ('reserved', '<i4', (11,)), ('src', '<u8')])
REC_WORDS = REC.itemsize // 4
assert REC.itemsize == _lib.CT_OPTIM_REC_BYTES


def adam_scalars(step, lr, beta1, beta2, eps, weight_decay):
    """the seven scalars of an Adam record, in double (torch/optim/adam.py::_single_tensor_adam, non-capturable)"""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return (1 - beta1, beta2, 1 - beta2, lr / bias_correction1, bias_correction2 ** 0.5, eps, weight_decay)


def table_words(n):
    """int32 words of the table of ``n`` tensors: the records, then the chunk prefix"""
    return n * REC_WORDS + n + 1


def pack(kind, items, out=None, src=None):
    """The table ``ct_optim_step`` reads, as int32 words: ``len(items)`` records, then the prefix of chunk starts.
    ``items``: per tensor ``(p, g, m, v, numel, scalars, first)`` -- four device addresses (0: absent), the element
    count, up to eight Python floats and the SGD flag.  ``out``: an int32 numpy array to fill instead of a fresh one.
    ``src``: per tensor the device address ``ct_optim_pack_grads`` gathers ``g`` from (the record's last 8 bytes, which
    stay zero without it).  Returns ``(words array, n, chunks)``.  Pure host code."""
    if kind not in (_lib.CT_OPTIM_ADAM, _lib.CT_OPTIM_SGD):
        raise CTError('optim.pack: kind %r is neither CT_OPTIM_ADAM nor CT_OPTIM_SGD' % (kind,))
    n = len(items)
    if n < 1 or n > MAX_TENSORS:
        raise CTError('optim.pack: %d tensors outside [1, %d]' % (n, MAX_TENSORS))
    p, g, m, v, numel, scalars, first = zip(*items)
    rec = np.zeros(n, REC)
    rec['p'], rec['g'], rec['m'], rec['v'], rec['numel'], rec['first'] = p, g, m, v, numel, first
    s = np.asarray(scalars, np.float64)
    if s.ndim != 2 or s.shape[1] > _lib.CT_OPTIM_SCALARS:
        raise CTError('optim.pack: every tensor carries the same number (at most %d) of scalars' % _lib.CT_OPTIM_SCALARS)
    rec['s'][:, :s.shape[1]] = s                 # double -> float32, rounded to nearest
    null = (rec['p'] == 0) | (rec['g'] == 0)
    if kind == _lib.CT_OPTIM_ADAM:
        null |= (rec['m'] == 0) | (rec['v'] == 0)
    if null.any():
        raise CTError('optim.pack: null pointer in a record')
    if ((rec['p'] | rec['g'] | rec['m'] | rec['v']) & 3).any():
        raise CTError('optim.pack: a pointer that is not 4-byte aligned')
    if (rec['numel'] <= 0).any():
        raise CTError('optim.pack: a tensor without elements')
    if src is not None:
        if len(src) != n:
            raise CTError('optim.pack: %d source addresses for %d tensors' % (len(src), n))
        rec['src'] = src
        if (rec['src'] == 0).any():
            raise CTError('optim.pack: null source pointer in a record')
        if (rec['src'] & 3).any():
            raise CTError('optim.pack: a source pointer that is not 4-byte aligned')
    prefix = np.zeros(n + 1, np.int64)
    np.cumsum((rec['numel'] + (CHUNK - 1)) // CHUNK, out=prefix[1:])
    if prefix[-1] >= 1 << 31:
        raise CTError('optim.pack: %d chunks do not fit one launch' % prefix[-1])
    words = table_words(n)
    if out is None:
        out = np.empty(words, np.int32)
    elif out.dtype != np.int32 or out.ndim != 1 or out.size < words:
        raise CTError('optim.pack: out must be an int32 vector of at least %d words' % words)
    out[:n * REC_WORDS] = rec.view(np.int32)
    out[n * REC_WORDS:words] = prefix
    return out, n, int(prefix[-1])


def flat_layout(numels):
    """Where ``ct_optim_pack_grads`` puts the tensors of ``numels`` elements in the flat buffer: ``(offsets, total_elems)``,
    tensor ``t`` at element ``prefix[t] * CHUNK`` -- the chunk prefix of ``pack`` -- and ``total_elems = chunks * CHUNK``."""
    numels = np.asarray(numels, np.int64).reshape(-1)
    if numels.size < 1 or (numels <= 0).any():
        raise CTError('optim.flat_layout: every tensor has at least one element (got %s)' % (numels.tolist(),))
    prefix = np.zeros(numels.size + 1, np.int64)
    np.cumsum((numels + (CHUNK - 1)) // CHUNK, out=prefix[1:])
    return [int(c) * CHUNK for c in prefix[:-1]], int(prefix[-1]) * CHUNK


def reference_pack(grads, scale):
    """``ct_optim_pack_grads`` restated on the host, for the tests: the flat float32 numpy array that holds ``float32(g) *
    float32(scale)`` of every gradient at its ``flat_layout`` offset and +0.0 in the tail of every tensor's last chunk"""
    grads = [np.asarray(g, np.float32).reshape(-1) for g in grads]
    offsets, total = flat_layout([g.size for g in grads])
    flat = np.zeros(total, np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for off, g in zip(offsets, grads):
            flat[off:off + g.size] = g * np.float32(scale)
    return flat


def find_tensor(prefix, chunk):
    """the binary search of optim_step_kernel: the tensor t with prefix[t] <= chunk < prefix[t + 1]"""
    lo, hi = 0, len(prefix) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if prefix[mid] <= chunk:
            lo = mid
        else:
            hi = mid
    return lo


_FMA = {}


def _fma(a, b, c, fused):
    """``a * b + c`` on numpy arrays of one dtype: rounded once when ``fused`` (libm's fma / fmaf, element by element --
    sizes of a test), product and sum rounded separately otherwise"""
    if not fused:
        return a * b + c
    dtype = np.result_type(a, b, c)
    if dtype not in _FMA:
        import ctypes
        import ctypes.util
        libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
        fn, ct = (libm.fma, ctypes.c_double) if dtype == np.float64 else (libm.fmaf, ctypes.c_float)
        fn.restype, fn.argtypes = ct, [ct] * 3
        _FMA[dtype] = np.frompyfunc(fn, 3, 1)
    return _FMA[dtype](a, b, c).astype(dtype)


GUARD = np.dtype([('sumsq', '<f8'), ('norm', '<f8'), ('norm_sum', '<f8'), ('norm_max', '<f8'), ('nonfinite', '<i8'),
                  ('steps', '<i8'), ('skipped', '<i8'), ('clipped', '<i8'), ('nonfinite_steps', '<i8'), ('coef', '<f4'),
                  ('skip', '<i4')])                  # ct_optim_guard of include/centertrack_hip.h
GUARD_SLOT = 128                                 # bytes the guard takes in front of the per-tensor sums of its buffer
assert GUARD.itemsize <= GUARD_SLOT


def norms_workspace_bytes(n, chunks):
    """what ``ct_optim_norms_workspace_bytes`` answers, restated: 16 bytes per chunk and per tensor"""
    if n < 1 or n > MAX_TENSORS or chunks < n or chunks >= 1 << 31:
        return 0
    return 16 * (chunks + n)


def reference_guard(grads, max_norm=None, skip_nonfinite=False, dtype=np.float64, norm=None, eps=1e-6, clamp=True):
    """The rule of ``ct_optim_norms`` on numpy arrays, for the tests: ``grads`` are the gradients of one step (``None``
    entries are left out).  Returns ``sumsq`` (the squares added in float64, tensor by tensor), ``norm``, ``nonfinite``
    (elements that are NaN or +-Inf), ``skip`` and ``coef``: 1 when ``max_norm`` is ``None`` or <= 0 or a gradient is
    not finite, else ``c = max_norm / (norm + 1e-6)`` in double, clamped at 1 -- ``clip_grad_norm_``'s rule.  ``coef`` is
    a ``dtype`` value: the device's float32, or the double torch's float64 tensors are scaled by.  ``norm``: a total norm
    to use instead (torch's own, which adds in another order).  ``eps`` and ``clamp`` are the rule's two constants, there
    so that a test can show what fails without them."""
    grads = [np.asarray(g) for g in grads if g is not None]
    per = [float((g.astype(np.float64).ravel() ** 2).sum()) for g in grads]
    sumsq = 0.0
    for x in per:
        sumsq += x
    nonfinite = int(sum(int((~np.isfinite(g)).sum()) for g in grads))
    norm = float(np.sqrt(sumsq)) if norm is None else float(norm)
    coef = 1.0
    if max_norm is not None and max_norm > 0 and nonfinite == 0:
        with np.errstate(divide='ignore'):
            c = float(np.float64(max_norm) / np.float64(norm + eps))
        coef = c if (c < 1.0 or not clamp) else 1.0
    return dict(sumsq=sumsq, norm=norm, per_tensor=per, nonfinite=nonfinite, skip=bool(nonfinite > 0 and skip_nonfinite),
                coef=np.dtype(dtype).type(coef))


def reference_step(kind, p, g, state, hyper, fused=None, guard=None, zero_first=True):
    """One step of torch's single-tensor Adam / SGD (``foreach=False``) on numpy arrays, in ``p``'s dtype (float64 or
    float32), as torch's CPU kernels compute it: the scalars are formed in double and rounded to that dtype; the
    operations come in the kernels' order.  ``p`` and ``state`` (``{}`` before the first step; ``step`` an int) are
    updated in place.  ``hyper``: ``lr``, ``betas``, ``eps``, ``weight_decay`` / ``lr``, ``momentum``, ``weight_decay``.
    For the tests.

    Two things of those kernels are not plain IEEE operation by operation.  ``fused`` (default: whether torch dispatches
    to its AVX2 / AVX-512 kernels on this CPU): ``add(alpha)``, ``lerp`` and ``addcmul`` round their last product and sum
    once there (a fused multiply-add).  And the square root is torch's own: its vectorised CPU square root is not
    correctly rounded (it differs from numpy's in 0.7% of float64 values), so no restatement reproduces it.
    The device kernel (csrc/optim.hip) fuses nothing, rounds division and square root correctly and forms
    ``-step_size (m / denom)`` where the CPU kernel forms ``(-step_size m) / denom``.

    ``guard``: what ``reference_guard`` returned for this step's gradients.  ``g * coef`` (one product in ``p``'s dtype)
    takes the place of ``g``; under ``skip`` nothing moves, but Adam's ``step`` still advances (the host cannot know of
    the skip) and an SGD momentum buffer this step was to create is created as zeros (``zero_first``; the next step's
    ``momentum * 0 + g`` is then torch's first step)."""
    if fused is None:
        fused = torch.backends.cpu.get_cpu_capability() != 'DEFAULT'
    dt = p.dtype.type
    g = np.asarray(g, p.dtype)
    if guard is not None:
        if guard['skip']:
            if kind == 'adam':
                if not state:
                    state.update(step=0, exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
                state['step'] += 1
            elif kind == 'sgd':
                if hyper.get('momentum', 0) != 0 and 'momentum_buffer' not in state and zero_first:
                    state['momentum_buffer'] = np.zeros_like(p)
            else:
                raise CTError('optim.reference_step: kind %r is neither "adam" nor "sgd"' % (kind,))
            return
        g = g * dt(guard['coef'])
    wd = hyper.get('weight_decay', 0)
    if kind == 'adam':
        if not state:
            state.update(step=0, exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
        state['step'] += 1
        b1, b2 = hyper.get('betas', (0.9, 0.999))
        omb1, b2, omb2, step_size, bc2_sqrt, eps, wd = (
            dt(x) for x in adam_scalars(state['step'], hyper['lr'], b1, b2, hyper.get('eps', 1e-8), wd))
        if wd != 0:
            g = _fma(p, wd, g, fused)
        m, v = state['exp_avg'], state['exp_avg_sq']
        m[...] = _fma(omb1, g - m, m, fused)
        v *= b2
        v[...] = _fma(omb2 * g, g, v, fused)
        denom = torch.from_numpy(np.ascontiguousarray(v)).sqrt().numpy() / bc2_sqrt + eps
        p += (-step_size * m) / denom
    elif kind == 'sgd':
        lr, mom, wd = dt(hyper['lr']), dt(hyper.get('momentum', 0)), dt(wd)
        if wd != 0:
            g = _fma(p, wd, g, fused)
        if mom != 0:
            if 'momentum_buffer' not in state:
                state['momentum_buffer'] = np.array(g, copy=True)
            else:
                buf = state['momentum_buffer']
                buf *= mom
                buf += g
            g = state['momentum_buffer']
        p[...] = _fma(g, -lr, p, fused)
    else:
        raise CTError('optim.reference_step: kind %r is neither "adam" nor "sgd"' % (kind,))


def _check_tensor(t, like, what, who):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided
            and t.is_contiguous()):
        got = '%s %s %s' % (t.device, t.dtype, t.layout) if torch.is_tensor(t) else type(t).__name__
        raise CTError('%s: %s must be a CUDA float32 contiguous dense tensor (got %s); no CPU fallback' % (who, what, got))
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise CTError('%s: %s of shape %s on %s for a parameter of shape %s on %s'
                      % (who, what, tuple(t.shape), t.device, tuple(like.shape), like.device))


class _FusedStep(object):
    """what ``Adam`` and ``SGD`` share: the refusals and the launch"""
    _kind = None
    _refused = ()                                # group keys that must be falsy

    def _check_group(self, group):
        who = type(self).__name__
        for k in self._refused:
            if group.get(k):
                raise CTError('centertrack_amd.optim.%s: %s=%r is not supported' % (who, k, group[k]))
        if torch.is_tensor(group['lr']):
            raise CTError('centertrack_amd.optim.%s: a tensor lr is not supported (a Python float is)' % who)

    # What step() knows about a parameter from its last visit: [p address, numel, device, the state tensors (identity),
    # their addresses, (Adam) the step tensor, its version counter and its value as an int].  A visit re-reads the
    # parameter's address and compares the state tensors by identity; anything else -- first visit, ``p.data = ...``,
    # ``load_state_dict``, ``Trainer.set_device`` -- goes through the full checks of ``_admit`` again.
    def _gradient(self, p):
        g = p.grad
        if g is not None and (g.layout is not torch.strided or not g.is_contiguous()):
            raise CTError('centertrack_amd.optim.%s: a gradient must be a contiguous dense tensor (got %s, strides %s); '
                          'no CPU fallback' % (type(self).__name__, g.layout, g.stride() if g.layout is torch.strided else '-'))
        return g

    def _advance(self, visited):
        """``step += 1`` for every visited tensor in one call, as torch's float32 scalars on the CPU"""
        if visited:
            torch._foreach_add_([c[5] for c in visited], 1)
            for c in visited:
                c[6] = c[5]._version

    def guard(self, max_norm=None, skip_nonfinite=False):
        """Put the device-side guard in front of every later ``step()``; returns ``self``.

        ``max_norm`` > 0: the gradients are scaled by ``torch.nn.utils.clip_grad_norm_``'s coefficient ``min(1, max_norm /
        (norm + 1e-6))`` over all tensors of the optimizer that have a gradient (2-norm; the coefficient is formed in
        double and applied as one float32 product inside the update).  ``skip_nonfinite``: a step whose gradients hold a
        NaN or an Inf changes no parameter and no state.  ``guard()`` with both off restores the unguarded ``step()``.

        A guarded ``step()`` enqueues one copy and three launches and still waits for nothing; its buffers are allocated
        once and grown on demand.  What differs from torch: ``p.grad`` is NOT scaled in place (``clip_grad_norm_``
        does that), and the host counts every ``step()`` call, also one the device skips -- it cannot know of the skip
        without waiting -- so ``state['step']`` and ``state_dict`` advance as torch's do and the bias correction after
        a skipped step is one step ahead.  (``GradScaler`` differs there: it does not call ``step``.)  All parameters
        must be on one device.  ``grad_stats()`` reads the outcome."""
        max_norm = 0.0 if max_norm is None else float(max_norm)
        if max_norm != max_norm:
            raise CTError('centertrack_amd.optim.%s.guard: max_norm is NaN' % type(self).__name__)
        on = max_norm > 0 or bool(skip_nonfinite)
        self.__dict__['_guard'] = (max_norm if max_norm > 0 else 0.0, bool(skip_nonfinite)) if on else None
        return self

    def _guard_buffers(self, device, n, chunks, words):
        """the table, the guard with the per-tensor sums behind it and the workspace of a guarded step: kept, grown by
        doubling (the guard's counters move along)"""
        b = self.__dict__.setdefault('_gbufs', {'device': device, 'table': None, 'state': None, 'work': None, 'cap': 0,
                                                'n': 0, 'last': None})
        if b['device'] != device:
            raise CTError('centertrack_amd.optim.%s: a guarded step takes the parameters of one device (got %s and %s)'
                          % (type(self).__name__, b['device'], device))

        def grown(have, need):
            cap = max(have, 1024)
            while cap < need:
                cap *= 2
            return cap
        if b['table'] is None or b['table'].numel() < words:
            b['table'] = torch.empty(grown(0 if b['table'] is None else b['table'].numel(), words), dtype=torch.int32,
                                     device=device)
        if b['state'] is None or b['cap'] < n:
            cap = grown(b['cap'], n)
            state = torch.zeros(GUARD_SLOT + 8 * cap, dtype=torch.uint8, device=device)
            if b['state'] is not None:
                state[:GUARD_SLOT].copy_(b['state'][:GUARD_SLOT])
            b['state'], b['cap'] = state, cap
        need = norms_workspace_bytes(n, chunks)
        if b['work'] is None or b['work'].numel() < need:
            b['work'] = torch.empty(grown(0 if b['work'] is None else b['work'].numel(), need), dtype=torch.uint8,
                                    device=device)
        b['n'] = n
        return b

    def _launch_guarded(self, per_device, guard):
        from . import ops
        if len(per_device) > 1:
            raise CTError('centertrack_amd.optim.%s: a guarded step takes the parameters of one device (got %s)'
                          % (type(self).__name__, sorted(str(d) for d in per_device)))
        ring = self.__dict__.setdefault('_ring', [])
        for device, items in per_device.items():
            words = table_words(len(items))
            entry = _staging.take(ring, words, torch.int32)
            _, n, chunks = pack(self._kind, items, out=entry['host'].numpy())
            with torch.cuda.device(device):
                b = self._guard_buffers(device, n, chunks, words)
                stream = torch.cuda.current_stream()
                if b['last'] is not None and b['last'][0] != stream.cuda_stream:
                    stream.wait_event(b['last'][1])          # (the buffers are shared between steps: keep them in order)
                b['table'][:words].copy_(entry['host'][:words], non_blocking=True)
                ops.optim_norms(b['table'], n, chunks, guard[0], guard[1], b['state'][GUARD_SLOT:], b['state'], b['work'])
                ops.optim_step_guarded(b['table'], n, chunks, self._kind, b['state'])
                entry['event'].record()
                b['last'] = (stream.cuda_stream, entry['event'])

    def guard_counters(self):
        """the guard's running ``[norm_sum, steps, skipped, clipped, nonfinite_steps]`` as a float64 DEVICE tensor (no
        wait), or ``None`` before the first guarded step"""
        b = self.__dict__.get('_gbufs')
        if self.__dict__.get('_guard') is None or b is None or b['state'] is None:
            return None
        st = b['state']
        return torch.cat([st[16:24].view(torch.float64), st[40:72].view(torch.int64).double()])

    def grad_stats(self):
        """What the last guarded ``step()`` found, read from the device (the one call of the guard that waits): ``norm``,
        ``sumsq``, ``nonfinite``, ``coef``, ``skip`` of that step; the running ``steps``, ``skipped``, ``clipped``,
        ``nonfinite_steps``, ``norm_max`` and ``norm_mean`` (over the steps whose gradients were finite); ``per_tensor``,
        the norm of every tensor that had a gradient in that step, in the optimizer's order."""
        b = self.__dict__.get('_gbufs')
        if b is None or b['state'] is None:
            raise CTError('centertrack_amd.optim.%s.grad_stats: no guarded step has run' % type(self).__name__)
        host = b['state'][:GUARD_SLOT + 8 * b['n']].cpu().numpy()
        g = host[:GUARD.itemsize].view(GUARD)[0]
        out = {k: (float(g[k]) if GUARD[k].kind == 'f' else int(g[k])) for k in GUARD.names if k != 'norm_sum'}
        out['skip'] = bool(out['skip'])
        finite = out['steps'] - out['nonfinite_steps']
        out['norm_mean'] = float(g['norm_sum']) / finite if finite else 0.0
        out['per_tensor'] = np.sqrt(host[GUARD_SLOT:].view(np.float64))
        return out

    def distribute(self, group=None):
        """Data-parallel training, one process per GPU: every later ``step()`` averages the gradients
        over the ranks of ``group`` (``None``: the default group of ``torch.distributed``; a group of one rank is allowed)
        before it updates; returns ``self``.  ``distribute(False)`` restores the local ``step()``.

        A distributed ``step()`` takes the parameters of one device.  It uploads one table, as before, in which every
        record's gradient pointer leads into ONE flat buffer (``flat_layout``; kept, grown by doubling) and ``src`` to
        ``p.grad``; ``ct_optim_pack_grads`` gathers ``p.grad * float32(1 / world)`` there in one launch, one ``all_reduce(SUM)``
        (``parallel.all_reduce_flat``) exchanges the buffer, and the unguarded or guarded step runs on the same table.
        With a guard, norm, clip coefficient and skip decision are formed from the averaged gradient and are therefore the
        same on every rank; a NaN or Inf on one rank reaches every rank through the sum, so all ranks skip together.
        Under ``nccl`` the collective is enqueued on the device and the host waits for nothing; under ``gloo`` the buffer
        goes through a pinned host block and the host WAITS -- that path is there so that tests and boxes without RCCL run
        the same code.  ``p.grad`` is not written (the rule of the guard); ``reduced_grads()`` hands out the averaged
        gradients.

        The tensors that carry a gradient are fixed by the first distributed step: there the ranks compare a hash of
        their element counts and raise on every rank if they differ, and a later step with another list raises
        ``CTError`` on its rank before any collective."""
        if group is False:
            self.__dict__['_dist'] = None
            return self
        from . import parallel
        if not parallel.group_active():
            raise CTError('centertrack_amd.optim.%s.distribute: no torch.distributed process group (start one process per '
                          'GPU with torchrun and call parallel.init_from_env first)' % type(self).__name__)
        self.__dict__['_dist'] = {'group': group, 'layout': None, 'flat': None, 'device': None, 'last': None}
        return self

    def _check_layout(self, per_device):
        """a distributed step: one device, and the element counts the first such step fixed (compared across ranks there)"""
        d = self.__dict__.get('_dist')
        if d is None:
            return
        who = 'centertrack_amd.optim.%s' % type(self).__name__
        if len(per_device) != 1:
            raise CTError('%s: a distributed step takes the gradients of one device (got %s)'
                          % (who, sorted(str(dev) for dev in per_device) or 'no gradient at all'))
        numels = tuple(it[4] for items in per_device.values() for it in items)
        if d['layout'] is None:
            from . import parallel
            parallel.check_same_digest(','.join(str(v) for v in numels), 'the list of tensors that carry a gradient',
                                       d['group'])
            d['layout'] = numels
            d['offsets'], d['total'] = flat_layout(numels)
        elif numels != d['layout']:
            raise CTError('%s: the tensors that carry a gradient changed after the first distributed step (%d tensors, %d '
                          'elements then; %d tensors, %d elements now): the layout of the reduced buffer is fixed'
                          % (who, len(d['layout']), sum(d['layout']), len(numels), sum(numels)))

    def _launch_distributed(self, per_device, d):
        from . import ops, parallel
        guard = self.__dict__.get('_guard')
        ring = self.__dict__.setdefault('_ring', [])
        (device, items), = per_device.items()
        offsets, total = d['offsets'], d['total']
        with torch.cuda.device(device):
            if d['flat'] is None or d['device'] != device or d['flat'].numel() < total:
                cap = max(d['flat'].numel() if d['flat'] is not None and d['device'] == device else 0, 1 << 16)
                while cap < total:
                    cap *= 2
                d['flat'], d['device'] = torch.zeros(cap, dtype=torch.float32, device=device), device
            flat, base = d['flat'][:total], d['flat'].data_ptr()
            words = table_words(len(items))
            entry = _staging.take(ring, words, torch.int32)
            _, n, chunks = pack(self._kind, [it[:1] + (base + 4 * off,) + it[2:] for it, off in zip(items, offsets)],
                                out=entry['host'].numpy(), src=[it[1] for it in items])
            stream = torch.cuda.current_stream()
            if d['last'] is not None and d['last'][0] != stream.cuda_stream:
                stream.wait_event(d['last'][1])              # (the flat buffer is shared between steps: keep them in order)
            if guard is not None:
                b = self._guard_buffers(device, n, chunks, words)
                if b['last'] is not None and b['last'][0] != stream.cuda_stream:
                    stream.wait_event(b['last'][1])
                table = b['table']
            else:
                table = torch.empty(words, dtype=torch.int32, device=device)
            table[:words].copy_(entry['host'][:words], non_blocking=True)
            world = parallel.world_size(d['group'])
            ops.optim_pack_grads(table, n, chunks, np.float32(1.0 / world))
            parallel.all_reduce_flat(flat, d['group'])
            if guard is not None:
                ops.optim_norms(table, n, chunks, guard[0], guard[1], b['state'][GUARD_SLOT:], b['state'], b['work'])
                ops.optim_step_guarded(table, n, chunks, self._kind, b['state'])
            else:
                ops.optim_step(table, n, chunks, self._kind)
            entry['event'].record()
            d['last'] = (stream.cuda_stream, entry['event'])
            if guard is not None:
                b['last'] = d['last']

    def _grad_params(self):
        return [p for group in self.param_groups for p in group['params'] if p.grad is not None and p.numel() > 0]

    def reduced_grads(self):
        """The gradients the last distributed ``step()`` applied -- averaged over the ranks, before the guard's clipping --
        as views into the flat buffer: one per parameter in the optimizer's order, in the parameter's shape, ``None`` for
        a parameter without a gradient.  Valid until the next ``step()``; no wait."""
        d = self.__dict__.get('_dist')
        if d is None or d['flat'] is None or d['layout'] is None:
            raise CTError('centertrack_amd.optim.%s.reduced_grads: no distributed step has run' % type(self).__name__)
        with_grad = self._grad_params()
        if tuple(p.numel() for p in with_grad) != d['layout']:
            raise CTError('centertrack_amd.optim.%s.reduced_grads: the gradients are not those of the last distributed step'
                          % type(self).__name__)
        views = {p: d['flat'][off:off + p.numel()].view(p.shape) for p, off in zip(with_grad, d['offsets'])}
        return [views.get(p) for group in self.param_groups for p in group['params']]

    def check_in_sync(self):
        """Compare the parameters across the ranks on request: every rank forms a checksum of its parameters' bits, the
        checksums are all-gathered, and ``CTError`` is raised on every rank, naming the ranks that differ from rank 0.
        A read that WAITS."""
        d = self.__dict__.get('_dist')
        if d is None:
            raise CTError('centertrack_amd.optim.%s.check_in_sync: distribute() is off' % type(self).__name__)
        from . import parallel
        params = [p for group in self.param_groups for p in group['params'] if p.numel() > 0]
        with torch.no_grad():
            sums = torch.stack([p.detach().contiguous().view(torch.int32).to(torch.int64).sum() for p in params])
            weights = torch.arange(1, len(params) + 1, dtype=torch.int64, device=sums.device)
            mine = torch.stack([sums.sum(), (sums * weights).sum()])     # (int64 wraps: a checksum)
        bad = parallel.ranks_that_differ(mine, d['group'])
        if bad:
            raise CTError('centertrack_amd.optim.%s.check_in_sync: the parameters of rank(s) %s differ from those of rank 0'
                          % (type(self).__name__, bad))

    def _launch(self, per_device):
        from . import ops
        d = self.__dict__.get('_dist')
        if d is not None:
            return self._launch_distributed(per_device, d)
        guard = self.__dict__.get('_guard')
        if guard is not None:
            return self._launch_guarded(per_device, guard)
        ring = self.__dict__.setdefault('_ring', [])
        for device, items in per_device.items():
            words = table_words(len(items))
            entry = _staging.take(ring, words, torch.int32)
            _, n, chunks = pack(self._kind, items, out=entry['host'].numpy())
            with torch.cuda.device(device):
                table = torch.empty(words, dtype=torch.int32, device=device)
                table.copy_(entry['host'][:words], non_blocking=True)
                ops.optim_step(table, n, chunks, self._kind)
                entry['event'].record()

    @staticmethod
    def _closure(closure):
        if closure is None:
            return None
        with torch.enable_grad():
            return closure()


class Adam(_FusedStep, torch.optim.Adam):
    """``torch.optim.Adam`` with the step on ``ct_optim_step``"""
    _kind = _lib.CT_OPTIM_ADAM
    _refused = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        for k, v in (('amsgrad', amsgrad), ('maximize', maximize), ('capturable', capturable),
                     ('differentiable', differentiable), ('decoupled_weight_decay', decoupled_weight_decay)):
            if v:
                raise CTError('centertrack_amd.optim.Adam: %s=%r is not supported' % (k, v))
        if torch.is_tensor(lr):
            raise CTError('centertrack_amd.optim.Adam: a tensor lr is not supported (a Python float is)')
        torch.optim.Adam.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                  foreach=foreach, maximize=maximize, capturable=capturable,
                                  differentiable=differentiable, fused=fused,
                                  decoupled_weight_decay=decoupled_weight_decay)

    def _admit(self, p, g, state):
        who = 'centertrack_amd.optim.Adam'
        _check_tensor(p, None, 'a parameter', who)
        _check_tensor(g, p, 'a gradient', who)
        if p.numel() == 0:
            return None
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        m, v, st = state['exp_avg'], state['exp_avg_sq'], state['step']
        _check_tensor(m, p, 'exp_avg', who)
        _check_tensor(v, p, 'exp_avg_sq', who)
        if st.device.type != 'cpu':                  # (one read that waits; torch keeps this scalar on the CPU)
            st = state['step'] = st.cpu()
        return [p.data_ptr(), p.numel(), p.device, m, v, st, st._version, int(st), m.data_ptr(), v.data_ptr()]

    @torch.no_grad()
    def step(self, closure=None):
        loss = self._closure(closure)
        cache = self.__dict__.setdefault('_cache', {})
        per_device, visited = {}, []
        try:
            for group in self.param_groups:
                self._check_group(group)
                beta1, beta2 = group['betas']
                if torch.is_tensor(beta1) or torch.is_tensor(beta2):
                    raise CTError('centertrack_amd.optim.Adam: tensor betas are not supported')
                lr, eps, wd = group['lr'], group['eps'], group['weight_decay']
                scalars = {}
                for p in group['params']:
                    g = self._gradient(p)
                    if g is None:
                        continue
                    c, state, ptr = cache.get(p), self.state[p], p.data_ptr()
                    if (c is None or c[0] != ptr or state.get('exp_avg') is not c[3] or state.get('exp_avg_sq') is not c[4]
                            or state.get('step') is not c[5] or c[5]._version != c[6]):
                        c = cache[p] = self._admit(p, g, state)
                        if c is None:
                            continue
                    t = c[7] = c[7] + 1
                    visited.append(c)
                    if t not in scalars:
                        scalars[t] = adam_scalars(t, lr, beta1, beta2, eps, wd)
                    per_device.setdefault(c[2], []).append((c[0], g.data_ptr(), c[8], c[9], c[1], scalars[t], 0))
            self._check_layout(per_device)
            self._advance(visited)
        except BaseException:
            cache.clear()
            raise
        self._launch(per_device)
        return loss


class SGD(_FusedStep, torch.optim.SGD):
    """``torch.optim.SGD`` (momentum, weight decay) with the step on ``ct_optim_step``"""
    _kind = _lib.CT_OPTIM_SGD
    _refused = ('nesterov', 'dampening', 'maximize', 'differentiable')

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        for k, v in (('nesterov', nesterov), ('dampening', dampening), ('maximize', maximize),
                     ('differentiable', differentiable)):
            if v:
                raise CTError('centertrack_amd.optim.SGD: %s=%r is not supported' % (k, v))
        if torch.is_tensor(lr) or torch.is_tensor(weight_decay):
            raise CTError('centertrack_amd.optim.SGD: a tensor lr / weight_decay is not supported (a Python float is)')
        torch.optim.SGD.__init__(self, params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                 nesterov=nesterov, maximize=maximize, foreach=foreach, differentiable=differentiable,
                                 fused=fused)

    def _admit(self, p, g, state, momentum):
        who = 'centertrack_amd.optim.SGD'
        _check_tensor(p, None, 'a parameter', who)
        _check_tensor(g, p, 'a gradient', who)
        if p.numel() == 0:
            return None
        buf, first = None, 0
        if momentum != 0:
            buf = state.get('momentum_buffer')
            if buf is None:
                buf = state['momentum_buffer'] = torch.empty_like(p, memory_format=torch.preserve_format)
                first = 1                            # the kernel writes it: buf = grad
            _check_tensor(buf, p, 'momentum_buffer', who)
        return [p.data_ptr(), p.numel(), p.device, buf, buf.data_ptr() if buf is not None else 0, first]

    @torch.no_grad()
    def step(self, closure=None):
        loss = self._closure(closure)
        cache = self.__dict__.setdefault('_cache', {})
        per_device = {}
        try:
            for group in self.param_groups:
                self._check_group(group)
                lr, momentum, wd = group['lr'], group['momentum'], group['weight_decay']
                if torch.is_tensor(wd):
                    raise CTError('centertrack_amd.optim.SGD: a tensor weight_decay is not supported')
                scalars = (lr, momentum, wd)
                for p in group['params']:
                    g = self._gradient(p)
                    if g is None:
                        continue
                    c, ptr = cache.get(p), p.data_ptr()
                    # (torch keeps no state at all without momentum: self.state[p] is not touched then)
                    buf = self.state[p].get('momentum_buffer') if momentum != 0 else None
                    if c is None or c[0] != ptr or buf is not c[3] or buf is None and momentum != 0:
                        c = cache[p] = self._admit(p, g, self.state[p] if momentum != 0 else None, momentum)
                        if c is None:
                            continue
                    per_device.setdefault(c[2], []).append((c[0], g.data_ptr(), c[4], 0, c[1], scalars, c[5]))
                    c[5] = 0
            self._check_layout(per_device)
        except BaseException:
            cache.clear()
            raise
        self._launch(per_device)
        return loss


_NORM_RING = []


def grad_norms(params):
    """The 2-norm of the gradients of ``params`` (parameters with a ``.grad``, or the gradient tensors themselves) by
    ``ct_optim_norms``, without an optimizer: ``(total, per_tensor)``, a float64 scalar and a float64 vector on the
    device, in the order given; parameters without a gradient are left out.  No host wait."""
    from . import ops
    grads = []
    for t in params:
        g = t.grad if getattr(t, 'grad', None) is not None or getattr(t, 'requires_grad', False) else t
        if g is None or g.numel() == 0:
            continue
        _check_tensor(g, None, 'a gradient', 'centertrack_amd.optim.grad_norms')
        if grads and g.device != grads[0].device:
            raise CTError('centertrack_amd.optim.grad_norms: gradients on %s and %s' % (grads[0].device, g.device))
        grads.append(g.detach())
    if not grads:
        raise CTError('centertrack_amd.optim.grad_norms: no gradient')
    device = grads[0].device
    items = [(g.data_ptr(), g.data_ptr(), 0, 0, g.numel(), (0.0, 0.0, 0.0), 0) for g in grads]   # (p is never read)
    words = table_words(len(items))
    entry = _staging.take(_NORM_RING, words, torch.int32)
    _, n, chunks = pack(_lib.CT_OPTIM_SGD, items, out=entry['host'].numpy())
    with torch.cuda.device(device):
        table = torch.empty(words, dtype=torch.int32, device=device)
        table.copy_(entry['host'][:words], non_blocking=True)
        state = torch.zeros(GUARD_SLOT + 8 * n, dtype=torch.uint8, device=device)
        work = torch.empty(norms_workspace_bytes(n, chunks), dtype=torch.uint8, device=device)
        ops.optim_norms(table, n, chunks, 0.0, False, state[GUARD_SLOT:], state, work)
        entry['event'].record()
    return state[8:16].view(torch.float64)[0], state[GUARD_SLOT:].view(torch.float64).sqrt()


def guard_options(opt):
    """``(max_norm or None, skip_nonfinite)`` from ``opt.max_grad_norm`` / ``opt.skip_nonfinite``, both optional"""
    max_norm = getattr(opt, 'max_grad_norm', None)
    if max_norm is not None and not max_norm > 0:
        max_norm = None
    return max_norm, bool(getattr(opt, 'skip_nonfinite', False))


def get_optimizer(opt, model):
    """the reference's src/main.py:17-26 with the classes above; ``opt.max_grad_norm`` / ``opt.skip_nonfinite``, where an
    ``opt`` has them, switch the guard on"""
    if opt.optim == 'adam':
        optimizer = Adam(model.parameters(), opt.lr)
    elif opt.optim == 'sgd':
        print('Using SGD')
        optimizer = SGD(model.parameters(), opt.lr, momentum=0.9, weight_decay=0.0001)
    else:
        assert 0, opt.optim
    max_norm, skip_nonfinite = guard_options(opt)
    if max_norm is not None or skip_nonfinite:
        optimizer.guard(max_norm, skip_nonfinite)
    return optimizer
