"""The pinned staging ring of ``TargetBuilder.render`` and ``InputBuilder.render``: a list of ``{'host': pinned tensor,
'event': torch.cuda.Event}``.  A call packs into an entry, enqueues the copy and records the entry's event; the next call
takes an entry only when its event answers "finished" (``event.query()`` only asks -- never a wait), else a new one."""


def take(ring, count, dtype, floor=4096):
    """an entry of ``ring`` (changed in place) whose pinned ``host`` tensor holds at least ``count`` elements of
    ``dtype`` and that no call in flight still reads; idle entries that are too small are dropped"""
    import torch
    for e in ring:
        if e['host'].numel() >= count and e['event'].query():
            return e
    ring[:] = [e for e in ring if not (e['host'].numel() < count and e['event'].query())]
    cap = floor
    while cap < count:
        cap *= 2
    e = {'host': torch.empty(cap, dtype=dtype).pin_memory(), 'event': torch.cuda.Event()}
    ring.append(e)
    return e
