"""centertrack_amd: MI355X-native (gfx950) CenterTrack per-frame inference hot path.

Host code is Python on PyTorch-ROCm (device memory, streams, torch.distributed);
all device compute is hand-written HIP behind the C ABI declared in
``include/centertrack_hip.h`` (``centertrack_amd/csrc`` -> ``libcentertrack_hip.so``).
Importing the package does not load the HIP library; the first op call does, and
fails loudly if it is missing (there is no CPU fallback).

Training: ``dla_seg`` / ``losses`` run a training step on these kernels and ``targets.TargetBuilder``
builds the step's targets (heat maps and slot tensors) on the device from per-sample object lists;
``inputs.InputBuilder`` builds its images (warp, flip, colour augmentation, normalisation) on the device from raw u8 frames.
"""
__version__ = '0.1.0'
