"""The argument rules the data-path classes share (RealSequenceBatches, SyntheticBatches, CropAugment, CameraRoll,
AirPosePlusSequence) and, for the device, the metric classes behind _stream_metric.py: the refusals in `owner`'s name, worded once.
A class checks what every argument is first and where it lives last, so that a wrong argument is named as such on any machine.
"""
import operator

import torch


def cuda_device(owner, device):
    """the device of an object with no CPU path: a CUDA device, None = the current one (a given index constructs without a GPU)"""
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError("%s: device must be a CUDA (ROCm) device, got %s; there is no CPU path" % (owner, device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return device


def epoch_index(owner, epoch):
    """the epoch that counts the draws: an integer in 0 .. 2^31 - 1 -> int"""
    try:
        epoch = operator.index(epoch)
    except TypeError:
        raise RuntimeError("%s: epoch must be an integer, got %s" % (owner, type(epoch).__name__)) from None
    if not 0 <= epoch < 2 ** 31:
        raise RuntimeError("%s: epoch must be in 0 .. 2^31 - 1, got %r" % (owner, epoch))
    return epoch


def is_tensor(owner, t, name):
    if not torch.is_tensor(t):
        raise RuntimeError("%s: %s must be a tensor, got %s" % (owner, name, type(t).__name__))


def exact_tensor(owner, t, dtype, name):
    """a tensor of exactly `dtype`: nothing is cast (_stream_metric.check_what is the other rule: any floating type, cast)"""
    is_tensor(owner, t, name)
    if t.dtype != dtype:
        raise RuntimeError("%s: %s must be %s (nothing is cast), got %s" % (owner, name, str(dtype).replace("torch.", ""), t.dtype))


def lives_on(owner, t, dev, name, anchor):
    """where a tensor must live: on the GPU, on dev (None: any CUDA device), which is where `anchor` ("the batches") lives"""
    if not t.is_cuda:
        raise RuntimeError("%s: %s lives on %s; it must be a CUDA (ROCm) tensor, there is no CPU path" % (owner, name, t.device))
    if dev is not None and t.device != dev:
        raise RuntimeError("%s: %s lives on %s, %s on %s" % (owner, name, t.device, anchor, dev))


def pair_view(a, b):
    """a and b as ONE (2, ...) tensor without a copy where b lies right behind a in one allocation (the batch classes' views of
    their (2, n, ...) outputs), else None"""
    if not (a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device):
        return None
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr() or b.storage_offset() != a.storage_offset() + a.numel():
        return None
    return a.as_strided((2,) + tuple(a.shape), (a.numel(),) + tuple(a.stride()))
