"""What every entry point does between its arguments and the ctypes call into libvap.so: pointers, the context on torch's
current stream, reusable output buffers, and host-or-device inputs as contiguous device tensors.  Private; shape checks
that are an entry point's own, and their messages, stay with the entry point."""
import ctypes as C

import numpy as np
import torch

from . import _lib

_NP_DTYPE = {torch.float64: np.float64, torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32}


def ptr(t):
    """A tensor's address for a ``void *`` argument; None stays None (the C-ABI's "not asked for")."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dptr(a):
    """A host fp64 array as ``const double *``; None or an empty array gives None."""
    return a.ctypes.data_as(_lib.dp) if a is not None and a.size else None


def context_for(dev, ctx):
    """``ctx``, or the device's shared context, put on torch's current stream of ``dev``."""
    if ctx is None:
        ctx = _lib.default_context(dev.index if dev.index is not None else torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return ctx


def buffers(out, shapes, dev):
    """``out`` (or a new dict) with a contiguous tensor on ``dev`` for every ``name: (shape, dtype)`` of ``shapes``: an
    entry that already fits is kept, any other is allocated; entries not named in ``shapes`` are left alone."""
    res = {} if out is None else out
    for k, (shp, dt) in shapes.items():
        t = res.get(k)
        if t is None or tuple(t.shape) != shp or t.dtype != dt or t.device != dev or not t.is_contiguous():
            res[k] = torch.empty(shp, dtype=dt, device=dev)
    return res


def device_array(a, dev, dtype):
    """``a`` as a contiguous tensor of ``dtype`` on ``dev``: a tensor is converted where it is needed, host data is
    uploaded once.  None stays None."""
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        t = a.to(device=dev, dtype=dtype)
    else:
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=_NP_DTYPE[dtype]), device=dev)
    return t.contiguous()


def time_rows(rows, counts, dev=None, device=0, what=None):
    """Time-domain rows and their counts as contiguous device tensors: (rows (B, cap, 8) fp64, counts (B, k) int32, single,
    device).  ``rows`` is a device tensor (used in place; it must be on ``dev`` if that is given) or a host array (uploaded
    to ``dev``, else to HIP device ``device``), (n, 8) for a single trajectory; ``counts`` is (B, k), (B,) or, for a single
    trajectory, None (all n rows).  ``what`` names the argument in the messages."""
    pre = "" if what is None else f"{what}: "
    if isinstance(rows, torch.Tensor):
        if rows.device.type != "cuda" or rows.dtype != torch.float64:
            raise ValueError(f"{pre}rows must be an fp64 tensor on a HIP device (or a host array)")
        if dev is not None and rows.device != dev:
            raise ValueError(f"{pre}rows are on {rows.device}, the other side on {dev}")
        dev = rows.device
    else:
        dev = dev if dev is not None else torch.device("cuda", device)
        rows = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64), device=dev)
    single = rows.dim() == 2
    if single:
        rows = rows.unsqueeze(0)
    if rows.dim() != 3 or rows.shape[2] != 8:
        raise ValueError(f"{pre}rows must be (B, capacity, 8) or (n, 8), got {tuple(rows.shape)}")
    rows = rows.contiguous()
    B = int(rows.shape[0])
    if counts is None:
        if not single:
            raise ValueError(f"{pre}counts is needed for a batch of rows")
        counts = torch.full((1, 1), int(rows.shape[1]), dtype=torch.int32, device=dev)
    else:
        counts = device_array(counts, dev, torch.int32)
    if counts.dim() < 2:
        counts = counts.reshape(B, 1)
    if counts.dim() != 2 or counts.shape[0] != B:
        raise ValueError(f"{pre}counts must be ({B}, k) or ({B},), got {tuple(counts.shape)}")
    return rows, counts, single, dev
