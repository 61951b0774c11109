"""Host-side helpers every module of the package shares: the current stream as the C ABI takes it, the "device tensors only"
refusal, host lengths and int32 arrays for ctypes.  A leaf: torch, numpy and ctypes only, so that any module can import it."""
import ctypes as C

import numpy as np
import torch


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _require_cuda(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not x.is_cuda:
        raise RuntimeError("fastspeech2_amd runs on an MI355X only (no CPU fallback): %s is on %s" % (name, x.device))


def _lens(olens, B=None, name="olens"):
    L = torch.as_tensor(olens).detach().to("cpu", torch.int64).reshape(-1)
    if B is not None and L.numel() != B:
        raise ValueError("%s has %d entries for %d utterances" % (name, L.numel(), B))
    if (L < 0).any():
        raise ValueError("%s must be >= 0" % name)
    return L


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))
