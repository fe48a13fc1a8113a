"""What the wrappers of the native library share (encoders.py, model_ctc.py, transducer.py, lm.py): the life cycle of a native handle, the one
place a workspace is allocated, default lengths, the text of a rejected workspace query, the no-CPU-fallback error and the checkpoint plumbing
of the model classes.  Nothing here launches a kernel; everything but the device allocations runs without a GPU and without the library
(tests/test_native_host.py).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib


def workspace(nbytes: int, device) -> torch.Tensor:
    """A fresh workspace of `nbytes` bytes on `device`: every workspace the package hands to the library comes from here.  Test hook
    (include/effconf.h): the environment variable below, read at every call, holds the byte a fresh workspace is filled with - 255 = NaN
    patterns in fp32 / bf16 / fp16, 127 = huge finite values, 0 = zeros; a kernel that reads workspace nobody wrote shows up as a difference."""
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    fill = os.environ.get("EFFCONF_POISON_WORKSPACE", "")
    if fill:
        ws.fill_(int(fill))
    return ws


def lengths(x_len, batch: int, t: int, device) -> torch.Tensor:
    """The lengths a native call reads: int64, contiguous, on `device`; None = every one of the `batch` rows is `t` long.  A tensor that
    already is all of that comes back as the same object."""
    if x_len is None:
        x_len = torch.full((batch,), t, dtype=torch.int64, device=device)
    return torch.as_tensor(x_len).to(device=device, dtype=torch.int64).contiguous()


def sized(lib, entry_name: str, nbytes: int, **args) -> int:
    """`nbytes` as `<entry_name>_workspace_bytes` returned it for the sizes `args`, or - it returned 0: sizes outside what the entry takes -
    an EffconfError that names them (in the order given) with the library's reason."""
    nbytes = int(nbytes)
    if nbytes == 0:
        raise _lib.EffconfError("%s_workspace_bytes rejected (%s): %s" % (entry_name, ", ".join("%s %d" % kv for kv in args.items()),
                                                                          lib.effconf_last_error().decode()))
    return nbytes


def require_hip(t: torch.Tensor):
    """There is no CPU path: a tensor (an input, or the parameters) that is not on a HIP device is an error."""
    if not t.is_cuda:
        raise RuntimeError("efficientconformer_amd runs on a HIP device only (no CPU fallback)")


class Handle:
    """Owner of one native handle of the family `family` ("encoder", "rnnt", "lm": the entries effconf_<family>_create / _destroy /
    _load_tensor / _finalize).  ``ptr`` is the handle the other entries take, None before the first ``rebuild`` and after ``close``.
    `lib`: the library to call instead of libeffconf.so (tests)."""

    def __init__(self, family: str, lib=None):
        self._entry = "effconf_%s_%%s" % family
        self._what = "" if family == "encoder" else family + "_"      # how error texts name an entry: the encoder's carry no family name
        self._lib = lib
        self.ptr = None

    def rebuild(self, cfg, tensors: Iterable[Tuple[str, torch.Tensor]], before_load: Optional[Callable] = None):
        """A new handle for the config struct `cfg` in place of the current one: destroy, create, ``before_load(ptr)`` (what has to be set
        before the weights arrive), upload every (key, tensor) as contiguous host fp32 with its shape, finalize.  Raises EffconfError with the
        library's text at the first step that fails; ``ptr`` then is a handle that is not ready, which the next ``rebuild`` destroys."""
        self.close()
        lib = self._lib if self._lib is not None else _lib.load()
        ptr = getattr(lib, self._entry % "create")(C.byref(cfg))
        if not ptr:
            raise _lib.EffconfError("%s: %s" % (self._entry % "create", lib.effconf_last_error().decode()))
        self.ptr = ptr
        if before_load is not None:
            before_load(ptr)
        load_tensor = getattr(lib, self._entry % "load_tensor")
        for key, t in tensors:
            arr = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            _lib.check(load_tensor(ptr, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim), "%sload_tensor(%s)" % (self._what, key), lib)
        _lib.check(getattr(lib, self._entry % "finalize")(ptr), self._what + "finalize", lib)

    def close(self):
        """Destroy the handle, if there is one.  A handle exists only after the library was loaded; if the library is gone (interpreter exit),
        so is everything the handle owned."""
        lib = self._lib if self._lib is not None else _lib._lib
        if self.ptr is not None and lib is not None:
            getattr(lib, self._entry % "destroy")(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeModel(nn.Module):
    """Checkpoint plumbing of the model classes (ModelCTC, Transducer, LanguageModel): whatever replaces parameters also invalidates the packed
    native weights, through the subclass's ``_invalidate``."""

    def _invalidate(self):
        raise NotImplementedError

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        # strip the DDP / DataParallel infix first (model.py:367-370: "encoder.module.preprocessing.*" in a raw DDP state dict),
        # then drop torchaudio's frontend buffers (the native frontend builds its own window / filterbank tables)
        sd = {k.replace(".module.", "."): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if not k.startswith("encoder.preprocessing.")}
        r = super().load_state_dict(sd, strict=strict, **kw)
        self._invalidate()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def load(self, path):
        """Reference ``Model.load`` (model.py:361-384): a ``.ckpt`` path or dict; restores weights and the pickled tokenizer."""
        from .checkpoint import load_checkpoint
        return load_checkpoint(self, path)
