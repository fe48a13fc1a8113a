"""Token-sequence arguments shared by ModelCTC, Transducer and LanguageModel: strings, id lists or a padded tensor -> device tensors."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def ids(tokenizer, y):
    """Strings -> id lists through the tokenizer; anything else as it is."""
    if not isinstance(y, torch.Tensor) and len(y) and isinstance(y[0], str):
        if tokenizer is None:
            raise _lib.EffconfError("string targets need a tokenizer (tokenizer.encode)")
        return [tokenizer.encode(r) for r in y]
    return y


def targets(tokenizer, y, y_len, device):
    """(targets (B, U) i32, target_len (B,) i64) on `device` from a padded integer tensor + lengths, a list of id lists, or a list of
    strings (needs a tokenizer).  A list is padded on the host and copied once."""
    if isinstance(y, torch.Tensor):
        if y.dim() != 2:
            raise _lib.EffconfError("targets must be (batch, tokens); got shape %s" % (tuple(y.shape),))
        tg = y.to(device=device, dtype=torch.int32).contiguous()
        if y_len is None:
            y_len = torch.full((y.shape[0],), y.shape[1], dtype=torch.int64)
        return tg, torch.as_tensor(y_len).to(device=device, dtype=torch.int64).contiguous()
    rows = [[int(c) for c in r] for r in ids(tokenizer, y)]
    lens = [len(r) for r in rows] if y_len is None else [int(v) for v in (y_len.tolist() if hasattr(y_len, "tolist") else y_len)]
    host = np.zeros((len(rows), max([len(r) for r in rows] + [0])), dtype=np.int32)
    for i, r in enumerate(rows):
        host[i, :len(r)] = r
    return torch.from_numpy(host).to(device), torch.tensor(lens, dtype=torch.int64).to(device)
