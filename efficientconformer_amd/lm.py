"""LSTM language model (reference models/lm.py:33-81 with configs/LM-RNN.json): scoring of token sequences and the one-token decode step on
the GPU (csrc/lm.hip), for n-best rescoring of the CTC beam search (``ModelCTC.rescore_nbest``).

Keeps the reference's attribute names and state-dict keys (``decoder.embedding``, ``decoder.rnn``, ``fc``) and its ``decode(x, hidden)`` /
``forward(batch)`` signatures; the modules are parameter containers, never executed in Python.  For a sequence y of U tokens (ids 1 .. V - 1) the
LM reads x = [0, y_0 .. y_{U-1}] (lm.py:71 prepends the blank) and ``token_logprobs`` returns log_softmax(fc(h_u) / lm_tmp)[y_u] for u < U,
``score`` their sum.  Only ``arch == "RNN"`` is native: the reference's Transformer LM block does not run as shipped.
Training (``forward`` with gradients, the cross-entropy loss) is out of scope.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib, _native, _targets
from .config import load_config
from .transducer import RnnDecoder

# One call's workspace stays under this many bytes: the class splits the sequences into chunks (multiples of 64, at least 64) whose (h, c)
# state - 12 * num_layers * dim_model bytes per sequence - fits.  LM-RNN (4096 x 3): 147 KiB per sequence, 4096 sequences = 576 MiB per call.
WORKSPACE_CAP = 1 << 30


class LanguageModel(_native.NativeModel):

    def __init__(self, lm_params: dict, tokenizer_params: Optional[dict] = None, training_params: Optional[dict] = None,
                 decoding_params: Optional[dict] = None, name: Optional[str] = None, tokenizer=None):
        super().__init__()
        if lm_params.get("arch", "RNN") != "RNN":
            if lm_params.get("arch") == "Transformer":
                raise NotImplementedError("native language model: arch 'RNN' (configs/LM-RNN.json); the reference's Transformer LM does not run as shipped")
            raise Exception("Unknown model architecture:", lm_params.get("arch"))
        vocab = int(lm_params["vocab_size"])
        if tokenizer_params is not None and int(tokenizer_params.get("vocab_size", vocab)) != vocab:
            raise ValueError("lm_params['vocab_size'] = %d but tokenizer_params['vocab_size'] = %d" % (vocab, tokenizer_params["vocab_size"]))
        self.decoder = RnnDecoder(lm_params)
        self.fc = nn.Linear(int(lm_params["dim_model"]), vocab)
        decoding_params = decoding_params or {}
        self.lm_tmp = float(decoding_params.get("lm_tmp", 1))                        # model.py:72
        self._cfg = (vocab, int(lm_params["dim_model"]), int(lm_params["num_layers"]))
        self.tokenizer = tokenizer
        self.name = name
        self._native = _native.Handle("lm")
        self._packed = False
        self.eval()

    @classmethod
    def from_config(cls, cfg, tokenizer=None):
        cfg = load_config(cfg)
        return cls(cfg["lm_params"], cfg.get("tokenizer_params"), cfg.get("training_params"), cfg.get("decoding_params"),
                   cfg.get("model_name"), tokenizer)

    def _invalidate(self):
        self._packed = False

    # ------------------------------------------------------------------ native handle
    @property
    def _handle(self):
        """The native LM handle (None before the first pack); ``self._native`` owns it."""
        return self._native.ptr

    def _ensure(self):
        if self._packed:
            return
        self._native.rebuild(_lib.EcLmConfig(*self._cfg), self.state_dict().items())
        self._packed = True

    def _device(self):
        _native.require_hip(self.fc.weight)
        return self.fc.weight.device

    def chunk_size(self) -> int:
        """Sequences per native call: the largest multiple of 64 whose workspace stays under ``WORKSPACE_CAP`` (at least 64)."""
        _, h, layers = self._cfg
        return max(64, WORKSPACE_CAP // (12 * layers * h) // 64 * 64)

    # ------------------------------------------------------------------ scoring
    def token_logprobs(self, y, y_len=None, lm_tmp: Optional[float] = None):
        """log P(y_u | y_0 .. y_{u-1}) of every token: `y` a padded (N, U) integer tensor (+ `y_len`), a list of id lists, or a list of strings
        when a tokenizer is attached -> (token_logp (N, U) f32, status (N,) i32) on the device.  token_logp is 0 at or beyond a sequence's
        length.  status 2: a token outside 1 .. vocab - 1 or a length outside 0 .. U - the whole row is -inf, the other rows are untouched."""
        out = self._score(y, y_len, lm_tmp, True)
        return out[0], out[2]

    def score(self, y, y_len=None, lm_tmp: Optional[float] = None) -> torch.Tensor:
        """log P(y) of every sequence, (N,) f32 on the device: the fp32 sum of ``token_logprobs`` in ascending position; 0 for an empty
        sequence, -inf where ``token_logprobs`` reports status 2."""
        return self._score(y, y_len, lm_tmp, False)[1]

    def _score(self, y, y_len, lm_tmp, want_tokens):
        tmp = float(self.lm_tmp if lm_tmp is None else lm_tmp)
        if not 0 < tmp < float("inf"):
            raise _lib.EffconfError("lm_tmp must be > 0; got %r" % (tmp,))
        dev = y.device if isinstance(y, torch.Tensor) and y.is_cuda else self._device()
        tg, tl = _targets.targets(self.tokenizer, y, y_len, dev)
        n, u = int(tg.shape[0]), int(tg.shape[1])
        if tl.shape[0] != n:
            raise _lib.EffconfError("lengths: %d entries for %d sequences" % (tl.shape[0], n))
        # longest first (a device sort, no synchronisation): the sequences that finish early share column tiles, which the step and head kernels
        # skip once every sequence of a tile is done; a sequence's results do not depend on where it sits
        order = torch.argsort(tl, descending=True, stable=True)
        tg, tl = tg[order].contiguous(), tl[order].contiguous()
        token_logp = torch.empty(n, u, dtype=torch.float32, device=dev) if want_tokens else None
        score = torch.empty(n, dtype=torch.float32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        step = self.chunk_size()
        with torch.cuda.device(dev):
            self._ensure()
            lib = _lib.load()
            for lo in range(0, n, step):
                m = min(step, n - lo)
                ws = _native.workspace(_native.sized(lib, "effconf_lm", lib.effconf_lm_workspace_bytes(self._handle, m, u), n=m, U=u), dev)
                _lib.check(lib.effconf_lm_score(self._handle, tg[lo:].data_ptr(), tl[lo:].data_ptr(), m, u, tmp,
                                                token_logp[lo:].data_ptr() if want_tokens else None, score[lo:].data_ptr(), status[lo:].data_ptr(),
                                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "lm_score")
        inv = torch.empty_like(order)
        inv[order] = torch.arange(n, device=dev)
        return token_logp[inv] if want_tokens else None, score[inv], status[inv]

    # ------------------------------------------------------------------ the reference's step and forward
    def decode(self, x: torch.Tensor, hidden=None):
        """Reference signature (lm.py:55-63): x (N, 1) token ids, hidden = (h, c) of shape (num_layers, N, dim_model) or None (zeros) ->
        (logits (N, 1, V): the raw fc outputs, no temperature; (h', c'))."""
        _native.require_hip(x)
        if x.dim() != 2 or x.shape[1] != 1:
            raise _lib.EffconfError("decode takes one token per sequence, x of shape (N, 1); got %s" % (tuple(x.shape),))
        dev = x.device
        vocab, h, layers = self._cfg
        n = int(x.shape[0])
        if n > self.chunk_size():
            raise _lib.EffconfError("decode: at most %d sequences per call (WORKSPACE_CAP)" % self.chunk_size())
        tok = x.reshape(n).to(torch.int32).contiguous()
        hin = cin = None
        if hidden is not None:
            hin, cin = (t.to(device=dev, dtype=torch.float32).contiguous() for t in hidden)
            if tuple(hin.shape) != (layers, n, h) or tuple(cin.shape) != (layers, n, h):
                raise _lib.EffconfError("hidden must be (h, c) of shape (%d, %d, %d); got %s, %s" % (layers, n, h, tuple(hin.shape), tuple(cin.shape)))
        logits = torch.empty(n, 1, vocab, dtype=torch.float32, device=dev)
        hout = torch.empty(layers, n, h, dtype=torch.float32, device=dev)
        cout = torch.empty(layers, n, h, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self._ensure()
            lib = _lib.load()
            ws = _native.workspace(lib.effconf_lm_workspace_bytes(self._handle, n, 0), dev)
            _lib.check(lib.effconf_lm_step(self._handle, tok.data_ptr(), None if hin is None else hin.data_ptr(), None if cin is None else cin.data_ptr(),
                                           n, logits.data_ptr(), hout.data_ptr(), cout.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(dev).cuda_stream), "lm_step")
        return logits, (hout, cout)

    def forward(self, batch):
        """Reference ``forward`` (lm.py:65-81), eval mode: batch = (x (B, U) ids, x_len or None, y ignored) -> logits (B, U + 1, V) of the inputs
        [0, x_0 .. x_{U-1}], through ``decode`` steps.  Rows at or beyond x_len + 1 are fc's bias, as the reference's padded LSTM output (zeros)
        gives them."""
        x, x_len, _ = batch
        _native.require_hip(x)
        b, u = x.shape
        xp = torch.nn.functional.pad(x.to(torch.int32), pad=(1, 0, 0, 0), value=0)
        out = torch.empty(b, u + 1, self._cfg[0], dtype=torch.float32, device=x.device)
        hidden = None
        for k in range(u + 1):
            logits, hidden = self.decode(xp[:, k:k + 1].clamp(0, self._cfg[0] - 1), hidden)
            out[:, k] = logits[:, 0]
        if x_len is not None:
            beyond = torch.arange(u + 1, device=x.device)[None, :] >= (x_len.to(x.device) + 1)[:, None]
            out[beyond] = self.fc.bias.detach().to(out.device, torch.float32)
        return out
