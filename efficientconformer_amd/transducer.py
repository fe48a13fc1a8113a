"""Transducer (RNN-T) wrapper: encoder + prediction network + joint network with greedy decoding on the GPU
(reference models/transducer.py:52-186, models/decoders.py:41-70, models/joint_networks.py:33-104).

Keeps the reference's attribute names (``encoder``, ``decoder.embedding``, ``decoder.rnn``, ``joint_network.linear_*``),
state-dict keys and method names (``gready_search_decoding``, the reference's spelling).  The per-utterance Python loop
of the reference — one decoder call, one joint call and one ``.argmax()`` host sync per decision — runs as one
persistent HIP kernel per batch (effconf_rnnt_greedy).  ``beam_search_decoding`` (transducer.py:188-327) runs as one persistent
HIP kernel per batch as well (effconf_rnnt_beam, one workgroup per utterance), with the reference's algorithm, tie rules and fp32
scores.  With a ``LanguageModel`` attached as ``lm`` (or passed) and ``lm_weight`` > 0 the search adds the reference's neural-LM shallow
fusion term (transducer.py:259-273: ``lm_weight * (lm.decode(y, hidden_lm) / lm_tmp).softmax().log()`` before the top-k; effconf_rnnt_beam_lm:
the search kernel and one chip-wide LM step over every utterance's pending hypotheses alternate).  The n-gram (KenLM) terms are not
implemented.  For a KNOWN transcript, ``lattice`` gives the two log-probabilities per (t, u) cell the RNN-T loss sees
(csrc/rnnt_lattice.hip: the (B, T, U + 1, V) logits of transducer.py:88-107 never reach memory), ``score_labels`` log P(y | x) = -rnnt_loss
and ``align`` the frame at which each token is emitted (csrc/rnnt_align.hip: forward recursion and Viterbi over the lattice).  ``open_stream`` / ``open_decode_stream`` decode
streams push by push from a carried prediction-network state (effconf_rnnt_greedy_resume), with the tokens of the whole-utterance greedy decode.  Training
(``forward`` with gradients, the RNN-T loss' backward) is out of scope (HISTORY.md).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _native, _targets
from .config import load_config
from .encoders import ConformerEncoder

# One call's workspace of the fused beam search stays under this many bytes where more than one utterance is decoded: per utterance the LM nodes
# take (2 * beam + max_expansions + 64) * (2 * num_layers * dim_model + vocab) * 4 bytes (LM-RNN 4096 x 3 at beam 16: 36 MB, 256 utterances 9.2 GB).
BEAM_LM_WORKSPACE_CAP = 16 << 30

_JOINT_MODES = {"sum": 0}
_JOINT_ACTS = {"tanh": 0}


class TransducerAlignment(NamedTuple):
    """Forced alignment of one utterance (``Transducer.align``): token u is emitted at encoder frame frame[u], i.e. at second time[u]
    (frame x ``ConformerEncoder.frame_seconds``); token_logp[u] is its log-probability at that lattice cell, ``score`` the log-probability
    of the whole best path (its blanks included), ``log_likelihood`` log P(tokens | audio) over all paths.  status: 0 ok, 1 tokens but no
    frames, 2 a token id outside 1 .. vocab - 1 (then frame is -1 and both scores -inf)."""
    tokens: List[int]
    frame: List[int]
    time: List[float]
    token_logp: List[float]
    score: float
    log_likelihood: float
    status: int


class RnnDecoder(nn.Module):
    """Parameter container with the reference's key names (decoders.py:46-47); never executed in Python."""

    def __init__(self, params: dict):
        super().__init__()
        self.embedding = nn.Embedding(params["vocab_size"], params["dim_model"], padding_idx=0)
        self.rnn = nn.LSTM(input_size=params["dim_model"], hidden_size=params["dim_model"], num_layers=params["num_layers"],
                           batch_first=True, bidirectional=False)


class JointNetwork(nn.Module):
    """Parameter container with the reference's key names (joint_networks.py:41-52)."""

    def __init__(self, dim_encoder: int, dim_decoder: int, vocab_size: int, params: dict):
        super().__init__()
        assert params["act"] in ["tanh", "relu", "swish", None]
        assert params["joint_mode"] in ["concat", "sum"]
        if params.get("dim_model") is None or params["joint_mode"] not in _JOINT_MODES or params["act"] not in _JOINT_ACTS:
            raise NotImplementedError("native joint network: joint_mode 'sum', act 'tanh', dim_model set "
                                      "(every shipped Transducer config); got %r" % (params,))
        self.linear_encoder = nn.Linear(dim_encoder, params["dim_model"])
        self.linear_decoder = nn.Linear(dim_decoder, params["dim_model"])
        self.linear_joint = nn.Linear(params["dim_model"], vocab_size)
        self.joint_mode, self.act_name = params["joint_mode"], params["act"]


class Transducer(_native.NativeModel):

    def __init__(self, encoder_params: dict, decoder_params: dict, joint_params: dict, tokenizer_params: Optional[dict] = None,
                 training_params: Optional[dict] = None, decoding_params: Optional[dict] = None, name: str = "model",
                 tokenizer=None):
        super().__init__()
        if encoder_params.get("arch", "Conformer") != "Conformer":
            raise Exception("Unknown encoder architecture:", encoder_params.get("arch"))
        if decoder_params.get("arch", "RNN") != "RNN":
            raise NotImplementedError("native prediction network: arch 'RNN' (every shipped Transducer config)")
        self.encoder = ConformerEncoder(encoder_params)
        self.decoder = RnnDecoder(decoder_params)
        self.joint_network = JointNetwork(self.encoder.plan.dim_out, decoder_params["dim_model"], decoder_params["vocab_size"],
                                          joint_params)
        self.max_consec_dec_step = decoder_params.get("max_consec_dec_step", 5)      # transducer.py:83
        decoding_params = decoding_params or {}
        self.beam_size = int(decoding_params.get("beam_size", 1))                    # model.py:60-61
        self.tmp = float(decoding_params.get("tmp", 1))
        # the reference's attribute and decoding_params (model.py:70-72): a LanguageModel attached by the caller, fused into the beam search.  Assigning
        # one registers it as a submodule, as in the reference: state_dict() then carries its tensors under ``lm.``
        self.lm = None
        self.lm_weight = float(decoding_params.get("lm_weight", 0))
        self.lm_tmp = float(decoding_params.get("lm_tmp", 1))
        self._cfg = (self.encoder.plan.dim_out, decoder_params["dim_model"], joint_params["dim_model"],
                     decoder_params["vocab_size"], decoder_params["num_layers"])
        self.tokenizer = tokenizer
        self.name = name
        self._native = _native.Handle("rnnt")
        self._rnnt_packed = False
        self._rnnt_generation = 0                # counts the native handle's rebuilds: what a decode stream was opened on
        self._beam_ws = None
        self._beam_rounds = None
        self.eval()

    @classmethod
    def from_config(cls, cfg, tokenizer=None):
        cfg = load_config(cfg)
        return cls(cfg["encoder_params"], cfg["decoder_params"], cfg["joint_params"], cfg.get("tokenizer_params"),
                   cfg.get("training_params"), cfg.get("decoding_params"), cfg.get("model_name", "model"), tokenizer)

    def _invalidate(self):
        self.encoder.repack()
        self._rnnt_packed = False

    def forward(self, batch):
        raise NotImplementedError("Transducer.forward returns the (B, T, U+1, V) training logits (transducer.py:88-107): training is out of "
                                  "scope of the native inference path; lattice() gives the per-cell blank / label log-probabilities of a "
                                  "transcript, score_labels() its log-likelihood, align() its token frames")

    # ------------------------------------------------------------------ native handle
    @property
    def _rnnt(self):
        """The native decoder handle (None before the first pack); ``self._native`` owns it."""
        return self._native.ptr

    def _ensure_rnnt(self):
        if self._rnnt_packed:
            return
        de, h, j, v, layers = self._cfg
        cfg = _lib.EcRnntConfig(de, h, j, v, layers, int(self.max_consec_dec_step), _JOINT_MODES[self.joint_network.joint_mode],
                                _JOINT_ACTS[self.joint_network.act_name])
        self._native.rebuild(cfg, [(prefix + key, t) for prefix, mod in (("decoder.", self.decoder), ("joint_network.", self.joint_network))
                                   for key, t in mod.state_dict().items()])
        self._rnnt_packed = True
        self._rnnt_generation += 1

    def set_decode_option(self, name: str, value: int):
        """Forward an option to the native decoder (effconf_rnnt_set_option), e.g. ``cluster_decode`` = -1 auto / 0 / 1."""
        self._ensure_rnnt()
        _lib.check(_lib.load().effconf_rnnt_set_option(self._rnnt, name.encode(), int(value)), "rnnt_set_option(%s)" % name)

    # ------------------------------------------------------------------ decoding
    def decode_encoded(self, f: torch.Tensor, f_len: Optional[torch.Tensor]):
        """Greedy RNN-T decode of encoder outputs f (B, T, Denc) fp32 on the GPU -> (tokens (B, max_tok) i32, token_len (B) i32)."""
        _native.require_hip(f)
        with torch.cuda.device(f.device):             # the C library allocates / launches on the current device
            return self._decode_encoded(f, f_len)

    def _decode_encoded(self, f: torch.Tensor, f_len: Optional[torch.Tensor]):
        self._ensure_rnnt()
        lib = _lib.load()
        f = f.contiguous().float()
        b, t, _ = f.shape
        f_len = _native.lengths(f_len, b, t, f.device)
        max_tok = int(lib.effconf_rnnt_max_tokens(self._rnnt, t))
        tokens = torch.empty(b, max_tok, dtype=torch.int32, device=f.device)
        token_len = torch.empty(b, dtype=torch.int32, device=f.device)
        ws = _native.workspace(lib.effconf_rnnt_workspace_bytes(self._rnnt, b, t), f.device)
        _lib.check(lib.effconf_rnnt_greedy(self._rnnt, f.data_ptr(), f_len.data_ptr(), b, t, tokens.data_ptr(), token_len.data_ptr(),
                                           max_tok, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(f.device).cuda_stream),
                   "rnnt_greedy")
        return tokens, token_len

    def greedy_tokens(self, x: torch.Tensor, x_len: Optional[torch.Tensor], from_mel: bool = False) -> List[List[int]]:
        """Greedy token-id sequences (without the start token), one list per utterance."""
        f, f_len, _ = self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len)
        tokens, token_len = self.decode_encoded(f, f_len)
        tokens, token_len = tokens.cpu(), token_len.cpu()          # one D2H copy per batch
        return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]

    def gready_search_decoding(self, x, x_len):
        """Reference spelling (transducer.py:139).  Decoded strings when a tokenizer is attached
        (``tokenizer.decode(y[:, 1:].tolist())``, transducer.py:179), otherwise the id lists."""
        ids = self.greedy_tokens(x, x_len)
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    greedy_search_decoding = gready_search_decoding

    # ------------------------------------------------------------------ streaming
    def open_decode_stream(self, max_streams: int):
        """The greedy decode resumed per stream, the decoder alone: ``push(f, f_len, streams)`` decodes the new encoder frames of the listed streams from the
        prediction-network state each of them carries (efficientconformer_amd/streaming.py: RnntStreamState; effconf_rnnt_greedy_resume)."""
        from .streaming import RnntStreamState
        return RnntStreamState(self, max_streams)

    def open_stream(self, max_streams: int, max_frames: Optional[int] = None):
        """``ConformerEncoder.open_stream`` on the (causal, bf16) encoder plus the resumed greedy decode: ``push_mel`` / ``push_audio`` return the new token ids
        per stream, ``tokens(stream)`` the hypothesis so far (streaming.py: StreamingTransducer).  Greedy only: the beam searches do not stream."""
        from .streaming import StreamingTransducer
        return StreamingTransducer(self, max_streams, max_frames)

    # ------------------------------------------------------------------ beam search
    def decode_encoded_beam(self, f: torch.Tensor, f_len: Optional[torch.Tensor], beam_size: Optional[int] = None,
                            max_expansions_per_frame: Optional[int] = None, max_tokens: Optional[int] = None):
        """Beam search of encoder outputs f (B, T, Denc) fp32 on the GPU (effconf_rnnt_beam) -> (tokens (B, max_tokens) i32,
        token_len (B) i32, score (B) f32, status (B) i32).  status 1 / 2: the utterance hit the expansion / token cap and has no tokens.
        Defaults: beam_size = self.beam_size, max_expansions_per_frame = 16 * beam, max_tokens = max(16, beam) * T.
        With ``self.lm`` attached and ``self.lm_weight`` > 0 this is ``decode_encoded_beam_lm`` on them (the fused search)."""
        return self.decode_encoded_beam_lm(f, f_len, beam_size, max_expansions_per_frame, max_tokens)

    def decode_encoded_beam_lm(self, f: torch.Tensor, f_len: Optional[torch.Tensor], beam_size: Optional[int] = None,
                               max_expansions_per_frame: Optional[int] = None, max_tokens: Optional[int] = None, lm=None,
                               lm_weight: Optional[float] = None, lm_tmp: Optional[float] = None):
        """``decode_encoded_beam`` with the fusion arguments spelled out: lm (default ``self.lm``), lm_weight (``self.lm_weight``), lm_tmp
        (``self.lm_tmp``).  With a LanguageModel and a weight > 0 the search fuses the LM's log-probabilities (effconf_rnnt_beam_lm; the batch is
        split into chunks whose workspace stays under ``BEAM_LM_WORKSPACE_CAP``); without an LM, or at weight 0, it is the plain search
        (effconf_rnnt_beam).  A negative or non-finite weight with an LM raises ValueError."""
        lm, weight, ltmp = self._fusion(lm, lm_weight, lm_tmp)
        _native.require_hip(f)
        if lm is not None:
            _native.require_hip(lm.fc.weight)
        with torch.cuda.device(f.device):
            return self._decode_encoded_beam(f, f_len, beam_size, max_expansions_per_frame, max_tokens, lm, weight, ltmp)

    def _fusion(self, lm, lm_weight, lm_tmp):
        """(lm or None, weight, lm_tmp) a beam search runs with: the arguments, else the attributes; None when there is nothing to fuse."""
        lm = self.lm if lm is None else lm
        weight = float(self.lm_weight if lm_weight is None else lm_weight)
        ltmp = float(self.lm_tmp if lm_tmp is None else lm_tmp)
        if lm is None or weight == 0:
            return None, 0.0, ltmp
        if not 0 < weight < float("inf"):
            raise ValueError("lm_weight must be >= 0 and finite; got %r" % (weight,))
        if not 0 < ltmp < float("inf"):
            raise ValueError("lm_tmp must be > 0 and finite; got %r" % (ltmp,))
        return lm, weight, ltmp

    def _decode_encoded_beam(self, f, f_len, beam_size, max_expansions_per_frame, max_tokens, lm=None, lm_weight=0.0, lm_tmp=1.0):
        beam = int(self.beam_size if beam_size is None else beam_size)
        vocab = self._cfg[3]
        if not 1 <= beam <= min(16, vocab):
            raise _lib.EffconfError("beam_size must be in 1 .. min(16, vocab_size = %d); got %d" % (vocab, beam))
        if not self.tmp > 0:
            raise _lib.EffconfError("decoding_params['tmp'] must be > 0; got %r" % (self.tmp,))
        self._ensure_rnnt()
        lib = _lib.load()
        f = f.contiguous().float()
        b, t, _ = f.shape
        f_len = _native.lengths(f_len, b, t, f.device)
        max_exp = int(16 * beam if max_expansions_per_frame is None else max_expansions_per_frame)
        max_tok = int(max(16, beam) * max(t, 1) if max_tokens is None else max_tokens)
        tokens = torch.empty(b, max_tok, dtype=torch.int32, device=f.device)
        token_len = torch.empty(b, dtype=torch.int32, device=f.device)
        score = torch.empty(b, dtype=torch.float32, device=f.device)
        status = torch.empty(b, dtype=torch.int32, device=f.device)
        stream = torch.cuda.current_stream(f.device).cuda_stream
        if lm is None:
            nbytes = _native.sized(lib, "effconf_rnnt_beam", lib.effconf_rnnt_beam_workspace_bytes(self._rnnt, b, t, beam, max_exp, max_tok),
                                   batch=b, T=t, beam=beam, max_expansions=max_exp, max_tokens=max_tok)
            ws = _native.workspace(nbytes, f.device)
            _lib.check(lib.effconf_rnnt_beam(self._rnnt, f.data_ptr(), f_len.data_ptr(), b, t, beam, float(self.tmp), max_exp, tokens.data_ptr(),
                                             token_len.data_ptr(), score.data_ptr(), status.data_ptr(), max_tok, ws.data_ptr(), ws.numel(), stream),
                       "rnnt_beam")
            self._beam_ws, self._beam_rounds = [(ws, b)], None
            return tokens, token_len, score, status
        lm._ensure()
        size = lambda n: _native.sized(lib, "effconf_rnnt_beam_lm",
                                       lib.effconf_rnnt_beam_lm_workspace_bytes(self._rnnt, lm._handle, n, t, beam, max_exp, max_tok),
                                       batch=n, T=t, beam=beam, max_expansions=max_exp, max_tokens=max_tok)
        # rows are independent: chunks of utterances whose workspace stays under the cap (one utterance at the least)
        step = max(1, b)
        while step > 1 and size(step) > BEAM_LM_WORKSPACE_CAP:
            step = (step + 1) // 2
        self._beam_ws, self._beam_rounds = [], []
        rounds = C.c_int32(0)
        for lo in range(0, b, step):
            n = min(step, b - lo)
            ws = _native.workspace(size(n), f.device)
            _lib.check(lib.effconf_rnnt_beam_lm(self._rnnt, lm._handle, f[lo:].data_ptr(), f_len[lo:].data_ptr(), n, t, beam, float(self.tmp),
                                                lm_weight, lm_tmp, max_exp, tokens[lo:].data_ptr(), token_len[lo:].data_ptr(), score[lo:].data_ptr(),
                                                status[lo:].data_ptr(), max_tok, C.byref(rounds), ws.data_ptr(), ws.numel(), stream), "rnnt_beam_lm")
            self._beam_ws.append((ws, n))
            self._beam_rounds.append(int(rounds.value))
        return tokens, token_len, score, status

    def last_beam_stats(self) -> np.ndarray:
        """Per-utterance counters of the last decode_encoded_beam / decode_encoded_beam_lm call: (B, 4) i32 = evaluation batches, evaluated hypotheses,
        expansions, frames (the head of the workspace, include/effconf.h)."""
        out = []
        for ws, b in self._beam_ws:
            off = (-ws.data_ptr()) % 256
            out.append(ws[off:off + 16 * b].view(torch.int32).view(b, 4).cpu().numpy())
        return np.concatenate(out) if out else np.zeros((0, 4), dtype=np.int32)

    def last_beam_rounds(self) -> Optional[List[int]]:
        """Search launches of the last decode_encoded_beam / decode_encoded_beam_lm call, one entry per chunk of the batch (an LM step ran between two of them); None after
        a plain search, which is one launch."""
        return self._beam_rounds

    def beam_tokens(self, x: torch.Tensor, x_len: Optional[torch.Tensor], beam_size: Optional[int] = None,
                    from_mel: bool = False, lm=None, lm_weight: Optional[float] = None, lm_tmp: Optional[float] = None) -> List[List[int]]:
        """Beam-search token-id sequences (without the start token), one list per utterance; lm / lm_weight / lm_tmp as decode_encoded_beam_lm.
        Raises EffconfError naming the utterances that hit the expansion or token cap (never a silently truncated result)."""
        self._fusion(lm, lm_weight, lm_tmp)                            # the argument rules, before the encoder runs
        f, f_len, _ = self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len)
        tokens, token_len, _, status = self.decode_encoded_beam_lm(f, f_len, beam_size, lm=lm, lm_weight=lm_weight, lm_tmp=lm_tmp)
        tokens, token_len, status = tokens.cpu(), token_len.cpu(), status.cpu()
        capped = {1: [i for i in range(len(status)) if int(status[i]) == 1], 2: [i for i in range(len(status)) if int(status[i]) == 2]}
        if capped[1] or capped[2]:
            msg = []
            if capped[1]:
                msg.append("utterances %s hit the expansion cap (max_expansions_per_frame: B never filled, the reference would not "
                           "terminate)" % capped[1])
            if capped[2]:
                msg.append("utterances %s hit the token cap (max_tokens)" % capped[2])
            raise _lib.EffconfError("beam search: " + "; ".join(msg))
        return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]

    def beam_search_decoding(self, x, x_len, beam_size=None):
        """Reference name and signature (transducer.py:188).  Decoded strings when a tokenizer is attached
        (``tokenizer.decode(best_hyp["prediction"][1:])`` per utterance, transducer.py:323), otherwise the id lists.  With ``self.lm`` attached and
        ``self.lm_weight`` > 0 the search fuses the LM (``self.lm_tmp``), as the reference's does."""
        ids = self.beam_tokens(x, x_len, beam_size)
        return [self.tokenizer.decode(i) for i in ids] if self.tokenizer is not None else ids

    # ------------------------------------------------------------------ lattice scoring, forced alignment
    def _ids(self, y):
        """Strings -> id lists through the tokenizer; anything else as it is."""
        return _targets.ids(self.tokenizer, y)

    def _targets(self, y, y_len, device):
        """(targets (B, U) i32, target_len (B,) i64) on `device` from a padded integer tensor + lengths, a list of id lists, or a list of
        strings (needs a tokenizer).  A list is padded on the host and copied once."""
        return _targets.targets(self.tokenizer, y, y_len, device)

    def lattice(self, f: torch.Tensor, f_len: Optional[torch.Tensor], y, y_len=None):
        """The RNN-T lattice of encoder outputs f (B, T, Denc) fp32 and transcripts `y` ((B, U) integers + `y_len`, or a list of id lists) on
        the GPU (effconf_rnnt_lattice), temperature ``self.tmp`` -> (lp_blank, lp_label (B, T, U + 1) f32, status (B,) i32).  For t < f_len[b],
        u <= y_len[b]: lp_blank = log P(blank | t, u), lp_label = log P(y[u] | t, u) (-inf at u = y_len[b]); 0 outside.  With tmp = 1 these
        are the entries of log_softmax(joint logits) the RNN-T loss reads.  include/effconf.h has the details."""
        if f.dim() != 3:
            raise _lib.EffconfError("encoder outputs must be (batch, frames, dim); got shape %s" % (tuple(f.shape),))
        _native.require_hip(f)
        if not 0 < self.tmp < float("inf"):
            raise _lib.EffconfError("decoding_params['tmp'] must be > 0; got %r" % (self.tmp,))
        dev = f.device
        tg, tl = self._targets(y, y_len, dev)
        b, t, _ = f.shape
        if tg.shape[0] != b or tl.shape[0] != b:
            raise _lib.EffconfError("targets: %d rows for %d utterances" % (tg.shape[0], b))
        u = int(tg.shape[1])
        with torch.cuda.device(dev):
            self._ensure_rnnt()
            lib = _lib.load()
            nbytes = _native.sized(lib, "effconf_rnnt_lattice", lib.effconf_rnnt_lattice_workspace_bytes(self._rnnt, b, t, u), batch=b, T=t, U=u)
            f = f.contiguous().float()
            f_len = _native.lengths(f_len, b, t, dev)
            lp_blank = torch.empty(b, t, u + 1, dtype=torch.float32, device=dev)
            lp_label = torch.empty(b, t, u + 1, dtype=torch.float32, device=dev)
            status = torch.empty(b, dtype=torch.int32, device=dev)
            ws = _native.workspace(nbytes, dev)
            _lib.check(lib.effconf_rnnt_lattice(self._rnnt, f.data_ptr(), f_len.data_ptr(), b, t, tg.data_ptr(), tl.data_ptr(), u, float(self.tmp),
                                                lp_blank.data_ptr(), lp_label.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream(dev).cuda_stream), "rnnt_lattice")
        return lp_blank, lp_label, status

    def align_lattice(self, lp_blank: torch.Tensor, lp_label: torch.Tensor, f_len: Optional[torch.Tensor], y_len, scores_only: bool = False,
                      status: Optional[torch.Tensor] = None):
        """The lattice's dynamic programs on the GPU (effconf_rnnt_align) -> dict of device tensors: ``log_likelihood`` (B,) f32 =
        log P(y | x) over all paths, ``status`` (B,) i32 (starts from `status`, the lattice's, when given) and, unless `scores_only`,
        ``score`` (B,) f32 = log-probability of the best path, ``token_frame`` (B, U) i32 (the frame token u is emitted at, -1 at or beyond
        y_len) and ``token_logp`` (B, U) f32."""
        if lp_blank.dim() != 3 or lp_blank.shape != lp_label.shape:
            raise _lib.EffconfError("planes must be two (batch, frames, tokens + 1) tensors; got %s and %s" % (tuple(lp_blank.shape), tuple(lp_label.shape)))
        b, t, e = lp_blank.shape
        if e < 1:
            raise _lib.EffconfError("planes need at least the column u = 0")
        u = e - 1
        dev = lp_blank.device
        lib = _lib.load()
        nbytes = _native.sized(lib, "effconf_rnnt_align", lib.effconf_rnnt_align_workspace_bytes(b, t, u), batch=b, T=t, U=u)
        _native.require_hip(lp_blank)
        with torch.cuda.device(dev):
            lp_blank, lp_label = lp_blank.contiguous().float(), lp_label.contiguous().float()
            f_len = _native.lengths(f_len, b, t, dev)
            y_len = torch.as_tensor(y_len).to(device=dev, dtype=torch.int64).contiguous()
            if f_len.shape[0] != b or y_len.shape[0] != b:
                raise _lib.EffconfError("lengths: %d / %d entries for %d utterances" % (f_len.shape[0], y_len.shape[0], b))
            st = torch.zeros(b, dtype=torch.int32, device=dev) if status is None else status.to(device=dev, dtype=torch.int32).clone()
            out = {"log_likelihood": torch.empty(b, dtype=torch.float32, device=dev), "status": st}
            if not scores_only:
                out["score"] = torch.empty(b, dtype=torch.float32, device=dev)
                out["token_frame"] = torch.empty(b, u, dtype=torch.int32, device=dev)
                out["token_logp"] = torch.empty(b, u, dtype=torch.float32, device=dev)
            ws = _native.workspace(nbytes, dev)
            ptr = lambda k: out[k].data_ptr() if k in out else None
            _lib.check(lib.effconf_rnnt_align(lp_blank.data_ptr(), lp_label.data_ptr(), f_len.data_ptr(), y_len.data_ptr(), b, t, u,
                                              ptr("log_likelihood"), ptr("score"), ptr("token_frame"), ptr("token_logp"), ptr("status"),
                                              ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "rnnt_align")
        return out

    def _encode(self, x, x_len, from_mel):
        _native.require_hip(x)
        f, f_len, _ = self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len)
        return f, f_len

    def align(self, x: torch.Tensor, x_len: Optional[torch.Tensor], y, y_len=None, from_mel: bool = False) -> List[TransducerAlignment]:
        """Token timestamps of known transcripts: encoder, ``lattice``, ``align_lattice`` -> one ``TransducerAlignment`` per utterance.
        `y`: a padded (B, U) integer tensor (+ `y_len`), a list of id lists, or a list of strings when a tokenizer is attached."""
        y = self._ids(y)
        f, f_len = self._encode(x, x_len, from_mel)
        tg, tl = self._targets(y, y_len, f.device)
        lp_blank, lp_label, status = self.lattice(f, f_len, tg, tl)
        out = self.align_lattice(lp_blank, lp_label, f_len, tl, status=status)
        fs = self.encoder.frame_seconds
        host = {k: v.cpu() for k, v in out.items()}                     # one D2H copy per batch (per output tensor)
        tg, tl = tg.cpu(), tl.cpu()
        recs = []
        for i in range(tg.shape[0]):
            n = max(0, min(int(tl[i]), tg.shape[1]))
            fr = host["token_frame"][i, :n].tolist()
            recs.append(TransducerAlignment(tg[i, :n].tolist(), fr, [k * fs for k in fr], host["token_logp"][i, :n].tolist(),
                                            float(host["score"][i]), float(host["log_likelihood"][i]), int(host["status"][i])))
        return recs

    def score_labels(self, x: torch.Tensor, x_len: Optional[torch.Tensor], y, y_len=None, from_mel: bool = False) -> torch.Tensor:
        """log P(y | x) of every utterance, (B,) fp32 on the device (-inf where the transcript cannot be scored): the lattice and its
        forward recursion alone (no Viterbi pass, no back-pointers), = -rnnt_loss at tmp = 1."""
        y = self._ids(y)
        f, f_len = self._encode(x, x_len, from_mel)
        tg, tl = self._targets(y, y_len, f.device)
        lp_blank, lp_label, status = self.lattice(f, f_len, tg, tl)
        return self.align_lattice(lp_blank, lp_label, f_len, tl, scores_only=True, status=status)["log_likelihood"]
