"""CTC model wrapper: the caller side of the hot path (reference models/model_ctc.py:39-136).

``ModelCTC`` keeps the reference's attribute names (``encoder``, ``fc``), state-dict keys
(``encoder.*``, ``fc.*``) and method names (including the reference's spelling
``gready_search_decoding``), but the head and the greedy collapse run as HIP kernels
(effconf_ctc_greedy) instead of ``nn.Linear`` + a Python loop with ``.item()`` per token.
``beam_search_decoding`` (model_ctc.py:138-181) is ctcdecode's CTC prefix beam search without the n-gram scorer: the head's
fp32 logits go to one persistent HIP kernel per batch (effconf_ctc_beam, one workgroup per utterance) instead of a host copy and
8 CPU processes.  The n-gram (KenLM) terms (``ngram_path``, ``ngram_alpha``, ``ngram_beta``) and
probability cutoffs below the shipped ones are not implemented; a ``LanguageModel`` attached as ``lm`` rescores the search's ranked n-best after
it (``rescore_nbest``, ``beam_labels_rescored``, ``beam_search_rescored``; csrc/lm.hip) or is fused INTO the search (``decode_logits_beam_lm``,
``beam_labels_fused``, ``beam_search_fused``; effconf_ctc_beam_lm: every frame's candidates are ranked with the LM's score of the prefix).  Token timestamps and transcript scores come from the forced alignment instead:
``align`` / ``greedy_alignment`` (Viterbi over the CTC trellis: which frames each token covers) and ``score_labels`` (the CTC forward
algorithm: log P(y | x), -ctc_loss without the host copy) run on the same logits in csrc/ctc_align.hip (effconf_ctc_align).  On a stream the plain search is
resumed push by push from a carried beam (``open_stream(..., beam_size=k)``, ``open_beam_decode_stream``; effconf_ctc_beam_resume).  Training
(losses with gradients, optimizer, schedules), WER scoring and word-level (SentencePiece-merging) timestamps are out of scope (HISTORY.md).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _native, _targets
from .config import load_config
from .encoders import ConformerEncoder, ConformerEncoderInterCTC


class Alignment(NamedTuple):
    """Forced alignment of one utterance (``ModelCTC.align``): token u covers the encoder frames start_frame[u] .. end_frame[u] - 1, i.e. the
    seconds start_time[u] .. end_time[u] (frame x ``ConformerEncoder.frame_seconds``); token_logp[u] is the log-probability summed over these
    frames, ``score`` the log-probability of the whole best path, ``log_likelihood`` log P(tokens | audio) over all paths.  status: 0 ok,
    1 too few frames for the tokens, 2 a token id outside 1 .. vocab - 1 (then the spans are -1 and both scores -inf)."""
    tokens: List[int]
    start_frame: List[int]
    end_frame: List[int]
    start_time: List[float]
    end_time: List[float]
    token_logp: List[float]
    score: float
    log_likelihood: float
    status: int


class HeadMargins(NamedTuple):
    """``ModelCTC.head_margins``: the greedy labels with the top-2 logit margins they were taken at, all on the device.  labels (B, T) i32 with a zero
    tail, label_len (B,) i32, frame_margin (B, T) f32 (largest minus second largest logit of every frame of the rectangle), min_margin (B,) f32 / min_frame
    (B,) i32: the smallest margin over an utterance's valid frames and the first frame that holds it (+inf / -1 without frames), logits (B, T, V) or None."""
    labels: torch.Tensor
    label_len: torch.Tensor
    frame_margin: torch.Tensor
    min_margin: torch.Tensor
    min_frame: torch.Tensor
    logits: Optional[torch.Tensor]


# Default band of ``ModelCTC.greedy_exact``: twice the largest per-frame spread max_v d_v - min_v d_v, d = bf16-mode logits - split-mode logits, measured
# over tools/label_exact_band.py's grid (profiles/label_exact_band.txt), rounded up to two digits: the worst spread, 2.97, comes from the
# "trained" weight recipe of synth.make_stressed_state_dict on EfficientConformerCTCLarge (make_state_dict alone: 0.084).
LABEL_EXACT_BAND = 6.0
# Largest workspace of one effconf_ctc_beam_lm call: ``decode_logits_beam_lm`` splits the batch into chunks that stay under it (an utterance holds
# 2 * beam + 1 LM slots of 2 * layers * dim_model + vocab floats; rows are independent)
BEAM_LM_WORKSPACE_CAP = 16 << 30


def select_rerun(min_margin: torch.Tensor, band: float) -> torch.Tensor:
    """The rows of a batch that margin-gated decoding runs again in the split mode: those whose smallest top-2 margin is not known to be at least
    `band` - ``not (min_margin >= band)``, so a NaN margin is selected, +inf (an utterance without frames) never, a margin equal to the band is kept.
    Returns their indices, ascending, int64, on `min_margin`'s device.  Pure: no model, no GPU."""
    mm = torch.as_tensor(min_margin)
    return torch.nonzero(~(mm >= float(band)), as_tuple=False).reshape(-1)


def select_nbest(am_score: torch.Tensor, lm_score: torch.Tensor, token_len: torch.Tensor, lm_weight: float, length_bonus: float = 0.0):
    """The selection rule of ``ModelCTC.rescore_nbest`` on (B, beam) scores: total = am_score + lm_weight * lm_score + length_bonus * token_len
    in fp32 (the LM term is left out at lm_weight == 0, so an LM score of -inf cannot turn it into NaN); ranks whose am_score is -inf take no
    part; the best total wins, ties go to the lower rank (also when every rank is excluded: rank 0).  Returns (best_rank (B,) i64, total).
    Pure torch ops on the scores' device: no model, no GPU needed."""
    am = torch.as_tensor(am_score).float()
    total = am.clone()
    if lm_weight:
        total = total + float(lm_weight) * torch.as_tensor(lm_score).to(am.device).float()
    if length_bonus:
        total = total + float(length_bonus) * torch.as_tensor(token_len).to(am.device).float()
    key = torch.where(torch.isneginf(am) | torch.isnan(total), torch.full_like(total, float("-inf")), total)
    top = key.max(dim=1, keepdim=True).values
    beam = key.shape[1]
    rank = torch.arange(beam, device=key.device).expand_as(key)
    best = torch.where(key == top, rank, torch.full_like(rank, beam)).min(dim=1).values      # the first rank that holds the maximum
    return best.clamp(max=beam - 1), total


class ModelCTC(_native.NativeModel):
    _encoder_cls = ConformerEncoder

    def __init__(self, encoder_params: dict, tokenizer_params: dict, training_params: Optional[dict] = None,
                 decoding_params: Optional[dict] = None, name: str = "model", tokenizer=None):
        super().__init__()
        if encoder_params.get("arch", "Conformer") != "Conformer":
            raise Exception("Unknown encoder architecture:", encoder_params.get("arch"))
        self.encoder = self._encoder_cls(encoder_params)
        self.fc = nn.Linear(self.encoder.plan.dim_out, tokenizer_params["vocab_size"])
        self.encoder.attach_head(self.fc)
        decoding_params = decoding_params or {}
        self.beam_size = int(decoding_params.get("beam_size", 1))                    # model.py:60-61
        self.tmp = float(decoding_params.get("tmp", 1))
        self.label_exact_band = float(decoding_params.get("label_exact_band", LABEL_EXACT_BAND))
        self.tokenizer = tokenizer
        self.name = name
        self._beam_ws = None
        self._beam_rounds = None
        # the reference's attribute and decoding_params (model.py:70-72): a LanguageModel attached by the caller; rescoring only.  Assigning one
        # registers it as a submodule, as in the reference: state_dict() then carries its tensors under ``lm.``
        self.lm = None
        self.lm_weight = float(decoding_params.get("lm_weight", 0))
        self.lm_tmp = float(decoding_params.get("lm_tmp", 1))
        self.eval()

    @classmethod
    def from_config(cls, cfg, tokenizer=None):
        cfg = load_config(cfg)
        if cls is ModelCTC and cfg.get("model_type") == "InterCTC":      # functions.py:59-66: model_type selects the class
            cls = InterCTC
        return cls(cfg["encoder_params"], cfg["tokenizer_params"], cfg.get("training_params"),
                   cfg.get("decoding_params"), cfg.get("model_name", "model"), tokenizer)

    def _invalidate(self):
        self.encoder.repack()

    # ---- reference ModelCTC.forward (model_ctc.py:57-68): batch = (x, y, x_len, y_len)
    def forward(self, batch, return_attentions: bool = False):
        x, _, x_len, _ = batch
        enc, enc_len, attentions = self.encoder(x, x_len, return_attentions=return_attentions)[:3]
        logits, _, _ = self._head(enc, enc_len, want_logits=True)
        return logits, enc_len, attentions

    # workspace of the greedy head per frame of the (rows, t) rectangle: the i32 argmax the collapse reads and, in the margin instance, the fp32
    # top-2 margin next to it (the sizes effconf_ctc_greedy / _bf16 / _margin check, csrc/encoder.hip)
    _GREEDY_WS, _MARGIN_WS = 4, 8

    def open_stream(self, max_streams: int, max_frames: Optional[int] = None, beam_size: Optional[int] = None):
        """``ConformerEncoder.open_stream`` with the greedy head on the new frames: ``push_mel`` / ``push_audio`` return the new token ids per stream, the
        repeat collapse carried across pushes (streaming.py: ctc_collapse_carry).  With a `beam_size`: a ``StreamingCTCBeam`` - the prefix beam search resumed
        on the new rows' logits (effconf_ctc_beam_resume), which returns the newly COMMITTED tokens of every push and needs `max_frames`
        (ValueError without it).  Not built: LM fusion in a streaming search, trie compaction for unbounded streams."""
        from .streaming import StreamingCTC, StreamingCTCBeam
        if beam_size is not None:
            return StreamingCTCBeam(self, max_streams, max_frames, int(beam_size))
        return StreamingCTC(self, max_streams, max_frames)

    def open_beam_decode_stream(self, max_streams: int, max_frames: int, beam_size: Optional[int] = None, device=None):
        """The streaming decoder alone (the counterpart of ``Transducer.open_decode_stream``): a ``CtcBeamStreamState`` whose ``push`` resumes the CTC prefix
        beam search of `max_streams` streams on new head logits; `max_frames` logit frames per utterance at the most; beam_size None: ``self.beam_size``.
        `device`: where the state lives when the model's parameters are not on a HIP device (the decoder reads logits only)."""
        from .streaming import CtcBeamStreamState
        return CtcBeamStreamState(self, max_streams, max_frames, beam_size, device)

    def _greedy_rows(self, rows: torch.Tensor, as_bf16: bool, lens: torch.Tensor, lo: int, hi: int, labels, label_len, logits=None, margins=None):
        """The greedy head on utterances [lo, hi) of `rows` (B, T, D) - and of every other tensor given - on the current stream:
        effconf_ctc_greedy / effconf_ctc_greedy_bf16, or with `margins` = (frame_margin or None, min_margin, min_frame) effconf_ctc_greedy_margin."""
        lib, b, t = _lib.load(), hi - lo, rows.shape[1]
        ws = _native.workspace(b * t * (self._GREEDY_WS if margins is None else self._MARGIN_WS), rows.device)
        stream = torch.cuda.current_stream(rows.device).cuda_stream
        at = lambda tns: None if tns is None else tns[lo:].data_ptr()
        if margins is None:
            fn = lib.effconf_ctc_greedy_bf16 if as_bf16 else lib.effconf_ctc_greedy
            _lib.check(fn(self.encoder._handle, at(rows), at(lens), b, t, at(labels), at(label_len), at(logits), ws.data_ptr(), ws.numel(), stream),
                       "ctc_greedy")
        else:
            frame_margin, min_margin, min_frame = margins
            _lib.check(lib.effconf_ctc_greedy_margin(self.encoder._handle, at(rows), int(as_bf16), at(lens), b, t, at(labels), at(label_len), at(logits),
                                                     at(frame_margin), at(min_margin), at(min_frame), ws.data_ptr(), ws.numel(), stream),
                       "ctc_greedy_margin")

    def _head_inputs(self, enc: torch.Tensor, enc_len: Optional[torch.Tensor]):
        """-> (rows, as_bf16, lengths) as the greedy head takes them."""
        _native.require_hip(enc)
        # bf16 rows (a gathered chunk of the multi-rank path on a bf16 wire) go to the head as they are: effconf_ctc_greedy_bf16 - no widening pass,
        # two MFMAs per 16 k, labels identical to the fp32-input head on the same values
        # (only while the handle's head IS the split-bf16 kernel, option ctc_mfma = 2, the default: with 0 / 1 the fp32 head is a k-ordered fp32 chain and the
        # bf16 rows are widened to it, so gathered and local chunks keep producing the same labels)
        as_bf16 = enc.dtype == torch.bfloat16 and self.encoder.precision == "bf16" and self.encoder._options.get("ctc_mfma", 2) == 2
        enc = enc.contiguous() if as_bf16 else enc.contiguous().float()
        return enc, as_bf16, _native.lengths(enc_len, enc.shape[0], enc.shape[1], enc.device)

    def _head(self, enc: torch.Tensor, enc_len: Optional[torch.Tensor], want_logits: bool = False):
        enc, as_bf16, enc_len = self._head_inputs(enc, enc_len)
        b, t, _ = enc.shape
        labels = torch.empty(b, t, dtype=torch.int32, device=enc.device)
        label_len = torch.empty(b, dtype=torch.int32, device=enc.device)
        logits = torch.empty(b, t, self.fc.out_features, dtype=torch.float32, device=enc.device) if want_logits else None
        with torch.cuda.device(enc.device):          # the C library launches on the current device
            self.encoder._ensure_packed()
            self._greedy_rows(enc, as_bf16, enc_len, 0, b, labels, label_len, logits)
        return logits, labels, label_len

    def head_margins(self, enc: torch.Tensor, enc_len: Optional[torch.Tensor], want_logits: bool = False) -> HeadMargins:
        """``_head`` with the top-2 logit margin of every frame and its minimum per utterance (effconf_ctc_greedy_margin): the same head kernel as
        ``_head`` takes for this handle and row type, so labels, label counts and logits are bit-identical to its; frame_margin is the fp32 difference
        of the two largest logits of a frame (0 for a duplicated maximum)."""
        enc, as_bf16, enc_len = self._head_inputs(enc, enc_len)
        b, t, _ = enc.shape
        dev = enc.device
        out = HeadMargins(torch.empty(b, t, dtype=torch.int32, device=dev), torch.empty(b, dtype=torch.int32, device=dev),
                          torch.empty(b, t, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.float32, device=dev),
                          torch.empty(b, dtype=torch.int32, device=dev),
                          torch.empty(b, t, self.fc.out_features, dtype=torch.float32, device=dev) if want_logits else None)
        with torch.cuda.device(dev):          # the C library launches on the current device
            self.encoder._ensure_packed()
            self._greedy_rows(enc, as_bf16, enc_len, 0, b, out.labels, out.label_len, out.logits, (out.frame_margin, out.min_margin, out.min_frame))
        return out

    def _range_head(self, margins: bool):
        """-> (range_hook, state) for ``ConformerEncoder.forward``: the hook runs the greedy head on a row range, on that range's stream, into outputs
        for the whole batch that the first range allocates - state["labels"] (B, T) i32, state["label_len"] (B,) i32 and, with `margins`,
        state["min_margin"] (B,) f32 / state["min_frame"] (B,) i32."""
        state = {}

        def hook(lo, hi, out, out_len):
            if not state:
                b, t = out.shape[0], out.shape[1]
                state["labels"] = torch.empty(b, t, dtype=torch.int32, device=out.device)
                state["label_len"] = torch.empty(b, dtype=torch.int32, device=out.device)
                if margins:
                    state["min_margin"] = torch.empty(b, dtype=torch.float32, device=out.device)
                    state["min_frame"] = torch.empty(b, dtype=torch.int32, device=out.device)
            self._greedy_rows(out, False, out_len, lo, hi, state["labels"], state["label_len"],
                              margins=(None, state["min_margin"], state["min_frame"]) if margins else None)
            st = torch.cuda.current_stream(out.device)
            for tns in state.values():
                tns.record_stream(st)

        return hook, state

    def _encode_margins(self, x, x_len, from_mel, x_len_host):
        """Encoder + margin head, the head per row range on that range's stream as in ``encode_greedy`` -> (labels, label_len, min_margin, min_frame)."""
        hook, state = self._range_head(margins=True)
        (self.encoder.forward_mel if from_mel else self.encoder)(x, x_len, range_hook=hook, x_len_host=x_len_host)
        return state["labels"], state["label_len"], state["min_margin"], state["min_frame"]

    def greedy_exact(self, x: torch.Tensor, x_len: torch.Tensor, band: Optional[float] = None, from_mel: bool = False, x_len_host=None):
        """Margin-gated label-exact greedy decoding: the bf16 ragged forward with the margin head; every utterance whose smallest top-2
        logit margin over its valid frames is not at least `band` runs again - all of them as ONE ragged ``precision = "split"`` batch, trimmed to
        their longest - and takes the split mode's labels.  If `band` is at least the per-frame spread of (bf16 logit - split logit), the result is the
        split mode's labels for the whole batch: with a the bf16 argmax of a frame and m its margin, split[a] - split[v] >= m - spread > 0 for every
        other v.  `band` None: ``decoding_params["label_exact_band"]``, else ``LABEL_EXACT_BAND`` (measured, not proven: profiles/label_exact_band.txt).
        0 runs nothing again, inf everything.

        Returns (labels (B, T) i32 with zero tails, label_len (B,) i32, report); report: ``band``; ``min_margin`` (B,) f32 on the HOST and
        ``min_frame`` (B,) i32 on the device, of the bf16 pass; ``rerun``: the row indices that ran again (host, int64, ascending); ``changed``: (B,) bool
        on the device, the rows whose labels moved; ``exact_min_margin``: the split pass's smallest margins of the rows in ``rerun`` (device).

        Needs ``encoder.ragged`` - the only batch semantics in which an utterance's labels do not depend on its neighbours, so that running a subset
        again reproduces them - and ``encoder.precision == "bf16"``.  One synchronisation (the copy of min_margin to the host, plus that of `x_len` when
        `x_len_host` is not given), so it refuses to run while a stream is being captured.  The handle is packed for the split mode once (it serves
        the bf16 path as well); ``precision`` is "bf16" again on return, also after an error."""
        enc = self.encoder
        _native.require_hip(x)
        if not enc.ragged:
            raise RuntimeError("greedy_exact needs encoder.ragged = True: only a ragged forward gives an utterance the same labels in every batch")
        if enc.precision != "bf16":
            raise RuntimeError("greedy_exact gates the bf16 path: encoder.precision is %r (that mode's greedy_labels are already what it computes)" % enc.precision)
        if x_len is None:
            raise ValueError("greedy_exact needs x_len (a ragged batch)")
        band = float(self.label_exact_band if band is None else band)
        if band != band or band < 0:
            raise ValueError("band must be >= 0; got %r" % band)
        with torch.cuda.device(x.device):
            if enc._capturing(x.device):
                raise RuntimeError("greedy_exact synchronises (min_margin goes to the host): not while a stream is being captured")
            if not (enc._packed and enc._exact_packed == 2):
                try:                               # pack for the split mode: that handle serves both passes
                    enc.precision = "split"
                    enc._ensure_packed()
                finally:
                    enc.precision = "bf16"
            host = x_len_host if x_len_host is not None else x_len.cpu()
            host = np.ascontiguousarray(np.asarray(host.cpu() if torch.is_tensor(host) else host, dtype=np.int64))
            check = enc.check_host_lengths
            try:
                enc.check_host_lengths = check and x_len_host is not None      # a copy made here needs no comparison with its source
                labels, label_len, min_margin, min_frame = self._encode_margins(x, x_len, from_mel, host)
            finally:
                enc.check_host_lengths = check
            mm = min_margin.cpu()                  # the one D2H copy the gate needs
            rerun = select_rerun(mm, band)
            report = {"band": band, "min_margin": mm, "min_frame": min_frame, "rerun": rerun,
                      "changed": torch.zeros(x.shape[0], dtype=torch.bool, device=x.device),
                      "exact_min_margin": torch.empty(0, dtype=torch.float32, device=x.device)}
            if rerun.numel() == 0:
                return labels, label_len, report
            idx = rerun.to(x.device)
            sub_host = host[rerun.numpy()]
            n = int(sub_host.max())
            xs = (x[idx, :, :n] if from_mel else x[idx, :n]).contiguous()
            ls = x_len.to(x.device, torch.int64)[idx].contiguous()
            try:
                enc.precision = "split"
                enc.check_host_lengths = False     # both gathered from lengths the first pass has compared
                lab2, len2, mm2, _ = self._encode_margins(xs, ls, from_mel, sub_host)
            finally:
                enc.precision = "bf16"
                enc.check_host_lengths = check
            t2 = lab2.shape[1]                     # <= labels.shape[1]: the selected rows' own longest output
            new = torch.zeros(idx.numel(), labels.shape[1], dtype=torch.int32, device=x.device)
            new[:, :t2] = lab2
            report["changed"][idx] = (new != labels[idx]).any(dim=1) | (len2 != label_len[idx])
            report["exact_min_margin"] = mm2
            labels[idx] = new
            label_len[idx] = len2
        return labels, label_len, report

    def encode_greedy(self, x: torch.Tensor, x_len: Optional[torch.Tensor], from_mel: bool = False, **encoder_kwargs):
        """Encoder + CTC head with the head launched PER ROW RANGE on that range's stream (``ConformerEncoder.sub_batches``): the
        fc + argmax + collapse of range i overlaps the other ranges' encoder kernels instead of running after the join
        (reference: model_ctc.py:90-133 runs them one after the other).  Returns (enc, enc_len, labels, label_len); the labels are
        the same as ``_head(enc, enc_len)`` on the joined output - the head is row-local."""
        hook, state = self._range_head(margins=False)
        with torch.cuda.device(x.device):
            enc, enc_len = (self.encoder.forward_mel if from_mel else self.encoder)(x, x_len, range_hook=hook, **encoder_kwargs)[:2]
        return enc, enc_len, state["labels"], state["label_len"]

    def greedy_labels(self, x: torch.Tensor, x_len: Optional[torch.Tensor], from_mel: bool = False, *, label_exact: Optional[str] = None,
                      band: Optional[float] = None) -> List[List[int]]:
        """Greedy CTC label-id sequences (blank 0 removed, repeats collapsed), one list per utterance.  `label_exact`: None - one forward in
        ``encoder.precision``; "auto" - ``greedy_exact`` (utterances with a top-2 margin under `band` run again in the split mode); "always" - every
        utterance runs again (band = inf)."""
        if label_exact not in (None, "auto", "always"):
            raise ValueError("label_exact must be None, 'auto' or 'always'; got %r" % (label_exact,))
        if label_exact is not None:
            labels, label_len, _ = self.greedy_exact(x, x_len, float("inf") if label_exact == "always" else band, from_mel)
        else:
            enc, enc_len = (self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len))[:2]      # [:2]: the InterCTC encoder returns four values
            _, labels, label_len = self._head(enc, enc_len)
        labels, label_len = labels.cpu(), label_len.cpu()          # one D2H copy per batch, not one per token
        return [labels[b, :int(label_len[b])].tolist() for b in range(labels.shape[0])]

    def gready_search_decoding(self, x, x_len, label_exact: Optional[str] = None):
        """Reference spelling (model_ctc.py:90).  Returns decoded strings when a tokenizer is attached
        (``tokenizer.decode(list_of_id_lists)``, model_ctc.py:136), otherwise the id lists.  `label_exact`: as ``greedy_labels``."""
        ids = self.greedy_labels(x, x_len, label_exact=label_exact)
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    greedy_search_decoding = gready_search_decoding

    # ------------------------------------------------------------------ beam search
    def _check_beam(self, beam: int, vocab: int):
        if not 1 <= beam <= 32:
            raise _lib.EffconfError("beam_size must be in 1 .. 32; got %d" % beam)
        if not 2 <= vocab <= 1024:
            raise _lib.EffconfError("vocab_size must be in 2 .. 1024 for the CTC beam search; got %d" % vocab)
        if not 0 < self.tmp < float("inf"):
            raise _lib.EffconfError("decoding_params['tmp'] must be > 0; got %r" % (self.tmp,))

    def decode_logits_beam(self, logits: torch.Tensor, logits_len: Optional[torch.Tensor], beam_size: Optional[int] = None):
        """CTC prefix beam search of head logits (B, T, V) fp32 on the GPU (effconf_ctc_beam), temperature ``self.tmp`` ->
        (tokens (B, beam, T) i32, token_len (B, beam) i32, score (B, beam) f32), ranked best first.  score = log(P_blank + P_nonblank)
        of the prefix; ranks without a hypothesis have length 0 and score -inf."""
        beam = int(self.beam_size if beam_size is None else beam_size)
        if logits.dim() != 3:
            raise _lib.EffconfError("logits must be (batch, frames, vocab); got shape %s" % (tuple(logits.shape),))
        b, t, v = logits.shape
        self._check_beam(beam, v)
        _native.require_hip(logits)
        lib = _lib.load()
        nbytes = _native.sized(lib, "effconf_ctc_beam", lib.effconf_ctc_beam_workspace_bytes(b, t, v, beam), batch=b, T=t, vocab=v, beam=beam)
        with torch.cuda.device(logits.device):
            logits = logits.contiguous().float()
            logits_len = _native.lengths(logits_len, b, t, logits.device)
            tokens = torch.empty(b, beam, t, dtype=torch.int32, device=logits.device)
            token_len = torch.empty(b, beam, dtype=torch.int32, device=logits.device)
            score = torch.empty(b, beam, dtype=torch.float32, device=logits.device)
            ws = _native.workspace(nbytes, logits.device)
            _lib.check(lib.effconf_ctc_beam(logits.data_ptr(), logits_len.data_ptr(), b, t, v, beam, float(self.tmp), tokens.data_ptr(),
                                            token_len.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(logits.device).cuda_stream), "ctc_beam")
        self._beam_ws, self._beam_rounds = ([(ws, b)], b, t, beam, 0), None
        return tokens, token_len, score

    def last_beam_trace(self) -> List[dict]:
        """The workspace of the last decode_logits_beam / decode_logits_beam_lm call (layout: include/effconf.h), one dict per utterance: ``len``
        (frames decoded), ``candidates`` (candidates scored, summed over frames), ``lm_rows`` (LM evaluations the utterance asked for; 0: plain search), ``node`` (len, beam) i32 and ``pb`` / ``pnb`` / ``score``
        (len, beam) f32 = the beam after each frame in rank order (node -1: no member), ``parent`` / ``token`` / ``length`` (nodes,)
        i32 = the prefix trie (node 0: the empty prefix).  After a fused call also ``lm`` / ``total`` (len, beam) f32 = L and the total the ranks
        are ordered by, and ``node_lm`` (nodes,) f32 = the L every trie node holds."""
        chunks, _, t, beam, slot_floats = self._beam_ws

        def al(x):
            return (x + 255) // 256 * 256
        ncap = 1 + beam * t
        h = 1
        while h < 2 * ncap:
            h <<= 1
        o_nodes = al(16 * t * beam)
        per_utt = o_nodes + al(16 * ncap) + al(8 * h) + al(4 * h)
        o_trace2 = per_utt
        if slot_floats:
            per_utt += al(8 * t * beam) + al(4 * (2 * beam + 1) * slot_floats)
        out = []
        for ws, b in chunks:
            base = (-ws.data_ptr()) % 256                              # the library aligns the workspace up to 256 bytes
            head = ws[base:base + al(16 * b)].cpu().numpy()
            stats = head[:16 * b].view(np.int32).reshape(b, 4)
            for i in range(b):
                u = base + al(16 * b) + i * per_utt
                raw = ws[u:u + o_trace2 + (8 * t * beam if slot_floats else 0)].cpu().numpy()
                n, nn = int(stats[i, 0]), int(stats[i, 2])
                tr = raw[:16 * t * beam].view(np.int32).reshape(t, beam, 4)[:n]
                trf = tr.view(np.float32)
                nd = raw[o_nodes:o_nodes + 16 * ncap].view(np.int32).reshape(ncap, 4)[:nn]
                d = {"len": n, "candidates": int(stats[i, 1]), "lm_rows": int(stats[i, 3]), "node": tr[:, :, 0].copy(), "pb": trf[:, :, 1].copy(),
                     "pnb": trf[:, :, 2].copy(), "score": trf[:, :, 3].copy(), "parent": nd[:, 0].copy(), "token": nd[:, 1].copy(),
                     "length": nd[:, 2].copy()}
                if slot_floats:
                    t2 = raw[o_trace2:o_trace2 + 8 * t * beam].view(np.float32).reshape(t, beam, 2)[:n]
                    d.update(lm=t2[:, :, 0].copy(), total=t2[:, :, 1].copy(), node_lm=nd[:, 3].copy().view(np.float32))
                out.append(d)
        return out

    def beam_labels(self, x: torch.Tensor, x_len: Optional[torch.Tensor], beam_size: Optional[int] = None,
                    from_mel: bool = False) -> List[List[int]]:
        """Best CTC beam-search label-id sequence per utterance: encoder, head logits (``_head(want_logits=True)``), effconf_ctc_beam."""
        beam = int(self.beam_size if beam_size is None else beam_size)
        self._check_beam(beam, self.fc.out_features)
        _native.require_hip(x)
        enc, enc_len = (self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len))[:2]      # [:2]: the InterCTC encoder returns four values
        logits, _, _ = self._head(enc, enc_len, want_logits=True)
        tokens, token_len, _ = self.decode_logits_beam(logits, enc_len, beam)
        tokens, token_len = tokens[:, 0].cpu(), token_len[:, 0].cpu()          # one D2H copy per batch
        return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]

    def beam_search_decoding(self, x, x_len, beam_size=None):
        """Reference name and signature (model_ctc.py:138).  ``tokenizer.decode(list_of_id_lists)`` of the best beam when a tokenizer
        is attached (model_ctc.py:181), otherwise the id lists.  Without the n-gram terms: the ``ngram_*`` and ``lm_*`` entries of
        decoding_params are ignored."""
        ids = self.beam_labels(x, x_len, beam_size)
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    # ------------------------------------------------------------------ beam search with the neural LM fused into it
    def _fusion(self, lm, lm_weight, lm_tmp, length_bonus):
        """(lm or None, weight, lm_tmp, bonus) a fused search runs with: the arguments, else the attributes.  lm None: nothing to fuse (no LM, or weight
        0) - then a non-zero bonus is an error, there is no total to add it to.  A negative or non-finite weight with an LM, lm_tmp <= 0 and a non-finite
        bonus raise ValueError."""
        lm = self.lm if lm is None else lm
        weight = float(self.lm_weight if lm_weight is None else lm_weight)
        ltmp = float(self.lm_tmp if lm_tmp is None else lm_tmp)
        bonus = float(length_bonus)
        if not -float("inf") < bonus < float("inf"):
            raise ValueError("length_bonus must be finite; got %r" % (bonus,))
        if lm is None or weight == 0:
            if bonus != 0:
                raise ValueError("length_bonus needs a fused search: a LanguageModel and lm_weight > 0 (rescore_nbest takes a bonus without an LM)")
            return None, 0.0, ltmp, 0.0
        if not 0 < weight < float("inf"):
            raise ValueError("lm_weight must be >= 0 and finite; got %r" % (weight,))
        if not 0 < ltmp < float("inf"):
            raise ValueError("lm_tmp must be > 0 and finite; got %r" % (ltmp,))
        return lm, weight, ltmp, bonus

    def decode_logits_beam_lm(self, logits: torch.Tensor, logits_len: Optional[torch.Tensor], beam_size: Optional[int] = None, lm=None,
                              lm_weight: Optional[float] = None, lm_tmp: Optional[float] = None, length_bonus: float = 0.0):
        """CTC prefix beam search with the LanguageModel fused INTO the search (effconf_ctc_beam_lm): every frame's candidates are
        ranked by total = am_score + lm_weight * lm_score + length_bonus * token_len, lm_score = the LM's log-probability of the prefix ->
        (tokens (B, beam, T) i32, token_len (B, beam) i32, total, am_score, lm_score (B, beam) f32), ranked by total.  lm / lm_weight / lm_tmp None:
        ``self.lm`` / ``decoding_params["lm_weight"]`` / ``decoding_params["lm_tmp"]``.  With no LM or weight 0 (and bonus 0) it is
        ``decode_logits_beam`` through the plain entry: total = am_score, lm_score 0.  The batch is split into chunks whose workspace stays under
        ``BEAM_LM_WORKSPACE_CAP`` (rows are independent).  The call synchronises once per round (``last_beam_rounds``): not while a stream is captured."""
        lm, weight, ltmp, bonus = self._fusion(lm, lm_weight, lm_tmp, length_bonus)
        if lm is None:
            tokens, token_len, score = self.decode_logits_beam(logits, logits_len, beam_size)
            return tokens, token_len, score.clone(), score, torch.zeros_like(score)
        beam = int(self.beam_size if beam_size is None else beam_size)
        if logits.dim() != 3:
            raise _lib.EffconfError("logits must be (batch, frames, vocab); got shape %s" % (tuple(logits.shape),))
        b, t, v = logits.shape
        self._check_beam(beam, v)
        _native.require_hip(logits)
        _native.require_hip(lm.fc.weight)
        if lm._cfg[0] != v:
            raise _lib.EffconfError("the LM's vocab_size is %d, the logits have %d entries" % (lm._cfg[0], v))
        lib = _lib.load()
        dev = logits.device
        with torch.cuda.device(dev):
            lm._ensure()
            size = lambda n: _native.sized(lib, "effconf_ctc_beam_lm", lib.effconf_ctc_beam_lm_workspace_bytes(lm._handle, n, t, v, beam),
                                           batch=n, T=t, vocab=v, beam=beam)
            step = max(1, b)
            while step > 1 and size(step) > BEAM_LM_WORKSPACE_CAP:
                step = (step + 1) // 2
            logits = logits.contiguous().float()
            logits_len = _native.lengths(logits_len, b, t, dev)
            tokens = torch.empty(b, beam, t, dtype=torch.int32, device=dev)
            token_len = torch.empty(b, beam, dtype=torch.int32, device=dev)
            total, am, lms = (torch.empty(b, beam, dtype=torch.float32, device=dev) for _ in range(3))
            stream = torch.cuda.current_stream(dev).cuda_stream
            chunks, rounds_all = [], []
            rounds = C.c_int32(0)
            for lo in range(0, b, step):
                n = min(step, b - lo)
                ws = _native.workspace(size(n), dev)
                at = lambda x: x[lo:].data_ptr() if x.numel() else x.data_ptr()
                _lib.check(lib.effconf_ctc_beam_lm(lm._handle, at(logits), at(logits_len), n, t, v, beam, float(self.tmp), weight, ltmp, bonus,
                                                   at(tokens), at(token_len), at(total), at(am), at(lms), C.byref(rounds), ws.data_ptr(), ws.numel(),
                                                   stream), "ctc_beam_lm")
                chunks.append((ws, n))
                rounds_all.append(int(rounds.value))
        self._beam_ws = (chunks, b, t, beam, 2 * lm._cfg[2] * lm._cfg[1] + v)
        self._beam_rounds = rounds_all
        return tokens, token_len, total, am, lms

    def last_beam_rounds(self) -> Optional[List[int]]:
        """Search launches of the last ``decode_logits_beam_lm`` call, one entry per chunk of the batch (an LM step ran between two of them); None after
        a plain search, which is one launch."""
        return self._beam_rounds

    def beam_labels_fused(self, x: torch.Tensor, x_len: Optional[torch.Tensor], beam_size: Optional[int] = None, from_mel: bool = False,
                          lm=None, lm_weight: Optional[float] = None, length_bonus: float = 0.0) -> List[List[int]]:
        """``beam_labels`` with the attached LanguageModel fused into the search (``decode_logits_beam_lm``): the label-id sequence of the best total
        per utterance.  With no LM attached or lm_weight == 0 (and bonus 0): exactly ``beam_labels``' result."""
        if self._fusion(lm, lm_weight, None, length_bonus)[0] is None:
            return self.beam_labels(x, x_len, beam_size, from_mel)
        beam = int(self.beam_size if beam_size is None else beam_size)
        self._check_beam(beam, self.fc.out_features)
        logits, _, _, enc_len = self._logits(x, x_len, from_mel)
        tokens, token_len = self.decode_logits_beam_lm(logits, enc_len, beam, lm, lm_weight, None, length_bonus)[:2]
        tokens, token_len = tokens[:, 0].cpu(), token_len[:, 0].cpu()          # one D2H copy per batch
        return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]

    def beam_search_fused(self, x, x_len, beam_size=None):
        """``beam_search_decoding`` through ``beam_labels_fused``: strings when a tokenizer is attached, otherwise the id lists."""
        ids = self.beam_labels_fused(x, x_len, beam_size)
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    # ------------------------------------------------------------------ n-best rescoring with a neural LM
    def rescore_nbest(self, tokens: torch.Tensor, token_len: torch.Tensor, am_score: torch.Tensor, lm=None, lm_weight: Optional[float] = None,
                      length_bonus: float = 0.0):
        """Rescore the ranked n-best of ``decode_logits_beam`` (tokens (B, beam, T) i32, token_len (B, beam) i32, am_score (B, beam) f32) with a
        ``LanguageModel`` (`lm`, else ``self.lm``): all B * beam hypotheses go through csrc/lm.hip together ->
        (best_rank (B,) i64, total (B, beam) f32, lm_score (B, beam) f32) on the device, total = am_score + lm_weight * lm_score +
        length_bonus * token_len in fp32.  Ranks with am_score = -inf (no hypothesis) are excluded; ties go to the lower rank.  With no LM or
        lm_weight == 0 the LM is not run: lm_score is 0 and total = am_score + length_bonus * token_len.  `lm_weight` None:
        ``decoding_params["lm_weight"]``; the LM's temperature is ``decoding_params["lm_tmp"]``.  The hypotheses go to the LM at their
        padded width T without a copy of the lengths to the host: positions at or beyond the longest hypothesis cost launches whose waves return
        at once (csrc/lm.hip), no weight or state traffic."""
        lm = self.lm if lm is None else lm
        w = float(self.lm_weight if lm_weight is None else lm_weight)
        if tokens.dim() != 3 or token_len.shape != tokens.shape[:2] or am_score.shape != tokens.shape[:2]:
            raise _lib.EffconfError("n-best: tokens (B, beam, T), token_len (B, beam), am_score (B, beam); got %s, %s, %s"
                                    % (tuple(tokens.shape), tuple(token_len.shape), tuple(am_score.shape)))
        b, beam, t = tokens.shape
        am = am_score.float()
        if lm is None or w == 0.0:
            lm_score = torch.zeros_like(am)
        else:
            lm_score = lm.score(tokens.reshape(b * beam, t), token_len.reshape(b * beam), lm_tmp=self.lm_tmp).reshape(b, beam)
        best, total = select_nbest(am, lm_score, token_len, w, length_bonus)
        return best, total, lm_score

    def beam_labels_rescored(self, x: torch.Tensor, x_len: Optional[torch.Tensor], beam_size: Optional[int] = None, from_mel: bool = False,
                             lm=None, lm_weight: Optional[float] = None, length_bonus: float = 0.0) -> List[List[int]]:
        """``beam_labels`` with the n-best rescored by the attached LanguageModel (``rescore_nbest``): the label-id sequence of the best total
        score per utterance.  With no LM attached or lm_weight == 0: exactly ``beam_labels``' result."""
        lm = self.lm if lm is None else lm
        w = float(self.lm_weight if lm_weight is None else lm_weight)
        if lm is None or w == 0.0:
            return self.beam_labels(x, x_len, beam_size, from_mel)
        beam = int(self.beam_size if beam_size is None else beam_size)
        self._check_beam(beam, self.fc.out_features)
        logits, _, _, enc_len = self._logits(x, x_len, from_mel)
        tokens, token_len, score = self.decode_logits_beam(logits, enc_len, beam)
        best, _, _ = self.rescore_nbest(tokens, token_len, score, lm, w, length_bonus)
        idx = torch.arange(tokens.shape[0], device=tokens.device)
        tokens, token_len = tokens[idx, best].cpu(), token_len[idx, best].cpu()      # one D2H copy per batch
        return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]

    def beam_search_rescored(self, x, x_len, beam_size=None):
        """``beam_search_decoding`` through ``beam_labels_rescored``: strings when a tokenizer is attached, otherwise the id lists."""
        ids = self.beam_labels_rescored(x, x_len, beam_size)
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    # ------------------------------------------------------------------ forced alignment, transcript scoring
    def _targets(self, y, y_len, device):
        """(targets (B, U) i32, target_len (B,) i64) on `device` from a padded integer tensor + lengths, a list of id lists, or a list of
        strings (needs a tokenizer).  A list is padded on the host and copied once."""
        return _targets.targets(self.tokenizer, y, y_len, device)

    def _ids(self, y):
        """Strings -> id lists through the tokenizer; anything else as it is."""
        return _targets.ids(self.tokenizer, y)

    def align_logits(self, logits: torch.Tensor, logits_len: Optional[torch.Tensor], targets, target_len=None, scores_only: bool = False):
        """Forced alignment of head logits (B, T, V) fp32 to `targets` ((B, U) integers + `target_len`, or a list of id lists) on the GPU
        (effconf_ctc_align), temperature ``self.tmp`` -> dict of device tensors: ``log_likelihood`` (B,) f32 = log P(target | logits),
        ``status`` (B,) i32 and, unless `scores_only`, ``score`` (B,) f32 = log-probability of the best path, ``frame_token`` (B, T) i32
        (target index per frame, -1 blank / beyond the length), ``token_start`` / ``token_end`` (B, U) i32 (first frame, last frame + 1) and
        ``token_logp`` (B, U) f32.  include/effconf.h has the details."""
        if logits.dim() != 3:
            raise _lib.EffconfError("logits must be (batch, frames, vocab); got shape %s" % (tuple(logits.shape),))
        b, t, v = logits.shape
        if not 2 <= v <= 1024:
            raise _lib.EffconfError("vocab_size must be in 2 .. 1024 for the CTC alignment; got %d" % v)
        if not 0 < self.tmp < float("inf"):
            raise _lib.EffconfError("decoding_params['tmp'] must be > 0; got %r" % (self.tmp,))
        _native.require_hip(logits)
        dev = logits.device
        tg, tl = self._targets(targets, target_len, dev)
        if tg.shape[0] != b or tl.shape[0] != b:
            raise _lib.EffconfError("targets: %d rows for %d utterances" % (tg.shape[0], b))
        u = int(tg.shape[1])
        if u > 2047:
            raise _lib.EffconfError("at most 2047 target tokens per utterance; got %d" % u)
        lib = _lib.load()
        nbytes = _native.sized(lib, "effconf_ctc_align", lib.effconf_ctc_align_workspace_bytes(b, t, v, u), batch=b, T=t, vocab=v, U=u)
        with torch.cuda.device(dev):
            logits = logits.contiguous().float()
            logits_len = _native.lengths(logits_len, b, t, dev)
            out = {"log_likelihood": torch.empty(b, dtype=torch.float32, device=dev), "status": torch.empty(b, dtype=torch.int32, device=dev)}
            if not scores_only:
                out["score"] = torch.empty(b, dtype=torch.float32, device=dev)
                out["frame_token"] = torch.empty(b, t, dtype=torch.int32, device=dev)
                out["token_start"] = torch.empty(b, u, dtype=torch.int32, device=dev)
                out["token_end"] = torch.empty(b, u, dtype=torch.int32, device=dev)
                out["token_logp"] = torch.empty(b, u, dtype=torch.float32, device=dev)
            ws = _native.workspace(nbytes, dev)
            ptr = lambda k: out[k].data_ptr() if k in out else None
            _lib.check(lib.effconf_ctc_align(logits.data_ptr(), logits_len.data_ptr(), b, t, v, tg.data_ptr(), tl.data_ptr(), u, float(self.tmp),
                                             ptr("log_likelihood"), ptr("score"), ptr("status"), ptr("frame_token"), ptr("token_start"),
                                             ptr("token_end"), ptr("token_logp"), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream(dev).cuda_stream), "ctc_align")
        return out

    def _logits(self, x, x_len, from_mel):
        _native.require_hip(x)
        enc, enc_len = (self.encoder.forward_mel(x, x_len) if from_mel else self.encoder(x, x_len))[:2]      # [:2]: the InterCTC encoder returns four values
        return self._head(enc, enc_len, want_logits=True) + (enc_len,)

    def _records(self, out, tg, tl) -> List[Alignment]:
        fs = self.encoder.frame_seconds
        host = {k: v.cpu() for k, v in out.items()}                     # one D2H copy per batch (per output tensor)
        tg, tl = tg.cpu(), tl.cpu()
        recs = []
        for i in range(tg.shape[0]):
            n = max(0, min(int(tl[i]), tg.shape[1]))
            st, en = host["token_start"][i, :n].tolist(), host["token_end"][i, :n].tolist()
            recs.append(Alignment(tg[i, :n].tolist(), st, en, [f * fs for f in st], [f * fs for f in en], host["token_logp"][i, :n].tolist(),
                                  float(host["score"][i]), float(host["log_likelihood"][i]), int(host["status"][i])))
        return recs

    def align(self, x: torch.Tensor, x_len: Optional[torch.Tensor], y, y_len=None, from_mel: bool = False) -> List[Alignment]:
        """Token timestamps of known transcripts: encoder, head logits, effconf_ctc_align -> one ``Alignment`` per utterance.  `y`: a padded
        (B, U) integer tensor (+ `y_len`), a list of id lists, or a list of strings when a tokenizer is attached."""
        y = self._ids(y)
        logits, _, _, enc_len = self._logits(x, x_len, from_mel)
        tg, tl = self._targets(y, y_len, logits.device)
        return self._records(self.align_logits(logits, enc_len, tg, tl), tg, tl)

    def score_labels(self, x: torch.Tensor, x_len: Optional[torch.Tensor], y, y_len=None, from_mel: bool = False) -> torch.Tensor:
        """log P(y | x) of every utterance, (B,) fp32 on the device (-inf where the transcript cannot be aligned): the CTC forward algorithm
        alone (no Viterbi pass, no backpointers), = -ctc_loss(log_softmax(logits / tmp)) without the copy of the logits to the host."""
        y = self._ids(y)
        logits, _, _, enc_len = self._logits(x, x_len, from_mel)
        return self.align_logits(logits, enc_len, y, y_len, scores_only=True)["log_likelihood"]

    def greedy_alignment(self, x: torch.Tensor, x_len: Optional[torch.Tensor], from_mel: bool = False) -> List[Alignment]:
        """The greedy labels with their timestamps: ``align`` on the greedy labels of the same logits (one encoder pass, one head pass)."""
        logits, labels, label_len, enc_len = self._logits(x, x_len, from_mel)
        u = min(int(labels.shape[1]), 2047)
        tg, tl = labels[:, :u].contiguous(), label_len.to(torch.int64)
        return self._records(self.align_logits(logits, enc_len, tg, tl), tg, tl)


class InterCTC(ModelCTC):
    """The reference's ``InterCTC`` model (models/model_ctc.py:183-215; ``model_type: "InterCTC"``): a CTC model on ``ConformerEncoderInterCTC`` -
    self-conditioned CTC after the blocks of ``encoder_params["interctc_blocks"]``, with ``vocab_size`` taken from the tokenizer params.
    ``forward(batch)`` returns the reference's four values (logits, lengths, attentions, interctc_probs); every decoder of ``ModelCTC`` - greedy,
    ``greedy_exact``, beam search, rescoring, ``align``, ``score_labels``, ``greedy_alignment`` - is inherited unchanged: they read the encoder's output
    rows only.  Training (``LossInterCTC``) is out of scope, as for ``ModelCTC``."""
    _encoder_cls = ConformerEncoderInterCTC

    def __init__(self, encoder_params: dict, tokenizer_params: dict, training_params: Optional[dict] = None,
                 decoding_params: Optional[dict] = None, name: str = "model", tokenizer=None):
        encoder_params = dict(encoder_params)
        encoder_params["vocab_size"] = tokenizer_params["vocab_size"]          # model_ctc.py:189
        super().__init__(encoder_params, tokenizer_params, training_params, decoding_params, name, tokenizer)

    def forward(self, batch, return_attentions: bool = False, return_interctc: bool = True):
        x, _, x_len, _ = batch
        enc, enc_len, attentions, interctc_probs = self.encoder(x, x_len, return_attentions=return_attentions, return_interctc=return_interctc)
        logits, _, _ = self._head(enc, enc_len, want_logits=True)
        return logits, enc_len, attentions, interctc_probs
