"""Chunked streaming inference of causal encoders: a session keeps, per stream and per block, the attention keys / values of the left context and the last
k - 1 inputs of the depthwise convolution (the C library's effconf_stream_*), encodes only the frames that are new, and the concatenation of its outputs is
the whole-utterance causal forward.

The session arithmetic is plain Python on the plan (no GPU, no library; tests/test_stream_host.py):
  stream_align(plan)            chunk granularity in subsampled rows (12 for Tiny and every Efficient Conformer = 24 mel frames)
  rows_to_encode(...)           the emission rule: after N mel frames of an unfinished stream N // 2 rows are complete (row t reads the mel frames
                                2 t - 1 .. 2 t + 1) and whole multiples of the alignment are encoded; a final push encodes the remaining (N - 1) // 2 + 1 - done
  cache_capacities(plan, ...)   grouped K / V rows kept per block: the band of forward_common.h (left_context // (mask_stride * group)), an unlimited
                                left_context: what max_frames gives
  ctc_collapse_carry(...)       greedy CTC collapse with the repeat carried across pushes
  beam_push_refusal(...)        why a push of the resumed beam search is refused on the host; common_prefix_len: what its stable_len is

CTC beam search: ``CtcBeamStreamState`` carries the beam and the prefix trie per stream and resumes the prefix beam search on the new logit frames
(effconf_ctc_beam_resume); ``StreamingCTCBeam`` is the encoder session, the head and that search, and returns the tokens no later frame can change.

Transducers: ``RnntStreamState`` carries the prediction network's state per stream and resumes the greedy RNN-T decode on the new encoder frames
(effconf_rnnt_greedy_resume); ``StreamingTransducer`` is the encoder session plus that decode.
"""
from __future__ import annotations

import ctypes as C
from math import gcd
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, _native

UNLIMITED = 1 << 30


# ------------------------------------------------------------------ arithmetic (host only)
def stream_refusal(plan, precision: str = "bf16", sub_batches: Optional[int] = 1) -> Optional[str]:
    """Why a plan cannot stream (None: it can).  The library repeats the checks it can see (effconf_stream_create)."""
    if not plan.causal:
        return "streaming sessions need a causal plan (causal: true): the symmetric depthwise padding and the two-sided relative positions of other plans look ahead"
    if 0 < plan.right_context < UNLIMITED:
        return "streaming sessions with lookahead (right_context > 0) are not native"
    if precision != "bf16":
        return "streaming sessions run on the bf16 path (precision %r is not native)" % precision
    if getattr(plan, "interctc_blocks", None):
        return "streaming sessions of InterCTC encoders are not native"
    if sub_batches is not None and sub_batches > 1:
        return "streaming sessions run as one row range (sub_batches > 1 is refused)"
    if plan.sub_layers != 1:
        return "streaming sessions need the one-layer subsampler (the two-layer subsampler of the plain Conformer configurations is not native here)"
    return None


def stream_align(plan) -> int:
    """Chunk granularity in subsampled rows: the least common multiple, over the blocks, of group_size x (product of the conv strides before the block) and of
    the cumulative stride behind every strided block - a chunk that is a multiple starts every block on a whole attention group and every strided block on
    an even row."""
    lcm = lambda a, b: a // gcd(a, b) * b
    l, ms = 1, 1
    for bp in plan.blocks:
        l = lcm(l, bp.group_size * ms)
        ms *= bp.conv_stride
        l = lcm(l, ms)
    return l


def rows_to_encode(frames: int, done: int, align: int, final: bool) -> int:
    """Subsampled rows a stream encodes now: `frames` mel frames received in all, `done` rows encoded before."""
    if final:
        return max(((frames - 1) // 2 + 1 if frames > 0 else 0) - done, 0)
    return max((frames // 2 - done) // align * align, 0)


def block_rows(plan, rows: int) -> List[int]:
    """Rows entering every block for `rows` subsampled rows, and (last entry) the rows leaving the encoder: T -> (T - 1) // s + 1 behind a strided block."""
    out, t = [], rows
    for bp in plan.blocks:
        out.append(t)
        if bp.conv_stride > 1 and t > 0:
            t = (t - 1) // bp.conv_stride + 1
    return out + [t]


def cache_capacities(plan, max_frames: Optional[int] = None) -> List[int]:
    """Grouped K / V rows every block keeps per stream: band(c, mask_stride, G).l of forward_common.h, capped by the grouped rows a block can see at all -
    max_pos_encoding // G, or what max_frames mel frames bring to it.  An unlimited left_context is therefore sized by max_frames."""
    rows = block_rows(plan, (max_frames - 1) // 2 + 1) if max_frames else None
    out, ms = [], 1
    for i, bp in enumerate(plan.blocks):
        cap = min(plan.left_context // (ms * bp.group_size), bp.max_pos // bp.group_size)
        out.append(cap if rows is None else min(cap, -(-rows[i] // bp.group_size)))
        ms *= bp.conv_stride
    return out


def ctc_collapse_carry(frame_labels: Sequence[int], carry: int) -> Tuple[List[int], int]:
    """Greedy CTC collapse of one push: `frame_labels` the argmax of every new frame, `carry` the label of the stream's last frame before it (0 = blank or
    none).  -> (tokens to emit, new carry).  A label equal to the previous frame's is not emitted again - across the push boundary too; blank resets."""
    out, prev = [], int(carry)
    for l in frame_labels:
        l = int(l)
        if l != 0 and l != prev:
            out.append(l)
        prev = l
    return out, prev


def merge_collapsed(labels: Sequence[int], first: int, last: int, carry: int) -> Tuple[List[int], int]:
    """The same from what the native greedy head returns for a push of at least one frame: its collapsed `labels` and the argmax of the first and of the
    last frame."""
    labels = [int(l) for l in labels]
    if first != 0 and first == carry and labels:
        labels = labels[1:]
    return labels, int(last)


# ------------------------------------------------------------------ the session
class StreamingEncoder:
    """``ConformerEncoder.open_stream``: `max_streams` independent streams; stream b is row b of every push."""

    def __init__(self, encoder, max_streams: int, max_frames: Optional[int] = None):
        why = stream_refusal(encoder.plan, encoder.precision, encoder.sub_batches)
        if why:
            raise _lib.EffconfError(why)
        if max_streams < 1:
            raise ValueError("max_streams must be >= 1")
        self.encoder, self.plan = encoder, encoder.plan
        self.max_streams, self.max_frames = int(max_streams), int(max_frames or 0)
        self.align_rows = stream_align(self.plan)
        self.align_frames = 2 * self.align_rows
        self.device = encoder._param_device()
        _native.require_hip(encoder.linear.weight)
        lib = self._lib = _lib.load()
        with torch.cuda.device(self.device):
            encoder._ensure_packed()
            self._enc_handle = encoder._handle
            nbytes = _native.sized(lib, "effconf_stream_state", lib.effconf_stream_state_bytes(encoder._handle, self.max_streams, self.max_frames),
                                   streams=self.max_streams, frames=self.max_frames)
            self._state = _native.workspace(nbytes, self.device)
            self._ptr = lib.effconf_stream_create(encoder._handle, self.max_streams, self.max_frames, self._state.data_ptr(), self._state.numel())
        if not self._ptr:
            raise _lib.EffconfError("effconf_stream_create: %s" % lib.effconf_last_error().decode())
        self._ws = None
        n_mels = self.plan.n_mels
        self._zero2 = torch.zeros(n_mels, 2, dtype=torch.float32, device=self.device)
        self._buf = [self._zero2 for _ in range(self.max_streams)]        # column c = mel frame 2 done - 2 + c (two zero columns in front of frame 0)
        self._frames = [0] * self.max_streams
        self._done = [0] * self.max_streams
        self._ended = [False] * self.max_streams
        # push_audio: samples from sample _s0 on (a multiple of the hop), frames emitted so far
        self._audio = [None] * self.max_streams
        self._s0 = [0] * self.max_streams
        self._next_frame = [0] * self.max_streams

    def close(self):
        if getattr(self, "_ptr", None) and _lib._lib is not None:
            self._lib.effconf_stream_destroy(self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames_pending(self, stream: int) -> int:
        """Mel frames of `stream` received and not yet covered by an encoded row's centre (what the alignment holds back)."""
        return self._frames[stream] - 2 * self._done[stream] if not self._ended[stream] else 0

    def reset(self, stream: int):
        """`stream` starts a new utterance."""
        _lib.check(self._lib.effconf_stream_reset(self._ptr, int(stream)), "stream_reset", self._lib)
        self._buf[stream] = self._zero2
        self._frames[stream] = self._done[stream] = 0
        self._ended[stream] = False
        self._audio[stream], self._s0[stream], self._next_frame[stream] = None, 0, 0

    def _check_handle(self):
        if self.encoder._handle != self._enc_handle:
            raise _lib.EffconfError("the encoder was packed again after open_stream (new weights, options or precision): open a new session")

    def push_mel(self, mel: torch.Tensor, mel_len, final=None):
        """mel (B, n_mels, T) with B = max_streams, mel_len[b] new frames of stream b (any number, 0 included), final[b]: the stream ends with this push.
        -> (out (B, t_new_max, D) fp32, zero behind every stream's new frames; out_len (B,) int64)."""
        self._check_handle()
        B = self.max_streams
        lens = [int(v) for v in (mel_len.tolist() if isinstance(mel_len, torch.Tensor) else mel_len)]
        final = [bool(v) for v in (final.tolist() if isinstance(final, torch.Tensor) else final)] if final is not None else [False] * B
        if mel.shape[0] != B or len(lens) != B or len(final) != B:
            raise ValueError("push_mel takes one row per stream of the session (%d)" % B)
        _native.require_hip(mel)
        mel = mel.float()
        rows = []
        for b in range(B):
            if self._ended[b] and (lens[b] or final[b]):
                raise _lib.EffconfError("stream %d has ended: reset it before it takes frames again" % b)
            if lens[b]:
                self._buf[b] = torch.cat([self._buf[b], mel[b, :, :lens[b]]], 1)
                self._frames[b] += lens[b]
            rows.append(0 if self._ended[b] else rows_to_encode(self._frames[b], self._done[b], self.align_rows, final[b]))
        active = [b for b in range(B) if rows[b] > 0]
        d_out = self.plan.blocks[-1].dim_expand
        t_new = [block_rows(self.plan, r)[-1] if r else 0 for r in rows]
        out = torch.zeros(B, max(t_new), d_out, dtype=torch.float32, device=self.device)
        out_len = torch.tensor(t_new, dtype=torch.int64, device=self.device)
        if active:
            n, rmax = len(active), max(rows)
            pitch = (2 * rmax + 2 + 7) // 8 * 8
            staged = torch.zeros(n, self.plan.n_mels, pitch, dtype=torch.float32, device=self.device)
            for i, b in enumerate(active):
                w = min(self._buf[b].shape[1], 2 * rows[b] + 2)
                staged[i, :, :w] = self._buf[b][:, :w]
            lib = self._lib
            with torch.cuda.device(self.device):
                nbytes = _native.sized(lib, "effconf_stream", lib.effconf_stream_workspace_bytes(self._ptr, n, rmax, pitch), streams=n, rows=rmax, pitch=pitch)
                if self._ws is None or self._ws.numel() < nbytes:
                    self._ws = _native.workspace(nbytes, self.device)
                o = torch.empty(n, max(t_new), d_out, dtype=torch.float32, device=self.device)
                ol = torch.empty(n, dtype=torch.int64, device=self.device)
                ids = (C.c_int32 * n)(*active)
                rws = (C.c_int32 * n)(*[rows[b] for b in active])
                _lib.check(lib.effconf_stream_push_mel(self._ptr, ids, n, staged.data_ptr(), pitch, rws, o.data_ptr(), o.shape[1], ol.data_ptr(), self._ws.data_ptr(),
                                                       self._ws.numel(), torch.cuda.current_stream(self.device).cuda_stream), "stream_push_mel", lib)
            out[active] = o
        for b in range(B):
            if rows[b]:
                self._buf[b] = self._buf[b][:, 2 * rows[b]:]
                self._done[b] += rows[b]
            if final[b]:
                self._ended[b] = True
                self._buf[b] = self._zero2
        return out, out_len

    def push_audio(self, x: torch.Tensor, x_len, final=None):
        """x (B, samples) with x_len[b] new samples of stream b.  The mel kernel runs over [kept tail | new samples] of every stream; only frames whose
        n_fft-sample window lies inside the buffer are used (in the kernel's frame pairs), so the reflect padding applies at the true start and the true end
        alone and the frames are those of the whole-signal front end, bit for bit.  -> push_mel's result."""
        self._check_handle()
        B, hop, half = self.max_streams, self.plan.hop_length, self.plan.n_fft // 2
        lens = [int(v) for v in (x_len.tolist() if isinstance(x_len, torch.Tensor) else x_len)]
        final = [bool(v) for v in (final.tolist() if isinstance(final, torch.Tensor) else final)] if final is not None else [False] * B
        _native.require_hip(x)
        new = []
        for b in range(B):
            if lens[b]:
                piece = x[b, :lens[b]].float()
                self._audio[b] = piece if self._audio[b] is None else torch.cat([self._audio[b], piece])
            buf = self._audio[b]
            L = 0 if buf is None else buf.shape[0]
            end = self._s0[b] + L                                   # samples received in all
            # global frame f is centred on sample f * hop; complete when its window ends inside the signal (final: the last frame is end // hop).  The mel kernel
            # transforms the frames (2 m, 2 m + 1) as ONE complex FFT, so a frame carries rounding of its partner: frames are taken in whole pairs, from a buffer
            # that starts on an even frame - the pairs, and so every bit, are those of the whole-signal front end
            last = end // hop if final[b] else (end - half) // hop
            if not final[b] and last % 2 == 0:
                last -= 1
            f0 = self._next_frame[b]
            if L > half and last >= f0 and end > 0:
                mel, _ = self.encoder.mel_frontend(buf[None])
                j0 = f0 - self._s0[b] // hop
                new.append(mel[0, :, j0: j0 + last - f0 + 1])
                self._next_frame[b] = last + 1
                s0 = max(((self._next_frame[b] * hop - half) // hop - 1) // 2 * 2 * hop, 0)          # an even frame; the next frame's window starts behind it
                if s0 > self._s0[b]:
                    self._audio[b] = buf[s0 - self._s0[b]:]
                    self._s0[b] = s0
            else:
                new.append(None)
        n_new = [0 if m is None else m.shape[1] for m in new]
        mel = torch.zeros(B, self.plan.n_mels, max(max(n_new), 1), dtype=torch.float32, device=self.device)
        for b, m in enumerate(new):
            if m is not None:
                mel[b, :, :m.shape[1]] = m
        self.last_mel, self.last_mel_len = mel, n_new               # what this push added (tests)
        return self.push_mel(mel, n_new, final)


class StreamingCTC:
    """``ModelCTC.open_stream``: the session plus the greedy head on the new frames, the repeat collapse carried across pushes."""

    def __init__(self, model, max_streams: int, max_frames: Optional[int] = None):
        self.model = model
        self.session = StreamingEncoder(model.encoder, max_streams, max_frames)
        self._carry = [0] * max_streams

    align_frames = property(lambda self: self.session.align_frames)

    def frames_pending(self, stream: int) -> int:
        return self.session.frames_pending(stream)

    def reset(self, stream: int):
        self.session.reset(stream)
        self._carry[stream] = 0

    def _tokens(self, out: torch.Tensor, out_len: torch.Tensor) -> List[List[int]]:
        B = out.shape[0]
        lens = out_len.tolist()
        if out.shape[1] == 0 or not any(lens):
            return [[] for _ in range(B)]
        head = lambda rows, ln: self.model._head(rows, ln)[1:]
        labels, label_len = head(out, out_len)
        one = (out_len > 0).to(torch.int64)
        first, first_n = head(out[:, :1].contiguous(), one)
        idx = (out_len - 1).clamp(min=0)
        last, last_n = head(out[torch.arange(B, device=out.device), idx][:, None].contiguous(), one)
        labels, label_len, first, first_n, last, last_n = (z.tolist() for z in (labels, label_len, first, first_n, last, last_n))
        res = []
        for b in range(B):
            if not lens[b]:
                res.append([])
                continue
            f = first[b][0] if first_n[b] else 0
            l = last[b][0] if last_n[b] else 0
            toks, self._carry[b] = merge_collapsed(labels[b][:label_len[b]], f, l, self._carry[b])
            res.append(toks)
        return res

    def push_mel(self, mel, mel_len, final=None) -> List[List[int]]:
        return self._tokens(*self.session.push_mel(mel, mel_len, final))

    def push_audio(self, x, x_len, final=None) -> List[List[int]]:
        return self._tokens(*self.session.push_audio(x, x_len, final))


# ------------------------------------------------------------------ CTC: the prefix beam search resumed per stream
def beam_push_refusal(ids: Sequence[int], new_frames: Sequence[int], consumed: Sequence[int], max_streams: int, max_frames: int) -> Optional[str]:
    """Why a push of the resumed beam search is refused on the host (None: it is not): `ids` the listed streams, `new_frames[i]` the frames listed stream i
    brings, `consumed[s]` the frames stream s has had.  Pure: no GPU, no library."""
    if len(new_frames) != len(ids):
        return "push takes one stream id per row (%d rows, %d ids)" % (len(new_frames), len(ids))
    if any(not 0 <= s < max_streams for s in ids):
        return "stream ids must be in 0 .. %d; got %s" % (max_streams - 1, list(ids))
    if len(set(ids)) != len(ids):
        return "stream ids of a push must be distinct; got %s" % (list(ids),)
    for s, k in zip(ids, new_frames):
        if k < 0 or consumed[s] + k > max_frames:
            return "stream %d would hold %d frames: the stream state was sized for max_frames = %d" % (s, consumed[s] + k, max_frames)
    return None


def common_prefix_len(hyps: Sequence[Sequence[int]]) -> int:
    """Length of the longest common prefix of token strings: what ``stable_len`` is for the members of a beam."""
    if not hyps:
        return 0
    n = min(len(h) for h in hyps)
    for i in range(n):
        if any(h[i] != hyps[0][i] for h in hyps):
            return i
    return n


class CtcBeamStreamState:
    """``ModelCTC.open_beam_decode_stream``: the beam of `max_streams` streams (per stream the members' record and the stream's prefix trie, in one device
    buffer this object owns: include/effconf.h has the layout) and the CTC prefix beam search resumed from it, push by push (effconf_ctc_beam_resume).  The
    beam of a stream, whatever its push pattern, is bit for bit that of one ``decode_logits_beam`` of the same frames.  `max_frames`: logit frames (encoder
    output rows) a stream can take before it is reset - the trie only grows.  Not built: LM fusion in a streaming search (``decode_logits_beam_lm`` is
    whole-utterance only), a streaming RNN-T beam search, trie compaction for unbounded streams."""

    def __init__(self, model, max_streams: int, max_frames: int, beam_size: Optional[int] = None, device=None):
        if max_streams < 1:
            raise ValueError("max_streams must be >= 1")
        if max_frames is None or max_frames < 1:
            raise ValueError("max_frames must be >= 1: the stream's prefix trie is sized by it")
        self.model, self.max_streams, self.max_frames = model, int(max_streams), int(max_frames)
        self.beam = int(model.beam_size if beam_size is None else beam_size)
        model._check_beam(self.beam, model.fc.out_features)
        if device is None:
            _native.require_hip(model.fc.weight)
            device = model.fc.weight.device
        self.device = torch.device(device)
        lib = self._lib = _lib.load()
        nbytes = _native.sized(lib, "effconf_ctc_beam_stream_state", lib.effconf_ctc_beam_stream_state_bytes(self.max_streams, self.max_frames, self.beam),
                               streams=self.max_streams, frames=self.max_frames, beam=self.beam)
        self.state = _native.workspace(nbytes, self.device)
        self._frames = [0] * self.max_streams
        self._ws, self._last = None, None
        self.init()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def init(self):
        """Every stream starts a new utterance (only the flags are written: a record whose flag is clear is never read)."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.effconf_ctc_beam_stream_init(self.state.data_ptr(), self.state.numel(), self.max_streams, self.max_frames, self.beam,
                                                              self._stream()), "ctc_beam_stream_init", self._lib)
        self._frames = [0] * self.max_streams

    def reset(self, stream: int):
        """`stream` starts a new utterance."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.effconf_ctc_beam_stream_reset(self.state.data_ptr(), self.max_streams, int(stream), self._stream()),
                       "ctc_beam_stream_reset", self._lib)
        self._frames[stream] = 0

    def frames(self, stream: int) -> int:
        """Logit frames `stream` has consumed since its last reset (host counter)."""
        return self._frames[stream]

    def state_views(self):
        """(primed (S,) i32, records (S, 240) i32): views of the state buffer (tests)."""
        up = lambda x: (x + 255) // 256 * 256
        S, off = self.max_streams, (-self.state.data_ptr()) % 256
        ncap = 1 + self.beam * self.max_frames
        h = 1
        while h < 2 * ncap:
            h <<= 1
        per = up(960) + up(16 * ncap) + up(8 * h) + up(4 * h)
        primed = self.state[off: off + 4 * S].view(torch.int32)
        lo = off + up(4 * S)
        blocks = self.state[lo: lo + S * per].view(S, per)
        return primed, blocks[:, :960].view(torch.int32)

    def push(self, logits: torch.Tensor, logits_len, streams: Optional[Sequence[int]] = None, nbest: Optional[int] = None):
        """logits (n, t_new, V) fp32 on the GPU: logits_len[i] new frames of stream streams[i] (default 0 .. n - 1; distinct ids; 0 frames: the stream's beam
        is read, not changed) -> device tensors (tokens (n, nbest, max_tokens) i32 with zero tails, token_len (n, nbest) i32, score (n, nbest) f32, stable_len
        (n,) i32), the beam after the push, best first; nbest None: the whole beam.  max_tokens = the most frames a listed stream has consumed (at least 1), so
        nothing is truncated.  stable_len: the length of the common prefix of ALL members of the beam - these tokens are final.  Ids out of range, repeated ids
        and a push past max_frames raise ValueError before any launch (the lengths are read on the host)."""
        if logits.dim() != 3:
            raise _lib.EffconfError("logits must be (streams, frames, vocab); got shape %s" % (tuple(logits.shape),))
        n, t, v = logits.shape
        self.model._check_beam(self.beam, v)
        ids = list(range(n)) if streams is None else [int(s) for s in streams]
        lens = [t] * n if logits_len is None else [int(x) for x in (logits_len.tolist() if isinstance(logits_len, torch.Tensor) else logits_len)]
        lens = [min(max(k, 0), t) for k in lens]
        why = beam_push_refusal(ids, lens, self._frames, self.max_streams, self.max_frames)
        if why:
            raise ValueError(why)
        return self._launch(logits, lens, ids, int(self.beam if nbest is None else nbest))

    def _launch(self, logits, lens, ids, nbest, out=None, max_tokens=None):
        """``push`` behind its host checks of the ids and the capacity: the kernel's own guards answer a bad id with token_len -1 and a push past max_frames
        with -2 and leave the state alone.  `out`: the four output tensors to write instead of fresh ones, `max_tokens` their width (tests)."""
        _native.require_hip(logits)
        lib, dev = self._lib, self.device
        n, t, v = logits.shape
        if not 1 <= nbest <= self.beam:
            raise _lib.EffconfError("nbest must be in 1 .. beam (%d); got %d" % (self.beam, nbest))
        if max_tokens is None:
            max_tokens = max([1] + [self._frames[s] + k for s, k in zip(ids, lens) if 0 <= s < self.max_streams])
        with torch.cuda.device(dev):
            logits = logits.contiguous().float()
            tokens, token_len, score, stable = out if out is not None else (
                torch.empty(n, nbest, max_tokens, dtype=torch.int32, device=dev), torch.empty(n, nbest, dtype=torch.int32, device=dev),
                torch.empty(n, nbest, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            ln = torch.tensor(lens, dtype=torch.int64, device=dev)
            idt = torch.tensor(ids, dtype=torch.int32, device=dev)
            nbytes = _native.sized(lib, "effconf_ctc_beam_stream", lib.effconf_ctc_beam_stream_workspace_bytes(n, t, self.beam), streams=n, frames=t, beam=self.beam)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = _native.workspace(nbytes, dev)
            _lib.check(lib.effconf_ctc_beam_resume(self.state.data_ptr(), self.max_streams, self.max_frames, self.beam, idt.data_ptr(),
                                                   logits.data_ptr() if t > 0 and n > 0 else None, ln.data_ptr(), n, t, v, float(self.model.tmp), nbest,
                                                   tokens.data_ptr(), token_len.data_ptr(), score.data_ptr(), stable.data_ptr(), max_tokens,
                                                   self._ws.data_ptr(), self._ws.numel(), self._stream()), "ctc_beam_resume", lib)
        took = [0 <= s < self.max_streams and self._frames[s] + k <= self.max_frames for s, k in zip(ids, lens)]
        self._last = (n, t, [k if ok else None for k, ok in zip(lens, took)])
        for s, k, ok in zip(ids, lens, took):
            if ok:
                self._frames[s] += k
        return tokens, token_len, score, stable

    def last_push_trace(self) -> List[Optional[dict]]:
        """The workspace of the last push (layout: include/effconf.h), one dict per listed stream as ``ModelCTC.last_beam_trace`` gives per utterance, for the
        push's frames: ``len`` (frames of the push), ``candidates`` / ``nodes`` (candidates scored / trie nodes of the stream so far), ``frames`` (frames
        consumed so far), ``node`` (len, beam) i32 and ``pb`` / ``pnb`` / ``score`` (len, beam) f32.  None for a listed stream the kernel's guards turned away."""
        import numpy as np
        n, t, lens = self._last
        al = lambda x: (x + 255) // 256 * 256
        base = (-self._ws.data_ptr()) % 256
        raw = self._ws[base: base + al(16 * n) + n * al(16 * t * self.beam)].cpu().numpy()
        stats = raw[:16 * n].view(np.int32).reshape(n, 4)
        out = []
        for i in range(n):
            if lens[i] is None:
                out.append(None)
                continue
            u = al(16 * n) + i * al(16 * t * self.beam)
            tr = raw[u: u + 16 * t * self.beam].view(np.int32).reshape(t, self.beam, 4)[:int(stats[i, 0])]
            trf = tr.view(np.float32)
            out.append({"len": int(stats[i, 0]), "candidates": int(stats[i, 1]), "nodes": int(stats[i, 2]), "frames": int(stats[i, 3]),
                        "node": tr[:, :, 0].copy(), "pb": trf[:, :, 1].copy(), "pnb": trf[:, :, 2].copy(), "score": trf[:, :, 3].copy()})
        return out


class StreamingCTCBeam:
    """``ModelCTC.open_stream(..., beam_size=k)``: the encoder session, the head's logits on the push's rows, and the prefix beam search resumed over the streams
    that received rows.  ``push_mel`` / ``push_audio`` return, per stream, the NEWLY COMMITTED token ids - the growth of the beam's common prefix, which no later
    frame can change - and at a stream's final push also the rest of the best hypothesis: the concatenation over an utterance's pushes is its final best
    hypothesis, and it is that of ``decode_logits_beam`` on the concatenation of the session's own logits.  Not built: LM fusion in a streaming search, trie
    compaction for unbounded streams (so `max_frames` is required)."""

    def __init__(self, model, max_streams: int, max_frames: Optional[int], beam_size: int):
        if max_frames is None or max_frames < 1:
            raise ValueError("a streaming beam search needs max_frames (mel frames per utterance): the prefix trie of a stream only grows and is sized by the "
                             "encoder rows that many frames can produce")
        self.model = model
        self.session = StreamingEncoder(model.encoder, max_streams, max_frames)       # refuses what cannot stream (stream_refusal) before any device work
        rows = block_rows(model.encoder.plan, (int(max_frames) - 1) // 2 + 1)[-1]
        self.decoder = CtcBeamStreamState(model, max_streams, max(rows, 1), beam_size, device=self.session.device)
        self._committed = [[] for _ in range(max_streams)]
        self._hyp = [[([], 0.0)] for _ in range(max_streams)]
        self.last_push_logits = None

    align_frames = property(lambda self: self.session.align_frames)

    def frames_pending(self, stream: int) -> int:
        return self.session.frames_pending(stream)

    def reset(self, stream: int):
        """`stream` starts a new utterance."""
        self.session.reset(stream)
        self.decoder.reset(stream)
        self._committed[stream], self._hyp[stream] = [], [([], 0.0)]

    def committed(self, stream: int) -> List[int]:
        """The tokens returned so far: final."""
        return list(self._committed[stream])

    def hypothesis(self, stream: int) -> List[int]:
        """Rank 0 of the beam as it stands (it begins with ``committed``)."""
        return list(self._hyp[stream][0][0])

    def nbest(self, stream: int) -> List[Tuple[List[int], float]]:
        """[(ids, score)] of the beam as it stands, best first."""
        return [(list(ids), sc) for ids, sc in self._hyp[stream]]

    def text(self, stream: int) -> str:
        if self.model.tokenizer is None:
            raise _lib.EffconfError("text() needs a tokenizer attached to the model")
        return self.model.tokenizer.decode([self.hypothesis(stream)])[0]

    def _decode(self, out: torch.Tensor, out_len: torch.Tensor, final) -> List[List[int]]:
        B = out.shape[0]
        lens = out_len.tolist()
        final = [False] * B if final is None else [bool(v) for v in (final.tolist() if isinstance(final, torch.Tensor) else final)]
        new = [[] for _ in range(B)]
        active = [b for b in range(B) if lens[b] > 0]
        self.last_push_logits = None
        if active:
            ix = torch.tensor(active, dtype=torch.int64, device=out.device)
            alen = out_len[ix].contiguous()
            logits, _, _ = self.model._head(out[ix].contiguous(), alen, want_logits=True)
            self.last_push_logits = (logits, alen, list(active))
            tokens, token_len, score, stable = (z.tolist() for z in self.decoder.push(logits, [lens[b] for b in active], active))
            for i, b in enumerate(active):
                self._hyp[b] = [(tokens[i][r][:token_len[i][r]], score[i][r]) for r in range(len(score[i])) if score[i][r] != float("-inf") or r == 0]
                best = self._hyp[b][0][0]
                new[b] = best[len(self._committed[b]): stable[i]]
                self._committed[b] += new[b]
        for b in range(B):
            if final[b]:
                rest = self._hyp[b][0][0][len(self._committed[b]):]
                new[b] = new[b] + rest
                self._committed[b] += rest
        return new

    def push_mel(self, mel, mel_len, final=None) -> List[List[int]]:
        """``StreamingEncoder.push_mel``, the head, then the resumed search of the new rows -> the newly committed token ids per stream."""
        return self._decode(*self.session.push_mel(mel, mel_len, final), final)

    def push_audio(self, x, x_len, final=None) -> List[List[int]]:
        return self._decode(*self.session.push_audio(x, x_len, final), final)


# ------------------------------------------------------------------ RNN-T: the greedy decode resumed per stream
class RnntStreamState:
    """``Transducer.open_decode_stream``: the prediction network's state of `max_streams` streams (per stream h, c, linear_decoder(h) and one flag, in one
    device buffer this object owns: include/effconf.h has the layout) and the greedy decode resumed from it, push by push (effconf_rnnt_greedy_resume).  The
    tokens of a stream, whatever its push pattern, are those of one ``decode_encoded`` of the same frames on the per-utterance kernel."""

    def __init__(self, model, max_streams: int):
        if max_streams < 1:
            raise ValueError("max_streams must be >= 1")
        self.model, self.max_streams = model, int(max_streams)
        weight = model.joint_network.linear_joint.weight
        _native.require_hip(weight)
        self.device = weight.device
        lib = self._lib = _lib.load()
        with torch.cuda.device(self.device):
            model._ensure_rnnt()
            self._handle, self._generation = model._rnnt, model._rnnt_generation
            nbytes = _native.sized(lib, "effconf_rnnt_stream_state", lib.effconf_rnnt_stream_state_bytes(self._handle, self.max_streams), streams=self.max_streams)
            self.state = _native.workspace(nbytes, self.device)
            self.init()
        self._ws = None

    def _check_handle(self):
        if not self.model._rnnt_packed or self.model._rnnt_generation != self._generation:
            raise _lib.EffconfError("the decoder was packed again after open_decode_stream (new weights): open a new decode stream")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def init(self):
        """Every stream starts a new utterance (only the flags are written: a record whose flag is clear is never read)."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.effconf_rnnt_stream_init(self._handle, self.state.data_ptr(), self.state.numel(), self.max_streams, self._stream()),
                       "rnnt_stream_init", self._lib)

    def reset(self, stream: int):
        """`stream` starts a new utterance."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.effconf_rnnt_stream_reset(self._handle, self.state.data_ptr(), self.max_streams, int(stream), self._stream()),
                       "rnnt_stream_reset", self._lib)

    def state_views(self):
        """(h (S, H), c (S, H), gd (S, J) fp32, primed (S,) i32): views of the state buffer (tests)."""
        _, H, J, _, _ = self.model._cfg
        up = lambda x: (x + 255) // 256 * 256
        S, off = self.max_streams, (-self.state.data_ptr()) % 256
        primed = self.state[off: off + 4 * S].view(torch.int32)
        rec_bytes = up(4 * (2 * H + J))
        lo = off + up(4 * S)
        rec = self.state[lo: lo + S * rec_bytes].view(torch.float32).view(S, rec_bytes // 4)
        return rec[:, :H], rec[:, H: 2 * H], rec[:, 2 * H: 2 * H + J], primed

    def push(self, f: torch.Tensor, f_len, streams: Optional[Sequence[int]] = None):
        """f (n, t_new, Denc) fp32 on the GPU: f_len[i] new encoder frames of stream streams[i] (default 0 .. n - 1; distinct ids) -> device tensors (tokens (n,
        max_tok) i32 zero behind token_len, token_frames (n, max_tok) i32 the push-local frame of every token and -1 behind them, token_len (n,) i32,
        decoder_steps (n,) i32 the prediction-network steps this push ran)."""
        if f.dim() != 3:
            raise _lib.EffconfError("encoder outputs must be (streams, frames, dim); got shape %s" % (tuple(f.shape),))
        n = f.shape[0]
        ids = list(range(n)) if streams is None else [int(s) for s in streams]
        if len(ids) != n:
            raise ValueError("push takes one stream id per row (%d rows, %d ids)" % (n, len(ids)))
        if any(not 0 <= s < self.max_streams for s in ids):
            raise ValueError("stream ids must be in 0 .. %d; got %s" % (self.max_streams - 1, ids))
        if len(set(ids)) != n:
            raise ValueError("stream ids of a push must be distinct; got %s" % (ids,))
        return self._launch(f, f_len, ids)

    def _launch(self, f, f_len, ids, out=None):
        """``push`` behind its host checks of the ids.  `out`: the four output tensors to write instead of fresh ones (tests)."""
        self._check_handle()
        _native.require_hip(f)
        lib, dev = self._lib, self.device
        f = f.contiguous().float()
        n, t, _ = f.shape
        with torch.cuda.device(dev):
            max_tok = int(lib.effconf_rnnt_max_tokens(self._handle, t))
            if n == 0 or t == 0:              # nothing to launch: no token, no step
                return (torch.zeros(n, max_tok, dtype=torch.int32, device=dev), torch.full((n, max_tok), -1, dtype=torch.int32, device=dev),
                        torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
            # the kernel writes every element of the four for every listed stream
            tokens, token_frames, token_len, steps = out if out is not None else (
                torch.empty(n, max_tok, dtype=torch.int32, device=dev), torch.empty(n, max_tok, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            f_len = _native.lengths(f_len, n, t, dev)
            idt = torch.tensor(ids, dtype=torch.int32, device=dev)
            nbytes = _native.sized(lib, "effconf_rnnt_stream", lib.effconf_rnnt_stream_workspace_bytes(self._handle, n, t), streams=n, frames=t)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = _native.workspace(nbytes, dev)
            _lib.check(lib.effconf_rnnt_greedy_resume(self._handle, self.state.data_ptr(), self.max_streams, idt.data_ptr(), f.data_ptr(), f_len.data_ptr(), n, t,
                                                      tokens.data_ptr(), token_frames.data_ptr(), token_len.data_ptr(), steps.data_ptr(), max_tok,
                                                      self._ws.data_ptr(), self._ws.numel(), self._stream()), "rnnt_greedy_resume", lib)
        return tokens, token_frames, token_len, steps


class StreamingTransducer:
    """``Transducer.open_stream``: the encoder session plus the resumed greedy decode on the new frames.  Only streams that received output frames are listed
    in a push's decode."""

    def __init__(self, model, max_streams: int, max_frames: Optional[int] = None):
        self.model = model
        self.session = StreamingEncoder(model.encoder, max_streams, max_frames)       # refuses what cannot stream (stream_refusal) before any device work
        self.decoder = RnntStreamState(model, max_streams)
        self.encoder = model.encoder
        self._tokens = [[] for _ in range(max_streams)]
        self._steps = [0] * max_streams
        self._consumed = [0] * max_streams                       # encoder frames decoded so far
        self.last_token_frames = [[] for _ in range(max_streams)]
        self.last_encoded = None

    align_frames = property(lambda self: self.session.align_frames)

    def frames_pending(self, stream: int) -> int:
        return self.session.frames_pending(stream)

    def reset(self, stream: int):
        """`stream` starts a new utterance."""
        self.session.reset(stream)
        self.decoder.reset(stream)
        self._tokens[stream], self._steps[stream], self._consumed[stream] = [], 0, 0
        self.last_token_frames[stream] = []

    def tokens(self, stream: int) -> List[int]:
        """The stream's hypothesis so far."""
        return list(self._tokens[stream])

    def text(self, stream: int) -> str:
        if self.model.tokenizer is None:
            raise _lib.EffconfError("text() needs a tokenizer attached to the model")
        return self.model.tokenizer.decode([self._tokens[stream]])[0]

    def decoder_steps(self, stream: int) -> int:
        """Prediction-network steps of the stream so far: tokens + 1 once it has had a frame."""
        return self._steps[stream]

    def _decode(self, out: torch.Tensor, out_len: torch.Tensor) -> List[List[int]]:
        self.last_encoded = (out, out_len)
        B = out.shape[0]
        lens = out_len.tolist()
        new = [[] for _ in range(B)]
        self.last_token_frames = [[] for _ in range(B)]
        active = [b for b in range(B) if lens[b] > 0]
        if not active:
            return new
        ix = torch.tensor(active, dtype=torch.int64, device=out.device)
        tokens, frames, token_len, steps = (z.tolist() for z in self.decoder.push(out[ix], out_len[ix], active))
        for i, b in enumerate(active):
            k = token_len[i]
            new[b] = tokens[i][:k]
            self.last_token_frames[b] = [self._consumed[b] + t for t in frames[i][:k]]
            self._tokens[b] += new[b]
            self._steps[b] += steps[i]
            self._consumed[b] += lens[b]
        return new

    def push_mel(self, mel, mel_len, final=None) -> List[List[int]]:
        """``StreamingEncoder.push_mel``, then the decode of the new encoder frames -> the new token ids per stream.  ``last_token_frames[b]``: the encoder frame
        (counted from the stream's start; x ``encoder.frame_seconds`` = seconds) at which each of them was emitted."""
        return self._decode(*self.session.push_mel(mel, mel_len, final))

    def push_audio(self, x, x_len, final=None) -> List[List[int]]:
        return self._decode(*self.session.push_audio(x, x_len, final))
