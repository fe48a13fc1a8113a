"""-m gpu: the streaming CTC prefix beam search (csrc/ctc_beam.hip: ctc_beam_resume_kernel through effconf_ctc_beam_resume).

The kernel alone, through ModelCTC.open_beam_decode_stream on logits the test makes (no encoder runs): V in {32, 256, 1000} x beam in {1, 4, 16, 32} - V = 32 with
beam 16 makes K = V, beam 32 with V = 1000 uses all three exclusion words and K = 65 - four streams of 48, 1, 17 and 30 frames, through every push pattern of
tests/ctc_beam_stream_ref.py (whole, ones, first1, uneven, gaps, subsets).  All exact, no tolerance: the final tokens, token_len and score of every stream are
bit-identical to decode_logits_beam on the same logits; the pushes' traces concatenated equal the whole call's trace bit for bit (node, pb, pnb, score), and the
candidate and trie node counts are equal; stable_len equals the common prefix of the returned n-best (nbest = beam) and never decreases; a zero-frame push returns
the beam unchanged and leaves the record's bytes (in an all-zero round: the whole state buffer) unchanged; a second state sized for another max_frames gives the
same bits.  Every state buffer is filled with 0xFF before init, the outputs hold a sentinel, the workspace 0xFF, and NaN lies behind every stream's new frames.
Then: two state buffers used alternately, reset in mid-utterance, a stream alone, nbest < beam and a short max_tokens, ids out of range (-1, the rest
bit-identical to a run without them), a push past max_frames (ValueError on the host, nothing launched; the kernel's own guard: -2, state unchanged).

Sessions (ModelCTC.open_stream(beam_size=..)): Tiny with causal: true from synth, three streams of 100 / 47 / 73 mel frames with push_mel in 24-frame, 48-frame,
irregular and all-at-once pushes, and one push_audio run: per stream the committed tokens concatenated over the pushes equal hypothesis() after final, and rank 0
of decode_logits_beam on the session's own last_push_logits concatenated - exact.  No claim is made against the non-streaming forward."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_stream_ref as R
from efficientconformer_amd import ModelCTC, _lib, named_config, streaming, synth

pytestmark = pytest.mark.gpu

SENTINEL = -12345
LENS = (48, 1, 17, 30)
MAX_FRAMES = 48


@functools.lru_cache(maxsize=None)
def _decoder():
    """A ModelCTC used for its decoders only (the logits come from the test, not from the encoder)."""
    cfg = named_config("Tiny")
    return ModelCTC(cfg["encoder_params"], cfg["tokenizer_params"], decoding_params={"beam_size": 4, "tmp": 1.0})


@functools.lru_cache(maxsize=None)
def _logits(v):
    rng = np.random.default_rng(7000 + v)
    return tuple((rng.standard_normal((t, v)) * 1.5).astype(np.float32) for t in LENS)


@functools.lru_cache(maxsize=None)
def _whole(v, beam):
    """decode_logits_beam of the whole utterances with its trace: computed once per case, never modified."""
    rows = _logits(v)
    pad = np.full((len(rows), max(LENS), v), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        pad[i, :r.shape[0]] = r
    m = _decoder()
    tokens, token_len, score = m.decode_logits_beam(torch.from_numpy(pad).cuda(), torch.tensor(LENS).cuda(), beam)
    return tokens.cpu().numpy(), token_len.cpu().numpy(), score.cpu().numpy(), m.last_beam_trace()


def _fresh(beam, max_streams=len(LENS), max_frames=MAX_FRAMES):
    st = _decoder().open_beam_decode_stream(max_streams, max_frames, beam, device="cuda")
    st.state.fill_(0xFF)
    st.init()
    return st


class Run:
    """The utterances of a case pushed through a decode stream round by round; stream_of[b]: the stream utterance b goes to (default b)."""

    def __init__(self, st, v, nbest=None, max_tokens=MAX_FRAMES, stream_of=None, only=None):
        self.st, self.rows, self.v = st, _logits(v), v
        self.nbest = st.beam if nbest is None else nbest
        self.max_tokens = max_tokens
        self.stream_of = list(range(len(LENS))) if stream_of is None else stream_of
        self.only = list(range(len(LENS))) if only is None else only
        n = len(LENS)
        self.done = [0] * n
        self.last = [None] * n                       # (tokens, token_len, score, stable_len) of the stream's last push
        self.stable, self.trace = [[] for _ in range(n)], [[] for _ in range(n)]
        self.counts = [None] * n

    def round(self, rnd, extra_ids=()):
        """One push: rnd [(utterance, frames)]; extra_ids: further ids listed behind them with 3 frames each (out of range: the kernel turns them away)."""
        rnd = [(b, k) for b, k in rnd if b in self.only]
        if not rnd and not extra_ids:
            return None
        ids = [self.stream_of[b] for b, _ in rnd] + list(extra_ids)
        ks = [k for _, k in rnd] + [3] * len(extra_ids)
        n, tmax = len(ids), max(ks)
        lg = torch.full((n, tmax, self.v), float("nan"))
        for i, (b, k) in enumerate(rnd):
            lg[i, :k] = torch.from_numpy(self.rows[b][self.done[b]: self.done[b] + k])
        for i in range(len(rnd), n):
            lg[i, :3] = 0.0
        st = self.st
        out = (torch.full((n, self.nbest, self.max_tokens), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((n, self.nbest), SENTINEL, dtype=torch.int32, device="cuda"),
               torch.full((n, self.nbest), float("nan"), dtype=torch.float32, device="cuda"), torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"))
        if st._ws is not None:
            st._ws.fill_(0xFF)
        before = [st.frames(self.stream_of[b]) for b, _ in rnd]
        got = st._launch(lg.cuda(), ks, ids, self.nbest, out, self.max_tokens)
        assert all(a is z for a, z in zip(got, out))
        tokens, token_len, score, stable = (z.cpu().numpy() for z in got)
        tr = st.last_push_trace()
        for i, (b, k) in enumerate(rnd):
            what = (self.v, st.beam, b, k, self.done[b])
            assert st.frames(self.stream_of[b]) == before[i] + k == self.done[b] + k
            assert (token_len[i] >= 0).all() and (token_len[i] <= self.done[b] + k).all(), what
            hyps = []
            for r in range(self.nbest):
                d = min(int(token_len[i, r]), self.max_tokens)
                assert not tokens[i, r, d:].any(), (what, "tokens behind token_len are not zero")
                assert (tokens[i, r, :d] > 0).all() and (tokens[i, r, :d] < self.v).all(), what
                if r == 0 or token_len[i, r] > 0 or score[i, r] != -np.inf:
                    hyps.append(tuple(tokens[i, r, :d].tolist()))
            assert not np.isnan(score[i]).any(), what
            if self.nbest == st.beam and self.max_tokens >= self.done[b] + k:
                assert int(stable[i]) == streaming.common_prefix_len(hyps), (what, int(stable[i]), hyps)
            assert not self.stable[b] or int(stable[i]) >= self.stable[b][-1], (what, "stable_len decreased")
            if self.stable[b]:                   # the committed tokens stay
                keep = min(self.stable[b][-1], self.max_tokens)
                assert (tokens[i, 0, :keep] == self.last[b][0][0, :keep]).all(), what
            if k == 0 and self.last[b] is not None:
                assert all(np.array_equal(a, z, equal_nan=True) for a, z in zip((tokens[i], token_len[i], score[i], stable[i]), self.last[b])), (what, "a zero-frame push changed the beam")
            if k == 0 and self.last[b] is None:
                assert token_len[i, 0] == 0 and score[i, 0] == 0 and (score[i, 1:] == -np.inf).all() and stable[i] == 0, (what, "a stream without frames is the empty prefix")
            assert tr[i]["len"] == k and tr[i]["frames"] == self.done[b] + k, what
            self.trace[b].append(tr[i])
            self.counts[b] = (tr[i]["candidates"], tr[i]["nodes"])
            self.stable[b].append(int(stable[i]))
            self.last[b] = (tokens[i].copy(), token_len[i].copy(), score[i].copy(), stable[i].copy())
            self.done[b] += k
        return tokens, token_len, score, stable

    def all(self, pattern, seed=0):
        for rnd in R.schedule(pattern, list(LENS), seed):
            zero = all(k == 0 for _, k in rnd)
            recs = self.st.state_views()[1].cpu().clone()
            whole = self.st.state.cpu().clone() if zero else None
            self.round(rnd)
            after = self.st.state_views()[1].cpu()
            for b, k in rnd:
                if k == 0 and b in self.only and self.done[b] > 0:
                    assert torch.equal(after[self.stream_of[b]], recs[self.stream_of[b]]), (pattern, b, "a zero-frame push changed the record")
            if zero:
                assert torch.equal(self.st.state.cpu(), whole), (pattern, "a round of zero-frame pushes changed the state buffer")
        assert [self.done[b] for b in self.only] == [LENS[b] for b in self.only]
        return self

    def check_final(self, beam, what):
        """Bit-identical to the whole-utterance call: results, the concatenated trace, the counts."""
        tokens, token_len, score, trace = _whole(self.v, beam)
        for b in self.only:
            tk, tl, sc, _ = self.last[b]
            assert np.array_equal(tl, token_len[b][:self.nbest]), (what, b, tl, token_len[b])
            assert sc.tobytes() == score[b][:self.nbest].tobytes(), (what, b, sc, score[b])
            w = min(self.max_tokens, tokens.shape[2])
            assert np.array_equal(tk[:, :w], tokens[b][:self.nbest, :w]), (what, b)
            for key in ("node", "pb", "pnb", "score"):
                cat = np.concatenate([t[key] for t in self.trace[b]])
                assert cat.shape == trace[b][key].shape and cat.tobytes() == trace[b][key].tobytes(), (what, b, key)
            assert self.counts[b] == (trace[b]["candidates"], len(trace[b]["parent"])), (what, b, self.counts[b])


@pytest.mark.parametrize("v", [32, 256, 1000])
@pytest.mark.parametrize("beam", [1, 4, 16, 32])
def test_every_push_pattern_is_the_whole_utterance_search_bit_for_bit(v, beam):
    for pattern in R.PATTERNS:
        Run(_fresh(beam), v).all(pattern).check_final(beam, (v, beam, pattern))
    # another capacity: another hash size, the same bits (node numbering is creation order)
    Run(_fresh(beam, max_frames=61), v).all("uneven").check_final(beam, (v, beam, "max_frames 61"))


def test_independence_two_buffers_reset_alone_nbest_and_short_tokens():
    v, beam = 256, 4
    # two state buffers, pushed alternately with different patterns
    a, z = Run(_fresh(beam), v), Run(_fresh(beam), v)
    ra, rz = R.schedule("uneven", list(LENS)), R.schedule("subsets", list(LENS), 5)
    for r in range(max(len(ra), len(rz))):
        if r < len(ra):
            a.round(ra[r])
        if r < len(rz):
            z.round(rz[r])
    a.check_final(beam, "buffer a")
    z.check_final(beam, "buffer z")
    # reset in mid-utterance equals a fresh stream; the streams permuted
    st = _fresh(beam)
    first = Run(st, v)
    for rnd in R.schedule("uneven", list(LENS))[:2]:
        first.round(rnd)
    for s in range(len(LENS)):
        st.reset(s)
        assert st.frames(s) == 0
    assert st.state_views()[0].tolist() == [0] * len(LENS)
    Run(st, v, stream_of=[2, 0, 3, 1]).all("gaps").check_final(beam, "after reset")
    # a stream alone in a state of one
    for b in (0, 2):
        Run(_fresh(beam, max_streams=1), v, stream_of=[0] * len(LENS), only=[b]).all("uneven").check_final(beam, ("alone", b))
    # nbest < beam, and a token buffer shorter than the hypotheses: token_len stays the true depth
    Run(_fresh(beam), v, nbest=2).all("uneven").check_final(beam, "nbest 2")
    short = Run(_fresh(beam), v, nbest=1, max_tokens=3).all("uneven")
    short.check_final(beam, "max_tokens 3")
    assert max(int(short.last[b][1][0]) for b in range(len(LENS))) > 3, "no hypothesis is longer than the short token buffer"


def test_ids_out_of_range_and_pushes_past_the_capacity():
    v, beam = 32, 4
    rounds = R.schedule("uneven", list(LENS))
    clean = Run(_fresh(beam), v)
    dirty = Run(_fresh(beam), v)
    clean.round(rounds[0])
    dirty.round(rounds[0])
    before = dirty.st.state.cpu().clone()
    bad = [len(LENS), -1, 1000, -(1 << 31)]
    got = dirty.st._launch(torch.zeros(len(bad), 3, v, device="cuda"), [3] * len(bad), bad, beam,
                           (torch.full((len(bad), beam, 8), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((len(bad), beam), SENTINEL, dtype=torch.int32, device="cuda"),
                            torch.full((len(bad), beam), 7.0, device="cuda"), torch.full((len(bad),), SENTINEL, dtype=torch.int32, device="cuda")), 8)
    assert got[1].tolist() == [[-1] * beam] * len(bad)
    assert bool((got[0] == SENTINEL).all() and (got[2] == 7.0).all() and (got[3] == SENTINEL).all()), "a stream id out of range wrote more than token_len"
    assert torch.equal(dirty.st.state.cpu(), before), "a stream id out of range changed the state buffer"
    assert dirty.st.last_push_trace() == [None] * len(bad)
    # listed beside good streams: those are bit-identical to a run without the bad ids
    for rnd in rounds[1:]:
        c = clean.round(rnd)
        d = dirty.round(rnd, extra_ids=bad[:2])
        k = len(rnd)
        assert all(np.array_equal(x, y[:k], equal_nan=True) for x, y in zip(c, d))
        assert (d[1][k:] == -1).all() and (d[0][k:] == SENTINEL).all() and (d[3][k:] == SENTINEL).all()
    clean.check_final(beam, "clean")
    dirty.check_final(beam, "beside bad ids")
    # past the capacity: the Python entry refuses on the host, nothing is launched
    st = dirty.st
    state = st.state.cpu().clone()
    lg = torch.zeros(2, 2, v, device="cuda")
    for ids, lens in (([0, 1], [1, 1]), ([2], [MAX_FRAMES - LENS[2] + 1]), ([1, 1], [0, 0]), ([4], [1]), ([-1], [1])):
        with pytest.raises(ValueError):
            st.push(torch.zeros(len(ids), max(lens + [1]), v, device="cuda"), lens, ids)
    assert torch.equal(st.state.cpu(), state) and [st.frames(s) for s in range(4)] == list(LENS)
    # the kernel's own guard: -2 for the stream that would overflow, nothing else, and its neighbour goes on
    out = (torch.full((2, beam, 60), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((2, beam), SENTINEL, dtype=torch.int32, device="cuda"),
           torch.full((2, beam), 7.0, device="cuda"), torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda"))
    st._launch(lg, [1, 2], [0, 2], beam, out, 60)                 # stream 0 is full (48 of 48); stream 2 has 17
    assert out[1][0].tolist() == [-2] * beam and bool((out[0][0] == SENTINEL).all() and (out[2][0] == 7.0).all()) and int(out[3][0]) == SENTINEL
    assert st.frames(0) == LENS[0] and st.frames(2) == LENS[2] + 2 and int(out[1][1, 0]) >= 0 and int(out[3][1]) >= 0
    views = st.state_views()[1].cpu()
    assert int(views[0, 0]) == LENS[0] and int(views[2, 0]) == LENS[2] + 2
    # refused by the library before any launch
    lib = _lib.load()
    idt = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    ln = torch.tensor([0, 0], dtype=torch.int64, device="cuda")
    call = lambda **kw: lib.effconf_ctc_beam_resume(st.state.data_ptr(), 4, MAX_FRAMES, beam, idt.data_ptr(), lg.data_ptr(), ln.data_ptr(), 2, 2, v, 1.0, kw.get("nbest", beam),
                                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), kw.get("max_tokens", 60),
                                                    st._ws.data_ptr(), kw.get("ws", st._ws.numel()), None)
    assert call(nbest=beam + 1) != 0 and b"nbest" in lib.effconf_last_error()
    assert call(max_tokens=0) != 0 and b"max_tokens" in lib.effconf_last_error()
    assert call(ws=255) != 0 and b"workspace too small" in lib.effconf_last_error()
    assert lib.effconf_ctc_beam_stream_init(st.state.data_ptr(), st.state.numel() - 1, 4, MAX_FRAMES, beam, None) != 0 and b"state buffer too small" in lib.effconf_last_error()
    with pytest.raises(_lib.EffconfError):
        st.reset(4)
    # a read-only push of every stream without logits (t_new = 0)
    tokens, token_len, score, stable = st.push(torch.zeros(4, 0, v, device="cuda"), None)
    assert tokens.shape == (4, beam, MAX_FRAMES) and bool((token_len[:, 0] >= 0).all()) and stable.shape == (4,) and bool(torch.isfinite(score[:, 0]).all())


# ------------------------------------------------------------------ the session
MEL_LENS = (100, 47, 73)


@functools.lru_cache(maxsize=None)
def _session_model():
    cfg = named_config("Tiny")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    mel, lens = synth.make_mel(3, m.encoder.plan.n_mels, max(MEL_LENS), list(MEL_LENS), seed=31)
    rows = [lens.tolist().index(n) for n in MEL_LENS]               # make_mel sorts its lengths: back to 100 / 47 / 73
    return m.cuda(), torch.from_numpy(mel[rows]).cuda()


def _cumulative(name, total):
    """Frames received after every push of a pattern; the last push brings the rest."""
    if name == "all":
        return [total]
    steps = {"24": [24] * (total // 24 + 1), "48": [48] * (total // 48 + 1), "irregular": [7, 50, 1, 0, 23]}[name]
    cum, s = [], 0
    for x in steps:
        if s + x >= total:
            break
        s += x
        cum.append(s)
    return cum + [total]


def _check_session(m, sess, committed, logits, beam, what):
    for b in range(len(committed)):
        assert committed[b] == sess.hypothesis(b) == sess.committed(b), (what, b, committed[b], sess.hypothesis(b))
        assert sess.nbest(b)[0][0] == committed[b] and sess.frames_pending(b) == 0
        lg = torch.cat(logits[b])[None].contiguous()
        tokens, token_len, score = m.decode_logits_beam(lg, None, beam)
        assert committed[b] == tokens[0, 0, :int(token_len[0, 0])].tolist(), (what, b)
        nb = sess.nbest(b)
        assert [ids for ids, _ in nb] == [tokens[0, r, :int(token_len[0, r])].tolist() for r in range(len(nb))]
        assert np.array([s for _, s in nb], dtype=np.float32).tobytes() == score[0, :len(nb)].cpu().numpy().tobytes()


@pytest.mark.parametrize("pattern", ("24", "48", "irregular", "all"))
def test_session_commits_the_best_hypothesis_of_its_own_logits(pattern):
    m, mel = _session_model()
    beam, B = 4, len(MEL_LENS)
    sess = m.open_stream(B, max_frames=max(MEL_LENS), beam_size=beam)
    assert sess.align_frames == 24 and isinstance(sess, streaming.StreamingCTCBeam) and isinstance(m.open_stream(B), streaming.StreamingCTC)
    for attempt in range(2):                                          # the second time after reset: the same pushes give the same tokens
        cums = [_cumulative(pattern, n) for n in MEL_LENS]
        committed, logits = [[] for _ in range(B)], [[] for _ in range(B)]
        for r in range(max(len(c) for c in cums)):
            new, fin = [0] * B, [False] * B
            chunk = torch.zeros(B, mel.shape[1], mel.shape[2], device=mel.device)
            for b, c in enumerate(cums):
                if r < len(c):
                    lo = c[r - 1] if r else 0
                    new[b], fin[b] = c[r] - lo, r == len(c) - 1
                    chunk[b, :, :new[b]] = mel[b, :, lo: c[r]]
            got = sess.push_mel(chunk, new, fin)
            if sess.last_push_logits is not None:
                lg, ln, active = sess.last_push_logits
                for i, b in enumerate(active):
                    logits[b].append(lg[i, :int(ln[i])])
            for b in range(B):
                committed[b] += got[b]
                assert sess.committed(b) == committed[b] and sess.hypothesis(b)[:len(committed[b])] == committed[b], "the return value is not append-only"
        print("ctc_beam_stream | session pushes %-9s | committed tokens %s" % (pattern, [len(t) for t in committed]))
        assert sum(len(t) for t in committed) > 0, "the fixture commits no token at all"
        _check_session(m, sess, committed, logits, beam, (pattern, attempt))
        if attempt == 0:
            first = committed
            for b in range(B):
                sess.reset(b)
                assert sess.committed(b) == [] and sess.hypothesis(b) == []
        else:
            assert committed == first, (pattern, "the same pushes after reset differ")


def test_session_push_audio():
    m, _ = _session_model()
    lens = np.array([48000], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=4)).cuda()
    sess = m.open_stream(1, max_frames=48000 // m.encoder.plan.hop_length + 1, beam_size=8)
    committed, logits = [], []
    for lo in range(0, 48000, 4000):
        committed += sess.push_audio(audio[:, lo: lo + 4000], [4000], [lo + 4000 >= 48000])[0]
        if sess.last_push_logits is not None:
            lg, ln, _ = sess.last_push_logits
            logits.append(lg[0, :int(ln[0])])
    assert committed
    _check_session(m, sess, [committed], [logits], 8, "push_audio")
    with pytest.raises(_lib.EffconfError, match="tokenizer"):
        sess.text(0)
