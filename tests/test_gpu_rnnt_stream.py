"""-m gpu: the streaming RNN-T greedy decode (csrc/rnnt.hip: rnnt_greedy_resume_kernel through effconf_rnnt_greedy_resume).

The kernel alone, through Transducer.open_decode_stream on rnnt_shapes.native_decoder (no encoder runs): the cases of tests/rnnt_stream_ref.py - (20, 36, 44, 37)
where nothing divides 16, (12, 20, 28, 9) with the linear_encoder GEMM at K < 16, the shipped Small decoder (200, 320, 320, 1000), and (20, 36, 44, 37) without a
blank bias (five forced tokens on nearly every frame) - on rnnt_shapes.frames(Denc, 20, 12) with the ragged lengths (0, 1, several that are no multiple of the
kernel's 4 frames per joint pass), pushed 1, 3, 4, 5 and 12 frames at a time and in the irregular pattern [2, 0, 5, 1, rest] rotated by the stream index, where
a stream with no frames in a round is not listed.  All exact: the concatenated tokens of every stream are those of decode_encoded on the whole utterances
(cluster_decode = 0); the global emission frames are the chunked reference's for every utterance the margin rule of tests/rnnt_shapes.py does not excuse;
decoder steps sum to tokens + 1 (0 for the empty stream), and a resumed push runs exactly as many as it emits tokens; the final h, c and gd of every stream are
bit-identical across the push patterns; tokens behind token_len are zero and token frames -1.  The state buffer is filled with 0xFF bytes before init, the
frames behind every stream's new ones are NaN and the output buffers hold a sentinel.  The conditions met (a token and a forced decision on a push's last frame,
a blank-only push, pushes ending inside and on the edge of a group of 4 frames, an idle stream beside busy ones, a stream that never gets a frame) are collected
from what the kernel returned, and one test fails unless all were seen.  Then: ids outside 0 .. max_streams - 1, the refusals that need a device, and the
invariances (a stream alone or among 20, listed ids permuted, the same pushes after reset, two state buffers pushed alternately on one handle, a handle rebuilt
behind an open stream).

The session (Transducer.open_stream): TinyTransducer with causal: true, three streams of 100 / 47 / 73 mel frames in 24-frame, 48-frame, irregular and
all-at-once pushes that end at different pushes, and one push_audio run: per stream the concatenated tokens equal decode_encoded on the concatenation of the
session's own last_encoded rows, exactly, the token frames those of one whole decode of these rows, tokens(stream) is cumulative, and reset + the same pushes
reproduces everything.  The agreement with the whole-utterance greedy_tokens(from_mel = True) is printed, not asserted: the chunked encoder is held to the
whole-utterance forward by a tolerance, not bit for bit.  The whole file also passes with EFFCONF_POISON_WORKSPACE set."""
import functools

import numpy as np
import pytest
import torch

import rnnt_shapes as S
import rnnt_stream_ref as R
from efficientconformer_amd import Transducer, _lib, named_config, synth

pytestmark = pytest.mark.gpu

SENTINEL = -12345
STREAMS = S.GREEDY_BATCH


def _model(case):
    return S.native_decoder(*case)


@functools.lru_cache(maxsize=None)
def _whole(case):
    """decode_encoded of the whole utterances on the per-utterance kernel: computed once per case."""
    m = _model(case)
    f, lens = R.inputs(case[0])
    clean = R.weights(*case)["decoder.rnn.weight_hh_l0"]
    assert np.array_equal(m.decoder.rnn.weight_hh_l0.detach().cpu().numpy(), clean), "rnnt_shapes' cached weights were modified before this decoder was built"
    try:
        m.set_decode_option("cluster_decode", 0)
        assert _lib.load().effconf_rnnt_greedy_route(m._rnnt, f.shape[0]) == 0
        tokens, token_len = m.decode_encoded(torch.from_numpy(f).cuda(), torch.from_numpy(lens).cuda())
    finally:
        m.set_decode_option("cluster_decode", -1)
    tokens, token_len = tokens.cpu(), token_len.cpu()
    return [tokens[i, :int(token_len[i])].tolist() for i in range(tokens.shape[0])]


def _fresh(m, poison=True):
    st = m.open_decode_stream(STREAMS)
    if poison:
        st.state.fill_(0xFF)
        st.init()
    return st


class Run:
    """The utterances of a case pushed through a decode stream round by round.  streams: utterance b is stream streams[b] (default b); only: the utterances that
    take part; order(ids): the order a round lists its streams in."""

    def __init__(self, st, case, pattern, only=None, order=None, direct=True):
        self.st, self.case, self.pattern = st, case, pattern
        self.f, self.lens = R.inputs(case[0])
        self.only = list(range(len(self.lens))) if only is None else list(only)
        self.pf = R.all_pushes(pattern, self.lens)
        self.rounds = max(len(p) for p in self.pf)
        self.order, self.direct = order, direct
        n = len(self.lens)
        self.done, self.primed = [0] * n, [False] * n
        self.tokens, self.frames, self.steps = [[] for _ in range(n)], [[] for _ in range(n)], [0] * n
        self.records, self.rounds_listed = [], []

    def round(self, r):
        rf = [p[r] if r < len(p) else 0 for p in self.pf]
        ids = [b for b in R.listed(self.pattern, rf) if b in self.only]
        self.rounds_listed.append(ids if self.only == list(range(len(self.lens))) else R.listed(self.pattern, rf))
        if self.order is not None:
            ids = self.order(ids)
        if not ids:
            return
        de = self.case[0][0]
        tmax = max(max(rf[b] for b in ids), 1)
        f = torch.full((len(ids), tmax, de), float("nan"))
        for i, b in enumerate(ids):
            f[i, :rf[b]] = torch.from_numpy(self.f[b, self.done[b]: self.done[b] + rf[b]])
        ln = torch.tensor([rf[b] for b in ids], dtype=torch.int64)
        if self.direct:
            max_tok = S.MAX_CONSEC * tmax
            out = (torch.full((len(ids), max_tok), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((len(ids), max_tok), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((len(ids),), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((len(ids),), SENTINEL, dtype=torch.int32, device="cuda"))
            got = self.st._launch(f.cuda(), ln.cuda(), ids, out)
            assert all(a is b for a, b in zip(got, out))
        else:
            got = self.st.push(f.cuda(), ln.cuda(), ids)
        tokens, frames, token_len, steps = (z.cpu() for z in got)
        v = self.case[0][3]
        for i, b in enumerate(ids):
            n, k = rf[b], int(token_len[i])
            what = (self.case, self.pattern, r, b)
            assert 0 <= k <= S.MAX_CONSEC * max(n, 0) and (n > 0 or k == 0), what
            assert int(tokens[i, k:].abs().sum()) == 0, (what, "tokens behind token_len are not zero")
            assert bool((frames[i, k:] == -1).all()), (what, "token frames behind token_len are not -1")
            tk, fr = tokens[i, :k].tolist(), frames[i, :k].tolist()
            assert all(1 <= t < v for t in tk) and fr == sorted(fr) and all(0 <= t < n for t in fr), (what, tk, fr)
            assert all(fr.count(t) <= S.MAX_CONSEC for t in set(fr)), what
            want_steps = 0 if n == 0 else k + (0 if self.primed[b] else 1)
            assert int(steps[i]) == want_steps, (what, int(steps[i]), want_steps)
            on_last = fr.count(n - 1) if n else 0
            self.records.append(dict(stream=b, round=r, frames=n, tokens=k, last_frame_tokens=on_last, last_frame_forced=int(on_last == S.MAX_CONSEC), steps=int(steps[i])))
            self.tokens[b] += tk
            self.frames[b] += [self.done[b] + t for t in fr]
            self.steps[b] += int(steps[i])
            self.done[b] += n
            self.primed[b] = self.primed[b] or n > 0

    def all(self):
        for r in range(self.rounds):
            self.round(r)
        return self

    def state(self):
        """(h, c, gd) rows of the streams that had a frame, and the flags, on the host."""
        h, c, gd, primed = (z.cpu().clone() for z in self.st.state_views())
        live = [b for b in self.only if self.lens[b] > 0]
        return h[live], c[live], gd[live], primed


@functools.lru_cache(maxsize=None)
def _case(case):
    """Every pattern of a case through the kernel, with every assertion of the docstring -> the conditions met."""
    m = _model(case)
    dims, bias = case
    _, lens = R.inputs(dims)
    whole = _whole(case)
    trace = S.greedy_trace(dims, bias)
    excused = S.check_greedy(trace, whole, (case, "whole-utterance decode"))
    seen, first = set(), None
    for pattern in R.PATTERNS:
        ref, _ = R.reference(case, pattern)
        run = Run(_fresh(m), case, pattern).all()
        assert run.tokens == whole, (case, pattern, [b for b in range(len(lens)) if run.tokens[b] != whole[b]])
        for b in range(len(lens)):
            assert run.steps[b] == (len(whole[b]) + 1 if lens[b] else 0), (case, pattern, b, run.steps[b])
            if b not in excused:
                assert ref["tokens"][b] == whole[b] and run.frames[b] == ref["frames"][b], (case, pattern, b, run.frames[b], ref["frames"][b])
        h, c, gd, primed = run.state()
        assert primed.tolist() == [int(n > 0) for n in lens], (case, pattern, primed.tolist())
        assert bool(torch.isfinite(h).all() and torch.isfinite(c).all() and torch.isfinite(gd).all())
        first = first or (pattern, h, c, gd)
        for name, a, z in zip("h c gd".split(), first[1:], (h, c, gd)):
            assert torch.equal(a, z), (case, "final %s differs between the patterns %s and %s" % (name, first[0], pattern))
        got = R.conditions(run.records, lens, run.rounds_listed)
        print("rnnt_stream | %-28s | pushes %-9s | %3d tokens | excused %s | %s" % (R.case_id(case), pattern, sum(len(t) for t in run.tokens), excused, ", ".join(sorted(got))))
        seen |= got
    return frozenset(seen)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_push_pattern_gives_the_whole_utterance_decode(case):
    _case(case)


def test_the_cases_met_every_condition():
    seen = set()
    for case in R.CASES:
        seen |= _case(case)
    assert seen == set(R.CONDITIONS), set(R.CONDITIONS) - seen


def test_ids_out_of_range_and_the_refusals_that_need_a_device():
    case = R.SMALLEST
    m = _model(case)
    st = _fresh(m)
    Run(st, case, "4").round(0)                                   # every stream with frames is primed
    before = st.state.cpu().clone()
    f, _ = R.inputs(case[0])
    ids = [STREAMS, -1, 1000, -(1 << 31)]
    fd = torch.from_numpy(f[:len(ids), 4:8].copy()).cuda()
    ln = torch.full((len(ids),), 4, dtype=torch.int64, device="cuda")
    max_tok = S.MAX_CONSEC * 4
    out = (torch.full((len(ids), max_tok), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((len(ids), max_tok), SENTINEL, dtype=torch.int32, device="cuda"),
           torch.full((len(ids),), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((len(ids),), SENTINEL, dtype=torch.int32, device="cuda"))
    st._launch(fd, ln, ids, out)
    assert out[2].tolist() == [-1] * len(ids)
    assert all(bool((z == SENTINEL).all()) for z in (out[0], out[1], out[3])), "a stream id out of range wrote more than token_len"
    assert torch.equal(st.state.cpu(), before), "a stream id out of range changed the state buffer"
    # the Python entry checks the ids on the host
    for bad in ([0, 0, 1, 2], [0, 1, 2, STREAMS], [0, 1, 2, -1], [0, 1, 2]):
        with pytest.raises(ValueError):
            st.push(fd, ln, bad)
    with pytest.raises(_lib.EffconfError):
        st.reset(STREAMS)
    # refused before any launch: a short token buffer, a short workspace, a short state buffer
    lib = _lib.load()
    idt = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.effconf_rnnt_stream_workspace_bytes(m._rnnt, 4, 4), dtype=torch.uint8, device="cuda")
    call = lambda max_tokens, ws_bytes: lib.effconf_rnnt_greedy_resume(m._rnnt, st.state.data_ptr(), STREAMS, idt.data_ptr(), fd.data_ptr(), ln.data_ptr(), 4, 4, out[0].data_ptr(),
                                                                     out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), max_tokens, ws.data_ptr(), ws_bytes, None)
    assert call(max_tok - 1, ws.numel()) != 0 and b"token buffer" in lib.effconf_last_error()
    assert call(max_tok, ws.numel() - 1) != 0 and b"workspace too small" in lib.effconf_last_error()
    assert lib.effconf_rnnt_stream_init(m._rnnt, st.state.data_ptr(), st.state.numel() - 1, STREAMS, None) != 0 and b"state buffer too small" in lib.effconf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(st.state.cpu(), before) and out[2].tolist() == [-1] * len(ids), "a refused call wrote something"


def test_invariances_bit_for_bit():
    case = R.SMALLEST
    m = _model(case)
    _, lens = R.inputs(case[0])
    same = lambda a, b, only=None: all(a.tokens[i] == b.tokens[i] and a.frames[i] == b.frames[i] and a.steps[i] == b.steps[i] for i in (only or range(len(lens))))
    for pattern in ("3", "irregular"):
        st = _fresh(m)
        base = Run(st, case, pattern, direct=False).all()
        assert base.tokens == _whole(case)
        bh, bc, bgd, _ = base.state()
        # the same pushes after reset, the buffer as the first run left it
        for b in range(STREAMS):
            st.reset(b)
        assert st.state_views()[3].tolist() == [0] * STREAMS
        again = Run(st, case, pattern, direct=False).all()
        assert same(base, again) and all(torch.equal(a, z) for a, z in zip(base.state(), again.state())), (pattern, "the same pushes after reset differ")
        # listed ids in another order
        perm = Run(_fresh(m), case, pattern, order=lambda ids: ids[::-1][1:] + ids[::-1][:1], direct=False).all()
        assert same(base, perm) and all(torch.equal(a, z) for a, z in zip(base.state(), perm.state())), (pattern, "permuted ids differ")
        # a stream alone
        live = [b for b in range(len(lens)) if lens[b] > 0]
        for b in (0, 2, 5, 13):
            alone = Run(_fresh(m), case, pattern, only=[b], direct=False).all()
            ah, ac, agd, primed = alone.state()
            i = live.index(b)
            assert same(base, alone, [b]) and torch.equal(ah[0], bh[i]) and torch.equal(ac[0], bc[i]) and torch.equal(agd[0], bgd[i]), (pattern, b, "a stream alone differs")
            assert primed.tolist() == [int(s == b) for s in range(STREAMS)]
    # two state buffers on one handle, pushed alternately
    a, z = Run(_fresh(m), case, "3", direct=False), Run(_fresh(m), case, "irregular", direct=False)
    for r in range(max(a.rounds, z.rounds)):
        if r < a.rounds:
            a.round(r)
        if r < z.rounds:
            z.round(r)
    assert a.tokens == z.tokens == _whole(case) and a.frames == z.frames
    assert all(torch.equal(x, y) for x, y in zip(a.state()[:3], z.state()[:3]))
    # a handle rebuilt behind an open stream
    st = _fresh(m)
    m._invalidate()
    f, _ = R.inputs(case[0])
    with pytest.raises(_lib.EffconfError, match="open a new decode stream"):
        st.push(torch.from_numpy(f[:2, :3].copy()).cuda(), None)
    assert Run(_fresh(m), case, "5", direct=False).all().tokens == _whole(case)


# ------------------------------------------------------------------ the session
MEL_LENS = (100, 47, 73)


@functools.lru_cache(maxsize=None)
def _session_model():
    cfg = named_config("TinyTransducer")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = Transducer.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, None, prefix="encoder.")
    sd.update(synth.make_transducer_state_dict(m.encoder.plan.dim_out, cfg["decoder_params"], cfg["joint_params"], 7, blank_bias=1.2))
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


def _session_run(sess, mel, pattern):
    B = len(MEL_LENS)
    cums = [_cumulative(pattern, n) for n in MEL_LENS]
    new_tokens, frames, rows = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    for r in range(max(len(c) for c in cums)):
        new, fin = [0] * B, [False] * B
        chunk = torch.zeros(B, mel.shape[1], mel.shape[2], device=mel.device)
        for b, c in enumerate(cums):
            if r < len(c):
                lo = c[r - 1] if r else 0
                new[b], fin[b] = c[r] - lo, r == len(c) - 1
                chunk[b, :, :new[b]] = mel[b, :, lo: c[r]]
        got = sess.push_mel(chunk, new, fin)
        out, out_len = sess.last_encoded
        for b in range(B):
            new_tokens[b] += got[b]
            frames[b] += sess.last_token_frames[b]
            rows[b].append(out[b, :int(out_len[b])])
            assert len(got[b]) == len(sess.last_token_frames[b])
            assert sess.tokens(b) == new_tokens[b], "tokens(stream) is not the concatenation of the pushes' tokens"
    return new_tokens, frames, [torch.cat(r) for r in rows]


def _check_against_own_rows(m, tokens, frames, rows, steps, what):
    for b, enc in enumerate(rows):
        tk, tl = m.decode_encoded(enc[None].contiguous(), None)
        want = tk[0, :int(tl[0])].tolist()
        assert tokens[b] == want, (what, b, tokens[b], want)
        one = m.open_decode_stream(1)
        wt, wf, wl, ws = one.push(enc[None].contiguous(), None)
        assert wt[0, :int(wl[0])].tolist() == want and frames[b] == wf[0, :int(wl[0])].tolist(), (what, b, frames[b])
        assert frames[b] == sorted(frames[b]) and all(0 <= t < enc.shape[0] for t in frames[b])
        assert steps[b] == len(want) + 1 == int(ws[0]), (what, b, steps[b])


@pytest.mark.parametrize("pattern", ("24", "48", "irregular", "all"))
def test_session_tokens_equal_the_decode_of_its_own_encoder_rows(pattern):
    m, mel = _session_model()
    sess = m.open_stream(len(MEL_LENS), max_frames=max(MEL_LENS))
    assert sess.align_frames == 24
    tokens, frames, rows = _session_run(sess, mel, pattern)
    assert sum(len(t) for t in tokens) >= 20, "the fixture emits too few tokens to mean anything"
    _check_against_own_rows(m, tokens, frames, rows, [sess.decoder_steps(b) for b in range(len(MEL_LENS))], pattern)
    assert all(sess.frames_pending(b) == 0 for b in range(len(MEL_LENS)))
    whole = m.greedy_tokens(mel, torch.tensor(MEL_LENS).cuda(), from_mel=True)
    print("rnnt_stream | session pushes %-9s | tokens %s | equal to the whole-utterance greedy_tokens: %s | seconds of the first tokens of stream 0: %s" % (
        pattern, [len(t) for t in tokens], [tokens[b] == whole[b] for b in range(len(MEL_LENS))], ["%.2f" % (t * m.encoder.frame_seconds) for t in frames[0][:4]]))
    # reset, then the same pushes
    for b in range(len(MEL_LENS)):
        sess.reset(b)
        assert sess.tokens(b) == [] and sess.decoder_steps(b) == 0
    again = _session_run(sess, mel, pattern)
    assert again[0] == tokens and again[1] == frames and all(torch.equal(a, z) for a, z in zip(again[2], rows)), (pattern, "the same pushes after reset differ")


def test_session_push_audio():
    m, _ = _session_model()
    lens = np.array([48000], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=4)).cuda()
    sess = m.open_stream(1)
    tokens, frames, rows = [], [], []
    for lo in range(0, 48000, 4000):
        got = sess.push_audio(audio[:, lo: lo + 4000], [4000], [lo + 4000 >= 48000])
        out, out_len = sess.last_encoded
        tokens += got[0]
        frames += sess.last_token_frames[0]
        rows.append(out[0, :int(out_len[0])])
    assert tokens and sess.tokens(0) == tokens
    _check_against_own_rows(m, [tokens], [frames], [torch.cat(rows)], [sess.decoder_steps(0)], "push_audio")
    with pytest.raises(_lib.EffconfError, match="tokenizer"):
        sess.text(0)
