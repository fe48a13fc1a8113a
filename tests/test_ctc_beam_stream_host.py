"""Streaming CTC prefix beam search, host side (no GPU): the chunked specification (tests/ctc_beam_stream_ref.py) against the whole-utterance oracle
(tests/ctc_beam_ref.py) for every case and push pattern, exactly, on float64 and on fp32 log-probabilities; the stable prefix push after push; the injected
carry faults; the conditions the cases meet (a best hypothesis that changes in a token not yet committed, a prefix that leaves the beam and re-enters across a
push boundary); the state / workspace sizes against a Python mirror of csrc/decode_layout.h; every refusal that needs no device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ctc_beam_stream_ref as R
from ctc_beam_ref import beam_search, logp32, logp64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _flat(seed, lens, v, scale):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((t, v)) * scale).astype(np.float32) for t in lens]


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (logits per stream, beam)"""
    out = {"v6_beam3": (_flat(1, (14, 1, 9, 5), 6, 1.0), 3), "v5_beam1": (_flat(2, (11, 4, 7), 5, 2.0), 1), "v8_beam4": (_flat(3, (13, 2, 8, 10), 8, 0.5), 4),
           "v3_beam16": (_flat(4, (6, 3, 5), 3, 2.0), 16)}
    g = np.load(os.path.join(GOLDEN, "ctc_beam_reentry.npz"))
    for j in range(int(g["count"])):
        out["reentry_%d" % j] = ([g["logits_%d" % j].astype(np.float32)], int(g["beam_%d" % j]))
    return out


SMALLEST = "v6_beam3"


def _same(members, ref):
    return ([m[0] for m in members] == ref["prefixes"] and np.array_equal(np.array([m[1] for m in members]), ref["pb"])
            and np.array_equal(np.array([m[2] for m in members]), ref["pnb"]) and np.array_equal(R.scores(members), ref["score"]))


@pytest.mark.parametrize("logp", [logp64, logp32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", sorted(_cases()))
def test_chunked_reference_equals_the_whole_search_exactly(name, logp):
    logits, beam = _cases()[name]
    lp = [logp(x) for x in logits]
    whole = [beam_search(x, None, beam, trace=True) for x in lp]
    for pattern in R.PATTERNS:
        srch, hist = R.run(lp, pattern, beam)
        for b, s in enumerate(srch):
            assert s.frames == lp[b].shape[0]
            assert _same(s.members, whole[b]), (name, pattern, b)
            assert [[m[0] for m in fr] for fr in s.beams] == [[p for p, _, _ in fr] for fr in whole[b]["beams"]], (name, pattern, b)
            # the stable prefix: non-decreasing, a prefix of every later hypothesis of every rank and of the final best
            stable = [R.stable_prefix(m) for m in hist[b]]
            for i, sp in enumerate(stable):
                assert i == 0 or (len(sp) >= len(stable[i - 1]) and sp[:len(stable[i - 1])] == stable[i - 1]), (name, pattern, b, i)
                for later in hist[b][i:]:
                    assert all(m[0][:len(sp)] == sp for m in later), (name, pattern, b, i)
                assert whole[b]["prefixes"][0][:len(sp)] == sp
        if pattern == "gaps":
            for b in range(len(lp)):
                assert hist[b][-1] == hist[b][-2], "the trailing zero-frame push changed the beam"


def test_push_patterns_cover_what_they_claim():
    lens = [14, 1, 9, 5]
    for pattern in R.PATTERNS:
        rounds = R.schedule(pattern, lens)
        total = [0] * len(lens)
        for rnd in rounds:
            assert len({b for b, _ in rnd}) == len(rnd), "a stream is listed twice in a round"
            for b, k in rnd:
                total[b] += k
        assert total == lens, pattern
    assert len(R.schedule("whole", lens)) == 1
    assert all(k == 1 for rnd in R.schedule("ones", lens) for _, k in rnd)
    assert [k for b, k in R.schedule("first1", lens)[0]] == [1, 1, 1, 1]
    assert any(k == 0 for rnd in R.schedule("gaps", lens) for _, k in rnd)
    sub = R.schedule("subsets", lens)
    assert any(len(rnd) < sum(1 for b in range(4)) for rnd in sub) and any([b for b, _ in rnd] != sorted(b for b, _ in rnd) for rnd in sub)
    assert len({k for rnd in R.schedule("uneven", lens) for _, k in rnd}) >= 4


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_faults_change_the_result_on_the_smallest_case(fault):
    logits, beam = _cases()[SMALLEST]
    lp = [logp64(x) for x in logits]
    whole = [beam_search(x, None, beam) for x in lp]
    srch, _ = R.run(lp, "gaps", beam, fault=fault)
    assert any(not _same(s.members, whole[b]) for b, s in enumerate(srch)), fault


def test_the_cases_meet_the_conditions():
    changed, reentry = [], []
    for name, (logits, beam) in _cases().items():
        lp = [logp64(x) for x in logits]
        srch, hist = R.run(lp, "ones", beam)                      # a boundary at every frame
        for b, s in enumerate(srch):
            best = [m[0][0] for m in hist[b]]
            stable = [R.stable_prefix(m) for m in hist[b]]
            # the best hypothesis changes in a token that was not yet committed: a later best does not begin with an earlier best, beyond its stable prefix
            if any(best[j][:len(best[i])] != best[i] and len(best[i]) > len(stable[i]) for i in range(len(best)) for j in range(i + 1, len(best))):
                changed.append((name, b))
            sets = [{m[0] for m in fr} for fr in s.beams]
            for t1 in range(len(sets)):
                for p in sets[t1]:
                    out = [t for t in range(t1 + 1, len(sets)) if p not in sets[t]]
                    if out and any(p in sets[t] for t in range(out[0] + 1, len(sets))):
                        reentry.append((name, b))
    assert changed, "no case changes its best hypothesis in an uncommitted token"
    assert any(n.startswith("reentry_") for n, _ in reentry), "no re-entry fixture has a prefix that leaves the beam and comes back across a push boundary"


# ------------------------------------------------------------------ sizes and refusals
def _al(x):
    return (x + 255) // 256 * 256


def _state_bytes(max_streams, max_frames, beam):
    ncap = 1 + beam * max_frames
    h = 1
    while h < 2 * ncap:
        h <<= 1
    per = _al(4 * (16 + 7 * 32)) + _al(16 * ncap) + _al(8 * h) + _al(4 * h)
    return _al(4 * max_streams) + max_streams * per + 256


def _ws_bytes(n, t_new, beam):
    return _al(16 * n) + n * _al(16 * t_new * beam) + 256


def test_size_queries_against_the_python_mirror_of_the_layout():
    from efficientconformer_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        hdr = fh.read()
    for fn in ("effconf_ctc_beam_stream_state_bytes", "effconf_ctc_beam_stream_init", "effconf_ctc_beam_stream_reset", "effconf_ctc_beam_stream_workspace_bytes",
               "effconf_ctc_beam_resume"):
        assert fn in hdr and fn in _lib.SIGNATURES and hasattr(lib, fn)
    for s in (1, 3, 64, 65):
        for f in (1, 13, 125, 250):
            for beam in (1, 4, 16, 32):
                assert lib.effconf_ctc_beam_stream_state_bytes(s, f, beam) == _state_bytes(s, f, beam), (s, f, beam)
    for n in (0, 1, 5, 64):
        for t in (0, 1, 12, 48):
            for beam in (1, 4, 16, 32):
                assert lib.effconf_ctc_beam_stream_workspace_bytes(n, t, beam) == _ws_bytes(n, t, beam), (n, t, beam)
    for args in ((0, 10, 4), (-1, 10, 4), (2, 0, 4), (2, -1, 4), (2, 10, 0), (2, 10, 33), (2, 1 << 20, 16)):
        assert lib.effconf_ctc_beam_stream_state_bytes(*args) == 0, args
    for args in ((-1, 4, 4), (2, -1, 4), (2, 4, 0), (2, 4, 33), (2, 1 << 20, 16)):
        assert lib.effconf_ctc_beam_stream_workspace_bytes(*args) == 0, args
    # the existing entries keep their bytes (tests/test_decoder_layout_host.py holds the whole table)
    assert lib.effconf_ctc_beam_workspace_bytes(4, 50, 256, 16) == _al(16 * 4) + 4 * (_al(16 * 50 * 16) + _al(16 * 801) + _al(8 * 2048) + _al(4 * 2048)) + 256


def test_refusals_that_need_no_device():
    from efficientconformer_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(1 << 20)                                   # never dereferenced: every call below is refused before any launch
    err = lambda: lib.effconf_last_error()

    def resume(max_streams=4, max_frames=50, beam=4, n=2, t_new=5, vocab=32, tmp=1.0, nbest=4, max_tokens=50, ws_bytes=1 << 20, ptr=fake, logits=fake):
        return lib.effconf_ctc_beam_resume(ptr, max_streams, max_frames, beam, ptr, logits, ptr, n, t_new, vocab, tmp, nbest, ptr, ptr, ptr, ptr, max_tokens, ptr,
                                           ws_bytes, None)
    for kw, text in ((dict(beam=0), b"beam"), (dict(beam=33), b"beam"), (dict(vocab=1), b"vocab"), (dict(vocab=1025), b"vocab"),
                     (dict(max_frames=1 << 20, beam=16), b"too large"), (dict(max_streams=0), b"max_streams"), (dict(max_frames=0), b"max_frames"),
                     (dict(n=-1), b"bad shape"), (dict(t_new=-1), b"bad shape"), (dict(nbest=0), b"nbest"), (dict(nbest=5), b"nbest"), (dict(max_tokens=0), b"max_tokens"), (dict(max_tokens=(1 << 24) + 1), b"max_tokens"),
                     (dict(tmp=0.0), b"temperature"), (dict(tmp=float("inf")), b"temperature"), (dict(tmp=float("nan")), b"temperature"),
                     (dict(ws_bytes=_ws_bytes(2, 5, 4) - 1), b"workspace too small"), (dict(ptr=None), b"null argument"), (dict(logits=None), b"null argument")):
        assert resume(**kw) != 0 and text in err(), (kw, err())
    assert resume(n=0, ptr=None, logits=None) == 0               # nothing listed: nothing to do
    assert lib.effconf_ctc_beam_stream_init(fake, _state_bytes(4, 50, 4) - 1, 4, 50, 4, None) != 0 and b"state buffer too small" in err()
    assert lib.effconf_ctc_beam_stream_init(None, 1 << 30, 4, 50, 4, None) != 0 and b"null argument" in err()
    assert lib.effconf_ctc_beam_stream_init(fake, 1 << 30, 4, 50, 33, None) != 0 and b"beam" in err()
    for sid in (-1, 4, 1 << 30):
        assert lib.effconf_ctc_beam_stream_reset(fake, 4, sid, None) != 0 and b"stream id" in err()
    assert lib.effconf_ctc_beam_stream_reset(None, 4, 0, None) != 0 and b"null argument" in err()


def test_python_refusals_on_the_host():
    from efficientconformer_amd import ModelCTC, _lib, named_config, streaming
    r = streaming.beam_push_refusal
    assert r([0, 1], [3, 4], [0, 0, 0], 3, 10) is None
    assert r([2, 0], [10, 0], [0, 10, 0], 3, 10) is None
    assert "distinct" in r([0, 0], [1, 1], [0, 0, 0], 3, 10)
    assert "must be in 0 .. 2" in r([0, 3], [1, 1], [0, 0, 0], 3, 10) and "must be in 0 .. 2" in r([-1], [1], [0, 0, 0], 3, 10)
    assert "max_frames = 10" in r([1], [4], [0, 7, 0], 3, 10) and r([1], [3], [0, 7, 0], 3, 10) is None
    assert "one stream id per row" in r([0, 1], [1], [0, 0, 0], 3, 10)
    assert streaming.common_prefix_len([[1, 2, 3], [1, 2], [1, 2, 4]]) == 2 and streaming.common_prefix_len([[], [1]]) == 0
    assert streaming.common_prefix_len([[5, 6]]) == 2 and streaming.common_prefix_len([[1], [2]]) == 0
    cfg = named_config("Tiny")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = ModelCTC.from_config(cfg)
    with pytest.raises(ValueError, match="max_frames"):
        m.open_stream(2, None, beam_size=4)                       # the trie of a stream is sized by max_frames
    with pytest.raises(ValueError):
        m.open_beam_decode_stream(0, 10, 4)
    with pytest.raises(ValueError):
        m.open_beam_decode_stream(2, 0, 4)
    for beam in (0, 33):
        with pytest.raises(_lib.EffconfError):
            m.open_beam_decode_stream(2, 10, beam)
    with pytest.raises(RuntimeError):                             # parameters on the CPU and no device named: no fallback
        m.open_beam_decode_stream(2, 10, 4)
    plain = ModelCTC.from_config(named_config("Tiny"))            # not causal: everything stream_refusal refuses stays refused
    with pytest.raises((_lib.EffconfError, RuntimeError)):
        plain.open_stream(2, 100, beam_size=4)
