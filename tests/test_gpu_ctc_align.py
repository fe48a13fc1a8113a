"""CTC forced alignment and transcript scoring on the GPU (effconf_ctc_align, csrc/ctc_align.hip) against the float64 oracle
(tests/ctc_align_ref.py): path validity, spans, scores, likelihood, optimality and path identity on the shapes where the kernel changes
its work split, the status codes, independence of the batch / padding / workspace contents, the greedy property, the beam search's
scores and the model pipeline.

Bounds.  Scores against float64: 1e-5 (1 + |v|), the bound of the beam tests (about 11x the float32-vs-float64 noise of the recursions,
8.7e-7 (1 + |v|) for the likelihood and 7.8e-7 (1 + |v|) for the Viterbi score over 60 random cases up to T = 400).  Path identity with the
oracle is required wherever the oracle's smallest decision margin along its path is at least 1e-3; at most 1 case in 8 of a test may be
excused by a smaller margin (the seeds keep the oracle alone within that share)."""
import functools

import numpy as np
import pytest
import torch

from ctc_align_ref import check_path, forward, logp64, path_logp, status_of, viterbi
from efficientconformer_amd import ModelCTC, named_config, synth

pytestmark = pytest.mark.gpu

REL = 1e-5
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _aligner(tmp=1.0):
    """A ModelCTC used for align_logits / decode_logits_beam only (the logits come from the test, not from the encoder)."""
    cfg = named_config("Tiny")
    return ModelCTC(cfg["encoder_params"], cfg["tokenizer_params"], decoding_params={"beam_size": 4, "tmp": tmp})


def _pad(rows, tpad=None, fill=0.0):
    t = max([r.shape[0] for r in rows] + [1]) if tpad is None else tpad
    out = np.full((len(rows), t, rows[0].shape[1]), fill, dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out, np.array([r.shape[0] for r in rows], dtype=np.int64)


def _pad_targets(targets, upad=None, fill=0):
    u = max([len(y) for y in targets] + [0]) if upad is None else upad
    out = np.full((len(targets), u), fill, dtype=np.int32)
    for i, y in enumerate(targets):
        out[i, :len(y)] = y
    return out, np.array([len(y) for y in targets], dtype=np.int64)


def _align(logits, lens, targets, tmp=1.0, upad=None, ufill=0, scores_only=False):
    tg, tl = _pad_targets(targets, upad, ufill)
    out = _aligner(tmp).align_logits(torch.as_tensor(logits).cuda(), torch.as_tensor(np.asarray(lens, dtype=np.int64)).cuda(),
                                     torch.as_tensor(tg).cuda(), torch.as_tensor(tl).cuda(), scores_only=scores_only)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _close(a, b):
    if np.isneginf(b):
        return bool(np.isneginf(a))
    return bool(np.isfinite(a)) and abs(float(a) - b) <= REL * (1.0 + abs(b))


def _runs(ft, u):
    """first frame / last frame + 1 of every target index in a frame_token row"""
    start, end = [-1] * u, [-1] * u
    for t, c in enumerate(ft):
        if c >= 0:
            if t == 0 or ft[t - 1] != c:
                assert start[c] == -1, (c, t)
                start[c] = t
            end[c] = t + 1
    return start, end


def _check(logits, lens, targets, out, tmp=1.0):
    """Every invariant, the likelihood, optimality and - where the oracle's margin allows - path identity, for every utterance.
    -> (cases, cases excused from identity by a margin below 1e-3)."""
    b, t_all, v = logits.shape
    umax = out["token_start"].shape[1]
    assert out["frame_token"].shape == (b, t_all) and out["token_end"].shape == (b, umax) and out["token_logp"].shape == (b, umax)
    excused = 0
    for i in range(b):
        y = list(targets[i])
        u = len(y)
        n = int(min(max(lens[i], 0), t_all))
        st = status_of(n, y, v)
        tag = (i, n, u, st)
        assert out["status"][i] == st, tag
        ft = out["frame_token"][i]
        assert (ft[n:] == -1).all(), tag
        assert (out["token_start"][i, u:] == -1).all() and (out["token_end"][i, u:] == -1).all() and (out["token_logp"][i, u:] == 0).all(), tag
        if st != 0:
            assert np.isneginf(out["log_likelihood"][i]) and np.isneginf(out["score"][i]), tag
            assert (ft == -1).all() and (out["token_start"][i] == -1).all() and (out["token_end"][i] == -1).all(), tag
            assert (out["token_logp"][i] == 0).all(), tag
            continue
        assert check_path(ft[:n], y) is None, (tag, check_path(ft[:n], y))
        start, end = _runs(ft[:n].tolist(), u)
        assert out["token_start"][i, :u].tolist() == start and out["token_end"][i, :u].tolist() == end, tag
        lp = logp64(logits[i, :n], tmp)
        mine = path_logp(lp, ft[:n], y)
        assert _close(out["score"][i], mine), (tag, out["score"][i], mine)
        for k in range(u):
            want = float(lp[start[k]:end[k], y[k]].sum())
            assert _close(out["token_logp"][i, k], want), (tag, k, out["token_logp"][i, k], want)
        ll = forward(lp, n, y)
        assert _close(out["log_likelihood"][i], ll), (tag, out["log_likelihood"][i], ll)
        ref = viterbi(lp, n, y)
        assert abs(mine - ref["score"]) <= REL * (1 + abs(ref["score"])), (tag, mine, ref["score"])      # optimal whatever the ties do
        assert mine <= ll + 1e-9 * (1 + abs(ll)), tag
        if ref["margin"] >= MARGIN:
            assert ft[:n].tolist() == ref["frame_token"].tolist(), (tag, ref["margin"])
        else:
            excused += 1
    return b, excused


def _targets(rng, v, u, repeats=0.15):
    y = rng.integers(1, v, u).tolist()
    for k in range(1, u):
        if rng.random() < repeats:
            y[k] = y[k - 1]
    return y


def _need(y):
    return len(y) + sum(a == b for a, b in zip(y[:-1], y[1:]))


def _rows(rng, v, ts, scale=2.0):
    return [(rng.standard_normal((t, v)) * scale).astype(np.float32) for t in ts]


def shape_case(u):
    """Thread ownership changes with S = 2 U + 1 at 256 threads: one state per thread up to U = 127, two up to U = 255, three from 256 on.
    Frames: the feasibility edge (one path only), one above it, and room to spare."""
    rng = np.random.default_rng(7000 + u)
    targets = [_targets(rng, 32, u) for _ in range(4)]
    ts = [_need(targets[0]), _need(targets[1]) + 1, _need(targets[2]) + 37, 2 * _need(targets[3]) + 5]
    logits, lens = _pad(_rows(rng, 32, ts))
    return logits, lens, targets


@pytest.mark.parametrize("u", [0, 1, 2, 127, 128, 255, 256])
def test_states_per_thread_and_the_feasibility_edge(u):
    logits, lens, targets = shape_case(u)
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert excused == 0


def equal_case():
    rng = np.random.default_rng(31)
    targets, ts = [], []
    for u in (1, 2, 5, 64, 130):
        for extra in (0, 1, 4):
            targets.append([int(rng.integers(1, 8))] * u)
            ts.append(2 * u - 1 + extra)
    logits, lens = _pad(_rows(rng, 8, ts))
    return logits, lens, targets


def test_all_equal_targets_force_blanks():
    logits, lens, targets = equal_case()
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert 8 * excused <= n
    for i, y in enumerate(targets):                              # at T = 2 U - 1 the only path alternates token and blank
        if lens[i] == 2 * len(y) - 1:
            assert out["frame_token"][i, :lens[i]].tolist() == [k // 2 if k % 2 == 0 else -1 for k in range(lens[i])]


def vocab_case(v):
    rng = np.random.default_rng(9000 + v)
    us = [0, 3, 17, 40]
    targets = [_targets(rng, v, u) for u in us]
    ts = [5, _need(targets[1]) + 2, 3 * _need(targets[2]), 2 * _need(targets[3]) + 11]
    logits, lens = _pad(_rows(rng, v, ts, scale=3.0))
    return logits, lens, targets


@pytest.mark.parametrize("v", [2, 3, 257, 1000, 1024])
def test_vocabulary_sizes(v):
    """V = 2: every target is all-equal.  257 / 1000: rows off the 16-byte grid, a partial last quad.  1024: every lane's four quads."""
    logits, lens, targets = vocab_case(v)
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert excused == 0


@pytest.mark.parametrize("tmp", [0.5, 2.0])
def test_temperature(tmp):
    logits, lens, targets = vocab_case(257)
    out = _align(logits, lens, targets, tmp=tmp)
    n, excused = _check(logits, lens, targets, out, tmp=tmp)
    assert excused == 0
    other = _align(logits, lens, targets, tmp=1.0)
    assert not np.array_equal(out["log_likelihood"], other["log_likelihood"])


def test_one_frame_and_no_frames():
    rng = np.random.default_rng(3)
    logits = (rng.standard_normal((6, 1, 16)) * 2).astype(np.float32)
    lens = [1, 1, 1, 0, 0, 7]                                    # 7: clamped to T = 1
    targets = [[], [5], [5, 6], [], [5], [9]]
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert excused == 0
    assert out["status"].tolist() == [0, 0, 1, 0, 1, 0]
    assert out["log_likelihood"][3] == 0 and out["score"][3] == 0
    assert out["frame_token"][:, 0].tolist() == [-1, 0, -1, -1, -1, 0]
    # T = 0: no frame at all
    out = _align(np.zeros((2, 0, 16), dtype=np.float32), [0, 0], [[], [3]])
    assert out["status"].tolist() == [0, 1] and out["log_likelihood"][0] == 0 and np.isneginf(out["log_likelihood"][1])
    assert out["frame_token"].shape == (2, 0) and out["token_start"].tolist() == [[-1], [-1]]


def longest_case():
    rng = np.random.default_rng(2047)
    y = _targets(rng, 1024, 2047, repeats=0.01)
    t = _need(y)
    return (rng.standard_normal((1, t, 1024)) * 2).astype(np.float32), np.array([t]), [y]


def test_the_longest_target_at_its_smallest_frame_count():
    """U = 2047: S = 4095, 16 states per thread, backpointers in the workspace; at T = U + repeats there is exactly one path."""
    logits, lens, targets = longest_case()
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert excused == 0
    assert out["score"][0] == pytest.approx(out["log_likelihood"][0], rel=1e-6)


def test_status_codes_leave_the_rest_of_the_batch_alone():
    rng = np.random.default_rng(17)
    v = 40
    good = [_targets(rng, v, u) for u in (6, 9, 4)]
    ts = [20, 31, 12]
    rows = _rows(rng, v, ts)
    alone = [_align(r[None], [r.shape[0]], [y]) for r, y in zip(rows, good)]
    bad0 = list(good[1]); bad0[3] = 0                            # the blank as a target
    badv = list(good[1]); badv[8] = v                            # the first id outside the vocabulary
    few = _targets(rng, v, 14, repeats=0.0)
    few[5] = few[4]                                              # 15 frames needed
    batch_rows = [rows[0], rows[1], rows[1], rows[1][:14], rows[1][:15], rows[2]]
    targets = [good[0], bad0, badv, few, few, good[2]]
    logits, lens = _pad(batch_rows)
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert excused == 0
    assert out["status"].tolist() == [0, 2, 2, 1, 0, 0]
    for i, k in ((0, 0), (5, 2)):
        t, u = ts[k], len(good[k])
        for key in ("log_likelihood", "score", "status"):
            assert out[key][i].tobytes() == alone[k][key][0].tobytes(), (i, key)
        assert np.array_equal(out["frame_token"][i, :t], alone[k]["frame_token"][0])
        for key in ("token_start", "token_end", "token_logp"):
            assert out[key][i, :u].tobytes() == alone[k][key][0].tobytes(), (i, key)
    # an id beyond target_len is not an error: it is never read
    pad, _ = _pad_targets([good[0]], upad=10, fill=v + 5)
    m = _aligner()
    o = m.align_logits(torch.as_tensor(rows[0][None]).cuda(), None, torch.as_tensor(pad).cuda(), torch.tensor([6]).cuda())
    assert int(o["status"][0]) == 0


def test_results_do_not_depend_on_batch_padding_or_workspace(monkeypatch):
    rng = np.random.default_rng(23)
    v = 257                                                      # V % 4 = 1: a row's alignment changes with its position in the batch
    us = [12, 0, 33, 130, 5]
    targets = [_targets(rng, v, u) for u in us]
    ts = [40, 9, 70, 300, 5]
    rows = _rows(rng, v, ts)
    i = 2
    alone = _align(rows[i][None], [ts[i]], [targets[i]])
    _check(rows[i][None], [ts[i]], [targets[i]], alone)

    def same(out, k, what):
        for key in ("log_likelihood", "score", "status"):
            assert out[key][k].tobytes() == alone[key][0].tobytes(), (what, key)
        assert np.array_equal(out["frame_token"][k, :ts[i]], alone["frame_token"][0]) and (out["frame_token"][k, ts[i]:] == -1).all(), what
        for key in ("token_start", "token_end", "token_logp"):
            assert out[key][k, :us[i]].tobytes() == alone[key][0].tobytes(), (what, key)
            assert (out[key][k, us[i]:] == (0 if key == "token_logp" else -1)).all(), (what, key)

    logits, lens = _pad(rows)
    batch = _align(logits, lens, targets)
    same(batch, i, "batch of 5")
    _check(logits, lens, targets, batch)
    # larger T and U padding, NaN rows at or beyond len, garbage ids at or beyond target_len; U padding 600 also changes the launch's
    # states-per-thread bound (2 -> 8) and moves the backpointers from LDS to the workspace
    logits, lens = _pad(rows, tpad=420, fill=np.nan)
    padded = _align(logits, lens, targets, upad=600, ufill=-123456)
    same(padded, i, "padded")
    for k in range(5):
        assert padded["log_likelihood"][k].tobytes() == batch["log_likelihood"][k].tobytes(), k
        assert padded["score"][k].tobytes() == batch["score"][k].tobytes(), k
        assert np.array_equal(padded["frame_token"][k, :ts[k]], batch["frame_token"][k, :ts[k]]), k
        assert padded["token_logp"][k, :us[k]].tobytes() == batch["token_logp"][k, :us[k]].tobytes(), k
    same(_align(logits, lens, targets, upad=600, ufill=-123456), i, "second call")
    monkeypatch.setenv("EFFCONF_POISON_WORKSPACE", "255")
    same(_align(logits, lens, targets, upad=600, ufill=2 ** 31 - 1), i, "poisoned workspace, padded")
    same(_align(rows[i][None], [ts[i]], [targets[i]]), 0, "poisoned workspace, alone")


def test_scoring_only_is_bit_identical():
    for case in (shape_case(128), vocab_case(1000), longest_case()):
        logits, lens, targets = case
        full = _align(logits, lens, targets)
        only = _align(logits, lens, targets, scores_only=True)
        assert set(only) == {"log_likelihood", "status"}
        assert only["log_likelihood"].tobytes() == full["log_likelihood"].tobytes()
        assert np.array_equal(only["status"], full["status"])


def _peaked(seed, v=256, tmax=200):
    """The peaked (CTC-like) family of test_gpu_ctc_beam.py: a blank or one token stands out on every frame."""
    rng = np.random.default_rng(seed)
    t = int(rng.integers(20, tmax + 1))
    x = (rng.standard_normal((t, v)) * 1.5).astype(np.float32)
    spike = rng.random(t) < 0.35
    tok = rng.integers(1, v, t)
    x[np.arange(t), 0] += np.where(spike, 0.0, 9.0).astype(np.float32)
    x[np.arange(t), tok] += np.where(spike, 9.0, 0.0).astype(np.float32)
    return x, t


def _collapse(path):
    lab, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            lab.append(int(c))
        prev = c
    return lab


def peaked_case():
    rows = [_peaked(s)[0] for s in range(1001, 1017)]
    logits, lens = _pad(rows)
    targets = [_collapse(r.argmax(axis=1)) for r in rows]
    return rows, logits, lens, targets


def test_greedy_labels_align_to_the_argmax_path():
    """The best path over ALL labellings is the per-frame argmax, so the best path of the greedy labels is that path."""
    rows, logits, lens, targets = peaked_case()
    out = _align(logits, lens, targets)
    n, excused = _check(logits, lens, targets, out)
    assert 8 * excused <= n
    for i, r in enumerate(rows):
        lp = logp64(r)
        want = float(lp.max(axis=1).sum())
        assert _close(out["score"][i], want), (i, out["score"][i], want)
        top2 = np.sort(lp, axis=1)
        clear = top2[:, -1] - top2[:, -2] > MARGIN
        am = lp.argmax(axis=1)
        got = np.array([0 if c < 0 else targets[i][c] for c in out["frame_token"][i, :lens[i]]])
        assert np.array_equal(got[clear], am[clear]), i


def test_likelihood_bounds_the_beam_score():
    """The beam's score sums the alignments of its tokens that survived the pruning: never above log P(tokens), equal when nothing is pruned."""
    m = _aligner()
    rows, logits, lens, _ = peaked_case()
    lg, ln = torch.as_tensor(logits).cuda(), torch.as_tensor(lens).cuda()
    tokens, token_len, score = m.decode_logits_beam(lg, ln, 8)
    out = m.align_logits(lg, ln, tokens[:, 0, :min(lg.shape[1], 2047)].contiguous(), token_len[:, 0], scores_only=True)
    ll, sc = out["log_likelihood"].cpu().numpy(), score[:, 0].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all()
    for i in range(len(rows)):
        assert ll[i] >= sc[i] - REL * (1 + abs(sc[i])), (i, ll[i], sc[i])
    rng = np.random.default_rng(5)
    small = [(rng.standard_normal((t, 3)) * 2).astype(np.float32) for t in (1, 2, 3, 4, 5, 6, 6, 6)]
    logits, lens = _pad(small)
    lg, ln = torch.as_tensor(logits).cuda(), torch.as_tensor(lens).cuda()
    tokens, token_len, score = m.decode_logits_beam(lg, ln, 32)
    out = m.align_logits(lg, ln, tokens[:, 0].contiguous(), token_len[:, 0])
    ll, sc = out["log_likelihood"].cpu().numpy(), score[:, 0].cpu().numpy()
    for i in range(len(small)):
        assert abs(ll[i] - sc[i]) <= REL * (1 + abs(sc[i])), (i, ll[i], sc[i])
    host = {k: v.cpu().numpy() for k, v in out.items()}
    tl = token_len[:, 0].cpu().numpy()
    _check(logits, lens, [tokens[i, 0, :tl[i]].cpu().tolist() for i in range(len(small))], host)


class _Tok:
    def encode(self, s):
        return [int(c) for c in s.split()]


@functools.lru_cache(maxsize=None)
def _tiny():
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


@pytest.mark.parametrize("from_mel", [False, True])
def test_pipeline(from_mel):
    m = _tiny()
    fs = m.encoder.frame_seconds
    if from_mel:
        x, ln = synth.make_mel(3, m.encoder.plan.n_mels, 300, [300, 180, 77], seed=17)
    else:
        ln = np.array([48000, 32000, 9000], dtype=np.int64)
        x = synth.make_audio(ln, seed=3)
    x, x_len = torch.from_numpy(x).cuda(), torch.from_numpy(np.asarray(ln)).cuda()
    before = (m.greedy_labels(x, x_len, from_mel=from_mel), m.beam_labels(x, x_len, 4, from_mel=from_mel))
    enc, enc_len, _ = m.encoder.forward_mel(x, x_len) if from_mel else m.encoder(x, x_len)
    logits, _, _ = m._head(enc, enc_len, want_logits=True)
    if not from_mel:
        fwd, fwd_len, _ = m((x, None, x_len, None))
        assert torch.equal(fwd, logits) and torch.equal(fwd_len, enc_len)
    v = logits.shape[2]
    rng = np.random.default_rng(11)
    nfr = enc_len.cpu().numpy()
    y = [_targets(rng, v, int(max(0, min(n // 3, 12)))) for n in nfr]
    y[2] = [y[2][0], y[2][0], y[2][1]]                           # equal neighbours: a blank between them
    want = m.align_logits(logits, enc_len, y)
    want = {k: t.cpu().numpy() for k, t in want.items()}
    _check(logits.cpu().numpy(), nfr, y, want)
    recs = m.align(x, x_len, y, from_mel=from_mel)
    scores = m.score_labels(x, x_len, y, from_mel=from_mel)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.cpu().numpy().tobytes() == want["log_likelihood"].tobytes()
    for i, r in enumerate(recs):
        u = len(y[i])
        assert r.tokens == y[i] and r.status == 0
        assert r.start_frame == want["token_start"][i, :u].tolist() and r.end_frame == want["token_end"][i, :u].tolist()
        assert r.start_time == [f * fs for f in r.start_frame] and r.end_time == [f * fs for f in r.end_frame]
        assert np.float32(r.score).tobytes() == want["score"][i].tobytes()
        assert np.float32(r.log_likelihood).tobytes() == want["log_likelihood"][i].tobytes()
        assert np.asarray(r.token_logp, dtype=np.float32).tobytes() == want["token_logp"][i, :u].tobytes()
        for k in range(u):
            assert 0 <= r.start_frame[k] < r.end_frame[k] <= nfr[i]
            if k + 1 < u:
                assert r.end_frame[k] <= r.start_frame[k + 1]
                if y[i][k] == y[i][k + 1]:
                    assert r.end_frame[k] < r.start_frame[k + 1]
    # strings through the tokenizer, a padded tensor with lengths
    m.tokenizer = _Tok()
    try:
        assert m.align(x, x_len, [" ".join(str(c) for c in r) for r in y], from_mel=from_mel) == recs
    finally:
        m.tokenizer = None
    tg, tl = _pad_targets(y, upad=20, fill=0)
    assert m.align(x, x_len, torch.as_tensor(tg), torch.as_tensor(tl), from_mel=from_mel) == recs
    # greedy labels with their timestamps = align on the greedy labels
    greedy = m.greedy_alignment(x, x_len, from_mel=from_mel)
    assert [g.tokens for g in greedy] == before[0]
    assert greedy == m.align(x, x_len, before[0], from_mel=from_mel)
    assert before == (m.greedy_labels(x, x_len, from_mel=from_mel), m.beam_labels(x, x_len, 4, from_mel=from_mel))
