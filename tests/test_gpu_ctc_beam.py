"""CTC prefix beam search on the GPU (effconf_ctc_beam; reference model_ctc.py:138-181 = ctcdecode without the n-gram scorer):
every frame's beam against a float64 recomputation from the kernel's own previous beam, token identity with the float64 oracle
(tests/ctc_beam_ref.py) where the oracle's decisions are clear, exact cases, prefix re-entry, independence of the batch and the
padding, edge cases and the model pipeline."""
import functools
import os

import numpy as np
import pytest
import torch

from ctc_beam_ref import beam_search, brute_force, ctc_log_prob, logp32, logp64, lse
from efficientconformer_amd import ModelCTC, named_config, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# peaked (CTC-like) utterances whose float64 beams at 1 / 4 / 16 have no decision closer than 1e-3 (found with the oracle)
PEAKED_SEEDS = [1001, 1002, 1003, 1009, 1010, 1012, 1013, 1014, 1015, 1017, 1018, 1022, 1023, 1024, 1026, 1028]


@functools.lru_cache(maxsize=None)
def _decoder(tmp=1.0):
    """A ModelCTC used for decode_logits_beam only (the logits come from the test, not from the encoder)."""
    cfg = named_config("Tiny")
    return ModelCTC(cfg["encoder_params"], cfg["tokenizer_params"], decoding_params={"beam_size": 4, "tmp": tmp})


def _decode(logits, lens, beam, tmp=1.0, trace=False):
    m = _decoder(tmp)
    lg = torch.as_tensor(logits).cuda()
    ln = None if lens is None else torch.as_tensor(np.asarray(lens, dtype=np.int64)).cuda()
    tokens, token_len, score = m.decode_logits_beam(lg, ln, beam)
    tokens, token_len, score = tokens.cpu().numpy(), token_len.cpu().numpy(), score.cpu().numpy()
    assert tokens.shape == (lg.shape[0], beam, lg.shape[1]) and score.shape == (lg.shape[0], beam)
    for i in range(tokens.shape[0]):
        for r in range(beam):
            assert not tokens[i, r, token_len[i, r]:].any()                         # zero-filled tails
    toks = [[tuple(tokens[i, r, :token_len[i, r]].tolist()) for r in range(beam)] for i in range(tokens.shape[0])]
    return toks, token_len, score, (m.last_beam_trace() if trace else None)


def _flat(rng, b, t, v):
    return (rng.standard_normal((b, t, v)) * 1.0).astype(np.float32)


def _peaked(seed, v=256, tmax=200):
    rng = np.random.default_rng(seed)
    t = int(rng.integers(20, tmax + 1))
    x = (rng.standard_normal((t, v)) * 1.5).astype(np.float32)
    spike = rng.random(t) < 0.35
    tok = rng.integers(1, v, t)
    x[np.arange(t), 0] += np.where(spike, 0.0, 9.0).astype(np.float32)
    x[np.arange(t), tok] += np.where(spike, 9.0, 0.0).astype(np.float32)
    return x, t


def _pad(rows, tpad=None, fill=0.0):
    t = tpad or max(r.shape[0] for r in rows)
    out = np.full((len(rows), t, rows[0].shape[1]), fill, dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out, np.array([r.shape[0] for r in rows], dtype=np.int64)


def _strings(tr):
    """node -> token string of the kernel's trie"""
    memo = {0: ()}

    def get(n):
        chain = []
        while n not in memo:
            chain.append(n)
            n = int(tr["parent"][n])
        s = memo[n]
        for c in reversed(chain):
            s = s + (int(tr["token"][c]),)
            memo[c] = s
        return s
    return get


def _close(a, b, rel):
    if np.isneginf(b):
        return np.isneginf(a)
    return np.isfinite(a) and abs(a - b) <= rel * (1.0 + abs(b))


def _check_steps(logits, lens, beam, tmp, tr):
    """Every frame: the kernel's beam at t is a duplicate-free subset of the candidates of its own beam at t - 1 (recomputed in
    float64, every candidate), pb / pnb within 1e-5 (1 + |v|), nothing dropped above the smallest kept score beyond 1e-5 (1 + |s|),
    ranks ordered."""
    for i in range(logits.shape[0]):
        L = int(min(max(lens[i], 0), logits.shape[1]))
        u = tr[i]
        assert u["len"] == L
        lp = logp64(logits[i, :L], tmp)
        name = _strings(u)
        members = [((), 0.0, -np.inf)]
        v = lp.shape[1]
        for t in range(L):
            row = lp[t]
            n = len(members)
            s = np.array([float(lse(pb, pnb)) for _, pb, pnb in members])
            mpb = row[0] + s
            mnb = np.array([row[p[-1]] + pnb if p else -np.inf for p, _, pnb in members])
            ext = row[None, :] + s[:, None]
            for k, (p, pb, _) in enumerate(members):
                if p:
                    ext[k, p[-1]] = row[p[-1]] + pb
            valid = np.ones((n, v), dtype=bool)
            valid[:, 0] = False
            pos = {p: k for k, (p, _, _) in enumerate(members)}
            for k, (p, _, _) in enumerate(members):
                if p and p[:-1] in pos:
                    j = pos[p[:-1]]
                    mnb[k] = float(lse(mnb[k], ext[j, p[-1]]))
                    valid[j, p[-1]] = False
            msc = np.array([float(lse(a, b)) for a, b in zip(mpb, mnb)])
            nodes = u["node"][t]
            kept = [int(x) for x in nodes if x >= 0]
            assert list(nodes[:len(kept)]) == kept and len(kept) == min(beam, n + int(valid.sum()))
            strs = [name(x) for x in kept]
            assert len(set(strs)) == len(strs), (i, t)
            keep_m = np.zeros(n, dtype=bool)
            keep_e = np.zeros((n, v), dtype=bool)
            kept_scores = []
            for r, q in enumerate(strs):
                if q in pos:
                    k = pos[q]
                    want_pb, want_nb, want_s = mpb[k], mnb[k], msc[k]
                    keep_m[k] = True
                else:
                    assert q and q[:-1] in pos and valid[pos[q[:-1]], q[-1]], (i, t, q)
                    k, c = pos[q[:-1]], q[-1]
                    want_pb, want_nb, want_s = -np.inf, ext[k, c], ext[k, c]
                    keep_e[k, c] = True
                assert _close(float(u["pb"][t, r]), want_pb, 1e-5) and _close(float(u["pnb"][t, r]), want_nb, 1e-5), \
                    (i, t, r, u["pb"][t, r], want_pb, u["pnb"][t, r], want_nb)
                kept_scores.append(want_s)
            dropped = np.concatenate([msc[~keep_m], ext[valid & ~keep_e]])
            if dropped.size and np.isfinite(dropped.max()):
                lo = min(kept_scores)
                assert lo >= dropped.max() - 1e-5 * (1 + abs(lo)), (i, t, lo, dropped.max())
            ks = u["score"][t, :len(kept)]
            assert all(ks[r] >= ks[r + 1] for r in range(len(kept) - 1)), (i, t, ks)
            members = [(q, float(u["pb"][t, r]), float(u["pnb"][t, r])) for r, q in enumerate(strs)]


@pytest.mark.parametrize("v", [32, 256, 1000])
@pytest.mark.parametrize("beam", [1, 4, 16, 32])
def test_every_frame_against_float64_candidates(v, beam):
    rng = np.random.default_rng(1000 * v + beam)
    for tmp in (0.5, 1.0, 2.0):
        t = 200 if v < 1000 else 120
        logits = _flat(rng, 8, t, v)
        lens = rng.integers(1, t + 1, 8)
        lens[0] = t
        _, _, _, tr = _decode(logits, lens, beam, tmp, trace=True)
        _check_steps(logits, lens, beam, tmp, tr)


@pytest.mark.parametrize("beam", [1, 4, 16])
def test_identity_with_the_oracle_on_peaked_logits(beam):
    assert len(PEAKED_SEEDS) == 16
    rows = [_peaked(s)[0] for s in PEAKED_SEEDS]
    logits, lens = _pad(rows)
    toks, _, score, _ = _decode(logits, lens, beam)
    for i, s in enumerate(PEAKED_SEEDS):
        lp = logp64(rows[i])
        ref = beam_search(lp, int(lens[i]), beam)
        assert ref["gap"] >= 1e-3, (s, ref["gap"])
        assert toks[i][:len(ref["prefixes"])] == ref["prefixes"], (s, beam)
        assert np.all(np.abs(score[i, :len(ref["score"])] - ref["score"]) <= 1e-4 * np.abs(ref["score"])), (s, beam)
        # the kernel's best score is a lower bound of the total probability of its tokens
        assert score[i, 0] <= ctc_log_prob(lp, int(lens[i]), toks[i][0]) + 1e-4


def test_exact_distribution_when_nothing_is_pruned():
    """V = 3, T <= 3, beam 16: every reachable labelling is in the beam with its total log-probability."""
    rng = np.random.default_rng(5)
    rows = [(rng.standard_normal((t, 3)) * 2).astype(np.float32) for t in (1, 2, 3, 3, 2, 3)]
    logits, lens = _pad(rows)
    toks, tlen, score, _ = _decode(logits, lens, 16)
    for i, r in enumerate(rows):
        want = brute_force(logp64(r))
        got = {toks[i][k]: float(score[i, k]) for k in range(16) if np.isfinite(score[i, k]) and (k == 0 or tlen[i, k] > 0 or toks[i][k] == ())}
        got = {p: s for p, s in got.items() if np.isfinite(s)}
        assert set(got) == set(want), (i, sorted(got), sorted(want))
        for p, s in got.items():
            assert abs(s - want[p]) <= 1e-5 * (1 + abs(want[p])), (p, s, want[p])


def test_prefix_reentry_merges_by_string():
    """Fixtures on which identifying prefixes by (parent slot, token) changes the best tokens: the kernel follows string identity."""
    g = np.load(os.path.join(GOLDEN, "ctc_beam_reentry.npz"))
    assert int(g["count"]) >= 2
    for j in range(int(g["count"])):
        lg, beam = g["logits_%d" % j], int(g["beam_%d" % j])
        want, slot = tuple(g["best_string_%d" % j].tolist()), tuple(g["best_slot_%d" % j].tolist())
        lp = logp64(lg)
        assert beam_search(lp, None, beam)["prefixes"][0] == want
        assert beam_search(lp, None, beam, slot_identity=True)["prefixes"][0] == slot != want
        toks, _, score, _ = _decode(lg[None], None, beam)
        assert toks[0][0] == want, (j, toks[0][0], want, slot)
        assert score[0, 0] <= ctc_log_prob(lp, lg.shape[0], want) + 1e-4


def test_results_do_not_depend_on_batch_or_padding():
    rng = np.random.default_rng(9)
    pool = [_peaked(s, v=128, tmax=120)[0] for s in range(24)] + [(rng.standard_normal((int(rng.integers(1, 90)), 128))).astype(np.float32)
                                                                  for _ in range(8)]
    alone = [_decode(r[None], None, 8) for r in pool]
    src = rng.integers(0, len(pool), 64)
    logits, lens = _pad([pool[s] for s in src], tpad=150, fill=np.nan)       # frames at or beyond len are never read
    toks, tlen, score, _ = _decode(logits, lens, 8)
    for k, s in enumerate(src):
        assert toks[k] == alone[s][0][0]
        assert score[k].tobytes() == alone[s][2][0].tobytes() and (tlen[k] == alone[s][1][0]).all()
    again = _decode(logits, lens, 8)
    assert again[0] == toks and again[2].tobytes() == score.tobytes()


def test_edge_cases():
    rng = np.random.default_rng(13)
    lg = _flat(rng, 4, 6, 16)
    toks, tlen, score, _ = _decode(lg, [0, 1, 6, 100], 4)
    assert toks[0][0] == () and score[0, 0] == 0 and (tlen[0] == 0).all() and np.isneginf(score[0, 1:]).all()
    ref = beam_search(logp64(lg[1]), 1, 4)
    assert toks[1][:len(ref["prefixes"])] == ref["prefixes"]
    assert toks[3] == _decode(lg[3:4], [6], 4)[0][0]                         # len > T is clamped
    # all-blank frames: the empty prefix wins
    blank = np.zeros((2, 30, 16), dtype=np.float32)
    blank[:, :, 0] = 12.0
    toks, _, score, _ = _decode(blank, None, 4)
    assert toks[0][0] == () and toks[1][0] == () and score[0, 0] > -0.01
    # gaps above 150: -inf log-probabilities, no NaN; the oracle on torch's fp32 softmax().log() (what the kernel evaluates)
    rows = []
    for s in range(4):
        x, _ = _peaked(500 + s, v=64, tmax=60)
        x[:, :] *= 20.0
        rows.append(x)
    logits, lens = _pad(rows)
    for beam in (1, 4, 16):
        toks, _, score, _ = _decode(logits, lens, beam)
        assert not np.isnan(score).any()
        for i, r in enumerate(rows):
            lp = logp32(r)
            assert np.isneginf(lp).any()
            ref = beam_search(lp, int(lens[i]), beam, shortcut=True)
            assert toks[i][:len(ref["prefixes"])] == ref["prefixes"], (i, beam)
            fin = np.isfinite(ref["score"])
            assert np.all(np.abs(score[i, :len(fin)][fin] - ref["score"][fin]) <= 1e-4 * (1 + np.abs(ref["score"][fin])))
            assert np.isneginf(score[i, :len(fin)][~fin]).all()
    # beam > V, V = 2, V = 1024, T = 2000: every frame against float64
    for b, t, v, beam in [(3, 40, 2, 8), (3, 40, 3, 32), (2, 60, 1024, 16), (2, 2000, 64, 4)]:
        lg = _flat(rng, b, t, v)
        lens = np.array([t] + [max(1, t // 2)] * (b - 1))
        _, _, _, tr = _decode(lg, lens, beam, trace=True)
        _check_steps(lg, lens, beam, 1.0, tr)


class _Tok:
    def decode(self, ids):
        return [" ".join(str(i) for i in x) for x in ids]


@functools.lru_cache(maxsize=None)
def _small(precision):
    cfg = named_config("EfficientConformerCTCSmall")
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.encoder.precision = precision
    return m.cuda()


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_pipeline_matches_decode_of_the_model_logits(precision):
    m = _small(precision)
    assert m.beam_size == 16
    lens = np.array([48000, 32000, 16000], dtype=np.int64)
    x = torch.from_numpy(synth.make_audio(lens, seed=3)).cuda()
    x_len = torch.from_numpy(lens).cuda()
    ids = m.beam_search_decoding(x, x_len)
    logits, logits_len, _ = m((x, None, x_len, None))
    tokens, token_len, score = m.decode_logits_beam(logits, logits_len)
    want = [tokens[i, 0, :int(token_len[i, 0])].tolist() for i in range(3)]
    assert ids == want
    assert np.isfinite(score[:, 0].cpu().numpy()).all()
    m.tokenizer = _Tok()
    try:
        assert m.beam_search_decoding(x, x_len) == _Tok().decode(want)
    finally:
        m.tokenizer = None
    mel, ln = synth.make_mel(2, 80, 300, [300, 180], seed=17)
    mel, ln = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    got = m.beam_labels(mel, ln, beam_size=4, from_mel=True)
    enc, enc_len, _ = m.encoder.forward_mel(mel, ln)
    lg, _, _ = m._head(enc, enc_len, want_logits=True)
    t4, l4, _ = m.decode_logits_beam(lg, enc_len, 4)
    assert got == [t4[i, 0, :int(l4[i, 0])].tolist() for i in range(2)]
