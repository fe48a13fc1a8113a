"""CTC prefix beam search with neural-LM shallow fusion on the GPU (effconf_ctc_beam_lm): token identity at every rank with the float64
oracle (tests/ctc_beam_lm_ref.py) on the fixtures of tests/ctc_beam_lm_cases.py (whose decisions tests/test_ctc_beam_lm_host.py shows to be clear), the
scores against float64 within the bounds of the two halves (the plain search's 1e-4 (1 + |s|); 8 x the float32 noise of the LM, measured on the CPU, times the
length), every frame of the kernel's trace against a float64 recomputation from its own previous beam, the total's formula bit for bit, independence of the
batch / order / padding / chunking / workspace contents, and the model pipeline."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_cases as cases
import lm_ref
from ctc_beam_ref import logp64, lse
from lm_cases import fixture, float32_noise
from efficientconformer_amd import LanguageModel, ModelCTC, model_ctc, named_config, synth
from efficientconformer_amd.model_ctc import select_nbest

pytestmark = pytest.mark.gpu
FACTOR = 8.0
NAMES = [c.name for c in cases.CASES]


@functools.lru_cache(maxsize=None)
def _decoder(tmp=1.0):
    """A ModelCTC used for decode_logits_beam_lm only (the logits come from the test, not from the encoder)."""
    cfg = named_config("Tiny")
    return ModelCTC(cfg["encoder_params"], cfg["tokenizer_params"], decoding_params={"beam_size": 4, "tmp": tmp})


@functools.lru_cache(maxsize=None)
def _lm(name):
    c = cases.BY_NAME[name]
    m = LanguageModel(cases.lm_params(c))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.lm_weights(name).items()})
    return m.cuda()


def _decode(name, logits, lens, trace=False):
    c = cases.BY_NAME[name]
    m = _decoder(c.tmp)
    lg = torch.as_tensor(logits).cuda()
    ln = torch.as_tensor(np.asarray(lens, dtype=np.int64)).cuda()
    out = m.decode_logits_beam_lm(lg, ln, c.beam, lm=_lm(name), lm_weight=c.weight, lm_tmp=c.lm_tmp, length_bonus=c.bonus)
    tokens, token_len, total, am, lms = (x.cpu().numpy() for x in out)
    assert tokens.shape == (lg.shape[0], c.beam, lg.shape[1]) and total.shape == am.shape == lms.shape == token_len.shape == (lg.shape[0], c.beam)
    for i in range(tokens.shape[0]):
        for r in range(c.beam):
            assert not tokens[i, r, token_len[i, r]:].any()                         # zero-filled tails
    rounds = m.last_beam_rounds()
    assert rounds is not None and all(1 <= r <= lg.shape[1] + 2 for r in rounds), (rounds, lg.shape)
    return {"tokens": tokens, "token_len": token_len, "total": total, "am": am, "lm": lms, "rounds": rounds,
            "trace": m.last_beam_trace() if trace else None, "dev": out}


def _lm_bound(name, tokens, token_len):
    """(float64 LM score of every hypothesis, the bound a float32 LM score is held to: 8 x the case's float32 noise x the length)."""
    c = cases.BY_NAME[name]
    flat = tokens.reshape(-1, tokens.shape[-1]).astype(np.int64)
    flat_len = token_len.reshape(-1).astype(np.int64)
    if flat.shape[1] == 0:
        flat = np.zeros((flat.shape[0], 1), dtype=np.int64)
    sd = cases.lm_weights(name)
    want_lp, want, _ = lm_ref.token_logprobs(sd, flat, flat_len, c.lm_tmp)
    noise = float32_noise(cases.lm_params(c), sd, flat, flat_len, c.lm_tmp, want_lp)
    return want.reshape(token_len.shape), noise, FACTOR * noise * np.maximum(token_len, 1)


@pytest.mark.parametrize("name", NAMES)
def test_identity_with_the_oracle_and_the_score_bounds(name):
    c = cases.BY_NAME[name]
    _, pad, lens = cases.logits(name)
    got = _decode(name, pad, lens)
    want_lm, noise, bound = _lm_bound(name, got["tokens"], got["token_len"])
    worst = 0.0
    for i, ref in enumerate(cases.oracle(name)):
        k = len(ref["prefixes"])
        toks = [tuple(got["tokens"][i, r, :got["token_len"][i, r]].tolist()) for r in range(c.beam)]
        assert toks[:k] == ref["prefixes"], (name, i)
        fin = np.isfinite(ref["score"])                                           # a prefix without mass yet: -inf on both sides
        assert np.array_equal(np.isneginf(got["am"][i, :k]), ~fin), (name, i)
        assert np.all(np.abs(got["am"][i, :k][fin] - ref["score"][fin]) <= 1e-4 * (1 + np.abs(ref["score"][fin]))), (name, i)
        err = np.abs(got["lm"][i, :k].astype(np.float64) - ref["lm"])
        assert np.all(err <= bound[i, :k]), (name, i, err.max(), noise)
        assert np.allclose(ref["lm"], want_lm[i, :k], rtol=0, atol=1e-9)          # the oracle's L is lm_ref's score of the same tokens
        worst = max(worst, float((err / np.maximum(bound[i, :k] / FACTOR, 1e-30)).max()) if noise > 0 else 0.0)
        # ranks without a hypothesis
        assert not got["token_len"][i, k:].any() and np.all(np.isneginf(got["total"][i, k:])) and np.all(np.isneginf(got["am"][i, k:]))
        assert not got["lm"][i, k:].any()
    print("%s: float32 noise of the LM %.3g, worst |lm_score - float64| / (noise x length) %.3g, rounds %s" % (name, noise, worst, got["rounds"]))
    # total is select_nbest's formula on the returned scores, bit for bit; the ranks are in its order
    tokens_d, token_len_d, total_d, am_d, lm_d = got["dev"]
    _, want_total = select_nbest(am_d, lm_d, token_len_d, c.weight, c.bonus)
    assert np.array_equal(want_total.cpu().numpy(), got["total"])
    assert np.all(got["total"][:, :-1] >= got["total"][:, 1:])
    # lm_score against LanguageModel.score of the returned tokens: two float32 evaluations of the same sum
    b, beam, t = tokens_d.shape
    if t:
        sc = _lm(name).score(tokens_d.reshape(b * beam, t), token_len_d.reshape(-1), lm_tmp=c.lm_tmp).reshape(b, beam).cpu().double().numpy()
        assert np.all(np.abs(sc - got["lm"]) <= bound), (name, np.abs(sc - got["lm"]).max())


def _strings(tr):
    """node -> token string of the kernel's trie"""
    memo = {0: ()}

    def get(n):
        chain = []
        while n not in memo:
            chain.append(n)
            n = int(tr["parent"][n])
        s = memo[n]
        for x in reversed(chain):
            s = s + (int(tr["token"][x]),)
            memo[x] = s
        return s
    return get


def _close(a, b, rel):
    if np.isneginf(b):
        return np.isneginf(a)
    return np.isfinite(a) and abs(a - b) <= rel * (1.0 + abs(b))


@pytest.mark.parametrize("name", ["v32_b4_cols16", "v257_b4_cols32", "v1024_b32_cols64", "v2_b4_short", "v32_b16_tmps", "v257_b1_bonus"])
def test_every_frame_against_float64_candidates(name):
    """Every frame: the kernel's beam at t is a duplicate-free subset of the candidates of its own beam at t - 1 (recomputed in float64, every candidate),
    pb / pnb within 1e-5 (1 + |v|), the L of every member within the LM bound of the float64 L of its string and identical every time the string shows up,
    the traced total the formula's bits, and nothing dropped whose total lies above the smallest kept total by more than 1e-5 (1 + |total|) plus the LM bound."""
    c = cases.BY_NAME[name]
    rows, pad, lens = cases.logits(name)
    got = _decode(name, pad, lens, trace=True)
    lm64 = cases.rows64(name)
    _, noise, _ = _lm_bound(name, got["tokens"], got["token_len"])
    w, bonus, v, beam = c.weight, c.bonus, c.v, c.beam
    f32 = np.float32
    assert len(got["trace"]) == len(lens)
    for i, u in enumerate(got["trace"]):
        L = int(lens[i])
        assert u["len"] == L
        lp = logp64(rows[i], c.tmp) if L else np.zeros((0, v))
        name_of = _strings(u)
        members = [((), 0.0, -np.inf)]
        Lseen = {(): f32(0.0)}
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
            mtot = np.array([msc[k] + w * lm64.L(p) + bonus * len(p) for k, (p, _, _) in enumerate(members)])
            etot = np.stack([ext[k] + w * (lm64.L(p) + lm64.row(p)) + bonus * (len(p) + 1) for k, (p, _, _) in enumerate(members)])
            nodes = u["node"][t]
            kept = [int(x) for x in nodes if x >= 0]
            assert list(nodes[:len(kept)]) == kept and len(kept) == min(beam, n + int(valid.sum()))
            strs = [name_of(x) for x in kept]
            assert len(set(strs)) == len(strs), (i, t)
            keep_m = np.zeros(n, dtype=bool)
            keep_e = np.zeros((n, v), dtype=bool)
            kept_tot = []
            maxlen = max(len(q) for q in strs) + 1
            for r, q in enumerate(strs):
                if q in pos:
                    k = pos[q]
                    want_pb, want_nb, want_t = mpb[k], mnb[k], mtot[k]
                    keep_m[k] = True
                else:
                    assert q and q[:-1] in pos and valid[pos[q[:-1]], q[-1]], (i, t, q)
                    k, tok = pos[q[:-1]], q[-1]
                    want_pb, want_nb, want_t = -np.inf, ext[k, tok], etot[k, tok]
                    keep_e[k, tok] = True
                assert _close(float(u["pb"][t, r]), want_pb, 1e-5) and _close(float(u["pnb"][t, r]), want_nb, 1e-5), \
                    (i, t, r, u["pb"][t, r], want_pb, u["pnb"][t, r], want_nb)
                Lk = u["lm"][t, r]
                assert abs(float(Lk) - lm64.L(q)) <= FACTOR * noise * max(len(q), 1), (i, t, q, Lk, lm64.L(q))
                assert Lseen.setdefault(q, Lk) == Lk and u["node_lm"][kept[r]] == Lk, (i, t, q)      # one L per string, the node's
                want_total = f32(f32(u["score"][t, r]) + f32(f32(w) * Lk)) + f32(f32(bonus) * f32(len(q)))
                assert u["total"][t, r] == f32(want_total) or (np.isneginf(u["score"][t, r]) and np.isneginf(u["total"][t, r])), (i, t, r)
                kept_tot.append(want_t)
            dropped = np.concatenate([mtot[~keep_m], etot[valid & ~keep_e]])
            if dropped.size and np.isfinite(dropped.max()):
                lo = min(kept_tot)
                assert lo >= dropped.max() - 1e-5 * (1 + abs(lo)) - 2 * w * FACTOR * noise * maxlen, (i, t, lo, dropped.max())
            ks = u["total"][t, :len(kept)]
            assert all(ks[r] >= ks[r + 1] for r in range(len(kept) - 1)), (i, t, ks)
            members = [(q, float(u["pb"][t, r]), float(u["pnb"][t, r])) for r, q in enumerate(strs)]


def test_results_do_not_depend_on_batch_order_padding_chunks_or_workspace(monkeypatch):
    name = "v32_b4_cols16"
    c = cases.BY_NAME[name]
    rows, pad, lens = cases.logits(name)
    keys = ("tokens", "token_len", "total", "am", "lm")

    def bits(out, i, t=None):
        return [out[k][i, :, :t].copy() if k == "tokens" else out[k][i].copy().view(np.int32) for k in keys]

    def same(a, b, what):
        for x, y, k in zip(a, b, keys):
            assert np.array_equal(x, y), (what, k)
    alone = []
    for i, r in enumerate(rows):
        out = _decode(name, r[None], [r.shape[0]])
        alone.append(bits(out, 0))
    # a mixed batch of 33: the four utterances among truncated copies, padded to the longest; NaN behind every length
    order = [j % 4 for j in range(33)]
    cut = [rows[j].shape[0] if k < 4 else max(1, rows[j].shape[0] - 3 * (k // 4)) for k, j in enumerate(order)]
    tmax = max(cut) + 5
    big = np.full((33, tmax, c.v), np.nan, dtype=np.float32)
    for k, j in enumerate(order):
        big[k, :cut[k]] = rows[j][:cut[k]]
    mixed = _decode(name, big, cut)
    assert max(mixed["rounds"]) <= tmax + 2
    for k in range(4):
        same(bits(mixed, k, rows[order[k]].shape[0]), alone[order[k]], "batch of 33 + NaN padding")
        assert not mixed["tokens"][k, :, rows[order[k]].shape[0]:].any()
    rev = _decode(name, big[::-1].copy(), cut[::-1])
    for k in range(33):
        same(bits(rev, 32 - k), bits(mixed, k), "reversed")
    # the Python chunk boundary: a cap that one utterance's workspace already exceeds -> 33 calls of one utterance
    monkeypatch.setattr(model_ctc, "BEAM_LM_WORKSPACE_CAP", 1)
    chunked = _decode(name, big, cut)
    monkeypatch.undo()
    assert len(chunked["rounds"]) == 33
    for k in range(33):
        same(bits(chunked, k), bits(mixed, k), "chunked")
    monkeypatch.setenv("EFFCONF_POISON_WORKSPACE", "255")
    poisoned = _decode(name, big, cut)
    monkeypatch.delenv("EFFCONF_POISON_WORKSPACE")
    for k in range(33):
        same(bits(poisoned, k), bits(mixed, k), "0xFF workspace")


class _Tok:
    def decode(self, ids):
        return [" ".join(str(i) for i in row) for row in ids]


def test_pipeline_on_the_tiny_model_with_the_tiny_lm():
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(dict(cfg, decoding_params={"beam_size": 8, "tmp": 1}))
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    # TinyLM's widths at Tiny's vocabulary (the golden TinyLM has its own vocabulary of 40: the fused entry refuses an LM whose vocabulary is not the logits')
    g, params, _ = fixture("TinyLM")
    v = cfg["tokenizer_params"]["vocab_size"]
    params = dict(params, vocab_size=v)
    lsd = synth.make_lm_state_dict(params, 21, bias=(np.random.default_rng(21).standard_normal(v) * 2.0).astype(np.float32))
    lm = LanguageModel(params)
    lm.load_state_dict({k: torch.from_numpy(x) for k, x in lsd.items()})
    lm = lm.cuda()
    w = float(g["rescore_lm_weight"])
    with pytest.raises(Exception, match="vocab"):
        wrong = LanguageModel(fixture("TinyLM")[1]).cuda()
        m.decode_logits_beam_lm(torch.zeros(1, 3, v, device="cuda"), None, lm=wrong, lm_weight=w)
    lens = np.array([32000, 24000, 16000], dtype=np.int64)
    x, x_len = torch.from_numpy(synth.make_audio(lens, seed=3)).cuda(), torch.from_numpy(lens).cuda()
    plain = m.beam_labels(x, x_len)
    assert m.beam_search_fused(x, x_len) == plain                                               # no LM attached: beam_labels' result
    assert m.beam_labels_fused(x, x_len, lm=lm, lm_weight=0.0) == plain                         # weight 0
    assert m.last_beam_rounds() is None
    logits, logits_len, _ = m((x, None, x_len, None))
    tokens, token_len, total, am, lms = m.decode_logits_beam_lm(logits, logits_len, lm=lm, lm_weight=w)
    want = [tokens[i, 0, :int(token_len[i, 0])].tolist() for i in range(3)]
    assert want != plain                                                                        # this LM moves a winner: the pipeline is seen to use it
    assert torch.equal(total, select_nbest(am, lms, token_len, w)[1])
    assert max(m.last_beam_rounds()) <= logits.shape[1] + 2
    p0, l0, t0, a0, z0 = m.decode_logits_beam_lm(logits, logits_len, lm=lm, lm_weight=0.0)
    p1, l1, s1 = m.decode_logits_beam(logits, logits_len)
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(t0, s1) and torch.equal(a0, s1) and not z0.any()
    try:
        m.lm, m.lm_weight = lm, w
        assert m.beam_search_fused(x, x_len) == want
        assert m.beam_labels(x, x_len) == plain                                                 # beam_labels itself ignores the LM
        m.tokenizer = _Tok()
        assert m.beam_search_fused(x, x_len) == _Tok().decode(want)
    finally:
        m.lm, m.lm_weight, m.tokenizer = None, 0.0, None
