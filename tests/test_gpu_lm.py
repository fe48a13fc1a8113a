"""LSTM language model on the GPU (csrc/lm.hip: effconf_lm_score / effconf_lm_step) against the float64 oracle (tests/lm_ref.py) and the
reference's own runs (tests/golden/lm_*.npz), and n-best rescoring of the CTC beam search (ModelCTC.rescore_nbest) end to end.

Bound.  Per position, |GPU - float64| <= 8 x the float32 noise of that case: the largest |torch float32 nn.LSTM + Linear + log_softmax - float64|
over the case's valid positions, measured at run time on the CPU (lm_cases.float32_noise) - the reference's own arithmetic, never the kernel's.
The factor 8 is the lattice contract's.  A score: the same bound times the sequence's length.  Every case prints its measured
ratio (GPU error / noise); DESIGN.md 6g records them.

decode against token_logprobs.  decode returns raw logits and the scorer keeps its log-softmax inside the head kernel (one float leaves it).
The LSTM kernels are shared, so the (h, c) state after every sequence's last token - ragged lengths: after 0, 1, 2, .. steps - is bit-identical
on both paths (read from the scorer's workspace by a helper of this file); the logits are therefore the same bits, and token_logp is held at every
position to the float64 log_softmax of the walk's own fp32 logits within the fp32 rounding of the head's softmax (``_head_bound``)."""
import functools
import os

import numpy as np
import pytest
import torch

import lm_ref
from lm_cases import GOLDEN, fixture, float32_noise
from efficientconformer_amd import LanguageModel, ModelCTC, _lib, named_config, synth

pytestmark = pytest.mark.gpu

FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def _lm(h, layers, v, seed=5):
    params = dict(arch="RNN", vocab_size=v, dim_model=h, num_layers=layers)
    sd = synth.make_lm_state_dict(params, seed)
    m = LanguageModel(params)
    m.load_state_dict({k: torch.from_numpy(v_) for k, v_ in sd.items()})
    return m.cuda(), params, sd


@functools.lru_cache(maxsize=None)
def _fixture_lm(name):
    g, params, sd = fixture(name)
    m = LanguageModel(params)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda(), g, params, sd


def _sequences(seed, n, u_max, v, kind):
    rng = np.random.default_rng(seed)
    if kind == "full":
        lens = np.full(n, u_max)
    elif kind == "short":                            # 0, 1, 2 and the longest among ragged ones
        lens = rng.integers(0, u_max + 1, n)
        lens[:min(n, 4)] = [0, 1, 2, u_max][:min(n, 4)]
    else:
        lens = rng.integers(1, u_max + 1, n)
        lens[-1] = u_max
    y = np.zeros((n, u_max), dtype=np.int64)
    for i, m in enumerate(lens):
        y[i, :m] = rng.integers(1, v, m)
    return y, lens.astype(np.int64)


# H: 32 (K16 = 2), 48 (K16 = 3, odd), 64, 320; N around the 16-column tile and beyond one workgroup's 64 columns (1 / 2 / 4 column tiles per wave)
CASES = [(32, 2, 40, 1, "full", 40, 1.0), (48, 3, 257, 17, "ragged", 23, 2.0), (64, 1, 1000, 16, "full", 9, 1.0),
         (320, 2, 257, 33, "short", 40, 1.0), (32, 1, 40, 33, "short", 12, 2.0), (320, 3, 1000, 17, "ragged", 17, 2.0),
         (48, 2, 40, 70, "ragged", 5, 1.0)]


@pytest.mark.parametrize("h,layers,v,n,kind,u_max,tmp", CASES)
def test_token_logprobs_against_float64(h, layers, v, n, kind, u_max, tmp):
    m, params, sd = _lm(h, layers, v)
    y, lens = _sequences(100 * h + n, n, u_max, v, kind)
    want, want_score, _ = lm_ref.token_logprobs(sd, y, lens, tmp)
    noise = float32_noise(params, sd, y, lens, tmp, want)
    lp, status = m.token_logprobs(torch.from_numpy(y).cuda(), torch.from_numpy(lens).cuda(), lm_tmp=tmp)
    score = m.score(torch.from_numpy(y), torch.from_numpy(lens), lm_tmp=tmp)
    lp, status, score = lp.cpu().double().numpy(), status.cpu().numpy(), score.cpu().double().numpy()
    valid = np.arange(u_max)[None, :] < lens[:, None]
    err = np.abs(lp - want)
    serr = np.abs(score - want_score) / np.maximum(lens, 1)
    print("lm ratio H %d L %d V %d N %d %s U %d tmp %g: noise %.3g, token error %.3g (%.2f x), score error per token %.3g (%.2f x)"
          % (h, layers, v, n, kind, u_max, tmp, noise, err[valid].max(initial=0.0), err[valid].max(initial=0.0) / noise, serr.max(), serr.max() / noise))
    assert noise > 0
    assert (status == 0).all()
    assert (lp[~valid] == 0).all()
    assert err[valid].max(initial=0.0) <= FACTOR * noise
    assert (np.abs(score - want_score) <= FACTOR * noise * np.maximum(lens, 1)).all()
    assert (score[lens == 0] == 0).all()
    # the score is the fp32 sum of the token log-probabilities in ascending position
    lp32 = lp.astype(np.float32)
    acc = np.zeros(n, dtype=np.float32)
    for k in range(u_max):
        acc = np.where(valid[:, k], acc + lp32[:, k], acc).astype(np.float32)
    assert np.array_equal(acc, score.astype(np.float32))


@pytest.mark.parametrize("name", ["TinyLM", "LM257"])
def test_forward_and_decode_against_the_reference_runs(name):
    m, g, params, sd = _fixture_lm(name)
    y, lens = torch.from_numpy(g["tokens"].astype(np.int64)).cuda(), torch.from_numpy(g["token_len"]).cuda()
    logits = m((y, lens, None)).cpu().double().numpy()
    noise = float(np.abs(g["logits_f32"].astype(np.float64) - g["logits_f64"]).max())
    err = float(np.abs(logits - g["logits_f64"]).max())
    print("lm ratio golden %s forward: noise %.3g, error %.3g (%.2f x)" % (name, noise, err, err / noise))
    assert logits.shape == g["logits_f64"].shape and err <= FACTOR * noise
    hidden = None
    wnoise = float(np.abs(g["walk_logits_f32"].astype(np.float64) - g["walk_logits_f64"]).max())
    for k in range(g["walk_tokens"].shape[0]):
        lg, hidden = m.decode(torch.from_numpy(g["walk_tokens"][k].astype(np.int64))[:, None].cuda(), hidden)
        assert lg.shape == (3, 1, params["vocab_size"])
        werr = float(np.abs(lg[:, 0].cpu().double().numpy() - g["walk_logits_f64"][k]).max())
        assert werr <= FACTOR * wnoise
    snoise = max(float(np.abs(g["walk_%s_f32" % s].astype(np.float64) - g["walk_%s_f64" % s]).max()) for s in "hc")
    serr = max(float(np.abs(hidden[i].cpu().double().numpy() - g["walk_%s_f64" % s]).max()) for i, s in enumerate("hc"))
    print("lm ratio golden %s decode walk: logits noise %.3g, state noise %.3g, state error %.3g (%.2f x)" % (name, wnoise, snoise, serr, serr / snoise))
    assert serr <= FACTOR * snoise


def _native_score(m, y, lens, tmp):
    """effconf_lm_score called directly, on a workspace the test keeps -> (token_logp (N, U), status, h, c): the scorer's outputs and every
    sequence's (h, c) after its own last token, each (L, N, H), read from the workspace as include/effconf.h lays it out.  Step u reads h buffer
    u & 1 and writes the other one for as long as the sequence's column group (16 columns x the 1 / 2 / 4 tiles a wave owns at N <= 16 / <= 32 /
    more) holds an unfinished sequence: the final h of a group whose longest sequence has G tokens is in buffer G & 1."""
    lib = _lib.load()
    n, u = y.shape
    vocab, h, layers = m._cfg
    with torch.cuda.device(0):
        m._ensure()
        tg, tl = torch.from_numpy(y.astype(np.int32)).cuda(), torch.from_numpy(lens.astype(np.int64)).cuda()
        ws = torch.empty(int(lib.effconf_lm_workspace_bytes(m._handle, n, u)), dtype=torch.uint8, device="cuda")
        lp = torch.empty(n, u, dtype=torch.float32, device="cuda")
        sc = torch.empty(n, dtype=torch.float32, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        _lib.check(lib.effconf_lm_score(m._handle, tg.data_ptr(), tl.data_ptr(), n, u, tmp, lp.data_ptr(), sc.data_ptr(), st.data_ptr(), ws.data_ptr(),
                                        ws.numel(), torch.cuda.current_stream().cuda_stream), "lm_score")
        torch.cuda.synchronize()
    npad = (n + 63) // 64 * 64
    off = (-ws.data_ptr()) % 256 + (4 * n + 255) // 256 * 256
    state = ws[off:off + layers * 3 * npad * h * 4].view(torch.float32).view(layers, 3, npad, h)
    group = 16 * (4 if n > 32 else 2 if n > 16 else 1)
    longest = np.array([lens[i // group * group:(i // group + 1) * group].max() for i in range(n)])
    buf, col = torch.from_numpy(longest & 1).cuda(), torch.arange(n, device="cuda")
    k = torch.arange(h, device="cuda")
    perm = (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3)
    return lp, st, state[:, buf, col][:, :, perm].contiguous(), state[:, 2, :n].contiguous()


def _head_bound(z, y):
    """What fp32 rounding allows between the scorer's token_logp and the float64 log_softmax of the SAME fp32 logits z (V,), at column y.
    The head computes lp = z_y - (M + logf(s)) with s = sum_i exp(z_i - M) built from partial (max, sum) pairs: a lane's four rows per tile,
    merged over its tiles, over the four k-slots of a wave (2 levels), over the non-empty waves in order.  With eps = 2^-24 (half an ulp,
    relative), expf and logf within 1 ulp = 2 eps (the HIP math API's stated accuracy):
      * term i reaches s through factors exp(a), a <= 0, whose arguments sum to -(M - z_i) = -d_i exactly; each subtraction is rounded (eps |a|):
        a relative error eps d_i, weighted by the term's share p_i of s: eps sum_i p_i d_i;
      * per merge level one expf (2 eps), one product and one sum (eps each, fused or not): 4 eps; in the lane's tile one expf and three sums: 5 eps;
        a merge with an empty part multiplies by 1 and adds 0, exactly;
      * logf(s): 2 eps |ln s|; M + ln s: eps |lse|; z_y - lse: eps |lp|.
    levels = 2 (tile pairs per wave, rounded up) + 2 + (non-empty waves - 1)."""
    z = np.asarray(z, dtype=np.float64)
    v = z.shape[0]
    pairs = ((v + 15) // 16 + 1) // 2
    levels = 2 * ((pairs + 7) // 8) + 2 + (min(pairs, 8) - 1)
    d = z.max() - z
    s = np.exp(-d).sum()
    lse = z.max() + np.log(s)
    lp = z[y] - lse
    eps = 2.0 ** -24
    return lp, eps * ((np.exp(-d) / s * d).sum() + 4 * levels + 5 + 2 * abs(np.log(s)) + abs(lse) + abs(lp))


@pytest.mark.parametrize("h,layers,v,n,tmp", [(48, 3, 257, 19, 1.0), (32, 2, 40, 70, 2.0)])
def test_decode_walk_reproduces_the_scorer(h, layers, v, n, tmp):
    """A token-by-token decode walk against the scorer on ragged lengths (0, 1, 2, .., u_max).  The LSTM kernels are the same, so every sequence's
    (h, c) after its own last token is bit-identical on both paths - with ragged lengths that is the state after 0, 1, 2, .. steps.  decode returns
    the raw logits acc + b, the scorer takes its log-softmax of (acc + b) / lm_tmp inside the head kernel (lm_tmp 1 and 2: the division is exact), so
    what separates token_logp from the float64 log_softmax of the walk's own logits is the fp32 rounding of that softmax alone: ``_head_bound``,
    at every position."""
    m, params, sd = _lm(h, layers, v)
    u = 11
    y, lens = _sequences(77 + n, n, u, v, "short")
    lp, status, h_s, c_s = _native_score(m, y, lens, tmp)
    assert (status == 0).all()
    x = torch.nn.functional.pad(torch.from_numpy(y).cuda(), pad=(1, 0, 0, 0), value=0)
    hidden, walk = None, []
    h_w, c_w = torch.zeros_like(h_s), torch.zeros_like(c_s)
    for k in range(u):
        lg, hidden = m.decode(x[:, k:k + 1], hidden)
        walk.append(lg[:, 0])
        done = torch.from_numpy(lens == k + 1).cuda()
        h_w[:, done], c_w[:, done] = hidden[0][:, done], hidden[1][:, done]
    walk = torch.stack(walk, dim=1)
    assert set(lens.tolist()) >= {0, 1, 2, u} and len(set(lens.tolist())) >= 6
    assert torch.equal(h_w, h_s) and torch.equal(c_w, c_s)
    assert float(h_w.abs().max()) > 0 and not h_w[:, torch.from_numpy(lens == 0).cuda()].any()
    # forward is the same walk
    assert torch.equal(m((torch.from_numpy(y[:, :u - 1]).cuda(), None, None)), walk)
    z, got = walk.cpu().double().numpy() / tmp, lp.cpu().double().numpy()
    worst = 0.0
    for i in range(n):
        for k in range(int(lens[i])):
            want, bound = _head_bound(z[i, k], int(y[i, k]))
            worst = max(worst, abs(got[i, k] - want) / bound)
            assert abs(got[i, k] - want) <= bound, (i, k, got[i, k], want, bound)
    print("lm walk H %d V %d tmp %g: largest |token_logp - float64 log_softmax(walk logits)| / bound %.3f" % (h, v, tmp, worst))


def test_a_sequence_does_not_depend_on_its_batch(monkeypatch):
    m, params, sd = _lm(48, 2, 257)
    v, u = 257, 9
    rng = np.random.default_rng(9)
    s = rng.integers(1, v, u)

    def run(y, lens, row):
        lp, st = m.token_logprobs(torch.from_numpy(y).cuda(), torch.from_numpy(lens).cuda(), lm_tmp=2.0)
        sc = m.score(torch.from_numpy(y).cuda(), torch.from_numpy(lens).cuda(), lm_tmp=2.0)
        assert int(st[row]) == 0
        return lp[row, :u].cpu().numpy().view(np.int32), sc[row].cpu().numpy().view(np.int32)
    alone = run(s[None, :].copy(), np.array([u]), 0)
    assert np.isfinite(alone[0].view(np.float32)).all()
    y, lens = _sequences(10, 33, 14, v, "short")
    y[5, :u], lens[5] = s, u
    y[5, u:] = 0
    batch = run(y, lens, 5)
    rev = run(y[::-1].copy(), lens[::-1].copy(), 33 - 1 - 5)
    pad = run(np.concatenate([y, np.zeros((33, 7), dtype=np.int64)], axis=1), lens, 5)
    junk = y.copy()
    for i in range(33):                              # NaN bit patterns, negative and too large ids behind every length
        junk[i, lens[i]:] = np.resize(np.array([0x7FC00000, -5, v + 1000, -2 ** 31, 2 ** 31 - 1]), 14 - lens[i])
    garbage = run(junk, lens, 5)
    monkeypatch.setenv("EFFCONF_POISON_WORKSPACE", "255")
    poisoned = run(y, lens, 5)
    monkeypatch.delenv("EFFCONF_POISON_WORKSPACE")
    for name, got in (("batch of 33", batch), ("reversed", rev), ("u_max + 7", pad), ("garbage", garbage), ("0xFF workspace", poisoned)):
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1]), name


def test_status_2_leaves_the_neighbours_alone():
    m, params, sd = _lm(48, 2, 257)
    v, n, u = 257, 20, 8
    y, lens = _sequences(31, n, u, v, "ragged")
    for row, m_ in ((3, 5), (7, 6)):                 # long enough for the slots that are spoilt below
        lens[row] = m_
        y[row, :m_] = 1 + (np.arange(m_) * 37 + row) % (v - 1)
        y[row, m_:] = 0
    clean_lp, clean_st = m.token_logprobs(torch.from_numpy(y).cuda(), torch.from_numpy(lens).cuda())
    clean_sc = m.score(torch.from_numpy(y).cuda(), torch.from_numpy(lens).cuda())
    bad, bad_len = y.copy(), lens.copy()
    bad[3, 1] = v                                    # one past the table
    bad[7, 4] = 0                                    # the blank inside a sequence
    bad[13, 0] = -1
    bad_len[9] = u + 1
    bad_len[11] = -1
    bad[15, lens[15]:] = v + 5                       # behind the length: not an error
    lp, st = m.token_logprobs(torch.from_numpy(bad).cuda(), torch.from_numpy(bad_len).cuda())
    sc = m.score(torch.from_numpy(bad).cuda(), torch.from_numpy(bad_len).cuda())
    rows = [3, 7, 9, 11, 13]
    want = np.zeros(n, dtype=np.int32)
    want[rows] = 2
    assert (clean_st == 0).all() and np.array_equal(st.cpu().numpy(), want)
    assert torch.isneginf(lp[rows]).all() and torch.isneginf(sc[rows]).all()
    keep = [i for i in range(n) if i not in rows]
    assert torch.equal(lp[keep], clean_lp[keep]) and torch.equal(sc[keep], clean_sc[keep])
    assert np.array_equal(lm_ref.token_logprobs(sd, bad, bad_len)[2], want)


@functools.lru_cache(maxsize=None)
def _tiny_ctc():
    cfg = named_config("Tiny")
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def test_rescoring_end_to_end_on_the_tiny_ctc_logits():
    ctc = _tiny_ctc()
    lm, g, params, sd = _fixture_lm("TinyLM")
    w = float(g["rescore_lm_weight"])
    moved = kept = 0
    for tm in (100, 47):
        gold = np.load(os.path.join(GOLDEN, "tiny_T%d.npz" % tm))
        logits, out_len = torch.from_numpy(gold["logits"]).cuda(), torch.from_numpy(gold["out_len"]).cuda()
        tokens, token_len, am = ctc.decode_logits_beam(logits, out_len, 16)
        best, total, lms = ctc.rescore_nbest(tokens, token_len, am, lm=lm, lm_weight=w)
        b, beam, t = tokens.shape
        # the LM scores are those of the hypotheses, held to the oracle
        flat, flat_len = tokens.reshape(b * beam, t).cpu().numpy().astype(np.int64), token_len.reshape(-1).cpu().numpy().astype(np.int64)
        want_lp, want, _ = lm_ref.token_logprobs(sd, flat, flat_len)
        noise = float32_noise(params, sd, flat, flat_len, 1.0, want_lp)
        assert torch.equal(lms.reshape(-1), lm.score(tokens.reshape(b * beam, t), token_len.reshape(-1)))
        assert (np.abs(lms.reshape(-1).cpu().double().numpy() - want) <= FACTOR * noise * np.maximum(flat_len, 1)).all()
        # selection is exact: a host recomputation from the returned device scores
        am_h, lms_h = am.cpu(), lms.cpu()
        total_h = am_h + w * lms_h
        assert torch.equal(total.cpu(), total_h)
        for i in range(b):
            key = [(-float("inf") if am_h[i, k] == -float("inf") else float(total_h[i, k])) for k in range(beam)]
            assert int(best[i]) == key.index(max(key))
            moved += int(best[i]) != 0
            kept += int(best[i]) == 0
    # what keeps this test honest: the fixture's fc bias makes the LM overturn some acoustic winners and confirm others
    assert moved >= 1 and kept >= 1, (moved, kept)


def test_rescored_labels_and_the_cases_that_change_nothing():
    ctc = _tiny_ctc()
    lm, g, params, sd = _fixture_lm("TinyLM")
    w = float(g["rescore_lm_weight"])
    mel, ln = synth.make_mel(3, 80, 100, [100, 77, 52], seed=4421)
    mel, ln = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    plain = ctc.beam_labels(mel, ln, 16, from_mel=True)
    assert ctc.lm is None and ctc.lm_weight == 0
    assert ctc.beam_labels_rescored(mel, ln, 16, from_mel=True) == plain                        # no LM
    assert ctc.beam_labels_rescored(mel, ln, 16, from_mel=True, lm=lm, lm_weight=0.0) == plain  # weight 0
    assert ctc.beam_labels_rescored(mel, ln, 16, from_mel=True, lm=None, lm_weight=w) == plain  # weight without an LM
    enc, enc_len, _ = ctc.encoder.forward_mel(mel, ln)
    logits, _, _ = ctc._head(enc, enc_len, want_logits=True)
    tokens, token_len, am = ctc.decode_logits_beam(logits, enc_len, 16)
    best, total, lms = ctc.rescore_nbest(tokens, token_len, am, lm=lm, lm_weight=w)
    want = [tokens[i, int(best[i]), :int(token_len[i, int(best[i])])].tolist() for i in range(3)]
    assert ctc.beam_labels_rescored(mel, ln, 16, from_mel=True, lm=lm, lm_weight=w) == want
    b0, t0, l0 = ctc.rescore_nbest(tokens, token_len, am, lm=lm, lm_weight=0.0)
    assert b0.tolist() == [0, 0, 0] and torch.equal(t0, am) and not l0.any()
    try:
        ctc.lm, ctc.lm_weight = lm, w
        assert ctc.beam_labels_rescored(mel, ln, 16, from_mel=True) == want
        assert ctc.beam_labels(mel, ln, 16, from_mel=True) == plain                             # beam_labels itself ignores the LM
    finally:
        ctc.lm, ctc.lm_weight = None, 0.0
