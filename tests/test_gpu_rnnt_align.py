"""RNN-T lattice scoring and forced alignment on the GPU (effconf_rnnt_lattice / effconf_rnnt_align, csrc/rnnt_lattice.hip and
csrc/rnnt_align.hip) against the float64 oracle (tests/rnnt_align_ref.py): the lattice planes of TinyTransducer and
EfficientConformerTransducerMedium, the dynamic programs on synthetic planes at the shapes where the kernel's thread count and back-pointer
words change, the status codes, independence of the batch / padding / workspace contents, the beam search's scores and the model pipeline.

Bounds.  Lattice planes, per cell against float64: 8 x the float32 noise of the same formula evaluated on the CPU (torch float32 against
float64, maximum over every cell of the three lattice cases at both temperatures; on Medium at tmp = 1, where |lp| reaches 8.9: 1.78e-6
on one host, 1.31e-6 on another - the BLAS' summation order), i.e. 1.42e-5 / 1.05e-5 - computed at run time from the reference
computation (rnnt_align_cases.float32_noise), never from the kernel.  The kernel's measured error against float64: 7.3e-7 / 5.6e-7 on
"tiny" at tmp 1 / 2, 2.15e-6 / 2.06e-6 on "medium", 7.6e-7 / 6.7e-7 on "tiny17" (printed by the test).
Scores of the dynamic programs against float64: 1e-5 (1 + |v|), the existing bound of these recursions (tests/test_gpu_ctc_align.py).  Path
identity with the oracle is required wherever the oracle's smallest decision margin along its path is at least 1e-3; at most 1 case in 8 of
a test may be excused by a smaller margin (tests/test_rnnt_align_host.py keeps the oracle alone within that share for these seeds)."""
import functools
import os

import numpy as np
import pytest
import torch

import rnnt_align_cases as cases
from rnnt_align_ref import check_path, forward, path_logp, status_of, viterbi
from efficientconformer_amd import Transducer, synth

pytestmark = pytest.mark.gpu

REL = 1e-5
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def _model(name):
    tsd, cfg = cases.weights(name)
    m = Transducer.from_config(cfg)
    g = np.load(os.path.join(cases.GOLDEN, "rnnt_%s.npz" % name))
    sd = synth.make_state_dict(m.encoder.plan, int(g["weight_seed"]), None, prefix="encoder.")
    sd.update(tsd)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


def _pad_targets(targets, upad=None, fill=0):
    u = max([len(y) for y in targets] + [0]) if upad is None else upad
    out = np.full((len(targets), u), fill, dtype=np.int32)
    for i, y in enumerate(targets):
        out[i, :len(y)] = y
    return out, np.array([len(y) for y in targets], dtype=np.int64)


def _lattice(name, f, f_len, targets, tmp=1.0, upad=None, ufill=0, y_len=None):
    m = _model(name)
    tg, tl = _pad_targets(targets, upad, ufill)
    if y_len is not None:
        tl = np.asarray(y_len, dtype=np.int64)
    m.tmp = tmp
    try:
        lpb, lpl, st = m.lattice(torch.as_tensor(f).cuda(), None if f_len is None else torch.as_tensor(np.asarray(f_len, dtype=np.int64)).cuda(),
                                 torch.as_tensor(tg).cuda(), torch.as_tensor(tl).cuda())
    finally:
        m.tmp = 1.0
    return lpb.cpu().numpy(), lpl.cpu().numpy(), st.cpu().numpy()


def _dp(lpb, lpl, f_len, y_len, scores_only=False, status=None):
    m = _model("TinyTransducer")
    out = m.align_lattice(torch.as_tensor(lpb).cuda(), torch.as_tensor(lpl).cuda(), torch.as_tensor(np.asarray(f_len, dtype=np.int64)).cuda(),
                          torch.as_tensor(np.asarray(y_len, dtype=np.int64)).cuda(), scores_only=scores_only,
                          status=None if status is None else torch.as_tensor(status))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _close(a, b):
    if np.isneginf(b):
        return bool(np.isneginf(a))
    return bool(np.isfinite(a)) and abs(float(a) - b) <= REL * (1.0 + abs(b))


# ---------------------------------------------------------------------------------------------------------------- 1. lattice planes
@pytest.mark.parametrize("tmp", cases.TEMPERATURES)
@pytest.mark.parametrize("case", ["tiny", "medium", "tiny17"])
def test_lattice_planes_match_the_float64_oracle(case, tmp):
    name, f, f_len, targets = cases.lattice_case(case)
    noise = cases.float32_noise()
    bound = 8 * noise
    lpb, lpl, st = _lattice(name, f, f_len, targets, tmp)
    umax = max(len(y) for y in targets)
    assert lpb.shape == lpl.shape == (f.shape[0], f.shape[1], umax + 1) and (st == 0).all()
    worst = 0.0
    for i, (ob, ol) in enumerate(cases.oracle_planes(case, tmp)):
        n, u = int(f_len[i]), len(targets[i])
        assert not lpb[i, n:].any() and not lpb[i, :, u + 1:].any() and not lpl[i, n:].any() and not lpl[i, :, u + 1:].any(), i
        assert np.isneginf(lpl[i, :n, u]).all(), i
        assert np.isfinite(lpb[i, :n, :u + 1]).all() and np.isfinite(lpl[i, :n, :u]).all(), i
        worst = max(worst, float(np.abs(lpb[i, :n, :u + 1] - ob).max()), float(np.abs(lpl[i, :n, :u] - ol[:, :u]).max()) if u else 0.0)
    print("%s tmp %g: kernel vs float64 %.3g, float32 noise %.3g, bound %.3g" % (case, tmp, worst, noise, bound))
    assert worst <= bound, (worst, bound)


# ---------------------------------------------------------------------------------------------------------------- 2. dynamic programs
def _check_dp(planes, out, f_len=None, y_len=None):
    """Every invariant, the likelihood, optimality and - where the oracle's margin allows - path identity -> (cases, excused)."""
    umax = out["token_frame"].shape[1]
    excused = 0
    for i, (b, l) in enumerate(planes):
        n = b.shape[0] if f_len is None else int(f_len[i])
        u = b.shape[1] - 1 if y_len is None else int(y_len[i])
        b, l = b[:n, :u + 1], l[:n, :u + 1]
        tag = (i, n, u)
        assert out["status"][i] == 0, tag
        fr = out["token_frame"][i]
        assert (fr[u:] == -1).all() and (out["token_logp"][i, u:] == 0).all(), tag
        assert check_path(fr[:u], n, u) is None, (tag, check_path(fr[:u], n, u))
        assert all(0 <= fr[k] < n and (k == 0 or fr[k - 1] <= fr[k]) for k in range(u)), tag
        assert out["token_logp"][i, :u].tobytes() == np.array([l[fr[k], k] for k in range(u)], dtype=np.float32).tobytes(), tag
        mine = path_logp(b, l, fr[:u], n)
        assert _close(out["score"][i], mine), (tag, out["score"][i], mine)
        ll = forward(b, l)
        assert _close(out["log_likelihood"][i], ll), (tag, out["log_likelihood"][i], ll)
        ref = viterbi(b, l)
        assert abs(mine - ref["score"]) <= REL * (1 + abs(ref["score"])), (tag, mine, ref["score"])      # optimal whatever the ties do
        assert mine <= ll + 1e-9 * (1 + abs(ll)), tag
        assert out["score"][i] <= out["log_likelihood"][i] + REL * (1 + abs(ll)), tag
        if ref["margin"] >= MARGIN:
            assert fr[:u].tolist() == ref["token_frame"].tolist(), (tag, ref["margin"])
        else:
            excused += 1
    return len(planes), excused


@pytest.mark.parametrize("kind,n", [("u", u) for u in cases.DP_U] + [("t", t) for t in cases.DP_T] + [("ragged", None)])
def test_dynamic_programs_match_the_float64_oracle(kind, n):
    planes = cases.dp_case(kind, n)
    lpb, lpl, f_len, y_len = cases.pad_planes(planes)
    out = _dp(lpb, lpl, f_len, y_len)
    count, excused = _check_dp(planes, out)
    assert 8 * excused <= count


# ---------------------------------------------------------------------------------------------------------------- 3. status codes
def test_status_codes_leave_the_rest_of_the_batch_alone():
    name, f, f_len, targets = cases.lattice_case("tiny")
    v = cases.weights(name)[1]["decoder_params"]["vocab_size"]
    good = [targets[0], targets[2]]
    alone = []
    for k, src in ((0, 0), (1, 2)):
        b, l, s = _lattice(name, f[src:src + 1], f_len[src:src + 1], [good[k]])
        alone.append((b, l, _dp(b, l, f_len[src:src + 1], [len(good[k])], status=s)))
    bad0 = list(targets[2]); bad0[3] = 0                          # the blank as a target
    badv = list(targets[2]); badv[8] = v                          # the first id outside the vocabulary
    rows = [0, 2, 2, 1, 1, 2, 3]
    lens = [int(f_len[0]), int(f_len[2]), int(f_len[2]), 0, 0, int(f_len[2]), int(f_len[3])]
    ys = [good[0], bad0, badv, [4, 5], [], good[1], [7, 7, 7]]
    y_len = [len(y) for y in ys]
    y_len[6] = 10                                                 # more tokens than the padded width: status 2
    want = [0, 2, 2, 1, 0, 0, 2]
    lpb, lpl, st = _lattice(name, f[rows], lens, ys, y_len=y_len)
    assert st.tolist() == want
    assert [status_of(lens[i], ys[i], v) for i in range(6)] == want[:6]
    out = _dp(lpb, lpl, lens, y_len, status=st)
    assert out["status"].tolist() == want
    for i in (1, 2, 6):                                           # status 2: zero rows, -inf scores, no alignment
        assert not lpb[i].any() and not lpl[i].any()
    for i in (1, 2, 3, 6):
        assert np.isneginf(out["log_likelihood"][i]) and np.isneginf(out["score"][i])
        assert (out["token_frame"][i] == -1).all() and (out["token_logp"][i] == 0).all()
    assert out["log_likelihood"][4] == 0 and out["score"][4] == 0 and (out["token_frame"][4] == -1).all()
    for i, k in ((0, 0), (5, 1)):
        b, l, o = alone[k]
        n, u = b.shape[1], len(good[k])
        assert lpb[i, :n, :u + 1].tobytes() == b[0].tobytes() and lpl[i, :n, :u + 1].tobytes() == l[0].tobytes(), i
        for key in ("log_likelihood", "score", "status"):
            assert out[key][i].tobytes() == o[key][0].tobytes(), (i, key)
        for key in ("token_frame", "token_logp"):
            assert out[key][i, :u].tobytes() == o[key][0].tobytes(), (i, key)
    # the align entry point on its own (zeros as the incoming status) finds what it can see: the lengths
    own = _dp(lpb, lpl, lens, y_len)
    assert own["status"].tolist() == [0, 0, 0, 1, 0, 0, 2]


# ---------------------------------------------------------------------------------------------------------------- 4. independence
def test_results_do_not_depend_on_batch_order_padding_or_workspace(monkeypatch):
    name, f, f_len, _ = cases.lattice_case("tiny")
    v = cases.weights(name)[1]["decoder_params"]["vocab_size"]
    rng = np.random.default_rng(2424)
    src = [i % f.shape[0] for i in range(24)]
    lens = np.array([max(1, int(f_len[s]) - (i // 4) % 3) for i, s in enumerate(src)], dtype=np.int64)
    targets = [rng.integers(1, v, int(rng.integers(0, 14))).tolist() for _ in src]
    fb = np.ascontiguousarray(f[src])

    def run(rows, **kw):
        ys = [targets[i] for i in rows]
        lpb, lpl, st = _lattice(name, fb[rows], lens[rows], ys, **kw)
        out = _dp(lpb, lpl, lens[rows], [len(y) for y in ys], status=st)
        only = _dp(lpb, lpl, lens[rows], [len(y) for y in ys], scores_only=True, status=st)
        assert set(only) == {"log_likelihood", "status"}
        assert only["log_likelihood"].tobytes() == out["log_likelihood"].tobytes() and np.array_equal(only["status"], out["status"])
        return lpb, lpl, out

    def same(got, k, want, j, what):
        n, u = int(lens[rows_of[what][k]]), len(targets[rows_of[what][k]])
        assert got[0][k, :n, :u + 1].tobytes() == want[0][j, :n, :u + 1].tobytes(), (what, k, "lp_blank")
        assert got[1][k, :n, :u + 1].tobytes() == want[1][j, :n, :u + 1].tobytes(), (what, k, "lp_label")
        assert not got[0][k, n:].any() and not got[0][k, :, u + 1:].any() and not got[1][k, n:].any() and not got[1][k, :, u + 1:].any()
        for key in ("log_likelihood", "score", "status"):
            assert got[2][key][k].tobytes() == want[2][key][j].tobytes(), (what, k, key)
        for key in ("token_frame", "token_logp"):
            assert got[2][key][k, :u].tobytes() == want[2][key][j, :u].tobytes(), (what, k, key)
            assert (got[2][key][k, u:] == (0 if key == "token_logp" else -1)).all(), (what, k, key)

    every = list(range(24))
    rows_of = {"alone": every, "reversed": every[::-1], "padded": every, "again": every, "poisoned": every}
    batch = run(every)
    count, excused = _check_dp([(batch[0][i, :lens[i], :len(targets[i]) + 1], batch[1][i, :lens[i], :len(targets[i]) + 1]) for i in every], batch[2])
    assert 8 * excused <= count
    for i in every:
        rows_of["alone"] = [i]
        same(run([i]), 0, batch, i, "alone")
    rev = run(every[::-1])
    for k in range(24):
        same(rev, k, batch, 23 - k, "reversed")
    padded = run(every, upad=40, ufill=-123456)                   # garbage ids at or beyond y_len, a wider lattice
    again = run(every)
    monkeypatch.setenv("EFFCONF_POISON_WORKSPACE", "255")
    poisoned = run(every, upad=40, ufill=2 ** 31 - 1)
    for k in every:
        same(padded, k, batch, k, "padded")
        same(again, k, batch, k, "again")
        same(poisoned, k, batch, k, "poisoned")


# ---------------------------------------------------------------------------------------------------------------- 5. beam search
def test_a_beam_hypothesis_is_one_lattice_path():
    """At tmp = 1 the beam search's score is the log-probability of ONE path of its tokens' lattice: never above the best path's, which is
    never above the sum over all paths."""
    name = "TinyTransducer"
    m = _model(name)
    g = np.load(os.path.join(cases.GOLDEN, "rnnt_%s.npz" % name))
    bg = np.load(os.path.join(cases.GOLDEN, "rnnt_beam_%s.npz" % name))
    f, f_len = torch.from_numpy(g["f"]).cuda(), torch.from_numpy(g["f_len"]).cuda()
    offs = bg["offsets_b16"]
    want = [bg["tokens_b16"][offs[i]:offs[i + 1]].tolist() for i in range(f.shape[0])]
    tokens, token_len, score, status = m.decode_encoded_beam(f, f_len, 16)
    assert [tokens[i, :int(token_len[i])].tolist() for i in range(f.shape[0])] == want and (status == 0).all()
    lpb, lpl, st = m.lattice(f, f_len, want)
    out = m.align_lattice(lpb, lpl, f_len, [len(y) for y in want], status=st)
    beam, best, ll = score.cpu().numpy(), out["score"].cpu().numpy(), out["log_likelihood"].cpu().numpy()
    assert (out["status"].cpu().numpy() == 0).all() and sum(len(y) for y in want) > 0
    for i in range(f.shape[0]):
        tol = REL * (1 + abs(float(best[i])))
        assert beam[i] <= best[i] + tol and best[i] <= ll[i] + tol, (i, beam[i], best[i], ll[i])
        ob, ol = cases.lattice_planes(cases.weights(name)[0], g["f"][i], int(g["f_len"][i]), want[i])
        assert _close(ll[i], forward(ob, ol)), (i, ll[i])


# ---------------------------------------------------------------------------------------------------------------- 6. pipeline
class _Tok:
    def encode(self, s):
        return [int(c) for c in s.split()]


def test_pipeline_from_mel():
    m = _model("TinyTransducer")
    fs = m.encoder.frame_seconds
    mel, ln = synth.make_mel(3, m.encoder.plan.n_mels, 100, [100, 61, 20], seed=17)
    mel, ln = torch.from_numpy(mel).cuda(), torch.from_numpy(ln).cuda()
    f, f_len, _ = m.encoder.forward_mel(mel, ln)
    nfr = f_len.cpu().numpy()
    rng = np.random.default_rng(11)
    y = [rng.integers(1, 40, int(k)).tolist() for k in (6, 0, 4)]
    lpb, lpl, st = m.lattice(f, f_len, y)
    want = {k: t.cpu().numpy() for k, t in m.align_lattice(lpb, lpl, f_len, [len(r) for r in y], status=st).items()}
    _check_dp([(lpb[i, :nfr[i], :len(y[i]) + 1].cpu().numpy(), lpl[i, :nfr[i], :len(y[i]) + 1].cpu().numpy()) for i in range(3)], want)
    recs = m.align(mel, ln, y, from_mel=True)
    scores = m.score_labels(mel, ln, y, from_mel=True)
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.cpu().numpy().tobytes() == want["log_likelihood"].tobytes()
    for i, r in enumerate(recs):
        u = len(y[i])
        assert r.tokens == y[i] and r.status == 0 and r.frame == want["token_frame"][i, :u].tolist()
        assert r.time == [k * fs for k in r.frame] and all(0 <= k < nfr[i] for k in r.frame)
        assert np.float32(r.score).tobytes() == want["score"][i].tobytes()
        assert np.float32(r.log_likelihood).tobytes() == want["log_likelihood"][i].tobytes()
        assert np.asarray(r.token_logp, dtype=np.float32).tobytes() == want["token_logp"][i, :u].tobytes()
    # a padded tensor with lengths; strings through a tokenizer; strings without one
    tg, tl = _pad_targets(y, upad=9, fill=0)
    assert m.align(mel, ln, torch.as_tensor(tg), torch.as_tensor(tl), from_mel=True) == recs
    with pytest.raises(Exception) as e:
        m.align(mel, ln, [" ".join(str(c) for c in r) for r in y], from_mel=True)
    assert "tokenizer" in str(e.value)
    m.tokenizer = _Tok()
    try:
        assert m.align(mel, ln, [" ".join(str(c) for c in r) for r in y], from_mel=True) == recs
    finally:
        m.tokenizer = None
