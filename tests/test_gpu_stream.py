"""-m gpu: chunked streaming - the two kernels alone (stream.hip) through effconf_stream_attention and effconf_stream_dwconv, then sessions end to end.

Attention: causal instances of tests/attention_cases.py, every utterance a stream with its own length, fed chunk by chunk - the chunk's queries against the
stream's K / V ring and the chunk's own keys - and the stitched rows compared with the WHOLE-utterance float64 reference (A.reference on the ragged case: each
utterance at its own length).  Bounds: those of tests/test_gpu_attention_edges.py, unchanged - every ratio of A.ratios <= 1 (stage_ratios against the float32
run with P rounded, share factor 2, and element-wise 2^-7 sum_j p_ij |v_j| + 2e-5).  512 bytes of NaN patterns lie behind every operand of every round and in
every ring slot that no chunk has written; the outputs are pre-filled with a sentinel.  Between them the chunk sizes 1, 3, 4, 20, 33, 64, 65 (grouped rows)
reach an empty cache (every first round), a cache shorter than the band (sizes 1, 3, 4 under band 6), a cache of exactly the band (size 3 after two rounds,
size 64 under band 64 after one), a ring that has wrapped more than twice (band 6: capacity 6 against 140 grouped rows; band 64: capacity 64 against 200), a
stream with no rows beside a busy one (the three streams end at different rounds), a final chunk with group-padding rows (lengths that are no multiple of
G = 3) and chunks of more than one 16-query tile (20, 33, 64, 65).

Depthwise: (k, C) = (15, 120), (31, 176), (7, 10), strides 1 and 2, 150 and 91 frames as two streams in chunks of 2, 14, 16 and 64 rows (2 and 14 are shorter
than k - 1 at k = 15 / 31: the state keeps the tail of the old one), against the float64 depthwise stage with F.pad(h, (k - 1, 0)) over the whole sequence
(oracle/ref_bf16.py depthwise).  Bounds: those of the ``dw`` stage of tests/bf16_parity.py, unchanged - stage_ratios(.., k, bf16, share_factor = 0) <= 1 and
element-wise 2^-8 |ref| + 2e-5.  The state buffer is poisoned before the first chunk: the first chunk must see zeros.

profiles/stream_edges.txt holds the lines of the first passing run.

Sessions (ConformerEncoder.open_stream / ModelCTC.open_stream): the stream_tiny_causal* goldens' three utterances as three streams that end at different pushes,
in 24-frame, 48-frame, irregular ([7, 50, 1, 0, 23, rest]) and all-at-once pushes - out_len equal to the golden's and every valid row within 0.09 max / 0.012
mean of its ``out``, the project's bounds of the whole-utterance causal forward (tests/test_gpu_round3.py; the distance to the encoder's own forward_mel is
printed, not bounded); EfficientConformerCTC-Small (601 / 433 frames) in 24- and 96-frame pushes against the golden's rows [::4] and its argmax wherever its
margin exceeds 0.15, and with left_context = 64 against the float32 oracle; bit-for-bit invariances (a stream alone or among three, the same pushes after
reset, a second session on a recycled state buffer); push_audio (the whole-signal front end's mel frames bit for bit, the output against the oracle);
ModelCTC.open_stream's tokens against the whole-utterance greedy labels.  The whole file also passes with EFFCONF_POISON_WORKSPACE set."""
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import attention_cases as A
from attention_cases import F32, F64, UNL
from efficientconformer_amd import ModelCTC, _lib, named_config, synth
from oracle import ref_bf16 as Q
from oracle import ref_encoder as R

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
NAN_TAIL = 256           # bf16 elements = 512 bytes

#            name     instance  frames  lens            left band (grouped rows)
INSTANCES = {"d90-band6": (A.I90, 419, (419, 250, 2), 6),
             "d64-unlimited": (A.I64, 150, (150, 97, 1), UNL),
             "d32-band64": (A.I32, 200, (200, 131, 5), 64),
             "d135-band6": (A.I135, 290, (290, 194, 4), 6),
             "d42-band6": (A.I42, 386, (386, 230, 1), 6)}
CHUNKS = (1, 3, 4, 20, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def _attention_case(name):
    """The ragged causal case of an instance, its operands and its whole-utterance references: computed once, shared by the chunk sizes, never modified."""
    inst, frames, lens, band = INSTANCES[name]
    case = A.Case("stream-" + name, inst, frames, lens, (band, 0), True, True, (1,), "")
    torch.set_num_threads(16)
    ops = A.operands(case, seed=7300 + sorted(INSTANCES).index(name))
    with torch.no_grad():
        o64, env = A.reference(case, ops, F64)
        o32, _ = A.reference(case, ops, F32, round_p=True)
    return case, ops, o64, o32, env


def _with_tail(z):
    return torch.cat([z.reshape(-1), torch.full((NAN_TAIL,), float("nan"), dtype=torch.bfloat16, device="cuda")])


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_stream_attention_chunk_by_chunk_equals_the_whole_utterance_reference(name, chunk):
    lib = _lib.load()
    case, ops, o64, o32, env = _attention_case(name)
    D, H, G, d, dpad, tp, tg = A.dims(case)
    band = case.band[0]
    cap = tg if band >= UNL else band
    B = len(case.lens)
    lay = A.layout(case)
    live = A.live_rows(case)
    qu, k, v = (ops[n].to(torch.bfloat16).cuda() for n in ("qu", "k", "v"))
    e = _with_tail(ops["e"].to(torch.bfloat16).cuda())       # the causal table of the longest utterance: distance delta = grouped row tg - 1 - delta for every stream
    dvu = torch.zeros(H, dpad, dtype=torch.float32)
    for h in range(H):
        dvu[h, :d] = ops["dv"][(h * d + torch.arange(d)) % D].float()            # pack.hip dvu_table
    dvu = dvu.cuda().contiguous()
    kc, vc = (torch.full((B * cap * G * D + NAN_TAIL,), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(2))
    got = torch.full((o64.shape[0], D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    pos, cached = [0] * B, [0] * B
    seen = set()
    rounds = 0
    while any(pos[b] * G < lay[b][1] for b in range(B)):
        idx, row_off, rows, ngs = [], [], [], []
        for b, (q0, r, _, t) in enumerate(lay):
            ng = max(0, min(chunk, r // G - pos[b]))
            n = max(0, min(ng * G, case.lens[b] - pos[b] * G))
            row_off.append(len(idx)); rows.append(n); ngs.append(ng)
            idx += list(range(q0 + pos[b] * G, q0 + (pos[b] + ng) * G))
            if ng:
                seen.add("empty cache" if not cached[b] else "cache shorter than the band" if cached[b] < band < UNL else "cache exactly the band" if cached[b] == band else "cache")
                if pos[b] + ng > 3 * cap:
                    seen.add("ring wrapped more than twice")
                if n < ng * G:
                    seen.add("final chunk with group padding")
        if any(ngs) and not all(ngs):
            seen.add("idle stream")
        ix = torch.tensor(idx, dtype=torch.int64, device="cuda")
        quc, kcc, vcc = (_with_tail(z[ix]) for z in (qu, k, v))
        out = torch.full((len(idx), D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        desc = [_i32(z) for z in (row_off, rows, cached, pos)]          # held until the round has run
        _lib.check(lib.effconf_stream_attention(quc.data_ptr(), kcc.data_ptr(), vcc.data_ptr(), e.data_ptr(), tg, dvu.data_ptr(), dpad, kc.data_ptr(), vc.data_ptr(), cap,
                                                desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(), B, max(rows), H, G, D,
                                                band, out.data_ptr(), D, 1, torch.cuda.current_stream().cuda_stream), "stream_attention", lib)
        torch.cuda.synchronize()
        got[ix] = out
        for b in range(B):
            pos[b] += ngs[b]
            cached[b] = min(cached[b] + ngs[b], cap)
        rounds += 1
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), (name, chunk, "NaN / inf in the output: an unused ring slot or a load behind a buffer's end reached the result")
    assert not bool((got == SENTINEL).any()), (name, chunk, "output rows left unwritten")
    assert float(got[~live].abs().sum()) == 0.0, (name, chunk, "group-padding rows are not zero")
    r = A.ratios(case, got[live], o64[live], o32[live], env[live])
    print("stream_edges | attention %-14s | chunk %2d | rounds %3d | rows %4d | %s | %s" % (name, chunk, rounds, int(live.sum()), "  ".join("%s %.3g" % kv for kv in sorted(r.items())),
                                                                                          ", ".join(sorted(seen))))
    fails = []
    for stat, val in r.items():
        if not val <= 1.0:
            err = (got - o64).abs() / (2.0 ** -7 * env + 2e-5)
            i = int(err.max(-1).values.argmax())
            fails.append("%s: %.3g x its bound (worst row %d of %d, column %d)" % (stat, val, i, got.shape[0], int(err[i].argmax())))
    assert not fails, (name, chunk, fails)


# ------------------------------------------------------------------ depthwise convolution with a carried state
BP = namedtuple("BP", "index kernel_size conv_stride")
DW_LENS = (150, 91)


@functools.lru_cache(maxsize=None)
def _dw_case(ksize, C, stride):
    """Seeded weights (a state dict of the convolution module's depthwise layer and BatchNorm), GLU rows holding bf16 numbers, and the whole-sequence references."""
    gen = torch.Generator().manual_seed(8800 + 100 * ksize + 10 * stride + C)
    p = "blocks.0.convolution_module.layers"
    sd = {p + ".4.weight": torch.randn(C, 1, ksize, generator=gen) * ksize ** -0.5, p + ".4.bias": torch.randn(C, generator=gen) * 0.1,
          p + ".5.weight": 1.0 + 0.1 * torch.randn(C, generator=gen), p + ".5.bias": 0.1 * torch.randn(C, generator=gen),
          p + ".5.running_mean": 0.1 * torch.randn(C, generator=gen), p + ".5.running_var": 1.0 + 0.2 * torch.rand(C, generator=gen)}
    bp = BP(0, ksize, stride)
    gs = [Q.q(torch.randn(n, C, generator=gen)) for n in DW_LENS]
    torch.set_num_threads(16)
    with torch.no_grad():
        d64 = torch.cat([Q.depthwise(g[None], sd, bp, F64, True)[0] for g in gs])
        runs = [Q.f32_runs(lambda g=g: Q.depthwise(g[None], sd, bp, F32, True)[0]) for g in gs]
        d32 = [torch.cat([u[i] for u in runs]) for i in range(len(runs[0]))]
        # the folded taps as the kernels hold them: float32 folds (ref_bf16.depthwise)
        sc = sd[p + ".5.weight"] / torch.sqrt(sd[p + ".5.running_var"] + Q.R.BN_EPS)
        taps = (sd[p + ".4.weight"][:, 0, :] * sc[:, None]).t().contiguous()
        bias = sd[p + ".4.bias"] * sc + (sd[p + ".5.bias"] - sd[p + ".5.running_mean"] * sc)
    return gs, d64, d32, taps, bias


@pytest.mark.parametrize("chunk", (2, 14, 16, 64))
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("ksize,C", ((15, 120), (31, 176), (7, 10)))
def test_stream_dwconv_chunk_by_chunk_equals_the_whole_sequence_reference(ksize, C, stride, chunk):
    lib = _lib.load()
    gs, d64, d32, taps, bias = _dw_case(ksize, C, stride)
    B, ld = len(gs), (C + 7) // 8 * 8
    louts = [(n - 1) // stride + 1 for n in DW_LENS]
    gd = []
    for g in gs:       # rows of ld columns; the pad columns hold NaN: the kernel masks them
        z = torch.full((g.shape[0], ld), float("nan"), dtype=torch.bfloat16)
        z[:, :C] = g.to(torch.bfloat16)
        gd.append(z.cuda())
    taps_d, bias_d = taps.cuda(), bias.contiguous().cuda()
    state = torch.full((B * (ksize - 1) * ld + NAN_TAIL,), float("nan"), dtype=torch.bfloat16, device="cuda")      # poisoned: hist = 0 makes it read as zeros
    got = [torch.full((lo, ld), SENTINEL, dtype=torch.bfloat16, device="cuda") for lo in louts]
    done, hist = [0] * B, [0] * B
    rounds = 0
    while any(done[b] < DW_LENS[b] for b in range(B)):
        ns = [max(0, min(chunk, DW_LENS[b] - done[b])) for b in range(B)]
        in_off, out_off, parts, no = [], [], [], []
        for b in range(B):
            in_off.append(sum(x.shape[0] for x in parts)); parts.append(gd[b][done[b]: done[b] + ns[b]])
            no.append((ns[b] - 1) // stride + 1 if ns[b] else 0)
            out_off.append(sum(no[:-1]))
        gin = _with_tail(torch.cat(parts))
        out = torch.full((sum(no), ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
        desc = [_i32(z) for z in (in_off, ns, hist, out_off)]           # held until the round has run
        _lib.check(lib.effconf_stream_dwconv(gin.data_ptr(), ld, C, taps_d.data_ptr(), bias_d.data_ptr(), ksize, stride, state.data_ptr(), desc[0].data_ptr(),
                                             desc[1].data_ptr(), desc[2].data_ptr(), desc[3].data_ptr(), B, max(ns), out.data_ptr(), 1,
                                             torch.cuda.current_stream().cuda_stream), "stream_dwconv", lib)
        torch.cuda.synchronize()
        for b in range(B):
            if ns[b]:
                o0 = done[b] // stride          # chunks of a strided layer start on even rows (the chunk sizes are even)
                got[b][o0: o0 + no[b]] = out[out_off[b]: out_off[b] + no[b]]
            done[b] += ns[b]
            hist[b] = min(hist[b] + ns[b], ksize - 1)
        rounds += 1
    full = torch.cat(got).double().cpu()
    dg = full[:, :C]
    assert bool(torch.isfinite(dg).all()), "NaN / inf in the output: the poisoned state or a pad column reached the result"
    assert not bool((dg == SENTINEL).any()), "output rows left unwritten"
    assert float(full[:, C:].abs().sum()) == 0.0, "pad columns are not zero"
    r = {s: x for s, x in Q.stage_ratios(dg, d64, d32, ksize, True, share_factor=0.0).items() if not s.startswith(("noise", "single"))}
    r["ulp"] = float(((dg - d64).abs() / (2.0 ** -8 * d64.abs() + 2e-5)).max())
    print("stream_edges | dwconv k %2d C %3d stride %d | chunk %2d | rounds %3d | rows %3d | %s" % (ksize, C, stride, chunk, rounds, dg.shape[0], "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
    bad = {s: x for s, x in r.items() if not x <= 1.0}
    assert not bad, (ksize, C, stride, chunk, bad, Q.worst_element(dg, d64, 2.0 ** -8 * d64.abs() + 2e-5))


# ------------------------------------------------------------------ sessions end to end
STREAM_MAX, STREAM_MEAN = 0.09, 0.012        # the project's bounds of the whole-utterance causal forward (tests/test_gpu_round3.py): the chunked path gets no extra margin
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pattern(name, total):
    """Cumulative frame counts after every push of a pattern; the last push brings the rest."""
    if name == "all":
        return [total]
    steps = {"24": [24] * (total // 24 + 1), "48": [48] * (total // 48 + 1), "96": [96] * (total // 96 + 1), "irregular": [7, 50, 1, 0, 23]}[name]
    cum, s = [], 0
    for x in steps:
        if s + x >= total:
            break
        s += x
        cum.append(s)
    return cum + [total]


def _stream_model(gname):
    g = np.load(os.path.join(GOLDEN, gname))
    small = "small" in gname
    cfg = named_config("EfficientConformerCTCSmall" if small else "Tiny")
    extra = {k[4:]: (bool(g[k]) if k == "cfg/causal" else int(g[k])) for k in g.files if k.startswith("cfg/")}
    cfg["encoder_params"] = dict(cfg["encoder_params"], **extra)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, int(g["weight_seed"]), cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    lens = g["mel_len"].tolist()
    mel, _ = synth.make_mel(len(lens), 80, max(lens), lens, seed=int(g["mel_seed"]))
    return g, m.cuda(), osd, torch.from_numpy(mel).cuda(), lens


def _run_pushes(sess, mel, lens, pattern, streams=None):
    """Every utterance as one stream pushed by `pattern` (its own cumulative counts: the streams end at different pushes) -> [out rows per stream]."""
    B = sess.max_streams
    streams = list(range(len(lens))) if streams is None else streams
    cums = {s: _pattern(pattern, lens[i]) for i, s in enumerate(streams)}
    rounds = max(len(c) for c in cums.values())
    outs = {s: [] for s in streams}
    for r in range(rounds):
        new, fin = [0] * B, [False] * B
        chunk = torch.zeros(B, mel.shape[1], max(mel.shape[2], 1), device=mel.device)
        for i, s in enumerate(streams):
            c = cums[s]
            if r < len(c):
                lo = c[r - 1] if r else 0
                new[s], fin[s] = c[r] - lo, r == len(c) - 1
                chunk[s, :, :new[s]] = mel[i, :, lo: c[r]]
        out, out_len = sess.push_mel(chunk, new, fin)
        for s in streams:
            outs[s].append(out[s, :int(out_len[s])])
    return [torch.cat(outs[s]) for s in streams]


@pytest.mark.parametrize("pattern", ("24", "48", "irregular", "all"))
@pytest.mark.parametrize("gname", ("stream_tiny_causal_T47.npz", "stream_tiny_causal_T100.npz", "stream_tiny_causal_l12_T47.npz", "stream_tiny_causal_l12_T100.npz"))
def test_session_on_tiny_equals_the_reference_goldens(gname, pattern):
    g, m, sd, mel, lens = _stream_model(gname)
    sess = m.encoder.open_stream(len(lens), max_frames=max(lens))
    assert sess.align_frames == 24
    got = _run_pushes(sess, mel, lens, pattern)
    whole, _, _ = m.encoder.forward_mel(mel, torch.tensor(lens).cuda())          # printed, not bounded: the distance to the encoder's own forward
    ref = torch.from_numpy(g["out"])
    worst = (0.0, 0.0)
    for b, n in enumerate(g["out_len"].tolist()):
        assert got[b].shape[0] == n, (gname, pattern, b, got[b].shape, n)
        assert bool(torch.isfinite(got[b]).all())
        d = (got[b].cpu() - ref[b, :n]).abs()
        own = (got[b] - whole[b, :n]).abs()
        print("stream_session | %-32s | pushes %-9s | stream %d | rows %2d | to the golden: max %.4f mean %.5f | to the encoder's own forward_mel: max %.4f mean %.5f" % (
            gname, pattern, b, n, float(d.max()), float(d.mean()), float(own.max()), float(own.mean())))
        worst = (max(worst[0], float(d.max())), max(worst[1], float(d.mean())))
    assert worst[0] < STREAM_MAX and worst[1] < STREAM_MEAN, (gname, pattern, worst)


def test_session_invariances_bit_for_bit():
    g, m, sd, mel, lens = _stream_model("stream_tiny_causal_l12_T100.npz")
    sess = m.encoder.open_stream(3)
    three = _run_pushes(sess, mel, lens, "irregular")
    for s in range(3):
        sess.reset(s)
    again = _run_pushes(sess, mel, lens, "irregular")
    assert all(torch.equal(a, b) for a, b in zip(three, again)), "the same pushes after reset differ"
    # stream 1 alone (as stream 2 of the session, the others idle) equals stream 1 among three
    for s in range(3):
        sess.reset(s)
    alone = _run_pushes(sess, mel[1:2], lens[1:2], "irregular", streams=[2])
    assert torch.equal(alone[0], three[1]), "a stream alone differs from the same stream among three"
    # a second session on the first one's state buffer, recycled as it is
    state = sess._state
    sess.close()
    other = m.encoder.open_stream(3)
    other.close()
    lib = other._lib
    other._state = state
    other._ptr = lib.effconf_stream_create(m.encoder._handle, 3, 0, state.data_ptr(), state.numel())
    assert other._ptr
    recycled = _run_pushes(other, mel, lens, "irregular")
    assert all(torch.equal(a, b) for a, b in zip(three, recycled)), "a second session on a recycled state buffer differs"


def test_push_audio_gives_the_whole_signal_mel_frames_and_the_oracle_output():
    cfg = named_config("Tiny")
    cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True)
    m = ModelCTC.from_config(cfg)
    sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    osd = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}
    m = m.cuda()
    lens = np.array([48000], dtype=np.int64)
    audio = torch.from_numpy(synth.make_audio(lens, seed=4))
    whole_mel, _ = m.encoder.mel_frontend(audio.cuda())
    sess = m.encoder.open_stream(1)
    mels, outs = [], []
    for lo in range(0, 48000, 4000):
        out, out_len = sess.push_audio(audio[:, lo: lo + 4000].cuda(), [4000], [lo + 4000 >= 48000])
        mels.append(sess.last_mel[0, :, :sess.last_mel_len[0]])
        outs.append(out[0, :int(out_len[0])])
    mel = torch.cat(mels, 1)
    assert mel.shape == whole_mel[0].shape and torch.equal(mel, whole_mel[0]), "push_audio's mel frames are not the whole-signal front end's"
    got = torch.cat(outs).cpu()
    with torch.no_grad():
        ref, ref_len = R.encoder(audio, torch.from_numpy(lens), osd, m.encoder.plan)
    assert got.shape[0] == int(ref_len[0])
    d = (got - ref[0, :got.shape[0]]).abs()
    print("stream_session | push_audio Tiny causal 3 s in pushes of 4000 samples | to the oracle: max %.4f mean %.5f" % (float(d.max()), float(d.mean())))
    assert float(d.max()) < STREAM_MAX and float(d.mean()) < STREAM_MEAN


def test_model_ctc_stream_tokens_equal_the_whole_utterance_greedy_labels():
    g, m, sd, mel, lens = _stream_model("stream_tiny_causal_T47.npz")       # (the oracle's smallest frame margins: 0.009, 0.64, 0.76)
    ln = torch.tensor(lens).cuda()
    out, out_len, _ = m.encoder.forward_mel(mel, ln)
    hm = m.head_margins(out, out_len)
    st = m.open_stream(len(lens))
    toks = [[] for _ in lens]
    B = len(lens)
    for lo in range(0, max(lens), 24):
        new = [max(0, min(24, n - lo)) for n in lens]
        fin = [lo < n <= lo + 24 for n in lens]
        chunk = torch.zeros(B, mel.shape[1], 24, device=mel.device)
        for b in range(B):
            chunk[b, :, :new[b]] = mel[b, :, lo: lo + new[b]]
        for b, t in enumerate(st.push_mel(chunk, new, fin)):
            toks[b] += t
    safe = 0
    for b in range(B):
        want = hm.labels[b, :int(hm.label_len[b])].tolist()
        if float(hm.min_margin[b]) > 0.15:
            safe += 1
            assert toks[b] == want, (b, toks[b], want)
    assert safe >= 1, "no utterance of the case has every frame margin above 0.15"


@pytest.mark.parametrize("left", (None, 64))
@pytest.mark.parametrize("pattern", ("24", "96"))
def test_session_on_small_equals_the_reference(pattern, left):
    """EfficientConformerCTC-Small causal (601 / 433 frames): the golden's rows [::4] and its argmax wherever its margin exceeds 0.15; with left_context = 64
    the same against the float32 oracle computed here."""
    g, m, sd, mel, lens = _stream_model("stream_small_causal.npz")
    if left is not None:
        cfg = named_config("EfficientConformerCTCSmall")
        cfg["encoder_params"] = dict(cfg["encoder_params"], causal=True, left_context=left)
        m2 = ModelCTC.from_config(cfg)
        m2.load_state_dict(m.state_dict())
        m = m2.cuda()
        torch.set_num_threads(16)
        with torch.no_grad():
            ref, ref_len = R.encoder_from_mel(mel.cpu(), torch.tensor(lens), sd, m.encoder.plan)
            logits = R.ctc_logits(ref, sd)
        top2 = logits.topk(2, -1).values
        out_len, rows, argmax, margin = ref_len.numpy(), ref[:, ::4], logits.argmax(-1).numpy(), (top2[..., 0] - top2[..., 1]).numpy()
    else:
        out_len, rows, argmax, margin = g["out_len"], torch.from_numpy(g["out_rows"]), g["argmax"], g["margin"]
    sess = m.encoder.open_stream(len(lens), max_frames=max(lens))
    got = _run_pushes(sess, mel, lens, pattern)
    worst, safe_n = (0.0, 0.0), 0
    for b, n in enumerate(out_len.tolist()):
        assert got[b].shape[0] == n, (b, got[b].shape, n)
        want = rows[b, :(n + 3) // 4]
        d = (got[b].cpu()[::4] - want).abs()
        worst = (max(worst[0], float(d.max())), max(worst[1], float(d.mean())))
        lg, _, _ = m._head(got[b][None].contiguous(), None, want_logits=True)
        am = lg[0].argmax(-1).cpu().numpy()
        safe = margin[b, :n] > 0.15
        safe_n += int(safe.sum())
        assert np.array_equal(am[safe], argmax[b, :n][safe]), (b, "argmax differs on frames whose margin exceeds 0.15")
    print("stream_session | Small causal left %s | pushes %s | max %.4f mean %.5f | %d safe frames" % (left, pattern, worst[0], worst[1], safe_n))
    assert safe_n > 20
    assert worst[0] < STREAM_MAX and worst[1] < STREAM_MEAN, worst
