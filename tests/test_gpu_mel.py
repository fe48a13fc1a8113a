"""The log-mel kernel (csrc/mel.hip) against the float64 restatement under the energy-aware bound of tests/mel_ref.py (-m gpu).

Every element of every valid frame is compared; the class constant comes from the CPU stand-ins (mel_ref.class_constant / calibrate) and the kernel
gets 4x its max and 8x its mean.  Rectangular batches run through ``mel_frontend``, ragged batches through the "mel" trace entry of a forward from
audio.  Every case prints one report line (profiles/mel_parity.txt is the -s output of this file)."""
import numpy as np
import pytest
import torch

import mel_ref as M
from efficientconformer_amd import ModelCTC, _lib, named_config, synth

pytestmark = pytest.mark.gpu

FLOOR32 = float(np.log(np.float32(1e-9)))
NORM = dict(normalize=True, mean=M.SHIPPED_MEAN, std=M.SHIPPED_STD)
# classes whose construction does not depend on the default frame geometry: run under every front-end setting
SETTING_CLASSES = ("noise_0.1", "tone_between_bins", "tone_near_nyquist", "chirp", "impulses", "silence_inside", "tone_plus_noise_-50dB")
_ENC = {}


def _encoder(**front):
    """The Tiny encoder with front-end parameters replaced (reference JSON keys); cached per setting."""
    key = tuple(sorted(front.items()))
    if key not in _ENC:
        cfg = named_config("Tiny")
        cfg["encoder_params"].update(front)
        m = ModelCTC.from_config(cfg)
        sd = synth.make_state_dict(m.encoder.plan, 7, cfg["tokenizer_params"]["vocab_size"], prefix="encoder.")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _ENC[key] = m.cuda().encoder
    return _ENC[key]


def _settings(enc) -> M.Settings:
    p = enc.plan
    return M.Settings(p.n_fft, p.win_length, p.hop_length, p.n_mels, p.sample_rate, p.normalize, p.mean if p.normalize else 0.0,
                      p.std if p.normalize else 1.0)


def _rect(enc, audio):
    mel, _ = enc.mel_frontend(torch.from_numpy(audio).cuda())
    return mel.cpu().numpy()


def _ragged(enc, audio, lens):
    enc.ragged = True
    try:
        _, _, tr = enc.trace_forward(torch.from_numpy(audio).cuda(), torch.from_numpy(lens).cuda())
    finally:
        enc.ragged = False
    return tr["mel"].numpy().reshape(audio.shape[0], enc.plan.n_mels, -1)


def _check(case, got, ref, const):
    v = M.verdict(got, ref, const)
    line = M.report_line(case, const, v)
    print(line)
    assert v["ok"], line
    return v


def _check_silent(case, got, audio, lens, st):
    """An all-zero frame yields log(1e-9) (its normalised value) to 1e-5, whatever the frame it shares a transform with holds."""
    sil = M.silent_frames(audio, lens, st)
    want = (FLOOR32 - st.mean) / st.std if st.normalize else FLOOR32
    if sil.any():
        d = np.abs(np.transpose(got, (0, 2, 1))[sil].astype(np.float64) - want)
        print("%-46s %d all-zero frames: worst distance from the floor %.3e" % (case, int(sil.sum()), d.max()))
        assert d.max() <= 1e-5, (case, float(d.max()))
    return int(sil.sum())


# ---------------------------------------------------------------------------------------------------------------- zoo, default settings
@pytest.mark.parametrize("name", M.ZOO)
def test_zoo_rectangular_vs_float64_bound(name):
    enc = _encoder()
    audio, ln, ref, _ = M.zoo_case(name, 0)
    got = _rect(enc, audio)
    assert got.shape == ref.mel.shape and ref.valid.all()
    _check(name + "/rect", got, ref, M.class_constant(name))
    assert _check_silent(name + "/rect", got, audio, None, M.DEFAULT) > 0          # every class has the zero tail of its shorter rows


@pytest.mark.parametrize("name", M.ZOO)
def test_zoo_ragged_vs_float64_bound(name):
    enc = _encoder()
    audio, ln, ref, _ = M.zoo_case(name, 0, M.DEFAULT, True)
    got = _ragged(enc, audio, ln)
    _check(name + "/ragged", got, ref, M.class_constant(name, M.DEFAULT, True))
    _check_silent(name + "/ragged", got, audio, ln, M.DEFAULT)


@pytest.mark.parametrize("name", ["step_even_silent", "step_odd_silent", "ends_loud", "silence_inside", "impulses"])
def test_all_zero_frames_read_the_floor_next_to_any_partner(name):
    """The classes built for it: silent frames that share a transform with a loud one, on both parities, rectangular and ragged, plain and
    normalised.  The separation X_b = (Z[k] - conj Z[N-k]) / 2i cancels the loud frame only to float32 precision; the definition has no such term."""
    for front in ({}, NORM):
        enc = _encoder(**front)
        st = _settings(enc)
        audio, lens = M.make_signal(name, 1)
        n = _check_silent("%s/rect/%s" % (name, st.tag()), _rect(enc, audio), audio, None, st)
        n += _check_silent("%s/ragged/%s" % (name, st.tag()), _ragged(enc, audio, lens), audio, lens, st)
        assert n > 10
        if name.startswith("step"):          # the partner of a silent frame IS loud here
            fr, _ = M.frames64(audio, None, st)
            e = np.sqrt((fr ** 2).sum(-1))
            sil = M.silent_frames(audio, None, st)
            t = np.arange(e.shape[1])
            assert (e[:, np.minimum(t ^ 1, e.shape[1] - 1)][sil] > 1.0).sum() > 10


# ---------------------------------------------------------------------------------------------------------------- length edges
def _edge_lengths(hop=160, n_fft=512):
    ls = {n_fft // 2 + 1, 50 * hop - 1, 50 * hop, 50 * hop + 1}
    for t in (2, 31, 32, 33, 64, 65, 257):                       # frame counts at the pair edge and at the 32-frame tile edge
        ls |= {l for l in ((t - 1) * hop, (t - 1) * hop + 1, t * hop - 1) if l > n_fft // 2}
    return np.array(sorted(ls, reverse=True), dtype=np.int64)


def _edge_batch(seed, lens):
    """Loud noise plus a tone up to every row's last sample and impulses on the reflect boundaries: a frame that reflects at the wrong index, or a
    row that reads its neighbour's samples, lands far outside the bound."""
    g = np.random.Generator(np.random.PCG64([seed, 0xED6E]))
    x = np.zeros((len(lens), int(lens.max())), dtype=np.float32)
    for b, n in enumerate(lens.tolist()):
        row = np.clip(0.3 * g.standard_normal(n) + 0.4 * np.sin(2 * np.pi * 1234.5 * np.arange(n) / 16000 + g.uniform(0, 6.28)), -1, 1)
        row[[0, n - 1]] = 1.0
        row[[1, n - 2]] = -1.0
        x[b, :n] = row
    return x


def test_length_edges_ragged_and_alone():
    enc = _encoder()
    lens = _edge_lengths()
    frames = sorted(set((lens // 160 + 1).tolist()))
    assert frames == [2, 31, 32, 33, 50, 51, 64, 65, 257] and 257 in lens.tolist()
    const = M.calibrate([M.case_of(_edge_batch(seed, lens), lens) for seed in M.CAL_SEEDS])
    audio = _edge_batch(7, lens)
    ref = M.reference(audio, lens)
    rag = _ragged(enc, audio, lens)
    _check("length_edges/ragged", rag, ref, const)
    alone_all = np.full_like(rag, np.nan)
    for b, n in enumerate(lens.tolist()):
        tb = n // 160 + 1
        alone = _rect(enc, np.ascontiguousarray(audio[b:b + 1, :n]))
        assert alone.shape == (1, 80, tb)
        # a ragged row IS the utterance alone on its valid frames, bit for bit; columns at or past its own frame count are not compared
        assert np.array_equal(alone[0].view(np.uint32), np.ascontiguousarray(rag[b, :, :tb]).view(np.uint32)), (n, tb, float(np.abs(alone[0] - rag[b, :, :tb]).max()))
        alone_all[b, :, :tb] = alone[0]
    _check("length_edges/alone", alone_all, ref, const)


def test_one_frame_does_not_exist_and_is_refused_by_name():
    """Frame count 1 needs fewer than hop samples, reflect padding needs more than n_fft / 2 > hop: the shortest utterance has 2 frames (257 samples, in
    test_length_edges_ragged_and_alone); anything shorter is an error that says so, ragged and rectangular."""
    enc = _encoder()
    audio = torch.from_numpy(synth.make_audio(np.array([4000, 4000]), seed=3)).cuda()
    enc.ragged = True
    try:
        with pytest.raises(_lib.EffconfError, match="length"):
            enc(audio, torch.tensor([4000, 256]).cuda())
        with pytest.raises(_lib.EffconfError, match="length"):
            enc(audio, torch.tensor([4000, 159]).cuda())
    finally:
        enc.ragged = False
    with pytest.raises(_lib.EffconfError, match="n_fft / 2"):
        enc.mel_frontend(audio[:, :256].contiguous())


# ---------------------------------------------------------------------------------------------------------------- settings
def _run_setting(front, classes=SETTING_CLASSES):
    enc = _encoder(**front)
    st = _settings(enc)
    for name in classes:
        audio, ln, ref, _ = M.zoo_case(name, 0, st)
        got = _rect(enc, audio)
        assert got.shape == ref.mel.shape, (got.shape, ref.mel.shape)
        _check("%s/rect/%s" % (name, st.tag()), got, ref, M.class_constant(name, st))
        _check_silent("%s/rect/%s" % (name, st.tag()), got, audio, None, st)
    return enc, st


@pytest.mark.parametrize("n_mels", [40, 64, 68, 80, 84, 128])
def test_settings_n_mels(n_mels):
    """Fewer mels than lanes, exactly one per lane, the second slot per lane (m = lane + 64) at 4, 16, 20 and 64 entries, the MM = 128 instantiation."""
    _, st = _run_setting(dict(n_mels=n_mels))
    assert st.n_mels == n_mels


@pytest.mark.parametrize("n_mels", [65, 81])
def test_settings_n_mels_not_a_multiple_of_four_is_refused_by_name(n_mels):
    """The mel image's rows feed 16-byte loads of the subsampling kernels: the library takes multiples of 4 only and says so (effconf_encoder_create)."""
    with pytest.raises(_lib.EffconfError, match="n_mels = %d" % n_mels):
        _encoder(n_mels=n_mels).mel_frontend(torch.zeros(1, 4000).cuda())
    _ENC.pop((("n_mels", n_mels),), None)


def test_settings_sample_rate_8000_filters_above_nyquist_read_the_floor():
    enc, st = _run_setting(dict(sample_rate=8000))
    assert (st.sr, st.win, st.hop) == (8000, 200, 80)
    dead = np.nonzero(M.filterbank(512, 80, 8000).sum(0) == 0)[0]
    assert len(dead) > 10
    audio, _ = M.make_signal("noise_1.0", 2, 8000)
    got = _rect(enc, audio)
    assert np.abs(got[:, dead].astype(np.float64) - FLOOR32).max() <= 1e-5


def test_settings_sample_rate_32000():
    _, st = _run_setting(dict(sample_rate=32000, win_length_ms=10, hop_length_ms=5))
    assert (st.sr, st.win, st.hop) == (32000, 320, 160)


@pytest.mark.parametrize("win", [320, 400, 512])
def test_settings_win_length(win):
    _, st = _run_setting(dict(win_length_ms=win / 16.0))
    assert st.win == win


@pytest.mark.parametrize("hop", [80, 160, 200])
def test_settings_hop(hop):
    _, st = _run_setting(dict(hop_length_ms=hop / 16.0))
    assert st.hop == hop


def test_settings_normalize_with_the_shipped_statistics():
    _, st = _run_setting(NORM, SETTING_CLASSES + ("step_even_silent", "noise_1e-4"))
    assert st.normalize and (st.mean, st.std) == (M.SHIPPED_MEAN, M.SHIPPED_STD)


def test_settings_ragged_at_another_hop_and_mel_count():
    """The ragged frame count Lb / hop + 1 and the (b, m) row pitch with settings other than 160 / 80."""
    enc = _encoder(hop_length_ms=12.5, n_mels=40)
    st = _settings(enc)
    assert (st.hop, st.n_mels) == (200, 40)
    for name in ("noise_0.1", "impulses"):
        audio, lens = M.make_signal(name, 0)
        got = _ragged(enc, audio, lens)
        _check("%s/ragged/%s" % (name, st.tag()), got, M.reference(audio, lens, st), M.class_constant(name, st, True))
