"""Float64 restatement of the log-mel front end, an energy-aware per-element error bound, float32 stand-ins and a signal zoo.

The front end (csrc/mel.hip) is all float32 and transforms TWO frames as one complex FFT.  Its error is not a flat number in the log domain:

  * a float32 FFT leaves about eps32 * ||frame|| in EVERY bin, so a mel bin whose true power lies 1e-7 below the frame's energy (the
    leakage floor of a pure tone) is noise-dominated whoever computes it;
  * the pair separation X_b = (Z[k] - conj Z[N-k]) / 2i cancels frame a's spectrum only to float32 precision: a loud frame writes
    about eps32 * |X_a| into the frame it shares a transform with (t xor 1).

``bound`` restates that.  For output (b, m, t), with X the float64 spectrum of the windowed frame, fb the filterbank, M = sum_k fb[k,m] |X_k|^2,
e_own / e_partner the L2 norms of the windowed frame and of its partner (0 when the partner does not exist):

    delta = eps32 * sqrt(e_own^2 + e_partner^2)                      spectral error scale (per bin; a DFT's rounding error is spread
                                                                     evenly over the bins and is proportional to the INPUT's norm)
    A     = [sum_k fb[k,m] (2 |X_k| delta + delta^2) + eps32 * M] / (M + 1e-9)          log-domain model, constant 1
    U     = 3 eps32 |y|  (normalised: (3 eps32 |y| + eps32 |y - mean|) / std + eps32 |out|)   a few ulp of the log value itself

and an implementation with class constant c passes when  err <= c * A + U  for every element.  U is not scaled: it covers logf (<= 2 ulp on
the device), the rounding of sum + 1e-9 and of the float32 literal 1e-9, each below one ulp of a value near -20.7; 3 eps32 |y| = 7.4e-6 at the
floor, inside the 1e-5 the silent-tail assertion has always used.  Where A = 0 (an all-zero frame whose partner is all zero or absent) the
bound is U alone: the output must BE the floor.

The constants come from two CPU stand-ins, never from the kernel:
    (i)  ``standin_single``: float32 framing / window / rfft (complex64) / power / filterbank / log, one frame per transform (e_partner = 0)
    (ii) ``standin_paired``: the same arithmetic, two frames per complex64 FFT and the float32 pair separation
per signal class the constant is the worst ratio (err - U)+ / A of both over CAL_SEEDS; the kernel is held to MAX_MARGIN x the worst max and
MEAN_MARGIN x the worst mean (the margins of tests/bf16_parity.py for "reference noise against a different float32 summation order").
No torch.stft, no oracle/ref_encoder.py anywhere in this file.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23
FLOOR = 1e-9
MAX_MARGIN, MEAN_MARGIN = 4.0, 8.0
CAL_SEEDS = (0, 1, 2, 3, 4)
SHIPPED_MEAN, SHIPPED_STD = -5.6501, 4.2280


@dataclass(frozen=True)
class Settings:
    n_fft: int = 512
    win: int = 400
    hop: int = 160
    n_mels: int = 80
    sr: int = 16000
    normalize: bool = False
    mean: float = 0.0
    std: float = 1.0

    def tag(self) -> str:
        d = Settings()
        parts = ["%s=%s" % (k, getattr(self, k)) for k in ("win", "hop", "n_mels", "sr", "normalize") if getattr(self, k) != getattr(d, k)]
        return ",".join(parts) or "default"


DEFAULT = Settings()


# ---------------------------------------------------------------------------------------------------------------------------- definition
def hann(win: int, n_fft: int, symmetric: bool = False, off: Optional[int] = None) -> np.ndarray:
    """Hann(win), periodic, centred in n_fft (what torch.stft does with a window shorter than n_fft)."""
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2 if off is None else off
    w[off:off + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / (win - 1 if symmetric else win))
    return w


def filterbank(n_fft: int, n_mels: int, sr: int, slaney: bool = False, start_shift: int = 0) -> np.ndarray:
    """HTK triangles over [0, 8000] Hz on the rfft grid of `sr`, no area normalisation: (n_fft / 2 + 1, n_mels) float64."""
    freqs = np.linspace(0.0, sr // 2, n_fft // 2 + 1)
    if slaney:
        lin, step = 1000.0, 200.0 / 3.0
        mel = lambda f: np.where(f < lin, f / step, lin / step + np.log(np.maximum(f, 1e-30) / lin) / (np.log(6.4) / 27.0))
        inv = lambda m: np.where(m < lin / step, m * step, lin * np.exp((np.log(6.4) / 27.0) * (m - lin / step)))
    else:
        mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
        inv = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    m_pts = np.linspace(float(mel(np.float64(0.0))), float(mel(np.float64(8000.0))), n_mels + 2)
    f_pts = inv(m_pts)
    down = (freqs[:, None] - f_pts[None, :-2]) / (f_pts[1:-1] - f_pts[:-2])[None, :]
    up = (f_pts[None, 2:] - freqs[:, None]) / (f_pts[2:] - f_pts[1:-1])[None, :]
    fb = np.maximum(0.0, np.minimum(down, up))
    if start_shift:                                # fault: every filter starts one bin late (its first tap is lost)
        for m in range(n_mels):
            nz = np.nonzero(fb[:, m])[0]
            if len(nz):
                fb[nz[0]:nz[0] + start_shift, m] = 0.0
    return fb


def frame_index(length: int, n_fft: int, hop: int, pad_edge: bool = False, shift: int = 0) -> np.ndarray:
    """(T, n_fft) sample indices of the centred frames of an utterance of `length` samples, reflect padding at ITS OWN ends; T = length // hop + 1."""
    if length <= n_fft // 2:
        raise ValueError("reflect padding needs more than n_fft / 2 samples, got %d" % length)
    t = length // hop + 1
    s = hop * np.arange(t)[:, None] - n_fft // 2 + np.arange(n_fft)[None, :] + shift
    if pad_edge:
        return np.clip(s, 0, length - 1)
    s = np.abs(s)
    s = np.where(s >= length, 2 * (length - 1) - s, s)
    if s.min() < 0 or s.max() >= length:
        raise ValueError("reflection out of range")
    return s


def frames64(audio, lengths=None, st: Settings = DEFAULT):
    """Windowed float64 frames (B, Tm, n_fft) and the validity mask (B, Tm).  lengths = None: every row at the full row length (what a
    rectangular batch computes, zeros past an utterance's end are samples); else row b is padded, reflected and framed at lengths[b]."""
    a = np.asarray(audio, dtype=np.float64)
    bsz, n = a.shape
    tm = n // st.hop + 1
    w = hann(st.win, st.n_fft)
    fr = np.zeros((bsz, tm, st.n_fft))
    valid = np.zeros((bsz, tm), dtype=bool)
    for b in range(bsz):
        lb = n if lengths is None else int(lengths[b])
        idx = frame_index(lb, st.n_fft, st.hop)
        fr[b, :idx.shape[0]] = a[b][idx] * w
        valid[b, :idx.shape[0]] = True
    return fr, valid


def _fbsum(x, fb):
    """x (B, T, K) @ fb (K, n_mels) in float64 without the BLAS thread pool (a few hundred frames: its start-up costs more than the sum)."""
    return np.einsum("btk,km->btm", x, fb)


@dataclass
class Reference:
    mel: np.ndarray            # (B, n_mels, Tm) float64; NaN at columns that do not exist for the row
    valid: np.ndarray          # (B, Tm)
    model: np.ndarray          # A of the module docstring, (B, n_mels, Tm)
    ulp: np.ndarray            # U
    settings: Settings = field(default=DEFAULT)


def reference(audio, lengths=None, st: Settings = DEFAULT) -> Reference:
    fr, valid = frames64(audio, lengths, st)
    spec = np.fft.rfft(fr, axis=-1)
    mag = np.abs(spec)                                                      # (B, Tm, K)
    fb = filterbank(st.n_fft, st.n_mels, st.sr)
    m_pow = _fbsum(mag ** 2, fb)                                            # (B, Tm, n_mels)
    y = np.log(m_pow + FLOOR)
    e = np.sqrt((fr ** 2).sum(-1)) * valid                                   # (B, Tm)
    tm = e.shape[1]
    partner = np.arange(tm) ^ 1
    e_p = np.where((partner < tm)[None, :], e[:, np.minimum(partner, tm - 1)], 0.0)
    e_p = e_p * np.where(partner < tm, valid[:, np.minimum(partner, tm - 1)], False)
    delta = EPS32 * np.sqrt(e ** 2 + e_p ** 2)                              # (B, Tm)
    fsum = fb.sum(0)                                                        # (n_mels,)
    perr = 2.0 * delta[:, :, None] * _fbsum(mag, fb) + (delta ** 2)[:, :, None] * fsum[None, None, :] + EPS32 * m_pow
    model = perr / (m_pow + FLOOR)
    if st.normalize:
        out = (y - st.mean) / st.std
        ulp = (3.0 * EPS32 * np.abs(y) + EPS32 * np.abs(y - st.mean)) / st.std + EPS32 * np.abs(out)
        model = model / st.std
    else:
        out, ulp = y, 3.0 * EPS32 * np.abs(y)
    out = np.where(valid[:, :, None], out, np.nan)
    if not np.isfinite(out[valid]).all():
        raise AssertionError("float64 reference is not finite on a valid frame")
    tr = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1))
    return Reference(tr(out), valid, tr(model), tr(ulp), st)


def mel_fp64(audio, lengths=None, n_fft=512, win=400, hop=160, n_mels=80, sr=16000, normalize=False, mean=0.0, std=1.0) -> np.ndarray:
    """Independent float64 restatement of Spectrogram(power=2) + MelScale(htk, norm=None, f_max=8000) + log(x + 1e-9) (+ normalisation):
    explicit framing, numpy rfft in float64 -> (B, n_mels, L // hop + 1); with `lengths`, NaN past each row's own last frame."""
    return reference(audio, lengths, Settings(n_fft, win, hop, n_mels, sr, normalize, mean, std)).mel


def _elements(got, ref: Reference):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.mel.shape, (got.shape, ref.mel.shape)
    v = np.broadcast_to(ref.valid[:, None, :], got.shape)
    g, r, a, u = got[v], ref.mel[v], ref.model[v], ref.ulp[v]
    assert g.size == int(ref.valid.sum()) * got.shape[1] and g.size > 0          # every element of every valid frame, nothing left out
    if not np.isfinite(r).all():
        raise AssertionError("reference not finite")
    err = np.abs(g - r)
    return np.where(np.isfinite(err), err, np.inf), a, u                        # a NaN / inf output is an infinite error, never a skipped element


def ratios(got, ref: Reference) -> Tuple[float, float, float]:
    """(max, mean) of (err - U)+ / A over EVERY element of every valid frame, and the raw worst log-domain error.  A = 0: 0 if err <= U else inf."""
    err, a, u = _elements(got, ref)
    ex = np.maximum(err - u, 0.0)
    q = np.where(a > 0.0, ex / np.where(a > 0.0, a, 1.0), np.where(ex > 0.0, np.inf, 0.0))
    return float(q.max()), float(q.mean()), float(err.max())


def fill(got, ref: Reference, c: float) -> float:
    """Worst err / (c * A + U): how much of the bound with constant c an implementation uses (<= 1 passes)."""
    err, a, u = _elements(got, ref)
    return float((err / (c * a + u)).max())


# ---------------------------------------------------------------------------------------------------------------------------- stand-ins
FAULTS = ("hann_symmetric", "window_offset_55", "pad_edge", "frame_shift_1", "bins_swapped", "pair_sign_leak_1e-4", "slaney_scale",
          "filter_start_off_by_one", "floor_1e-10", "std_for_inv_std", "mean_dropped", "silent_frame_1e-2_off")


def _standin(audio, lengths, st: Settings, paired: bool, fault: Optional[str]) -> np.ndarray:
    a = np.asarray(audio, dtype=np.float32)
    bsz, n = a.shape
    tm = n // st.hop + 1
    w = hann(st.win, st.n_fft, symmetric=fault == "hann_symmetric",
             off=55 if fault == "window_offset_55" else None).astype(np.float32)
    fb = torch.from_numpy(filterbank(st.n_fft, st.n_mels, st.sr, slaney=fault == "slaney_scale",
                                     start_shift=1 if fault == "filter_start_off_by_one" else 0).astype(np.float32))
    out = np.full((bsz, st.n_mels, tm), np.nan, dtype=np.float32)
    for b in range(bsz):
        lb = n if lengths is None else int(lengths[b])
        idx = frame_index(lb, st.n_fft, st.hop, pad_edge=fault == "pad_edge", shift=0)
        if fault == "frame_shift_1":
            idx = np.clip(idx + 1, 0, lb - 1)
        fr = torch.from_numpy(a[b][idx] * w[None, :])                       # float32 (T, n_fft)
        t = fr.shape[0]
        k = st.n_fft // 2 + 1
        if not paired:
            z = torch.fft.rfft(fr, dim=-1)
            re, im = z.real, z.imag
        else:
            fe = torch.cat([fr, torch.zeros((t & 1), st.n_fft)], 0) if t & 1 else fr
            z = torch.fft.fft(torch.complex(fe[0::2], fe[1::2]), dim=-1)    # complex64 (T/2, n_fft)
            zc = torch.roll(torch.flip(z, dims=[-1]), 1, dims=-1)           # Z[(N - k) % N]
            zr, zi, cr, ci = z.real[:, :k], z.imag[:, :k], zc.real[:, :k], zc.imag[:, :k]
            ar, ai = 0.5 * (zr + cr), 0.5 * (zi - ci)
            br, bi = 0.5 * (zi + ci), 0.5 * (cr - zr)
            if fault is not None and fault.startswith("pair_sign_leak_"):   # each spectrum picks up 1e-4 (or what the name says) of the other's
                lk = np.float32(float(fault.rsplit("_", 1)[1]))
                ar, ai, br, bi = ar + lk * br, ai + lk * bi, br + lk * ar, bi + lk * ai
            re = torch.stack([ar, br], 1).reshape(-1, k)[:t]
            im = torch.stack([ai, bi], 1).reshape(-1, k)[:t]
        p = re * re + im * im
        if fault == "bins_swapped":
            p = p.clone(); p[:, [40, 41]] = p[:, [41, 40]]
        mel = p @ fb
        y = torch.log(mel + np.float32(1e-10 if fault == "floor_1e-10" else FLOOR))
        if fault == "silent_frame_1e-2_off":
            silent = (fr == 0).all(-1)
            y = torch.where(silent[:, None], y + np.float32(1e-2), y)
        if st.normalize:
            mean = np.float32(0.0 if fault == "mean_dropped" else st.mean)
            scale = np.float32(st.std) if fault == "std_for_inv_std" else np.float32(1.0) / np.float32(st.std)
            y = (y - mean) * scale
        out[b, :, :t] = y.numpy().T
    return out


def standin_single(audio, lengths=None, st: Settings = DEFAULT, fault: Optional[str] = None) -> np.ndarray:
    return _standin(audio, lengths, st, False, fault)


def standin_paired(audio, lengths=None, st: Settings = DEFAULT, fault: Optional[str] = None) -> np.ndarray:
    return _standin(audio, lengths, st, True, fault)


def reference_single(audio, lengths=None, st: Settings = DEFAULT) -> Reference:
    """The bound of an implementation that transforms every frame alone: e_partner = 0."""
    ref = reference(audio, lengths, st)
    fr, valid = frames64(audio, lengths, st)
    e = np.sqrt((fr ** 2).sum(-1)) * valid
    spec = np.abs(np.fft.rfft(fr, axis=-1))
    fb = filterbank(st.n_fft, st.n_mels, st.sr)
    m_pow = _fbsum(spec ** 2, fb)
    delta = EPS32 * e
    perr = 2.0 * delta[:, :, None] * _fbsum(spec, fb) + (delta ** 2)[:, :, None] * fb.sum(0)[None, None, :] + EPS32 * m_pow
    model = perr / (m_pow + FLOOR) / (st.std if st.normalize else 1.0)
    return Reference(ref.mel, ref.valid, np.ascontiguousarray(model.transpose(0, 2, 1)), ref.ulp, st)


def silent_frames(audio, lengths=None, st: Settings = DEFAULT) -> np.ndarray:
    """(B, Tm) mask of the valid frames whose windowed samples are ALL zero: the definition gives exactly log(1e-9) there."""
    fr, valid = frames64(audio, lengths, st)
    return valid & (fr == 0.0).all(-1)


# ---------------------------------------------------------------------------------------------------------------------------- signal zoo
ZOO_LEN = 24000                                     # 151 frames at hop 160
ZOO_LENGTHS = (24000, 17461, 9120)                  # last frames 150 (even), 109 (odd), 57 (odd); 9120 = 57 * 160 exactly


def _rng(seed: int, name: str):
    return np.random.Generator(np.random.PCG64([seed, sum(ord(c) * (i + 1) for i, c in enumerate(name))]))


def _noise(g, n, amp):
    return np.clip(amp * g.standard_normal(n), -1.0, 1.0)


def _tone(g, n, hz, sr, amp=1.0):
    return amp * np.sin(2.0 * np.pi * hz * np.arange(n) / sr + g.uniform(0.0, 2.0 * np.pi))


def _bursts(n, start, width=160, period=640):
    """0 / 1 mask: `width` samples on from `start` every `period` samples.  With hop 160 and a 400-tap window, start = -200 lights frame 4j (even)
    and leaves its partner 4j + 1 untouched; start = +200 lights frame 4j + 1 (odd) and leaves its partner 4j untouched."""
    m = np.zeros(n)
    for s in range(start, n, period):
        m[max(s, 0):max(s + width, 0)] = 1.0
    return m


def _filter_peak_hz(m=40, n_mels=80):
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    m_pts = np.linspace(mel(0.0), mel(8000.0), n_mels + 2)
    return float(700.0 * (10.0 ** (m_pts[m + 1] / 2595.0) - 1.0))


def _impulses(g, n, row):
    x = np.zeros(n)
    amp = g.uniform(0.5, 1.0)
    t = int(g.integers(8, 40))
    pos = {0: [0, 160 * t - 256, n - 1],                         # reflect boundary itself, a frame's first sample, the last sample
           1: [1, 160 * t - 200, 160 * (t + 9) - 199, n - 2],   # next to the boundary, the window's zero tap and its first non-zero tap
           2: [255, 256, 257, 160 * t + 199, n - 256, n - 257]}[row % 3]
    for p in pos:
        x[p] = amp
    return x


def _loud(g, n, sr):
    return 0.7 * _tone(g, n, 1000.0, sr) + np.clip(0.1 * g.standard_normal(n), -0.3, 0.3)


def _make_row(name: str, g, n: int, row: int, sr: int) -> np.ndarray:
    nyq = sr / 2.0
    bin_hz = sr / 512.0
    if name.startswith("noise_"):
        return _noise(g, n, float(name[6:]))
    if name == "tone_bin_centre":
        return _tone(g, n, 32 * bin_hz, sr)
    if name == "tone_between_bins":
        return _tone(g, n, 32.5 * bin_hz, sr)
    if name == "tone_bin_1":
        return _tone(g, n, bin_hz, sr)
    if name == "tone_near_nyquist":
        return _tone(g, n, nyq - 0.5 * bin_hz, sr)
    if name == "tone_filter_peak":
        return _tone(g, n, min(_filter_peak_hz(), 0.9 * nyq), sr)
    if name == "dc_offset":
        return np.full(n, g.uniform(0.3, 0.9))
    if name == "chirp":
        t = np.arange(n) / sr
        f0, f1 = 50.0, 0.98 * min(nyq, 8000.0)
        return np.sin(2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / (n / sr)) + g.uniform(0.0, 2.0 * np.pi))
    if name == "square_clipped":
        return np.clip(10.0 * _tone(g, n, 440.0, sr), -1.0, 1.0)
    if name == "impulses":
        return _impulses(g, n, row)
    if name == "tone_plus_noise_-50dB":
        return np.clip(0.9 * _tone(g, n, 1000.0, sr) + 10.0 ** -2.5 * g.standard_normal(n), -1.0, 1.0)
    if name == "silence_inside":
        x = _noise(g, n, 0.3)
        for s in (2000, 5000, n - 3000):
            x[s:s + 1000 + 160 * row] = 0.0
        return x
    if name.startswith("step_"):
        # step_<loud frame parity>_<quiet level>: loud bursts that fall in even (odd) frames only next to a partner that holds `quiet`
        _, parity, quiet = name.split("_")
        mask = _bursts(n, -200 if parity == "even" else 200)
        q = 0.0 if quiet == "silent" else float(quiet)
        return mask * _loud(g, n, sr) + (1.0 - mask) * q * g.standard_normal(n)
    if name == "ends_loud":
        return np.clip(0.5 * g.standard_normal(n) + 0.5 * _tone(g, n, 2000.0, sr), -1.0, 1.0)
    raise KeyError(name)


ZOO = ("noise_1.0", "noise_0.1", "noise_1e-4", "noise_1e-6", "tone_bin_centre", "tone_between_bins", "tone_bin_1", "tone_near_nyquist",
       "tone_filter_peak", "dc_offset", "chirp", "square_clipped", "impulses", "tone_plus_noise_-50dB", "silence_inside",
       "step_even_silent", "step_odd_silent", "step_even_1e-3", "step_odd_1e-3", "step_even_1e-4", "ends_loud")


def zoo_lengths(name: str, hop: int = 160) -> Tuple[int, ...]:
    if name == "ends_loud":
        # rectangular: the first frame that holds no sample of the utterance is ceil((Lb + win/2) / hop): odd for 15900 (its partner, frame 100,
        # is loud), even for 16000; ragged: last frames 99 (odd) and 100 (even, no partner)
        return (ZOO_LEN, 16000, 15900)
    return ZOO_LENGTHS


def make_signal(name: str, seed: int, sr: int = 16000):
    """(audio (B, L) float32 with zeros past each row's length, lengths (B,) int64) of zoo class `name`."""
    lens = np.asarray(zoo_lengths(name), dtype=np.int64)
    x = np.zeros((len(lens), int(lens.max())), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = _make_row(name, _rng(seed, "%s/%d" % (name, b)), int(n), b, sr).astype(np.float32)
    return x, lens


# ---------------------------------------------------------------------------------------------------------------------------- constants
@functools.lru_cache(maxsize=None)
def zoo_case(name: str, seed: int, st: Settings = DEFAULT, ragged: bool = False):
    """(audio, lengths or None, bound of the paired evaluation, bound of the single-frame evaluation) of one zoo class and seed."""
    audio, lens = make_signal(name, seed, st.sr)
    ln = lens if ragged else None
    return audio, ln, reference(audio, ln, st), reference_single(audio, ln, st)


def calibrate(cases) -> Dict[str, float]:
    """Worst (max, mean) ratio of the two stand-ins, each against its own bound, over `cases` = [(audio, lengths or None, paired bound, single bound)]."""
    out = {"single_max": 0.0, "single_mean": 0.0, "paired_max": 0.0, "paired_mean": 0.0}
    for audio, ln, ref_p, ref_s in cases:
        for tag, fn, ref in (("single", standin_single, ref_s), ("paired", standin_paired, ref_p)):
            mx, mean, _ = ratios(fn(audio, ln, ref.settings), ref)
            out[tag + "_max"] = max(out[tag + "_max"], mx)
            out[tag + "_mean"] = max(out[tag + "_mean"], mean)
    out["c_max"] = max(out["single_max"], out["paired_max"])
    out["c_mean"] = max(out["single_mean"], out["paired_mean"])
    return out


@functools.lru_cache(maxsize=None)
def class_constant(name: str, st: Settings = DEFAULT, ragged: bool = False) -> Dict[str, float]:
    """The constant of zoo class `name`: ``calibrate`` over CAL_SEEDS."""
    return calibrate([zoo_case(name, seed, st, ragged) for seed in CAL_SEEDS])


def case_of(audio, lengths, st: Settings = DEFAULT):
    return audio, lengths, reference(audio, lengths, st), reference_single(audio, lengths, st)


def verdict(got, ref: Reference, const: Dict[str, float]) -> Dict[str, float]:
    mx, mean, raw = ratios(got, ref)
    return {"max": mx, "mean": mean, "raw": raw, "fill": fill(got, ref, MAX_MARGIN * const["c_max"]), "max_limit": MAX_MARGIN * const["c_max"], "mean_limit": MEAN_MARGIN * const["c_mean"],
            "ok": bool(mx <= MAX_MARGIN * const["c_max"] and mean <= MEAN_MARGIN * const["c_mean"])}


def report_line(case: str, const: Dict[str, float], v: Dict[str, float]) -> str:
    return ("%-46s standin c_max %9.3g c_mean %9.3g (single %.3g / paired %.3g) | kernel max %9.3g (limit %9.3g) mean %9.3g (limit %9.3g) raw %.3e fill %.3f %s"
            % (case, const["c_max"], const["c_mean"], const["single_max"], const["paired_max"], v["max"], v["max_limit"], v["mean"],
               v["mean_limit"], v["raw"], v["fill"], "ok" if v["ok"] else "EXCEEDED"))
