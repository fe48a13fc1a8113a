#!/usr/bin/env python3
"""Capture golden vectors by executing the ACTUAL reference (build container only).

Imports burchim/EfficientConformer from /root/reference with import-time stubs for
its absent third-party dependencies, loads key-seeded
weights (efficientconformer_amd/synth.py), drives the reference encoder *from
mel* on seeded inputs and writes small fixtures to tests/golden/.  Only tensors
leave this script: no reference source, bytecode or text is written anywhere.
It refuses to run where /root/reference is absent (e.g. the GPU box).

    python tools/make_goldens.py            # regenerate every fixture
    python tools/make_goldens.py --only-rnnt-beam   # only tests/golden/rnnt_beam_*.npz (from the stored rnnt_*.npz encoder outputs)
    python tools/make_goldens.py --only-rnnt-beam-lm   # only tests/golden/rnnt_beam_lm_*.npz (the beam search with the reference's LM attached; stored rnnt_*.npz, lm_TinyLM.npz)
    python tools/make_goldens.py --only-rnnt-lattice   # only tests/golden/rnnt_lattice_*.npz (from the stored rnnt_*.npz encoder outputs)
    python tools/make_goldens.py --only-interctc       # only tests/golden/interctc_tiny_*.npz (the reference's ConformerEncoderInterCTC on Tiny)
    python tools/make_goldens.py --only-lm           # only tests/golden/lm_*.npz (LSTM language model; TinyLM's rescoring bias from tiny_T*.npz)
"""
import os
import sys
import types
import zlib

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from efficientconformer_amd import synth  # noqa: E402
from efficientconformer_amd.config import build_plan, named_config  # noqa: E402


def import_reference():
    if not os.path.isdir(REF):
        sys.exit("make_goldens: %s not present; goldens can only be regenerated in the build container" % REF)

    class _Any(nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

        def forward(self, x, *a, **k):
            return x
    ta = types.ModuleType("torchaudio")
    tr = types.ModuleType("torchaudio.transforms")
    for n in ("Spectrogram", "MelScale", "FrequencyMasking", "TimeMasking"):
        setattr(tr, n, _Any)
    ta.transforms = tr
    sys.modules["torchaudio"] = ta
    sys.modules["torchaudio.transforms"] = tr
    sys.path.insert(0, REF)
    import models.attentions as att
    import models.encoders as enc
    return enc, att


def reference_rnnt_greedy(f, f_len, dec_params, joint_params, sd):
    """Execute the reference's own Transducer.gready_search_decoding (transducer.py:139-186) on given encoder
    outputs: a Transducer object is assembled around the reference's RnnDecoder / JointNetwork classes (without
    Model.__init__: no tokenizer file, optimizer or loss here) and its real method is called."""
    _stub_third_party()
    import models.transducer as tr
    import models.decoders as dec
    import models.joint_networks as jn
    obj = tr.Transducer.__new__(tr.Transducer)
    nn.Module.__init__(obj)
    obj.decoder = dec.RnnDecoder(dec_params).eval()
    obj.joint_network = jn.JointNetwork(f.shape[-1], dec_params["dim_model"], dec_params["vocab_size"], joint_params).eval()
    obj.decoder.load_state_dict(to_torch({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}), strict=True)
    obj.joint_network.load_state_dict(to_torch({k[len("joint_network."):]: v for k, v in sd.items() if k.startswith("joint_network.")}), strict=True)
    obj.max_consec_dec_step = dec_params.get("max_consec_dec_step", 5)

    class _Ids:                                   # tokenizer.decode(list of id lists) -> keep the ids
        @staticmethod
        def decode(lists):
            return [list(map(int, l)) for l in lists]
    obj.tokenizer = _Ids()
    object.__setattr__(obj, "encoder", lambda x, x_len: (f, f_len, None))
    obj.eval()
    with torch.no_grad():
        return obj.gready_search_decoding(torch.zeros(f.shape[0], 1), f_len)


def to_torch(sd):
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


def run_encoder(enc_mod, name, mel, lens, seed, hooks=False, extra=None):
    """Reference ConformerEncoder driven from mel (encoders.py:107-140) + fc head.  extra: encoder_params overrides (causal / contexts)."""
    cfg = named_config(name)
    if extra:
        cfg["encoder_params"] = dict(cfg["encoder_params"], **extra)
    plan = build_plan(cfg["encoder_params"])
    vocab = cfg["tokenizer_params"]["vocab_size"]
    sd = synth.make_state_dict(plan, seed, vocab)
    model = enc_mod.ConformerEncoder(cfg["encoder_params"]).eval()
    missing = model.load_state_dict(to_torch({k: v for k, v in sd.items() if not k.startswith("fc.")}), strict=True)
    fc = nn.Linear(plan.dim_out, vocab).eval()
    fc.load_state_dict({"weight": torch.from_numpy(sd["fc.weight"]), "bias": torch.from_numpy(sd["fc.bias"])})
    trace = {}
    handles = []
    if hooks:
        def grab(key):
            def fn(mod, inp, out):
                trace[key] = (out[0] if isinstance(out, tuple) else out).detach().clone()
            return fn
        handles.append(model.subsampling_module.register_forward_hook(grab("subsample")))
        handles.append(model.linear.register_forward_hook(grab("linear")))
        for i, blk in enumerate(model.blocks):
            p = "blocks.%d" % i
            handles.append(blk.feed_forward_module1.register_forward_hook(grab(p + ".ffn1")))
            handles.append(blk.multi_head_self_attention_module.register_forward_hook(grab(p + ".mhsa")))
            handles.append(blk.convolution_module.register_forward_hook(grab(p + ".conv")))
            handles.append(blk.feed_forward_module2.register_forward_hook(grab(p + ".ffn2")))
            handles.append(blk.register_forward_hook(grab(p + ".out")))
    model.preprocessing.forward = lambda x, l: (x, l)      # frontend lives in torchaudio (absent): start from mel
    with torch.no_grad():
        x, out_len, atts = model(torch.from_numpy(mel), torch.from_numpy(lens))
        logits = fc(x)
    for h in handles:
        h.remove()
    return plan, x, out_len, logits, atts, trace


def _stub_third_party():
    for n, attrs in (("jiwer", ()), ("kenlm", ()), ("warp_rnnt", ("rnnt_loss",)), ("ctcdecode", ("CTCBeamDecoder",)),
                     ("torch.utils.tensorboard", ("SummaryWriter",)), ("sentencepiece", ("SentencePieceProcessor", "SentencePieceTrainer"))):
        if n not in sys.modules or n == "sentencepiece":
            m = types.ModuleType(n)
            for a in attrs:
                setattr(m, a, object)
            sys.modules.setdefault(n, m)


def greedy_reference(logits, lens):
    """The reference's OWN greedy method (models/model_ctc.py:90-136), called as imported: a stand-in `self` whose encoder returns the
    given logits, whose fc is the identity and whose tokenizer keeps the id lists."""
    _stub_third_party()
    import models.model_ctc as mc
    fake = types.SimpleNamespace(encoder=lambda x, x_len: (x, x_len, None), fc=lambda x: x,
                                 tokenizer=types.SimpleNamespace(decode=lambda lists: [list(map(int, l)) for l in lists]))
    with torch.no_grad():
        return mc.ModelCTC.gready_search_decoding(fake, logits, lens)


def pack_labels(lists):
    flat = np.asarray([t for l in lists for t in l], dtype=np.int32)
    offs = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    return flat, offs


def margins(logits):
    top2 = logits.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]).numpy().astype(np.float32)


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def rnnt_goldens(enc_mod):
    """RNN-T greedy decode (BASELINE.json configs[3]): the reference encoder's own output f -> the reference's greedy
    token lists, for purely random joint weights (blank almost never wins: the max_consec_dec_step rule fires on every
    frame) and with a boosted blank bias (trained-model-like token rate)."""
    for name, tm, lens, seed in (("TinyTransducer", 100, [100, 77, 52, 9], 7), ("EfficientConformerTransducerMedium", 1001, [1001, 640], 0)):
        cfg = named_config(name)
        mel, ln = synth.make_mel(len(lens), 80, tm, lens, seed=4321)
        plan, f, f_len, _, _, _ = run_encoder(enc_mod, name, mel, ln, seed=seed)
        arrs = {"mel_seed": np.int64(4321), "weight_seed": np.int64(seed), "mel_len": ln, "f": f.numpy(), "f_len": f_len.numpy()}
        for tag, bb in (("rand", 0.0), ("blank", 1.2)):
            sd = synth.make_transducer_state_dict(plan.dim_out, cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=bb)
            toks = reference_rnnt_greedy(f, f_len, cfg["decoder_params"], cfg["joint_params"], sd)
            flat, offs = pack_labels(toks)
            arrs["tokens_" + tag], arrs["offsets_" + tag], arrs["blank_bias_" + tag] = flat, offs, np.float32(bb)
            print("  %s/%s: tokens per utterance %s (frames %s)" % (name, tag, [len(t) for t in toks], f_len.tolist()))
        save("rnnt_" + name, **arrs)


def reference_rnnt_beam(f, f_len, dec_params, joint_params, sd, beam_size, lm=None, lm_weight=0, lm_tmp=1):
    """Execute the reference's own Transducer.beam_search_decoding (transducer.py:188-327) on given encoder outputs, in the state of a
    plain checkpoint load: no n-gram file (ngram_path None) and no LM (lm None, lm_weight 0), temperature 1 - or with `lm` (reference_lm)
    attached as Model.lm, lm_weight and lm_tmp as decoding_params set them (model.py:70-72)."""
    _stub_third_party()
    import models.transducer as tr
    import models.decoders as dec
    import models.joint_networks as jn
    obj = tr.Transducer.__new__(tr.Transducer)
    nn.Module.__init__(obj)
    obj.decoder = dec.RnnDecoder(dec_params).eval()
    obj.joint_network = jn.JointNetwork(f.shape[-1], dec_params["dim_model"], dec_params["vocab_size"], joint_params).eval()
    obj.decoder.load_state_dict(to_torch({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}), strict=True)
    obj.joint_network.load_state_dict(to_torch({k[len("joint_network."):]: v for k, v in sd.items() if k.startswith("joint_network.")}), strict=True)
    obj.beam_size, obj.tmp, obj.ngram_path, obj.lm, obj.lm_weight, obj.lm_tmp = beam_size, 1, None, lm, lm_weight, lm_tmp

    class _Ids:                                   # tokenizer.decode(one id list per utterance) -> keep the ids
        @staticmethod
        def decode(ids):
            return list(map(int, ids))
    obj.tokenizer = _Ids()
    object.__setattr__(obj, "encoder", lambda x, x_len: (f, f_len, None))
    obj.eval()
    with torch.no_grad():
        return obj.beam_search_decoding(torch.zeros(f.shape[0], 1), f_len)


def rnnt_beam_goldens():
    """RNN-T beam search: the reference's own beam_search_decoding on the encoder outputs stored in rnnt_<name>.npz (blank bias 1.2).
    Only beams the reference terminates on: Tiny at beam 1 and Medium at beam 4 never see blank in the top of the popped hypothesis
    in some frame, and the reference's loop (transducer.py:237) runs forever there."""
    for name, beams in (("TinyTransducer", (4, 16)), ("EfficientConformerTransducerMedium", (16,))):
        cfg = named_config(name)
        g = np.load(os.path.join(OUT, "rnnt_%s.npz" % name))
        f, f_len, seed, bb = torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"]), int(g["weight_seed"]), 1.2
        sd = synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=bb)
        arrs = {"weight_seed": np.int64(seed), "blank_bias": np.float32(bb), "beams": np.asarray(beams, dtype=np.int32)}
        for beam in beams:
            toks = reference_rnnt_beam(f, f_len, cfg["decoder_params"], cfg["joint_params"], sd, beam)
            arrs["tokens_b%d" % beam], arrs["offsets_b%d" % beam] = pack_labels(toks)
            print("  %s beam %d: tokens per utterance %s (frames %s)" % (name, beam, [len(t) for t in toks], f_len.tolist()))
        save("rnnt_beam_" + name, **arrs)


RNNT_BEAM_LM = dict(blank_bias=2.0, lm_weight=0.3, lm_tmp=1.0)


def rnnt_beam_lm_goldens():
    """RNN-T beam search with neural-LM shallow fusion: the reference's own beam_search_decoding with its LanguageModel (TinyLM of lm_TinyLM.npz: weight seed
    and fc bias) attached, on the encoder outputs stored in rnnt_TinyTransducer.npz.  Blank bias 2.0: at 1.2 the LM's mass on token 0 keeps blank out of
    the top of the popped hypothesis at beam 4 and the reference's loop does not end."""
    name, beams = "TinyTransducer", (4, 16)
    cfg = named_config(name)
    g = np.load(os.path.join(OUT, "rnnt_%s.npz" % name))
    gl = np.load(os.path.join(OUT, "lm_TinyLM.npz"))
    lm_params = dict(LM_MODELS[0][1])
    lm_sd = synth.make_lm_state_dict(lm_params, int(gl["weight_seed"]), bias=gl["fc_bias_extra"])
    f, f_len, seed = torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"]), int(g["weight_seed"])
    sd = synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=RNNT_BEAM_LM["blank_bias"])
    arrs = {"weight_seed": np.int64(seed), "blank_bias": np.float32(RNNT_BEAM_LM["blank_bias"]), "beams": np.asarray(beams, dtype=np.int32),
            "lm_weight": np.float64(RNNT_BEAM_LM["lm_weight"]), "lm_tmp": np.float64(RNNT_BEAM_LM["lm_tmp"]),
            "lm_weight_seed": np.int64(gl["weight_seed"]), "fc_bias_extra": gl["fc_bias_extra"]}
    for beam in beams:
        toks = reference_rnnt_beam(f, f_len, cfg["decoder_params"], cfg["joint_params"], sd, beam, reference_lm(lm_params, lm_sd, False),
                                   RNNT_BEAM_LM["lm_weight"], RNNT_BEAM_LM["lm_tmp"])
        arrs["tokens_b%d" % beam], arrs["offsets_b%d" % beam] = pack_labels(toks)
        print("  %s + TinyLM beam %d: tokens per utterance %s (frames %s)" % (name, beam, [len(t) for t in toks], f_len.tolist()))
    save("rnnt_beam_lm_" + name, **arrs)


RNNT_LATTICE = (("TinyTransducer", (5, 0, 9, 3), 501), ("EfficientConformerTransducerMedium", (17, 30), 502))


def rnnt_lattice_targets(name):
    """The fixed transcripts of the lattice goldens: token ids 1 .. V - 1 from a seeded generator, padded with 0."""
    cfg = named_config(name)
    lens, seed = next((l, s) for n, l, s in RNNT_LATTICE if n == name)
    rng = np.random.default_rng(seed)
    y = np.zeros((len(lens), max(lens)), dtype=np.int32)
    for i, u in enumerate(lens):
        y[i, :u] = rng.integers(1, cfg["decoder_params"]["vocab_size"], u)
    return y, np.asarray(lens, dtype=np.int64), seed


def rnnt_lattice_goldens():
    """RNN-T lattice: the reference's own RnnDecoder and JointNetwork run as Transducer.forward runs them (transducer.py:96-104: y padded
    with the start token, the decoder over the packed (B, U + 1) batch, the joint network's (B, T, U + 1, V) logits) on the encoder outputs
    stored in rnnt_<name>.npz (blank bias 1.2), reduced with log_softmax to the two fp32 planes the RNN-T loss reads: column 0 and column
    y[u] of every cell.  Outside an utterance's rectangle the planes are 0; lp_label is -inf at u = U."""
    _stub_third_party()
    import models.decoders as dec
    import models.joint_networks as jn
    for name, _, _ in RNNT_LATTICE:
        cfg = named_config(name)
        g = np.load(os.path.join(OUT, "rnnt_%s.npz" % name))
        f, f_len, seed, bb = torch.from_numpy(g["f"]), torch.from_numpy(g["f_len"]), int(g["weight_seed"]), 1.2
        sd = synth.make_transducer_state_dict(f.shape[-1], cfg["decoder_params"], cfg["joint_params"], seed, blank_bias=bb)
        decoder = dec.RnnDecoder(cfg["decoder_params"]).eval()
        joint = jn.JointNetwork(f.shape[-1], cfg["decoder_params"]["dim_model"], cfg["decoder_params"]["vocab_size"], cfg["joint_params"]).eval()
        decoder.load_state_dict(to_torch({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}), strict=True)
        joint.load_state_dict(to_torch({k[len("joint_network."):]: v for k, v in sd.items() if k.startswith("joint_network.")}), strict=True)
        y, y_len, tseed = rnnt_lattice_targets(name)
        with torch.no_grad():
            yp = torch.nn.functional.pad(torch.from_numpy(y).long(), pad=(1, 0, 0, 0), value=0)
            gg, _ = decoder(yp, None, torch.from_numpy(y_len) + 1)
            lp = torch.log_softmax(joint(f, gg), dim=-1)                      # (B, T, U + 1, V)
        b, t, e = lp.shape[:3]
        lpb, lpl = np.zeros((b, t, e), dtype=np.float32), np.zeros((b, t, e), dtype=np.float32)
        for i in range(b):
            n, u = int(f_len[i]), int(y_len[i])
            lpb[i, :n, :u + 1] = lp[i, :n, :u + 1, 0].numpy()
            lpl[i, :n, u] = -np.inf
            for k in range(u):
                lpl[i, :n, k] = lp[i, :n, k, int(y[i, k])].numpy()
        print("  %s: frames %s, tokens %s" % (name, f_len.tolist(), y_len.tolist()))
        save("rnnt_lattice_" + name, weight_seed=np.int64(seed), blank_bias=np.float32(bb), target_seed=np.int64(tseed), targets=y,
             target_len=y_len, f_len=f_len.numpy(), lp_blank=lpb, lp_label=lpl)


LM_MODELS = (("TinyLM", dict(arch="RNN", vocab_size=40, dim_model=32, num_layers=2), 11, (12, 0, 1, 2, 7, 12), 601),
             ("LM257", dict(arch="RNN", vocab_size=257, dim_model=48, num_layers=3), 12, (9, 0, 1, 2, 5), 602))
LM_RESCORE_WEIGHT = 0.5          # lm_weight of the rescoring test (tests/test_gpu_lm.py)


def reference_lm(lm_params, sd, double):
    """The reference's LanguageModel around its own RnnDecoder and an nn.Linear (without Model.__init__: no tokenizer file, optimizer or loss
    here); its real ``forward`` and ``decode`` methods are called."""
    _stub_third_party()
    import models.decoders as dec
    import models.lm as lm
    obj = lm.LanguageModel.__new__(lm.LanguageModel)
    nn.Module.__init__(obj)
    obj.decoder = dec.RnnDecoder(lm_params)
    obj.fc = nn.Linear(lm_params["dim_model"], lm_params["vocab_size"])
    if sd is not None:
        obj.load_state_dict(to_torch(sd), strict=True)
    obj.eval()
    return obj.double() if double else obj


def _lm_rescore_bias(lm_params, seed):
    """An fc bias for TinyLM under which n-best rescoring of the Tiny CTC goldens' logits (beam 16, lm_weight LM_RESCORE_WEIGHT) moves the winner of at
    least two utterances and keeps rank 0 in at least two, every decision by more than 0.05: tests/ctc_beam_ref.py + tests/lm_ref.py on the CPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctc_beam_ref
    import lm_ref
    nbest = []
    for tm in (100, 47):
        g = np.load(os.path.join(OUT, "tiny_T%d.npz" % tm))
        for i in range(g["logits"].shape[0]):
            r = ctc_beam_ref.beam_search(ctc_beam_ref.logp32(g["logits"][i]), int(g["out_len"][i]), 16)
            nbest.append((r["prefixes"], r["score"]))
    for trial in range(200):
        rng = np.random.Generator(np.random.PCG64(7000 + trial))
        bias = (2.0 * rng.standard_normal(lm_params["vocab_size"])).astype(np.float32)
        sd = synth.make_lm_state_dict(lm_params, seed, bias=bias)
        best, margin = [], []
        for prefixes, am in nbest:
            u = max(len(p) for p in prefixes)
            y = np.zeros((len(prefixes), max(u, 1)), dtype=np.int64)
            for k, p in enumerate(prefixes):
                y[k, :len(p)] = p
            _, lms, _ = lm_ref.token_logprobs(sd, y, [len(p) for p in prefixes])
            total = np.where(np.isfinite(am), am + LM_RESCORE_WEIGHT * lms, -np.inf)
            order = np.argsort(-total, kind="stable")
            best.append(int(order[0]))
            margin.append(total[order[0]] - total[order[1]])
        moved, kept = sum(b != 0 for b in best), sum(b == 0 for b in best)
        if moved >= 2 and kept >= 2 and min(margin) > 0.05:
            print("  rescoring bias: trial %d, winners %s, smallest decision %.3f" % (trial, best, min(margin)))
            return bias, np.asarray(best, dtype=np.int64)
    sys.exit("make_goldens: no rescoring bias found")


def lm_goldens():
    """LSTM language model: the reference's own RnnDecoder + nn.Linear as LanguageModel.forward and .decode run them (lm.py:55-81), in fp32 and in
    float64 (.double()), on synthetic weights.  Also the state-dict keys and shapes of the reference's LanguageModel for configs/LM-RNN.json
    (built on the meta device: no 1.4 GB of weights), as bytes and integers."""
    import json
    with torch.device("meta"):
        big = reference_lm(json.load(open(os.path.join(REF, "configs", "LM-RNN.json")))["lm_params"], None, False)
    keys = list(big.state_dict().keys())
    shapes = np.zeros((len(keys), 2), dtype=np.int64)
    for i, k in enumerate(keys):
        shp = tuple(big.state_dict()[k].shape)
        shapes[i, :len(shp)] = shp
    for name, params, seed, lens, tseed in LM_MODELS:
        arrs = {"weight_seed": np.int64(seed), "token_seed": np.int64(tseed), "vocab_size": np.int64(params["vocab_size"]),
                "dim_model": np.int64(params["dim_model"]), "num_layers": np.int64(params["num_layers"]),
                "lmrnn_keys": np.frombuffer("\n".join(keys).encode(), dtype=np.uint8), "lmrnn_shapes": shapes}
        bias = None
        if name == "TinyLM":
            bias, best = _lm_rescore_bias(params, seed)
            arrs["fc_bias_extra"], arrs["rescore_best_rank"], arrs["rescore_lm_weight"] = bias, best, np.float64(LM_RESCORE_WEIGHT)
        sd = synth.make_lm_state_dict(params, seed, bias=bias)
        rng = np.random.default_rng(tseed)
        y = np.zeros((len(lens), max(lens)), dtype=np.int64)
        for i, u in enumerate(lens):
            y[i, :u] = rng.integers(1, params["vocab_size"], u)
        walk = rng.integers(0, params["vocab_size"], (5, 3))
        arrs["tokens"], arrs["token_len"], arrs["walk_tokens"] = y.astype(np.int32), np.asarray(lens, dtype=np.int64), walk.astype(np.int32)
        for tag, double in (("f32", False), ("f64", True)):
            m = reference_lm(params, sd, double)
            with torch.no_grad():
                arrs["logits_" + tag] = m.forward((torch.from_numpy(y), torch.from_numpy(arrs["token_len"]), None)).numpy()
                hidden, steps = None, []
                for k in range(walk.shape[0]):
                    lg, hidden = m.decode(torch.from_numpy(walk[k])[:, None], hidden)
                    steps.append(lg[:, 0].numpy())
            arrs["walk_logits_" + tag] = np.stack(steps)
            arrs["walk_h_" + tag], arrs["walk_c_" + tag] = hidden[0].numpy(), hidden[1].numpy()
        save("lm_" + name, **arrs)


STREAMING = (("causal", dict(causal=True)), ("ctx_l20_r4", dict(left_context=20, right_context=4)),
             ("causal_l12", dict(causal=True, left_context=12)), ("ctx_l3_r0", dict(left_context=3, right_context=0)))


def streaming_goldens(enc_mod):
    """Streaming / causal contexts (reference encoders.py:68, 94; attentions.py:1377-1403, 506; layers.py:94-101): the reference encoder
    with `causal` and finite `left_context` / `right_context`, tiny config (both sequence lengths) and EfficientConformerCTCSmall."""
    for tag, extra in STREAMING:
        for tm, lens in ((47, [47, 40, 23]), (100, [100, 77, 52])):
            mel, ln = synth.make_mel(3, 80, tm, lens, seed=4321 + tm)
            plan, x, out_len, logits, atts, _ = run_encoder(enc_mod, "Tiny", mel, ln, seed=7, extra=extra)
            lab, offs = pack_labels(greedy_reference(logits, out_len))
            save("stream_tiny_%s_T%d" % (tag, tm), mel_seed=np.int64(4321 + tm), weight_seed=np.int64(7), mel_len=ln, out=x.numpy(),
                 out_len=out_len.numpy(), labels=lab, label_offsets=offs, **{"cfg/" + k: np.int64(v) for k, v in extra.items()})
    for tag, extra in (("causal", dict(causal=True)), ("ctx_l64_r16", dict(left_context=64, right_context=16))):
        mel, ln = synth.make_mel(2, 80, 601, [601, 433], seed=4321)
        plan, x, out_len, logits, atts, _ = run_encoder(enc_mod, "EfficientConformerCTCSmall", mel, ln, seed=0, extra=extra)
        save("stream_small_%s" % tag, mel_seed=np.int64(4321), weight_seed=np.int64(0), mel_len=ln, out_rows=x[:, ::4].numpy(),
             out_len=out_len.numpy(), argmax=logits.argmax(-1).numpy().astype(np.int16), margin=margins(logits),
             **{"cfg/" + k: np.int64(v) for k, v in extra.items()})


def interctc_goldens(enc_mod):
    """Self-conditioned CTC: the reference's own ConformerEncoderInterCTC (encoders.py:144-215) driven from mel on Tiny with interctc_blocks = [1, 3, 5]
    (both transition blocks and the last block) and vocabulary 32, the two batches of tiny_T*.npz, weight seed 7, in the two weight recipes of
    tests/interctc_ref.py (flat: the key-seeded tensors; peaky: confident rows, p.max() = 1).  Arrays and key names only."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import interctc_ref as IR
    params = IR.tiny_params()
    plan = build_plan(params, interctc=True)
    for recipe in IR.RECIPES:
        sd = IR.tiny_state_dict(recipe)
        for tm, lens in IR.BATCHES:
            mel, ln = IR.tiny_mel(tm, lens)
            model = enc_mod.ConformerEncoderInterCTC(dict(params)).eval()
            model.load_state_dict(to_torch({k: v for k, v in sd.items() if not k.startswith("fc.")}), strict=True)
            keys = sorted(model.state_dict().keys())
            fc = nn.Linear(plan.dim_out, IR.TINY_VOCAB).eval()
            fc.load_state_dict({"weight": torch.from_numpy(sd["fc.weight"]), "bias": torch.from_numpy(sd["fc.bias"])})
            model.preprocessing.forward = lambda x, l: (x, l)      # frontend lives in torchaudio (absent): start from mel
            with torch.no_grad():
                x, out_len, _, probs = model(torch.from_numpy(mel), torch.from_numpy(ln))
                logits = fc(x)
            lab, offs = pack_labels(greedy_reference(logits, out_len))
            arrs = {"mel_seed": np.int64(4321 + tm), "weight_seed": np.int64(IR.WEIGHT_SEED), "mel_len": ln, "vocab_size": np.int64(IR.TINY_VOCAB),
                    "interctc_blocks": np.asarray(IR.TINY_BLOCKS, dtype=np.int64), "out": x.numpy(), "out_len": out_len.numpy(), "logits": logits.numpy(),
                    "labels": lab, "label_offsets": offs, "state_dict_keys": np.frombuffer("\n".join(keys).encode(), dtype=np.uint8)}
            for k, p in zip(IR.TINY_BLOCKS, probs):
                arrs["probs_%d" % k] = p.numpy()
            pmax, pmin = max(float(p.max()) for p in probs), min(float(p.min()) for p in probs)
            print("  %s T%d: p.max %.6g p.min %.3g, labels per utterance %s" % (recipe, tm, pmax, pmin, np.diff(offs).tolist()))
            save("interctc_tiny_%s_T%d" % (recipe, tm), **arrs)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    enc_mod, att_mod = import_reference()
    if "--only-interctc" in sys.argv:
        return interctc_goldens(enc_mod)
    if "--only-rnnt" in sys.argv:
        return rnnt_goldens(enc_mod)
    if "--only-rnnt-beam" in sys.argv:
        return rnnt_beam_goldens()
    if "--only-rnnt-beam-lm" in sys.argv:
        return rnnt_beam_lm_goldens()
    if "--only-rnnt-lattice" in sys.argv:
        return rnnt_lattice_goldens()
    if "--only-lm" in sys.argv:
        return lm_goldens()
    if "--only-streaming" in sys.argv:
        return streaming_goldens(enc_mod)
    rnnt_goldens(enc_mod)
    rnnt_beam_goldens()
    rnnt_lattice_goldens()
    streaming_goldens(enc_mod)
    interctc_goldens(enc_mod)
    # lm_goldens() reads tiny_T*.npz: after section 1 below (or --only-lm on stored ones)

    # ---- 1. tiny config: every module output, two sequence lengths (T1 % 3 == 0 and != 0)
    for tm, lens in ((47, [47, 40, 23]), (100, [100, 77, 52])):
        mel, ln = synth.make_mel(3, 80, tm, lens, seed=4321 + tm)
        plan, x, out_len, logits, atts, trace = run_encoder(enc_mod, "Tiny", mel, ln, seed=7, hooks=True)
        arrs = {"mel_seed": np.int64(4321 + tm), "weight_seed": np.int64(7), "mel_len": ln,
                "out": x.numpy(), "out_len": out_len.numpy(), "logits": logits.numpy(),
                "att0": atts[0].numpy(), "att_last": atts[-1].numpy()}
        for k, v in trace.items():
            arrs["trace/" + k] = v.numpy()
        lab, offs = pack_labels(greedy_reference(logits, out_len))
        arrs["labels"], arrs["label_offsets"] = lab, offs
        save("tiny_T%d" % tm, **arrs)
    lm_goldens()
    rnnt_beam_lm_goldens()                                   # reads lm_TinyLM.npz

    # ---- 2. EfficientConformerCTCSmall, B=4, Tm=1001, ragged
    mel, ln = synth.make_mel(4, 80, 1001, [1001, 900, 800, 700], seed=4321)
    plan, x, out_len, logits, atts, _ = run_encoder(enc_mod, "EfficientConformerCTCSmall", mel, ln, seed=0)
    lab, offs = pack_labels(greedy_reference(logits, out_len))
    save("small_B4_T1001", mel_seed=np.int64(4321), weight_seed=np.int64(0), mel_len=ln,
         out=x.numpy(), out_len=out_len.numpy(), argmax=logits.argmax(-1).numpy().astype(np.int16),
         margin=margins(logits), labels=lab, label_offsets=offs,
         logits_sample=logits[:, ::8].numpy())

    # ---- 3. other BASELINE.json configs: sampled rows + labels + margins (B=2, ragged)
    for name, tm, lens in (("EfficientConformerCTCMedium", 1001, [1001, 640]),
                           ("EfficientConformerCTCLarge", 1001, [1001, 640]),
                           ("EfficientConformerTransducerMedium", 1001, [1001, 640]),
                           ("ConformerCTCLarge", 501, [501, 333])):
        mel, ln = synth.make_mel(2, 80, tm, lens, seed=4321)
        plan, x, out_len, logits, atts, _ = run_encoder(enc_mod, name, mel, ln, seed=0)
        lab, offs = pack_labels(greedy_reference(logits, out_len))
        save(name + "_B2", mel_seed=np.int64(4321), weight_seed=np.int64(0), mel_len=ln,
             out_rows=x[:, ::8].numpy(), out_sum=np.float64(x.double().sum().item()),
             out_abssum=np.float64(x.double().abs().sum().item()), out_len=out_len.numpy(),
             argmax=logits.argmax(-1).numpy().astype(np.int16), margin=margins(logits),
             labels=lab, label_offsets=offs)

    # ---- 4. op-level: the reference's attention classes on their own (closed-form pin)
    for group, t, lens in ((1, 47, [47, 30]), (3, 47, [47, 31]), (3, 48, [48, 9]), (1, 126, [126, 88]), (3, 250, [250, 101])):
        dim, heads = 48, 4
        g = np.random.Generator(np.random.PCG64(1000 + 10 * t + group))
        xin = g.standard_normal((2, t, dim)).astype(np.float32)
        keys = [("u", (dim,), "uv"), ("v", (dim,), "uv")]
        for n in ("query_layer", "key_layer", "value_layer", "output_layer", "pos_layer"):
            keys += [(n + ".weight", (dim, dim), "weight"), (n + ".bias", (dim,), "bias")]
        sd = {k: synth.make_tensor("att." + k, s, kind, 3) for k, s, kind in keys}
        if group > 1:
            mod = att_mod.GroupedRelPosMultiHeadSelfAttention(dim, heads, False, 600, group).eval()
        else:
            mod = att_mod.RelPosMultiHeadSelfAttention(dim, heads, False, 600).eval()
        mod.load_state_dict(to_torch(sd), strict=True)
        ln = torch.tensor(lens)
        mask = att_mod.StreamingMask(600, 600)(torch.zeros(2, 1, t), ln)
        with torch.no_grad():
            xt = torch.from_numpy(xin)
            o, w, _ = mod(xt, xt, xt, mask)
        arrs = {"x": xin, "lens": np.asarray(lens, dtype=np.int64), "out": o.numpy(), "probs": w.numpy(),
                "group": np.int64(group), "heads": np.int64(heads)}
        arrs.update({"w/" + k: v for k, v in sd.items()})
        save("att_G%d_T%d" % (group, t), **arrs)


if __name__ == "__main__":
    main()
