"""The weight packing (csrc/pack.h, csrc/pack.hip) checked on the CPU: `effconf_debug_pack_digest` (include/effconf_debug.h) runs every packing step of
`effconf_encoder_finalize` on the loaded host tensors and hashes each buffer where `upload` would copy it to a device.  Asserted here is what does not depend
on the machine: the dry run needs no device and is deterministic, it uploads exactly the buffers the packers uploaded before they moved out of encoder.hip (count
and bytes recorded from that commit), and it leaves the handle not finalized.  Digests themselves are compared between two trees on one machine only
(tools/pack_digest.py, profiles/pack_digest_parity.txt): the sinusoid and mel tables go through libm."""
import ctypes as C
import functools
import importlib.util
import os

import pytest

from efficientconformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pack_digest", os.path.join(ROOT, "tools", "pack_digest.py"))
pack_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digest)

# (model, precision) -> (buffers, bytes) of the packers as they were inside encoder.hip (the parent of the commit that moved them), weights: the recipe of
# tests/test_gpu_exact_and_sweep.py::_model (CTC head, vocab capped at 256, seed 7).  EfficientConformerCTCLarge in split mode (1701 buffers, 1 586 994 444
# bytes) takes 5 s per dry run: it is in the parity table of profiles/pack_digest_parity.txt only.
# The split entries are that commit's minus the natural-order FFN images of the fused FFN kernel the chain kernel has since replaced (profiles/
# split_one_ffn_kernel.txt): one buffer of 2 ceil(F / 32) 64 (16 KS + 32 NT) bytes per feed-forward module of a width D in the chains' list, KS = ceil((D + 1) / 16),
# NT = ceil(D / 32), F = 4 D.  Tiny 865 - 12, 10649972 - 729088; ConformerCTCSmall 2202 - 32, 302505404 - 34603008; EfficientConformerCTCSmall 2091 - 30,
# 323482128 - 35942400; EfficientConformerCTCMedium 2055 - 21 (eleven modules at 360 have no image), 560470972 - 36126720; EfficientConformerTransducerSmall
# 2091 - 30, 251017056 - 25804800.
PARENT = {
    ("Tiny", "bf16"): (375, 5655092),
    ("Tiny", "split"): (853, 9920884),
    ("ConformerCTCSmall", "bf16"): (947, 91079292),
    ("ConformerCTCSmall", "split"): (2170, 267902396),
    ("EfficientConformerCTCSmall", "bf16"): (908, 96120272),
    ("EfficientConformerCTCSmall", "split"): (2061, 287539728),
    ("EfficientConformerCTCMedium", "bf16"): (860, 163303564),
    ("EfficientConformerCTCMedium", "split"): (2034, 524344252),
    ("EfficientConformerTransducerSmall", "bf16"): (908, 85047552),
    ("EfficientConformerTransducerSmall", "split"): (2061, 225212256),
    ("EfficientConformerCTCLarge", "bf16"): (633, 431002156),
}


@functools.lru_cache(maxsize=1)
def _weights(name):
    return pack_digest.state_dict(name)


@pytest.mark.parametrize("name,precision", sorted(PARENT))
def test_dry_run_packs_what_the_parent_packed_and_leaves_the_handle_unfinalized(name, precision):
    lib = _lib.load_debug()
    plan, vocab, sd = _weights(name)
    h = pack_digest.create(lib, plan, vocab, precision, sd)
    try:
        first = pack_digest.dry_run(lib, h)
        second = pack_digest.dry_run(lib, h)
        assert first[0] == 0, lib.effconf_last_error()
        assert first == second                                  # deterministic, and the first run left the host tensors in place
        assert first[1] != 0 and first[2:] == PARENT[(name, precision)]
        # not finalized: the sizes still answer, every entry that needs packed weights refuses before it touches a (null) device pointer
        assert lib.effconf_encoder_workspace_bytes(h, 2, 64, 0) > 0 and lib.effconf_encoder_out_frames(h, 64, 0) > 0
        refusals = [lib.effconf_encoder_forward_mel(h, None, None, 2, 64, None, None, None, 0, None),
                    lib.effconf_encoder_forward(h, None, None, 2, 16000, None, None, None, 0, None),
                    lib.effconf_encoder_forward_ragged(h, None, None, None, 2, 64, 0, None, 0, None, None, 0, None),
                    lib.effconf_mel_frontend(h, None, 2, 16000, None, None),
                    lib.effconf_ffn(h, 0, 0, None, 8, None, None, 0, None),
                    lib.effconf_conv_module(h, 0, None, 2, 8, None, None, 0, None),
                    lib.effconf_subsample(h, None, 2, 64, None, None, 0, None),
                    lib.effconf_ctc_greedy(h, None, None, 2, 8, None, None, None, None, 0, None)]
        assert all(rc != 0 for rc in refusals)
        assert lib.effconf_encoder_forward_mel(h, None, None, 2, 64, None, None, None, 0, None) != 0 and lib.effconf_last_error() == b"encoder not finalized"
    finally:
        lib.effconf_encoder_destroy(h)


def test_dry_run_reports_the_split_range_refusal_of_finalize():
    """A weight beyond the per-module split images' range: the dry run fails with finalize's error text (index and value), and again on a second run."""
    lib = _lib.load_debug()
    plan, vocab, sd = pack_digest.state_dict("Tiny", "refused")
    h = pack_digest.create(lib, plan, vocab, "split", sd)
    try:
        for _ in range(2):
            assert pack_digest.dry_run(lib, h)[0] != 0
            assert lib.effconf_last_error() == b"split mode: blocks.1.convolution_module.layers.7.weight[3][5] = 70000.000000 is outside the split images' range |w| < 65000"
        assert pack_digest.dry_run(lib, None)[0] != 0
    finally:
        lib.effconf_encoder_destroy(h)


def test_pack_digest_tool_touches_no_device():
    """tools/pack_digest.py runs with every GPU hidden and prints one JSON line per case."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_digest.py"), "Tiny:bf16", "Tiny:fp32"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert [(x["model"], x["precision"], x["buffers"], x["bytes"]) for x in rows] == [("Tiny", "bf16", 375, 5655092), ("Tiny", "fp32", rows[1]["buffers"], rows[1]["bytes"])]
    assert rows[1]["buffers"] > 375 and "error" not in rows[0] and "error" not in rows[1]
