"""A dry run of the packing (effconf_debug_pack_digest, tests/test_pack_host.py) leaves no trace on the handle: a handle that was dry-run and then finalized
computes what a handle that was only finalized computes, bit for bit."""
import importlib.util
import os

import pytest
import torch

from efficientconformer_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pack_digest", os.path.join(ROOT, "tools", "pack_digest.py"))
pack_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digest)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_finalize_after_a_dry_run_equals_finalize_alone(precision):
    """Tiny, B = 2 (lengths 64 and 50 of 64 mel frames): effconf_encoder_forward_mel through the C ABI on both handles, torch.equal outputs and lengths."""
    lib = _lib.load_debug()
    plan, vocab, sd = pack_digest.state_dict("Tiny")
    batch, tm = 2, 64
    mel_np, lens_np = synth.make_mel(batch, plan.n_mels, tm, lengths=[64, 50])
    mel, lens = torch.from_numpy(mel_np).cuda().contiguous(), torch.from_numpy(lens_np).cuda()
    outs = []
    for dry in (True, False):
        h = pack_digest.create(lib, plan, vocab, precision, sd)
        try:
            if dry:
                assert pack_digest.dry_run(lib, h)[0] == 0, lib.effconf_last_error()
            _lib.check(lib.effconf_encoder_finalize(h), "finalize", lib)
            t_out = lib.effconf_encoder_out_frames(h, tm, 0)
            out = torch.zeros(batch, t_out, plan.dim_out, dtype=torch.float32, device="cuda")
            out_len = torch.zeros(batch, dtype=torch.int64, device="cuda")
            ws = torch.empty(lib.effconf_encoder_workspace_bytes(h, batch, tm, 0), dtype=torch.uint8, device="cuda")
            _lib.check(lib.effconf_encoder_forward_mel(h, mel.data_ptr(), lens.data_ptr(), batch, tm, out.data_ptr(), out_len.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       torch.cuda.current_stream().cuda_stream), "forward_mel", lib)
            torch.cuda.synchronize()
            outs.append((out.cpu(), out_len.cpu()))
        finally:
            lib.effconf_encoder_destroy(h)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0][0]).all()) and float(outs[0][0][0].abs().max()) > 0 and int(outs[0][1][0]) == outs[0][0].shape[1]
