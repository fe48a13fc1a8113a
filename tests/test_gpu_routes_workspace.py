"""The ragged workspace holds front-end scratch for the route that runs (csrc/routes.h: front_route / front_scratch) and nothing for the others: the fused front
ends need none, the one-layer conv + GEMM route the subsampler's output rows.  EfficientConformerCTC-Small, 3 utterances of 97 / 64 / 33 mel frames."""
import ctypes as C
import hashlib
import importlib.util
import os

import pytest
import torch

from efficientconformer_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pack_digest", os.path.join(ROOT, "tools", "pack_digest.py"))
pack_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digest)

LENGTHS = [97, 64, 33]
CANARY = 1 << 20


def _al(n):
    return (n + 255) & ~255


@pytest.mark.gpu
def test_ragged_workspace_reserves_front_end_scratch_for_the_route_that_runs(monkeypatch):
    monkeypatch.setenv("EFFCONF_POISON_GUARDS", "1")          # read at effconf_encoder_create: NaN guard regions around every parameter buffer
    lib = _lib.load()
    plan, vocab, sd = pack_digest.state_dict("EfficientConformerCTCSmall")
    h = pack_digest.create(lib, plan, vocab, "bf16", sd)
    try:
        _lib.check(lib.effconf_encoder_finalize(h), "finalize", lib)
        B, n = len(LENGTHS), max(LENGTHS)
        host_len = (C.c_int64 * B)(*LENGTHS)
        size = {}
        for fuse in (0, 2, 3):
            _lib.check(lib.effconf_encoder_set_option(h, b"fuse_subsample", fuse), "set_option", lib)
            size[fuse] = lib.effconf_encoder_workspace_bytes_ragged(h, host_len, B, n, 0)
        # rows of the subsampler's output per utterance at the input's pitch, rounded up to block 0's group size; C x F/2 bf16 columns
        t1, g, c0, d0 = (n - 1) // 2 + 1, plan.blocks[0].group_size, plan.sub_filters[0], plan.blocks[0].dim_model
        sub = _al(B * (t1 + g - 1) * c0 * (plan.n_mels // 2) * 2)
        xrect = _al(B * t1 * d0 * 4)
        print("ragged workspace bytes: fuse_subsample 0 / 2 / 3 = %d / %d / %d; sub %d, xrect %d" % (size[0], size[2], size[3], sub, xrect))
        assert size[3] == size[2] > 0                   # both fused routes (sublinear3.hip, sublinear2.hip): no front-end scratch
        assert size[0] == size[2] + sub                 # conv + GEMM: the subsampler's output rows, no rectangular Linear output

        # a forward on sublinear3.hip in exactly the reported bytes = the forward in what was reserved before (output rows + rectangular Linear output on top)
        mel, lens = synth.make_mel(B, plan.n_mels, n, LENGTHS, seed=4321)
        x, dev_len = torch.from_numpy(mel).cuda(), torch.from_numpy(lens).cuda()
        frames = lib.effconf_encoder_out_frames(h, n, 0)
        stream = torch.cuda.current_stream().cuda_stream
        digests = []
        for nbytes in (size[3], size[3] + sub + xrect):
            buf = torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
            out = torch.zeros(B, frames, plan.blocks[-1].dim_expand, dtype=torch.float32, device="cuda")
            out_len = torch.zeros(B, dtype=torch.int64, device="cuda")
            rc = lib.effconf_encoder_forward_ragged(h, x.data_ptr(), dev_len.data_ptr(), host_len, B, n, 0, out.data_ptr(), frames, out_len.data_ptr(),
                                                    buf.data_ptr(), nbytes, stream)
            assert rc == 0, lib.effconf_last_error()
            torch.cuda.synchronize()
            assert bool((buf[nbytes:] == 0xA5).all()), "a kernel wrote behind the workspace"
            assert bool(torch.isfinite(out).all())
            digests.append((hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), out_len.cpu().tolist()))
        assert digests[0] == digests[1]
        assert lib.effconf_encoder_forward_ragged(h, x.data_ptr(), dev_len.data_ptr(), host_len, B, n, 0, out.data_ptr(), frames, out_len.data_ptr(),
                                                  buf.data_ptr(), size[3] - 1, stream) != 0          # one byte less is refused, not run
    finally:
        lib.effconf_encoder_destroy(h)
