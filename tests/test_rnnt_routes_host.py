"""Which kernel the greedy RNN-T decode runs (effconf_rnnt_greedy_route, csrc/rnnt.hip greedy_route) against a hand-written table: 0 one
workgroup per utterance, 1 clusters of 8 workgroups x 8 utterances x 2 frames, 2 clusters of 16 x 16 x 1.  The entry needs neither
finalize nor a device.

The rules the table is written from (include/effconf.h):
  a cluster shape needs H % 64 == 0, J % 64 == 0, at most 128 vocabulary entries per workgroup (V <= 1024 with 8 workgroups, 2048 with 16), at most
    512 gate rows per workgroup (H <= 1024 with 8, 2048 with 16) and its state in 159.5 KB of LDS: 8 x 8 x 2 takes (8 H + 24 J + 5 H + 256) x 4 B,
    16 x 16 x 1 (16 H + 32 J + 5 H + 256) x 4 B;
  cluster_decode 0 never clusters; -1 (auto) needs two full clusters' worth of utterances (16 / 32) and at most 256 workgroups (128 with
    cluster_by_slice = 0); 1 forces whatever the batch (16 x 16 x 1: at most 256 workgroups);
  cluster_shape 1 asks for 16 x 16 x 1 first, and where that does not run decides as cluster_shape 0 does."""
import ctypes as C

import pytest

from efficientconformer_amd import _lib

TINY = (48, 32, 32, 40)
MEDIUM = (360, 640, 640, 1000)
A_ONLY = (360, 832, 832, 1000)        # 16 x 16 x 1 needs (21 x 832 + 32 x 832 + 256) x 4 = 177 KB of LDS, 8 x 8 x 2 (13 x 832 + 24 x 832 + 256) x 4 = 124 KB
B_ONLY = (360, 640, 640, 1500)        # 188 vocabulary entries per workgroup of 8, 94 per workgroup of 16
NOT64 = (40, 96, 128, 100)            # H % 64 != 0

# (config, cluster_decode, cluster_shape, cluster_by_slice, batch) -> route
TABLE = [
    # Tiny: H = J = 32, no cluster shape under any option
    (TINY, -1, 0, 1, 19, 0), (TINY, -1, 1, 1, 64, 0), (TINY, 1, 0, 1, 19, 0), (TINY, 1, 1, 1, 19, 0), (TINY, 1, 0, 0, 19, 0), (TINY, 0, 0, 1, 19, 0),
    (NOT64, 1, 0, 1, 64, 0), (NOT64, 1, 1, 1, 64, 0),
    # Medium, auto, 8 x 8 x 2: from 16 utterances, up to 256 workgroups (by slice) or 128 (by cluster)
    (MEDIUM, -1, 0, 1, 1, 0), (MEDIUM, -1, 0, 1, 15, 0), (MEDIUM, -1, 0, 1, 16, 1), (MEDIUM, -1, 0, 1, 31, 1), (MEDIUM, -1, 0, 1, 32, 1),
    (MEDIUM, -1, 0, 1, 256, 1), (MEDIUM, -1, 0, 1, 257, 0),
    (MEDIUM, -1, 0, 0, 128, 1), (MEDIUM, -1, 0, 0, 129, 0), (MEDIUM, -1, 0, 0, 256, 0),
    (MEDIUM, -1, -1, 1, 64, 1),                                        # cluster_shape -1 is 0
    # Medium, auto, 16 x 16 x 1 asked: from 32 utterances; below that the 8 x 8 x 2 decision
    (MEDIUM, -1, 1, 1, 15, 0), (MEDIUM, -1, 1, 1, 16, 1), (MEDIUM, -1, 1, 1, 31, 1), (MEDIUM, -1, 1, 1, 32, 2), (MEDIUM, -1, 1, 1, 256, 2),
    (MEDIUM, -1, 1, 1, 257, 0),
    (MEDIUM, -1, 1, 0, 128, 2), (MEDIUM, -1, 1, 0, 129, 0),
    # Medium, forced
    (MEDIUM, 1, 0, 1, 1, 1), (MEDIUM, 1, 0, 1, 15, 1), (MEDIUM, 1, 0, 1, 256, 1), (MEDIUM, 1, 0, 0, 256, 1),
    (MEDIUM, 1, 1, 1, 1, 2), (MEDIUM, 1, 1, 1, 15, 2), (MEDIUM, 1, 1, 1, 256, 2), (MEDIUM, 1, 1, 0, 256, 2),
    (MEDIUM, 1, 0, 1, 257, 1), (MEDIUM, 1, 1, 1, 257, 1),              # the launch refuses these (batch <= 256): never a quiet per-utterance decode
    # cluster_decode 0
    (MEDIUM, 0, 0, 1, 64, 0), (MEDIUM, 0, 1, 1, 64, 0), (A_ONLY, 0, 0, 1, 64, 0), (B_ONLY, 0, 1, 1, 64, 0),
    # 8 x 8 x 2 only: cluster_shape 1 falls back to it (the advisor's case)
    (A_ONLY, -1, 0, 1, 64, 1), (A_ONLY, -1, 1, 1, 64, 1), (A_ONLY, 1, 1, 1, 20, 1), (A_ONLY, 1, 0, 1, 20, 1), (A_ONLY, -1, 1, 1, 15, 0),
    # 16 x 16 x 1 only: 8 x 8 x 2 is refused, so cluster_shape 0 decodes per utterance
    (B_ONLY, -1, 0, 1, 64, 0), (B_ONLY, 1, 0, 1, 64, 0), (B_ONLY, -1, 1, 1, 64, 2), (B_ONLY, 1, 1, 1, 20, 2), (B_ONLY, -1, 1, 1, 31, 0),
    (B_ONLY, 1, 1, 1, 257, 0),
    # nothing to decode
    (MEDIUM, 1, 0, 1, 0, 0),
]


def _handle(lib, dims):
    h = lib.effconf_rnnt_create(C.byref(_lib.EcRnntConfig(*dims, 1, 5, 0, 0)))
    assert h, lib.effconf_last_error()
    return h


def test_route_entry_is_declared():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "effconf.h")) as fh:
        assert "effconf_rnnt_greedy_route" in fh.read()
    assert "effconf_rnnt_greedy_route" in _lib.SIGNATURES
    assert _lib.load().effconf_rnnt_greedy_route(None, 4) != 0


@pytest.mark.parametrize("dims", [TINY, NOT64, MEDIUM, A_ONLY, B_ONLY])
def test_greedy_route_table(dims):
    lib = _lib.load()
    rows = [r for r in TABLE if r[0] == dims]
    assert rows
    h = _handle(lib, dims)
    try:
        for _, mode, shape, by_slice, batch, want in rows:
            for name, value in (("cluster_decode", mode), ("cluster_shape", shape), ("cluster_by_slice", by_slice)):
                assert lib.effconf_rnnt_set_option(h, name.encode(), value) == 0
            assert lib.effconf_rnnt_greedy_route(h, batch) == want, (dims, mode, shape, by_slice, batch)
    finally:
        lib.effconf_rnnt_destroy(h)


def test_defaults_are_auto_8x8x2_by_slice():
    lib = _lib.load()
    h = _handle(lib, MEDIUM)
    try:
        assert [lib.effconf_rnnt_greedy_route(h, b) for b in (15, 16, 200, 256, 257)] == [0, 1, 1, 1, 0]
    finally:
        lib.effconf_rnnt_destroy(h)


def test_cluster_shape_outside_its_values_is_refused():
    lib = _lib.load()
    h = _handle(lib, MEDIUM)
    try:
        assert lib.effconf_rnnt_set_option(h, b"cluster_shape", 1) == 0
        for bad in (2, -2, 16):
            assert lib.effconf_rnnt_set_option(h, b"cluster_shape", bad) != 0
            assert b"cluster_shape" in lib.effconf_last_error()
        assert lib.effconf_rnnt_greedy_route(h, 64) == 2             # a refused value leaves the option as it was
        assert lib.effconf_rnnt_set_option(h, b"cluster_shape", -1) == 0 and lib.effconf_rnnt_greedy_route(h, 64) == 1
    finally:
        lib.effconf_rnnt_destroy(h)
