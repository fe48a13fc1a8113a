"""Workspace sizes of the seven decoder entries, host side (no GPU): every `*_workspace_bytes` over a grid of shapes against the table
tests/golden/decoder_workspace_bytes.json, recorded from the commit before the layouts moved onto csrc/decode_layout.h's WsPlan
(`PYTHONPATH=<that checkout> python tests/test_decoder_layout_host.py --record FILE` runs the same loop there).

Six entries return that commit's value exactly.  The greedy entry had a size formula and a hand carve that disagreed (one 256-byte slack reserved, two
alignments spent); its linear_encoder region is now a planned, aligned region, so its size may grow by the padding of that region: less than 256 bytes."""
import ctypes as C
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_workspace_bytes.json")

BATCH = (0, 1, 7, 19, 256)
T_OUT = (1, 13, 250)
BEAM = (1, 4, 16)
U_MAX = (0, 5, 1023)
# (dim_encoder, dim_decoder, dim_joint, vocab): the three test shapes, Transducer-Medium's widths, and widths that are no multiple of 16 (beam / lattice refuse)
RNNT = ((48, 32, 32, 40), (48, 64, 64, 40), (48, 128, 128, 50), (360, 640, 640, 1000), (48, 40, 40, 40))
LM = ((40, 32, 1), (50, 64, 2), (1000, 1024, 4))          # (vocab, dim_model, num_layers)


def rows(lib, _lib):
    """{entry: {"args as text": bytes}}: the grid, then every refused combination the host tests of the entries name (these return 0)."""
    out = {k: {} for k in ("rnnt_greedy", "rnnt_beam", "rnnt_lattice", "rnnt_align", "lm", "ctc_beam", "ctc_align")}

    def put(entry, args, value):
        out[entry][" ".join(str(a) for a in args)] = int(value)
    for dims in RNNT:
        h = lib.effconf_rnnt_create(C.byref(_lib.EcRnntConfig(*dims, 1, 5, 0, 0)))
        assert h
        try:
            for b, t in itertools.product(BATCH, T_OUT):
                put("rnnt_greedy", dims + (b, t), lib.effconf_rnnt_workspace_bytes(h, b, t))
                for beam in BEAM:
                    put("rnnt_beam", dims + (b, t, beam, 16 * beam, 16 * t), lib.effconf_rnnt_beam_workspace_bytes(h, b, t, beam, 16 * beam, 16 * t))
                for u in U_MAX:
                    put("rnnt_lattice", dims + (b, t, u), lib.effconf_rnnt_lattice_workspace_bytes(h, b, t, u))
            for args in ((-1, 13), (4, -1)):
                put("rnnt_greedy", dims + args, lib.effconf_rnnt_workspace_bytes(h, *args))
            for args in ((4, 13, 17, 256, 208), (4, 13, 0, 256, 208), (4, 13, 4, 0, 208), (4, 13, 4, 64, 0), (-1, 13, 4, 64, 64), (4, 0, 4, 64, 64)):
                put("rnnt_beam", dims + args, lib.effconf_rnnt_beam_workspace_bytes(h, *args))
            for args in ((4, 50, -1), (4, 50, 1024), (-1, 50, 20), (4, -1, 20), (1 << 15, 1 << 10, 63)):
                put("rnnt_lattice", dims + args, lib.effconf_rnnt_lattice_workspace_bytes(h, *args))
        finally:
            lib.effconf_rnnt_destroy(h)
    for args in list(itertools.product(BATCH, T_OUT, U_MAX)) + [(4, 50, -1), (4, 50, 1024), (-1, 50, 20), (4, -1, 20), (1 << 15, 1 << 10, 63), (0, 0, 0)]:
        put("rnnt_align", args, lib.effconf_rnnt_align_workspace_bytes(*args))
    for dims in LM:
        h = lib.effconf_lm_create(C.byref(_lib.EcLmConfig(*dims)))
        assert h
        try:
            for args in list(itertools.product(BATCH + (17, 33, 40), (0, 6, 1023))) + [(-1, 4), (4, -1), (4, 4097), (1 << 20, 2048), ((1 << 21) + 1, 1)]:
                put("lm", dims + args, lib.effconf_lm_workspace_bytes(h, *args))
        finally:
            lib.effconf_lm_destroy(h)
    for b, t, beam in itertools.product(BATCH, T_OUT + (0,), (1, 4, 16, 32)):
        put("ctc_beam", (b, t, 40, beam), lib.effconf_ctc_beam_workspace_bytes(b, t, 40, beam))
    for args in ((4, 50, 256, 0), (4, 50, 256, 33), (4, 50, 1, 16), (4, 50, 1025, 16), (-1, 50, 256, 16), (4, -1, 256, 16)):
        put("ctc_beam", args, lib.effconf_ctc_beam_workspace_bytes(*args))
    for b, t, u in itertools.product(BATCH, T_OUT + (0,), U_MAX + (127, 128, 2047)):      # 127 / 128: one and two states per thread
        put("ctc_align", (b, t, 40, u), lib.effconf_ctc_align_workspace_bytes(b, t, 40, u))
    for args in ((4, 50, 1, 20), (4, 50, 1025, 20), (4, 50, 256, -1), (4, 50, 256, 2048), (-1, 50, 256, 20), (4, -1, 256, 20)):
        put("ctc_align", args, lib.effconf_ctc_align_workspace_bytes(*args))
    return out


def _tables():
    from efficientconformer_amd import _lib
    with open(GOLDEN) as fh:
        want = json.load(fh)
    return want, rows(_lib.load(), _lib)


def test_six_entries_return_the_recorded_sizes():
    want, got = _tables()
    assert set(got) == set(want)
    for entry in sorted(set(got) - {"rnnt_greedy"}):
        assert got[entry].keys() == want[entry].keys(), entry
        bad = {k: (v, want[entry][k]) for k, v in got[entry].items() if v != want[entry][k]}
        assert not bad, (entry, dict(list(bad.items())[:8]))
        assert any(v == 0 for v in got[entry].values()) and any(v > 0 for v in got[entry].values()), entry


def test_greedy_size_grows_by_less_than_one_alignment():
    want, got = _tables()
    assert got["rnnt_greedy"].keys() == want["rnnt_greedy"].keys()
    grown = 0
    for k, v in got["rnnt_greedy"].items():
        w = want["rnnt_greedy"][k]
        if w == 0:
            assert v == 0, k
            continue
        assert w <= v < w + 256, (k, v, w)
        grown += v > w
    # B T J 4 % 256 != 0 somewhere in the grid (B T odd, J = 32): the planned region is padded there, and only there
    assert grown > 0
    for k, v in got["rnnt_greedy"].items():
        de, h, j, vocab, b, t = (int(x) for x in k.split())
        if want["rnnt_greedy"][k]:
            assert v - want["rnnt_greedy"][k] == -(b * t * j * 4) % 256, k


if __name__ == "__main__":
    from efficientconformer_amd import _lib as L
    assert sys.argv[1] == "--record"
    with open(sys.argv[2], "w") as out:
        json.dump(rows(L.load(), L), out, indent=0, sort_keys=True)
        out.write("\n")
