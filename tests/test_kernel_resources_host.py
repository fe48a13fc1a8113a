"""Compile-time resources of the stage-2 / stage-3 chain kernels, of the head-width-64 attention kernel and of the decoder kernels (no GPU: hipcc cross-compiles
for gfx950).

A scratch reload inside one of these kernels waits on the vmcnt queue its own prefetches are in (LDS-DMAs of the weight ring, the K / V / E loads one key block
ahead): the reload of a spilled lane constant drains what was just issued.  The kernels are kept free of scratch altogether; their occupancy (waves per SIMD) is
what the launch shapes were chosen for and may not be traded for registers.  Only the compiler's kernel-resource-usage remarks are read."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from efficientconformer_amd import _build


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")

_REMARKS = {}


def _compile(source):
    cmd = [_hipcc()] + _build.FLAGS + _build.NO_PACKED_FP32 + _build.PER_SOURCE.get(source, []) + \
          ["--cuda-device-only", "-c", os.path.join(_build.CSRC, source), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"\(anonymous namespace\)::", "", n).split("(")[0].replace("void ", ""): v for n, v in zip(names, rows.values())}


def _resources(source):
    """{demangled kernel name: {"vgpr", "occupancy", "scratch"}} of one source under the product flags (the sources are compiled once, side by side)."""
    if not _REMARKS:
        sources = sorted({s for s, _, _, _ in BROUGHT_TO_ZERO + STAY_AT_ZERO + SCRATCH_BOUNDED})
        with ThreadPoolExecutor(max_workers=len(sources)) as ex:
            _REMARKS.update(zip(sources, ex.map(_compile, sources)))
    return _REMARKS[source]


# (source, kernel, waves per SIMD, scratch bytes per lane).  Every kernel of this list is at zero scratch: none needs a bound of its own.
BROUGHT_TO_ZERO = [
    ("chain3.hip", "chain3_kernel<16, 1, false>", 3, 0),
    ("chain3.hip", "chain3_kernel<16, 2, false>", 3, 0),
    ("chain3.hip", "chain3_kernel<16, 3, false>", 3, 0),
    ("attention2.hip", "relpos_attention2_kernel<64, 4, 1, 1>", 3, 0),
    ("chain.hip", "chain_kernel<12, 8, 3, 0, false>", 2, 0),
]
# kernels of the flagship step that had no scratch before: they keep none (and their occupancy)
STAY_AT_ZERO = [
    ("chain.hip", "chain_kernel<8, 4, 2, 0, false>", 2, 0),
    ("chain.hip", "chain_kernel<8, 4, 2, 1, false>", 2, 0),
    ("chain2.hip", "chain2_kernel<16, false>", 2, 0),
    ("attention2.hip", "relpos_attention2_kernel<96, 4, 1, 1>", 2, 0),
    # the chunked front end (sub_chunked.h) in its two formats: the occupancies the 1 / 4 / 6 / 12-tile instances had as two separate kernels
    ("sublinear3.hip", "sublinear3_kernel<1>", 5, 0),
    ("sublinear3.hip", "sublinear3_kernel<4>", 3, 0),
    ("sublinear3.hip", "sublinear3_kernel<6>", 2, 0),
    ("sublinear3.hip", "sublinear3_kernel<12>", 1, 0),
    ("sxf_sub.hip", "sxf_sublin_kernel<1>", 4, 0),
    ("sxf_sub.hip", "sxf_sublin_kernel<4>", 2, 0),
    ("sxf_sub.hip", "sxf_sublin_kernel<6>", 1, 0),
    ("sxf_sub.hip", "sxf_sublin_kernel<12>", 1, 0),
]
# instances that carry scratch today, or are newer than the lists above: their occupancy and an upper bound on their scratch (a bound, not an equality: less is
# welcome).  The bounds are the ones set when the chains' shared pieces moved into chain_common.h; measured at that commit, before and after alike
# (profiles/kernel_resources.txt): 0, 0, 0, 12, 0, 36, 24, 60, 52 bytes in the order below
SCRATCH_BOUNDED = [
    ("chain2.hip", "chain2_kpad_kernel<16>", 2, 0),
    ("chain3.hip", "chain3_kpad_kernel<16, 2>", 3, 0),
    ("chain3.hip", "chain3_kpad_kernel<16, 3>", 3, 0),
    ("chain3.hip", "chain3_kpad_kernel<16, 1>", 3, 12),
    ("chain.hip", "chain_kpad_kernel<12, 8, 3, 0>", 2, 36),
    ("chain.hip", "chain_kpad_kernel<12, 8, 3, 1>", 2, 84),
    ("chain.hip", "chain_kpad_kernel<12, 8, 3, 3>", 2, 64),
    ("chain.hip", "chain_kernel<12, 8, 3, 1, false>", 2, 96),
    ("chain.hip", "chain_kernel<12, 8, 3, 3, false>", 2, 84),
]
# the decoders: the occupancies their kernels had before the LSTM cell, the 16-column LSTM step and the vocabulary log-softmax loop moved into decode_common.h
# (profiles/decoder_common.txt has the registers before and after), and no scratch
DECODERS = [
    ("rnnt.hip", "rnnt_greedy_kernel", 4, 0),
    ("rnnt.hip", "rnnt_cluster_kernel<8, 8, 2>", 2, 0),
    ("rnnt.hip", "rnnt_cluster_kernel<16, 16, 1>", 2, 0),
    ("rnnt_beam.hip", "rnnt_beam_kernel", 4, 0),
    ("rnnt_lattice.hip", "rnnt_prednet_kernel", 5, 0),
    ("rnnt_lattice.hip", "rnnt_joint_kernel", 6, 0),
    ("lm.hip", "lm_lstm_step_kernel<4>", 2, 0),
    ("lm.hip", "lm_lstm_step_kernel<2>", 4, 0),
    ("lm.hip", "lm_lstm_step_kernel<1>", 7, 0),
    ("lm.hip", "lm_head_kernel<false>", 8, 0),
    ("lm.hip", "lm_head_kernel<true>", 8, 0),
    ("ctc_beam.hip", "ctc_beam_kernel", 4, 0),
    ("ctc_align.hip", "ctc_trellis_kernel<16, true>", 4, 0),
    ("ctc_align.hip", "ctc_trellis_kernel<16, false>", 6, 0),
]
STAY_AT_ZERO = STAY_AT_ZERO + DECODERS


@pytest.mark.parametrize("source,kernel,occupancy,scratch", BROUGHT_TO_ZERO + STAY_AT_ZERO, ids=[k for _, k, _, _ in BROUGHT_TO_ZERO + STAY_AT_ZERO])
def test_kernel_keeps_its_occupancy_and_uses_no_scratch(source, kernel, occupancy, scratch):
    res = _resources(source)
    assert kernel in res, (kernel, sorted(res))
    got = res[kernel]
    print("%s: %d VGPRs, %d waves/SIMD, %d scratch bytes/lane" % (kernel, got["vgpr"], got["occupancy"], got["scratch"]))
    assert got["occupancy"] == occupancy, got
    assert got["scratch"] == scratch, got
    assert got["vgpr"] <= 512 // occupancy, got


@pytest.mark.parametrize("source,kernel,occupancy,scratch", SCRATCH_BOUNDED, ids=[k for _, k, _, _ in SCRATCH_BOUNDED])
def test_kernel_keeps_its_occupancy_and_its_scratch_bound(source, kernel, occupancy, scratch):
    res = _resources(source)
    assert kernel in res, (kernel, sorted(res))
    got = res[kernel]
    print("%s: %d VGPRs, %d waves/SIMD, %d scratch bytes/lane" % (kernel, got["vgpr"], got["occupancy"], got["scratch"]))
    assert got["occupancy"] == occupancy, got
    assert got["scratch"] <= scratch, got
    assert got["vgpr"] <= 512 // occupancy, got
