// Stand-alone host program for a sanitizer run of csrc/decode_layout.h (not part of the test suite): WsPlan and the decoder layouts written on it (the seven entries' and the fused beam search's), over
// the grid of tests/test_decoder_layout_host.py.  For every layout: the regions are 256-aligned, ascending and disjoint, an utterance's regions stay inside its
// stride, and for every misalignment of the caller's pointer (p % 256 in steps of 16) the aligned base plus the end of the last region stays inside
// p + total() - the property the greedy decoder's hand carve lacked.  Plain C++, no device, nothing linked.  From the repository root:
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/decoder_layout_sanitize.cpp -o decoder_layout_sanitize && ./decoder_layout_sanitize
// (or hipcc with -Xarch_host in front of the two sanitizer flags, as tools/routes_sanitize.cpp)
#include "../efficientconformer_amd/csrc/decode_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace ecdec;

namespace {

struct Region { size_t off, bytes; };
long long checked = 0;

void fail(const char* what, const char* layout) {
    std::fprintf(stderr, "decoder_layout_sanitize: %s in %s\n", what, layout);
    std::exit(1);
}

// regions in plan order inside a space of `space` bytes (a workspace without its slack, or one utterance's stride)
void check_regions(const char* layout, const std::vector<Region>& r, size_t space) {
    size_t prev_end = 0;
    for (const Region& x : r) {
        if (x.off % 256) fail("a region that is not 256-aligned", layout);
        if (x.off < prev_end) fail("overlapping or descending regions", layout);
        prev_end = x.off + x.bytes;
    }
    if (prev_end > space) fail("a region beyond the end", layout);
    ++checked;
}

void check_total(const char* layout, const std::vector<Region>& r, size_t total) {
    check_regions(layout, r, total - 256);
    const size_t end = r.back().off + r.back().bytes;
    for (uintptr_t mis = 0; mis < 256; mis += 16) {
        const uintptr_t p = (uintptr_t)1 << 20 | mis;
        const uintptr_t base = reinterpret_cast<uintptr_t>(WsPlan::base(reinterpret_cast<void*>(p)));
        if (base % 256 || base < p) fail("a base that is not the pointer aligned up", layout);
        if (base + end > p + total) fail("the last region beyond the reported size", layout);
    }
}

}  // namespace

int main() {
    const int batches[] = {0, 1, 7, 19, 256}, frames[] = {0, 1, 13, 250}, beams[] = {1, 4, 16, 32}, umaxes[] = {0, 5, 127, 128, 1023, 2047};
    const int rnnt[][4] = {{48, 32, 32, 40}, {48, 64, 64, 40}, {48, 128, 128, 50}, {360, 640, 640, 1000}, {48, 40, 40, 40}, {12, 4, 12, 2}};
    for (const auto& d : rnnt) {
        EcRnntConfig c{};
        c.dim_encoder = d[0]; c.dim_decoder = d[1]; c.dim_joint = d[2]; c.vocab_size = d[3]; c.num_layers = 1; c.max_consec_dec_step = 5;
        const size_t H = d[1], J = d[2];
        for (int b : batches) for (int t : frames) {
            const int shapes[][3] = {{8, 8, 2}, {16, 16, 1}};
            for (const auto& s : shapes) {
                const GreedyLayout L = greedy_layout(c, b, t, s[0], s[1], s[2]);
                const size_t n = L.ncl, cand = n * s[0] * s[1] * s[2] * 4;
                if (L.status != L.sync + n * 256 || L.sync_bytes != n * 256 + 256) fail("counters and status word apart", "greedy_layout");
                check_total("greedy_layout", {{L.fe, (size_t)b * t * J * 4}, {L.sync, L.sync_bytes}, {L.xh, n * s[1] * H * 4}, {L.xgd, n * s[1] * J * 4}, {L.xav, cand}, {L.xai, cand}},
                            L.total);
            }
            {   // the resumed greedy decode: `b` listed streams' push workspace, and the state buffer of b streams
                const RnntStreamWs W = rnnt_stream_ws(c, b, t);
                check_total("rnnt_stream_ws", {{W.fe, (size_t)b * t * J * 4}}, W.total);
                const RnntStreamLayout L = rnnt_stream_layout(c, b);
                check_regions("rnnt_stream_layout (stream)", {{0, (2 * H + J) * 4}}, L.rec_bytes);
                check_total("rnnt_stream_layout", {{L.primed, (size_t)b * 4}, {L.rec, (size_t)b * L.rec_bytes}}, L.total);
            }
            for (int beam : beams) {
                if (beam > 16) continue;
                const BeamLayout L = beam_layout(c, b, t, beam, 16 * beam);
                check_regions("beam_layout (utterance)", {{L.nodes, (size_t)L.nnodes * L.ns * 4}, {L.topv, (size_t)L.ecap * beam * 4}, {L.topl, (size_t)L.ecap * beam * 4},
                                                           {L.a, (size_t)L.acap * BEAM_HYP_BYTES}, {L.b, (size_t)beam * BEAM_HYP_BYTES}, {L.trail, (size_t)L.tcap * 8}}, L.per_utt);
                check_total("beam_layout", {{L.stats, (size_t)b * 16}, {L.fe, (size_t)b * t * J * 4}, {L.utt, (size_t)b * L.per_utt}}, L.total);
            }
            for (int u : umaxes) {
                if (u > 1023) continue;
                const size_t E = u + 1;
                const LatLayout L = lat_layout(c, b, t, u);
                check_total("lat_layout", {{L.tlen, (size_t)b * 4}, {L.ulen, (size_t)b * 4}, {L.start, ((size_t)b + 1) * 4}, {L.h, b * E * H * 4}, {L.gd, b * E * J * 4},
                                           {L.fe, (size_t)b * t * J * 4}}, L.total);
            }
        }
    }
    for (int b : batches) for (int t : frames) for (int u : umaxes) {
        if (u <= 1023) {
            const RnntAlignLayout L = rnnt_align_layout(b, t, u);
            check_regions("rnnt_align_layout (utterance)", {{0, (size_t)(u + 1) * L.wpu * 4}}, L.bp_utt);
            check_total("rnnt_align_layout", {{L.bp, (size_t)b * L.bp_utt}}, L.total);
        }
        const CtcAlignLayout L = ctc_align_layout(b, t, u);
        check_regions("ctc_align_layout (utterance)", {{0, (size_t)t * L.rbmax}}, L.bp_utt);
        check_total("ctc_align_layout", {{L.emit, (size_t)b * t * L.E * 4}, {L.path, (size_t)b * t * 4}, {L.bp, (size_t)b * L.bp_utt}}, L.total);
    }
    for (int b : batches) for (int t : frames) for (int beam : beams) {
        const CtcBeamLayout L = ctc_beam_layout(b, t, beam);
        check_regions("ctc_beam_layout (utterance)", {{L.trace, (size_t)t * beam * 16}, {L.nodes, (size_t)L.ncap * 16}, {L.hkeys, (size_t)L.hcap * 8}, {L.hvals, (size_t)L.hcap * 4}},
                      L.per_utt);
        check_total("ctc_beam_layout", {{L.stats, (size_t)b * 16}, {L.utt, (size_t)b * L.per_utt}}, L.total);
        {   // the resumed search: `b` listed streams' push workspace, and the state buffer of b streams of t frames
            const CtcBeamStreamWs W = ctc_beam_stream_ws(b, t, beam);
            check_regions("ctc_beam_stream_ws (stream)", {{0, (size_t)t * beam * 16}}, W.per_trace);
            check_total("ctc_beam_stream_ws", {{W.stats, (size_t)b * 16}, {W.trace, (size_t)b * W.per_trace}}, W.total);
            const CtcBeamStreamLayout S = ctc_beam_stream_layout(b, t, beam);
            if (S.ncap != L.ncap || S.hcap != L.hcap) fail("a trie that is not ctc_beam_layout's", "ctc_beam_stream_layout");
            check_regions("ctc_beam_stream_layout (stream)", {{S.rec, (size_t)CTC_BEAM_REC_INTS * 4}, {S.nodes, (size_t)S.ncap * 16}, {S.hkeys, (size_t)S.hcap * 8},
                                                               {S.hvals, (size_t)S.hcap * 4}}, S.per_stream);
            check_total("ctc_beam_stream_layout", {{S.primed, (size_t)b * 4}, {S.blocks, (size_t)b * S.per_stream}}, S.total);
        }
    }
    const int lms[][3] = {{40, 32, 1}, {50, 64, 2}, {1000, 1024, 4}};
    for (const auto& d : lms) {
        EcLmConfig c{};
        c.vocab_size = d[0]; c.dim_model = d[1]; c.num_layers = d[2];
        for (int n : {0, 1, 5, 17, 33, 40, 256}) {
            const LmLayout L = lm_layout(c, n);
            if (L.layer != (size_t)3 * lm_npad(n) * d[1] * 4) fail("a layer that is not h[2] + c of the padded batch", "lm_layout");
            check_total("lm_layout", {{L.ulen, (size_t)n * 4}, {L.state, (size_t)d[2] * L.layer}}, L.total);
        }
    }
    // the beam search with an LM: the search's regions + LM nodes per utterance, then requests, resume records, the round counter, the LM step state and its logits
    for (const auto& d : rnnt) {
        if (d[1] % 16 || d[2] % 16) continue;
        EcRnntConfig c{};
        c.dim_encoder = d[0]; c.dim_decoder = d[1]; c.dim_joint = d[2]; c.vocab_size = d[3]; c.num_layers = 1; c.max_consec_dec_step = 5;
        const int lmdims[][2] = {{32, 2}, {48, 3}, {4096, 3}};
        for (const auto& m : lmdims) {
            EcLmConfig mc{};
            mc.vocab_size = d[3]; mc.dim_model = m[0]; mc.num_layers = m[1];
            for (int b : batches) for (int t : frames) for (int beam : beams) {
                if (beam > 16 || t < 1 || (m[0] == 4096 && b > 19)) continue;
                const BeamLmLayout L = beam_lm_layout(c, mc, b, t, beam, 16 * beam);
                const BeamLayout P = beam_layout(c, b, t, beam, 16 * beam);
                const size_t ncol = (size_t)b * BEAM_LM_COLS, nlm = (size_t)L.nls + L.vocab;
                if (L.nls != 2 * m[1] * m[0] || L.vocab != d[3]) fail("an LM node that is not (h, c) per layer + the row", "beam_lm_layout");
                if (L.s.nodes != P.nodes || L.s.topv != P.topv || L.s.topl != P.topl || L.s.a != P.a || L.s.b != P.b || L.s.trail != P.trail || L.s.nnodes != P.nnodes)
                    fail("search regions that are not beam_layout's", "beam_lm_layout");
                check_regions("beam_lm_layout (utterance)", {{L.s.nodes, (size_t)L.s.nnodes * L.s.ns * 4}, {L.s.topv, (size_t)L.s.ecap * beam * 4}, {L.s.topl, (size_t)L.s.ecap * beam * 4},
                                                              {L.s.a, (size_t)L.s.acap * BEAM_HYP_BYTES}, {L.s.b, (size_t)beam * BEAM_HYP_BYTES}, {L.s.trail, (size_t)L.s.tcap * 8},
                                                              {L.lmnodes, (size_t)L.s.nnodes * nlm * 4}}, L.s.per_utt);
                const LmLayout M = lm_layout(mc, (int)ncol);
                check_regions("beam_lm_layout (LM step)", {{L.lml.ulen, ncol * 4}, {L.lml.state, (size_t)m[1] * L.lml.layer}}, M.total - 256);
                if (L.lml.layer != M.layer || L.lml.state != M.state) fail("an LM step state that is not lm_layout's", "beam_lm_layout");
                check_total("beam_lm_layout", {{L.s.stats, (size_t)b * 16}, {L.s.fe, (size_t)b * t * d[2] * 4}, {L.s.utt, (size_t)b * L.s.per_utt}, {L.req, ncol * 16}, {L.slot, ncol * 8},
                                               {L.resume, (size_t)b * BEAM_LM_RESUME_INTS * 4}, {L.counter, 4}, {L.lm, M.total - 256}, {L.logits, ncol * d[3] * 4}}, L.total);
            }
        }
    }
    const int ctclm[][3] = {{32, 32, 1}, {257, 48, 3}, {1000, 4096, 3}};
    for (const auto& d : ctclm) {
        EcLmConfig mc{};
        mc.vocab_size = d[0]; mc.dim_model = d[1]; mc.num_layers = d[2];
        for (int b : batches) for (int t : frames) for (int beam : beams) {
            if (d[1] == 4096 && b > 19) continue;
            const CtcBeamLmLayout L = ctc_beam_lm_layout(mc, b, t, beam);
            const CtcBeamLayout P = ctc_beam_layout(b, t, beam);
            const size_t ncol = (size_t)b * beam, nlm = (size_t)L.nls + L.vocab;
            if (L.nls != 2 * d[2] * d[1] || L.vocab != d[0] || L.nslots != 2 * beam + 1) fail("LM slots that are not 2 beam + 1 of (h, c) per layer + the row", "ctc_beam_lm_layout");
            if (L.s.trace != P.trace || L.s.nodes != P.nodes || L.s.hkeys != P.hkeys || L.s.hvals != P.hvals || L.s.ncap != P.ncap || L.s.hcap != P.hcap)
                fail("search regions that are not ctc_beam_layout's", "ctc_beam_lm_layout");
            check_regions("ctc_beam_lm_layout (utterance)", {{L.s.trace, (size_t)t * beam * 16}, {L.s.nodes, (size_t)L.s.ncap * 16}, {L.s.hkeys, (size_t)L.s.hcap * 8},
                                                              {L.s.hvals, (size_t)L.s.hcap * 4}, {L.trace2, (size_t)t * beam * 8}, {L.lmnodes, (size_t)L.nslots * nlm * 4}}, L.s.per_utt);
            const LmLayout M = lm_layout(mc, (int)ncol);
            if (L.lml.layer != M.layer || L.lml.state != M.state) fail("an LM step state that is not lm_layout's", "ctc_beam_lm_layout");
            check_total("ctc_beam_lm_layout", {{L.s.stats, (size_t)b * 16}, {L.s.utt, (size_t)b * L.s.per_utt}, {L.req, ncol * 16}, {L.slot, ncol * 8},
                                               {L.resume, (size_t)b * CTC_BEAM_LM_REC_INTS * 4}, {L.counter, 4}, {L.lm, M.total - 256}, {L.logits, ncol * d[0] * 4}}, L.total);
        }
    }
    std::printf("decoder_layout_sanitize: %lld layouts checked\n", checked);
    return 0;
}
