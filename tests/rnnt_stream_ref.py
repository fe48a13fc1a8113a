"""The streaming RNN-T greedy decode as a specification (test helper, not a test module): a chunked greedy decode in torch with the explicit carried state
(h, c, gd, primed) of DESIGN.md 6k, built from oracle.ref_transducer.lstm_step / joint_logits; the cases and push patterns of tests/test_gpu_rnnt_stream.py and
tests/test_rnnt_stream_host.py; the conditions a run must have met for its result to mean something; and the faults a GPU implementation could have.

The invariant.  In the greedy loop (oracle.ref_transducer.greedy_decode) the frame index advances only through a blank or a decision forced by
max_consec_dec_step, and both reset the consecutive counter; after every emitted token the prediction network runs again on the same frame.  So at every frame
boundary, and only there, the counter is 0, the LSTM state has consumed every token emitted so far and gd = linear_decoder(h) + bias is what the next joint
evaluation reads.  A stream that has not seen a frame is the exception: zero state, the start token 0 not yet consumed (primed = 0).  ``chunked_greedy`` asserts
all of that at the end of every push that had a frame, and that every logit vector it forms from the carried gd is the oracle's joint_logits on the carried h,
bit for bit.

Pushes run in rounds over all streams in ascending order, as a session issues them: round r brings pushes[b][r] frames to stream b."""
import functools

import torch

import rnnt_shapes as S
from efficientconformer_amd import synth
from oracle.ref_transducer import _t, joint_logits, lstm_step

KF = 4                       # encoder frames per joint pass of the kernel (csrc/rnnt.hip)
# (Denc, H, J, V), blank bias
CASES = (((20, 36, 44, 37), 1.2),        # nothing divides 16: the matvec remainder
         ((12, 20, 28, 9), 1.2),         # linear_encoder GEMM with K < 16
         ((200, 320, 320, 1000), 1.2),   # the shipped Small decoder
         ((20, 36, 44, 37), 0.0))        # five forced tokens on nearly every frame
SMALLEST = CASES[1]
PATTERNS = ("1", "3", "4", "5", "12", "irregular")
CONDITIONS = ("token on a push's last frame", "forced decision on a push's last frame", "blank-only push", "push ending inside a KF group",
              "push ending on a KF group's edge", "idle stream beside busy ones", "stream that never gets a frame")
FAULTS = ("step_rerun", "hc_zeroed", "gd_stale", "start_not_consumed", "frames_not_offset")


def case_id(case):
    return "%s-bias%g" % ("x".join(str(d) for d in case[0]), case[1])


@functools.lru_cache(maxsize=None)
def weights(dims, blank_bias):
    """The weights of rnnt_shapes.weights(dims, blank_bias) as this module's own arrays: rnnt_shapes' cached ones are shared with tests that write faults into
    them, so a reference that must not move is computed from these.  Never modified."""
    de, h, j, v = dims
    return synth.make_transducer_state_dict(de, {"dim_model": h, "vocab_size": v, "num_layers": 1}, {"dim_model": j, "joint_mode": "sum", "act": "tanh"},
                                            S.SEED, blank_bias=blank_bias)


def inputs(dims):
    """Encoder outputs (20, 12, Denc) and ragged lengths (0, 1, and several that are no multiple of KF)."""
    return S.frames(dims[0], S.GREEDY_BATCH, S.GREEDY_T), S.ragged(S.GREEDY_BATCH, S.GREEDY_T)


def pushes(pattern, n, stream):
    """Frames per round of a stream with n frames.  "k": k frames a round until the stream ends (then 0: listed with no frames); "irregular": [2, 0, 5, 1, rest]
    rotated by the stream index - a 0 there means the stream is idle and NOT listed in that round."""
    if pattern == "irregular":
        base = [2, 0, 5, 1]
        steps = base[stream % 4:] + base[:stream % 4]
    else:
        k = int(pattern)
        steps = [k] * ((S.GREEDY_T + k - 1) // k)
    out, s = [], 0
    for x in steps:
        x = min(x, n - s)
        out.append(x)
        s += x
    if pattern == "irregular":
        out.append(n - s)
    assert sum(out) == n
    return out


def listed(pattern, round_frames):
    """Which streams a round lists: every one in the fixed patterns (a finished or empty stream with out_len 0), those with frames in the irregular one."""
    return [b for b, x in enumerate(round_frames) if x > 0 or pattern != "irregular"]


def all_pushes(pattern, lens):
    return [pushes(pattern, int(n), b) for b, n in enumerate(lens)]


def chunked_greedy(sd, f, push_frames, max_consec=S.MAX_CONSEC, dtype=torch.float32, fault=None, lists=None, fresh_gd=None):
    """The greedy decode of f (B, T, Denc), stream b fed push_frames[b][r] frames in round r, from the carried state alone.  `lists(round frames)`: the streams a
    round lists (default: those with frames).  -> dict: tokens, frames (the global encoder frame of every token), steps (LSTM steps over the stream's life), per
    push records (stream, round, frames, tokens, forced decisions and tokens on its last frame, steps) and the final state (h, c, gd, primed) of every stream."""
    assert fault is None or fault in FAULTS
    # the faults:
    #   step_rerun          a resumed push runs a decoder step (on the stream's last token) before its first joint evaluation
    #   hc_zeroed           a resumed push starts from h = c = 0 (gd is carried)
    #   gd_stale            gd is not carried: a resumed push reads what the last decoder step of ANY stream left behind
    #   start_not_consumed  a fresh stream is taken for a primed one: no step on the start token, the joint reads the record as it lies (`fresh_gd`; default:
    #                       the NaN patterns the GPU test fills the state buffer with)
    #   frames_not_offset   emission frames are push-local
    sd = {k: _t(sd, k).to(dtype) for k in sd if k.startswith(("decoder.", "joint_network."))}
    f = torch.as_tensor(f).to(dtype)
    wd, bd = sd["joint_network.linear_decoder.weight"], sd["joint_network.linear_decoder.bias"]
    we, be = sd["joint_network.linear_encoder.weight"], sd["joint_network.linear_encoder.bias"]
    wj, bj = sd["joint_network.linear_joint.weight"], sd["joint_network.linear_joint.bias"]
    B, H, J = f.shape[0], wd.shape[1], wd.shape[0]
    h = [torch.zeros(H, dtype=dtype) for _ in range(B)]
    c = [torch.zeros(H, dtype=dtype) for _ in range(B)]
    gd = [torch.full((J,), float("nan"), dtype=dtype) for _ in range(B)]          # never read while primed is clear
    primed = [False] * B
    last = [0] * B                                    # the last token: what only the step_rerun fault reads
    scratch_gd = torch.zeros(J, dtype=dtype)          # where a gd that is not carried would be left behind (gd_stale)
    done = [0] * B
    tokens, frames, steps, records = [[] for _ in range(B)], [[] for _ in range(B)], [0] * B, []
    rounds = max(len(p) for p in push_frames)
    with torch.no_grad():
        for r in range(rounds):
            rf = [p[r] if r < len(p) else 0 for p in push_frames]
            for b in (lists(rf) if lists is not None else [b for b in range(B) if rf[b] > 0]):
                n = rf[b]
                rec = dict(stream=b, round=r, frames=n, tokens=0, last_frame_tokens=0, last_frame_forced=0, steps=0, primed=primed[b])
                records.append(rec)
                if n == 0:
                    continue                          # no frame: the record stays as it is
                hb, cb, gb = h[b], c[b], gd[b]
                run_dec = not primed[b]
                if fault == "start_not_consumed" and not primed[b]:
                    run_dec, gb = False, (gb if fresh_gd is None else fresh_gd.to(dtype))
                if primed[b]:
                    if fault == "step_rerun":
                        run_dec = True
                    if fault == "hc_zeroed":
                        hb, cb = torch.zeros_like(hb), torch.zeros_like(cb)
                    if fault == "gd_stale":
                        gb = scratch_gd.clone()
                y, t, consec = last[b] if fault == "step_rerun" else 0, 0, 0
                while t < n:
                    if run_dec:
                        hb, cb = lstm_step(sd, y, hb, cb)
                        gb = wd @ hb + bd
                        scratch_gd = gb
                        rec["steps"] += 1
                    run_dec = True
                    while t < n:
                        ft = f[b, done[b] + t]
                        logits = wj @ torch.tanh(we @ ft + be + gb) + bj
                        if fault is None:
                            assert torch.equal(logits, joint_logits(sd, ft, hb)), "the carried gd is not linear_decoder of the carried h"
                        pred = int(logits.argmax())
                        forced = consec == max_consec
                        if pred == 0 or forced:
                            consec = 0
                            if t == n - 1 and forced:
                                rec["last_frame_forced"] += 1
                            t += 1
                        else:
                            consec += 1
                            y = pred
                            tokens[b].append(pred)
                            frames[b].append(t if fault == "frames_not_offset" else done[b] + t)
                            rec["tokens"] += 1
                            if t == n - 1:
                                rec["last_frame_tokens"] += 1
                            break
                steps[b] += rec["steps"]
                if fault is None:
                    # the boundary invariant
                    assert consec == 0, "a push ended with the consecutive counter running"
                    assert torch.equal(gb, wd @ hb + bd), "gd is not linear_decoder(h) + bias at the frame boundary"
                    assert steps[b] == len(tokens[b]) + 1, "the LSTM has not consumed exactly the emitted tokens"
                    assert rec["tokens"] <= max(max_consec * n, 1), "the per-push token bound"
                h[b], c[b], gd[b], primed[b], last[b] = hb, cb, gb, True, y
                done[b] += n
    return dict(tokens=tokens, frames=frames, steps=steps, records=records, h=h, c=c, gd=gd, primed=primed)


def conditions(records, lens, rounds_listed):
    """Which of CONDITIONS a run met.  records: per push dicts with stream, frames, tokens, last_frame_tokens, last_frame_forced; rounds_listed: per round the
    listed streams."""
    seen = set()
    for r in records:
        if r["frames"] == 0:
            continue
        if r["last_frame_tokens"]:
            seen.add(CONDITIONS[0])
        if r["last_frame_forced"]:
            seen.add(CONDITIONS[1])
        if r["tokens"] == 0:
            seen.add(CONDITIONS[2])
            # without a token the joint passes of a push are whole KF groups from its first frame on
            seen.add(CONDITIONS[3] if r["frames"] % KF else CONDITIONS[4])
    busy = {(r["round"], r["stream"]) for r in records if r["frames"] > 0}
    for rnd, ids in enumerate(rounds_listed):
        if any((rnd, b) in busy for b in ids) and len(ids) < len(lens) and any(int(lens[b]) > 0 for b in range(len(lens)) if b not in ids):
            seen.add(CONDITIONS[5])
    if any(int(n) == 0 for n in lens):
        seen.add(CONDITIONS[6])
    return seen


@functools.lru_cache(maxsize=None)
def reference(case, pattern, dtype=torch.float32, fault=None):
    """chunked_greedy of a case under a pattern (computed once, shared, never modified) and the streams every round lists."""
    dims, bias = case
    f, lens = inputs(dims)
    pf = all_pushes(pattern, lens)
    rounds = max(len(p) for p in pf)
    rl = [listed(pattern, [p[r] if r < len(p) else 0 for p in pf]) for r in range(rounds)]
    out = chunked_greedy(weights(dims, bias), f, pf, dtype=dtype, fault=fault, lists=lambda rf: listed(pattern, rf))
    return out, rl
