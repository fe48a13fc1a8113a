"""Test helper (no tests here): a float64 CHUNKED encoder written from the oracle's own stage functions (oracle/ref_encoder.py), with an explicit K / V cache
and an explicit depthwise-convolution state per block - the specification of the streaming session's state machine (efficientconformer_amd/streaming.py,
csrc/forward_stream.hip).  One stream; ``push(mel_new, final)`` returns the new output rows.  tests/test_stream_host.py holds it to
R.encoder_from_mel(..., dtype = float64) on whole utterances and injects the faults below to show that the GPU test's bound sees each of them.

The state machine:
  mel       frames not yet consumed, from mel frame 2 done - 2 on (two zero columns in front of frame 0): row t reads the frames 2 t - 1 .. 2 t + 1
  per block K, V: the grouped rows of the last `capacity` positions (streaming.cache_capacities); conv: the last k - 1 GLU rows (zeros before the first chunk)
  attention scores of query i, key j (ABSOLUTE grouped positions): (Qu_i . K_j + Qv_i . E[i - j]) / sqrt(d), visible iff 0 <= i - j <= band; E[delta] =
            pos_layer(sinusoid(G delta + G - 1 .. G delta)) - the causal table's grouped row, whatever the sequence length
"""
import torch
import torch.nn.functional as F

from efficientconformer_amd import streaming as S
from oracle import ref_encoder as R

FAULTS = ("cache one grouped row short", "band off by one", "conv state stale for one chunk", "E indexed from the chunk's start", "strided block starts on an odd row")


class ChunkedRef:
    def __init__(self, sd, plan, max_frames, dtype=torch.float64, fault=None, fault_chunk=1):
        assert S.stream_refusal(plan) is None
        self.sd, self.plan, self.dtype = R.cast_state_dict(sd, dtype), plan, dtype
        self.align = S.stream_align(plan)
        self.cap = S.cache_capacities(plan, max_frames)
        self.fault, self.fault_chunk = fault, fault_chunk
        self.buf = torch.zeros(plan.n_mels, 2, dtype=dtype)
        self.frames = self.done = self.chunks = 0
        nb = len(plan.blocks)
        self.k = [None] * nb
        self.v = [None] * nb
        self.pos = [0] * nb                       # absolute grouped position of the next query, per block
        self.conv = [torch.zeros(bp.kernel_size - 1, bp.dim_expand, dtype=dtype) for bp in plan.blocks]
        self.e = []
        ms = 1
        self.band = []
        for i, bp in enumerate(plan.blocks):
            self.band.append(min(plan.left_context // (ms * bp.group_size), S.UNLIMITED))
            ms *= bp.conv_stride
            n_dist = self.cap[i] + 1 + 64          # distances up to the capacity + the largest chunk of the tests (in grouped rows)
            m = "blocks.%d.multi_head_self_attention_module.mhsa." % bp.index
            rows = R.rel_sinusoid_rows_causal(bp.group_size * n_dist, bp.dim_model, dtype)
            e = F.linear(rows, R._t(self.sd, m + "pos_layer.weight"), R._t(self.sd, m + "pos_layer.bias"))
            d = bp.group_size * bp.dim_model // bp.num_heads
            self.e.append(e.reshape(n_dist, bp.num_heads, d).flip(0))          # [delta][head][d]

    # ------------------------------------------------------------------ one block on a chunk's rows
    def _attention(self, i, bp, x, faulty):
        sd, G, H = self.sd, bp.group_size, bp.num_heads
        p = "blocks.%d.multi_head_self_attention_module" % bp.index
        m = p + ".mhsa."
        n, D = x.shape
        h = F.layer_norm(x, (D,), R._t(sd, p + ".norm.weight"), R._t(sd, p + ".norm.bias"), R.LN_EPS)
        q, k, v = (F.linear(h, R._t(sd, m + nm + ".weight"), R._t(sd, m + nm + ".bias")) for nm in ("query_layer", "key_layer", "value_layer"))
        pad = -n % G
        if pad:                                    # only a final chunk: zeros behind the projections, so the rows become Qu = u, Qv = v, K = V = 0
            q, k, v = (F.pad(z, (0, 0, 0, pad)) for z in (q, k, v))
        d = G * D // H
        tg = (n + pad) // G
        qu = (q + R._t(sd, m + "u")).reshape(tg, H, d)
        qv = (q + R._t(sd, m + "v")).reshape(tg, H, d)
        k, v = k.reshape(tg, H, d), v.reshape(tg, H, d)
        ck, cv = self.k[i], self.v[i]
        if faulty and self.fault == FAULTS[0] and ck is not None and ck.shape[0] > 0:
            ck, cv = ck[1:], cv[1:]
        cached = 0 if ck is None else ck.shape[0]
        keys = k if not cached else torch.cat([ck, k])
        vals = v if not cached else torch.cat([cv, v])
        pi = self.pos[i] + torch.arange(tg)                              # absolute positions of the queries
        pj = self.pos[i] - cached + torch.arange(cached + tg)            # and of the keys
        delta = pi[:, None] - pj[None, :]
        band = self.band[i] - (1 if faulty and self.fault == FAULTS[1] else 0)
        vis = (delta >= 0) & (delta <= band)
        look = delta
        if faulty and self.fault == FAULTS[3]:
            look = torch.arange(tg)[:, None] - torch.arange(cached + tg)[None, :]       # both indices counted from their buffers' starts
        e = self.e[i][look.clamp(0, self.e[i].shape[0] - 1)]             # (tg, keys, H, d)
        s = (torch.einsum("ihd,jhd->hij", qu, keys) + torch.einsum("ihd,ijhd->hij", qv, e)) / d ** 0.5
        s = s.masked_fill(~vis[None], float("-inf"))
        o = torch.einsum("hij,jhd->ihd", s.softmax(-1), vals).reshape(tg * G, D)[:n]
        keep = self.cap[i]
        self.k[i], self.v[i] = (keys[max(keys.shape[0] - keep, 0):], vals[max(vals.shape[0] - keep, 0):]) if keep else (keys[:0], vals[:0])
        self.pos[i] += tg
        return F.linear(o, R._t(sd, m + "output_layer.weight"), R._t(sd, m + "output_layer.bias"))

    def _conv(self, i, bp, x, faulty):
        sd, ks, s = self.sd, bp.kernel_size, bp.conv_stride
        p = "blocks.%d.convolution_module.layers" % bp.index
        D = x.shape[-1]
        h = F.layer_norm(x, (D,), R._t(sd, p + ".0.weight"), R._t(sd, p + ".0.bias"), R.LN_EPS)
        h = F.linear(h, R._t(sd, p + ".2.weight")[:, :, 0], R._t(sd, p + ".2.bias"))
        a, g = h.chunk(2, dim=-1)
        glu = a * torch.sigmoid(g)
        full = torch.cat([self.conv[i], glu])                            # the k - 1 rows in front of the chunk, then the chunk
        odd = faulty and self.fault == FAULTS[4] and s > 1
        y = F.conv1d(full.t()[None], R._t(sd, p + ".4.weight"), R._t(sd, p + ".4.bias"), stride=1, groups=full.shape[1])[0].t()      # one output per chunk row
        y = y[(1 if odd and y.shape[0] > 1 else 0)::s]
        if not (faulty and self.fault == FAULTS[2]):
            self.conv[i] = full[full.shape[0] - (ks - 1):]
        y = F.batch_norm(y.t()[None], R._t(sd, p + ".5.running_mean"), R._t(sd, p + ".5.running_var"), R._t(sd, p + ".5.weight"), R._t(sd, p + ".5.bias"),
                         False, 0.0, R.BN_EPS)[0].t()
        y = y * torch.sigmoid(y)
        return F.linear(y, R._t(sd, p + ".7.weight")[:, :, 0], R._t(sd, p + ".7.bias")), odd

    def _block(self, i, bp, x, faulty):
        sd, p = self.sd, "blocks.%d" % bp.index
        x = x + 0.5 * R.ffn(x, sd, p + ".feed_forward_module1")
        x = x + self._attention(i, bp, x, faulty)
        c, odd = self._conv(i, bp, x, faulty)
        xs = x[(1 if odd and x.shape[0] > 1 else 0)::bp.conv_stride]
        res = F.linear(xs, R._t(sd, p + ".conv_res.1.weight")[:, :, 0], R._t(sd, p + ".conv_res.1.bias")) if bp.transition else xs
        x = res + c
        x = x + 0.5 * R.ffn(x, sd, p + ".feed_forward_module2")
        return F.layer_norm(x, (x.shape[-1],), R._t(sd, p + ".norm.weight"), R._t(sd, p + ".norm.bias"), R.LN_EPS)

    # ------------------------------------------------------------------ the session
    def push(self, mel_new, final=False):
        """mel_new (n_mels, t) -> the new output rows (t_new, D_last)."""
        plan = self.plan
        if mel_new.shape[1]:
            self.buf = torch.cat([self.buf, mel_new.to(self.dtype)], 1)
            self.frames += mel_new.shape[1]
        n = S.rows_to_encode(self.frames, self.done, self.align, final)
        d_out = plan.blocks[-1].dim_expand
        if n == 0:
            return torch.zeros(0, d_out, dtype=self.dtype)
        win = self.buf[:, :2 * n + 2]
        if win.shape[1] < 2 * n + 2:                                    # a final chunk: the subsampler's zero padding behind the last frame
            win = F.pad(win, (0, 2 * n + 2 - win.shape[1]))
        sub, _ = R.subsample(win[None], None, self.sd, plan.sub_layers)
        x = F.linear(sub[0].t()[1: n + 1], R._t(self.sd, "linear.weight"), R._t(self.sd, "linear.bias"))      # window row i + 1 = chunk row i
        faulty = self.fault is not None and self.chunks == self.fault_chunk
        for i, bp in enumerate(plan.blocks):
            x = self._block(i, bp, x, faulty)
        self.buf = self.buf[:, 2 * n:]
        self.done += n
        self.chunks += 1
        return x


def run(sd, plan, mel, pushes, fault=None, fault_chunk=1, dtype=torch.float64):
    """mel (n_mels, T) pushed as `pushes` (frame counts; the last push ends the stream and brings whatever is left) -> every output row."""
    ref = ChunkedRef(sd, plan, mel.shape[1], dtype, fault, fault_chunk)
    out, lo = [], 0
    for i, t in enumerate(pushes):
        last = i == len(pushes) - 1
        hi = mel.shape[1] if last else min(lo + t, mel.shape[1])
        out.append(ref.push(mel[:, lo:hi], final=last))
        lo = hi
    return torch.cat(out)


def pushes_of(name, total):
    """The push patterns of the tests as frame counts."""
    if name == "all":
        return [total]
    if name == "irregular":
        return [7, 50, 1, 0, 23, total]
    step = int(name)
    return [step] * (total // step) + [total]
