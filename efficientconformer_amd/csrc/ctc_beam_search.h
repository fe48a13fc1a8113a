// The body of the CTC prefix beam search, shared by the three kernels of ctc_beam.hip: NOT a stand-alone header.  ctc_beam.hip includes it inside
// ctc_beam_kernel (LM = false: the plain search), inside ctc_beam_lm_kernel (LM = true: the fused search, resumable) and inside ctc_beam_resume_kernel (LM = false,
// STREAM = true: the plain search of one push, its beam and trie carried in the stream's state); it reads `a` (CtcBeamArgs), `fz` (CtcLmSide), `sz` (CtcStreamSide)
// and the constants `LM` and `STREAM` of the enclosing kernel.  The search is written once; an `if constexpr` branch is not compiled into the kernels it is not for.
// STREAM: workgroup b runs stream sz.streams[b]; frames and trace are push-local (0 .. len - 1), the trie and its hash live in the stream's block of the state.
// (As a function template called from two one-line kernels the plain kernel came out one VGPR larger than it was as a kernel of its own; as the kernel's own body
// it is compiled to the registers it had.)
    __shared__ float slp[MAXV];                   // the frame's log-probabilities
    __shared__ int spos[MAXV];                    // token -> position in the frame's top-K list, -1 otherwise
    __shared__ unsigned hist[2][256];
    __shared__ unsigned long long selk[MAXK];     // top-K tokens, unordered: (okey(lp) << 32) | ~id, larger = earlier
    __shared__ int stop[MAXK];                    // top-K tokens in (lp desc, id asc) order
    __shared__ float sredm[CNW], sreds[CNW];
    __shared__ int sscan[CNW];
    // the beam, double buffered by frame parity, rank order
    __shared__ int bnode[2][MAXB], blast[2][MAXB], bpar[2][MAXB], bdep[2][MAXB];
    __shared__ float bpb[2][MAXB], bpnb[2][MAXB], bs[2][MAXB];
    __shared__ int bpm[MAXB];                     // rank of the member whose prefix is this member's parent, -1: none
    __shared__ unsigned bexcl[MAXB][3];           // top-K positions that are not plain extensions of the member
    // candidates: [0, n) members, [n, 2n) repeat extensions, [2n, 2n + n beam) plain extensions (member i: 2n + i beam + r)
    __shared__ float cs[MAXS], cpb[MAXS], cpnb[MAXS];
    __shared__ int ck[MAXS];                      // ((last token + 1) << 16) | canonical index; INT_MAX: empty slot
    __shared__ unsigned long long ckey[MAXS];     // cand_key(cs, ck); 0: empty slot
    __shared__ int nsel[MAXB];                    // candidate slot of each rank of the next beam
    __shared__ int s_n, s_nn, s_nsel, s_nvalid, s_digit, s_need;
    // the fused search: L and LM slot of the members, whether a member's row is still the LM step's raw logits; L of the candidates
    __shared__ float bL[2][LM ? MAXB : 1], cL[LM ? MAXS : 1];
    __shared__ int bslot[2][LM ? MAXB : 1], spend[LM ? MAXB : 1], s_susp;

    const CtcBeamLayout& L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, V = a.V, beam = a.beam, T = a.T;
    const int K = 2 * beam + 1 < V ? 2 * beam + 1 : V;
    long long lenll = a.lens[b];
    const int len = lenll < 0 ? 0 : (lenll > T ? T : (int)lenll);
    int sid = b;
    if constexpr (STREAM) {                        // the first guard, before any address of the state is formed (workgroup-uniform)
        sid = sz.streams[b];
        if (sid < 0 || sid >= sz.max_streams) {
            if (tid < sz.nbest) a.token_len[(size_t)b * sz.nbest + tid] = -1;
            return;
        }
    }
    char* base = a.utt + (size_t)b * L.per_utt;
    char* tbase = STREAM ? sz.blocks + (size_t)sid * sz.per_stream : base;     // where the trie lives
    int4* trace = reinterpret_cast<int4*>(base + L.trace);
    int4* nodes = reinterpret_cast<int4*>(tbase + L.nodes);
    unsigned long long* hkeys = reinterpret_cast<unsigned long long*>(tbase + L.hkeys);
    int* hvals = reinterpret_cast<int*>(tbase + L.hvals);
    const unsigned hmask = (unsigned)L.hcap - 1;
    const float* lrow = a.logits + (size_t)b * T * V;
    int t0 = 0;
    long long ncand0 = 0;
    int nreq = 1;                                  // the fused search, thread 0: LM rows asked for (the root's is the first)
    int* rec = nullptr;
    float* lmn = nullptr;                          // the utterance's LM slots
    float2* trace2 = nullptr;
    int nf = 0;                                    // floats of an LM slot
    bool fresh = true;
    if constexpr (LM) {
        rec = fz.resume + (size_t)b * CTC_LM_RESUME_INTS;
        if (rec[R_PHASE] == 2) return;             // finished in an earlier launch (workgroup-uniform)
        fresh = rec[R_PHASE] == 0;
        lmn = reinterpret_cast<float*>(base + fz.lmnodes);
        trace2 = reinterpret_cast<float2*>(base + fz.trace2);
        nf = fz.nls + V;
    }
    int consumed = 0;                              // STREAM: frames of the stream before this push
    if constexpr (STREAM) {
        // the second guard: it reads the stream's flag and, where that is set, the frame count of its record - nothing else, and writes nothing (uniform)
        rec = reinterpret_cast<int*>(tbase + sz.rec);
        fresh = sz.primed[sid] == 0;
        consumed = fresh ? 0 : rec[S_FRAMES];
        if (len > sz.max_frames - consumed) {
            if (tid < sz.nbest) a.token_len[(size_t)b * sz.nbest + tid] = -2;
            return;
        }
    }

    if (fresh) {
        // STREAM: a push without frames writes nothing to the state (the beam of a stream that never had a frame is the empty prefix, in LDS alone)
        const int hinit = !STREAM || len > 0 ? L.hcap : 0;
        for (int i = tid; i < hinit; i += CT) __hip_atomic_store(hkeys + i, HEMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (!LM) {
            for (int i = tid; i < MAXV; i += CT) spos[i] = -1;
            hist[0][tid] = 0u;
        }
        if (tid == 0) {
            if (!STREAM || len > 0) nodes[0] = make_int4(-1, -1, 0, 0);
            bnode[0][0] = 0; blast[0][0] = -1; bpar[0][0] = -1; bdep[0][0] = 0;
            bpb[0][0] = 0.f; bpnb[0][0] = -INFINITY; bs[0][0] = 0.f;
            s_n = 1; s_nn = 1; s_nsel = 0; s_nvalid = 0;
            if constexpr (LM) { bL[0][0] = 0.f; bslot[0][0] = 0; spend[0] = 1; }      // the root's row: request 0 of the LM step before the first launch
        }
    } else if constexpr (LM) {                     // resume: the beam as the suspended launch left it
        const int* ra = rec + CTC_LM_RESUME_HEAD;
        if (tid < rec[R_N]) {
            bnode[0][tid] = ra[tid]; blast[0][tid] = ra[MAXB + tid]; bpar[0][tid] = ra[2 * MAXB + tid]; bdep[0][tid] = ra[3 * MAXB + tid];
            bpb[0][tid] = __int_as_float(ra[4 * MAXB + tid]); bpnb[0][tid] = __int_as_float(ra[5 * MAXB + tid]);
            bs[0][tid] = __int_as_float(ra[6 * MAXB + tid]); bL[0][tid] = __int_as_float(ra[7 * MAXB + tid]);
            bslot[0][tid] = ra[8 * MAXB + tid]; spend[tid] = ra[9 * MAXB + tid];
        }
        if (tid == 0) {
            s_n = rec[R_N]; s_nn = rec[R_NN]; s_nsel = 0; s_nvalid = 0;
            ncand0 = ((long long)rec[R_NCHI] << 32) | (unsigned)rec[R_NCLO];
            nreq = rec[R_NREQ];
        }
        t0 = rec[R_FRAME];
    } else if constexpr (STREAM) {                 // resume: the beam as the stream's last push with frames left it.  The LDS the radix select counts on is
        const int* ra = rec + CTC_STREAM_HEAD;     // set in every launch
        for (int i = tid; i < MAXV; i += CT) spos[i] = -1;
        hist[0][tid] = 0u;
        const int rn = rec[S_N] < beam ? rec[S_N] : beam;
        if (tid < rn) {
            bnode[0][tid] = ra[tid]; blast[0][tid] = ra[MAXB + tid]; bpar[0][tid] = ra[2 * MAXB + tid]; bdep[0][tid] = ra[3 * MAXB + tid];
            bpb[0][tid] = __int_as_float(ra[4 * MAXB + tid]); bpnb[0][tid] = __int_as_float(ra[5 * MAXB + tid]);
            bs[0][tid] = __int_as_float(ra[6 * MAXB + tid]);
        }
        if (tid == 0) {
            s_n = rn; s_nn = rec[S_NN]; s_nsel = 0; s_nvalid = 0;
            ncand0 = ((long long)rec[S_NCHI] << 32) | (unsigned)rec[S_NCLO];
        }
    }
    float nx[TPT];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int v = tid * TPT + q;
        nx[q] = (t0 < len && v < V) ? lrow[(size_t)t0 * V + v] : 0.f;
    }
    int cur = 0;
    long long ncand = ncand0;
    __syncthreads();
    if constexpr (LM) {
        // ---- the rows the LM step left as raw logits -> log softmax(x / lm_tmp) in the member's slot: logf(expf(x / lm_tmp - max) / sum), one wave per row,
        // lane l owns tokens l, 64 + l, ..; the sum is a fixed butterfly over the lanes' partial sums
        const int n0 = s_n;
        for (int r = wave; r < n0; r += CNW) {
            if (!spend[r]) continue;
            const int col = fz.slot[(size_t)b * beam + r];                          // the packed column of this rank's request (live, so >= 0)
            const float* src = fz.logits + (size_t)(col < 0 ? 0 : col) * V;
            float* dst = lmn + (size_t)bslot[0][r] * nf + fz.nls;
            float xv[MAXV / 64], mx = -INFINITY;
#pragma unroll
            for (int q = 0; q < MAXV / 64; ++q) {
                const int v = lane + 64 * q;
                xv[q] = v < V ? src[v] / fz.tmp : -INFINITY;
                mx = fmaxf(mx, xv[q]);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float sm = 0.f;
#pragma unroll
            for (int q = 0; q < MAXV / 64; ++q) { xv[q] = lane + 64 * q < V ? expf(xv[q] - mx) : 0.f; sm += xv[q]; }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) sm += __shfl_xor(sm, o);
#pragma unroll
            for (int q = 0; q < MAXV / 64; ++q)
                if (lane + 64 * q < V) dst[lane + 64 * q] = logf(xv[q] / sm);
        }
        __syncthreads();
        if (tid < MAXB) spend[tid] = 0;
    }

    for (int t = t0; t < len; ++t) {
        float x[TPT];
#pragma unroll
        for (int q = 0; q < TPT; ++q) x[q] = nx[q];
        if (t + 1 < len) {                         // prefetch frame t + 1 under this frame's work
#pragma unroll
            for (int q = 0; q < TPT; ++q) {
                const int v = tid * TPT + q;
                if (v < V) nx[q] = lrow[(size_t)(t + 1) * V + v];
            }
        }
        // ---- lp = (x / tmp).softmax().log() in fp32
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            x[q] = x[q] / a.tmp;
            if (v < V) m = fmaxf(m, x[q]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) sredm[wave] = m;
        __syncthreads();
        m = sredm[0];
#pragma unroll
        for (int w = 1; w < CNW; ++w) m = fmaxf(m, sredm[w]);
        float e[TPT], ssum = 0.f;
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            e[q] = v < V ? expf(x[q] - m) : 0.f;
            ssum += e[q];
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ssum += __shfl_xor(ssum, o);
        if (lane == 0) sreds[wave] = ssum;
        __syncthreads();
        ssum = sreds[0];
#pragma unroll
        for (int w = 1; w < CNW; ++w) ssum += sreds[w];
        unsigned key[TPT];
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            key[q] = 0u;
            if (v < V) {
                const float l = logf(e[q] / ssum);
                slp[v] = l;
                key[q] = okey(l);
            }
        }
        int n, S;
        if constexpr (!LM) {
        // ---- radix select: the K-th largest key (8 bits per pass); `need` = how many keys equal to it are taken
        unsigned prefix = 0u, pmask = 0u;
        int need = K;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            unsigned* h = hist[pass & 1];
#pragma unroll
            for (int q = 0; q < TPT; ++q)
                if (tid * TPT + q < V && (key[q] & pmask) == prefix) atomicAdd(h + ((key[q] >> shift) & 255u), 1u);
            hist[(pass + 1) & 1][tid] = 0u;
            __syncthreads();
            if (wave == 0) {                       // lane l holds digits 255 - 4 l .. 252 - 4 l (descending)
                unsigned hv[4], c = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { hv[j] = h[255 - 4 * lane - j]; c += hv[j]; }
                const int incl = wave_incl_scan((int)c, lane), excl = incl - (int)c;
                if (excl < need && incl >= need) {
                    int cum = excl, j = 0;
                    while (cum + (int)hv[j] < need) { cum += (int)hv[j]; ++j; }
                    s_digit = 255 - 4 * lane - j;
                    s_need = need - cum;
                }
            }
            __syncthreads();
            prefix |= (unsigned)s_digit << shift;
            pmask |= 255u << shift;
            need = s_need;
        }
        // ---- the K tokens: keys above the threshold, and the `need` lowest ids among the keys equal to it
        int nt = 0;
#pragma unroll
        for (int q = 0; q < TPT; ++q) nt += (tid * TPT + q < V && key[q] == prefix);
        const int incl = wave_incl_scan(nt, lane);
        if (lane == 63) sscan[wave] = incl;
        __syncthreads();
        int toff = incl - nt;
        for (int w = 0; w < wave; ++w) toff += sscan[w];
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int v = tid * TPT + q;
            if (v >= V) continue;
            bool sel = key[q] > prefix;
            if (key[q] == prefix) { sel = toff < need; ++toff; }
            if (sel) selk[atomicAdd(&s_nsel, 1)] = ((unsigned long long)key[q] << 32) | (0xffffffffu - (unsigned)v);
        }
        n = s_n;
        // parent member of every member (a compare of nodes: node identity is string identity)
        if (tid < n) {
            const int par = bpar[cur][tid];
            int pm = -1;
            if (par >= 0)
                for (int j = 0; j < n; ++j) if (bnode[cur][j] == par) pm = j;
            bpm[tid] = pm;
        }
        __syncthreads();
        if (tid < K) {                             // order the K tokens by (lp desc, id asc): one 64-bit compare per pair
            const unsigned long long kv = selk[tid];
            int r = 0;
#pragma unroll 8
            for (int j = 0; j < K; ++j) r += selk[j] > kv;
            const int v = (int)(0xffffffffu - (unsigned)kv);
            stop[r] = v;
            spos[v] = r;
        }
        S = 2 * n + n * beam;
        for (int j = 2 * n + tid; j < S; j += CT) { ck[j] = 0x7fffffff; ckey[j] = 0ull; }
        __syncthreads();
        // ---- members: exclusion masks, the member candidate (merges included) and the repeat extension
        if (tid < n) {
            const int i = tid, li = blast[cur][i];
            unsigned ex[3] = {0u, 0u, 0u};
            auto setb = [&](int p) { if (p >= 0) ex[p >> 5] |= 1u << (p & 31); };
            setb(spos[0]);
            if (li >= 0) setb(spos[li]);
            bool rep = li >= 0;
            for (int k = 0; k < n; ++k)
                if (bpm[k] == i) {
                    const int lk = blast[cur][k];
                    setb(spos[lk]);
                    if (lk == li) rep = false;     // P last(P) is a member: the repeat term goes to that member
                }
            bexcl[i][0] = ex[0]; bexcl[i][1] = ex[1]; bexcl[i][2] = ex[2];
            const float si = bs[cur][i];
            float nb = li >= 0 ? slp[li] + bpnb[cur][i] : -INFINITY;
            const int pm = bpm[i];
            if (pm >= 0) nb = lse(nb, slp[li] + (li == blast[cur][pm] ? bpb[cur][pm] : bs[cur][pm]));
            const float bb = slp[0] + si;
            cs[i] = lse(bb, nb); cpb[i] = bb; cpnb[i] = nb; ck[i] = ((li + 1) << 16) | i; ckey[i] = cand_key(cs[i], ck[i]);
            if (rep) {
                const float r = slp[li] + bpb[cur][i];
                cs[n + i] = r; cpb[n + i] = -INFINITY; cpnb[n + i] = r; ck[n + i] = ((li + 1) << 16) | (n + i * V + li);
                ckey[n + i] = cand_key(r, ck[n + i]);
            } else {
                ck[n + i] = 0x7fffffff; ckey[n + i] = 0ull;
            }
        }
        __syncthreads();
        // ---- plain extensions: member i's r-th plain token in top-K order, r < beam
        for (int j = tid; j < n * K; j += CT) {
            const int i = j / K, p = j - i * K;
            const unsigned w = bexcl[i][p >> 5];
            if (w & (1u << (p & 31))) continue;
            int r = __popc(~w & ((1u << (p & 31)) - 1u));
            for (int q = 0; q < (p >> 5); ++q) r += __popc(~bexcl[i][q]);
            if (r >= beam) continue;
            const int c = stop[p], slot = 2 * n + i * beam + r;
            const float nb = slp[c] + bs[cur][i];
            const int k = ((c + 1) << 16) | (n + i * V + c);
            cs[slot] = nb; cpb[slot] = -INFINITY; cpnb[slot] = nb; ck[slot] = k; ckey[slot] = cand_key(nb, k);
        }
        __syncthreads();
        if (tid < K) spos[stop[tid]] = -1;
        } else {
        n = s_n;
        if (tid < n) {
            const int par = bpar[cur][tid];
            int pm = -1;
            if (par >= 0)
                for (int j = 0; j < n; ++j) if (bnode[cur][j] == par) pm = j;
            bpm[tid] = pm;
        }
        S = 2 * n + n * beam;
        for (int j = 2 * n + tid; j < S; j += CT) { ck[j] = 0x7fffffff; ckey[j] = 0ull; }
        __syncthreads();
        // ---- members: the member candidate (merges included) and the repeat extension, ranked by total
        if (tid < n) {
            const int i = tid, li = blast[cur][i], di = bdep[cur][i];
            bool rep = li >= 0;
            for (int k = 0; k < n; ++k)
                if (bpm[k] == i && blast[cur][k] == li) rep = false;     // P last(P) is a member: the repeat term goes to that member
            const float si = bs[cur][i], Li = bL[cur][i];
            float nb = li >= 0 ? slp[li] + bpnb[cur][i] : -INFINITY;
            const int pm = bpm[i];
            if (pm >= 0) nb = lse(nb, slp[li] + (li == blast[cur][pm] ? bpb[cur][pm] : bs[cur][pm]));
            const float bb = slp[0] + si;
            cs[i] = lse(bb, nb); cpb[i] = bb; cpnb[i] = nb; cL[i] = Li; ck[i] = ((li + 1) << 16) | i;
            ckey[i] = cand_key(fused_total(cs[i], Li, di, fz.w, fz.bonus), ck[i]);
            if (rep) {
                const float r = slp[li] + bpb[cur][i];
                const float Lq = Li + lmn[(size_t)bslot[cur][i] * nf + fz.nls + li];
                cs[n + i] = r; cpb[n + i] = -INFINITY; cpnb[n + i] = r; cL[n + i] = Lq; ck[n + i] = ((li + 1) << 16) | (n + i * V + li);
                ckey[n + i] = cand_key(fused_total(r, Lq, di + 1, fz.w, fz.bonus), ck[n + i]);
            } else {
                ck[n + i] = 0x7fffffff; ckey[n + i] = 0ull;
            }
        }
        // ---- plain extensions: one wave per member; lane l owns tokens l, 64 + l, ..; `beam` rounds of a wave-wide maximum of (a_P desc, id asc) over the
        // member's plain tokens (not blank, not last(P), P c not a member), a_P[c] = lp[c] + w row_P[c]
        for (int i = wave; i < n; i += CNW) {
            const float* row = lmn + (size_t)bslot[cur][i] * nf + fz.nls;
            const int li = blast[cur][i], di = bdep[cur][i];
            const float si = bs[cur][i], Li = bL[cur][i];
            unsigned avail = 0u, akey[MAXV / 64];
#pragma unroll
            for (int q = 0; q < MAXV / 64; ++q) {
                const int v = lane + 64 * q;
                akey[q] = 0u;
                if (v < V) {
                    akey[q] = okey(lm_scaled_sum(slp[v], fz.w, row[v]));
                    if (v != 0 && v != li) avail |= 1u << q;
                }
            }
            for (int k = 0; k < n; ++k)
                if (bpm[k] == i) {
                    const int lk = blast[cur][k];
                    if ((lk & 63) == lane) avail &= ~(1u << (lk >> 6));
                }
            for (int r = 0; r < beam; ++r) {
                unsigned bk = 0u;
                int bq = -1;
#pragma unroll
                for (int q = 0; q < MAXV / 64; ++q)
                    if (((avail >> q) & 1u) && (bq < 0 || akey[q] > bk)) { bk = akey[q]; bq = q; }
                unsigned long long p = bq >= 0 ? ((unsigned long long)bk << 32) | (0xffffffffu - (unsigned)(lane + 64 * bq)) : 0ull;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const unsigned long long op = __shfl_xor(p, o);
                    p = op > p ? op : p;
                }
                if (p == 0ull) break;              // wave-uniform: no plain token is left
                const int c = (int)(0xffffffffu - (unsigned)p);
                if ((c & 63) == lane) avail &= ~(1u << (c >> 6));
                if (lane == 0) {
                    const int slot = 2 * n + i * beam + r;
                    const float nb = slp[c] + si, Lq = Li + row[c];
                    const int k = ((c + 1) << 16) | (n + i * V + c);
                    cs[slot] = nb; cpb[slot] = -INFINITY; cpnb[slot] = nb; cL[slot] = Lq; ck[slot] = k;
                    ckey[slot] = cand_key(fused_total(nb, Lq, di + 1, fz.w, fz.bonus), k);
                }
            }
        }
        __syncthreads();
        }
        // ---- selection: rank = number of candidates before this one (one 64-bit compare per pair; empty slots never count)
        for (int j = tid; j < S; j += CT) {
            const unsigned long long kj = ckey[j];
            if (kj == 0ull) continue;
            int r = 0;
#pragma unroll 8
            for (int q = 0; q < S; ++q) r += ckey[q] > kj;
            if (r < beam) nsel[r] = j;
            atomicAdd(&s_nvalid, 1);
        }
        __syncthreads();
        // ---- the next beam: nodes of new prefixes (old node if the string was seen before), trace
        if (wave == 0) {
            const int nv = s_nvalid, nnew = nv < beam ? nv : beam, nn0 = s_nn, nxt = cur ^ 1;
            int node = -1, last = -1, par = -1, dep = 0;
            float pb = -INFINITY, pnb = -INFINITY, sc = -INFINITY;
            bool isnew = false;
            unsigned long long hk = 0ull;
            float Lm = 0.f;                        // the fused search: L, LM slot (entrants: their parent's), entered the beam as an extension
            int lslot = 0;
            bool enters = false;
            if (lane < nnew) {
                const int j = nsel[lane], kj = ck[j], idx = kj & 0xffff;
                pb = cpb[j]; pnb = cpnb[j]; sc = cs[j];
                if constexpr (LM) Lm = cL[j];
                if (idx < n) {
                    node = bnode[cur][idx]; last = blast[cur][idx]; par = bpar[cur][idx]; dep = bdep[cur][idx];
                    if constexpr (LM) lslot = bslot[cur][idx];
                } else {
                    const int i = (idx - n) / V, c = idx - n - i * V;
                    if constexpr (LM) { lslot = bslot[cur][i]; enters = true; }
                    par = bnode[cur][i]; last = c; dep = bdep[cur][i] + 1;
                    hk = ((unsigned long long)(unsigned)par << 32) | (unsigned)c;
                    unsigned sl = hash_slot(par, c, hmask);
                    for (unsigned pr = 0; pr <= hmask; ++pr) {
                        const unsigned long long k = hload(hkeys + sl);
                        if (k == hk) { node = __hip_atomic_load(hvals + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                        if (k == HEMPTY) break;
                        sl = (sl + 1) & hmask;
                    }
                    isnew = node < 0;
                }
            }
            const unsigned long long nm = __ballot(isnew);
            if (isnew) {
                node = nn0 + __popcll(nm & ((1ull << lane) - 1ull));
                nodes[node] = make_int4(par, last, dep, LM ? __float_as_int(Lm) : 0);      // L(P): set when the node is created, read ever after
                unsigned sl = hash_slot(par, last, hmask);
                for (unsigned pr = 0; pr <= hmask; ++pr) {
                    if (atomicCAS(hkeys + sl, HEMPTY, hk) == HEMPTY) {
                        __hip_atomic_store(hvals + sl, node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    sl = (sl + 1) & hmask;
                }
            }
            if (lane < beam) trace[(size_t)t * beam + lane] = make_int4(node, __float_as_int(pb), __float_as_int(pnb), __float_as_int(sc));
            if (lane < nnew) {
                bnode[nxt][lane] = node; blast[nxt][lane] = last; bpar[nxt][lane] = par; bdep[nxt][lane] = dep;
                bpb[nxt][lane] = pb; bpnb[nxt][lane] = pnb; bs[nxt][lane] = sc;
            }
            if constexpr (LM) {
                if (enters && !isnew) Lm = __int_as_float(nodes[node].w);      // a prefix seen before: the L its node holds
                // an entrant takes the lowest of the slots 1 .. 2 beam that no member of the old beam holds (bit s - 1 = slot s): its parent's state stays
                // valid until the LM step has run, and no survivor's slot is taken
                unsigned long long used = 0ull;
                for (int k = 0; k < n; ++k)
                    if (bslot[cur][k] > 0) used |= 1ull << (bslot[cur][k] - 1);
                const unsigned long long em = __ballot(enters);
                const bool susp = em != 0ull && t + 1 < len;                   // after the last frame no row is needed any more
                int myslot = lslot;
                if (enters) {
                    unsigned long long fr = ~used & (2 * beam >= 64 ? ~0ull : (1ull << (2 * beam)) - 1ull);
                    for (int k = __popcll(em & ((1ull << lane) - 1ull)); k > 0; --k) fr &= fr - 1ull;
                    myslot = __ffsll((long long)fr);                           // >= 1: at most beam bits are used, at most beam candidates enter
                }
                if (lane < beam) {
                    trace2[(size_t)t * beam + lane] = lane < nnew ? make_float2(Lm, fused_total(sc, Lm, dep, fz.w, fz.bonus)) : make_float2(0.f, -INFINITY);
                    if (susp) fz.req[(size_t)b * beam + lane] = enters ? make_int4(last, lslot, myslot, 1) : make_int4(0, 0, 0, 0);
                }
                if (lane < nnew) { bL[nxt][lane] = Lm; bslot[nxt][lane] = myslot; spend[lane] = enters ? 1 : 0; }
                if (lane == 0) { s_susp = susp ? 1 : 0; nreq += susp ? __popcll(em) : 0; }
            }
            if (lane == 0) {
                ncand += nv;
                s_nn = nn0 + __popcll(nm); s_n = nnew; s_nvalid = 0; s_nsel = 0;
            }
        }
        __syncthreads();
        cur ^= 1;
        if constexpr (LM) {
            if (s_susp) {                          // workgroup-uniform: save the beam, wait for the LM step
                int* ra = rec + CTC_LM_RESUME_HEAD;
                if (tid < s_n) {
                    ra[tid] = bnode[cur][tid]; ra[MAXB + tid] = blast[cur][tid]; ra[2 * MAXB + tid] = bpar[cur][tid]; ra[3 * MAXB + tid] = bdep[cur][tid];
                    ra[4 * MAXB + tid] = __float_as_int(bpb[cur][tid]); ra[5 * MAXB + tid] = __float_as_int(bpnb[cur][tid]);
                    ra[6 * MAXB + tid] = __float_as_int(bs[cur][tid]); ra[7 * MAXB + tid] = __float_as_int(bL[cur][tid]);
                    ra[8 * MAXB + tid] = bslot[cur][tid]; ra[9 * MAXB + tid] = spend[tid];
                }
                if (tid == 0) {
                    rec[R_PHASE] = 1; rec[R_FRAME] = t + 1; rec[R_N] = s_n; rec[R_NN] = s_nn;
                    rec[R_NCLO] = (int)(unsigned)(ncand & 0xffffffffll); rec[R_NCHI] = (int)(ncand >> 32); rec[R_NREQ] = nreq;
                    atomicAdd(fz.active, 1);
                }
                return;
            }
        }
    }
    const int n = s_n;
    if constexpr (STREAM) {
    // ---- the record (only after a push with frames), then the outputs of the beam as it stands
    if (len > 0) {
        int* ra = rec + CTC_STREAM_HEAD;
        if (tid < n) {
            ra[tid] = bnode[cur][tid]; ra[MAXB + tid] = blast[cur][tid]; ra[2 * MAXB + tid] = bpar[cur][tid]; ra[3 * MAXB + tid] = bdep[cur][tid];
            ra[4 * MAXB + tid] = __float_as_int(bpb[cur][tid]); ra[5 * MAXB + tid] = __float_as_int(bpnb[cur][tid]);
            ra[6 * MAXB + tid] = __float_as_int(bs[cur][tid]);
        }
        if (tid == 0) {
            rec[S_FRAMES] = consumed + len; rec[S_N] = n; rec[S_NN] = s_nn;
            rec[S_NCLO] = (int)(unsigned)(ncand & 0xffffffffll); rec[S_NCHI] = (int)(ncand >> 32);
            sz.primed[sid] = 1;
        }
    }
    const int nbest = sz.nbest, MT = sz.max_tokens;
    if (tid < nbest) {                             // token_len is the true depth; tokens beyond max_tokens are not written
        int* out = a.tokens + ((size_t)b * nbest + tid) * MT;
        int d = 0;
        float sc = -INFINITY;
        if (tid < n) {
            d = bdep[cur][tid];
            sc = bs[cur][tid];
            int node = bnode[cur][tid];
            for (int i = d - 1; i >= 0; --i) {
                const int4 nd = nodes[node];
                if (i < MT) out[i] = nd.y;
                node = nd.x;
            }
        }
        a.token_len[(size_t)b * nbest + tid] = d;
        a.score[(size_t)b * nbest + tid] = sc;
    }
    for (int j = tid; j < nbest * MT; j += CT) {
        const int r = j / MT, i = j - r * MT;
        if (i >= (r < n ? bdep[cur][r] : 0)) a.tokens[((size_t)b * nbest + r) * MT + i] = 0;
    }
    // the longest common prefix of all members (one wave): lift every member's node to the smallest depth, then step the parents together until all agree.
    // Node identity is string identity, so equal nodes at equal depth are equal prefixes; at depth 0 every node is the root
    if (wave == 0) {
        int node = lane < n ? bnode[cur][lane] : 0, d = lane < n ? bdep[cur][lane] : 0x7fffffff, dmin = d;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int od = __shfl_xor(dmin, o); dmin = od < dmin ? od : dmin; }
        if (lane < n)
            for (; d > dmin; --d) node = nodes[node].x;
        while (dmin > 0 && __ballot(lane < n && node != __shfl(node, 0)) != 0ull) {      // wave-uniform; lane 0 is always a member
            if (lane < n) node = nodes[node].x;
            --dmin;
        }
        if (lane == 0) sz.stable_len[b] = dmin;
    }
    if (tid == 0) {
        a.stats[4 * b + 0] = len;
        a.stats[4 * b + 1] = (int)(ncand < 0x7fffffffll ? ncand : 0x7fffffffll);
        a.stats[4 * b + 2] = s_nn;
        a.stats[4 * b + 3] = consumed + len;
    }
    } else {
    // ---- outputs in rank order: tokens by walking the trie from each member's node
    if (tid < beam) {
        int* out = a.tokens + ((size_t)b * beam + tid) * T;
        int d = 0;
        float sc = -INFINITY;
        if (tid < n) {
            d = bdep[cur][tid];
            sc = bs[cur][tid];
            int node = bnode[cur][tid];
            for (int i = d - 1; i >= 0; --i) { const int4 nd = nodes[node]; out[i] = nd.y; node = nd.x; }
        }
        a.token_len[(size_t)b * beam + tid] = d;
        a.score[(size_t)b * beam + tid] = sc;
        if constexpr (LM) {
            const float Lm = tid < n ? bL[cur][tid] : 0.f;
            fz.lm_score[(size_t)b * beam + tid] = Lm;
            fz.total[(size_t)b * beam + tid] = tid < n ? fused_total(sc, Lm, d, fz.w, fz.bonus) : -INFINITY;
            fz.req[(size_t)b * beam + tid] = make_int4(0, 0, 0, 0);           // nothing to ask of the rounds other utterances still need
        }
    }
    for (int j = tid; j < beam * T; j += CT) {
        const int r = j / T, i = j - r * T;
        if (i >= (r < n ? bdep[cur][r] : 0)) a.tokens[((size_t)b * beam + r) * T + i] = 0;
    }
    if (tid == 0) {
        a.stats[4 * b + 0] = len;
        a.stats[4 * b + 1] = (int)(ncand < 0x7fffffffll ? ncand : 0x7fffffffll);
        a.stats[4 * b + 2] = s_nn;
        a.stats[4 * b + 3] = LM ? nreq : 0;
        if constexpr (LM) rec[R_PHASE] = 2;
    }
    }
