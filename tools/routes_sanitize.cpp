// Stand-alone host program for a sanitizer run of csrc/routes.h (not part of the test suite): front_route / front_scratch, block_routes and attention_route, and
// the split schedule's exact_forward_routes / exact_block_routes / exact_attention_split, on a hand-filled two-block handle under a sweep of the options they read.  routes.h calls the kernels' own `*_supported` predicates, so the program links the product
// objects of an in-tree build; no kernel is launched and no device is needed.  From the repository root, after `python -m efficientconformer_amd._build`:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -c tools/routes_sanitize.cpp -o routes_sanitize.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined routes_sanitize.o $(ls efficientconformer_amd/build/*.o | grep -v -e _dbg.o -e _pk.o -e debug.o) -o routes_sanitize
//   ./routes_sanitize
#include "../efficientconformer_amd/csrc/routes.h"

#include <cstdio>

int main() {
    static const uint16_t image = 0;             // "packed" = any non-null pointer
    static const float consts = 0.f;
    EcEncoder e;
    e.blocks = {EcBlock{120, 360, 4, 4, 15, 3, 512, 2}, EcBlock{360, 360, 4, 4, 15, 1, 512, 1}};      // dim_model, dim_expand, ff_ratio, heads, kernel, group, max_pos, stride
    e.cfg = EcConfig{};
    e.cfg.n_mels = 80; e.cfg.sub_layers = 1; e.cfg.sub_filters[0] = 120; e.cfg.num_blocks = 2; e.cfg.blocks = e.blocks.data();
    e.bw.assign(2, BlockW());
    e.bw[0].chain_in = e.bw[0].chain_out = true;
    long long sum = 0;
    int calls = 0;
    for (int layers = 1; layers <= 2; ++layers)
    for (int images = 0; images < 8; ++images)
    for (int fuse = 0; fuse <= 3; ++fuse)
    for (int opts = 0; opts < 64; ++opts)
    for (int ragged = 0; ragged < 2; ++ragged) {
        e.cfg.sub_layers = layers; e.cfg.sub_filters[1] = layers == 2 ? 120 : 0;
        e.sub3.wimg = images & 1 ? &image : nullptr;
        e.lin_rs = images & 2 ? reinterpret_cast<const bf16_t*>(&image) : nullptr;
        e.lin_fused = images & 4 ? reinterpret_cast<const bf16_t*>(&image) : nullptr;
        e.bw[0].cc_full = images & 1 ? &consts : nullptr;
        e.fuse_subsample = fuse;
        e.sub3_auto = opts & 1; e.fuse_chain = (opts & 2) != 0; e.chain_pair = opts & 4 ? 5 : 0; e.tiled_auto = (opts >> 3) & 3 ? ((opts >> 3) & 3) - 1 : 1;
        e.wide_gemm = opts & 32 ? 2 : 0; e.attention_v2 = opts % 3; e.dwconv_mfma = opts % 3; e.chain_max_dim = opts & 8 ? 128 : 256; e.chain_full_max = opts & 16 ? 0 : 192;
        e.tiled_auto_on = tiled_auto_rule(&e);
        const FrontScratch fs = front_scratch(&e, ragged != 0, 3, 97, 49);
        sum += front_route(&e, ragged != 0) + (long long)(fs.sub + fs.sub1 + fs.xrect);
        for (size_t k = 0; k < e.blocks.size(); ++k) {
            const BlockRoutes r = block_routes(&e, k);
            sum += r.head + 3 * r.tail + r.ffn1_fused + r.qkv_rs + r.chain_b + r.outp_rs + r.pw1_rs + r.dw_mfma + r.res_rs + r.pw2_rs + r.ffn2_fused;
            for (int dpad = 32; dpad <= 192; dpad += 32)
                for (int streaming = 0; streaming < 2; ++streaming) {
                    const AttentionRoute a = attention_route(&e, dpad, ragged != 0, streaming != 0);
                    sum += a.waves + (a.refusal ? a.refusal[0] : 0);
                }
        }
        ++calls;
    }
    // the label-exact split schedule: which images exist x its four options x the kind of forward x the shape fact of the merged head
    e.blocks[1] = EcBlock{120, 120, 4, 4, 15, 3, 512, 1};
    e.blocks[0].dim_expand = 120; e.blocks[0].conv_stride = 1;
    for (int mode = 0; mode < 2; ++mode)
    for (int images = 0; images < 64; ++images)
    for (int opts = 0; opts < 16; ++opts)
    for (int kind = 0; kind < 3; ++kind)
    for (int carry = 0; carry < 2; ++carry) {
        e.exact_split = mode != 0; e.cfg.sub_layers = 1; e.cfg.causal = images & 1;
        e.xsub.wimg = images & 1 ? &image : nullptr;
        for (int k = 0; k < 2; ++k) {
            BlockW& W = e.bw[k];
            W.xc_f[0] = images & (2 << k) ? &image : nullptr; W.xc_f[1] = images & (8 << k) ? &image : nullptr;
            W.xc_in = W.xc_f[0] && (images & 32); W.xc_out = W.xc_f[1] != nullptr;
        }
        e.split_chain = opts & 1; e.split_ffn = (opts >> 1) & 1; e.split_sublin = (opts >> 2) & 1; e.trace_fused = (opts & 8) != 0;
        const ExactForwardRoutes f = exact_forward_routes(&e, kind == 1, kind == 2);
        sum += f.fused + 2 * f.sublin + 4 * f.ffn + 8 * f.chains + (f.refusal ? f.refusal[0] : 0) + split_fused_ok(&e);
        for (size_t k = 0; k < e.blocks.size(); ++k) {
            const ExactBlockRoutes r = exact_block_routes(&e, f, k, carry != 0, carry != 0);
            sum += r.head + 3 * r.tail + r.ffn1_fused + r.chain_b + r.ffn2_fused + exact_attention_split(&e, 90, images * 2048LL);
        }
        ++calls;
    }
    printf("routes_sanitize: %d option sets, checksum %lld\n", calls, sum);
    return 0;
}
