// The ConvNeXt net: weight banks of its ConvBlocks and the schedule of one forward (networks/new_unet.py:332-362, 365-430).
#include "runtime_internal.h"

// encoder_convs[0].blocks[0] projects cat[y, warped features] 96 -> 48 (new_unet.py:381-382): the features' half in the feature
// warp (warp.hip warp48_proj_kernel: `featw` then holds W_f warp(f) + bias), y's half in the epilogue of the block that forms y
bool next_pf_pre(const rvdd_t* h) {
    return h->is_next() && h->has_feat() && !h->opt.no_warp && h->opt.next_projfuse && h->opt.next_split && h->opt.next_pipe &&
           h->nx[NX_PRE].w.fc1_h && h->nx[NX_ENC0_0].half[0].frag && h->nx[NX_ENC0_0].half[1].frag;
}

int finalize_convnext(rvdd_t* h) {
    auto up = [&](const float** dst, const std::vector<float>& v) {
        float* p = nullptr;
        int rc = upload(h, &p, v);
        *dst = p;
        return rc;
    };
    for (int bi = h->has_feat() ? 0 : 1; bi < NX_COUNT; ++bi) {
        const std::string b = kNxNames[bi];
        NextBlk nb;
        const int pc = next_proj_cin(h, b);
        if (pc) {
            const HostTensor& pw = h->staged.at(b + ".proj.weight");
            nb.c1 = pc == 96 ? 48 : kNetInC;
            nb.c2 = pc == 96 ? 48 : 0;
            const int NJ = (nb.c1 + nb.c2) / 16;
            std::vector<float> a((size_t)NJ * 3 * 16 * 16, 0.f);
            for (int j = 0; j < NJ; ++j)
                for (int m = 0; m < 3; ++m)
                    for (int lr = 0; lr < 16; ++lr)
                        for (int g = 0; g < 4; ++g)
                            for (int i = 0; i < 4; ++i) {
                                const int c = 16 * j + 4 * g + i;
                                if (c >= pc) continue;
                                a[((((size_t)j * 3 + m) * 16 + lr) * 4 + g) * 4 + i] = pw.data[(size_t)(16 * m + lr) * pc + c];
                            }
            RC(up(&nb.w.proj_w, a));
            RC(up(&nb.w.proj_b, h->staged.at(b + ".proj.bias").data));
            if (pc == 96) {
                // the two halves W[:, 0:48], W[:, 48:96] as split-f16 fragments in fc1's arrangement (three row blocks of 16 outputs:
                // Fa = [wh0 wh1], Fb = [wl0 wl1], Fc = [wh2 wl2] over the input blocks 0, 1, 2), each scaled to |w'| in (1/2, 1]
                for (int hf = 0; hf < 2; ++hf) {
                    float mx = 0.f;
                    for (int o = 0; o < 48; ++o)
                        for (int c = 0; c < 48; ++c) mx = std::max(mx, std::fabs(pw.data[(size_t)o * 96 + 48 * hf + c]));
                    int sft = 0;
                    if (mx > 0.f && std::isfinite(mx)) sft = std::max(-15, std::min(15, (int)std::floor(std::log2(1.0 / mx))));
                    const float scale = std::ldexp(1.0f, sft);
                    std::vector<uint16_t> a1((size_t)3 * 1536, 0);
                    for (int m = 0; m < 3; ++m)
                        for (int kk = 0; kk < 4; ++kk)
                            for (int lr = 0; lr < 16; ++lr)
                                for (int e = 0; e < 8; ++e) {
                                    const int lane = 16 * kk + lr, row = 16 * m + lr, i = e & 3, blk = e >> 2;
                                    auto halves = [](float w, uint16_t& hi, uint16_t& lo) {
                                        hi = f16_bits(w, true);
                                        lo = f16_bits(w - f16_value(hi), false);
                                    };
                                    uint16_t h0, l0, h2, l2;
                                    halves(pw.data[(size_t)row * 96 + 48 * hf + 16 * blk + 4 * kk + i] * scale, h0, l0);
                                    halves(pw.data[(size_t)row * 96 + 48 * hf + 32 + 4 * kk + i] * scale, h2, l2);
                                    uint16_t* base = &a1[(size_t)m * 1536];
                                    base[lane * 8 + e] = h0;
                                    base[512 + lane * 8 + e] = l0;
                                    base[1024 + lane * 8 + e] = blk == 0 ? h2 : l2;
                                }
                    std::vector<float> f1(a1.size() / 2);
                    std::memcpy(f1.data(), a1.data(), a1.size() * 2);
                    RC(up(&nb.half[hf].frag, f1));
                    nb.half[hf].inv_e = -sft;
                    nb.half[hf].bias = nb.w.proj_b;      // applied by whichever half has nothing to add to (NextProj::add)
                }
            }
        }
        {   // depth-wise 7x7: [48][1][7][7] -> [49][48]
            const HostTensor& dw = h->staged.at(b + ".block.0.weight");
            std::vector<float> a((size_t)49 * 48);
            for (int c = 0; c < 48; ++c)
                for (int t = 0; t < 49; ++t) a[(size_t)t * 48 + c] = dw.data[(size_t)c * 49 + t];
            RC(up(&nb.w.dw_w, a));
            RC(up(&nb.w.dw_b, h->staged.at(b + ".block.0.bias").data));
        }
        RC(up(&nb.w.ln_w, h->staged.at(b + ".block.1.weight").data));
        RC(up(&nb.w.ln_b, h->staged.at(b + ".block.1.bias").data));
        {   // fc1 [192][48] -> [j][m][lane = 16g+lr][i] = W1[16m+lr][16j+4g+i]
            const HostTensor& w1 = h->staged.at(b + ".block.2.weight");
            std::vector<float> a((size_t)192 * 48);
            for (int j = 0; j < 3; ++j)
                for (int m = 0; m < 12; ++m)
                    for (int lr = 0; lr < 16; ++lr)
                        for (int g = 0; g < 4; ++g)
                            for (int i = 0; i < 4; ++i)
                                a[(((size_t)j * 12 + m) * 64 + g * 16 + lr) * 4 + i] =
                                    w1.data[(size_t)(16 * m + lr) * 48 + 16 * j + 4 * g + i];
            RC(up(&nb.w.fc1_w, a));
            RC(up(&nb.w.fc1_b, h->staged.at(b + ".block.2.bias").data));
        }
        {   // fc2 [48][192] -> [m][mo][lane = 16g+lr][r] = W2[16mo+lr][16m+4g+r]
            const HostTensor& w2 = h->staged.at(b + ".block.4.weight");
            std::vector<float> a((size_t)192 * 48);
            for (int m = 0; m < 12; ++m)
                for (int mo = 0; mo < 3; ++mo)
                    for (int lr = 0; lr < 16; ++lr)
                        for (int g = 0; g < 4; ++g)
                            for (int r = 0; r < 4; ++r)
                                a[(((size_t)m * 3 + mo) * 64 + g * 16 + lr) * 4 + r] =
                                    w2.data[(size_t)(16 * mo + lr) * 192 + 16 * m + 4 * g + r];
            RC(up(&nb.w.fc2_w, a));
            RC(up(&nb.w.fc2_b, h->staged.at(b + ".block.4.bias").data));
        }
        RC(up(&nb.w.ls, h->staged.at(b + ".layerscale.layerscale").data));
        {   // the same two matrices for the fused kernel's split-f16 MLP (convnext.hip SPLIT): w' = 2^s w, hi = f16(w') toward
            // zero, lo = f16(w' - hi); fragments in the k order the kernel's register pairs have
            const HostTensor& w1 = h->staged.at(b + ".block.2.weight");       // [192][48]
            const HostTensor& w2 = h->staged.at(b + ".block.4.weight");       // [48][192]
            auto pow2_scale = [](const std::vector<float>& v) {
                float mx = 0.f;
                for (float x : v) mx = std::max(mx, std::fabs(x));
                int sft = 0;
                if (mx > 0.f && std::isfinite(mx)) sft = (int)std::floor(std::log2(1.0 / mx));      // |w'| in (0.5, 1]
                return sft;
            };
            const int s1 = pow2_scale(w1.data), s2 = pow2_scale(w2.data);
            // The split form is used only where its f16 halves provably stay in range, whatever the frames are: the LayerNorm
            // bounds its output (|z_c| <= sqrt(47) for 48 channels, so |y_c| <= 6.86 |ln_w_c| + |ln_b_c|), that bounds fc1's
            // scaled sums, and |GELU(v)| <= |v|.  A block whose weights break the bound (or whose scales would push the scaled
            // GELU's constants out of the normal f32 range: |s| <= 15) keeps fc1_h null and runs the f32-MFMA form.
            bool split_ok = std::abs(s1) <= 15 && std::abs(s2) <= 15;
            {
                const std::vector<float>& lw = h->staged.at(b + ".block.1.weight").data;
                const std::vector<float>& lb = h->staged.at(b + ".block.1.bias").data;
                const std::vector<float>& b1 = h->staged.at(b + ".block.2.bias").data;
                double ymax[48], worst_y = 0.0, worst_h = 0.0;
                for (int c = 0; c < 48; ++c) {
                    ymax[c] = 6.86 * std::fabs((double)lw[c]) + std::fabs((double)lb[c]);
                    worst_y = std::max(worst_y, ymax[c]);
                }
                for (int j = 0; j < 192; ++j) {
                    double acc = std::fabs((double)b1[j]);
                    for (int c = 0; c < 48; ++c) acc += std::fabs((double)w1.data[(size_t)j * 48 + c]) * ymax[c];
                    worst_h = std::max(worst_h, acc * std::ldexp(1.0, s1));
                }
                if (!(worst_y < 32768.0) || !(worst_h < 32768.0)) split_ok = false;      // also catches NaN / inf weights
            }
            nb.w.fc1_scale = std::ldexp(1.0f, s1);
            nb.w.fc1_inv = std::ldexp(1.0f, -s1);
            nb.w.fc2_scale = std::ldexp(1.0f, s2);
            nb.w.fc2_inv = std::ldexp(1.0f, -s2);
            {   // the GELU on fc1's scaled accumulator (convnext.hip gelu_phi4_scaled): coefficients of gelu_phi4 times powers of s
                static const float C[6] = {2.992418740177527e-05f, -0.0007398742018267512f, 0.007977462373673916f,
                                           -0.05323818698525429f, -0.45891568064689636f, -1.1511471271514893f};
                for (int i = 0; i < 6; ++i) nb.w.gelu_c[i][0] = nb.w.gelu_c[i][1] = std::ldexp(C[i], -s1 * (6 - i));
                nb.w.gelu_c[6][0] = nb.w.gelu_c[6][1] = std::ldexp(6.36f, s1);
            }
            auto halves = [](float w, uint16_t& hi, uint16_t& lo) {
                hi = f16_bits(w, true);
                lo = f16_bits(w - f16_value(hi), false);
            };
            std::vector<uint16_t> a1((size_t)12 * 1536, 0), a2((size_t)6 * 3 * 2 * 512, 0);
            for (int m = 0; m < 12; ++m)
                for (int kk = 0; kk < 4; ++kk)
                    for (int lr = 0; lr < 16; ++lr)
                        for (int e = 0; e < 8; ++e) {
                            const int lane = 16 * kk + lr, row = 16 * m + lr, i = e & 3, blk = e >> 2;
                            uint16_t h0, l0, h2, l2;
                            halves(w1.data[(size_t)row * 48 + 16 * blk + 4 * kk + i] * nb.w.fc1_scale, h0, l0);      // blocks 0 / 1
                            halves(w1.data[(size_t)row * 48 + 32 + 4 * kk + i] * nb.w.fc1_scale, h2, l2);            // block 2
                            uint16_t* base = &a1[(size_t)m * 1536];
                            base[lane * 8 + e] = h0;                          // Fa = [wh0 wh1]
                            base[512 + lane * 8 + e] = l0;                    // Fb = [wl0 wl1]
                            base[1024 + lane * 8 + e] = blk == 0 ? h2 : l2;   // Fc = [wh2 wl2]
                        }
            for (int p = 0; p < 6; ++p)
                for (int mo = 0; mo < 3; ++mo)
                    for (int kk = 0; kk < 4; ++kk)
                        for (int lr = 0; lr < 16; ++lr)
                            for (int e = 0; e < 8; ++e) {
                                const int lane = 16 * kk + lr, hid = 16 * (2 * p + (e >> 2)) + 4 * kk + (e & 3);
                                uint16_t hi, lo;
                                halves(w2.data[(size_t)(16 * mo + lr) * 192 + hid] * nb.w.fc2_scale, hi, lo);
                                uint16_t* base = &a2[(size_t)((p * 3 + mo) * 2) * 512];
                                base[lane * 8 + e] = hi;                      // Gh
                                base[512 + lane * 8 + e] = lo;                // Gl
                            }
            std::vector<float> f1(a1.size() / 2), f2(a2.size() / 2);
            std::memcpy(f1.data(), a1.data(), a1.size() * 2);
            std::memcpy(f2.data(), a2.data(), a2.size() * 2);
            if (split_ok) {
                RC(up(&nb.w.fc1_h, f1));
                RC(up(&nb.w.fc2_h, f2));
            }
        }
        h->nx[bi] = nb;
    }
    RC(upload(h, &h->w_out, h->staged.at("postprocessing.1.weight").data));
    RC(upload(h, &h->b_out, h->staged.at("postprocessing.1.bias").data));
    return RVDD_OK;
}

// The sequences of `run` on stream s.
int run_convnext(rvdd_t* h, const NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
                 float* out_nhwc4, hipStream_t s) {
    const bool feat = h->has_feat();
    const int B = run.n;
    Level* lv = h->lv;
    const NextBlk* blocks = h->nx;
    // the fused kernel takes the split-f16 filter fragments unless the option asks for the f32-MFMA form
    auto fused_w = [&](const NextBlk& nb) {
        NextBlockW w = nb.w;
        if (!h->opt.next_split) w.fc1_h = nullptr;
        w.pipe = h->opt.next_pipe ? 1 : 0;
        return w;
    };
    auto T = [&](int l, int k) { return lv[l].t[k]; };
    auto SKIP = [&](int l) { return lv[l].skip; };
    // ConvBlock on an already-projected 48-channel map (new_unet.py:90-103)
    auto block = [&](int bi, const float* x, float* out, int lvl, int Hh, int Ww) -> int {
        const NextBlk& nb = blocks[bi];
        const double px = (double)B * Hh * Ww;
        // one kernel per block: 2 S of traffic (x in, out), no LayerNorm map
        Scope sc(h, s, "convblock_kernel", (2.0 * 49 * 48 + 2.0 * 2 * 48 * 192) * px, px * 384.0);
        HIPCHK(h, launch_next_block(x, out, fused_w(nb), B, Hh, Ww, s));
        return RVDD_OK;
    };
    auto proj = [&](int bi, const float* in1, const float* in2, float* out, int64_t npix) -> int {
        const NextBlk& nb = blocks[bi];
        const int creal = nb.c2 ? 96 : h->cin_real();
        Scope sc(h, s, "proj1x1_kernel", 2.0 * creal * 48 * (double)npix, (double)npix * 4.0 * (creal + 48));
        HIPCHK(h, launch_proj1x1(in1, nb.c1, in2, nb.c2, nb.w.proj_w, nb.w.proj_b, out, npix, s));
        return RVDD_OK;
    };
    const int H0 = lv[0].H, W0 = lv[0].W;
    const int64_t np0 = (int64_t)B * H0 * W0;

    // The 96 -> 48 projection of decoder_convs[i].blocks[0] (cat((x_dec, x_enc)), :321-329) as two halves in the epilogues of the
    // blocks that form x_enc (the last block of encoder level hi = 2 - i) and x_dec (decoder_ups[i]): where the upsampled map has the
    // skip's size (no zero_pad_features in between) and every kernel involved is the pipelined split-f16 block
    const bool pf_ok = h->opt.next_projfuse && h->opt.next_split && h->opt.next_pipe && h->opt.next_pool;
    auto pf_level = [&](int hi) {
        const int i = 2 - hi;
        return pf_ok && 2 * lv[hi + 1].H == lv[hi].H && 2 * lv[hi + 1].W == lv[hi].W && blocks[nx_enc(hi, 1)].w.fc1_h &&
               blocks[nx_up(i)].w.fc1_h && blocks[nx_dec(i, 0)].half[0].frag && blocks[nx_dec(i, 0)].half[1].frag;
    };
    auto block_proj = [&](int bi, const float* x, float* out, float* pooled, const NextProj& pj, int Hh, int Ww) -> int {
        const double px = (double)B * Hh * Ww;
        Scope sc(h, s, "convblock_kernel", (2.0 * 49 * 48 + 2.0 * 2 * 48 * 192 + 2.0 * 48 * 48) * px,
                 px * (384.0 + (pooled ? 48.0 : 0.0) + (pj.add ? 192.0 : 0.0)));
        HIPCHK(h, launch_next_block_proj(x, out, pooled, fused_w(blocks[bi]), pj, B, Hh, Ww, s));
        return RVDD_OK;
    };
    // ---- preprocessing + encoder level 0
    const float* e0 = T(0, 0);          // the projected input of encoder_convs[0].blocks[0], and the map that block writes
    float* e1 = T(0, 1);
    if (feat && run.featw_proj) {
        if (!run.netin_proj) RC(proj(NX_PRE, netin, nullptr, T(0, 0), np0));
        NextProj pj = blocks[NX_ENC0_0].half[0];
        pj.add = featw;                                                                  // W_f warp(features) + bias
        RC(block_proj(NX_PRE, T(0, 0), T(0, 1), nullptr, pj, H0, W0));
        e0 = T(0, 1);
        e1 = T(0, 0);
    } else if (feat) {
        if (!run.netin_proj) RC(proj(NX_PRE, netin, nullptr, T(0, 0), np0));
        RC(block(NX_PRE, T(0, 0), T(0, 1), 0, H0, W0));
        RC(proj(NX_ENC0_0, T(0, 1), featw, T(0, 0), np0));                              // cat[y, old_features] :381-382
    } else if (!run.netin_proj) {
        RC(proj(NX_ENC0_0, netin, nullptr, T(0, 0), np0));
    }
    // the last block of an encoder level feeds MaxPool2d(2) (DownConv, :200-204): the fused kernel pools in its epilogue
    auto block_pool = [&](int bi, const float* x, float* out, float* pooled, int lvl) -> int {
        if (pf_level(lvl)) return block_proj(bi, x, out, pooled, blocks[nx_dec(2 - lvl, 0)].half[1], lv[lvl].H, lv[lvl].W);
        if (!h->opt.next_pool) {
            RC(block(bi, x, out, lvl, lv[lvl].H, lv[lvl].W));
            Scope sc(h, s, "maxpool2_kernel", 0.0, (double)B * lv[lvl].H * lv[lvl].W * 192.0 * 1.25);
            HIPCHK(h, launch_maxpool2(out, pooled, B, lv[lvl].H, lv[lvl].W, s));
            return RVDD_OK;
        }
        const double px = (double)B * lv[lvl].H * lv[lvl].W;
        Scope sc(h, s, "convblock_kernel", (2.0 * 49 * 48 + 2.0 * 2 * 48 * 192) * px, px * (384.0 + 48.0));
        HIPCHK(h, launch_next_block_pool(x, out, pooled, fused_w(blocks[bi]), B, lv[lvl].H, lv[lvl].W, s));
        return RVDD_OK;
    };
    RC(block(NX_ENC0_0, e0, e1, 0, H0, W0));
    RC(block_pool(NX_ENC0_1, e1, SKIP(0), T(1, 0), 0));
    // ---- down path: MaxPool2d(2) then ConvBlock (:200-204), then two blocks
    for (int i = 0; i < 3; ++i) {
        const int l = i + 1;
        RC(block(nx_down(i), T(l, 0), T(l, 1), l, lv[l].H, lv[l].W));
        RC(block(nx_enc(l, 0), T(l, 1), T(l, 0), l, lv[l].H, lv[l].W));
        if (l < 3) RC(block_pool(nx_enc(l, 1), T(l, 0), SKIP(l), T(l + 1, 0), l));
        else RC(block(nx_enc(l, 1), T(l, 0), T(l, 1), l, lv[l].H, lv[l].W));
    }
    // ---- bottleneck (plain sequence, no residual sum)
    RC(block(NX_BOT0, T(3, 1), T(3, 0), 3, lv[3].H, lv[3].W));
    RC(block(NX_BOT1, T(3, 0), T(3, 1), 3, lv[3].H, lv[3].W));
    const float* d = T(3, 1);
    // ---- up path (:350-357)
    for (int i = 0; i < 3; ++i) {
        const int lo = 3 - i, hi = 2 - i;
        const int uh = 2 * lv[lo].H, uw = 2 * lv[lo].W;
        // maps of the upsampled size (smaller than the level's when a size was odd) are packed [batch][uh][uw]
        float* up0 = T(hi, 0);
        float* up1 = T(hi, 1);
        {
            Scope sc(h, s, "upsample2x_kernel", 0.0, (double)B * uh * uw * 192.0 * 1.25);
            HIPCHK(h, launch_upsample2x(d, up0, B, lv[lo].H, lv[lo].W, uh, uw, 0, 0, true, s));   // align_corners=True :145-149
        }
        if (pf_level(hi)) {
            // SKIP(hi) holds W_enc x_enc; this block stores W_dec x_dec + bias + that: the projected concat
            NextProj pj = blocks[nx_dec(i, 0)].half[0];
            pj.add = SKIP(hi);
            RC(block_proj(nx_up(i), up0, up1, nullptr, pj, uh, uw));
            RC(block(nx_dec(i, 0), up1, up0, hi, lv[hi].H, lv[hi].W));
            RC(block(nx_dec(i, 1), up0, up1, hi, lv[hi].H, lv[hi].W));
            d = up1;
            continue;
        }
        RC(block(nx_up(i), up0, up1, hi, uh, uw));
        const float* u = up1;
        if (uh != lv[hi].H || uw != lv[hi].W) {                                                    // zero_pad_features :56-66
            HIPCHK(h, launch_pad_copy(up1, T(hi, 2), B, uh, uw, lv[hi].H, lv[hi].W, (lv[hi].H - uh) / 2,
                                      (lv[hi].W - uw) / 2, s));
            u = T(hi, 2);
        }
        const int64_t np = (int64_t)B * lv[hi].H * lv[hi].W;
        RC(proj(nx_dec(i, 0), u, SKIP(hi), T(hi, 0), np));                                         // cat((x, x_enc)) :326
        RC(block(nx_dec(i, 0), T(hi, 0), T(hi, 1), hi, lv[hi].H, lv[hi].W));
        RC(block(nx_dec(i, 1), T(hi, 1), T(hi, 0), hi, lv[hi].H, lv[hi].W));
        d = T(hi, 0);
    }
    // ---- post-processing: two blocks (the second one is the hooked feature map :414-417), 1x1 -> 3
    float* fdst = feat_dst ? feat_dst : lv[0].t[2];
    float* p0 = d == T(0, 1) ? T(0, 0) : T(0, 1);
    RC(block(NX_POST0, d, p0, 0, H0, W0));
    {
        // the last block; the 1x1 conv 48 -> 3 rides in the epilogue of its MLP kernel
        const NextBlk& nb = blocks[NX_POST1];
        const double px = (double)np0;
        Scope sc(h, s, "convblock_kernel", (2.0 * 49 * 48 + 2.0 * 2 * 48 * 192 + 2.0 * 48 * 3) * px, px * (384.0 + 12.0 + 16.0));
        HIPCHK(h, launch_next_block_out3(p0, fdst, fused_w(nb), B, H0, W0, h->w_out, h->b_out, out_nchw, out_nhwc4, s));
    }
    return RVDD_OK;
}
