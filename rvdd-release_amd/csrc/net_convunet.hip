// The convunet: weight banks of its 3x3 convs, the composed first layer, and the schedule of one forward
// (networks/unet.py:544-588 as specialised by UNet_FixedFeatures[_feat], :595-825).
#include "runtime_internal.h"

namespace {

// OIHW [48][cin_total][3][3], channels [c0, c0+cn) -> [tap][j][m][lane = 16g + cout&15][i] with
// channel = c0 + 16j + 4g + i (zero beyond cn): the A-fragment order of conv3x3.hip (lane-linear).
std::vector<float> arrange_conv3x3(const HostTensor& t, int c0, int cn, int cin_pad) {
    const int cin_total = (int)t.shape[1];
    const int NJ = cin_pad / 16;
    std::vector<float> out((size_t)9 * NJ * 48 * 16, 0.f);
    for (int tap = 0; tap < 9; ++tap)
        for (int j = 0; j < NJ; ++j)
            for (int co = 0; co < 48; ++co)
                for (int g = 0; g < 4; ++g)
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * j + 4 * g + i;
                        if (c >= cn) continue;
                        out[(((size_t)(tap * NJ + j) * 3 + co / 16) * 64 + g * 16 + co % 16) * 4 + i] =
                            t.data[(((size_t)co * cin_total + c0 + c) * 3 + tap / 3) * 3 + tap % 3];
                    }
    return out;
}

// OIHW [48][cin_total][3][3], channels [c0, c0+48) -> U = G g G^T per (cout, cin), stored
// [pos 16][j 3][m 3][lane = 16g + (cout&15)][i 4] with channel = c0 + 16j+4g+i: the A-fragment order of wino3x3.hip,
// lane-linear so that each lane group of a ds_read_b128 covers one whole 256-B bank row (no bank conflict).
// nj = 3: input channels c0 .. c0+47 of the filter; nj = 1: the first layer, channels 0 .. cin_total-1 (6 or 9)
// zero-padded to 16
std::vector<float> arrange_wino3x3(const HostTensor& t, int c0, int nj = 3) {
    const int cin_total = (int)t.shape[1];
    const int nc = nj == 3 ? 48 : (cin_total < 16 ? cin_total : 16);
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> out((size_t)16 * nj * 3 * 256, 0.f);
    for (int co = 0; co < 48; ++co)
        for (int c = 0; c < nc; ++c) {
            const float* gk = &t.data[((size_t)co * cin_total + c0 + c) * 9];
            double tmp[4][3], u[4][4];
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 3; ++k) tmp[i][k] = G[i][0] * gk[k] + G[i][1] * gk[3 + k] + G[i][2] * gk[6 + k];
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 4; ++k) u[i][k] = tmp[i][0] * G[k][0] + tmp[i][1] * G[k][1] + tmp[i][2] * G[k][2];
            const int j = c / 16, g = (c % 16) / 4, ii = c % 4, m = co / 16, lr = co % 16;
            for (int pos = 0; pos < 16; ++pos)
                out[(((size_t)(pos * nj + j) * 3 + m) * 64 + g * 16 + lr) * 4 + ii] = (float)u[pos / 4][pos % 4];
        }
    return out;
}

// OIHW [48][cin_total][3][3], channels [c0, c0+48) -> the split bank of conv3x3h.hip: w' = 2^s w (s = the largest power
// keeping |w'| <= 1024, returned as 2^-s), hi = f16(w') toward zero, lo = f16(w' - hi); stored
// [chunk 14][cout block 3][hi, lo][lane = 16g + (cout & 15)][e 8] as f16 with 8-channel group G = 4 chunk + g = channels
// 8 (G % 6) + e of tap G / 6 (groups 54, 55 zero): lane-linear 16-B A fragments of v_mfma_f32_16x16x32_f16.
// (ks = 5: the composed first layer, [48][cin][5][5], 13 chunks)
std::vector<float> arrange_conv3x3h(const HostTensor& t, int c0, float* inv_scale, int cin_pad = 48, int ks = 3) {
    const int cin_total = (int)t.shape[1];
    const int nc = cin_pad == 48 ? 48 : std::min(cin_total, 16);      // 16: the first layer, 6 or 9 real channels, zero filters beyond
    const int ntap = ks * ks;
    const int gpt = cin_pad / 8, ng = ntap * gpt, nch = (ng + 3) / 4;
    float mx = 0.f;
    for (int co = 0; co < 48; ++co)
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < ntap; ++k) mx = std::max(mx, std::fabs(t.data[((size_t)co * cin_total + c0 + c) * ntap + k]));
    int sft = 0;
    if (mx > 0.f && std::isfinite(mx)) sft = std::min(40, std::max(-40, (int)std::floor(std::log2(1024.0 / mx))));
    const float sc = std::ldexp(1.0f, sft);
    *inv_scale = std::ldexp(1.0f, -sft);
    const size_t halves = (size_t)nch * 3 * 2 * 512;
    if (halves * 2 != (ks == 5 ? conv5x5h_weight_bytes(cin_pad) : conv3x3h_weight_bytes(cin_pad))) return {};
    std::vector<uint16_t> bank(halves, 0);
    for (int G = 0; G < ng; ++G) {
        const int j = G / 4, g = G % 4, tap = G / gpt, cg = (G % gpt) * 8;
        for (int co = 0; co < 48; ++co)
            for (int e = 0; e < 8; ++e) {
                if (cg + e >= nc) continue;
                const float w = t.data[((size_t)co * cin_total + c0 + cg + e) * ntap + tap] * sc;      // exact: a power of two
                const uint16_t hi = f16_bits(w, true);
                const uint16_t lo = f16_bits(w - f16_value(hi), false);
                const size_t frag = ((size_t)(j * 3 + co / 16) * 2) * 512 + (size_t)(g * 16 + co % 16) * 8 + e;
                bank[frag] = hi;
                bank[frag + 512] = lo;
            }
    }
    std::vector<float> out(halves / 2);
    std::memcpy(out.data(), bank.data(), halves * 2);
    return out;
}

// preprocessing_layer (3x3, cin -> 48, NO activation: networks/unet.py:742) followed by the first 48 input channels of
// EncoderConvs[0][0] (3x3, :743) is one linear map of the network input: out(p) = sum_d W2[d] y(p + d - 1), y(q) = b1 +
// sum_e W1[e] x(q + e - 1)  =>  out(p) = b + sum_u Wc[u] x(p + u - 2), Wc[u] = sum_{d + e = u} W2[d] W1[e] (5x5, 48 x cin),
// b = sum_d W2[d] b1 (+ the layer's own bias, which the pass already adds).  Composed in double.  One 16-channel 5x5 conv
// (K = 400) instead of a 16 -> 48 conv, a full-resolution 48-channel map written and read back, and a 48 -> 48 conv (K = 576).
// The one thing the composition gets wrong is the zero padding BETWEEN the layers: y is ZERO outside the image, the composed
// conv sees b1 + (partial windows) there.  Only pixels on the image border are affected; launch_pre_border_fix subtracts those
// terms (it needs W1, b1, W2 in plain layouts).
int compose_pre_enc0(rvdd_t* h) {
    const HostTensor& w1 = h->staged.at("preprocessing_layer.weight");            // [48 m][cin][3][3]
    const HostTensor& b1 = h->staged.at("preprocessing_layer.bias");
    const HostTensor& w2 = h->staged.at("EncoderConvs.0.blocks.0.0.weight");      // [48 o][96][3][3], channels 0..47 = m
    const int cin = (int)w1.shape[1];
    HostTensor wc;
    wc.shape = {48, cin, 5, 5};
    std::vector<double> acc((size_t)48 * cin * 25, 0.0);
    for (int o = 0; o < 48; ++o)
        for (int m = 0; m < 48; ++m)
            for (int d = 0; d < 9; ++d) {
                const double a = w2.data[((size_t)o * 96 + m) * 9 + d];
                if (a == 0.0) continue;
                const int dy = d / 3, dx = d % 3;
                for (int c = 0; c < cin; ++c)
                    for (int e = 0; e < 9; ++e)
                        acc[((size_t)o * cin + c) * 25 + (dy + e / 3) * 5 + dx + e % 3] += a * (double)w1.data[((size_t)m * cin + c) * 9 + e];
            }
    wc.data.resize(acc.size());
    for (size_t i = 0; i < acc.size(); ++i) wc.data[i] = (float)acc[i];
    std::vector<float> bc(48);
    for (int o = 0; o < 48; ++o) {
        double b = 0.0;
        for (int m = 0; m < 48; ++m)
            for (int d = 0; d < 9; ++d) b += (double)w2.data[((size_t)o * 96 + m) * 9 + d] * (double)b1.data[m];
        bc[o] = (float)(b + (double)h->staged.at("EncoderConvs.0.blocks.0.0.bias").data[o]);      // + the layer's own bias (pass 1 adds it)
    }
    RC(upload(h, &h->pre5_w, arrange_conv3x3h(wc, 0, &h->pre5_inv, 16, 5)));
    // without a future frame (6 real channels) the second 8-channel group of every tap is zero filters on zero input: the bank of
    // the first groups alone, 25 groups in 7 chunks.  Both banks are kept, "pre5_cin8" chooses per launch.
    h->pre5_w8 = nullptr;
    if (h->cin_real() <= 8) RC(upload(h, &h->pre5_w8, arrange_conv3x3h(wc, 0, &h->pre5_inv8, 8, 5)));
    RC(upload(h, &h->pre5_b, bc));
    std::vector<float> a1((size_t)9 * 16 * 48, 0.f), a2((size_t)9 * 48 * 48);
    for (int e = 0; e < 9; ++e)
        for (int c = 0; c < cin; ++c)
            for (int m = 0; m < 48; ++m) a1[((size_t)e * 16 + c) * 48 + m] = w1.data[((size_t)m * cin + c) * 9 + e];
    for (int d = 0; d < 9; ++d)
        for (int m = 0; m < 48; ++m)
            for (int o = 0; o < 48; ++o) a2[((size_t)d * 48 + m) * 48 + o] = w2.data[((size_t)o * 96 + m) * 9 + d];
    RC(upload(h, &h->pre_w1, a1));
    RC(upload(h, &h->pre_b1, b1.data));
    RC(upload(h, &h->pre_w2, a2));
    return RVDD_OK;
}

// ---- conv helper ---------------------------------------------------------------
const char* conv_name(int cin, int epi, bool acc) {
    static const char* names[2][4][2] = {
        {{"conv3x3_kernel<16, 0, false>", "conv3x3_kernel<16, 0, true>"},
         {"conv3x3_kernel<16, 1, false>", "conv3x3_kernel<16, 1, true>"},
         {"conv3x3_kernel<16, 2, false>", "conv3x3_kernel<16, 2, true>"},
         {"conv3x3_kernel<16, 3, false>", "conv3x3_kernel<16, 3, true>"}},
        {{"conv3x3_kernel<48, 0, false>", "conv3x3_kernel<48, 0, true>"},
         {"conv3x3_kernel<48, 1, false>", "conv3x3_kernel<48, 1, true>"},
         {"conv3x3_kernel<48, 2, false>", "conv3x3_kernel<48, 2, true>"},
         {"conv3x3_kernel<48, 3, false>", "conv3x3_kernel<48, 3, true>"}}};
    return names[cin == 48][epi][acc];
}

const char* wino_name(int epi, bool acc) {
    static const char* names[5][2] = {{"wino3x3_kernel<0, false>", "wino3x3_kernel<0, true>"},
                                      {"wino3x3_kernel<1, false>", "wino3x3_kernel<1, true>"},
                                      {"wino3x3_kernel<2, false>", "wino3x3_kernel<2, true>"},
                                      {"wino3x3_kernel<3, false>", "wino3x3_kernel<3, true>"},
                                      {"wino3x3_kernel<4, false>", "wino3x3_kernel<4, true>"}};
    return names[epi][acc];
}

const char* conv_name_h(int epi, bool acc) {
    static const char* names[5][2] = {{"conv3x3h_kernel<48, 0, false, false>", "conv3x3h_kernel<48, 0, true, false>"},
                                      {"conv3x3h_kernel<48, 1, false, false>", "conv3x3h_kernel<48, 1, true, false>"},
                                      {"conv3x3h_kernel<48, 2, false, false>", "conv3x3h_kernel<48, 2, true, false>"},
                                      {"conv3x3h_kernel<48, 3, false, false>", "conv3x3h_kernel<48, 3, true, false>"},
                                      {"conv3x3h_kernel<48, 4, false, false>", "conv3x3h_kernel<48, 4, true, false>"}};
    return names[epi][acc];
}

// Winograd needs enough 8x32-pixel units to fill the chip (its 144 KiB filter bank is loaded once
// per workgroup); the 1/8-resolution level of a single 720p sequence (60 units) runs faster direct
bool wino_applies(const rvdd_t* h, const NetRun& run, int H, int W) {
    return h->opt.wino_allowed() && (h->opt.wino_forced() || run.n * ((W + 31) / 32) * ((H + 7) / 8) >= 200);
}

int run_conv(rvdd_t* h, const NetRun& run, const Conv3& L, const ConvCall& c, hipStream_t s, Sub sub) {
    const int cin = L.cin_pad[c.src];
    const int Ho = c.epi == EPI_POOL ? c.H / 2 : (c.Hout ? c.Hout : c.H), Wo = c.epi == EPI_POOL ? c.W / 2 : (c.Wout ? c.Wout : c.W);
    const size_t px_in = (size_t)sub.b0 * c.H * c.W, px_out = (size_t)sub.b0 * Ho * Wo;
    ConvArgs a{};
    a.in = c.in + (c.ups ? px_in / 4 : px_in) * cin;
    a.ups = c.ups ? 1 : 0;
    a.w = L.w[c.src];
    a.bias = L.bias;
    a.acc_in = c.acc_in ? c.acc_in + px_in * kF : nullptr;
    a.res1 = c.res1 ? c.res1 + px_in * kF : nullptr;
    a.res2 = c.res2 ? c.res2 + px_in * kF : nullptr;
    a.out = c.out + px_out * kF;
    a.B = sub.nb;
    a.H = c.H;
    a.W = c.W;
    a.Hout = Ho;
    a.Wout = Wo;
    a.oy = c.oy;
    a.ox = c.ox;
    a.tiles_x = (c.W + 15) / 16;
    a.tiles_y = (c.H + 7) / 8;
    a.ntiles = a.B * a.tiles_x * a.tiles_y;
    const double px = (double)a.B * c.H * c.W;
    const double flops = 2.0 * 9.0 * L.cin_real[c.src] * 48.0 * px;
    double bytes = px * 4.0 * (L.cin_real[c.src] + (c.epi == EPI_POOL ? 12.0 : 48.0));
    if (c.acc_in) bytes += px * 192.0;
    if (c.epi == EPI_RELU_ADD2) bytes += px * 384.0;
    a.w3 = h->w_out;
    a.b3 = h->b_out;
    a.out3_nchw = c.out3_nchw ? c.out3_nchw + px_in * 3 : nullptr;
    a.out3_nhwc4 = c.out3_nhwc4 ? c.out3_nhwc4 + px_in * 4 : nullptr;
    a.amax_in = (c.amax_in >= 0 && h->opt.bfp) ? amax_words(h, c.amax_in, sub.b0) : nullptr;
    a.amax_out = (c.amax_out >= 0 && h->opt.bfp) ? amax_words(h, c.amax_out, sub.b0) : nullptr;
    const bool c16_ok = cin != 48 && !c.acc_in && (c.epi == EPI_NONE || c.epi == EPI_RELU);
    if (c.ups && !(cin == 48 && ((h->opt.split16() && L.wh[c.src]) || (L.wu[c.src] && wino_applies(h, run, c.H, c.W)))))
        return fail(h, RVDD_ERR_STATE, "run_conv: the fused upsample exists in the split-f16 and the Winograd kernels only");
    if (c.ups) bytes -= px * 4.0 * 36.0;          // reads the quarter-size map
    // the F16 matrix pipe with split operands: every layer of the convunet
    if (h->opt.split16() && L.wh[c.src] && (cin == 48 || c16_ok)) {
        a.w = L.wh[c.src];
        a.wscale = L.wh_inv[c.src];
        Scope sc(h, s, c.ups ? "conv3x3h_kernel<48, 1, false, true>" : cin == 48 ? conv_name_h(c.epi, c.acc_in != nullptr)
                           : (c.epi == EPI_NONE ? "conv3x3h_kernel<16, 0, false, false>" : "conv3x3h_kernel<16, 1, false, false>"), flops, bytes);
        HIPCHK(h, launch_conv3x3h(a, cin == 48 ? 48 : 16, c.epi, s, h->opt.cout_split));
        return RVDD_OK;
    }
    if ((cin == 48 || c16_ok) && L.wu[c.src] && wino_applies(h, run, c.H, c.W)) {
        a.w = L.wu[c.src];
        Scope sc(h, s, c.ups ? "wino3x3_ups_kernel<1>" : cin == 48 ? wino_name(c.epi, c.acc_in != nullptr)
                                 : (c.epi == EPI_NONE ? "wino3x3_c16_kernel<0>" : "wino3x3_c16_kernel<1>"), flops, bytes);
        HIPCHK(h, launch_wino3x3(a, cin == 48 ? 48 : 16, c.epi, s));
        return RVDD_OK;
    }
    Scope sc(h, s, conv_name(cin, c.epi, c.acc_in != nullptr), flops, bytes);
    HIPCHK(h, launch_conv3x3(a, cin, c.epi, s, c.variant));
    return RVDD_OK;
}

// The composed 5x5 conv of the network input (compose_pre_enc0) into `part`, and its border fix; sequences of `sub`.
int run_pre5(rvdd_t* h, const NetRun& run, const float* netin, float* part, hipStream_t s, Sub sub) {
    const int H = h->cfg.height, W = h->cfg.width;
    const size_t px0 = (size_t)sub.b0 * H * W;
    ConvArgs a{};
    a.in = netin + px0 * kNetInC;
    const bool c8 = h->opt.pre5_cin8 && h->pre5_w8;      // at most 8 real channels: only the first 8 of the 16-channel pixel are multiplied
    a.w = c8 ? h->pre5_w8 : h->pre5_w;
    a.wscale = c8 ? h->pre5_inv8 : h->pre5_inv;
    a.bias = h->pre5_b;
    a.out = part + px0 * kF;
    a.B = sub.nb;
    a.H = a.Hout = H;
    a.W = a.Wout = W;
    a.amax_in = h->opt.bfp ? amax_words(h, run.amax.base + AMAX_REL_NETIN, sub.b0) : nullptr;
    const double px = (double)sub.nb * H * W;
    {
        Scope sc(h, s, c8 ? "conv5x5h_kernel<8>" : "conv5x5h_kernel<16>", 2.0 * 25.0 * h->cin_real() * 48.0 * px, px * 4.0 * (h->cin_real() + 48.0));
        HIPCHK(h, c8 ? launch_conv5x5h_c8(a, s) : launch_conv5x5h_c16(a, s));
    }
    HIPCHK(h, launch_pre_border_fix(a.in, h->pre_w1, h->pre_b1, h->pre_w2, a.out, sub.nb, H, W, s));
    return RVDD_OK;
}

}  // namespace

// Full-resolution stages one sequence at a time (depth first) instead of all B sequences per layer -- an option
// (rvdd_set_option "seq_major"), off by default.  The idea: a 48-channel map of ONE 720p sequence (177 MB) stays in
// the 256 MiB Infinity Cache between the layer that writes it and the layer that reads it, the maps of four (708 MB)
// do not.  Measured (profiles/r02_c_seq_major.json): 424 frames/s against 456 batched -- per-sequence launches lose
// more to their tails (3600 units on 256 CUs = 14.06 rounds) and to four filter-bank loads per layer than the cache
// gives back.  Kept because it is free and pins an invariant the tests use: a launch's batch size does not enter a
// tile's sums, so both schedules give bit-identical frames.
bool seq_major_on(const rvdd_t* h, int n) { return n > 1 && h->opt.seq_major == 1; }
bool pre5_fused(const rvdd_t* h) { return !h->is_next() && h->has_feat() && h->opt.fuse_pre && h->opt.split16() && h->pre5_w; }

int finalize_convunet(rvdd_t* h) {
    for (const auto& n : convunet_conv_names(h->has_feat())) {
        const HostTensor& wt = h->staged.at(n + ".weight");
        Conv3 L;
        const int cin = (int)wt.shape[1];
        if (cin == 96) {
            L.nsrc = 2;
            for (int sidx = 0; sidx < 2; ++sidx) {
                L.cin_real[sidx] = 48;
                L.cin_pad[sidx] = 48;
                RC(upload(h, &L.w[sidx], arrange_conv3x3(wt, 48 * sidx, 48, 48)));
                RC(upload(h, &L.wu[sidx], arrange_wino3x3(wt, 48 * sidx)));
                RC(upload(h, &L.wh[sidx], arrange_conv3x3h(wt, 48 * sidx, &L.wh_inv[sidx])));
            }
        } else {
            L.nsrc = 1;
            L.cin_real[0] = cin;
            L.cin_pad[0] = cin == 48 ? 48 : kNetInC;
            RC(upload(h, &L.w[0], arrange_conv3x3(wt, 0, cin, L.cin_pad[0])));
            RC(upload(h, &L.wu[0], cin == 48 ? arrange_wino3x3(wt, 0) : arrange_wino3x3(wt, 0, 1)));
            RC(upload(h, &L.wh[0], arrange_conv3x3h(wt, 0, &L.wh_inv[0], cin == 48 ? 48 : 16)));
        }
        RC(upload(h, &L.bias, h->staged.at(n + ".bias").data));
        for (int li = 0; li < CU_COUNT; ++li)
            if (n == kCuNames[li]) h->cu[li] = L;
    }
    RC(upload(h, &h->w_out, h->staged.at("PostConvs.1.weight").data));
    RC(upload(h, &h->b_out, h->staged.at("PostConvs.1.bias").data));
    if (h->has_feat()) RC(compose_pre_enc0(h));
    return RVDD_OK;
}

// networks/unet.py:544-588 as specialised by UNet_FixedFeatures[_feat] (:595-825).
int run_convunet(rvdd_t* h, NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
                 float* out_nhwc4, hipStream_t s) {
    const bool feat = h->has_feat();
    const int B = run.n;
    Level* lv = h->lv;
    const Conv3* cu = h->cu;
    // `from` = the amax slot of the input map (L(the layer that wrote it), AMAX_NETIN, run.amax.feat_in); a layer's output slot is L(its id)
    auto conv = [&](int layer, const float* in, int from, float* out, int lvl, int epi, Sub sub) {
        ConvCall c;
        c.in = in; c.out = out; c.H = lv[lvl].H; c.W = lv[lvl].W; c.epi = epi;
        c.amax_in = from; c.amax_out = amax_layer(run, layer);
        return run_conv(h, run, cu[layer], c, s, sub);
    };
    const auto L = [&](int layer) { return amax_layer(run, layer); };
    const int AMAX_NETIN = run.amax.base + AMAX_REL_NETIN;
    // two-source (virtual concat) conv: pass 1 leaves bias + sum over source A in `part`
    auto conv2 = [&](int layer, const float* inA, int fromA, const float* inB, int fromB, float* out, int lvl, Sub sub) {
        ConvCall c;
        c.in = inA; c.src = 0; c.out = lv[lvl].part; c.H = lv[lvl].H; c.W = lv[lvl].W; c.epi = EPI_NONE;
        c.amax_in = fromA;
        RC(run_conv(h, run, cu[layer], c, s, sub));
        c.in = inB; c.src = 1; c.acc_in = lv[lvl].part; c.out = out; c.epi = EPI_RELU;
        c.amax_in = fromB; c.amax_out = amax_layer(run, layer);
        return run_conv(h, run, cu[layer], c, s, sub);
    };
    const Sub all{0, B};
    // the full-resolution stages run per sequence when that keeps their maps in the Infinity Cache (seq_major_on),
    // in an order that alternates from frame to frame so that a step begins with the sequence the last one ended on
    const bool per_seq = seq_major_on(h, B);
    const int nsub = per_seq ? B : 1;
    auto sub_at = [&](int k) { return per_seq ? Sub{h->serpentine ? B - 1 - k : k, 1} : all; };

    // ---- pre-stages + encoder level 0
    for (int k = 0; k < nsub; ++k) {
        const Sub sb = sub_at(k);
        if (run.in) RC(run_prologue(h, run, sb, s));
        if (pre5_fused(h)) {
            // preprocessing_layer (:742, no activation) and the first source of EncoderConvs[0][0] (:743) as ONE 5x5 conv of the
            // network input (compose_pre_enc0), its border ring put right, then the second source (the old features) as before
            RC(run_pre5(h, run, netin, lv[0].part, s, sb));
            if (run.zero_feat) {
                // the first step of a video: the second source is all +0, its pass adds +0 to `part` and applies the ReLU
                const size_t px0 = (size_t)sb.b0 * lv[0].H * lv[0].W;
                const double px = (double)sb.nb * lv[0].H * lv[0].W;
                Scope sc(h, s, "relu_part_kernel", 0.0, px * 384.0);
                HIPCHK(h, launch_relu_part(lv[0].part + px0 * kF, lv[0].t[1] + px0 * kF, sb.nb, (int64_t)lv[0].H * lv[0].W * kF,
                                           h->opt.bfp ? amax_words(h, L(CU_ENC0_0), sb.b0) : nullptr, s));
            } else {
                ConvCall c;
                c.in = featw; c.src = 1; c.acc_in = lv[0].part; c.out = lv[0].t[1]; c.H = lv[0].H; c.W = lv[0].W; c.epi = EPI_RELU;
                c.amax_in = run.amax.feat_in; c.amax_out = L(CU_ENC0_0);
                RC(run_conv(h, run, cu[CU_ENC0_0], c, s, sb));
            }
        } else if (feat) {
            RC(conv(CU_PRE, netin, AMAX_NETIN, lv[0].t[0], 0, EPI_NONE, sb));               // :742 (no activation)
            RC(conv2(CU_ENC0_0, lv[0].t[0], L(CU_PRE), featw, run.amax.feat_in, lv[0].t[1], 0, sb)); // cat[y, old_features] :743
        } else {
            RC(conv(CU_ENC0_0, netin, AMAX_NETIN, lv[0].t[1], 0, EPI_RELU, sb));
        }
        RC(conv(CU_ENC0_1, lv[0].t[1], L(CU_ENC0_0), lv[0].skip, 0, EPI_RELU, sb));
        RC(conv(CU_DOWN0, lv[0].skip, L(CU_ENC0_1), lv[1].t[0], 0, EPI_POOL, sb));          // :207-208
    }
    // ---- encoder levels 1..3 (all sequences per launch: these levels need the batch to fill the chip)
    for (int i = 1; i <= 3; ++i) {
        if (i > 1) RC(conv(cu_down(i - 1), lv[i - 1].skip, L(cu_enc(i - 1, 1)), lv[i].t[0], i - 1, EPI_POOL, all));
        RC(conv(cu_enc(i, 0), lv[i].t[0], L(cu_down(i - 1)), lv[i].t[1], i, EPI_RELU, all));
        RC(conv(cu_enc(i, 1), lv[i].t[1], L(cu_enc(i, 0)), i < 3 ? lv[i].skip : lv[3].t[2], i, EPI_RELU, all));
    }
    // ---- bottleneck: d = e3 + d1 + d2 (:561-567)
    float* e3 = lv[3].t[2];
    RC(conv(CU_BOT0, e3, L(cu_enc(3, 1)), lv[3].t[0], 3, EPI_RELU, all));
    {
        ConvCall c;
        c.in = lv[3].t[0]; c.out = lv[3].t[1]; c.H = lv[3].H; c.W = lv[3].W;
        c.epi = EPI_RELU_ADD2; c.res1 = e3; c.res2 = lv[3].t[0];
        c.amax_in = L(CU_BOT0); c.amax_out = L(CU_BOT1);
        RC(run_conv(h, run, cu[CU_BOT1], c, s, all));
    }
    const float* d = lv[3].t[1];
    int d_from = L(CU_BOT1);
    // ---- decoder (:570-579); its last level again per sequence, together with the post convs
    float* fdst = feat_dst ? feat_dst : lv[0].t[2];
    for (int i = 0; i < 3; ++i) {
        const int lo = 3 - i, hi = 2 - i;
        const int uh = 2 * lv[lo].H, uw = 2 * lv[lo].W;      // size after nn.Upsample(x2)
        for (int k = 0; k < (hi == 0 ? nsub : 1); ++k) {
            const Sub sb = hi == 0 ? sub_at(k) : all;
            const size_t lo_px = (size_t)sb.b0 * lv[lo].H * lv[lo].W, hi_px = (size_t)sb.b0 * lv[hi].H * lv[hi].W;
            // UpConv: bilinear x2, conv, ReLU (:137-142).  Where the Winograd kernel runs the conv, the interpolation
            // happens in its patch load and the upsampled map is never written; elsewhere it is made first.
            const bool fused = h->opt.fuse_upsample && (h->opt.split16() || wino_applies(h, run, uh, uw));
            if (!fused) {
                Scope sc(h, s, "upsample2x_kernel", 0.0, (double)sb.nb * uh * uw * 192.0 * 1.25);
                HIPCHK(h, launch_upsample2x(d + lo_px * kF, lv[hi].t[0] + (size_t)sb.b0 * uh * uw * kF, sb.nb, lv[lo].H, lv[lo].W, uh,
                                            uw, 0, 0, false, s));
            }
            // conv + ReLU at the upsampled size, written into a map of the skip's size
            // (zero_pad_features, :151-170; identity when sizes agree)
            ConvCall c;
            c.in = fused ? d : lv[hi].t[0]; c.ups = fused;
            c.out = lv[hi].t[1]; c.H = uh; c.W = uw; c.epi = EPI_RELU;
            c.Hout = lv[hi].H; c.Wout = lv[hi].W;
            c.oy = (lv[hi].H - uh) / 2; c.ox = (lv[hi].W - uw) / 2;
            // (an interpolated value never exceeds the map's maximum: the upsampled map shares the words of its source)
            c.amax_in = d_from; c.amax_out = L(cu_up(i));
            if (uh != lv[hi].H || uw != lv[hi].W)
                HIPCHK(h, hipMemsetAsync(lv[hi].t[1] + hi_px * kF, 0, (size_t)sb.nb * lv[hi].H * lv[hi].W * kF * sizeof(float), s));
            RC(run_conv(h, run, cu[cu_up(i)], c, s, sb));
            RC(conv2(cu_dec(i, 0), lv[hi].skip, L(cu_enc(hi, 1)), lv[hi].t[1], L(cu_up(i)), lv[hi].t[0], hi, sb));        // cat(skip, dec) :541
            RC(conv(cu_dec(i, 1), lv[hi].t[0], L(cu_dec(i, 0)), lv[hi].t[1], hi, EPI_RELU, sb));
            if (hi > 0) continue;
            // ---- post: hooked 48-ch map = next frame's features (:808-812), then 1x1 -> 3
            if (h->opt.split16() || wino_applies(h, run, lv[0].H, lv[0].W)) {
                // PostConvs[1] (1x1, 48 -> 3) rides in the epilogue of PostConvs[0]'s kernel (split-f16: at every size; Winograd
                // f32: where it runs) -- and with it the output frame's share of the words the next step's input bound reads
                ConvCall pc;
                pc.in = lv[0].t[1]; pc.out = fdst; pc.H = lv[0].H; pc.W = lv[0].W; pc.epi = EPI_RELU_OUT3;
                pc.out3_nchw = out_nchw; pc.out3_nhwc4 = out_nhwc4;
                pc.amax_in = L(cu_dec(2, 1)); pc.amax_out = run.amax.post_out;
                RC(run_conv(h, run, cu[CU_POST], pc, s, sb));
            } else {
                ConvCall pc;
                pc.in = lv[0].t[1]; pc.out = fdst; pc.H = lv[0].H; pc.W = lv[0].W; pc.epi = EPI_RELU;
                pc.amax_in = L(cu_dec(2, 1)); pc.amax_out = run.amax.post_out;
                RC(run_conv(h, run, cu[CU_POST], pc, s, sb));
                const size_t px0 = (size_t)sb.b0 * h->cfg.height * h->cfg.width;
                const double px = (double)sb.nb * h->cfg.height * h->cfg.width;
                Scope sc(h, s, "conv1x1_out_kernel", 2.0 * 48 * 3 * px, px * (192.0 + 12.0 + 16.0));
                HIPCHK(h, launch_conv1x1_out(fdst + px0 * kF, h->w_out, h->b_out, out_nchw + px0 * 3,
                                             out_nhwc4 ? out_nhwc4 + px0 * 4 : nullptr, sb.nb, h->cfg.height, h->cfg.width, s));
            }
        }
        d = lv[hi].t[1];
        d_from = L(cu_dec(i, 1));
    }
    return RVDD_OK;
}

extern "C" int rvdd_debug_conv_bench(rvdd_t* h, int32_t variant, int32_t level, int32_t iters, float* ms, void* stream) {
    if (!h || !ms || level < 0 || level > 3 || iters < 1) return fail(h, RVDD_ERR_ARG, "rvdd_debug_conv_bench: bad argument");
    ENTER(h);
    if (!h->finalized || h->is_next()) return fail(h, RVDD_ERR_STATE, "rvdd_debug_conv_bench: needs a finalized convunet handle");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool was = h->prof_on;
    const int was_conv = h->opt.conv;
    h->prof_on = false;
    const Conv3& L = h->cu[CU_ENC1_1];
    ConvCall c;
    // variant 3 = Winograd kernel, 4 = split-f16 kernel (the direct one where the layer has no split bank, never one by size),
    // 0..2 = direct kernel variants
    h->opt.conv = variant == 3 ? CONV_WINO : variant == 4 && L.wh[c.src] ? CONV_SPLIT16 : CONV_DIRECT;
    c.variant = variant >= 3 ? 0 : variant;
    c.in = h->lv[level].t[0]; c.out = h->lv[level].t[1]; c.H = h->lv[level].H; c.W = h->lv[level].W; c.epi = EPI_RELU;
    NetRun run;
    run.n = h->cfg.batch;
    const Sub all{0, run.n};
    int rc = run_conv(h, run, L, c, s, all);   // warm-up (also sets the function attribute)
    if (rc == RVDD_OK) {
        (void)hipEventRecord(h->t0, s);
        for (int i = 0; i < iters && rc == RVDD_OK; ++i) rc = run_conv(h, run, L, c, s, all);
        (void)hipEventRecord(h->t1, s);
        (void)hipEventSynchronize(h->t1);
        float t = 0.f;
        (void)hipEventElapsedTime(&t, h->t0, h->t1);
        *ms = t / iters;
    }
    h->prof_on = was;
    h->opt.conv = was_conv;
    return rc;
}
