// Kernel selection of yv3_conv2d (conv_select.h): every measured crossover of the convolution path lives in this file.
#include "conv_select.h"
#include <stdio.h>

yv3_conv_shape yv3_conv_out_shape(const yv3_conv_desc* d) {
    const int pad = (d->k - 1) / 2;
    yv3_conv_shape s;
    s.Ho = (d->H + 2 * pad - d->k) / d->stride + 1;
    s.Wo = (d->W + 2 * pad - d->k) / d->stride + 1;
    s.M = (long long)d->B * s.Ho * s.Wo;
    return s;
}

// =========================================================================================== plane kernels (bf16 / fp16 planes)

// Winograd F(2x2,3x3) form of a 3x3 / stride-1 fp16-plane layer?  (The per-launch rule of the fp16-plane mode.)
static bool planes_wino_rule(const yv3_conv_desc* d, int np, long long ncu) {
    const int npad = d->cout_pad;
    const bool k3 = d->k == 3, dual = d->cin_up > 0, out_f32 = d->out_dtype == YV3_F32;
    if (!(d->w_wino && np == 2 && k3 && d->stride == 1 && !out_f32 && !dual && d->alpha_wino && npad % 128 == 0 &&
          d->x_plane_stride <= 0 && d->y_plane_stride <= 0)) return false;
    // Winograd F(2x2,3x3) when its 128x128 tiles (a quarter of the direct kernel's row count) fill 0.55 ... 1.05 rounds of
    // the chip: same-box A/B against the direct kernel (tools/wino_ab.py): 256->512 @26x26 bs=32 (172 tiles) x1.28,
    // 512->1024 @13x13 bs=64 (200) x1.36, 256->512 @38x38 bs=16 (184) x1.26; but 340 tiles (1.33 rounds: @26x26 bs=64) x0.96,
    // 104 tiles (@13x13 bs=32, @19x19 bs=16) x0.78...0.80, and the 128-channel 52x52 layers x0.93 (input transform HBM-bound)
    const long long tiles = (((long long)d->B * ((d->H + 1) / 2) * ((d->W + 1) / 2) + 127) / 128) * (npad / 128);
    // Round 3, later (tools/wino_ab.py over bs = 48 ... 256, profiles/r03x_wino_rounds_map.log): what decides is how full the LAST
    // round of tiles is.  r = tiles / CUs: 0.59 x0.89, 0.78 x1.38, 0.97 x1.27, 1.00 x1.15 | 1.16 x0.85, 1.33 x0.94, 1.53 x1.06, 1.66 x1.16,
    // 1.94 x1.29, 2.31 x1.01, 2.64 x1.14, 3.06 x1.07, 3.97 x1.13, 5.28 x1.09.  Rule for a launch that has the chip to itself:
    // up to one round r >= 0.62; beyond, r / ceil(r) >= 0.75.  Under two concurrent lanes (YV3_OPT_TWO_LANES) the other lane's
    // launch fills the idle part of a round: r >= 0.27 (the 13x13 layers at 32 images per lane, 104 tiles, run x0.78 alone but the
    // two-lane step gains 2.6-3.8 % with them; at 64 / 128 images per lane the 1.33-round 26x26 layers gain too: bs=128 +2.9 %, bs=256
    // +5.5 %, profiles/r03y_wino_two_lanes_rule_ab.txt, r03x_wino_big_batch.txt)
    if (d->options & YV3_OPT_WINO_ALWAYS) return true;
#ifndef YV3_AB_NO_TWO_LANES_RULE
    if (d->options & YV3_OPT_TWO_LANES) return tiles * 100 >= 27 * ncu;
#endif
    if (tiles * 100 <= 105 * ncu) return tiles * 100 >= 62 * ncu;
    return tiles * 100 >= 75 * ((tiles + ncu - 1) / ncu) * ncu;
}

yv3_planes_choice yv3_select_planes(const yv3_conv_desc* d, int np, int ncu_) {
    yv3_planes_choice c = {};
    c.form = YV3_FORM_DIRECT; c.launches = 1;
    const auto fail = [&c](int rc) { c.rc = rc; return c; };
    const auto pick = [&c](yv3_planes_kernel k, int ntiles, yv3_planes_loop loop = YV3_LOOP_PLAIN) { c.kernel = k; c.ntiles = ntiles; c.loop = loop; return c; };
    const long long ncu = ncu_;
    const bool k3 = d->k == 3, dual = d->cin_up > 0, out_f32 = d->out_dtype == YV3_F32;
    const int npad = d->cout_pad, tune1 = d->tune[1];

    // ---- the shape errors yv3_conv2d reports before it launches anything
    if (d->dec_out && (d->out_dtype != YV3_F32 || d->cout % 3 || d->dec_stride <= 0.f)) return fail(YV3_ESHAPE);
    const yv3_conv_shape sh = yv3_conv_out_shape(d);
    const long long M = sh.M;
    if (M > 0x7fffffffLL) return fail(YV3_ESHAPE);
    c.Ho = sh.Ho; c.Wo = sh.Wo; c.M = (int)M;
    if (!out_f32 && (d->cout % 8)) return fail(YV3_ESHAPE);
    const int tb = npad < 128 ? npad : 128;
    if (tb <= 0 || npad % tb) return fail(YV3_ESHAPE);
    if (out_f32 && (k3 || dual)) return fail(YV3_ESHAPE);      // fp32 outputs are the 1x1 head convs
    const int nk = d->k * d->k * d->cin / YV3_SEL_CHUNK;
    const bool use_pp = !(d->options & YV3_OPT_NO_PINGPONG);   // ping-pong main loop (fp16x2 and the bf16 6-deep ring, 8-wave tiles) unless disabled

    // ---- the opt-in kw-tap reuse kernel (YV3_OPT_K3S1, conv_planes_k3s1.hip), BEFORE the Winograd rule: 44 % less L2->LDS traffic, same
    // results, but no faster on MI355X because this MFMA stream is power-limited -- opt-in until that changes.
    // (k = 3, stride 1, no dual source, plane output; channel tiles of 128 or 64)
    if (k3 && d->stride == 1 && !out_f32 && (d->options & YV3_OPT_K3S1) && d->cin % YV3_SEL_CHUNK == 0 && (npad % 128 == 0 || npad % 64 == 0)) {
        if (npad % 128 == 0) {
            const long long blocks256 = ((M + 255) / 256) * (npad / 128);
            return pick(blocks256 >= 512 ? YV3_PK_K3S1_256x128 : YV3_PK_K3S1_128x128, npad / 128);
        }
        return pick(YV3_PK_K3S1_128x64, npad / 64);
    }

    // ---- Winograd F(2x2,3x3): input transform (winograd.hip) + the 16-position GEMM with the output transform folded into the main loop
    if (planes_wino_rule(d, np, ncu)) {
        const long long T = (long long)d->B * ((d->H + 1) / 2) * ((d->W + 1) / 2);
        if (T > 0x7fffffffLL || npad % 128 || d->cin % 32) return fail(YV3_ESHAPE);
        const size_t vbytes = (size_t)2 * 16 * T * d->cin * sizeof(unsigned short);
        if (!d->wino_ws || d->wino_ws_bytes < vbytes) return fail(YV3_EWORKSPACE);
        c.form = YV3_FORM_WINOGRAD; c.launches = 2;
        const long long total = ((T + 127) / 128) * (npad / 128);
        // Schedules.  Default: one 128x128 tile (all 16 positions, 16 x Cin/32 chunks) per workgroup -- bitwise independent of the
        // batch composition.  YV3_OPT_WINO_EVEN: stream-K over transform positions -- one persistent workgroup per CU takes an equal,
        // contiguous range of (tile, position) units of its XCD and hands partial outputs over inside the XCD's L2 (see the
        // kernel); a split tile is summed head + tail.  Measured (tools/wino_ab.py, profiles/r03_wino_ab2.log): it only wins below
        // half a round of tiles (512->1024 @19x19 bs=16: 0.176 vs 0.202 ms) and loses 3...30 % above (256 KB of partial outputs per
        // split, no dynamic tile dispatch, and a partly filled round simply clocks higher on this power-limited chip): opt-in.
        const bool even = (d->options & YV3_OPT_WINO_EVEN) && ncu <= YV3_WINO_SK_MAX_WG && total * 16 >= ncu &&
                          (int)total % ncu_ != 0 && d->wino_ws_bytes >= vbytes + yv3_wino_sk_bytes();
        // two-group ping-pong loop (default) or the rolling single-phase loop (one barrier per chunk, fragment reads spread under the
        // MFMAs; tune[1] bit 1: A/B measurements -- bit-identical, equal speed: profiles/r04d_wino_roll_vs_pingpong_ab.log; the same stage
        // on FOUR waves with 64x64 wave tiles and the rolling loop was 1.4x slower, profiles/r04f_wino_4waves_roll_ab.log)
#ifndef YV3_WINO_ROLL
#define YV3_WINO_ROLL 0            // (A/B builds, -DYV3_MEASURE: 1 swaps the two loops' roles -- the build tools/timelines/roll.py reads its timeline from)
#endif
        if (even) { c.grid = ncu_; return pick(YV3_PK_WINO_EVEN, npad / 128, YV3_LOOP_PINGPONG); }
        if (((tune1 & YV3_T1P_WINO_OTHER_LOOP) != 0) != YV3_WINO_ROLL) return pick(YV3_PK_WINO_ROLL, npad / 128, YV3_LOOP_ROLLING);
        return pick(YV3_PK_WINO_PINGPONG, npad / 128, YV3_LOOP_PINGPONG);
    }

    // ---- direct tiles
    if (npad % 128 == 0) {
        // 256x128 tiles (8 waves, 144 KB LDS; 64x64 per wave) from half a round of tiles upwards, else 128x128 tiles
        // (8 waves of 32x64).  Measured at bs=64: the 13x13 layers have 172 / 344 big tiles (0.7 / 1.3 rounds) and are
        // still 5 % (3x3) to 26 % (1x1) faster than with 340 / 680 small ones -- the big tile does 1/3 less LDS
        // traffic per MFMA, and a partly filled round simply clocks higher on this power-limited kernel.
        const long long blocks256 = ((M + 255) / 256) * (npad / 128);
        const int nt128 = npad / 128, nt256 = npad / 256;
        // (with the stream-K schedule every CU gets the same share whatever the tile count: one tile per CU suffices)
        const bool sk_ok = np == 2 && d->workspace && use_pp;
        // The eight-wave 256x128 / 128x128 tiles (rows = 256 / 128): fp16 planes run the ping-pong loop (3- / 4-deep ring) unless it is disabled, one or
        // three bf16 planes the plain loop (the 2- / 3-deep ring; three planes have no ping-pong instantiation) -- and the fp16-plane ping-pong
        // tiles the persistent stream-K schedule, one workgroup per CU, by the rule below.

        // (num_cu: of the CURRENT device; multiple of 8: equal workgroups per XCD)
        // stream-K: opt-in (the caller passes yv3_conv_desc.workspace): a split tile is summed as head + middle.. + tail, so its rounding
        // depends on where the split falls, i.e. on the batch size / the image's position in the batch -- results stay
        // within the parity tolerance but are no longer bit-identical across batch compositions.
        // It is used only for launches of fewer than two rounds of tiles (the 13x13 layers at bs=64; nearly every layer of a
        // small batch, where it splits each tile's K range over the otherwise idle CUs): filling the idle CUs of a last
        // partial round buys nothing on this power-limited kernel (the busy CUs simply clock higher: measured -9 % on the
        // 2.6- and 5.3-round layers, which also lose the hardware's dynamic tile dispatch), but with 1.3 rounds the even
        // split wins, and it lets the 13x13 3x3 layers use 256x128 tiles (+9 ... +11 %).
        // Measured rule (tools/conv_bench.py, bs = 4 ... 64): it pays for the long-K 3x3 layers when the tiles fill 1 - 2
        // rounds (even split instead of a 30 - 100 % idle second round) or at most 0.4 rounds (each tile's K range spread
        // over the idle CUs: the 13x13 3x3 layer at bs=4 0.084 -> 0.039 ms); it loses for 1x1 layers (the accumulator
        // exchange outweighs their few K chunks) and around 0.7 rounds.
        const auto pick_w8 = [&](yv3_planes_kernel k, int rows) {
            const long long num_cu = ncu, total = ((M + rows - 1) / rows) * nt128;
            const bool sk_shape = k3 && ((total >= num_cu && total < 2 * num_cu) || 5 * total <= 2 * num_cu);
            c.stream_k = sk_ok && sk_shape && (long long)total * nk >= num_cu &&
                         num_cu <= YV3_SK_MAX_WG && d->workspace_bytes >= yv3_sk_bytes();
            if (c.stream_k) c.grid = ncu_;
            return pick(k, nt128, np == 2 && use_pp ? YV3_LOOP_PINGPONG : YV3_LOOP_PLAIN);
        };
        const int big_min = d->big_tile_min > 0 ? d->big_tile_min : 128;
        const int force = (int)((d->options >> YV3_OPT_TILE_SHIFT) & 0xffu);
        // (code 12: the four-wave 256x128 tile with 16-deep chunks, two workgroups per CU -- conv_planes_w4.hip; it needs two K chunks)
        const bool w4_shape = np == 2 && !out_f32 && !dual && nk >= 2;
        if (force == YV3_TILE_W4_192x128 && w4_shape) return pick(YV3_PK_W4_192x128, nt128);
        if (np != 3 && force == YV3_TILE_128x128_W4) return pick(YV3_PK_128x128_W4, nt128);
        // 256x128 tile on FOUR waves (128x64 wave tiles: 6 fragment reads per 8 MFMAs instead of 4 per 4), two workgroups per CU
        if (np == 1 && force == YV3_TILE_256x128_W4) return pick(YV3_PK_256x128_W4, nt128);
        // 256x256 tile on eight waves (128x64 wave tiles), one workgroup per CU, single-phase loop
        const bool t256_ok = np == 1 && npad % 256 == 0 && !out_f32;
        if (t256_ok && force == YV3_TILE_256x256) return pick(YV3_PK_256x256, nt256);
        // (code 8: the 256x256 tile with the rolling loop; code 9: 4-deep ring)
        if (t256_ok && force == YV3_TILE_256x256_ROLL) return pick(YV3_PK_256x256_ROLL, nt256, YV3_LOOP_ROLLING);
        if (t256_ok && force == YV3_TILE_256x256_ROLL4) return pick(YV3_PK_256x256_ROLL4, nt256, YV3_LOOP_ROLLING);
        // (code 11: the 192-row variant of the 256x256 rolling tile -- 96x64 wave tiles; also measured and dropped: 192x128 on four waves
        // and 128x256 on eight, profiles/r04aa_bf16_192row_tiles_ab.log)
        // (codes 13 / 14: the 256x256 tile with the eight-wave PING-PONG loop, 128x64 wave tiles, 3- / 4-deep ring; 14 is what the rule below ships)
        if (t256_ok && force == YV3_TILE_256x256_PP3) return pick(YV3_PK_256x256_PP3, nt256, YV3_LOOP_PINGPONG);
        if (t256_ok && force == YV3_TILE_256x256_PP4) return pick(YV3_PK_256x256_PP4, nt256, YV3_LOOP_PINGPONG);
        // (code 15: the 192-row variant with the ping-pong loop)
        if (t256_ok && force == YV3_TILE_192x256_PP3) return pick(YV3_PK_192x256_PP3, nt256, YV3_LOOP_PINGPONG);
        // (code 16: ... with a 4-deep ring: one more chunk of prefetch lead)
        if (t256_ok && force == YV3_TILE_192x256_PP4) return pick(YV3_PK_192x256_PP4, nt256, YV3_LOOP_PINGPONG);
        if (t256_ok && force == YV3_TILE_192x256_ROLL) return pick(YV3_PK_192x256_ROLL, nt256, YV3_LOOP_ROLLING);
        if (np == 2 && force == YV3_TILE_128x64) return pick(YV3_PK_128x64, npad / 64);
        // Round 5: the four-wave 192x128 tile, TWO workgroups per CU (conv_planes_w4.hip): one workgroup's prologue / epilogue / launch gap
        // under the other's main loop; bit-identical to the eight-wave tile (same K order).  Same-box A/B, bs=64 (profiles/r05e_w4_192x128_ab.txt):
        // 128->256 @52 +4 %, 64->128 @104 +5 %, 512->256 1x1 @26 +12 %, 256->128 1x1 @52 +6 %, 512->1024 s2 @13 +11 %; at bs=32 256->512 @26
        // +16 %, 512->1024 @13 +9 % (192-row tiles fill the chip's last round better); 256->512 @26 bs=64 -3 %, long K (512->256 3x3 @52) -5 %.
        // (tune[1] bit 5: off, bit 6: off for 1x1 layers, bit 7: off for 3x3 layers -- A/B measurements)
        // End to end (profiles/r05h_w4_end_to_end_ab_other_batches.txt, r05j_*): 416x416 bs=16 +7.7 %, bs=32 +3.8 %, bs=8 +2.3 %, 608x608 bs=16 +4 %,
        // dense 608x608 bs=8 +3.4 %, bs=64 on one lane +0.8 % (the chip is power-limited there: 16 % more tile rows per CU-cycle by the kernel's own
        // timeline, profiles/r05f_w4_timeline.txt, buy 4 % in isolation and ~1 % in the network).  Under TWO concurrent lanes the 3x3 layers lose
        // with it (bs=64: -1.2 %; three alternating passes) while the 1x1 layers still gain (+0.2 %): there only the 1x1 layers take it.
        const bool w4_lanes_ok = !(d->options & YV3_OPT_TWO_LANES) || !k3 || (tune1 & YV3_T1P_W4_LANES_3X3);
        if (force == YV3_TILE_AUTO && w4_shape && !(tune1 & YV3_T1P_NO_W4) && (k3 || nk >= 8) && !(tune1 & (k3 ? YV3_T1P_NO_W4_3X3 : YV3_T1P_NO_W4_1X1)) && w4_lanes_ok) {
            const long long t192 = ((M + YV3_SEL_W4_BM - 1) / YV3_SEL_W4_BM) * (npad / YV3_SEL_W4_BN);
            // from three quarters of a workgroup per CU upwards (512->1024 @19x19 bs=8: 128 tiles on 256 CUs, one four-wave workgroup on
            // every other CU, 219 instead of 292 TFLOP/s; 232 tiles @13x13 bs=32: +5 %; profiles/r05i_w4_layers_*.txt)
            if (t192 * 4 >= 3 * ncu) return pick(YV3_PK_W4_192x128, nt128);
        }
        // short-K 1x1 layers (K <= 512: 8-16 chunks per tile, mostly prologue / epilogue): two independent 4-wave workgroups
        // per CU (128x128 tiles, 2-deep ring) hide each other's IO -- in the network at bs=64 the step gains 0.8 %
        // (13.31 -> 13.20 ms, same box, alternating; K = 1024 does not gain); same K order, same bits
        // (the head convs at 52x52 / 26x26 included: +0.2...0.7 %; the 104x104 3x3 layers, K = 576, lose 1 % on it)
        if (np == 2 && !k3 && nk <= 16 && force == YV3_TILE_AUTO && blocks256 >= big_min && !(tune1 & YV3_T1P_NO_SHORT_K))
            return pick(YV3_PK_128x128_W4, nt128);
        if (force == YV3_TILE_256x128_W8) return pick_w8(YV3_PK_256x128_W8, 256);
        if (force == YV3_TILE_128x128_W8) return pick_w8(YV3_PK_128x128_W8, 128);
        // one bf16 plane (YV3_BF16): the same ping-pong loop with one MFMA per unit -- 608x608 bs=16: 2727 -> 3155
        // images/s on one lane (two 4-wave workgroups per CU instead: 2953)
        // (6-deep ring, 147 KB: with 8 MFMAs per chunk and wave a DMA piece needs several chunk times to land; 3-deep 3690, 4-deep
        // 3830, 6-deep 3870 images/s at 608x608 bs=16)
        // ... and from one tile per CU upwards the same 256x128 tile on FOUR waves (128x64 wave tiles: 6 fragment reads per 8 MFMAs
        // instead of 4 per 4, half the DMA pieces per MFMA and wave), two independent workgroups per CU (72 KB of LDS each, <= 256
        // registers), single-phase loop, epilogue in two rounds of 64 rows: same K order, bit-identical.  Same-box A/B
        // (tools/tile_ab.py, profiles/r03_bf16_tile_ab*.log), 608x608 bs=16: 128->256 @76 665 -> 772 TFLOP/s, 256->512 @38 670 -> 811,
        // 64->128 @152 559 -> 691, the stride-2 layers +11...18 %, 256->128 1x1 @76 +12 %; 416x416 bs=64: @52 663 -> 831, @26 825 -> 901,
        // @13 702 -> 846.  Below one tile per CU (512->1024 @19 at bs=16: 184 tiles, 1x1 layers at 38 / 19) the 8-wave ping-pong
        // tile wins by 7...30 % (twice the waves per tile).  A 256x256 / 8-wave tile (code 6) loses to both at these sizes.
        // (tune[2] > 0: threshold override for A/B measurements)
        // (code 7: the same tile with the rolling loop -- barrier between the k-steps, next chunk's first fragments read under the MFMAs)
        if (np == 1 && force == YV3_TILE_256x128_W4_ROLL) return pick(YV3_PK_256x128_W4_ROLL, nt128, YV3_LOOP_ROLLING);
        // Round 4 (tools/tile_ab.py, profiles/r04d_bf16_roll_ab.log, r04j_bf16_tiles_ab.log): the 3x3 layers take the ROLLING loop on that
        // tile (+2...6 %; the 1x1 layers lose 1-3 % on it and keep the plain loop) -- and a 256x256 tile on eight waves (128x64 wave tiles,
        // one workgroup per CU, rolling loop: 32 KB of DMA per 128 MFMAs instead of 24 KB per 64 -- the L2 -> LDS path delivers 62 B/clk/CU,
        // tools/probes/dma_rate.hip, and was the 256x128 tile's co-bottleneck) when its tile count fills the chip's last round:
        // 676 tiles (128->256 @52x52 bs=64) +8 %, 172 (512->1024 @13x13 bs=64) +15 %, 182 (256->512 @38x38 bs=16) +14 %; but 338
        // (1.32 rounds) -7 %, 361 -6 %, 92 -28 %.  Rule: r = tiles / CUs; r >= 0.6 up to one round, r / ceil(r) >= 0.8 beyond.
        if (np == 1 && force == YV3_TILE_AUTO && k3 && !out_f32 && npad % 256 == 0 && !(tune1 & YV3_T1P_BF16_ROUND3)) {
            const long long t256 = ((M + 255) / 256) * (npad / 256);
            const bool fill = t256 <= ncu ? t256 * 10 >= 6 * ncu : t256 * 10 >= 8 * ((t256 + ncu - 1) / ncu) * ncu;
            // ... and its 192-row variant (96x64 wave tiles; a wave stages 24 pixel rows = one DMA piece and a half) where that fills the
            // last round to >= 85 % and 256 rows leave it below 80 %: 256->512 @38x38 bs=16 (182 -> 242 tiles) +6 %, 512->1024 @13x13 bs=64
            // (172 -> 228) +5 %, 128->256 @76x76 bs=16 (361 -> 482) +2.6 %, @76x76 bs=8 +9 % (profiles/r04aa_bf16_192row_tiles_ab.log)
            const long long t192 = ((M + 191) / 192) * (npad / 256);
            const long long r256 = (t256 + ncu - 1) / ncu * ncu, r192 = (t192 + ncu - 1) / ncu * ncu;
            // Round 5: both tiles run the eight-wave PING-PONG loop on a 4-deep ring instead of the rolling loop (tune[1] bit 9: the rolling loop,
            // bit 10: ping-pong on the 3-deep ring -- A/B).  The rolling tile's eight waves leave their one barrier together, their fragment
            // reads (96 KB per chunk and CU) queue behind each other and ~350 of a chunk's 1500 cycles are exposed LDS latency
            // (tools/timeline.py --kernel roll_bf16, profiles/r05x_bf16_roll_timeline.txt); with one four-wave group reading while the other issues
            // MFMAs the layers run bit-identical and +5...+14 % faster in isolation, on uniform random operands and on the network's own
            // activations alike (profiles/r05y_bf16_pingpong_*_ab.txt, r05ad_*).  IN the network the 3-deep ring LOSES 2 % (its DMA lead is one
            // compute segment, ~1000 cycles: fine for L2-hot repeats of one layer, too short for a layer's first touch of its weights and
            // inputs); the 4-deep ring gains: conv kernel time 608x608 bs=16 3.17 -> 3.08 ms, 416x416 bs=64 5.21 -> 5.04 ms, step +2 %
            // (profiles/r05ae_*, r05af_*; a per-layer A/B decides nothing by itself).
            const bool roll = (tune1 & YV3_T1P_BF16_ROLL) != 0, pp3 = (tune1 & YV3_T1P_BF16_PP3) != 0;
            if (!(tune1 & YV3_T1P_BF16_NO_192) && t192 * 100 >= 85 * r192 && t256 * 100 < 80 * r256)
                return pick(roll ? YV3_PK_192x256_ROLL : pp3 ? YV3_PK_192x256_PP3 : YV3_PK_192x256_PP4, nt256, roll ? YV3_LOOP_ROLLING : YV3_LOOP_PINGPONG);
            if (fill) return pick(roll ? YV3_PK_256x256_ROLL : pp3 ? YV3_PK_256x256_PP3 : YV3_PK_256x256_PP4, nt256, roll ? YV3_LOOP_ROLLING : YV3_LOOP_PINGPONG);
        }
        const int w4_min = d->tune[2] > 0 ? d->tune[2] : 256;
        if (np == 1 && force == YV3_TILE_AUTO && k3 && blocks256 >= w4_min && !out_f32 && !(tune1 & YV3_T1P_BF16_ROUND3)) return pick(YV3_PK_256x128_W4_ROLL, nt128, YV3_LOOP_ROLLING);
        if (np == 1 && force == YV3_TILE_AUTO && blocks256 >= w4_min && !out_f32) return pick(YV3_PK_256x128_W4, nt128);
        if (np == 1 && use_pp && force == YV3_TILE_AUTO && blocks256 >= big_min) return pick(YV3_PK_256x128_W8_PP6, nt128, YV3_LOOP_PINGPONG);
        if (blocks256 >= (sk_ok ? 256 : big_min)) return pick_w8(YV3_PK_256x128_W8, 256);
        return pick_w8(YV3_PK_128x128_W8, 128);
    }
    // fp16 planes: 2-deep ring (49 KB) -> three workgroups per CU instead of two (+4 % on the 208x208 3x3 layer)
    if (npad % 64 == 0) return pick(YV3_PK_128x64, npad / 64);
    return pick(YV3_PK_128x32, npad / 32);      // (fp16 planes: +6 % on the 208x208 1x1 layer with the 2-deep ring)
}

// YV3_I8 (conv_planes_i8.hip).  An int8 K chunk is 64 elements = the 64-byte row of a 32-element bf16 chunk, so every count the rules
// above make (K chunks, tiles, rounds of the chip) is that of the bf16 layer with half the input channels: the same rules decide.  Left out of
// the descriptor they see: the opt-in k3s1 kernel, the Winograd operands and the stream-K workspace (rules for other modes anyway).
yv3_planes_choice yv3_select_planes_i8(const yv3_conv_desc* d, int ncu) {
    yv3_planes_choice bad = {};
    bad.rc = YV3_ESHAPE;
    if (d->cin % 64 || d->cin_up % 64 || (d->cin - d->cin_up) % 64 || d->cout % 8 || d->cout_pad % 32) return bad;
    if (d->x_plane_stride > 0 || d->x2_plane_stride > 0 || d->y_plane_stride > 0) return bad;       // (no batch slices)
    yv3_conv_desc h = *d;
    h.cin = d->cin / 2; h.cin_up = d->cin_up / 2;
    h.dtype = YV3_BF16; h.out_dtype = YV3_BF16;
    h.options &= ~(YV3_OPT_K3S1 | YV3_OPT_WINO_EVEN | YV3_OPT_WINO_ALWAYS);
    h.w_wino = nullptr; h.alpha_wino = nullptr; h.wino_ws = nullptr; h.wino_ws_bytes = 0; h.w_wino4 = nullptr;
    h.workspace = nullptr; h.workspace_bytes = 0; h.dec_out = nullptr;
    return yv3_select_planes(&h, 1, ncu);
}

// =========================================================================================== exact fp32

// The even schedule of an F(4x4) launch: n_full whole-item workgroups + the other items cut into `parts` ranges of 6 / parts patch rows (parts = 1:
// one item per workgroup throughout).  Measured (tools/wino4_even_ab.py, profiles/r06w_wino4_even_parts_calibration.txt): cutting pays when
// it puts otherwise idle CUs to work -- a tail of few items behind full rounds (520 items: 512 + 8 x 6: 0.259 -> 0.209 ms), small batches
// (512->1024 @13x13, one image: 16 items, 0.173 -> 0.062 ms, where the direct kernel takes 0.111) -- and not when the tail already
// covers most CUs once (784 items: 272 x 3 parts 0.355 against 0.360 ms; 1352 items of 128 channels: slower): lone workgroups run their
// rows 2x faster than two per CU, and every part pays its ring fill, hand-over and flag.  The rule is that model, in chunk times:
//   rows per part x chunks per row x (1 while the parts leave one workgroup per CU, 2 up to two, 2 x rounds beyond) + 29 + 5 parts
// against the uncut tail; behind full rounds only cuts that stay at one workgroup per CU.  The smallest wins (checked against all 23
// measured shapes).  Not under YV3_OPT_WINO4_TILES (callers that share the GPU with other work, net.stream_k = False: a range with
// row 0 waits for its partners).  tune[1]: 1 never, 2 no full rounds (every item cut: measurements); tune[2]: parts forced.
static long long wino4_tail_cost(long long tail, int P, int nkx, int ncu, bool lone_only) {
    const long long W = tail * P;
    if (P > 1 && (8 * ((tail + 7) / 8) * P > YV3_SEL_WINO4_MAX_TAIL_WG || (lone_only && W > ncu))) return -1;
    const long long f = W <= ncu ? 1 : W <= 2 * ncu ? 2 : 2 * ((W + 2 * ncu - 1) / (2 * ncu));
    return (6 / P) * nkx * f + (P > 1 ? 29 + 5 * P : 0);
}
static void wino4_schedule(const yv3_conv_desc* d, long long items, int ncu, int* n_full, int* parts) {
    const int slots = 2 * ncu;
    *n_full = (int)items; *parts = 1;
    if ((d->options & YV3_OPT_WINO4_TILES) || d->tune[1] == YV3_T1_WINO4_NO_EVEN || items < 1) return;
    const long long full = d->tune[1] == YV3_T1_WINO4_NO_FULL ? 0 : (items / slots) * slots;
    const long long tail = items - full;
    if (tail == 0) return;
    const int nkx = 6 * (d->cin / 32);
    int best = 1; long long best_cost = wino4_tail_cost(tail, 1, nkx, ncu, false);
    for (int P = 2; P <= 6; ++P) {
        if (6 % P) continue;
        const long long cost = wino4_tail_cost(tail, P, nkx, ncu, full > 0);
        if (cost >= 0 && cost < best_cost) { best = P; best_cost = cost; }
    }
    if ((d->tune[2] == 2 || d->tune[2] == 3 || d->tune[2] == 6) && wino4_tail_cost(tail, d->tune[2], nkx, ncu, false) >= 0) best = d->tune[2];
    if (best == 1) return;
    *n_full = (int)full; *parts = best;
}

// Is the F(4x4) form the fastest one of this launch?  From a number of items on, which depends on the channels (the direct kernel's
// competitiveness: it has 64 x 64 tiles for small launches) and on whether the even schedule may cut the items: >= 256 input channels:
// always (one 13x13 image, 16 items: 0.062 ms against the direct kernel's 0.111; 26x26: 0.053 / 0.059); 128: from 0.17 items per CU
// (44 items: 0.049 / 0.050; 24: 0.048 / 0.032); 64: from 0.39 (86 items: 0.044 / 0.039, 128: 0.044 / 0.048).  One item per workgroup
// only (YV3_OPT_WINO4_TILES): from 0.3 items per CU, the round-6 crossover (profiles/r06o_wino4_forms_by_batch.txt).
static bool wino4_pays(const yv3_conv_desc* d, long long items, long long ncu) {
    if ((d->options & YV3_OPT_WINO4_TILES) || d->tune[1] == YV3_T1_WINO4_NO_EVEN) return items * 10 >= 3 * ncu;
    return d->cin >= 256 ? true : d->cin == 128 ? items * 100 >= 17 * ncu : items * 100 >= 39 * ncu;
}

yv3_f32_choice yv3_select_f32(const yv3_conv_desc* d, int ncu_) {
    yv3_f32_choice c = {};
    c.form = YV3_FORM_DIRECT; c.launches = 1; c.parts = 1;
    const auto fail = [&c](int rc) { c.rc = rc; return c; };
    const auto pick = [&c](yv3_f32_kernel k, int ntiles) { c.kernel = k; c.ntiles = ntiles; return c; };
    const long long ncu = ncu_;
    const bool k3 = d->k == 3, dual = d->cin_up > 0;
    const int tune0 = d->tune[0];
    const yv3_conv_shape sh = yv3_conv_out_shape(d);
    const long long M = sh.M;
    if (M > 0x7fffffffLL) return fail(YV3_ESHAPE);
    c.Ho = sh.Ho; c.Wo = sh.Wo; c.M = (int)M;
    c.pin = !(d->options & YV3_OPT_TWO_LANES);                    // (see PIN, conv_igemm_f32.hip)

    // ---- F(4x4,3x3) (csrc/conv_wino4_f32.hip): 4x fewer matrix instructions than direct.  Its workgroups are 64 channels x 32 tiles of 4x4 pixels,
    // two per CU: taken by wino4_pays (tune[0] == 10: never, 11: whenever the filters are there).  Round 6, one item per workgroup, same box,
    // direct / F(2x2) / F(4x4) (profiles/r06o_wino4_forms_by_batch.txt): it is the fastest form of every eligible layer from 8 images of
    // 416x416 up (bs=8: 128->256 @52 0.139 / 0.117 / 0.070 ms, 256->512 @26 0.136 / 0.185 / 0.105; 64 workgroups: 0.187 / 0.337 / 0.182);
    // at 88 workgroups (bs=4 @52) 0.072 / 0.110 / 0.065, at 56 (bs=4 @26) 0.096 / 0.184 / 0.103 -- the crossover
    if (d->w_wino4 && d->wino_ws && k3 && d->stride == 1 && !dual && d->cout % YV3_SEL_WINO4_CHANNELS == 0 && (d->cin == 64 || d->cin % 128 == 0) &&
        d->cout_pad == d->cout && d->alpha && tune0 != YV3_T0_WINO4_NEVER) {
        // workgroups' worth of work of the GEMM stage = its items
        const long long T = (long long)d->B * ((d->H + 3) / 4) * ((d->W + 3) / 4);
        const long long items = ((T + YV3_SEL_WINO4_TILES - 1) / YV3_SEL_WINO4_TILES) * (d->cout / YV3_SEL_WINO4_CHANNELS);
        if ((d->options & YV3_OPT_WINO_ALWAYS) || tune0 == YV3_T0_WINO4_ALWAYS || wino4_pays(d, items, ncu)) {
            if (d->wino_ws_bytes < yv3_wino4_ws_bytes(d->B, d->H, d->W, d->cin)) return fail(YV3_EWORKSPACE);
            const unsigned long long vb = 36ull * T * d->cin * 4, ub = 36ull * d->cout * d->cin * 4;
            if (vb > 0xffffffffull || ub > 0xffffffffull) return fail(YV3_ESHAPE);        // (32-bit buffer offsets: V of at most 4 GB)
            if (items * 6 > 0x7fffffffLL) return fail(YV3_ESHAPE);
            c.form = YV3_FORM_WINOGRAD4; c.launches = 2;
            wino4_schedule(d, items, ncu_, &c.n_full, &c.parts);
            return pick(YV3_FK_WINO4, d->cout / YV3_SEL_WINO4_CHANNELS);
        }
    }

    // ---- F(2x2,3x3): fp32 MFMA throughout, 2.25x fewer matrix instructions; differs from the direct kernel (an fmaf chain in K order) by
    // fp32 round-off of the re-associated sums.
    if (d->w_wino && d->alpha_wino && k3 && d->stride == 1 && !dual && d->cout % 128 == 0 && d->cout_pad == d->cout) {
        // fp32 MFMA runs at the vector rate, so this layer is matrix-bound whatever its shape: Winograd whenever the 128x128 tiles
        // (a quarter of the direct kernel's rows) still fill a good part of the chip, or YV3_OPT_WINO_ALWAYS
        const long long T2 = (long long)d->B * ((d->H + 1) / 2) * ((d->W + 1) / 2);
        const long long t128 = ((T2 + 127) / 128) * (d->cout / 128);
        if ((d->options & YV3_OPT_WINO_ALWAYS) || t128 * 100 >= 40 * ncu) {
            if (!d->wino_ws || d->wino_ws_bytes < (size_t)16 * T2 * d->cin * sizeof(float)) return fail(YV3_EWORKSPACE);
            c.form = YV3_FORM_WINOGRAD; c.launches = 2;
            // Round 5: the stage keeps five accumulator sets (216 registers): its 128x128 eight-wave tile runs ONE workgroup per CU, and a launch whose
            // tiles fill e.g. 1.33 rounds of the chip (256->512 @26x26 bs=64: 340 tiles on 256 CUs) spends a whole second tile time on 84 tiles.  The
            // same wave tiles (32x64) as a 64x128 tile on FOUR waves, two workgroups per CU (2 x 55 KB of LDS), halve the scheduling quantum: the last
            // round's half-size tiles spread over more CUs.  Same K order per accumulator: bit-identical.  Chosen when the 128-row tiles leave the last
            // round at most two thirds full beyond the first round, or fill at most half of the chip (then twice as many CUs work).  Same box,
            // alternating (tools/wino_f32_tile_ab.py, profiles/r05t_f32_wino_four_wave_tile_ab.txt): 256->512 @26 bs=64 (340 tiles) 0.615 -> 0.515 ms,
            // 128->256 @52 bs=32 (338) 0.362 -> 0.308, 512->1024 @13 bs=32 (104) 0.549 -> 0.349, @19 bs=16 (104) 0.549 -> 0.349; 200 / 172 / 184 tiles
            // (0.67-0.78 of a round): 2-3 % slower, kept on the eight-wave tile.  (tune[0] == 8 / 9: force the four-wave / the eight-wave tile.)
            const long long last = t128 % ncu;
            c.wino2_half = tune0 == YV3_T0_WINO2_HALF || (tune0 != YV3_T0_WINO2_FULL && ((t128 > ncu && last > 0 && 3 * last <= 2 * ncu) || 2 * t128 <= ncu));
            return pick(YV3_FK_WINO2, d->cout / 128);
        }
    }

    // ---- the persistent GEMM (csrc/conv_gemm_f32.hip)?  Plain 1x1 / stride-1 layers and 3x3 layers (any stride; the Winograd forms are ruled
    // out above) without residual or upsample operand whose tiles fill at least one round of the chip (tune[0] == 13: never, 14: whenever
    // the shape fits)
    // (3x3 layers: built, bit-identical and measured -- 113-122 TFLOP/s where the 128x128 eight-wave tiles give 116-124: the long K loops
    // of these layers amortise a tile's prologue and epilogue anyway, profiles/r06ag_gemm_k3_stride2_ab.txt -- taken with tune[0] == 14 only)
    const int np = d->cout_pad;
    const bool g_k1 = d->k == 1 && d->stride == 1, g_k3 = k3 && d->cout % 128 == 0 && tune0 == YV3_T0_GEMM_ALWAYS;
    if ((g_k1 || g_k3) && !d->cin_up && !d->residual && d->cin % 32 == 0 && d->cout % 64 == 0 && d->cout <= 1024 && d->cout_pad == d->cout && tune0 != YV3_T0_GEMM_NEVER &&
        !((long long)d->B * d->H * d->W * d->cin * 4 > 0xfffffe00LL || M * d->cout * 4 > 0xffffffffLL || (long long)d->cout * d->cin * d->k * d->k * 4 > 0xffffffffLL)) {
        const bool wide = d->cout % 128 == 0;
        const int bm = (wide ? 2 : 4) * YV3_SEL_GEMM_WAVE_M, bn = (wide ? 4 : 2) * YV3_SEL_GEMM_WAVE_N, ntn = d->cout / bn;
        const long long mt = (M + bm - 1) / bm;
        if (tune0 == YV3_T0_GEMM_ALWAYS || mt * ntn >= ncu) {
            // Pixel-row tiles that run on the GEMM: whole rounds of the chip (one tile per CU and round), plus the last partial round when it is more
            // than half full (measured, profiles/r06am_gemm1x1_ring_depth4_ab.txt: a rest of 0.28 / 0.33 rounds is cheaper on the small tiles,
            // which fill the chip two to four to a CU -- 0.109 vs 0.111 ms, 0.106 vs 0.125; a rest of 0.64 rounds is cheaper as one more round
            // here: 0.100 vs 0.103, 0.054 vs 0.057; 1352 tiles = 5.28 rounds would cost 6).  Same K order per output element: same bits whoever
            // computes a row.
            long long mt_run = mt;
            if (d->tune[1] != YV3_T1_GEMM_ALL_ROWS) {                          // (every row here -- measurements)
                const long long rounds = mt * ntn / ncu, rest = mt * ntn - rounds * ncu;
                if (rounds >= 1 && rest > 0 && 2 * rest <= ncu) mt_run = rounds * ncu / ntn;
            }
            c.gemm_rows = (int)(mt_run * bm < M ? mt_run * bm : M);
            const long long tiles = ((c.gemm_rows + bm - 1) / bm) * ntn;
            c.gemm_grid = (int)(tiles < ncu ? (tiles + 7) / 8 * 8 : ncu);
            if (c.gemm_rows < M) {
                c.launches = 2;
                c.rest = k3 ? YV3_FK_128x128_W8 : np % 128 == 0 ? YV3_FK_64x64 : YV3_FK_128x64;
                c.rest_ntiles = k3 ? np / 128 : np / 64;
            }
            return pick(k3 ? YV3_FK_GEMM_K3 : wide ? YV3_FK_GEMM_128x128 : YV3_FK_GEMM_256x64, ntn);
        }
    }

    // ---- direct tiles: widest N tile the layer fills; for launches that would leave most of the
    // 256 CUs idle (small batch at 13x13 / 26x26) fall back to 64x64 tiles for 4x the blocks.
    if (np % 128 == 0) {
        const long long blocks128 = ((M + 127) / 128) * (np / 128);
        // (tune[0]: kernel-selection override for A/B measurements -- 6 four-wave 128x128, 2 64x64 tiles)
        if (blocks128 >= 384 && tune0 == YV3_T0_F32_TILE_128_W4) return pick(YV3_FK_128x128_W4, np / 128);
        // eight waves (4 x 2 of 32x64) per 128x128 tile, two workgroups per CU: four waves per SIMD hide each other's fragment
        // reads / barriers better than two (13x13 3x3 layer at bs=64: 80 -> 102 TFLOP/s, whole network +5 %)
        // 1x1 layers (K <= 1024: 8-32 chunks per tile) run better on 64x64 tiles, four workgroups per CU: 512->256 @26x26 at bs=64
        // 82 -> 103 TFLOP/s, 256->128 @52x52 95 -> 98 (tune[0] == 7: 128x128 tiles for them too)
        if (blocks128 >= 384 && tune0 != YV3_T0_F32_TILE_64 && (k3 || tune0 == YV3_T0_F32_TILE_128_1X1)) return pick(YV3_FK_128x128_W8, np / 128);
        return pick(YV3_FK_64x64, np / 64);
    }
    if (np % 64 == 0) return pick(YV3_FK_128x64, np / 64);
    return pick(YV3_FK_128x32, np / 32);
}

// =========================================================================================== names: what yv3_conv2d_kernel prints

const char* yv3_planes_kernel_name(yv3_planes_kernel k) {
    switch (k) {
#define N(x) case YV3_PK_##x: return #x;
        N(256x128_W8) N(128x128_W8) N(128x128_W4) N(128x64) N(128x32) N(256x128_W8_PP6) N(256x128_W4) N(256x128_W4_ROLL)
        N(256x256) N(256x256_ROLL) N(256x256_ROLL4) N(256x256_PP3) N(256x256_PP4) N(192x256_ROLL) N(192x256_PP3) N(192x256_PP4)
        N(W4_192x128) N(K3S1_256x128) N(K3S1_128x128) N(K3S1_128x64) N(WINO_PINGPONG) N(WINO_ROLL) N(WINO_EVEN)
#undef N
    }
    return "?";
}
const char* yv3_planes_loop_name(yv3_planes_loop l) {
    switch (l) {
        case YV3_LOOP_PLAIN: return "plain";
        case YV3_LOOP_ROLLING: return "rolling";
        case YV3_LOOP_PINGPONG: return "pingpong";
    }
    return "?";
}
const char* yv3_f32_kernel_name(yv3_f32_kernel k) {
    switch (k) {
#define N(x) case YV3_FK_##x: return #x;
        N(NONE) N(128x128_W8) N(128x128_W4) N(64x64) N(128x64) N(128x32) N(WINO2) N(WINO4) N(GEMM_128x128) N(GEMM_256x64) N(GEMM_K3)
#undef N
    }
    return "?";
}

// One line: the kernel's name and its channel tiles, the planes' loop / exact fp32's pin, then every other field of the choice that is not at
// its default (absent = no stream-K, no persistent grid, no F(2x2) half tile, not F(4x4), no GEMM rows, no rest)
namespace {
struct line {
    char* buf; size_t room, n = 0; bool ok = true;
    line(char* b, size_t bytes) : buf(b), room(bytes < YV3_KERNEL_LINE_BYTES ? bytes : YV3_KERNEL_LINE_BYTES) {}
    void took(int m) { if (m < 0 || (size_t)m >= room - n) ok = false; else n += m; }
    void word(const char* w) { if (ok) took(snprintf(buf + n, room - n, n ? " %s" : "%s", w)); }
    void field(const char* key, int v) { if (ok) took(snprintf(buf + n, room - n, " %s=%d", key, v)); }
    int rc() const { return ok ? 0 : YV3_EINVAL; }
};
}  // namespace

int yv3_describe_planes(const yv3_planes_choice& c, char* buf, size_t buf_bytes) {
    if (!buf || !buf_bytes) return YV3_EINVAL;
    line l(buf, buf_bytes);
    l.word(yv3_planes_kernel_name(c.kernel)); l.field("nt", c.ntiles);
    l.word(yv3_planes_loop_name(c.loop));
    if (c.stream_k) l.word("sk");
    if (c.grid) l.field("grid", c.grid);
    return l.rc();
}
int yv3_describe_f32(const yv3_f32_choice& c, char* buf, size_t buf_bytes) {
    if (!buf || !buf_bytes) return YV3_EINVAL;
    line l(buf, buf_bytes);
    l.word(yv3_f32_kernel_name(c.kernel)); l.field("nt", c.ntiles);
    l.field("pin", c.pin);
    if (c.wino2_half) l.word("half");
    if (c.kernel == YV3_FK_WINO4 || c.n_full || c.parts != 1) { l.field("full", c.n_full); l.field("parts", c.parts); }
    if (c.gemm_rows || c.gemm_grid) { l.field("rows", c.gemm_rows); l.field("grid", c.gemm_grid); }
    if (c.rest != YV3_FK_NONE || c.rest_ntiles) { l.word("rest"); l.word(yv3_f32_kernel_name(c.rest)); l.field("nt", c.rest_ntiles); }
    return l.rc();
}
