// Kernel selection of yv3_conv2d: which form, kernel, tile, ring depth, main loop, schedule and persistent grid a descriptor runs,
// decided in ONE place (conv_select.cpp) and apart from launching it.  Plain host code: no HIP, no runtime call, no static state -- the
// CU count is a parameter, and the selector is its only reader.  yv3_conv2d and its queries yv3_conv2d_form, yv3_conv2d_launches and
// yv3_conv2d_kernel (capi.hip) each call the selector once; the launchers (conv_planes.hip, conv_igemm_f32.hip, ...) fill their parameter
// structs from the descriptor and the choice, switch on the kernel enum and decide nothing: a choice they have no instantiation for is
// YV3_EINVAL.  yv3_conv_desc.options, .big_tile_min and .tune[0..2] are read here and nowhere else.
#pragma once
#include <stddef.h>
#include "yv3.h"

// ---- values of the descriptor's measurement fields (include/yv3.h keeps the public text; tools/ and tests set these numbers)
// bits 8..15 of yv3_conv_desc.options: forced tile of the plane kernels
enum {
    YV3_TILE_AUTO = 0,
    YV3_TILE_256x128_W8 = 1,        // 256x128 / 8 waves
    YV3_TILE_128x128_W8 = 2,        // 128x128 / 8 waves
    YV3_TILE_128x128_W4 = 3,        // 128x128 / 4 waves, two workgroups per CU
    YV3_TILE_128x64 = 4,            // fp16 planes: 128x64 / 4 waves, 2-deep ring
    YV3_TILE_256x128_W4 = 5,        // bf16: 256x128 on four waves, two workgroups per CU
    YV3_TILE_256x256 = 6,           // bf16: 256x256 on eight waves, single-phase loop
    YV3_TILE_256x128_W4_ROLL = 7,   // bf16: code 5 with the rolling loop
    YV3_TILE_256x256_ROLL = 8,      // bf16: code 6 with the rolling loop
    YV3_TILE_256x256_ROLL4 = 9,     //       ... on a 4-deep ring
    YV3_TILE_192x256_ROLL = 11,     // bf16: the 192-row variant of the 256x256 rolling tile
    YV3_TILE_W4_192x128 = 12,       // fp16 planes: the four-wave 192x128 tile of conv_planes_w4.hip
    YV3_TILE_256x256_PP3 = 13,      // bf16: 256x256, eight-wave ping-pong loop, 3-deep ring
    YV3_TILE_256x256_PP4 = 14,      //       ... 4-deep ring (what the rule ships)
    YV3_TILE_192x256_PP3 = 15,      // bf16: 192x256, ping-pong loop, 3-deep ring
    YV3_TILE_192x256_PP4 = 16,      //       ... 4-deep ring
};
// tune[0], exact fp32
enum {
    YV3_T0_F32_TILE_64 = 2,         // direct: 64x64 tiles
    YV3_T0_F32_TILE_128_W4 = 6,     // direct: four-wave 128x128 tiles
    YV3_T0_F32_TILE_128_1X1 = 7,    // direct: 128x128 tiles for the 1x1 layers too
    YV3_T0_WINO2_HALF = 8,          // F(2x2) stage: the four-wave 64x128 tile
    YV3_T0_WINO2_FULL = 9,          // F(2x2) stage: the eight-wave 128x128 tile
    YV3_T0_WINO4_NEVER = 10,
    YV3_T0_WINO4_ALWAYS = 11,       // whenever the filters are there
    YV3_T0_GEMM_NEVER = 13,
    YV3_T0_GEMM_ALWAYS = 14,        // whenever the shape fits (the 3x3 operand path included)
};
// tune[1], exact fp32
enum {
    YV3_T1_WINO4_NO_EVEN = 1,       // F(4x4): one item per workgroup
    YV3_T1_WINO4_NO_FULL = 2,       // F(4x4): no full rounds (every item cut)
    YV3_T1_GEMM_ALL_ROWS = 3,       // persistent GEMM: every row, no rest launch
};
// tune[1], plane kernels: a bit set
enum {
    YV3_T1P_NO_SHORT_K = 1,         // no two-workgroup tile for the short-K 1x1 layers
    YV3_T1P_WINO_OTHER_LOOP = 2,    // Winograd stage: the other main loop (rolling <-> ping-pong)
    YV3_T1P_BF16_ROUND3 = 8,        // bf16: round-3 tile selection (no rolling loop, no 256x256 tile)
    YV3_T1P_BF16_NO_192 = 16,       // bf16: no 192-row variant of the 256x256 tile
    YV3_T1P_NO_W4 = 32,             // fp16 planes: no four-wave 192x128 tile
    YV3_T1P_NO_W4_1X1 = 64,         //   ... not for 1x1 layers
    YV3_T1P_NO_W4_3X3 = 128,        //   ... not for 3x3 layers
    YV3_T1P_W4_LANES_3X3 = 256,     //   ... for 3x3 layers under two lanes too
    YV3_T1P_BF16_ROLL = 512,        // bf16 256x256 / 192x256: the rolling loop
    YV3_T1P_BF16_PP3 = 1024,        //   ... ping-pong on the 3-deep ring
};
// tune[2]: bf16 -- threshold (256x128 tiles) from which the four-wave tile is used; exact fp32 F(4x4) -- parts per tail item forced
// (2, 3 or 6).  (Measurement builds also read it inside kernels, through ConvParamsP::tune: the timeline's workgroup index.)

// ---- tile geometry the rules count with; each kernel file static_asserts that these equal its own
constexpr int YV3_SEL_CHUNK = 32;              // K elements per chunk of every convolution kernel
constexpr int YV3_SEL_W4_BM = 192, YV3_SEL_W4_BN = 128;        // conv_planes_w4.hip's tile
constexpr int YV3_SEL_GEMM_WAVE_M = 64, YV3_SEL_GEMM_WAVE_N = 32;      // conv_gemm_f32.hip: wave tile; 2 x 4 waves = 128x128, 4 x 2 = 256x64
constexpr int YV3_SEL_WINO4_TILES = 32, YV3_SEL_WINO4_CHANNELS = 64;  // conv_wino4_f32.hip: one item = 32 tiles of 4x4 pixels x 64 channels
// (the plane / fp32 implicit-GEMM tiles -- 256, 192, 128 or 64 rows by 256, 128, 64 or 32 channels -- are template arguments at the
// launchers' switch; an enumerator's name carries them)

// stream-K workspace of the direct fp16-plane tiles (yv3_conv_desc.workspace, yv3_conv_workspace_bytes()): YV3_SK_MAX_WG parts -- one
// 512-thread workgroup's accumulators per CU -- then as many flags
#define YV3_SK_MAX_WG 512
#define YV3_SK_PART_BYTES (512 * 64 * 4)
static inline size_t yv3_sk_bytes() { return (size_t)YV3_SK_MAX_WG * (YV3_SK_PART_BYTES + sizeof(int)); }
// Hand-over area of the Winograd stages' even schedules (tail of yv3_conv_desc.wino_ws): YV3_WINO_SK_MAX_WG parts, then as many flags.
// A part holds one workgroup's partial outputs: four output accumulator sets of a 512-thread workgroup (F(2x2), fp16 planes: 256 KB) or
// the sixteen outputs of a 256-thread workgroup (F(4x4), exact fp32: 128 KB of it).
#define YV3_WINO_SK_MAX_WG 512
#define YV3_WINO_SK_PART_BYTES (512 * 128 * 4)
static inline size_t yv3_wino_sk_bytes() { return (size_t)YV3_WINO_SK_MAX_WG * (YV3_WINO_SK_PART_BYTES + sizeof(int)) + 256; }
constexpr int YV3_SEL_WINO4_MAX_TAIL_WG = 2 * YV3_WINO_SK_MAX_WG - 1;     // tail workgroups of an even F(4x4) launch (their parts + one part's room for the flags fill the area)
// bytes of yv3_conv_desc.wino_ws for the F(4x4) form of a B x H x W x cin input: V + the hand-over area of the even schedule (parts +
// flags: the LAST yv3_wino_sk_bytes() bytes of whatever buffer the caller passes, rounded down to 256 -- zero-filled once by the
// caller, like the F(2x2) stage's)
static inline size_t yv3_wino4_v_bytes(int B, int H, int W, int cin) { return (size_t)36 * B * ((H + 3) / 4) * ((W + 3) / 4) * cin * sizeof(float); }
static inline size_t yv3_wino4_ws_bytes(int B, int H, int W, int cin) { return ((yv3_wino4_v_bytes(B, H, W, cin) + 255) & ~(size_t)255) + yv3_wino_sk_bytes(); }

// ---- the choice.  An enumerator names tile, waves and ring of a launch, the loop kind and the schedule beside it the main loop: together
// one kernel instantiation (the plane count NP, 3x3 / dual-source / fp32-output are properties of the descriptor, not choices: the
// launchers take them from there).
enum yv3_planes_kernel {
    // conv_planes_kernel.h launch_cfg<NP, BM, BN, WM, WN, ring, ...>: rows x channels, waves
    YV3_PK_256x128_W8,          // 8 waves; ring 2 (3 for fp16 planes).  fp16 planes: ping-pong loop (plain under YV3_OPT_NO_PINGPONG), stream-K by
                                // the rule; one or three bf16 planes: plain loop
    YV3_PK_128x128_W8,          // 8 waves; ring 3 (4 for fp16 planes); loops and schedule as above
    YV3_PK_128x128_W4,          // 4 waves, two workgroups per CU, ring 2, plain loop
    YV3_PK_128x64,              // 4 waves, ring 2, plain loop
    YV3_PK_128x32,              // 4 waves, ring 2, plain loop
    YV3_PK_256x128_W8_PP6,      // bf16: 8-wave ping-pong loop, 6-deep ring
    YV3_PK_256x128_W4,          // bf16: 4 waves, two workgroups per CU, ring 3, plain loop
    YV3_PK_256x128_W4_ROLL,     //   ... rolling loop
    YV3_PK_256x256,             // bf16: 8 waves, single-phase loop, ring 3
    YV3_PK_256x256_ROLL,        //   ... rolling loop, ring 3
    YV3_PK_256x256_ROLL4,       //   ... rolling loop, ring 4
    YV3_PK_256x256_PP3,         //   ... ping-pong loop, ring 3
    YV3_PK_256x256_PP4,         //   ... ping-pong loop, ring 4
    YV3_PK_192x256_ROLL,        // bf16: 8 waves of 96x64, rolling loop, ring 3
    YV3_PK_192x256_PP3,         //   ... ping-pong loop, ring 3
    YV3_PK_192x256_PP4,         //   ... ping-pong loop, ring 4
    YV3_PK_W4_192x128,          // conv_planes_w4.hip (a kernel with one main loop of its own: the loop kind says plain, as for the next three)
    YV3_PK_K3S1_256x128,        // conv_planes_k3s1.hip launch_k3s1<NP, 256, 128, 4, 2>
    YV3_PK_K3S1_128x128,        //   <NP, 128, 128, 4, 2>
    YV3_PK_K3S1_128x64,         //   <NP, 128, 64, 2, 2>
    YV3_PK_WINO_PINGPONG,       // Winograd F(2x2) stage, one 128x128 tile per workgroup: the tune bit's two main loops
    YV3_PK_WINO_ROLL,
    YV3_PK_WINO_EVEN,           //   ... stream-K over transform positions (YV3_OPT_WINO_EVEN): ping-pong loop, one persistent workgroup per CU
};
const char* yv3_planes_kernel_name(yv3_planes_kernel k);        // the enumerator without YV3_PK_
// main loop of conv_planes_kernel (its PP / ROLL template arguments)
enum yv3_planes_loop {
    YV3_LOOP_PLAIN,             // single phase, one barrier pair per chunk
    YV3_LOOP_ROLLING,           // single phase, next chunk's first fragments read under the MFMAs
    YV3_LOOP_PINGPONG,          // two four-wave groups: one reads fragments while the other issues MFMAs (eight-wave tiles, ring >= 3, <= 2 planes)
};
const char* yv3_planes_loop_name(yv3_planes_loop l);
struct yv3_planes_choice {
    int rc;                     // the YV3_E* code yv3_conv2d returns before anything is launched, or 0
    int form, launches;
    yv3_planes_kernel kernel;
    int Ho, Wo, M;
    int ntiles;                 // channel tiles of the launch
    yv3_planes_loop loop;       // the main loop that runs
    bool stream_k;              // YV3_PK_256x128_W8 / _128x128_W8 on fp16 planes, ping-pong loop: the persistent stream-K schedule (yv3_conv_desc.workspace)
    int grid;                   // workgroups of a persistent launch (stream_k, YV3_PK_WINO_EVEN: one per CU), else 0: one per tile
};

enum yv3_f32_kernel {
    YV3_FK_NONE,
    // conv_igemm_f32.hip launch<BM, BN, WM, WN>
    YV3_FK_128x128_W8, YV3_FK_128x128_W4, YV3_FK_64x64, YV3_FK_128x64, YV3_FK_128x32,
    YV3_FK_WINO2,               // F(2x2) stage: 128x128 on eight waves, or (half) 64x128 on four
    YV3_FK_WINO4,               // conv_wino4_f32.hip (even schedule iff parts > 1)
    // conv_gemm_f32.hip conv_gemm1x1_f32_kernel<WM, WN, K3>
    YV3_FK_GEMM_128x128, YV3_FK_GEMM_256x64, YV3_FK_GEMM_K3,
};
const char* yv3_f32_kernel_name(yv3_f32_kernel k);              // the enumerator without YV3_FK_
struct yv3_f32_choice {
    int rc;                     // the YV3_E* code yv3_conv2d returns before anything is launched, or 0
    int form, launches;
    yv3_f32_kernel kernel;
    int Ho, Wo, M;
    int ntiles;                 // channel tiles of the direct / F(2x2) launch
    bool pin;                   // !YV3_OPT_TWO_LANES: the direct and F(2x2) kernels' PIN instantiations (conv_igemm_f32.hip)
    bool wino2_half;            // F(2x2): the four-wave 64x128 tile
    int n_full, parts;          // F(4x4): whole-item workgroups, ranges per item of the rest (1: one item per workgroup throughout)
    int gemm_rows;              // persistent GEMM: the output pixels [0, gemm_rows) it takes ...
    int gemm_grid;              //   ... on this many workgroups (one per CU; a multiple of 8 when there are fewer tiles) ...
    yv3_f32_kernel rest;        //   ... and the direct kernel for the others (YV3_FK_NONE: none left)
    int rest_ntiles;
};

// Ho, Wo and M = B * Ho * Wo of a descriptor that passed yv3_conv2d's argument checks
struct yv3_conv_shape { int Ho, Wo; long long M; };
yv3_conv_shape yv3_conv_out_shape(const yv3_conv_desc* d);

yv3_planes_choice yv3_select_planes(const yv3_conv_desc* d, int np, int ncu);     // np = planes per tensor: 1 bf16 (or fp16: YV3_F16 takes YV3_BF16's choice), 2 fp16 hi+lo, 3 bf16 x3
// YV3_I8: the shape checks of the int8 kernels, then the one-bf16-plane choice for the layer's BYTES (an int8 layer of C input channels stages
// the rows of a bf16 layer of C/2) without the forms and kernels that have no int8 instantiation
yv3_planes_choice yv3_select_planes_i8(const yv3_conv_desc* d, int ncu);
yv3_f32_choice yv3_select_f32(const yv3_conv_desc* d, int ncu);

// One line (at most YV3_KERNEL_LINE_BYTES with its NUL) that holds every field of a choice that is not a function of the descriptor alone
// (those at their default left out): what yv3_conv2d_kernel writes.  Returns 0, or YV3_EINVAL when it does not fit into buf_bytes.
constexpr size_t YV3_KERNEL_LINE_BYTES = 96;
int yv3_describe_planes(const yv3_planes_choice& c, char* buf, size_t buf_bytes);
int yv3_describe_f32(const yv3_f32_choice& c, char* buf, size_t buf_bytes);
