// The convolution configuration ids of y5_conv2d_fwd (include/yolov5_hip.h: y5_conv_desc::cfg), host side only: ONE row per public id, holding the id and
// every template argument its launcher needs.  The launchers (conv.hip, convh3.hip, convg8.hip), y5_conv_cfg_info and the validation in conv2d_fwd_impl all
// read these tables; kCfgIndex maps an id to {family, row} and is checked at compile time to claim every id exactly once.
// To add a configuration: (1) raise Y5_CONV_NUM_CFGS and describe the id in include/yolov5_hip.h, (2) add its row to the family's table below, (3) pin its
// tile in tests/test_emu_conv_cfgs.py.  A new family also needs an entry in Y5ConvFam / y5_build_cfg_index, a `case` in y5_conv_cfg_info and conv2d_fwd_impl.
#pragma once
#include <stddef.h>

#include <type_traits>
#include <utility>

#include "../../include/yolov5_hip.h"
#include "y5_host.h"

enum Y5ConvFam : unsigned char { kFamIgemm, kFamUp, kFamPw, kFamK3, kFamH3, kFamPwk, kFamG8, kNumFam };

// ids other entry points name
constexpr int kCfgFp16Only0 = 22;    // "configurations 22 and above are fp16 only"
constexpr int kCfgK3s2 = 31;         // y5_conv_k3pw_fwd: the 3x3 s2 32->64 streaming configurations, two stages ...
constexpr int kCfgK3s2Default = 34;  // ... three stages (its default; maps to the two-stage kernel there) ...
constexpr int kCfgK3s2W8 = 81;       // ... and eight waves with one stage each
constexpr int kCfgPwHeadW8 = 87;     // y5_detect_head_fwd: the eight-wave form of id 56
constexpr int kCfgUpDefault = 89;    // cfg < 0 on a layer with up_c > 0

// ---- general implicit GEMM (conv_igemm.h): workgroup tile BM = wm*tm*32 pixels x BN = wn*tn*32 channels, LDS row bytes rb (K per stage = rb / elemsize),
// ns ring stages; prod / alias / sk = the PROD / ALIAS / SK template switches
struct IgemmCfg { int id, wm, wn, tm, tn, rb, ns; bool prod, alias, sk; };
constexpr IgemmCfg kIgemmCfgs[] = {
    // (fp32 is built for these four rows only: kNumIgemmF32)
    {0, 4, 1, 1, 1, 64, 2},    // 128 x  32, BK32
    {1, 4, 1, 1, 2, 64, 2},    // 128 x  64, BK32
    {2, 2, 2, 2, 2, 64, 2},    // 128 x 128, BK32
    {3, 2, 2, 2, 4, 64, 2},    // 128 x 256, BK32
    {4, 4, 1, 2, 1, 64, 2},    // 256 x  32, BK32
    {5, 4, 1, 2, 2, 64, 2},    // 256 x  64, BK32
    {6, 4, 1, 1, 1, 128, 2},   // 128 x  32, BK64
    {7, 4, 1, 1, 2, 128, 2},   // 128 x  64, BK64
    {8, 2, 2, 2, 2, 128, 2},   // 128 x 128, BK64
    {9, 2, 2, 2, 4, 128, 2},   // 128 x 256, BK64
    {10, 4, 1, 2, 2, 128, 2},  // 256 x  64, BK64
    {11, 2, 2, 1, 2, 128, 2},  //  64 x 128, BK64
    {12, 2, 2, 4, 2, 128, 2},  // 256 x 128, BK64
    {13, 4, 1, 2, 1, 128, 2},  // 256 x  32, BK64
    // 3-stage LDS ring (counted vmcnt, one raw barrier per chunk): the tile shapes of ids {1, 2, 3, 5, 7, 8, 11, 12}
    {22, 4, 1, 1, 2, 64, 3},
    {23, 2, 2, 2, 2, 64, 3},
    {24, 2, 2, 2, 4, 64, 3},
    {25, 4, 1, 2, 2, 64, 3},
    {26, 4, 1, 1, 2, 128, 3},
    {27, 2, 2, 2, 2, 128, 3},
    {28, 2, 2, 1, 2, 128, 3},
    {29, 2, 2, 4, 2, 128, 3},
    // large tiles for the deep layers (K >= 576, N >= 128).  The general mainloop is bound by the L2->LDS bytes in flight per CU, so these trade occupancy
    // for bytes per flop: 256-row tiles, BK32 chunks, deeper rings, 8 waves where the tile is 256 wide
    {35, 2, 2, 4, 2, 64, 4},   // 256 x 128, BK32, 4 stages, 4 waves
    {36, 4, 2, 2, 2, 64, 4},   // 256 x 128, BK32, 4 stages, 8 waves
    {37, 2, 4, 4, 2, 64, 4},   // 256 x 256, BK32, 4 stages, 8 waves
    {38, 2, 4, 4, 2, 64, 3},   // 256 x 256, BK32, 3 stages, 8 waves
    {39, 2, 4, 4, 2, 128, 2},  // 256 x 256, BK64, 2 stages, 8 waves
    // producer / consumer (conv_igemm.h PROD): as many LDS-DMA waves again as MFMA waves
    {40, 2, 2, 4, 2, 128, 3, true},  // 256 x 128, BK64, 3 stages, 4 + 4 waves
    {41, 2, 2, 4, 2, 64, 4, true},   // 256 x 128, BK32, 4 stages, 4 + 4 waves
    {42, 2, 2, 2, 2, 128, 3, true},  // 128 x 128, BK64, 3 stages, 4 + 4 waves
    {43, 2, 2, 2, 2, 64, 4, true},   // 128 x 128, BK32, 4 stages, 4 + 4 waves
    {44, 2, 2, 2, 4, 64, 4, true},   // 128 x 256, BK32, 4 stages, 4 + 4 waves
    {45, 4, 1, 1, 2, 128, 3, true},  // 128 x  64, BK64, 3 stages, 4 + 4 waves
    // high-occupancy 2-stage variants (conv_igemm.h ALIAS): epilogue scratch inside the idle ring stage
    {46, 2, 2, 2, 2, 64, 2, false, true},   // 128 x 128, BK32 (32 KB LDS, 4 workgroups per CU)
    {47, 4, 1, 1, 2, 64, 2, false, true},   // 128 x  64, BK32 (24 KB LDS)
    {48, 4, 1, 1, 2, 128, 2, false, true},  // 128 x  64, BK64 (48 KB LDS, 3 workgroups per CU)
    {49, 2, 2, 1, 2, 128, 2, false, true},  //  64 x 128, BK64 (48 KB LDS)
    // tile widths for the channel counts of yolov5m (multiples of 96) and yolov5x (multiples of 160): no padded filter rows
    {50, 2, 2, 2, 5, 64, 2},   // 128 x 320, BK32
    {51, 4, 1, 1, 5, 128, 2},  // 128 x 160, BK64
    {52, 2, 2, 2, 3, 64, 2},   // 128 x 192, BK32
    {53, 4, 1, 1, 3, 128, 2},  // 128 x  96, BK64
    {54, 4, 2, 2, 5, 64, 2},   // 256 x 320, BK32, 8 waves
    {55, 4, 2, 2, 3, 64, 2},   // 256 x 192, BK32, 8 waves
    // stream-K (conv_igemm.h SK): BK64, 2 stages
    {57, 2, 2, 2, 2, 128, 2, false, false, true},  // 128 x 128
    {58, 2, 4, 4, 2, 128, 2, false, false, true},  // 256 x 256, 8 waves
    {59, 2, 2, 4, 2, 128, 2, false, false, true},  // 256 x 128
    {60, 2, 2, 2, 4, 128, 2, false, false, true},  // 128 x 256
};
constexpr size_t kNumIgemmF32 = 4;
// the same kernel with the loader that reads `nn.Upsample(2) + Concat` virtually (conv_igemm.h UP2; 1x1 s1 fp16 layers with d->up_c > 0 ONLY, never the
// gather table): 88 = the producer / consumer ring of id 43, 89 = the plain 2-stage tile of id 8
constexpr IgemmCfg kUpCfgs[] = {
    {88, 2, 2, 2, 2, 64, 4, true},
    {89, 2, 2, 2, 2, 128, 2},
};

// ---- streaming pointwise (conv_pw.h): kc x rb / 2 input channels -> nt * 32 output channels, s ring stages per wave, epilogue in os channel groups,
// nwv waves per workgroup (32 pixels each)
struct PwCfg { int id, kc, rb, nt, s, os, nwv; };
constexpr PwCfg kPwCfgs[] = {
    {14, 1, 64, 1, 4, 1, 4},   //  32 ->  32, 4 stages
    {15, 1, 128, 1, 4, 1, 4},  //  64 ->  32
    {16, 1, 128, 2, 4, 1, 4},  //  64 ->  64
    {17, 1, 128, 2, 3, 1, 4},  //  64 ->  64, 3 stages
    {18, 2, 128, 2, 3, 1, 4},  // 128 ->  64
    {19, 2, 128, 4, 3, 1, 4},  // 128 -> 128
    {20, 2, 128, 4, 2, 1, 4},  // 128 -> 128, 2 stages
    {21, 2, 128, 2, 4, 1, 4},  // 128 ->  64, 4 stages
    {56, 2, 128, 8, 2, 2, 4},  // 128 -> 256 (the P3 Detect head), epilogue in two channel groups
    {84, 2, 128, 4, 1, 1, 8},  // 128 -> 128, eight waves, one stage per wave
    {85, 1, 128, 2, 1, 1, 8},  //  64 ->  64, eight waves
    {86, 2, 128, 2, 1, 1, 8},  // 128 ->  64, eight waves
    {87, 2, 128, 8, 1, 2, 8},  // 128 -> 256, eight waves, epilogue in two channel groups
};

// ---- streaming 3x3 (conv_k3.h): c1 -> nt * 32 channels at stride sh, s ring stages per wave, wreg = filter fragments in registers, nwv waves
struct K3Cfg { int id, c1, nt, sh, s; bool wreg; int nwv; };
constexpr K3Cfg kK3Cfgs[] = {
    {30, 32, 1, 1, 3, false, 4},  // 3x3 s1 32->32, 3 stages   (Bottleneck.cv2 @160)
    {31, 32, 2, 2, 2, false, 4},  // 3x3 s2 32->64, 2 stages   (Conv 1 @320->160)
    {32, 64, 2, 1, 2, false, 4},  // 3x3 s1 64->64, 2 stages   (Bottleneck.cv2 @80)
    {33, 32, 1, 1, 2, false, 4},  // 3x3 s1 32->32, 2 stages
    {34, 32, 2, 2, 3, false, 4},  // 3x3 s2 32->64, 3 stages
    {78, 64, 2, 1, 3, true, 4},   // 3x3 s1 64->64, filter fragments in registers, 3 stages
    {79, 64, 2, 1, 4, true, 4},   // the same, 4 stages
    {80, 64, 2, 1, 1, false, 8},  // 3x3 s1 64->64, EIGHT waves with one stage each (two waves per SIMD under one LDS filter copy)
    {81, 32, 2, 2, 1, false, 8},  // 3x3 s2 32->64, eight waves, one stage
    {82, 32, 1, 1, 1, false, 8},  // 3x3 s1 32->32, eight waves, one stage
    {83, 32, 1, 1, 2, false, 8},  // 3x3 s1 32->32, eight waves, two stages
};

// ---- halo-resident 3x3 (conv_h3.h): wm x wn waves of tm x tn 32 x 32 fragments, at most hpmax staged halo pixels, nsw filter ring stages
struct H3Cfg { int id, wm, wn, tm, tn, hpmax, nsw; };
constexpr H3Cfg kH3Cfgs[] = {
    {61, 2, 2, 5, 2, 496, 9},  // 320 pixels x 128 channels (8 x 40, 4 x 80, 16 x 20 output tiles)
    {62, 2, 2, 5, 1, 496, 9},  // 320 x  64
    {63, 2, 2, 7, 2, 512, 9},  // 448 x 128 (10 x 40: four tiles per 40 x 40 image; 20 x 20 whole images)
    {64, 2, 2, 4, 2, 400, 9},  // 256 x 128 (5 x 40, 10 x 20)
    {65, 2, 2, 7, 1, 512, 9},  // 448 x  64
    {66, 2, 2, 4, 1, 400, 9},  // 256 x  64
    // eight waves (two per SIMD: one wave's LDS latency and DMA issue hide behind the other's MFMAs)
    {67, 2, 4, 5, 1, 496, 9},  // 320 x 128
    {68, 2, 4, 7, 1, 512, 9},  // 448 x 128
    {69, 2, 4, 4, 1, 400, 9},  // 256 x 128
    {70, 4, 2, 2, 2, 400, 9},  // 256 x 128, waves 4 x 2
    // 128 x 128 (four waves) / 128 x 64 (eight waves) register tiles per wave: 2 MFMAs per fragment read
    {71, 4, 1, 4, 4, 512, 9},  // 512 x 128
    {72, 4, 2, 4, 2, 512, 9},  // 512 x 128, eight waves
    // 4-stage filter ring: two workgroups per CU (independent barriers: one's LDS-DMA issue and epilogue overlap the other's MFMAs)
    {73, 2, 2, 4, 2, 320, 4},  // 256 x 128 (5 x 40, 10 x 20)
    {74, 2, 2, 4, 1, 320, 4},  // 256 x  64
    {75, 2, 2, 3, 2, 320, 4},  // 192 x 128
    {76, 4, 2, 2, 2, 320, 4},  // 256 x 128, eight waves, two workgroups per CU
    {77, 4, 2, 2, 1, 320, 4},  // 256 x  64, eight waves, two workgroups per CU
    // small pixel tiles for the STRIDE-2 layers, whose halo is ~4.6x the output tile (4 x 16 outputs <- 9 x 33 inputs)
    {90, 2, 2, 1, 2, 320, 4},  //  64 x 128, four waves, 4-stage ring: two workgroups per CU
    {91, 4, 2, 1, 2, 592, 4},  // 128 x 128, eight waves, 4-stage ring (8 x 16 outputs <- 17 x 33 inputs)
    {92, 2, 2, 2, 2, 592, 4},  // 128 x 128, four waves, 4-stage ring
};

// ---- K-streamed pointwise (conv_pwk.h): ns ring stages, 256 pixels x nt * 32 channels
struct PwkCfg { int id, ns, nt; };
constexpr PwkCfg kPwkCfgs[] = {{93, 4, 8}, {94, 4, 4}};

// ---- 256-row / 8-phase implicit GEMM (conv_g8.h): 256 pixels x bn channels, K tile 64 (the two rows are two kernels: Y5G8Geom, Y5G8nGeom)
struct G8Cfg { int id, bn; };
constexpr G8Cfg kG8Cfgs[] = {{95, 256}, {96, 128}};

template <typename Row, size_t N>
constexpr size_t y5_num_rows(const Row (&)[N]) { return N; }

// ---- id -> {family, row of the family's table} -------------------------------------------------------------------------------------------
struct CfgRef { unsigned char fam, row; };
struct CfgIndex {
  CfgRef at[Y5_CONV_NUM_CFGS];
  int claims[Y5_CONV_NUM_CFGS];
  int stray;   // rows whose id lies outside 0 .. Y5_CONV_NUM_CFGS - 1
  constexpr CfgRef operator[](int id) const { return at[id]; }
};
template <typename Row, size_t N>
constexpr void y5_claim_ids(CfgIndex& ix, const Row (&rows)[N], Y5ConvFam fam) {
  for (size_t r = 0; r < N; ++r) {
    const int id = rows[r].id;
    if (id < 0 || id >= Y5_CONV_NUM_CFGS) { ++ix.stray; continue; }
    ix.at[id] = CfgRef{(unsigned char)fam, (unsigned char)r};
    ++ix.claims[id];
  }
}
constexpr CfgIndex y5_build_cfg_index() {
  CfgIndex ix{};
  y5_claim_ids(ix, kIgemmCfgs, kFamIgemm);
  y5_claim_ids(ix, kUpCfgs, kFamUp);
  y5_claim_ids(ix, kPwCfgs, kFamPw);
  y5_claim_ids(ix, kK3Cfgs, kFamK3);
  y5_claim_ids(ix, kH3Cfgs, kFamH3);
  y5_claim_ids(ix, kPwkCfgs, kFamPwk);
  y5_claim_ids(ix, kG8Cfgs, kFamG8);
  return ix;
}
constexpr CfgIndex kCfgIndex = y5_build_cfg_index();
constexpr bool y5_cfg_index_complete(const CfgIndex& ix) {
  for (int id = 0; id < Y5_CONV_NUM_CFGS; ++id)
    if (ix.claims[id] != 1) return false;
  return ix.stray == 0;
}
static_assert(y5_cfg_index_complete(kCfgIndex), "every configuration id 0 .. Y5_CONV_NUM_CFGS - 1 must be claimed by exactly one table row");
static_assert(kIgemmCfgs[kNumIgemmF32 - 1].id == (int)kNumIgemmF32 - 1 && kIgemmCfgs[0].id == 0, "the fp32 rows are ids 0 .. kNumIgemmF32 - 1");

constexpr const K3Cfg& y5_k3_cfg(int id) { return kK3Cfgs[kCfgIndex[id].row]; }

// ---- compile-time walk over a family's rows: calls f(std::integral_constant<size_t, I>) for I == row, which instantiates one launcher per row;
// a row outside I... is refused with `unknown`
template <typename F, size_t... I>
int y5_launch_row(int row, const char* unknown, F&& f, std::index_sequence<I...>) {
  int rc = 0;
  const bool found = ((row == (int)I && (rc = f(std::integral_constant<size_t, I>{}), true)) || ...);
  return found ? rc : y5_fail(Y5_ERR_BAD_ARG, unknown);
}
