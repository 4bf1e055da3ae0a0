// Routing policy of the LDS-DMA conv family (plain DMA tiles, masked tiles, KW3, KW3P, stream-K, the
// full-rounds + tail split, split-K, grouped launches): which kernel, tile, split-K factor, epilogue
// variant and workspace a problem gets. Policy only: host C++ over kernels.h, no HIP calls, no
// environment reads, no globals, no statics, so every rule can be tested on a CPU
// (tests/native/conv_dma_plan_check.cpp). conv_dma.hip supplies the knobs and the CU count
// (conv_dma_plan) and launches a plan (conv_dma_run); conv_dma_impl.h holds the kernels.
#pragma once
#include "kernels.h"

namespace dv {

// Which pooled-max epilogue a tile can take: shared by conv_dma_body / epilogue (the choice) and the planner (the
// route report of that choice), so the report cannot drift from the kernel. LDS ring of a tile in bytes; the
// transposed 8-B stores need 64-row waves; the LDS-staged form also the [BM/4][BN] values + codes in the ring.
constexpr int dma_ring_bytes(int BM, int BN, int BK, int STAGES, bool MASK) {
  return STAGES * ((MASK ? 2 : 1) * BM + BN) * BK * 2;
}
constexpr bool pool_t_fits(int FM) { return FM % 4 == 0; }
constexpr bool pool_lds_fits(int FM, int BM, int BN, int ring_bytes) {
  return pool_t_fits(FM) && BN % 16 == 0 && (BM / 4) * BN * 3 <= ring_bytes;
}

constexpr int kw3_a_i(int bm) { return bm == 256 ? 4 : 5; }  // KW3 A DMA instructions (16 slots each) per wave
constexpr int kKw3Pad = 8;  // zero slots between image rows: a row jump is +9 slots = +1 (mod 8)
constexpr int kKw3DefaultVar = 2;

// Every switch the family reads (conv_dma.hip:dma_knobs fills it from the environment and the tuner).
struct DmaKnobs {
  int kw3 = 1;                    // DV_KW3: 0 no shared-tap kernels, 2 forced for every eligible launch
  int kw3_var = kKw3DefaultVar;   // DV_KW3_VAR: 0 KW3, 2 KW3P, 11 KW3P with nt stores; 8 / 9 / 10 / 20 / 21: timing
                                  //   ablations with WRONG outputs (set only under DV_ALLOW_WRONG_ABLATION)
  bool kw3_tile_512 = false;      // DV_KW3_TILE=512x128: that KW3P tile for the 256-wide shapes too
  bool kw3_sk_all = false;        // DV_KW3_SK=all: stream-K on every eligible grid
  bool no_kw3_sk = false;         // DV_NO_KW3_SK
  bool kw3p_epi_reg = false;      // DV_KW3P_EPI=reg
  bool kw3p_unp_nt = true;        // DV_KW3P_UNP_NT=0 clears it
  bool no_kw3p_unpool = false;    // DV_NO_KW3P_UNPOOL
  bool kw3p_no_pre = false;       // DV_KW3P_NO_PRE
  bool no_auto_cfg = false;       // DV_NO_AUTO_CFG
  int small_tile_kmin = 0;        // DV_SMALL_TILE_KMIN
  bool no_splitk = false;         // DV_NO_SPLITK
  bool no_small_splitk = false;   // DV_NO_SMALL_SPLITK
  long long small_splitk_mn = 300000LL;  // DV_SMALL_SPLITK_MN
  int cfg = 0, ks = 0;            // tuning override (conv_dma_tune): tile id / split-K factor, 0 = automatic
};

// Every tile the DMA kernel is instantiated with, by config id: 1..17 are what the tuner can force
// (tools/tune_dma.py), 18 / 19 the narrow-output tiles, 20..23 the ReLU-masked dgrad tiles (the mask tile
// doubles A's LDS footprint: <= 128 KiB of LDS per workgroup at 2 stages; 16-bit epilogue only).
struct DmaTile {
  int WM, WN, FM, FN, BK, ST;
  bool MASK, FP;  // FP: register double-buffered fragments (+3 % on the big VGG layers)
  constexpr int bm() const { return WM * FM * 16; }
  constexpr int bn() const { return WN * FN * 16; }
};
constexpr DmaTile kDmaTiles[] = {
    {0, 0, 0, 0, 0, 0, false, false},
    {2, 4, 8, 4, 64, 2, false, true},   //  1: 256x256
    {2, 4, 4, 4, 64, 3, false, false},  //  2: 128x256 (the 3-stage ring wins slightly here and on 256x128)
    {4, 2, 2, 4, 64, 2, false, false},  //  3: 128x128
    {4, 2, 4, 4, 64, 3, false, false},  //  4: 256x128
    {8, 1, 2, 4, 64, 2, false, false},  //  5: 256x64
    {8, 1, 4, 4, 64, 2, false, false},  //  6: 512x64
    {4, 1, 2, 4, 64, 3, false, false},  //  7: 128x64, 4 waves
    {2, 2, 2, 2, 64, 3, false, false},  //  8: 64x64, 4 waves
    {2, 2, 4, 4, 64, 2, false, false},  //  9: 128x128, 4 waves
    {2, 2, 2, 4, 64, 3, false, false},  // 10: 64x128, 4 waves
    {4, 1, 4, 4, 64, 2, false, false},  // 11: 256x64, 4 waves
    // deep rings for latency-bound small GEMMs (more K tiles in flight per workgroup)
    {2, 2, 2, 2, 64, 6, false, false},  // 12: 64x64 w4 ST6
    {2, 2, 2, 2, 64, 8, false, false},  // 13: 64x64 w4 ST8
    {4, 1, 2, 4, 64, 6, false, false},  // 14: 128x64 w4 ST6
    {2, 2, 2, 4, 64, 6, false, false},  // 15: 64x128 w4 ST6
    // 8 waves on a 64x64 tile: half the LDS-DMA issues per wave and K tile (the small tiles' K loop
    // is DMA-issue bound: 4 x ~100 cycles per wave per K tile at 4 waves)
    {4, 2, 1, 2, 64, 3, false, false},  // 16: 64x64 w8
    {4, 2, 1, 2, 64, 4, false, false},  // 17: 64x64 w8 ST4
    {8, 1, 2, 1, 64, 2, false, false},  // 18: 256x16
    {8, 1, 4, 1, 64, 2, false, false},  // 19: 512x16
    {2, 4, 4, 4, 64, 2, true, false},   // 20: 128x256 masked
    {4, 2, 2, 4, 64, 2, true, false},   // 21: 128x128 masked
    {8, 1, 2, 4, 64, 2, true, false},   // 22: 256x64 masked
    {8, 1, 2, 1, 64, 2, true, false},   // 23: 256x16 masked
};
constexpr int kDmaTileForcedMax = 17, kDmaTileTail = 3;

enum DmaKernel : int { DK_DMA = 0, DK_KW3, DK_KW3P };

struct DmaPlan {
  int status;         // 0, or: -1 no such (A mode, epilogue), -2 grid size, -3 no tile for OCpad, -4 geometry, -5 forced tile misfit
                      //   (conv_dma_run adds -6: plan.sk without its workspace)
  int amode, epi;     // the launch's A mode and epilogue (ConvAMode / ConvEpi), as passed to the planner
  int kernel;         // DmaKernel
  int tile;           // DK_DMA: id into kDmaTiles
  int bm, bn, stages;
  bool mask;
  int ksplit;         // split-K factor (1 = none): the caller supplies ConvArgs::ws for ksplit planes and reduces
  int pool_epi;       // DK_DMA with the pooled-max epilogue: ConvRouteEpi of the form the kernel takes
  int kw3_epi;        // DK_KW3P: CR_E_REG / CR_E_LDS / CR_E_UNPOOL; DK_KW3: CR_E_NONE
  int kw3_var;        // DK_KW3P: store variant (0 plain, 1 no stores, 2 nt stores, 3 / 4 ablations); DK_KW3: VAR 0 / 8 / 9
  int kw3_pre;        // DK_KW3P: issue the step-1 DMA ahead of the epilogue stores
  bool sk;            // DK_KW3P stream-K: the caller supplies ConvArgs::skw / skflag / skslots >= cus
  int tiles_m_limit;  // KW3 / KW3P: launch only the first row tiles (the full rounds); 0 = all
  int m_base;         //   then a 128 x 128 DMA tail launch (kDmaTileTail) from this row; 0 = no tail
  int group_cfg;      // tile id a grouped launch of this problem would use (8 or 3), 0 = not groupable
  int cus;            // the CU count planned for (KW3P grids are min(tiles, cus); stream-K's is cus)
  bool bpack;         // KW3 / KW3P: B staged from the packed image (ConvArgs::wp)
};

namespace plan_detail {

inline long long tiles(const ConvArgs& a, int BM, int BN) { return (long long)((a.M + BM - 1) / BM) * (a.OCpad / BN); }

// Measured override of the size-based ladder for small and narrow-K problems (the DeepDream nets' 1x1 / 1x7 /
// 5x5 convs and dgrads; tools/tune_dma.py, profiles/tune_dma_c{3,5}.txt, docs/KERNELS.md). Small problems are
// bound by per-K-step latency, not MFMA rate: a 64x64 4-wave tile with a 3-stage ring; mid-size / short-K ones by
// the epilogue and DMA issue of one big tile per CU: 128x128. The big-K VGG16 layers keep the large tiles.
inline int auto_cfg(const ConvArgs& a, const DmaKnobs& k) {
  if (a.mask != nullptr || k.no_auto_cfg) return 0;
  const long long mn = (long long)a.M * a.OCpad;
  // (short K too: M 1600 x N 64 x K 64 4.2 vs 6.0 us for the size-based 256 x 64 tile in a graph,
  // tools/small_conv_latency.py; DV_SMALL_TILE_KMIN=256 restores the round-1 rule)
  if (a.OCpad % 64 == 0 && a.OC > 16 && mn <= 3000000LL && a.Kpad >= k.small_tile_kmin) return 8;
  if (a.OCpad % 128 == 0 && a.OC > 64 && a.Kpad < 4096 && (a.Kpad < 1024 || mn < 50000000LL)) return 3;
  return 0;
}

// The size-based ladder: the largest tile (best MFMA:LDS ratio) unless it leaves CUs idle. A problem with
// fewer big tiles than the chip has CUs (deep layers at small batch, strong-scaled tiles) drops to the next
// smaller tile, which doubles the workgroup count and fits 2 workgroups per CU in LDS. The masked tiles
// are smaller and fixed per width. (The narrowest rung does not test OCpad % 16: dma_plan does.)
inline int ladder_tile(const ConvArgs& a, long long cus) {
  const bool w256 = a.OCpad % 256 == 0 && a.OC > 128, w128 = a.OCpad % 128 == 0 && a.OC > 64,
             w64 = a.OCpad % 64 == 0 && a.OC > 16;
  if (a.mask != nullptr) return w256 ? 20 : (w128 ? 21 : (w64 ? 22 : 23));
  if (w256) return tiles(a, 256, 256) >= cus ? 1 : (tiles(a, 128, 256) >= cus ? 2 : 3);
  if (w128) return tiles(a, 256, 128) < cus ? 3 : 4;
  if (w64) return tiles(a, 512, 64) < cus ? 5 : 6;
  return tiles(a, 512, 16) < cus ? 18 : 19;
}

// Split-K factor for a launch that would leave most CUs idle: small M (batch-1 serving, deep layers of
// strong-scaled DeepDream tiles, dense layers) with a long K. 1 = no split. Computed from the automatic non-KW3
// tile, even under a forced config. The small-problem 64x64 tiles (auto_cfg 8: DeepDream's small octaves,
// replayed from hipGraphs) split a long K into 2 / 4 parts: in a graph the extra reduce launch costs ~2 us, each K
// tile of the serial K loop ~0.4 us (tools/small_conv_latency.py: M 1600 x N 160 x K 1440 14.8 -> 11.4 us).
inline int splitk(const ConvArgs& a, int ac, long long cus, const DmaKnobs& k) {
  const int nk = a.Kpad / 64;
  if (k.ks > 0) return k.ks < nk ? k.ks : nk;
  if (k.no_splitk) return 1;
  if (k.cfg == 0 && ac == 8) {
    // only the smallest problems: the reduce pass re-reads ks x M x OCpad fp32 partials, which
    // outweighs the shorter K loop once M x OCpad grows (full-model A/B, docs/KERNELS.md)
    if (k.no_small_splitk || (long long)a.M * a.OCpad > k.small_splitk_mn) return 1;
    return nk >= 20 ? 4 : (nk >= 16 ? 2 : 1);
  }
  const DmaTile t = kDmaTiles[ac == 8 ? 8 : (ac == 3 ? 3 : ladder_tile(a, cus))];
  const long long nwg = tiles(a, t.bm(), t.bn());
  if (nwg * 2 > cus || nk < 8) return 1;
  long long s = (cus + nwg - 1) / nwg;  // about one workgroup per CU
  if (s > nk / 4) s = nk / 4;           // >= 4 K tiles per split keeps the pipeline primed
  if (s > 32) s = 32;
  return s < 2 ? 1 : (int)s;
}

// The set_* functions fill a zero-initialized plan once, when they return 0 (a -4 leaves it untouched).
inline int set_dma(DmaPlan& p, const ConvArgs& a, int id) {
  const DmaTile t = kDmaTiles[id];
  const long long nwg = (long long)((a.M - a.m_base + t.bm() - 1) / t.bm()) * (a.OCpad / t.bn());
  if (nwg <= 0 || nwg > 0x7fffffffLL) return -2;
  p.kernel = DK_DMA; p.tile = id; p.bm = t.bm(); p.bn = t.bn(); p.stages = t.ST; p.mask = t.MASK;
  if (p.epi == CONV_E_POOL) {  // the pooled-max epilogue conv_dma_body takes: the kernel's own conditions
    const bool lds_fits = pool_lds_fits(t.FM, t.bm(), t.bn(), dma_ring_bytes(t.bm(), t.bn(), t.BK, t.ST, t.MASK));
    p.pool_epi = (lds_fits && a.pool_t == 2) ? CR_E_POOL_LDS : ((pool_t_fits(t.FM) && a.pool_t) ? CR_E_POOL_T : CR_E_POOL);
  }
  return 0;
}

// What every KW3P epilogue needs: its stores write exactly the C tile of a 16-bit output without residual,
// mask or accumulate, addressed through 31-bit buffer offsets; `vec`: with 16-B rows (LDS-sliced stores).
inline bool kw3p_ok(const ConvArgs& a, int BM, bool vec) {
  if (a.res != nullptr || a.emask != nullptr || a.accumulate || a.out2 != nullptr || a.OC != a.OCpad || a.H >= 4096 ||
      2LL * a.H * a.W + BM >= (1LL << 19) || a.OC % (vec ? 8 : 4) || a.out_ld % (vec ? 8 : 4))
    return false;
  return a.ucode != nullptr ? a.W >= 8 && a.ucode_div >= 1 : a.out_elems * 2 < 0x7FFFFFF0LL;
}
// KW3P epilogue of a problem (ConvRouteEpi), CR_E_NONE when it has none: the LDS-sliced 16-B stores unless
// DV_KW3P_EPI=reg (A/B) or the rows are not 16-B aligned (9-13 % faster per launch than the register-transposed
// 8-B stores, profiles/kw3_epi_ab_r5.txt), or the LDS-sliced max-unpool-out epilogue (DV_NO_KW3P_UNPOOL=1, A/B).
inline int kw3p_epi(const ConvArgs& a, int BM, const DmaKnobs& k) {
  const bool vec = kw3p_ok(a, BM, true);
  if (a.ucode != nullptr) return vec && !k.no_kw3p_unpool ? CR_E_UNPOOL : CR_E_NONE;
  return vec && !k.kw3p_epi_reg ? CR_E_LDS : (kw3p_ok(a, BM, false) ? CR_E_REG : CR_E_NONE);
}

// KW3P stream-K applies: a plain or unpool-out 16-bit forward launch with 16-B rows and no split-K, not
// switched off, one workgroup per CU with the column groups dividing the grid, more tiles than workgroups
// (and more output than one workspace slot per CU), every workgroup's range at least one tile long. Geometry
// only: the caller allocates the workspace when the plan says so. Only short grids (DV_KW3_SK=all: every one):
// it removes a partial last round; on many-round grids it costs 1-3 % (profiles/kw3_sk_ab_r5.txt).
inline bool kw3_sk_ok(const DmaPlan& p, const ConvArgs& a, int BM, int BN, const DmaKnobs& k) {
  if (p.amode != CONV_A_FWD || p.epi != CONV_E_BF16 || p.ksplit > 1 || a.ws != nullptr || a.mask != nullptr ||
      a.m_base != 0 || k.no_kw3_sk || !kw3p_ok(a, BM, true) || (a.dtype != DT_BF16 && a.dtype != DT_F16))
    return false;
  const long long G = p.cus, tiles_n = a.OCpad / BN, tiles_m = (a.M + BM - 1) / BM;
  const long long max_tiles = k.kw3_sk_all ? (1LL << 40) : 4LL * G;
  return G <= kSkMaxWg && (long long)a.M * a.OCpad > G * kSkSlotFloats && (long long)BM * BN <= kSkSlotFloats &&
         tiles_n >= 1 && G % tiles_n == 0 && tiles_m * tiles_n > G && tiles_m * tiles_n < max_tiles &&
         tiles_m >= G / tiles_n && tiles_m * (3LL * a.C / 32) < (1LL << 31);
}

// The shared-kw-tap kernels (3x3 s1 p1 forward: the three kw taps share one staged A tile) on BM x BN
// tiles; limit > 0: only the first `limit` row tiles. -4: not their problem.
inline int set_kw3(DmaPlan& p, const ConvArgs& a, int BM, int BN, int limit, const DmaKnobs& k) {
  if (p.amode != CONV_A_FWD || p.epi == CONV_E_POOL) return -4;
  if (k.kw3 == 0 || a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad_h != 1 || a.pad_w != 1 || a.H != a.OH ||
      a.W != a.OW || a.W < 1 || a.C % 32 || a.mask || p.ksplit > 1 || a.ws || a.OCpad % BN || a.m_base != 0 ||
      (long long)a.Kpad < 9LL * a.C)
    return -4;
  // zero-padded slots of a BM-row tile: BM + 2 + 8 x (image-row boundaries, <= (BM - 1) / W + 1)
  if (BM + 2 + kKw3Pad * ((BM - 1) / a.W + 1) > kw3_a_i(BM) * 8 * 16) return -4;  // W >= 9 (256), >= 35 (512)
  int tiles_m = (a.M + BM - 1) / BM;
  if (limit > 0 && limit < tiles_m) tiles_m = limit;
  const long long nwg = (long long)tiles_m * (a.OCpad / BN);
  if (nwg <= 0 || nwg > 0x7fffffffLL) return -2;
  const int var = k.kw3_var;
  const bool bf = a.dtype == DT_BF16;
  // VAR 10 / 11 / 20 / 21 (bf16 only): KW3P without epilogue stores (timing ablation) / with nt stores / ablations
  const bool abl = bf && (var == 10 || var == 11 || var == 20 || var == 21);
  p.bm = BM; p.bn = BN; p.tiles_m_limit = limit; p.bpack = a.wp != nullptr;
  p.kw3_epi = p.epi == CONV_E_BF16 && (var == 2 || abl) ? kw3p_epi(a, BM, k) : CR_E_NONE;
  if (p.kw3_epi == CR_E_NONE) {
    p.kernel = DK_KW3;
    p.kw3_var = (bf && p.epi == CONV_E_BF16 && (var == 8 || var == 9)) ? var : 0;
    return 0;
  }
  p.kernel = DK_KW3P;
  p.kw3_pre = k.kw3p_no_pre || var >= 20 ? 0 : 1;
  if (abl) {
    p.kw3_var = var == 10 ? 1 : (var == 11 ? 2 : (var == 20 ? 3 : 4));
    return 0;
  }
  p.sk = limit == 0 && kw3_sk_ok(p, a, BM, BN, k);  // the whole grid, no tail launch
  // the unpool-out epilogue's stores are non-temporal (the 4x-upsampled map, 3/4 zeros, streams past the
  // caches): config 2 +0.3 % (3 / 3 pairs, profiles/bench_c2_r5_unp_nt_ab.txt). DV_KW3P_UNP_NT=0: plain stores
  if (p.kw3_epi == CR_E_UNPOOL && k.kw3p_unp_nt && !p.sk) p.kw3_var = 2;
  return 0;
}

// KW3 256 x 256 runs one workgroup per CU (144 KiB of LDS), so a grid of R.f rounds pays a whole
// round for its fraction f (block5 at B*K = 1024: 1568 tiles = 6.125 rounds; at B = 256: 392 =
// 1.53). Split: the full rounds as KW3, the last partial round's rows as a tail launch of 128 x 128
// DMA tiles (4x the workgroups, 2 per CU) starting at row m_base. Same stream, in order.
inline int kw3_split(DmaPlan& p, const ConvArgs& a, const DmaKnobs& k) {
  if (kw3_sk_ok(p, a, 256, 256, k) && k.kw3_var == 2) {  // stream-K: no partial round, no tail launch
    const int rc = set_kw3(p, a, 256, 256, 0, k);
    if (rc != -4) return rc;
  }
  const long long cus = p.cus, tiles_m = (a.M + 255) / 256, tiles_n = a.OCpad / 256;
  const long long full = tiles_m * tiles_n / cus, rem = tiles_m * tiles_n % cus;
  const long long main_m = full * cus / tiles_n;  // row tiles of the full rounds
  if (full < 1 || rem == 0 || (full * cus) % tiles_n != 0 || main_m >= tiles_m) return set_kw3(p, a, 256, 256, 0, k);
  const int rc = set_kw3(p, a, 256, 256, (int)main_m, k);
  if (rc == 0) p.m_base = (int)(main_m * 256);
  return rc;
}

}  // namespace plan_detail

// The plan of one launch on `cus` compute units. Pointer inputs are only tested for null: mask, res, emask,
// ucode, out2, ws, wp. Rules in order: the forced config; DV_KW3=2 ahead of the small-problem tiles (the
// tests' small shapes, K = 9 C < 1024 or few rows, would all take those); the measured small-problem
// tiles (auto_cfg); the size-based ladder, with the shared-tap kernels where they apply.
// Split-K applies to the plain 16-bit and fp32 epilogues only (the reduce kernel applies bias / ReLU /
// accumulate / residual / emask; not the unpool scatter or the column split) and rules out KW3.
inline DmaPlan dma_plan(const ConvArgs& a, int amode, int epi, int cus, const DmaKnobs& k) {
  using namespace plan_detail;
  DmaPlan p{};
  p.amode = amode;
  p.epi = epi;
  p.cus = cus;
  p.ksplit = 1;
  const bool geom_ok = a.C % 8 == 0 && a.Kpad % 64 == 0 && a.x_ld % 8 == 0;
  const int ac = auto_cfg(a, k);
  // grouped launches take the measured small-problem tiles only (large problems keep their own launch
  // and tile choice; masked A, split-K workspaces, tuning overrides)
  if (k.cfg <= 0 && a.mask == nullptr && a.ws == nullptr && epi == CONV_E_BF16 &&
      (amode == CONV_A_FWD || amode == CONV_A_TRANSPOSE) && geom_ok && (ac == 8 || ac == 3))
    p.group_cfg = ac;
  if ((epi == CONV_E_BF16 || epi == CONV_E_F32) && a.ucode == nullptr && a.out2 == nullptr) p.ksplit = splitk(a, ac, cus, k);
  auto done = [&](int rc) { p.status = rc; return p; };
  if (!geom_ok) return done(-4);
  if (a.mask != nullptr) {  // ReLU-masked dgrad: the mask is staged with x's offsets
    if (a.mask_ld != a.x_ld || epi != CONV_E_BF16) return done(-4);
    if (amode != CONV_A_FWD && amode != CONV_A_TRANSPOSE) return done(-1);
    return done(a.OCpad % 16 ? -3 : set_dma(p, a, ladder_tile(a, cus)));
  }
  if (!(amode == CONV_A_FWD && (epi == CONV_E_BF16 || epi == CONV_E_POOL || epi == CONV_E_F32)) &&
      !(amode == CONV_A_TRANSPOSE && epi == CONV_E_BF16))
    return done(-1);
  if (k.cfg > 0)  // -5 = config does not fit this problem
    return done(k.cfg <= kDmaTileForcedMax && a.OCpad % kDmaTiles[k.cfg].bn() == 0 ? set_dma(p, a, k.cfg) : -5);
  const bool w256 = a.OCpad % 256 == 0 && a.OC > 128, w128 = a.OCpad % 128 == 0 && a.OC > 64;
  if (k.kw3 == 2 && (w256 || w128)) {
    const int rc = w256 ? set_kw3(p, a, 256, 256, 0, k) : set_kw3(p, a, 512, 128, 0, k);
    if (rc != -4) return done(rc);
  }
  if (ac) return done(set_dma(p, a, ac));
  const int t = ladder_tile(a, cus);
  if (w256) {
    if (k.kw3_tile_512) {
      const int rc = set_kw3(p, a, 512, 128, 0, k);
      if (rc != -4) return done(rc);
    }
    if (t == 1) {  // a 256 x 256 tile for every CU: the shared-tap kernel, full rounds + tail
      const int rc = kw3_split(p, a, k);
      if (rc != -4) return done(rc);
    }
  } else if (w128 && tiles(a, 512, 128) >= cus) {  // shared-kw-tap 512 x 128 tile
    const int rc = set_kw3(p, a, 512, 128, 0, k);
    if (rc != -4) return done(rc);
  }
  return done(a.OCpad % 16 ? -3 : set_dma(p, a, t));
}

// The route report of a planned launch (kernels.h ConvRoute), the single producer for this family.
inline ConvRoute plan_route(const DmaPlan& p) {
  if (p.kernel == DK_DMA)
    return ConvRoute{CR_DMA, p.bm, p.bn, p.stages, p.ksplit, p.pool_epi, p.mask ? CR_F_MASK : 0, 0, 0, 0};
  return ConvRoute{p.kernel == DK_KW3 ? CR_KW3 : CR_KW3P, p.bm, p.bn, 0, 0, p.kw3_epi,
                   (p.sk ? CR_F_SK : 0) | (p.m_base ? CR_F_TAIL : 0), p.m_base, 0, p.bpack ? 1 : 0};
}

}  // namespace dv
