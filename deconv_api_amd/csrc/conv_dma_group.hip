// Grouped LDS-DMA conv launches (conv_dma_impl.h: conv_dma_group_kernel): several independent
// problems with one tile config in one grid. The small-map InceptionV3 convs of DeepDream's early
// octaves are latency bound (~10 us per dependent launch whatever their size, docs/KERNELS.md), so
// the independent branch convs of a block run as ONE launch (ops/inception.py plans the levels).
#include "conv_dma_impl.h"

namespace dv {

namespace {

// the problems of one group on tile ID of the table (conv_dma_plan.h kDmaTiles)
template <int DT, int AMODE, int ID>
int group_run(const ConvArgs* ps, int n, hipStream_t s) {
  constexpr DmaTile T = kDmaTiles[ID];
  constexpr int BM = T.bm(), BN = T.bn();
  ConvGroup g{};
  g.n = n;
  long long tot = 0;
  bool aligned = true;
  for (int i = 0; i < n; ++i) {
    g.p[i] = ps[i];
    g.tiles_n[i] = ps[i].OCpad / BN;
    g.start[i] = (int)tot;
    tot += (long long)((ps[i].M + BM - 1) / BM) * g.tiles_n[i];
    aligned = aligned && (ps[i].C % T.BK) == 0;
  }
  for (int i = n; i <= kGroupMax; ++i) g.start[i] = (int)tot;
  if (tot <= 0 || tot > 0x7fffffffLL) return -2;
  if (aligned)
    hipLaunchKernelGGL((conv_dma_group_kernel<DT, T.WM, T.WN, T.FM, T.FN, T.BK, T.ST, AMODE, CONV_E_BF16, true>),
                       dim3((unsigned)tot), dim3(T.WM * T.WN * 64), 0, s, g);
  else
    hipLaunchKernelGGL((conv_dma_group_kernel<DT, T.WM, T.WN, T.FM, T.FN, T.BK, T.ST, AMODE, CONV_E_BF16, false>),
                       dim3((unsigned)tot), dim3(T.WM * T.WN * 64), 0, s, g);
  return (int)hipGetLastError();
}

// the measured small-problem configs (conv_dma_plan.h auto_cfg): 64x64 / 4 waves / 3 stages, 128x128 / 8 waves / 2 stages
template <int DT, int AMODE>
int group_cfg_run(const ConvArgs* ps, int n, int cfg, hipStream_t s) {
  return cfg == 8 ? group_run<DT, AMODE, 8>(ps, n, s) : (cfg == 3 ? group_run<DT, AMODE, 3>(ps, n, s) : -5);
}

}  // namespace

int conv_dma_group_launch(const ConvArgs* ps, int n, int amode, int epi, hipStream_t s) {
  if (n < 1 || n > kGroupMax || epi != CONV_E_BF16) return -4;
  const int cfg = conv_dma_plan(ps[0], amode, epi).group_cfg;
  if (cfg == 0) return -4;
  for (int i = 1; i < n; ++i)
    if (conv_dma_plan(ps[i], amode, epi).group_cfg != cfg || ps[i].dtype != ps[0].dtype) return -4;
  const bool f16 = ps[0].dtype == DT_F16;
  if (amode == CONV_A_FWD)
    return f16 ? group_cfg_run<DT_F16, CONV_A_FWD>(ps, n, cfg, s) : group_cfg_run<DT_BF16, CONV_A_FWD>(ps, n, cfg, s);
  return f16 ? group_cfg_run<DT_F16, CONV_A_TRANSPOSE>(ps, n, cfg, s)
             : group_cfg_run<DT_BF16, CONV_A_TRANSPOSE>(ps, n, cfg, s);
}

}  // namespace dv
