// LDS-DMA implicit-GEMM conv, host side: the family's knobs (the only place it reads the environment), plan = knobs +
// CU count + policy (conv_dma_plan.h), the dispatch of a plan over (dtype, A mode, epilogue) to the instantiation units
// conv_dma_*.hip, the split-K reduction and the tuning override. The kernels live in conv_dma_impl.h (design notes there).
#include "conv_dma_impl.h"

namespace dv {

// Tuning override (tools/tune_dma.py): force tile config `g_cfg` (> 0) and split-K factor
// `g_ks` (> 0) for every DMA conv launch until reset to 0. Host-side globals, set between launches.
int g_cfg = 0, g_ks = 0;
__thread ConvRoute g_route = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // route report (kernels.h)
void conv_dma_tune(int cfg, int ks) {
  g_cfg = cfg;
  g_ks = ks;
}

// Every switch of the family. The dispatch A/B switches are read per launch and only under DV_ABLATIONS=1
// (a serving process keeps its dispatch whatever its environment holds); the tile / split-K thresholds are
// latched at the first plan. DV_NO_KW3_SK is a production switch (ops/conv.py names it as the recovery
// from a stream-K hand-off timeout), read per launch.
static DmaKnobs dma_knobs() {
  static const bool no_auto_cfg = dv_ab_env("DV_NO_AUTO_CFG") != nullptr;  // A/B: the size-based choice only
  static const int kmin = dv_ab_env("DV_SMALL_TILE_KMIN") ? std::atoi(dv_ab_env("DV_SMALL_TILE_KMIN")) : 0;
  static const bool no_splitk = dv_ab_env("DV_NO_SPLITK") != nullptr;
  static const bool no_small_splitk = dv_ab_env("DV_NO_SMALL_SPLITK") != nullptr;
  static const long long mn = dv_ab_env("DV_SMALL_SPLITK_MN") ? std::atoll(dv_ab_env("DV_SMALL_SPLITK_MN")) : 300000LL;
  DmaKnobs k;
  k.no_auto_cfg = no_auto_cfg; k.small_tile_kmin = kmin; k.no_splitk = no_splitk; k.no_small_splitk = no_small_splitk;
  k.small_splitk_mn = mn; k.cfg = g_cfg; k.ks = g_ks;
  k.no_kw3_sk = std::getenv("DV_NO_KW3_SK") != nullptr;
  if (!dv_ablations_on()) return k;
  auto is = [](const char* e, const char* v) { return e != nullptr && std::strcmp(e, v) == 0; };
  if (const char* e = dv_ab_env("DV_KW3")) k.kw3 = std::atoi(e);
  if (const char* e = dv_ab_env("DV_KW3_VAR")) k.kw3_var = std::atoi(e);
  if (const int v = k.kw3_var; v == 8 || v == 9 || v == 10 || v == 20 || v == 21) {
    // timing ablations with wrong outputs: a stray DV_KW3_VAR in a serving process cannot corrupt convs
    const bool allow = dv_ab_env("DV_ALLOW_WRONG_ABLATION") != nullptr;
    static bool warned = false;
    if (!warned)
      fprintf(stderr, allow ? "deconv_api_amd: DV_KW3_VAR=%d: timing ablation, outputs are WRONG\n"
                            : "deconv_api_amd: DV_KW3_VAR=%d ignored (needs DV_ALLOW_WRONG_ABLATION=1)\n", v);
    warned = true;
    if (!allow) k.kw3_var = kKw3DefaultVar;
  }
  k.kw3_tile_512 = is(dv_ab_env("DV_KW3_TILE"), "512x128");
  k.kw3_sk_all = is(dv_ab_env("DV_KW3_SK"), "all");
  k.kw3p_epi_reg = is(dv_ab_env("DV_KW3P_EPI"), "reg");
  k.kw3p_unp_nt = !is(dv_ab_env("DV_KW3P_UNP_NT"), "0");
  k.no_kw3p_unpool = dv_ab_env("DV_NO_KW3P_UNPOOL") != nullptr;
  k.kw3p_no_pre = dv_ab_env("DV_KW3P_NO_PRE") != nullptr;
  return k;
}

DmaPlan conv_dma_plan(const ConvArgs& a, int amode, int epi) { return dma_plan(a, amode, epi, device_cus(), dma_knobs()); }

// The split-K epilogue: out = act(sum_s ws[s] + bias) with the kernel epilogue's full semantics
// (16-bit or fp32 output of row stride out_ld): v = sum + bias, [ReLU] (before an accumulate /
// residual add), += out (accumulate), += res then [ReLU], zeroed where emask <= 0.
template <int DT>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const ConvArgs a, int epi) {
  const long long total = (long long)a.M * a.OC;
  const long long plane = (long long)a.M * a.OCpad;
  for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int row = (int)(t / a.OC), col = (int)(t % a.OC);
    const float* w = a.ws + (long long)row * a.OCpad + col;
    float v = a.bias ? a.bias[col] : 0.f;
    for (int k = 0; k < a.ksplit; ++k) v += w[k * plane];
    if (relu_at(a, col) && !a.res) v = fmaxf(v, 0.f);
    const long long o = (long long)row * a.out_ld + col;
    if (!DV_BOUNDS(o, 1, a.out_elems, "splitk_reduce out")) continue;
    if (epi == CONV_E_F32) {
      float* out = reinterpret_cast<float*>(a.out);
      if (a.accumulate) v += out[o];
      out[o] = v;
      continue;
    }
    uint16_t* out = reinterpret_cast<uint16_t*>(a.out);
    if (a.accumulate) v += to_f<DT>(out[o]);
    if (a.res) {
      v += to_f<DT>(a.res[(long long)row * a.res_ld + col]);
      if (relu_at(a, col)) v = fmaxf(v, 0.f);
    }
    if (a.emask) {
      const uint32_t m = a.emask[(long long)row * a.emask_ld + col];
      if (m == 0u || (m & 0x8000u)) v = 0.f;
    }
    out[o] = from_f<DT>(v);
  }
}

int splitk_reduce_launch(const ConvArgs& a, int epi, hipStream_t s) {
  const long long total = (long long)a.M * a.OC;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 256LL * 16);
  if (a.dtype == DT_F16)
    hipLaunchKernelGGL(splitk_reduce_kernel<DT_F16>, dim3(grid), dim3(256), 0, s, a, epi);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel<DT_BF16>, dim3(grid), dim3(256), 0, s, a, epi);
  return (int)hipGetLastError();
}

int conv_dma_run(const ConvArgs& a, const DmaPlan& p, hipStream_t s) {
  if (p.status != 0) return p.status;
  const bool f16 = a.dtype == DT_F16, fwd = p.amode == CONV_A_FWD;
  const int rc = [&] {  // the instantiation units; fp16: DeepDream (BASELINE config 5) and the fp16 deconvnet
    if (p.mask)
      return fwd ? (f16 ? dma_run_mask<DT_F16, CONV_A_FWD>(a, p, s) : dma_run_mask<DT_BF16, CONV_A_FWD>(a, p, s))
                 : (f16 ? dma_run_mask<DT_F16, CONV_A_TRANSPOSE>(a, p, s) : dma_run_mask<DT_BF16, CONV_A_TRANSPOSE>(a, p, s));
    if (!fwd) return f16 ? dma_run_f16_tr(a, p, s) : dma_run_bf16_tr(a, p, s);
    if (p.epi == CONV_E_BF16) return f16 ? dma_run_f16_fwd(a, p, s) : dma_run_bf16_fwd(a, p, s);
    if (p.epi == CONV_E_POOL) return f16 ? dma_run_f16_fwd_pool(a, p, s) : dma_run_bf16_fwd_pool(a, p, s);
    return f16 ? dma_run_f16_fwd_f32(a, p, s) : dma_run_bf16_fwd_f32(a, p, s);
  }();
  if (rc < 0) return rc;  // refused: nothing ran, no route reported
  const int pre = g_route.flags & (CR_F_UNPOOL | CR_F_RELU_COPY);  // the pre-pass flags bindings.cpp set stay
  g_route = plan_route(p);
  g_route.flags |= pre;
  return rc;
}

}  // namespace dv
