// Host-visible launcher declarations for the gfx950 kernels.
// Included by the HIP translation units and by bindings.cpp (host-only).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <string>

// Runtime A/B switch of a measured alternative (deconv_api_amd/knobs.py ABLATION): the variable is read
// only when DV_ABLATIONS=1, so a serving / benchmark process takes one dispatch per shape whatever its
// environment holds; tools/*_ab.py and the variant tests set DV_ABLATIONS=1. (Host code only.)
static inline bool dv_ablations_on() {
  const char* on = std::getenv("DV_ABLATIONS");
  return on != nullptr && on[0] == '1' && on[1] == 0;
}
static inline const char* dv_ab_env(const char* name) { return dv_ablations_on() ? std::getenv(name) : nullptr; }

namespace dv {

// A-operand (implicit-GEMM gather) modes of the conv kernel.
enum ConvAMode : int {
  CONV_A_FWD = 0,        // x[n][oh*s-p+kh][ow*s-p+kw][c]
  CONV_A_UNPOOL = 1,     // max-unpool gather: x is pooled (H/2 x W/2), switch codes select
  CONV_A_TRANSPOSE = 2,  // transposed conv (dgrad of a strided conv): ih=(oh+p-kh)/s when divisible
};
// Epilogues.
enum ConvEpi : int {
  CONV_E_BF16 = 0,  // (+bias)(ReLU)(+=out) -> bf16
  CONV_E_POOL = 1,  // (+bias)(ReLU) -> fused 2x2/s2 max-pool, bf16 pooled + uint8 switch code
  CONV_E_F32 = 2,   // (+bias)(ReLU)(+=out) -> fp32
};

// 16-bit storage dtypes (ConvArgs::dtype, pool_launch)
enum { DT_BF16 = 0, DT_F16 = 1 };

struct ConvArgs {
  const uint16_t* x;      // NHWC bf16 input (pooled map in UNPOOL mode, dy in TRANSPOSE mode)
  long long x_ld;         // elements between consecutive pixels of x (>= C; concat slices)
  const uint16_t* mask;   // optional: zero A elements where mask <= 0 (backward through ReLU)
  long long mask_ld;
  const uint8_t* code;    // UNPOOL: switch codes [N/code_div][H/2][W/2][C]
  int code_div;
  const uint16_t* w;      // packed weights [OCpad][Kpad] bf16, K index = (kh*KW+kw)*C + c
  const float* bias;      // [OCpad] fp32 or nullptr
  void* out;              // bf16 or fp32 output, row stride out_ld elements
  long long out_ld;
  uint8_t* out_code;      // POOL: switch codes [M/4][OC]
  int N, H, W, C;         // conv input geometry (UNPOOL: the unpooled H, W)
  int OH, OW, OC, OCpad;
  int KH, KW, stride, pad_h, pad_w;
  int K, Kpad;
  int M;                  // GEMM rows = N*OH*OW
  int m_base;             // LDS-DMA / KW3 launches: first GEMM row of tile 0 (a tail launch after a
                          //   full-round one, conv_dma_plan.h:kw3_split); 0 otherwise
  int relu, relu_in, accumulate;
  int dtype;              // 16-bit storage dtype of x/w/mask/16-bit out: 0 bf16, 1 fp16
  const uint16_t* res;    // optional residual (LDS-DMA FWD, 16-bit out): out = [ReLU](acc + bias + res)
  long long res_ld;
  const uint16_t* emask;  // optional (16-bit out): out = 0 where emask <= 0 (same layout as out)
  long long emask_ld;
  int vec_epi;            // host-checked: 16-bit out/res/emask rows 16-B aligned -> LDS-staged epilogue
  int epi_batch;          // LDS-staged epilogue: load every chunk's res/acc/emask operands up front
  float* ws;              // split-K: fp32 partials [ksplit][M][OCpad] (LDS-DMA kernel), else nullptr
  int ksplit;
  double* stats;          // optional (row-streaming kernel): stats[n / stats_div] += {sum out, sum out^2}
  int stats_div;
  const uint8_t* ucode;   // optional (LDS-DMA, vector epilogue): max-unpool the output with these switch
  int ucode_div;          //   codes [N/ucode_div][OH][OW][OC]; out is then [N][2 OH][2 OW] rows of out_ld
  // storage extents in elements from each base pointer (bindings.cpp: storage bytes past the data
  // pointer); read only by the DV_DEBUG bounds checks (common.h DV_BOUNDS)
  long long x_elems, out_elems, res_elems, emask_elems;
  int relu_cols;          // > 0: ReLU only on output columns < relu_cols (merged GEMMs whose trailing
                          //   columns are pre-activation values, ops/inception.py); 0: every column
  void* out2;             // optional (LDS-staged 16-bit epilogue, plain): columns >= split_col go to
  long long out2_ld;      //   out2[row * out2_ld + col - split_col] instead of out (a merged GEMM whose
  int split_col;          //   leading columns are one consumer's output and the rest another's)
  long long out2_elems;
  const uint16_t* w2;     // optional second-GEMM weights of a fused epilogue (conv3x3_unpool_z_launch: the
                          //   next conv-down's taps as a [32][64] matrix, row tap*3+c = W[c][tap][:])
  int pool_t;             // host-checked (POOL epilogue): OC, out_ld % 4 == 0, out 8-B / out_code 4-B aligned ->
                          //   the transposed pooled-max epilogue (conv_dma_impl.h:epilogue_pool_t)
  float* skw;             // optional: KW3P stream-K workspace, kSkSlotFloats fp32 per workgroup (partial tiles)
  unsigned* skflag;       //   + one ready flag per workgroup; zeroed by the launcher before each launch
  int skslots;            //   workspace slots (workgroups) allocated: the launch needs G <= skslots
  unsigned* skerr;        //   host-coherent counter of hand-offs that timed out (bindings.cpp sk_errors())
  // 1-bit ReLU masks (LDS-staged epilogue only; host: OC % 8 == 0): bit c % 8 of byte c / 8 of row m.
  // obits: written with the output, bit = (stored 16-bit value > 0); ebits: replaces emask (read 1/16
  // of its bytes). The launcher sets them only on kernels whose epilogue is epilogue_lds (conv_pw).
  uint8_t* obits;
  long long obits_ld;     // bytes per row
  const uint8_t* ebits;
  long long ebits_ld;
  // fused stem (conv3x3_stem_pool_launch): the first conv's packed weights are w2 ([64][kpad2], K index
  // tap * 8 + c of the 8-channel RGB input) and its fp32 bias bias2
  const float* bias2;
  int kpad2;
  // optional (KW3 / KW3P kernels): the 3x3 weights as the byte image their B stages hold, built once at
  // weight-load time (ops/conv.py kw3_pack): 1-KiB pieces piece[step = cc*3 + kh][kw][row block of 16], lane l
  // of a piece = 8 elements of row rb*16 + (l >> 2) at w column (kh*3 + kw)*C + cc*32 + 8*((l & 3) ^ swizzle);
  // OCpad*9*C elements (no K padding). nullptr: absent or switched off (DV_KW3_BPACK=0), B is read from w
  const uint16_t* wp;
  long long wp_elems;     // storage extent of wp (DV_DEBUG bounds checks, as x_elems)
};
// KW3P stream-K: fp32 partial-tile slot per workgroup (BM x BN = 65536 for both KW3P tile shapes)
constexpr long long kSkSlotFloats = 256LL * 256LL;
constexpr int kSkMaxWg = 1024;

// grouped LDS-DMA launch of up to kGroupMax independent problems (conv_dma.hip:conv_dma_group_launch)
constexpr int kGroupMax = 4;
struct ConvGroup {
  ConvArgs p[kGroupMax];
  int start[kGroupMax + 1];  // first workgroup of each problem (prefix sums of the tile counts)
  int tiles_n[kGroupMax];
  int n;
};

// Route report: which kernel the last conv() call on this thread launched (bindings.cpp conv_route()).
// A plain thread-local record the launchers fill where they pick the kernel (a few integer stores, no
// getenv, no formatting on the launch path); bindings.cpp clears it at entry and formats it on request.
// Tests assert it, so a threshold change or another CU count cannot silently turn a kernel's test into
// a test of its fallback.
enum ConvRouteKind : int {
  CR_NONE = 0, CR_IGEMM, CR_HALO_V1, CR_HALO_V2, CR_POOL_V3, CR_C8_STREAM, CR_HS16, CR_HS32, CR_PW, CR_DMA,
  CR_KW3, CR_KW3P, CR_GROUP,
};
enum ConvRouteEpi : int {
  CR_E_NONE = 0, CR_E_REG, CR_E_LDS, CR_E_UNPOOL, CR_E_POOL, CR_E_STRIPS, CR_E_PERSIST,
  CR_E_POOL_T, CR_E_POOL_LDS,  // LDS-DMA pooled-max epilogues: DPP-transposed 8-B stores / staged through LDS
};
enum ConvRouteFlag : int {
  CR_F_SK = 1,        // KW3P stream-K
  CR_F_OCSPLIT = 2,   // halo-stream: two launches over the output-channel halves
  CR_F_TAIL = 4,      // KW3 / KW3P full rounds + a 128 x 128 DMA tail launch from row m_base
  CR_F_UNPOOL = 8,    // pre-pass: the unpooled input was materialized (unpool2x2)
  CR_F_RELU_COPY = 16,  // pre-pass: dense ReLU copy of the input
  CR_F_MASK = 32,     // ReLU-masked A operand (the masked DMA tiles)
};
struct ConvRoute {
  int kind, bm, bn, stages, ksplit, epi, flags, m_base, cfg;
  int bpack;  // KW3 / KW3P: B was staged from the packed image (not part of the route string; conv_bpack())
};
extern __thread ConvRoute g_route;  // defined in conv_dma.hip
// A launcher records its WHOLE choice (nothing of an earlier launcher that recorded and then declined, or of
// the first half of a two-launch form, survives); only the pre-pass flags bindings.cpp set before it stay.
static inline void route_set(int kind, int bm, int bn, int stages, int ksplit, int epi, int flags = 0) {
  g_route = ConvRoute{kind, bm, bn, stages, ksplit, epi, (g_route.flags & (CR_F_UNPOOL | CR_F_RELU_COPY)) | flags, 0, 0};
}

// The route as text, e.g. "dma 128x128 st2 ks1", "kw3p 256x256 lds sk", "kw3 256x256 + dma 128x128 tail
// m_base=65536", "unpool2x2 > dma 64x64 st3 ks1", "group cfg8"; "none": no launch recorded.
static inline std::string route_str(const ConvRoute& r) {
  static const char* const kEpi[] = {"", " reg", " lds", " unpool", " pool", " strips", " persist", " pool_t", " pool_lds"};
  const char* epi = (r.epi >= 0 && r.epi <= 8) ? kEpi[r.epi] : "";
  char b[160];
  switch (r.kind) {
    case CR_IGEMM: std::snprintf(b, sizeof b, "igemm %dx%d", r.bm, r.bn); break;
    case CR_HALO_V1: std::snprintf(b, sizeof b, "halo_v1%s", epi); break;
    case CR_HALO_V2: std::snprintf(b, sizeof b, "halo_v2"); break;
    case CR_POOL_V3: std::snprintf(b, sizeof b, "pool_v3"); break;
    case CR_C8_STREAM: std::snprintf(b, sizeof b, "c8_stream"); break;
    case CR_HS16:
    case CR_HS32:
      std::snprintf(b, sizeof b, "%s oc%d%s%s%s", r.kind == CR_HS16 ? "hs16" : "hs32", r.bn, epi,
                    (r.flags & CR_F_OCSPLIT) ? " ocsplit" : "", r.cfg == 1 ? " stem" : "");
      break;
    case CR_PW: std::snprintf(b, sizeof b, "pw %dx%d", r.bm, r.bn); break;
    case CR_DMA:
      std::snprintf(b, sizeof b, "dma %dx%d st%d ks%d%s%s", r.bm, r.bn, r.stages, r.ksplit, epi,
                    (r.flags & CR_F_MASK) ? " mask" : "");
      break;
    case CR_KW3:
    case CR_KW3P: {
      int n = std::snprintf(b, sizeof b, "%s %dx%d%s%s", r.kind == CR_KW3 ? "kw3" : "kw3p", r.bm, r.bn, epi,
                            (r.flags & CR_F_SK) ? " sk" : "");
      if ((r.flags & CR_F_TAIL) && n > 0 && n < (int)sizeof b)
        std::snprintf(b + n, sizeof b - n, " + dma 128x128 tail m_base=%d", r.m_base);
      break;
    }
    case CR_GROUP: std::snprintf(b, sizeof b, "group cfg%d", r.cfg); break;
    default: std::snprintf(b, sizeof b, "none"); break;
  }
  std::string out;
  if (r.flags & CR_F_UNPOOL) out += "unpool2x2 > ";
  if (r.flags & CR_F_RELU_COPY) out += "relu_copy > ";
  return out + b;
}

// The same for the multi-kernel launchers of misc.hip (seed_deconv3x3, maxpool2x2, unpool2x2) and for
// bindings.cpp:deprocess_mosaic: the name of the kernel (pair) the last such call on this thread chose
// (bindings.cpp misc_route()). One pointer store to a string literal on the launch path.
extern __thread const char* g_misc_route;  // defined in misc.hip

int conv_igemm_launch(const ConvArgs& a, int amode, int epi, hipStream_t stream);
// compute units of the current device, cached per device (bindings.cpp): the one source of the CU count. Per call
// only hipGetDevice, a host-side query that is legal during stream capture; the attribute is read once per device.
int device_cus();
// LDS-DMA family (FWD / TRANSPOSE, optionally ReLU-masked): the plan of a launch (conv_dma_plan.h) under the process's
// knobs on the current device, and the launch of a plan (< 0 when it declines: DmaPlan::status). The caller supplies the
// workspaces the plan asks for (ws / ksplit for plan.ksplit > 1, skw / skflag / skslots for plan.sk) and reduces.
struct DmaPlan;
DmaPlan conv_dma_plan(const ConvArgs& a, int amode, int epi);
int conv_dma_run(const ConvArgs& a, const DmaPlan& plan, hipStream_t stream);
// tuning override: force DMA tile config cfg (> 0, conv_dma_plan.h:kDmaTiles 1..17) and split-K ks (> 0); 0 = auto
void conv_dma_tune(int cfg, int ks);
// the split-K reduction epilogue (bias, ReLU, accumulate, residual, emask; 16-bit / fp32 out)
int splitk_reduce_launch(const ConvArgs& a, int epi, hipStream_t stream);
// launch of 1..kGroupMax problems that share a group config (plan.group_cfg != 0), dtype, A mode and epilogue
int conv_dma_group_launch(const ConvArgs* ps, int n, int amode, int epi, hipStream_t stream);
// direct VALU kernels for InceptionV3's conv2d_1 (8-ch padded RGB -> 32, 3x3 / stride 2): forward and
// input gradient (conv_stem.hip); < 0: unsupported geometry
int stem_conv_fwd_launch(const uint16_t* x, const float* w, const float* bias, uint16_t* y, int N, int H, int W,
                         int OH, int OW, int C, int cr, int cout, int k, int stride, int pad, int relu, long long x_ld,
                         long long y_ld, int dtype, hipStream_t s);
int stem_conv_dgrad_launch(const uint16_t* gy, const float* w, uint16_t* gx, int N, int H, int W, int OH, int OW,
                           int C, int cr, int cout, int k, int stride, int pad, long long gy_ld, long long gx_ld,
                           int dtype, hipStream_t s);
// persistent pointwise (1x1 / s1 / p0) conv at large M, 16-bit LDS-staged epilogue (conv_pw.hip);
// < 0: unsupported shape / mode (use conv_dma_run)
int conv_pw_launch(const ConvArgs& a, hipStream_t stream);

// ---- misc kernels (misc.hip) ----
// per-(image, channel) sums of a NHWC bf16 / fp16 (f16 = 1) tensor: sums[n][c] = sum_{hw} x[n][hw][c]
int channel_sum_launch(const uint16_t* x, float* sums, int N, int HW, int C, int f16, hipStream_t s);
// per-row stable top-k of positive values: idx[n][k] (-1 when fewer than k positives)
int topk_pos_launch(const float* v, int* idx, float* val, int N, int C, int k, hipStream_t s);
// one-channel seeded deconv: out[b][h][w][ci] = relu(sum_taps S[b][h+kh-1][w+kw-1] * wt[f_b][kh][kw][ci])
int seed_deconv3x3_launch(const float* S, const int* f, const uint16_t* wt, uint16_t* out,
                          int B, int H, int W, int Cin, int F, int f16, hipStream_t s);
// fp32 recon [B*4][224][224][3] -> u8 mosaic [B][448][448][3] (channel-reversed), Keras deprocess
int deprocess_mosaic_launch(const float* recon, uint8_t* out, int B, int H, int W, int tiles,
                            int reverse_channels, hipStream_t s);
// per-group {sum, sum of squares} (fp64, atomically ADDED to stats[g][2]) of fp32 data [groups][per_group]
int recon_stats_launch(const float* x, double* stats, long long per_group, int groups, hipStream_t s);
// deprocess with precomputed per-image stats (single pass, 4 px per thread); W % 4 == 0
int deprocess_apply_launch(const float* recon, const double* stats, uint8_t* out, int B, int H, int W, int tiles,
                           int reverse_channels, hipStream_t s);
// uint8 [B][Hs][Ws][3] RGB -> bf16 / fp16 (f16 = 1) NHWC [B][OH][OW][Cpad]: cv2 INTER_LINEAR resize +
// caffe mean subtract
int resize_preprocess_launch(const uint8_t* img, int B, int Hs, int Ws, uint16_t* out, int OH, int OW,
                             int Cpad, int mode, int f16, hipStream_t s);
// fmt: 0 bf16 preprocessed, 1 u8 resized RGB, 2 fp16 preprocessed
int resize_batch_launch(const uint8_t* blob, const long long* table, int B, void* out, int OH, int OW, int Cpad,
                        int fmt, hipStream_t s);
int preprocess_u8_launch(const uint8_t* in, uint16_t* out, long long P, int Cpad, int f16, hipStream_t s);
// standalone 2x2/s2 max pool with switch codes, and its inverse (unpool scatter to full res)
int maxpool2x2_launch(const uint16_t* x, uint16_t* out, uint8_t* code, int N, int H, int W, int C,
                      int f16, hipStream_t s);
// seed maps of the deconvnet's B*K chains (all / max mode, optional max-unpool for pool targets)
int seed_map_launch(const uint16_t* out4, const int* idx, const uint8_t* code, float* S, int BK, int K, int H, int W,
                    int C, int mode, int f16, hipStream_t s);
int unpool2x2_launch(const uint16_t* p, const uint8_t* code, uint16_t* out, int N, int H, int W,
                     int C, int code_div, int relu, hipStream_t s);

}  // namespace dv

namespace dv {
// k x k pooling (pool.hip). kind 0 max (idx = uint8 window position), 1 avg (count_include_pad=0);
// dir 0 forward (in = x [N,H,W,C], out = y [N,OH,OW,C]), 1 backward (in = gy, out = gx)
// strided-conv input gradient from its s x s (s <= 2) parity-class parts [N, hc, wc, ld] (nullptr: zero class),
// optional accumulate into gx and emask (zero where emask <= 0)
int subpixel_merge_launch(const uint16_t* const* p, const int* hc, const int* wc, const int* ld, const uint16_t* emask,
                          uint16_t* gx, int N, int H, int W, int C, int s, int acc, int dtype, hipStream_t st);
int subpixel_scatter_launch(const uint16_t* E, const uint16_t* emask, uint16_t* gx, int N, int H, int W, int C, int OH,
                            int OW, int s, int dtype, hipStream_t st);
int pool_launch(int kind, int dir, const uint16_t* in, uint16_t* out, uint8_t* idx, int N, int H, int W, int C,
                int OH, int OW, int k, int s, int pad, int dtype, hipStream_t st, long long x_ld = 0,
                long long y_ld = 0, const float* bias = nullptr, int relu = 0, int acc = 0);
// DeepDream loss: per-(image, block) partial sums of x^2 over the map minus a b-pixel border
// (part [N][parts]), and its gradient gx = 2*scale[n]*x in the core, 0 on the border
// fused DeepDream update: per-image mean |g| partials, loss from the sumsq partials, device-side
// max_loss flag, x += step * g / mean|g| (fp32) and the next 16-bit network input (8 channels)
int dream_update_launch(const uint16_t* g, float* x, uint16_t* xin, float* gpart, int gparts, const float* lpart,
                        const float* lcoef, int L, int lparts, uint8_t* done, float* loss, float step, float max_loss,
                        int N, int H, int W, int dtype, hipStream_t s);
// DeepDream octave transition: y = corner-aligned bilinear resize of (a + b - c) (fp32 NHWC, 3 channels; b, c may
// be null), optionally also written as the 16-bit 8-channel network input yin
int octave_resize_launch(const float* a, const float* b, const float* c, float* y, uint16_t* yin, int N, int Hs, int Ws, int Hd, int Wd,
                         int dtype, hipStream_t s);
// Laplacian-pyramid gradient normalisation (dream_lap.hip), one level per launch. A level's maps are cut into
// LAP_TILE_H x LAP_TILE_W tiles, one block and one partial each: parts = lap_tiles(H) * lap_tiles_w(W).
// src / dst: DT_BF16 / DT_F16 = the 16-bit 8-channel layout [N,H,W,8] (channels 0..2 used, 3..7 written as
// zero), LAP_F32 = fp32 [N,H,W,3].
constexpr int LAP_TILE_H = 16, LAP_TILE_W = 32, LAP_F32 = 2, LAP_MAX_LEVELS = 5;
inline int lap_tiles(int H) { return (H + LAP_TILE_H - 1) / LAP_TILE_H; }
inline int lap_tiles_w(int W) { return (W + LAP_TILE_W - 1) / LAP_TILE_W; }
// split: lo [N,ceil(H/2),ceil(W/2),3] = down(x), hi [N,H,W,3] = x - up(lo), hpart [N][parts] = block partials of
// sum hi^2; lpart (null unless this is the last level) [N][parts] = partials of sum lo^2
int lap_split_launch(const void* x, int src, float* lo, float* hi, float* hpart, float* lpart, int N, int H, int W,
                     hipStream_t s);
// merge: out [N,H,W,*] = up(sp * prev) + sh * hi. scales ([N][S], explicit): sh = scales[n][si], sp = scales[n][0]
// if first else 1; scales null: sh = 1 / max(sqrt(sum hpart[n][:hparts] / (3 H W)), eps), sp the same from ppart
// over prev's elements if first (prev is the coarsest lo) else 1
int lap_merge_launch(const float* prev, const float* hi, void* out, int dst, const float* scales, int S, int si,
                     const float* hpart, int hparts, const float* ppart, int pparts, float eps, int first, int N, int H,
                     int W, hipStream_t s);
// Occlusion sensitivity (occlusion.hip; Zeiler & Fergus section 4.2). A p x p patch slides over an S x S image with
// stride s: per axis g = ceil((S - p) / s) + 1 positions o_i = min(i s, S - p), P = g^2 patches. Valid geometry:
// 16 <= S <= 4096, 8 <= p <= S / 2, 4 <= s <= p, P <= 255; every launcher returns -1 outside it.
// OCC_PIX pixels per block (one per thread), one max|heat| partial per block: parts = occ_parts(S).
constexpr int OCC_PIX = 256, OCC_RUN = 16, OCC_MAX_P = 255;
inline int occ_parts(int S) { return (S * S + OCC_PIX - 1) / OCC_PIX; }
inline int occ_grid(int S, int p, int s) {  // g, or -1 outside the definition
  if (S < 16 || S > 4096 || p < 8 || 2 * p > S || s < 4 || s > p) return -1;
  const int g = (S - p + s - 1) / s + 1;
  return g * g <= OCC_MAX_P ? g : -1;
}
// xv [B (P + 1), S, S, 8] 16-bit: variant 0 = x0 [B, S, S, 8], variant 1 + i g + j = x0 with all 8 channels zero on
// rows o_i .. o_i + p - 1, columns o_j .. o_j + p - 1
int occlude_variants_launch(const uint16_t* x0, uint16_t* xv, int B, int S, int p, int s, hipStream_t st);
// heat [B, 4, S, S] fp32 = mean over the covering patches of scores[b, 0, f] - scores[b, 1 + i g + j, f], f = idx[b, k]
// (scores [B, P + 1, C] fp32, idx [B, 4] int32; f outside 0 .. C - 1: zero map); part [B, 4, parts] = block max |heat|
int occlusion_heat_launch(const float* scores, const int* idx, float* heat, float* part, int B, int C, int S, int p,
                          int s, hipStream_t st);
// out u8 [B, 2 S, 2 S, 3]: tile k at [[0, 1], [2, 3]] = x0 + mean colour blended with red (heat >= 0) / blue by
// 0.6 |heat| / max |heat[b, k]|; black where idx[b, k] < 0
int occlusion_overlay_launch(const float* heat, const float* part, const int* idx, const uint16_t* x0, uint8_t* out,
                             int B, int S, int dtype, hipStream_t st);
// Activation maps (actmap.hip): heat [B, 4, S, S] fp32 = channel idx[b, k] of act [B, H, W, C] (16-bit NHWC) upsampled
// bilinearly (half-pixel centres) by r = S / H; a filter outside 0 .. C - 1 gives a zero map; part [B, 4, occ_parts(S)] =
// block max |heat|, the layout occlusion_overlay_launch consumes. Valid: 16 <= S <= 4096, H == W, r a power of two in
// 1 .. 64, C % 8 == 0, H W C <= 2^31 - 1, 1 <= B <= 65535; -1 outside.
int activation_heat_launch(const uint16_t* act, const int* idx, float* heat, float* part, int B, int H, int W, int C,
                           int S, int dtype, hipStream_t st);
// tiled DeepDream step: rolled tile gather -> owned-pixel pack (+ unit loss / sum|g| tail) ->
// [all-gather of packs over ranks] -> update of the fp32 image straight from the packs
int tile_gather_launch(const float* x, uint16_t* xin, const int* plan, const int* shift, int units, int rank, int world,
                       int k0, int H, int W, int Th, int Tw, int dtype, hipStream_t s);
int tile_pack_launch(const uint16_t* g, uint16_t* pack, const int* plan, const float* lpart, const float* lcoef, int L,
                     int lparts, int units, int ucap, int rank, int world, int k0, int Th, int Tw, int dtype, hipStream_t s);
long long tile_pack_elems(int ucap, int Th, int Tw);  // 16-bit elements of one rank's pack
// packs: [chunks][world][pack_elems], units_per_rank = units per rank and chunk (dream.hip:tile_update_kernel)
int tile_update_launch(const uint16_t* packs, long long pack_elems, int units_per_rank, const int* plan, int nunits,
                       const int* shift, float* x, uint8_t* done, float* loss, float step, float max_loss, int world,
                       int H, int W, int Th, int Tw, int dtype, hipStream_t s);
int sumsq_core_launch(const uint16_t* x, float* part, int parts, int N, int H, int W, int C, int b, int dtype,
                      hipStream_t s);
int sumsq_core_bwd_launch(const uint16_t* x, const float* scale, const uint16_t* addend, uint16_t* gx, int N, int H, int W, int C, int b,
                          int dtype, hipStream_t s);
// sumsq_core_bwd + the forward partials (part [N][parts], as sumsq_core) in one pass
int sumsq_core_fused_launch(const uint16_t* x, const float* scale, const uint16_t* addend, uint16_t* gx, float* part,
                            int parts, int N, int H, int W, int C, int b, int dtype, hipStream_t s);
// guided DeepDream loss (dream_guide.hip): a [N,H,W,C] matched against the guide features y [G,Q,C] of guide
// gidx[n]; per core position the best-scoring guide row q* (lowest q on ties). part [N][parts] (optional) gets
// the block partials of sum_p s[p][q*], gx (optional) = addend + scale[n] * y[q*] * (mask ? a > 0 : 1) on the
// core and addend (or 0) on the border. C % 32 == 0, parts <= GUIDE_MAX_PARTS; < 0: refused
constexpr int GUIDE_MAX_PARTS = 32;
int guide_match_launch(const uint16_t* a, const uint16_t* y, const int* gidx, const float* scale,
                       const uint16_t* addend, uint16_t* gx, float* part, int parts, int N, int H, int W, int C, int Q,
                       int G, int b, int mask, int dtype, hipStream_t s);
// col2im of a strided conv's input gradient for <= 8 input channels (output padded to 8 channels)
struct Col2ImGeom {
  int N, H, W, OH, OW, KH, KW, stride, pad_h, pad_w, Cr, J_ld;
};
int col2im_launch(const uint16_t* cols, uint16_t* gx, const Col2ImGeom& g, int dtype, hipStream_t s);
// fused GEMM + col2im input gradient of ResNet-50's conv1 (conv_stem_dgrad.hip): dy [N,OH,OW,C],
// optional ReLU mask like dy, wb = the cols GEMM's B^T [w_rows][w_ld] (row (kh*KW+kw)*Cr+c),
// gx [N,H,W,8]; < 0: geometry not covered
struct StemDgradGeom {
  int N, H, W, OH, OW, C, KH, KW, stride, pad, Cr, w_rows, w_ld;
};
// ResNet-50 conv1 forward (7x7 / 2, pad 3, RGB -> 64) on the tap-paired MFMA kernel (conv_stem7.hip);
// < 0: not its geometry
int stem7_fwd_launch(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int N, int H, int W, int OH,
                     int OW, int relu, int dtype, hipStream_t s);
int stem_dgrad_fused_launch(const uint16_t* gy, const uint16_t* mask, const uint16_t* wb, uint16_t* gx,
                            const StemDgradGeom& g, int dtype, hipStream_t s);
// GPU baseline JPEG encode of B same-size RGB images (jpeg_gpu.hip): entropy-coded scans (restart
// marker after every MCU row, no header/EOI) packed back to back into `packed` at off[0..B];
// `tables` = a device copy of dvjpeg::GpuTables, `ws` = jpeg_gpu_ws_bytes(B, H, W) of workspace,
// `packed` >= B * jpeg_gpu_out_cap(H, W) bytes; W <= jpeg_gpu_max_width()
long long jpeg_gpu_ws_bytes(int B, int H, int W);
long long jpeg_gpu_out_cap(int H, int W);
int jpeg_gpu_max_width();
int jpeg_gpu_launch(const uint8_t* rgb, int B, int H, int W, const void* tables, void* ws, uint8_t* packed,
                    long long* off, hipStream_t s);
// GPU JPEG decode of a batch (jpeg_dec_gpu.hip): dequantize + IDCT into planes, then chroma upsampling +
// colour into packed RGB, two launches. `table`: device int32 [B][12] rows {coefficient offset, RGB offset,
// H, W, kind, quantizer offset, plane offset, first block, first 4-pixel item, 0, 0, 0}, byte offsets into
// `blob` (validated by bindings.cpp:jpeg_dec_batch); total_blocks / total_items: the sums behind the prefixes
int jpeg_dec_launch(uint8_t* blob, long long blob_bytes, const int* table, int B, int total_blocks, int total_items,
                    hipStream_t s);
// row softmax (fp32 [M][N])
int softmax_rows_launch(const float* x, float* y, int M, int N, hipStream_t s);
// bench.py --emulate-rccl-world: `channels` workgroups copy `bytes` (src repeated) paced to `gbs` GB/s (misc.hip)
int paced_copy_launch(const void* src, long long src_bytes, void* dst, long long bytes, int channels, double gbs,
                      hipStream_t s);
// halo-tile 3x3/s1/p1 conv for OC tiles of 16/64 at large spatial sizes (optional fused unpool)
int conv3x3_halo_launch(const ConvArgs& a, int unpool, int epi, hipStream_t s, bool* stats_done = nullptr);
// 3x3 conv 64 -> 64 + bias + ReLU + fused 2x2 max-pool/switch (bf16); < 0 if the shape is unsupported
int conv3x3_pool_v3_launch(const ConvArgs& a, hipStream_t s);
// unpool + 3x3 conv 64 -> 64 (ReLU) whose epilogue multiplies the tile by a.w2 ([32][64]): writes the
// per-tap partial products Z [N, H, W, 32] (bf16, out_ld 32) of the following 64 -> 3 conv-down
int conv3x3_unpool_z_launch(const ConvArgs& a, hipStream_t s);
// out[n, y, x, c] = ReLU(sum_taps Z[n, y+kh-1, x+kw-1, (kh*3+kw)*3 + c]) fp32 [N, H, W, 3] + optional
// per-image {sum, sum^2} (fp64, image n / stats_div): the 3x3 shift-add that finishes a Z map
int zsum3x3_launch(const uint16_t* z, float* out, int N, int H, int W, double* stats, int stats_div, hipStream_t s);
// first layer: 3x3 conv of an 8-channel image -> <= 64 channels, bias + ReLU, bf16 (< 0: unsupported)
int conv3x3_c8_stream_launch(const ConvArgs& a, hipStream_t s);
// fused VGG16 stem: 3x3 conv 8 (RGB) -> 64 + ReLU (weights a.w2 / a.bias2), 3x3 conv 64 -> 64 + ReLU
// (a.w / a.bias) and the 2x2 max-pool with switches, one hs16 launch; the 64-channel map between the two
// convs lives only in LDS (conv_halo_stream.hip; < 0: unsupported)
int conv3x3_stem_pool_launch(const ConvArgs& a, hipStream_t s);
// halo-stream 3x3 s1 p1 conv, C % 32 == 0 -> OCpad 64 / 128, 16-bit out or fused 2x2 max-pool +
// switch (epi CONV_E_BF16 / CONV_E_POOL; < 0: unsupported)
int conv3x3_hs_launch(const ConvArgs& a, int epi, hipStream_t s, bool* lepi_used = nullptr);
}  // namespace dv
