// Laplacian-pyramid gradient normalisation for DeepDream ("lapnorm"; engine/deepdream.py:DeepDream._fused_step
// with DreamSettings.lap_levels = n > 0). Per image and channel, fp32, NHWC with 3 channels:
//   k = [1, 4, 6, 4, 1] / 16, filter k (x) k, stride 2, TensorFlow SAME with zeros outside: for a side L the
//   coarse side is ceil(L / 2) and the leading pad is 1 (L even) or 2 (L odd)
//   down(x)[i][j]  = sum_ab k[a] k[b] x[2i + a - padH][2j + b - padW]
//   up(lo)[y][x]   = 4 sum k[a] k[b] lo[i][j] over 2i + a - padH = y, 2j + b - padW = x   (4 x the adjoint of down)
//   split:  lo = down(x); hi = x - up(lo); next level on lo       merge:  img = up(img) + s * hi
// Two kernels, one launch each per level (2n launches per step), no atomics, every output element written
// exactly once, nothing pre-zeroed:
//   lap_split_kernel  block = one LTH x LTW tile of hi. Stages the input tile with a 4-pixel halo in LDS (level 0
//                     reads the 16-bit 8-channel network-input gradient, deeper levels fp32), computes the
//                     (LTH/2 + 2) x (LTW/2 + 2) lo tile hi needs (one halo row / column each side recomputed by
//                     the neighbours), writes the lo rows / columns it owns, hi = x - up(lo), and its partial
//                     sums of hi^2 (and of the owned lo^2 on the last level) to part[n][block].
//   lap_merge_kernel  block = one tile of the level's output. Every block re-reduces the level's partials
//                     into the per-image scale s = 1 / max(sqrt(mean level^2), eps) in a fixed order (as
//                     dream_update_kernel does with gpart), stages the coarser image's tile in LDS (scaled by
//                     s[0] when it is the coarsest lo), writes up(prev) + s * hi: fp32, or on level 0 packed
//                     into the 16-bit 8-channel layout (channels 3..7 zero) with one 16-B store per pixel.
// The up taps per axis: 2 k[a] over the a with the parity of (y + pad): {1/8, 3/4, 1/8} or {1/2, 1/2}.
#include "common.h"
#include "kernels.h"

namespace dv {

namespace {

constexpr int LTH = LAP_TILE_H, LTW = LAP_TILE_W;  // hi / output tile in pixels (both even)
constexpr int LIH = LTH + 8, LIW = LTW + 8;        // staged input tile: 4 pixels of halo on every side
constexpr int LLH = LTH / 2 + 2, LLW = LTW / 2 + 2;  // lo tile: one halo row / column on every side
constexpr int SRC_F32 = LAP_F32;                   // (DT_BF16 / DT_F16: the 16-bit 8-channel layout)

__device__ __forceinline__ float lap_k(int a) { return a == 2 ? 0.375f : ((a & 1) ? 0.25f : 0.0625f); }

// block sum of v -> part[0] (thread 0); red: 4 floats of LDS
__device__ __forceinline__ void block_sum_to(float v, float* red, float* part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *part = (red[0] + red[1]) + (red[2] + red[3]);
}

// up(lo)[ly][lx] channel c from the lo tile (origin: coarse row y0/2 - 1, column x0/2 - 1; zeros outside the map)
__device__ __forceinline__ float lap_up(const float (*lo_t)[LLW * 3], int ly, int lx, int c, int pH, int pW) {
  float up = 0.f;
  for (int a = (ly + pH) & 1; a < 5; a += 2) {
    const int li = ((ly + pH - a) >> 1) + 1;
    float row = 0.f;
    for (int b = (lx + pW) & 1; b < 5; b += 2) row += 2.f * lap_k(b) * lo_t[li][(((lx + pW - b) >> 1) + 1) * 3 + c];
    up += 2.f * lap_k(a) * row;
  }
  return up;
}

}  // namespace

// x: level input [N, H, W, 3] fp32 (SRC_F32) or [N, H, W, 8] 16-bit (channels 0..2); lo [N, Hl, Wl, 3],
// hi [N, H, W, 3] fp32; hpart / lpart [N][gridDim.y * gridDim.x] (lpart: last level only, else null)
template <int SRC>
__global__ void __launch_bounds__(256) lap_split_kernel(const void* __restrict__ xv, float* __restrict__ lo,
                                                        float* __restrict__ hi, float* __restrict__ hpart,
                                                        float* __restrict__ lpart, int H, int W) {
  __shared__ float in_t[LIH][LIW * 3];
  __shared__ float lo_t[LLH][LLW * 3];
  __shared__ float red[2][4];
  const int n = blockIdx.z, y0 = blockIdx.y * LTH, x0 = blockIdx.x * LTW, tid = threadIdx.x;
  const int Hl = (H + 1) >> 1, Wl = (W + 1) >> 1, pH = (H & 1) ? 2 : 1, pW = (W & 1) ? 2 : 1;
  if constexpr (SRC == SRC_F32) {
    const float* x = reinterpret_cast<const float*>(xv) + (long long)n * H * W * 3;
    for (int e = tid; e < LIH * LIW * 3; e += 256) {
      const int r = e / (LIW * 3), q = e - r * (LIW * 3);
      const int y = y0 - 4 + r, xe = (x0 - 4) * 3 + q;
      float v = 0.f;
      if (y >= 0 && y < H && xe >= 0 && xe < W * 3) v = x[(long long)y * W * 3 + xe];
      in_t[r][q] = v;
    }
  } else {
    const uint16_t* x = reinterpret_cast<const uint16_t*>(xv) + (long long)n * H * W * 8;
    for (int p = tid; p < LIH * LIW; p += 256) {
      const int r = p / LIW, cc = p - r * LIW;
      const int y = y0 - 4 + r, xx = x0 - 4 + cc;
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      if (y >= 0 && y < H && xx >= 0 && xx < W) {
        const uint2 v = *reinterpret_cast<const uint2*>(x + ((long long)y * W + xx) * 8);  // channels 0..3
        v0 = to_f<SRC>(v.x & 0xFFFFu);
        v1 = to_f<SRC>(v.x >> 16);
        v2 = to_f<SRC>(v.y & 0xFFFFu);
      }
      in_t[r][cc * 3 + 0] = v0;
      in_t[r][cc * 3 + 1] = v1;
      in_t[r][cc * 3 + 2] = v2;
    }
  }
  __syncthreads();
  // lo tile: coarse rows y0/2 - 1 .. y0/2 + LTH/2; tile row li reads input-tile rows 2 li + 2 - pH + a
  float lacc = 0.f;
  float* lon = lo + (long long)n * Hl * Wl * 3;
  for (int e = tid; e < LLH * LLW * 3; e += 256) {
    const int li = e / (LLW * 3), q = e - li * (LLW * 3), lj = q / 3, c = q - lj * 3;
    const int i = (y0 >> 1) - 1 + li, j = (x0 >> 1) - 1 + lj;
    float v = 0.f;
    if (i >= 0 && i < Hl && j >= 0 && j < Wl) {
      const int rb = 2 * li + 2 - pH, cb = 2 * lj + 2 - pW;
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        float row = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) row += lap_k(b) * in_t[rb + a][(cb + b) * 3 + c];
        v += lap_k(a) * row;
      }
      if (li >= 1 && li <= LTH / 2 && lj >= 1 && lj <= LTW / 2) {  // the rows / columns this block owns
        lon[((long long)i * Wl + j) * 3 + c] = v;
        lacc += v * v;
      }
    }
    lo_t[li][q] = v;
  }
  __syncthreads();
  float hacc = 0.f;
  float* hin = hi + (long long)n * H * W * 3;
  for (int e = tid; e < LTH * LTW * 3; e += 256) {
    const int ly = e / (LTW * 3), q = e - ly * (LTW * 3), lx = q / 3, c = q - lx * 3;
    const int y = y0 + ly, xx = x0 + lx;
    if (y < H && xx < W) {
      const float h = in_t[ly + 4][(lx + 4) * 3 + c] - lap_up(lo_t, ly, lx, c, pH, pW);
      hin[((long long)y * W + xx) * 3 + c] = h;
      hacc += h * h;
    }
  }
  const long long pi = (long long)n * gridDim.y * gridDim.x + blockIdx.y * gridDim.x + blockIdx.x;
  block_sum_to(hacc, red[0], hpart + pi);
  if (lpart) block_sum_to(lacc, red[1], lpart + pi);
}

// out = up(sp * prev) + sh * hi for one level: prev [N, Hl, Wl, 3], hi [N, H, W, 3] fp32; out fp32 [N, H, W, 3]
// (OUT == SRC_F32) or 16-bit [N, H, W, 8]. Scales: explicit (scales [N][S]: sh = scales[n][si], sp = scales[n][0]
// when first) or from the partials: sh = 1 / max(sqrt(sum hpart[n][:] / hcount), eps), sp likewise from ppart
// when first (prev is the coarsest lo), else 1.
template <int OUT>
__global__ void __launch_bounds__(256) lap_merge_kernel(const float* __restrict__ prev, const float* __restrict__ hi,
                                                        void* __restrict__ outv, const float* __restrict__ scales,
                                                        int S, int si, const float* __restrict__ hpart, int hparts,
                                                        float hcount, const float* __restrict__ ppart, int pparts,
                                                        float pcount, float eps, int first, int H, int W) {
  __shared__ float lo_t[LLH][LLW * 3];
  __shared__ float sc[2];
  const int n = blockIdx.z, y0 = blockIdx.y * LTH, x0 = blockIdx.x * LTW, tid = threadIdx.x;
  const int Hl = (H + 1) >> 1, Wl = (W + 1) >> 1, pH = (H & 1) ? 2 : 1, pW = (W & 1) ? 2 : 1;
  if (tid < 64) {
    float s_hi, s_prev = 1.f;
    if (scales) {
      s_hi = scales[(long long)n * S + si];
      if (first) s_prev = scales[(long long)n * S];
    } else {
      float t = 0.f;
      for (int p = tid; p < hparts; p += 64) t += hpart[(long long)n * hparts + p];
      s_hi = 1.f / fmaxf(sqrtf(wave_sum(t) / hcount), eps);
      if (first) {
        float u = 0.f;
        for (int p = tid; p < pparts; p += 64) u += ppart[(long long)n * pparts + p];
        s_prev = 1.f / fmaxf(sqrtf(wave_sum(u) / pcount), eps);
      }
    }
    if (tid == 0) {
      sc[0] = s_hi;
      sc[1] = s_prev;
    }
  }
  __syncthreads();
  const float s_hi = sc[0], s_prev = sc[1];
  const float* pn = prev + (long long)n * Hl * Wl * 3;
  for (int e = tid; e < LLH * LLW * 3; e += 256) {
    const int li = e / (LLW * 3), q = e - li * (LLW * 3), lj = q / 3;
    const int i = (y0 >> 1) - 1 + li, j = (x0 >> 1) - 1 + lj;
    float v = 0.f;
    if (i >= 0 && i < Hl && j >= 0 && j < Wl) v = s_prev * pn[((long long)i * Wl + j) * 3 + (q - lj * 3)];
    lo_t[li][q] = v;
  }
  __syncthreads();
  const float* hn = hi + (long long)n * H * W * 3;
  if constexpr (OUT == SRC_F32) {
    float* on = reinterpret_cast<float*>(outv) + (long long)n * H * W * 3;
    for (int e = tid; e < LTH * LTW * 3; e += 256) {
      const int ly = e / (LTW * 3), q = e - ly * (LTW * 3), lx = q / 3, c = q - lx * 3;
      const int y = y0 + ly, xx = x0 + lx;
      if (y < H && xx < W) {
        const long long o = ((long long)y * W + xx) * 3 + c;
        on[o] = lap_up(lo_t, ly, lx, c, pH, pW) + s_hi * hn[o];
      }
    }
  } else {
    uint16_t* on = reinterpret_cast<uint16_t*>(outv) + (long long)n * H * W * 8;
    for (int p = tid; p < LTH * LTW; p += 256) {
      const int ly = p / LTW, lx = p - ly * LTW;
      const int y = y0 + ly, xx = x0 + lx;
      if (y < H && xx < W) {
        const long long o = (long long)y * W + xx;
        const float v0 = lap_up(lo_t, ly, lx, 0, pH, pW) + s_hi * hn[o * 3 + 0];
        const float v1 = lap_up(lo_t, ly, lx, 1, pH, pW) + s_hi * hn[o * 3 + 1];
        const float v2 = lap_up(lo_t, ly, lx, 2, pH, pW) + s_hi * hn[o * 3 + 2];
        *reinterpret_cast<uint4*>(on + o * 8) = uint4{pack2<OUT>(v0, v1), pack2<OUT>(v2, 0.f), 0u, 0u};
      }
    }
  }
}

static bool lap_geom_ok(int N, int H, int W) {
  return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W * 8 <= 0x7FFFFFFFLL && lap_tiles(H) <= 65535;
}

int lap_split_launch(const void* x, int src, float* lo, float* hi, float* hpart, float* lpart, int N, int H, int W,
                     hipStream_t s) {
  if (!lap_geom_ok(N, H, W) || src < 0 || src > SRC_F32) return -1;
  const dim3 grid((unsigned)lap_tiles_w(W), (unsigned)lap_tiles(H), (unsigned)N);
  if (src == SRC_F32)
    hipLaunchKernelGGL(lap_split_kernel<SRC_F32>, grid, dim3(256), 0, s, x, lo, hi, hpart, lpart, H, W);
  else if (src == DT_F16)
    hipLaunchKernelGGL(lap_split_kernel<DT_F16>, grid, dim3(256), 0, s, x, lo, hi, hpart, lpart, H, W);
  else
    hipLaunchKernelGGL(lap_split_kernel<DT_BF16>, grid, dim3(256), 0, s, x, lo, hi, hpart, lpart, H, W);
  return (int)hipGetLastError();
}

int lap_merge_launch(const float* prev, const float* hi, void* out, int dst, const float* scales, int S, int si,
                     const float* hpart, int hparts, const float* ppart, int pparts, float eps, int first, int N, int H,
                     int W, hipStream_t s) {
  if (!lap_geom_ok(N, H, W) || dst < 0 || dst > SRC_F32) return -1;
  if (scales ? (S < 2 || si < 1 || si >= S) : (!hpart || hparts < 1 || (first && (!ppart || pparts < 1)) || !(eps > 0.f)))
    return -1;
  const dim3 grid((unsigned)lap_tiles_w(W), (unsigned)lap_tiles(H), (unsigned)N);
  const float hcount = 3.f * (float)H * (float)W, pcount = 3.f * (float)((H + 1) / 2) * (float)((W + 1) / 2);
  if (dst == SRC_F32)
    hipLaunchKernelGGL(lap_merge_kernel<SRC_F32>, grid, dim3(256), 0, s, prev, hi, out, scales, S, si, hpart, hparts,
                       hcount, ppart, pparts, pcount, eps, first, H, W);
  else if (dst == DT_F16)
    hipLaunchKernelGGL(lap_merge_kernel<DT_F16>, grid, dim3(256), 0, s, prev, hi, out, scales, S, si, hpart, hparts,
                       hcount, ppart, pparts, pcount, eps, first, H, W);
  else
    hipLaunchKernelGGL(lap_merge_kernel<DT_BF16>, grid, dim3(256), 0, s, prev, hi, out, scales, S, si, hpart, hparts,
                       hcount, ppart, pparts, pcount, eps, first, H, W);
  return (int)hipGetLastError();
}

}  // namespace dv
