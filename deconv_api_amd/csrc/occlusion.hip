// Occlusion sensitivity maps (Zeiler & Fergus, "Visualizing and Understanding Convolutional Networks", section 4.2;
// engine/occlusion.py). A p x p patch of the mean colour (zero in preprocessed space) slides over the S x S network
// input with stride s; per axis g = ceil((S - p) / s) + 1 positions o_i = min(i s, S - p) (only the last one can
// be clamped), P = g^2 patches. The P + 1 variants of an image run through the VGG16 forward as one batch; the
// drop of a filter's score under patch (i, j) is spread over the pixels the patch covers.
// Three kernels, no atomics, every output element written exactly once, nothing pre-zeroed:
//   occlude_variants_kernel  thread = one pixel (16 B: the 8 16-bit channels), block = OCC_PIX pixels x a run of
//                            OCC_RUN variants. The pixel is loaded once and stored OCC_RUN times, as itself or as
//                            zeros, so x0 is read (P + 1) / OCC_RUN times in all and the kernel is a pure 16-B
//                            store stream (136 MB per image at the defaults: 196 x 11 blocks).
//   occlusion_heat_kernel    block = OCC_PIX pixels of one (image, filter k). The filter's P drops are staged in
//                            LDS; each thread sums the drops of its covering patches (i ascending, then j
//                            ascending, one fp32 accumulator), divides by their number and the block writes its
//                            max |heat| partial.
//   occlusion_overlay_kernel block = OCC_PIX pixels of one tile. Every block re-reduces its tile's partials in a
//                            fixed order (as dream_update_kernel does with gpart), so all blocks of a tile blend
//                            with the same maximum, then writes the tile's pixels of the 2 x 2 u8 mosaic.
#include "common.h"
#include "kernels.h"

namespace dv {

namespace {

__device__ __forceinline__ int occ_origin(int i, int s, int last) { return min(i * s, last); }

// block max of v >= 0 -> every thread; red: 4 floats of LDS
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

}  // namespace

__global__ void __launch_bounds__(OCC_PIX) occlude_variants_kernel(const uint4* __restrict__ x0, uint4* __restrict__ xv,
                                                                   int S, int p, int s, int g) {
  const int pix = blockIdx.x * OCC_PIX + threadIdx.x, SS = S * S, V = g * g + 1;
  if (pix >= SS) return;
  const int y = pix / S, x = pix - y * S, last = S - p;
  const uint4 v = x0[(long long)blockIdx.z * SS + pix];
  const int v0 = blockIdx.y * OCC_RUN, v1 = min(v0 + OCC_RUN, V);
  uint4* dst = xv + ((long long)blockIdx.z * V + v0) * SS + pix;
  for (int q = v0; q < v1; ++q, dst += SS) {
    bool in = false;
    if (q > 0) {
      const int i = (q - 1) / g, j = (q - 1) - i * g;
      const int oy = occ_origin(i, s, last), ox = occ_origin(j, s, last);
      in = y >= oy && y < oy + p && x >= ox && x < ox + p;
    }
    *dst = in ? uint4{0u, 0u, 0u, 0u} : v;
  }
}

__global__ void __launch_bounds__(OCC_PIX) occlusion_heat_kernel(const float* __restrict__ scores,
                                                                 const int* __restrict__ idx, float* __restrict__ heat,
                                                                 float* __restrict__ part, int C, int S, int p, int s,
                                                                 int g) {
  __shared__ float d[OCC_MAX_P + 1];
  __shared__ float red[4];
  const int b = blockIdx.z, k = blockIdx.y, tid = threadIdx.x, P = g * g, SS = S * S;
  const int f = idx[b * 4 + k];
  const bool live = f >= 0 && f < C;
  if (live && tid < P) {
    const float* sc = scores + (long long)b * (P + 1) * C + f;
    d[tid] = sc[0] - sc[(long long)(tid + 1) * C];
  }
  __syncthreads();
  const int pix = blockIdx.x * OCC_PIX + tid;
  float h = 0.f;
  if (live && pix < SS) {
    const int y = pix / S, x = pix - y * S, last = S - p;
    float acc = 0.f;
    int ny = 0, nx = 0;
    for (int i = 0; i < g; ++i) {
      const int oy = occ_origin(i, s, last);
      if (y < oy || y >= oy + p) continue;
      ++ny;
      nx = 0;
      for (int j = 0; j < g; ++j) {
        const int ox = occ_origin(j, s, last);
        if (x < ox || x >= ox + p) continue;
        ++nx;
        acc += d[i * g + j];
      }
    }
    h = acc / (float)(ny * nx);  // s <= p: every pixel is covered, ny, nx >= 1
  }
  if (pix < SS) heat[((long long)b * 4 + k) * SS + pix] = h;
  const float m = block_max(fabsf(h), red);
  if (tid == 0) part[((long long)b * 4 + k) * gridDim.x + blockIdx.x] = m;
}

template <int DT>
__global__ void __launch_bounds__(OCC_PIX) occlusion_overlay_kernel(const float* __restrict__ heat,
                                                                    const float* __restrict__ part,
                                                                    const int* __restrict__ idx,
                                                                    const uint16_t* __restrict__ x0,
                                                                    uint8_t* __restrict__ out, int S) {
  __shared__ float red[4];
  const int b = blockIdx.z, k = blockIdx.y, tid = threadIdx.x, SS = S * S, parts = gridDim.x;
  float m = 0.f;
  for (int q = tid; q < parts; q += OCC_PIX) m = fmaxf(m, part[((long long)b * 4 + k) * parts + q]);
  m = block_max(m, red);
  const int pix = blockIdx.x * OCC_PIX + tid;
  if (pix >= SS) return;
  const int y = pix / S, x = pix - y * S;
  uint8_t* o = out + (((long long)b * 2 * S + (k >> 1) * S + y) * 2 * S + (k & 1) * S + x) * 3;
  if (idx[b * 4 + k] < 0) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const float h = heat[((long long)b * 4 + k) * SS + pix];
  const float t = m > 0.f ? h / m : 0.f;
  const float a = 0.6f * fabsf(t);
  const uint2 v = *reinterpret_cast<const uint2*>(x0 + ((long long)b * SS + pix) * 8);  // channels 0..3
  const float bg[3] = {to_f<DT>(v.x & 0xFFFFu) + 103.939f, to_f<DT>(v.x >> 16) + 116.779f,
                       to_f<DT>(v.y & 0xFFFFu) + 123.68f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tint = (c == 0 && t >= 0.f) || (c == 2 && t < 0.f) ? 255.f : 0.f;
    const float bc = fminf(fmaxf(bg[c], 0.f), 255.f);
    o[c] = (uint8_t)floorf((1.f - a) * bc + a * tint + 0.5f);
  }
}

int occlude_variants_launch(const uint16_t* x0, uint16_t* xv, int B, int S, int p, int s, hipStream_t st) {
  const int g = occ_grid(S, p, s);
  if (g < 0 || B < 1 || B > 65535) return -1;
  const dim3 grid((unsigned)occ_parts(S), (unsigned)((g * g + 1 + OCC_RUN - 1) / OCC_RUN), (unsigned)B);
  hipLaunchKernelGGL(occlude_variants_kernel, grid, dim3(OCC_PIX), 0, st, reinterpret_cast<const uint4*>(x0),
                     reinterpret_cast<uint4*>(xv), S, p, s, g);
  return (int)hipGetLastError();
}

int occlusion_heat_launch(const float* scores, const int* idx, float* heat, float* part, int B, int C, int S, int p,
                          int s, hipStream_t st) {
  const int g = occ_grid(S, p, s);
  if (g < 0 || B < 1 || B > 65535 || C < 1 || (long long)(g * g + 1) * C > 0x7FFFFFFFLL) return -1;
  hipLaunchKernelGGL(occlusion_heat_kernel, dim3((unsigned)occ_parts(S), 4u, (unsigned)B), dim3(OCC_PIX), 0, st, scores,
                     idx, heat, part, C, S, p, s, g);
  return (int)hipGetLastError();
}

int occlusion_overlay_launch(const float* heat, const float* part, const int* idx, const uint16_t* x0, uint8_t* out,
                             int B, int S, int dtype, hipStream_t st) {
  if (S < 16 || S > 4096 || B < 1 || B > 65535 || (dtype != DT_BF16 && dtype != DT_F16)) return -1;
  const dim3 grid((unsigned)occ_parts(S), 4u, (unsigned)B);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(occlusion_overlay_kernel<DT_F16>, grid, dim3(OCC_PIX), 0, st, heat, part, idx, x0, out, S);
  else
    hipLaunchKernelGGL(occlusion_overlay_kernel<DT_BF16>, grid, dim3(OCC_PIX), 0, st, heat, part, idx, x0, out, S);
  return (int)hipGetLastError();
}

}  // namespace dv
