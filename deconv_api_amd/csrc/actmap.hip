// Activation maps (Zeiler & Fergus, figure 7 (b); engine/activations.py): the feature map of a filter, upsampled
// to the network input and laid over the image by occlusion_overlay_kernel (occlusion.hip).
// act [B, H, W, C] 16-bit NHWC is the target layer's output, S = r H the input side, r a power of two in 1..64.
// Bilinear with half-pixel centres (cv2.INTER_LINEAR, F.interpolate(align_corners=False)) in integers:
//   t = 2 y + 1 - r, y0 = floor(t / 2r), fy = (t - 2r y0) / 2r (exact in fp32), rows clamp(y0), clamp(y0 + 1);
//   heat = (1 - fy) ((1 - fx) a[ya, xa] + fx a[ya, xb]) + fy ((1 - fx) a[yb, xa] + fx a[yb, xb])   (fp32)
// One kernel, no atomics, every element of heat and part written exactly once, nothing pre-zeroed:
//   activation_heat_kernel  thread = one output pixel, block = OCC_PIX pixels of one image for ALL FOUR filters
//                           (grid (occ_parts(S), B)): idx[b, 0..3] is block-uniform, and at C = 64 the four
//                           channels of a tap sit in one 128-B line that is fetched once. The four taps are 2-byte
//                           loads (L1 / L2 hits for r >= 2, a gather at r = 1). The block reduces max |heat| per
//                           filter with wave shuffles + LDS and writes its four partials in the layout
//                           occlusion_overlay_kernel consumes. A filter outside 0 .. C - 1 gives a zero map.
// Index math is 32-bit inside an image (H W C <= 2^31 - 1 and S <= 4096, checked by the launcher); the per-image
// bases are 64-bit.
#include "common.h"
#include "kernels.h"

namespace dv {

template <int DT>
__global__ void __launch_bounds__(OCC_PIX) activation_heat_kernel(const uint16_t* __restrict__ act,
                                                                  const int* __restrict__ idx,
                                                                  float* __restrict__ heat, float* __restrict__ part,
                                                                  int H, int C, int S, int lr) {
  __shared__ float red[4][4];
  const int b = blockIdx.y, tid = threadIdx.x, SS = S * S;
  const int pix = blockIdx.x * OCC_PIX + tid;
  const bool in = pix < SS;
  const int p = in ? pix : SS - 1;  // a thread past the map computes a valid pixel and stores nothing
  const int y = p / S, x = p - y * S;
  const int r = 1 << lr, sh = lr + 1;
  const int ty = 2 * y + 1 - r, tx = 2 * x + 1 - r;
  const int y0 = ty >> sh, x0 = tx >> sh;  // floor: t >= 1 - r > -2r, so y0 >= -1
  const float inv = 1.f / (float)(2 * r);
  const float fy = (float)(ty - (y0 << sh)) * inv, fx = (float)(tx - (x0 << sh)) * inv;
  const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
  const int xa = min(max(x0, 0), H - 1), xb = min(max(x0 + 1, 0), H - 1);
  const int oaa = (ya * H + xa) * C, oab = (ya * H + xb) * C, oba = (yb * H + xa) * C, obb = (yb * H + xb) * C;
  const uint16_t* a = act + (long long)b * H * H * C;
  float m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = idx[b * 4 + k];
    float h = 0.f;
    if (f >= 0 && f < C) {
      const float aa = to_f<DT>(a[oaa + f]), ab = to_f<DT>(a[oab + f]);
      const float ba = to_f<DT>(a[oba + f]), bb = to_f<DT>(a[obb + f]);
      h = (1.f - fy) * ((1.f - fx) * aa + fx * ab) + fy * ((1.f - fx) * ba + fx * bb);
    }
    if (in) heat[((long long)b * 4 + k) * SS + pix] = h;
    m[k] = in ? fabsf(h) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = m[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((tid & 63) == 0) red[k][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4)
    part[((long long)b * 4 + tid) * gridDim.x + blockIdx.x] =
        fmaxf(fmaxf(red[tid][0], red[tid][1]), fmaxf(red[tid][2], red[tid][3]));
}

int activation_heat_launch(const uint16_t* act, const int* idx, float* heat, float* part, int B, int H, int W, int C,
                           int S, int dtype, hipStream_t st) {
  if (S < 16 || S > 4096 || B < 1 || B > 65535 || H < 1 || H != W || C < 8 || C % 8 != 0 || S % H != 0 ||
      (dtype != DT_BF16 && dtype != DT_F16))
    return -1;
  const int r = S / H;
  if (r > 64 || (r & (r - 1)) != 0 || (long long)H * H * C > 0x7FFFFFFFLL) return -1;
  int lr = 0;
  while ((1 << lr) < r) ++lr;
  const dim3 grid((unsigned)occ_parts(S), (unsigned)B);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(activation_heat_kernel<DT_F16>, grid, dim3(OCC_PIX), 0, st, act, idx, heat, part, H, C, S, lr);
  else
    hipLaunchKernelGGL(activation_heat_kernel<DT_BF16>, grid, dim3(OCC_PIX), 0, st, act, idx, heat, part, H, C, S, lr);
  return (int)hipGetLastError();
}

}  // namespace dv
