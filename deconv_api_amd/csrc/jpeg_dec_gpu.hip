// GPU half of the JPEG decode path: quantized DCT coefficients (host: jpeg_dec.cpp) -> RGB bytes that are
// bit-identical to libjpeg-turbo's default decode (islow IDCT, fancy upsampling, its YCbCr -> RGB tables),
// i.e. to what PIL hands the staging ring on the host path.
//
// Two launches per BATCH, whatever the image sizes (the batching of misc.hip:resize_batch_kernel):
//   jpeg_idct_kernel   one 8-lane group per 8x8 block, 32 blocks per workgroup. Lane c loads column c of the
//                      block (coefficients are stored column-major: one 16-byte load, and one more for the
//                      quantizer column), dequantizes and runs pass 1 (columns, descale 11); the 8x8
//                      transpose between the passes goes through LDS; lane r then runs pass 2 on row r
//                      (descale 18, +128, clamp) and stores its 8 samples as one 8-byte store into the
//                      component's plane (block-padded, in the batch's scratch region).
//   jpeg_color_kernel  one thread per 4 horizontal output pixels: the luma samples (one 4-byte load),
//                      chroma upsampled from the planes over the REAL chroma extent (the neighbouring chroma
//                      rows of another MCU row are simply there), colour conversion, 12 bytes out (three
//                      4-byte stores when the destination is 4-byte aligned, bytes otherwise). Work items are
//                      aligned to the image's ROWS, so with W % 4 != 0 only every fourth (W odd) or second row
//                      starts 4-byte aligned and the others take the byte stores, also from the staging
//                      ring's 16-byte aligned layout: correct, slower, and not yet measured apart.
// One int32 table row per image (kJdTab fields) tells both kernels where its data is; `start` fields
// hold the host-built prefix sums of the work items, an image is found by binary search.
// All offsets are int32 byte offsets into one blob (bindings.cpp checks every row against the blob size).
#include "common.h"

namespace dv {
namespace {

// table fields (ops/jpeg_dec.py:plan_batch writes them, bindings.cpp:jpeg_dec_batch validates them)
enum { JD_COEF = 0, JD_RGB = 1, JD_H = 2, JD_W = 3, JD_KIND = 4, JD_QT = 5, JD_PLANE = 6, JD_BLK0 = 7, JD_ITEM0 = 8 };
constexpr int kJdTab = 12;
enum { K444 = 0, K422 = 1, K420 = 2, KGREY = 3 };

// last row whose `field` is <= idx (the rows' starts ascend from 0)
__device__ __forceinline__ int find_image(const int* __restrict__ tab, int B, int field, int idx) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid * kJdTab + field] <= idx) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct Geom {
  int hs, vs, mcux, mcuy, nY, nC;
};
__device__ __forceinline__ Geom geom(int H, int W, int kind) {
  Geom g;
  g.hs = (kind == K422 || kind == K420) ? 2 : 1;
  g.vs = kind == K420 ? 2 : 1;
  g.mcux = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.nC = g.mcux * g.mcuy;
  g.nY = g.nC * g.hs * g.vs;
  return g;
}

// One 1-D pass of libjpeg's jidctint.c (13-bit constants), before the descale. The host bounds the
// inputs so that nothing here leaves int32 (jpeg_dec.cpp:block_in_bounds).
__device__ __forceinline__ void idct_pass(const int c[8], int o[8]) {
  int z1 = (c[2] + c[6]) * 4433;
  const int t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
  const int t0 = (c[0] + c[4]) * 8192, t1 = (c[0] - c[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446;
  a1 *= 16819;
  a2 *= 25172;
  a3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  o[0] = t10 + a3;
  o[7] = t10 - a3;
  o[1] = t11 + a2;
  o[6] = t11 - a2;
  o[2] = t12 + a1;
  o[5] = t12 - a1;
  o[3] = t13 + a0;
  o[4] = t13 - a0;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ void __launch_bounds__(256) jpeg_idct_kernel(uint8_t* __restrict__ blob, const int* __restrict__ tab, int B,
                                                        int total_blocks, long long blob_bytes) {
  __shared__ int ws[32][8][9];  // [block][row][column], rows padded to 9 words
  const int lb = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const int g = blockIdx.x * 32 + lb;
  const bool live = g < total_blocks;
  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int dst = 0;
  bool store = false;
  if (live) {
    const int* row = tab + find_image(tab, B, JD_BLK0, g) * kJdTab;
    const int bi = g - row[JD_BLK0];
    const Geom gm = geom(row[JD_H], row[JD_W], row[JD_KIND]);
    const int comp = bi < gm.nY ? 0 : 1 + (bi - gm.nY) / gm.nC;
    const int first = comp == 0 ? 0 : gm.nY + (comp - 1) * gm.nC;  // the component's first block
    const int bwc = gm.mcux * (comp == 0 ? gm.hs : 1);
    const int bc = bi - first;
    dst = row[JD_PLANE] + first * 64 + ((bc / bwc) * 8 + lane) * (bwc * 8) + (bc % bwc) * 8;
    store = DV_BOUNDS(dst, 8, blob_bytes, "jpeg_idct plane store");
    const int co = row[JD_COEF] + bi * 128 + lane * 16, qo = row[JD_QT] + comp * 128 + lane * 16;
    if (DV_BOUNDS(co, 16, blob_bytes, "jpeg_idct coefficient load") && DV_BOUNDS(qo, 16, blob_bytes, "jpeg_idct quantizer load")) {
      const uint4 cv = *reinterpret_cast<const uint4*>(blob + co);
      const uint4 qv = *reinterpret_cast<const uint4*>(blob + qo);
      const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[2 * k] = (int)(int16_t)(cw[k] & 0xFFFFu) * (int)(qw[k] & 0xFFFFu);
        c[2 * k + 1] = ((int)cw[k] >> 16) * (int)(qw[k] >> 16);
      }
    }
  }
  int o[8];
  idct_pass(c, o);
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[lb][r][lane] = (o[r] + (1 << 10)) >> 11;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = ws[lb][lane][k];
  idct_pass(c, o);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo |= (uint32_t)clamp255(((o[k] + (1 << 17)) >> 18) + 128) << (8 * k);
    hi |= (uint32_t)clamp255(((o[k + 4] + (1 << 17)) >> 18) + 128) << (8 * k);
  }
  if (live && store) *reinterpret_cast<uint2*>(blob + dst) = make_uint2(lo, hi);
}

// chroma sample for output pixel (x, y) of one plane `p` with row pitch pw: libjpeg's "fancy" (triangle)
// upsampling over the real chroma extent cw x ch, edge-replicated; plain replication when cw <= 2
// (jdsample.c takes the fancy routines only for downsampled_width > 2)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int kind, int x, int y, int cw, int ch) {
  if (kind == K444) return p[y * pw + x];
  const int i = x >> 1;
  if (kind == K422) {
    const uint8_t* r = p + y * pw;
    if (cw <= 2) return r[i];
    if (x & 1) return i == cw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
    return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
  }
  const int rn = y >> 1;
  const uint8_t* near = p + rn * pw;
  if (cw <= 2) return near[i];
  const int rf = (y & 1) ? (rn + 1 < ch ? rn + 1 : ch - 1) : (rn > 0 ? rn - 1 : 0);
  const uint8_t* far = p + rf * pw;
  const int s = 3 * near[i] + far[i];
  if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__global__ void __launch_bounds__(256) jpeg_color_kernel(uint8_t* __restrict__ blob, const int* __restrict__ tab, int B,
                                                         int total_items, long long blob_bytes) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total_items) return;
  const int* row = tab + find_image(tab, B, JD_ITEM0, g) * kJdTab;
  const int it = g - row[JD_ITEM0];
  const int H = row[JD_H], W = row[JD_W], kind = row[JD_KIND];
  const Geom gm = geom(H, W, kind);
  const int w4 = (W + 3) >> 2;
  const int y = it / w4, x0 = (it % w4) * 4;
  const int pwY = gm.mcux * gm.hs * 8, pwC = gm.mcux * 8;
  const int nvalid = W - x0 < 4 ? W - x0 : 4;
  const int yo = row[JD_PLANE] + y * pwY + x0;
  // the planes end at JD_PLANE + 64 (nY + 2 nC): the furthest chroma read is inside its plane by construction
  if (!DV_BOUNDS(yo, 4, blob_bytes, "jpeg_color luma load") ||
      !DV_BOUNDS(row[JD_PLANE], 64 * (gm.nY + (kind == KGREY ? 0 : 2 * gm.nC)), blob_bytes, "jpeg_color planes"))
    return;
  const uint32_t y4 = *reinterpret_cast<const uint32_t*>(blob + yo);
  const uint8_t* cbp = blob + row[JD_PLANE] + gm.nY * 64;
  const uint8_t* crp = cbp + gm.nC * 64;
  const int cw = (W + gm.hs - 1) / gm.hs, ch = (H + gm.vs - 1) / gm.vs;
  uint8_t px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = (int)((y4 >> (8 * j)) & 0xFFu);
    int r = Y, gr = Y, b = Y;
    if (kind != KGREY && j < nvalid) {
      const int cb = chroma_at(cbp, pwC, kind, x0 + j, y, cw, ch) - 128;
      const int cr = chroma_at(crp, pwC, kind, x0 + j, y, cw, ch) - 128;
      r = clamp255(Y + ((91881 * cr + 32768) >> 16));
      gr = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      b = clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
    px[3 * j] = (uint8_t)r;
    px[3 * j + 1] = (uint8_t)gr;
    px[3 * j + 2] = (uint8_t)b;
  }
  const int out = row[JD_RGB] + (y * W + x0) * 3;
  if (!DV_BOUNDS(out, 3 * nvalid, blob_bytes, "jpeg_color rgb store")) return;
  if (nvalid == 4 && (out & 3) == 0) {
    uint32_t* o = reinterpret_cast<uint32_t*>(blob + out);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)  // static indices keep px in registers
      if (k < 3 * nvalid) blob[out + k] = px[k];
  }
}

}  // namespace

int jpeg_dec_launch(uint8_t* blob, long long blob_bytes, const int* table, int B, int total_blocks, int total_items,
                    hipStream_t s) {
  if (B <= 0 || total_blocks <= 0 || total_items <= 0 || blob_bytes <= 0 || blob_bytes > 0x7FFFFFFFLL ||
      (reinterpret_cast<uintptr_t>(blob) & 15) != 0)
    return -1;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((total_blocks + 31) / 32), dim3(256), 0, s, blob, table, B, total_blocks,
                     blob_bytes);
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((total_items + 255) / 256), dim3(256), 0, s, blob, table, B, total_items,
                     blob_bytes);
  return (int)hipGetLastError();
}

}  // namespace dv
