// Guided DeepDream loss (engine/deepdream.py, ops/autograd.py:guide_core / guide_tap): every core
// position p of a loss layer's activation a [N, H, W, C] is matched against the Q feature vectors of
// its image's guide y [G, Q, C] (guide gidx[n]):
//   s[p][q] = sum_c a[p][c] * y[q][c]  (fp32),  q*[p] = argmax_q s[p][q]  (lowest q on ties)
//   loss partial = sum_p s[p][q*]      gx[p] = addend[p] + scale[n] * y[q*] * (a[p] > 0 | 1)
// and gx = addend (or 0) on the border. The scores never leave registers.
//
// Layout. A block owns 16 core positions at a time and computes their score tile TRANSPOSED, S^T = Y X^T,
// with mfma_f32_16x16x32: the A operand is 16 guide rows (lane l: row l & 15, channels 8 (l >> 4) .. + 7 of
// the 32-channel step), the B operand the 16 positions (lane l: position l & 15, same channels), both one
// 16-B global load per lane with no staging. The C/D map then puts the position on lane & 15 and guide row
// (lane >> 4) * 4 + reg on the registers, so each lane keeps a running (max, q) for ITS position over the
// guide rows it sees, in ascending q with a strict >. The block's four waves take the 64-row passes over the
// guide round-robin (four 16-row tiles share every activation fragment), which quarters the chain of dependent
// loads a position waits for. The combine crosses the four lane groups with two xor shuffles and the four
// waves through 128 B of LDS: larger max wins, a tie goes to the lower q. The block then gathers the winning
// rows, 16 B per thread, and applies scale, mask and addend in one fp32 expression.
//
// Bounds: guide rows q >= Q are loaded from row Q - 1 (a valid address) and never compared; the
// positions of a tail tile load position Pc - 1 and store nothing; gidx is clamped to [0, G).
// Deterministic: block (p, n) of the (parts, N) grid writes part[n][p], no atomics.
#include "common.h"
#include "kernels.h"

namespace dv {

template <int DT>
__device__ __forceinline__ typename Vec8<DT>::type ld_frag(const uint16_t* p) {
  return __builtin_bit_cast(typename Vec8<DT>::type, *reinterpret_cast<const uint4*>(p));
}

template <int DT>
__global__ void __launch_bounds__(256) guide_match_kernel(const uint16_t* __restrict__ a,
                                                          const uint16_t* __restrict__ y,
                                                          const int* __restrict__ gidx,
                                                          const float* __restrict__ scale,
                                                          const uint16_t* __restrict__ addend,
                                                          uint16_t* __restrict__ gx, float* __restrict__ part, int H,
                                                          int W, int C, int Q, int G, int b, int mask) {
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int cpp = C >> 3;
  const int Hc = H - 2 * b, Wc = W - 2 * b, Pc = Hc * Wc;
  const long long base = (long long)n * H * W * C;
  const uint16_t* an = a + base;
  const int g = min(max(gidx[n], 0), G - 1);
  const uint16_t* yg = y + (long long)g * Q * C;

  if (gx) {  // the border: gx = addend (or 0)
    const int total = H * W * cpp;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
      const int pix = t / cpp;
      const int ww = pix % W, hh = pix / W;
      if (hh >= b && hh < H - b && ww >= b && ww < W - b) continue;
      const long long o = base + (long long)t * 8;
      *reinterpret_cast<uint4*>(gx + o) = addend ? *reinterpret_cast<const uint4*>(addend + o) : uint4{0u, 0u, 0u, 0u};
    }
  }

  const float sc = gx ? scale[n] : 0.f;
  float loss = 0.f;
  const int ntile = (Pc + 15) >> 4;
  __shared__ float s_best[4][16];
  __shared__ int s_bq[4][16];
  __shared__ int s_win[16];
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {  // (block-uniform: barriers inside)
    const int pc = tile * 16 + col;
    const bool valid = pc < Pc;
    const int pcl = valid ? pc : Pc - 1;
    const uint16_t* xrow = an + ((long long)(pcl / Wc + b) * W + (pcl % Wc + b)) * C + grp * 8;
    float best = -INFINITY;
    int bq = 0;
    for (int q0 = wave * 64; q0 < Q; q0 += 256) {  // this wave's 64-row passes, ascending
      f32x4 acc[4];
      const uint16_t* yrow[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        yrow[t] = yg + (long long)min(q0 + t * 16 + col, Q - 1) * C + grp * 8;
      }
      // two 32-channel steps per trip: ten 16-B loads in flight ahead of eight MFMAs (the loop is latency-bound)
      int c0 = 0;
      for (; c0 + 64 <= C; c0 += 64) {
        const typename Vec8<DT>::type xb0 = ld_frag<DT>(xrow + c0), xb1 = ld_frag<DT>(xrow + c0 + 32);
        typename Vec8<DT>::type yb0[4], yb1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {  // (rows >= Q: row Q - 1, never compared)
          yb0[t] = ld_frag<DT>(yrow[t] + c0);
          yb1[t] = ld_frag<DT>(yrow[t] + c0 + 32);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mfma16x16x32<DT>(yb0[t], xb0, acc[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mfma16x16x32<DT>(yb1[t], xb1, acc[t]);
      }
      if (c0 < C) {  // C / 32 odd
        const typename Vec8<DT>::type xb = ld_frag<DT>(xrow + c0);
        typename Vec8<DT>::type yb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) yb[t] = ld_frag<DT>(yrow[t] + c0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mfma16x16x32<DT>(yb[t], xb, acc[t]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + t * 16 + grp * 4 + r;
          const float s = acc[t][r];
          if (q < Q && s > best) {
            best = s;
            bq = q;
          }
        }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {  // the four lane groups of a position
      const float ob = __shfl_xor(best, o, 64);
      const int oq = __shfl_xor(bq, o, 64);
      if (ob > best || (ob == best && oq < bq)) {
        best = ob;
        bq = oq;
      }
    }
    if (grp == 0) {
      s_best[wave][col] = best;
      s_bq[wave][col] = bq;
    }
    __syncthreads();
    if (threadIdx.x < 16) {  // the four waves' candidates of position `col`
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float ob = s_best[w][col];
        const int oq = s_bq[w][col];
        if (ob > best || (ob == best && oq < bq)) {
          best = ob;
          bq = oq;
        }
      }
      s_win[col] = bq;
      if (valid) loss += best;
    }
    __syncthreads();
    if (gx) {
      // 16 positions x cpp 16-B chunks over the block's 256 threads
      for (int i = threadIdx.x; i < 16 * cpp; i += 256) {
        const int pos = i / cpp, ch = i - pos * cpp;
        const int p2 = tile * 16 + pos;
        if (p2 >= Pc) continue;
        const int q = s_win[pos];
        const long long o = ((long long)(p2 / Wc + b) * W + (p2 % Wc + b)) * C + ch * 8;
        const uint4 yv = *reinterpret_cast<const uint4*>(yg + (long long)q * C + ch * 8);
        const uint4 av = mask ? *reinterpret_cast<const uint4*>(an + o) : uint4{0u, 0u, 0u, 0u};
        const uint4 dd = addend ? *reinterpret_cast<const uint4*>(addend + base + o) : uint4{0u, 0u, 0u, 0u};
        const uint32_t yi[4] = {yv.x, yv.y, yv.z, yv.w}, ai[4] = {av.x, av.y, av.z, av.w};
        const uint32_t di[4] = {dd.x, dd.y, dd.z, dd.w};
        uint32_t oi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dlo = to_f<DT>(di[e] & 0xFFFFu), dhi = to_f<DT>(di[e] >> 16);
          const bool mlo = !mask || to_f<DT>(ai[e] & 0xFFFFu) > 0.f, mhi = !mask || to_f<DT>(ai[e] >> 16) > 0.f;
          oi[e] = pack2<DT>(mlo ? dlo + sc * to_f<DT>(yi[e] & 0xFFFFu) : dlo,
                            mhi ? dhi + sc * to_f<DT>(yi[e] >> 16) : dhi);
        }
        *reinterpret_cast<uint4*>(gx + base + o) = uint4{oi[0], oi[1], oi[2], oi[3]};
      }
    }
  }
  if (part) {  // (only wave 0's first 16 lanes hold a loss)
    loss = wave_sum(loss);
    if (threadIdx.x == 0) part[(long long)n * gridDim.x + blockIdx.x] = loss;
  }
}

int guide_match_launch(const uint16_t* a, const uint16_t* y, const int* gidx, const float* scale,
                       const uint16_t* addend, uint16_t* gx, float* part, int parts, int N, int H, int W, int C, int Q,
                       int G, int b, int mask, int dtype, hipStream_t s) {
  if (C % 32 != 0 || b < 0 || H <= 2 * b || W <= 2 * b || parts < 1 || parts > GUIDE_MAX_PARTS || Q < 1 || G < 1 ||
      N < 1 || N > 65535 || (long long)H * W * (C / 8) > 0x7FFFFFFFLL || (!gx && !part))
    return -1;
  const dim3 grid((unsigned)parts, (unsigned)N);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(guide_match_kernel<DT_F16>, grid, dim3(256), 0, s, a, y, gidx, scale, addend, gx, part, H, W, C,
                       Q, G, b, mask);
  else
    hipLaunchKernelGGL(guide_match_kernel<DT_BF16>, grid, dim3(256), 0, s, a, y, gidx, scale, addend, gx, part, H, W, C,
                       Q, G, b, mask);
  return (int)hipGetLastError();
}

}  // namespace dv
