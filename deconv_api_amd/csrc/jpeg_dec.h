// Host-side entropy decoder for the GPU JPEG decode path (jpeg_dec.cpp): markers + Huffman decode of a
// baseline JPEG to quantized DCT coefficients. Dequantize, IDCT, chroma upsampling and colour run on the
// device (jpeg_dec_gpu.hip). Host-only C++ (no torch / HIP), safe to call with the GIL released.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dvjpeg {

enum DecStatus : int { DEC_OK = 0, DEC_UNSUPPORTED = 1 };
// sampling kinds; the numbers are shared with the kernels and ops/jpeg_dec.py
enum DecKind : int { DEC_444 = 0, DEC_422 = 1, DEC_420 = 2, DEC_GREY = 3 };

// Bounds on the dequantized values of one 8x8 block under which the device IDCT's int32 arithmetic is
// exact (derivation: jpeg_dec.cpp:block_in_bounds). A block outside them makes the file "unsupported".
constexpr int64_t kDecColL1Max = 5800;
constexpr int64_t kDecRowBudget = 2000000000LL;

struct DecHeader {
  int H = 0, W = 0;
  int ncomp = 0;           // 1 or 3
  int kind = 0;            // DecKind
  int mcux = 0, mcuy = 0;  // MCUs per row / column
  int hs = 1, vs = 1;      // luma blocks per MCU, horizontally / vertically (chroma: 1 x 1)
  uint16_t qt[3][64];      // quantizer of each component, natural (row-major) order
  // set by jpeg_dec_probe for jpeg_dec_decode
  size_t scan_off = 0;     // first entropy-coded byte
  int restart = 0;         // restart interval in MCUs (0: none)
  int dc_tab[3], ac_tab[3];
  // Huffman tables as read from DHT: [class 0 DC / 1 AC][id]
  uint8_t bits[2][4][17];
  uint8_t vals[2][4][256];
  bool have[2][4];
};

// Number of blocks of component c, padded to whole MCUs, and of all components
inline long long dec_comp_blocks(const DecHeader& h, int c) {
  return (long long)h.mcux * h.mcuy * (c == 0 ? h.hs * h.vs : 1);
}
inline long long dec_total_blocks(const DecHeader& h) {
  return dec_comp_blocks(h, 0) + (h.ncomp == 3 ? 2 * dec_comp_blocks(h, 1) : 0);
}

// Parse every marker up to the scan. DEC_OK: `h` is filled and the file is inside the accepted subset as
// far as the headers tell (SOF0, 8 bit, one interleaved Huffman scan, YCbCr 4:4:4 / 4:2:2 / 4:2:0 or one
// component, no Exif orientation other than 1, H * W <= max_pixels). Anything else: DEC_UNSUPPORTED.
int jpeg_dec_probe(const uint8_t* data, size_t n, long long max_pixels, DecHeader& h);

// Huffman-decode the scan into `coef`: dec_total_blocks(h) * 64 int16, which the caller has ZEROED.
// Component-major (Y, then Cb, then Cr), each component bh x bw blocks in raster order, each block 64
// values in COLUMN-major order (index col * 8 + row), so that one column is one aligned 16-byte load.
// DEC_UNSUPPORTED on any stream error, truncation, restart-marker or trailing anomaly, or a block outside
// the exactness bound. Never reads outside [data, data + n) and never writes outside
// [coef, coef + 64 * dec_total_blocks(h)).
int jpeg_dec_decode(const uint8_t* data, size_t n, const DecHeader& h, int16_t* coef);

}  // namespace dvjpeg
