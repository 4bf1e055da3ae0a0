// Host entropy decoder of the GPU JPEG decode path: the serial part of a baseline JPEG decode (markers,
// Huffman) -> quantized DCT coefficients; everything after it runs on the device (jpeg_dec_gpu.hip).
//
// The parser faces untrusted HTTP input. Its rule is: accept only what it understands completely, and
// report everything else as DEC_UNSUPPORTED so that the caller hands the file to PIL, which then decides
// the response exactly as before. libjpeg tolerates many damaged streams (it warns and goes on); this
// parser tolerates none, because the accepted files must decode bit-identically to libjpeg.
#include "jpeg_dec.h"

#include <cstring>

namespace dvjpeg {
namespace {

// zig-zag index -> natural (row-major) index
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// ---- Exif: the orientation of IFD0, when the segment parses completely -------------------------------
// returns 0: parsed, no orientation tag; > 0: the orientation; < 0: not understood
int exif_orientation(const uint8_t* p, size_t n) {
  if (n < 8) return -1;
  bool le;
  if (p[0] == 'I' && p[1] == 'I') le = true;
  else if (p[0] == 'M' && p[1] == 'M') le = false;
  else return -1;
  auto u16 = [&](size_t o) -> uint32_t { return le ? (uint32_t)(p[o] | (p[o + 1] << 8)) : (uint32_t)((p[o] << 8) | p[o + 1]); };
  auto u32 = [&](size_t o) -> uint32_t {
    return le ? (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24)
              : ((uint32_t)p[o] << 24) | ((uint32_t)p[o + 1] << 16) | ((uint32_t)p[o + 2] << 8) | (uint32_t)p[o + 3];
  };
  if (u16(2) != 42) return -1;
  const size_t ifd = u32(4);
  if (ifd > n || n - ifd < 2) return -1;
  const size_t cnt = u16(ifd);
  if ((n - ifd - 2) / 12 < cnt) return -1;
  int found = 0;
  for (size_t i = 0; i < cnt; ++i) {
    const size_t e = ifd + 2 + 12 * i;
    if (u16(e) != 0x0112) continue;
    if (u16(e + 2) != 3 || u32(e + 4) != 1) return -1;  // SHORT, one value
    const int v = (int)u16(e + 8);
    if (v < 1 || v > 8 || found) return -1;
    found = v;
  }
  return found;
}

// ---- Huffman decoding tables ------------------------------------------------------------------------
constexpr int kLook = 9;
struct HuffTab {
  // lut[next kLook bits] = (code length << 8) | symbol, 0 when the code is longer than kLook bits
  uint16_t lut[1 << kLook];
  int32_t maxcode[18];  // largest code of each length (-1: none); [17] = sentinel that always ends the search
  int32_t valoff[17];   // index into vals of the first symbol of a length, minus its first code
  uint8_t vals[256];
  // AC tables: fast[next kFast bits] = (value << 8) | (run << 4) | (code + magnitude bits), when both fit
  // in kFast bits (most coefficients of a photograph); 0 otherwise
  int16_t fast[1 << 10];
};
constexpr int kFast = 10;

// false: the counts do not describe a prefix code (libjpeg refuses such tables, too)
bool build_table(const uint8_t* bits, const uint8_t* vals, bool dc, HuffTab& t) {
  int total = 0;
  for (int l = 1; l <= 16; ++l) total += bits[l];
  if (total > 256) return false;
  std::memset(t.lut, 0, sizeof(t.lut));
  std::memcpy(t.vals, vals, 256);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t.valoff[l] = k - code;
    for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
      if (code >= (1 << l)) return false;
      if (dc && vals[k] > 15) return false;
      if (l <= kLook) {
        const int first = code << (kLook - l);
        for (int j = 0; j < (1 << (kLook - l)); ++j) t.lut[first + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    t.maxcode[l] = bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
  std::memset(t.fast, 0, sizeof(t.fast));
  if (!dc) {
    for (int i = 0; i < (1 << kFast); ++i) {
      const uint32_t e = t.lut[i >> (kFast - kLook)];
      const int len = (int)(e >> 8), run = (int)(e & 0xFF) >> 4, mag = (int)(e & 15);
      if (e == 0 || mag == 0 || len + mag > kFast) continue;
      int v = (i >> (kFast - len - mag)) & ((1 << mag) - 1);
      if (v < (1 << (mag - 1))) v += 1 - (1 << mag);
      if (v >= -128 && v <= 127) t.fast[i] = (int16_t)(v * 256 + run * 16 + len + mag);
    }
  }
  return true;
}

// ---- bit reader -------------------------------------------------------------------------------------
// Bits are the low `n` bits of `acc`. Past a marker (or the end of the data) the reader feeds zero bits
// and counts them in `fake`; a decode that consumed any of them ran past the segment's data.
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int n = 0;
  int fake = 0;
  bool stopped = false;  // at a marker (p points at its 0xFF) or at the end of the data

  inline void fill() {
    if (n <= 32 && !stopped && end - p >= 4) {  // four plain bytes at once
      const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
      // a byte of w is 0xFF iff the same byte of ~w is zero
      const uint32_t x = ~w;
      if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {
        acc = (acc << 32) | w;
        n += 32;
        p += 4;
      }
    }
    while (n <= 56) {
      uint32_t b = 0;
      if (!stopped) {
        if (p >= end) {
          stopped = true;
        } else if (*p != 0xFF) {
          b = *p++;
        } else if (p + 1 < end && p[1] == 0) {
          b = 0xFF;
          p += 2;
        } else {
          stopped = true;
        }
      }
      if (stopped) fake += 8;
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline uint32_t peek(int k) const { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1u); }
  inline void skip(int k) { n -= k; }
  inline bool overrun() const { return n < fake; }
  // real bits still buffered
  inline int left() const { return n - fake; }
  void reset() {
    acc = 0;
    n = 0;
    fake = 0;
    stopped = false;
  }
};

// next symbol, or -1 for a code no symbol has; needs 16 buffered bits
inline int decode_sym(Bits& b, const HuffTab& t) {
  const uint32_t e = t.lut[b.peek(kLook)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 0xFF);
  }
  int l = kLook + 1;
  int32_t code = (int32_t)b.peek(l);
  while (code > t.maxcode[l]) {
    ++l;
    if (l > 16) return -1;
    code = (int32_t)b.peek(l);
  }
  b.skip(l);
  return t.vals[(code + t.valoff[l]) & 0xFF];
}

inline int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// Exactness bound of the device IDCT (jpeg_dec_gpu.hip: libjpeg's "islow" in int32).
//
// Every intermediate of one 1-D pass is an integer combination sum_k a_k x_k of the pass's eight inputs.
// Summing the absolute constants along the data flow bounds |a_k| for EVERY intermediate, whatever the
// evaluation order, by kA[k] = {8192, 32501, 10703, 71869, 8192, 50643, 19570, 35521} (e.g. input 3:
// 25172 + 20995 + 16069 + 9633). The pass OUTPUTS have the much smaller true weights 8192 * sqrt(2) *
// cos(.) <= 11363 (< kW = 11400; ops/jpeg_dec.py:idct_gain measures them).
//   pass 1, column c with L1 norm S_c = sum_r |x[r][c]|: intermediates <= 71869 S_c + 2^10, outputs
//     |ws[r][c]| <= (kW S_c + 2^10) >> 11 <= kW S_c / 2048 + 1.
//   pass 2, any row r: intermediates <= sum_c kA[c] |ws[r][c]| + 2^17.
// With S_c <= kDecColL1Max = 5800 pass 1 stays below 4.2e8, and with sum_c kA[c] (kW S_c / 2048 + 2) <=
// kDecRowBudget = 2e9 pass 2 stays below 2^31: within both, the kernel's int32 arithmetic is exact.
//
// The oracle, libjpeg-turbo's x86 SIMD IDCT, is narrower than int32 in three places, and an accepted block
// must be exact there too:
//   * the dequantized values are 16-bit products, and each pass forms in0 +- in4, in7 + in3 and in5 + in1
//     with 16-bit adds. Pass 1: |x[0][c]| + |x[4][c]| etc. <= S_c <= 5800. Pass 2 works on the rows of ws,
//     so the PAIRS of column bounds must fit: (kW S_0 / 2048 + 2) + (kW S_4 / 2048 + 2) <= 32767, and the
//     same for columns (7, 3) and (5, 1);
//   * pass 1's outputs are packed to int16: |ws| <= kW 5800 / 2048 + 1 = 32287 (columns 2 and 6, which are
//     in no pair, need only this).
// Its 32-bit sums combine the same constants into fewer products, so kA bounds them as well. Its final
// packs saturate, i.e. clamp, as the kernel does. (libjpeg's C code masks its range-limit index instead of
// clamping; it agrees wherever the output is within a few hundred of 0..255, which is not checked here: the
// oracle is the SIMD build.) Real images sit far inside (a full-contrast noise block has S_0 ~ 1900 and
// S_c ~ 800, a row budget of ~1.1e9); a file with a block outside goes to PIL.
const int64_t kA[8] = {8192, 32501, 10703, 71869, 8192, 50643, 19570, 35521};
constexpr int64_t kW = 11400;
inline bool block_in_bounds(const int64_t* colsum) {
  int64_t budget = 0, ws[8];
  for (int c = 0; c < 8; ++c) {
    if (colsum[c] > kDecColL1Max) return false;
    ws[c] = kW * colsum[c] / 2048 + 2;
    budget += kA[c] * ws[c];
  }
  if (ws[0] + ws[4] > 32767 || ws[7] + ws[3] > 32767 || ws[5] + ws[1] > 32767) return false;
  return budget <= kDecRowBudget;
}

}  // namespace

int jpeg_dec_probe(const uint8_t* data, size_t n, long long max_pixels, DecHeader& h) {
  if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return DEC_UNSUPPORTED;
  std::memset(h.have, 0, sizeof(h.have));
  uint16_t qtab[4][64];
  bool have_q[4] = {false, false, false, false};
  bool sof = false, jfif = false, adobe = false, other_app1 = false;
  int adobe_transform = -1, orientation = 0 /* 0: no Exif orientation seen */;
  int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
  h.restart = 0;
  size_t p = 2;
  for (;;) {
    if (n - p < 4 || data[p] != 0xFF) return DEC_UNSUPPORTED;
    const int m = data[p + 1];
    if (m == 0xFF) {  // fill byte
      ++p;
      continue;
    }
    const size_t len = (size_t)be16(data + p + 2);
    if (len < 2 || len > n - p - 2) return DEC_UNSUPPORTED;
    const uint8_t* s = data + p + 4;
    const size_t sl = len - 2;
    p += 2 + len;
    if (m == 0xC0) {  // SOF0
      if (sof || sl < 6) return DEC_UNSUPPORTED;
      const int prec = s[0], nc = s[5];
      h.H = be16(s + 1);
      h.W = be16(s + 3);
      if (prec != 8 || h.H < 1 || h.W < 1 || (nc != 1 && nc != 3) || sl != (size_t)(6 + 3 * nc)) return DEC_UNSUPPORTED;
      if ((long long)h.H * h.W > max_pixels) return DEC_UNSUPPORTED;
      h.ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        cid[c] = s[6 + 3 * c];
        ch[c] = s[7 + 3 * c] >> 4;
        cv[c] = s[7 + 3 * c] & 15;
        ctq[c] = s[8 + 3 * c];
        if (ctq[c] > 3) return DEC_UNSUPPORTED;
      }
      sof = true;
    } else if (m == 0xC4) {  // DHT
      size_t o = 0;
      while (o < sl) {
        if (sl - o < 17) return DEC_UNSUPPORTED;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return DEC_UNSUPPORTED;
        int total = 0;
        h.bits[tc][th][0] = 0;
        for (int l = 1; l <= 16; ++l) total += (h.bits[tc][th][l] = s[o + l]);
        if (total > 256 || sl - o - 17 < (size_t)total) return DEC_UNSUPPORTED;
        std::memset(h.vals[tc][th], 0, 256);
        std::memcpy(h.vals[tc][th], s + o + 17, (size_t)total);
        h.have[tc][th] = true;
        o += 17 + (size_t)total;
      }
    } else if (m == 0xDB) {  // DQT
      size_t o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3) return DEC_UNSUPPORTED;
        const size_t need = pq ? 128 : 64;
        if (sl - o - 1 < need) return DEC_UNSUPPORTED;
        for (int k = 0; k < 64; ++k) {
          const int q = pq ? be16(s + o + 1 + 2 * k) : s[o + 1 + k];
          if (q == 0) return DEC_UNSUPPORTED;
          qtab[tq][kNatural[k]] = (uint16_t)q;
        }
        have_q[tq] = true;
        o += 1 + need;
      }
    } else if (m == 0xDD) {  // DRI
      if (sl != 2) return DEC_UNSUPPORTED;
      h.restart = be16(s);
    } else if (m == 0xE0) {
      // libjpeg honours a JFIF APP0 only with its 14 fixed bytes (and PIL cannot open a shorter one)
      if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) {
        if (sl < 14) return DEC_UNSUPPORTED;
        jfif = true;
      }
    } else if (m == 0xE1) {
      if (sl >= 6 && std::memcmp(s, "Exif\0\0", 6) == 0) {
        const int o = exif_orientation(s + 6, sl - 6);
        if (o < 0 || (o > 0 && orientation > 0)) return DEC_UNSUPPORTED;
        if (o > 0) orientation = o;
      } else {
        other_app1 = true;  // XMP may carry an orientation of its own
      }
    } else if (m == 0xEE) {
      if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if ((m >= 0xE2 && m <= 0xEF) || m == 0xFE) {
      // other application segments and comments carry nothing the pixels depend on
    } else if (m == 0xDA) {  // SOS
      if (!sof || sl != (size_t)(4 + 2 * h.ncomp) || s[0] != h.ncomp) return DEC_UNSUPPORTED;
      for (int c = 0; c < h.ncomp; ++c) {
        if (s[1 + 2 * c] != cid[c]) return DEC_UNSUPPORTED;
        h.dc_tab[c] = s[2 + 2 * c] >> 4;
        h.ac_tab[c] = s[2 + 2 * c] & 15;
        if (h.dc_tab[c] > 3 || h.ac_tab[c] > 3 || !h.have[0][h.dc_tab[c]] || !h.have[1][h.ac_tab[c]]) return DEC_UNSUPPORTED;
      }
      const uint8_t* t = s + 1 + 2 * h.ncomp;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return DEC_UNSUPPORTED;
      h.scan_off = p;
      break;
    } else {
      return DEC_UNSUPPORTED;  // progressive / arithmetic / lossless frames, DNL, DAC, anything else
    }
  }
  // orientation must be provably 1: an Exif tag saying so, or no Exif tag and no other APP1 (XMP)
  if (orientation > 1 || (orientation == 0 && other_app1)) return DEC_UNSUPPORTED;
  if (h.ncomp == 3) {
    if (!(jfif || (cid[0] == 1 && cid[1] == 2 && cid[2] == 3))) return DEC_UNSUPPORTED;
    if (adobe && adobe_transform != 1) return DEC_UNSUPPORTED;
    if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return DEC_UNSUPPORTED;
    if (ch[0] == 1 && cv[0] == 1) h.kind = DEC_444;
    else if (ch[0] == 2 && cv[0] == 1) h.kind = DEC_422;
    else if (ch[0] == 2 && cv[0] == 2) h.kind = DEC_420;
    else return DEC_UNSUPPORTED;
  } else {
    if (ch[0] != 1 || cv[0] != 1) return DEC_UNSUPPORTED;
    h.kind = DEC_GREY;
  }
  h.hs = ch[0];
  h.vs = cv[0];
  h.mcux = (h.W + 8 * h.hs - 1) / (8 * h.hs);
  h.mcuy = (h.H + 8 * h.vs - 1) / (8 * h.vs);
  for (int c = 0; c < h.ncomp; ++c) {
    if (!have_q[ctq[c]]) return DEC_UNSUPPORTED;
    std::memcpy(h.qt[c], qtab[ctq[c]], sizeof(h.qt[c]));
  }
  return DEC_OK;
}

int jpeg_dec_decode(const uint8_t* data, size_t n, const DecHeader& h, int16_t* coef) {
  if (h.scan_off > n || h.ncomp < 1 || h.ncomp > 3) return DEC_UNSUPPORTED;
  HuffTab dc[3], ac[3];
  for (int c = 0; c < h.ncomp; ++c) {
    if (!build_table(h.bits[0][h.dc_tab[c]], h.vals[0][h.dc_tab[c]], true, dc[c])) return DEC_UNSUPPORTED;
    if (!build_table(h.bits[1][h.ac_tab[c]], h.vals[1][h.ac_tab[c]], false, ac[c])) return DEC_UNSUPPORTED;
  }
  // zig-zag index -> position in the column-major block, and its column
  uint8_t pos[64];
  for (int k = 0; k < 64; ++k) pos[k] = (uint8_t)((kNatural[k] & 7) * 8 + (kNatural[k] >> 3));
  int16_t* base[3];
  int bw[3];
  {
    long long o = 0;
    for (int c = 0; c < h.ncomp; ++c) {
      base[c] = coef + o * 64;
      bw[c] = h.mcux * (c == 0 ? h.hs : 1);
      o += dec_comp_blocks(h, c);
    }
  }
  Bits b;
  b.p = data + h.scan_off;
  b.end = data + n;
  int pred[3] = {0, 0, 0};
  const long long nmcu = (long long)h.mcux * h.mcuy;
  long long until_restart = h.restart ? h.restart : nmcu;
  int next_rst = 0;
  long long mcu = 0;
  for (int my = 0; my < h.mcuy; ++my) {
    for (int mx = 0; mx < h.mcux; ++mx, ++mcu) {
      if (until_restart == 0) {
        // the interval's data must end inside the current byte, followed by the expected RSTn
        if (b.overrun() || !b.stopped || b.left() >= 8) return DEC_UNSUPPORTED;
        const uint8_t* q = b.p;
        while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
        if (b.end - q < 2 || q[0] != 0xFF || q[1] != 0xD0 + next_rst) return DEC_UNSUPPORTED;
        b.p = q + 2;
        b.reset();
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        until_restart = h.restart;
      }
      --until_restart;
      for (int c = 0; c < h.ncomp; ++c) {
        const int nh = c == 0 ? h.hs : 1, nv = c == 0 ? h.vs : 1;
        const uint16_t* q = h.qt[c];
        for (int v = 0; v < nv; ++v) {
          for (int u = 0; u < nh; ++u) {
            int16_t* blk = base[c] + ((long long)(my * nv + v) * bw[c] + (mx * nh + u)) * 64;
            int64_t colsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            b.fill();
            int s = decode_sym(b, dc[c]);
            if (s < 0) return DEC_UNSUPPORTED;
            int diff = 0;
            if (s) {
              diff = extend(b.peek(s), s);
              b.skip(s);
            }
            pred[c] += diff;
            if (pred[c] < -32768 || pred[c] > 32767) return DEC_UNSUPPORTED;
            blk[0] = (int16_t)pred[c];
            colsum[0] = (int64_t)(pred[c] < 0 ? -pred[c] : pred[c]) * q[0];
            for (int k = 1; k < 64; ++k) {
              b.fill();
              const int f = ac[c].fast[b.peek(kFast)];
              if (f) {
                k += (f >> 4) & 15;
                if (k > 63) return DEC_UNSUPPORTED;
                b.skip(f & 15);
                const int val = f >> 8;
                blk[pos[k]] = (int16_t)val;
                colsum[pos[k] >> 3] += (int64_t)(val < 0 ? -val : val) * q[kNatural[k]];
                continue;
              }
              const int rs = decode_sym(b, ac[c]);
              if (rs < 0) return DEC_UNSUPPORTED;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;  // end of block
                k += 15;
                if (k > 63) return DEC_UNSUPPORTED;
                continue;
              }
              k += r;
              if (k > 63) return DEC_UNSUPPORTED;
              const int val = extend(b.peek(s), s);
              b.skip(s);
              blk[pos[k]] = (int16_t)val;  // |val| < 2^15: s <= 15
              colsum[pos[k] >> 3] += (int64_t)(val < 0 ? -val : val) * q[kNatural[k]];
            }
            if (b.overrun() || !block_in_bounds(colsum)) return DEC_UNSUPPORTED;
          }
        }
      }
    }
  }
  // after the last MCU: the rest of the current byte, EOI, and nothing behind it
  if (b.overrun() || !b.stopped || b.left() >= 8) return DEC_UNSUPPORTED;
  const uint8_t* q = b.p;
  while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
  if (b.end - q != 2 || q[0] != 0xFF || q[1] != 0xD9) return DEC_UNSUPPORTED;
  return DEC_OK;
}

}  // namespace dvjpeg
