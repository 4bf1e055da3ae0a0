// Stand-alone stress of the host JPEG entropy decoder (deconv_api_amd/csrc/jpeg_dec.cpp), built with
// AddressSanitizer + UBSan by tests/test_jpeg_dec_sanitize.py. The parser faces untrusted HTTP input: for
// every truncation of a stream and for thousands of fixed-seed byte mutations it must answer "ok" or
// "unsupported" and touch nothing outside the two buffers it was given. Both buffers are heap blocks of
// exactly the promised size, so the sanitizer's red zones catch one byte too many in either direction.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "jpeg_dec.h"
#include "jpeg_enc.h"

namespace {

constexpr long long kMaxPixels = 1 << 16;  // mutated SOF sizes stay small
long long g_ok = 0, g_unsupported = 0;

// 0 ok / 1 unsupported, on exact-size copies
int run(const uint8_t* data, size_t n) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  std::memcpy(in.get(), data, n);
  dvjpeg::DecHeader h;
  int rc = dvjpeg::jpeg_dec_probe(in.get(), n, kMaxPixels, h);
  if (rc == dvjpeg::DEC_OK) {
    const size_t elems = (size_t)dvjpeg::dec_total_blocks(h) * 64;
    std::unique_ptr<int16_t[]> coef(new int16_t[elems]());
    rc = dvjpeg::jpeg_dec_decode(in.get(), n, h, coef.get());
  }
  if (rc != dvjpeg::DEC_OK && rc != dvjpeg::DEC_UNSUPPORTED) {
    std::printf("unexpected status %d\n", rc);
    std::exit(2);
  }
  (rc == dvjpeg::DEC_OK ? g_ok : g_unsupported)++;
  return rc;
}

std::vector<uint8_t> picture(int H, int W, uint32_t seed) {
  std::vector<uint8_t> px((size_t)H * W * 3);
  uint32_t s = seed;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) {
        s = s * 1664525u + 1013904223u;
        px[((size_t)y * W + x) * 3 + c] = (uint8_t)((x * 5 + y * 3 + c * 40 + ((s >> 24) & 31)) & 255);
      }
  return px;
}

}  // namespace

int main() {
  struct Case {
    int H, W, q, segments;
  };
  const Case cases[] = {{16, 16, 90, 1}, {33, 47, 75, 1}, {40, 24, 95, 3}, {9, 31, 30, 1}};
  std::vector<std::string> streams;
  for (const Case& c : cases) {
    const std::vector<uint8_t> px = picture(c.H, c.W, (uint32_t)(c.H * 131 + c.W));
    streams.push_back(dvjpeg::encode_jpeg(px.data(), c.H, c.W, c.q, c.segments));
    if (run(reinterpret_cast<const uint8_t*>(streams.back().data()), streams.back().size()) != dvjpeg::DEC_OK) {
      std::printf("the project's own encoder output was not accepted (%dx%d)\n", c.H, c.W);
      return 1;
    }
  }
  // every truncation of one stream (the one with restart markers)
  const std::string& t = streams[2];
  for (size_t n = 0; n < t.size(); ++n) {
    if (run(reinterpret_cast<const uint8_t*>(t.data()), n) == dvjpeg::DEC_OK) {
      std::printf("a truncated stream (%zu of %zu bytes) was accepted\n", n, t.size());
      return 1;
    }
  }
  // fixed-seed mutations: 1..4 bytes overwritten, inserted or deleted, biased towards the headers
  uint32_t s = 12345;
  auto rnd = [&s]() { return (s = s * 1664525u + 1013904223u) >> 8; };
  for (int it = 0; it < 6000; ++it) {
    std::string m = streams[it % streams.size()];
    const int edits = 1 + (int)(rnd() % 4);
    for (int e = 0; e < edits && !m.empty(); ++e) {
      const size_t span = (rnd() & 1) ? std::min<size_t>(m.size(), 700) : m.size();
      const size_t at = rnd() % span;
      switch (rnd() % 4) {
        case 0: m[at] = (char)rnd(); break;
        case 1: m[at] = (char)0xFF; break;
        case 2: m.insert(m.begin() + (long)at, (char)rnd()); break;
        default: m.erase(m.begin() + (long)at); break;
      }
    }
    run(reinterpret_cast<const uint8_t*>(m.data()), m.size());
  }
  std::printf("ok=%lld unsupported=%lld\n", g_ok, g_unsupported);
  return 0;
}
