"""Host cost of the two JPEG decode paths, per image, on the http_load corpus (no GPU needed).

    python tools/jpeg_decode_bench.py [--images 64] [--rounds 5] [--threads N]

  (a) PIL full decode: ``decode_image`` (what a front end does per request today);
  (b) native parse to coefficients: ``parse_jpeg_coeffs`` (what it does with DV_GPU_JPEG_DECODE=1; the
      IDCT, upsampling and colour conversion then run on the GPU).

Both are timed on one thread and on ``codec_workers`` threads (both release the GIL), as wall time
per image (threads: wall time of the whole corpus / images, i.e. the inverse throughput). The two
arms alternate within every round; the table reports the median and the minimum over rounds.
"""
from __future__ import annotations

import argparse
import base64
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=None, help="default: Config.codec_workers")
    a = ap.parse_args(argv)
    from http_load import corpus

    from deconv_api_amd.codec import decode_image, parse_jpeg_coeffs
    from deconv_api_amd.config import Config

    threads = a.threads or Config.from_env().codec_workers
    files = [base64.b64decode(u.split(",", 1)[1]) for u, _ in corpus(a.images, png_every=0)]
    parsed = [parse_jpeg_coeffs(f) for f in files]
    accepted = sum(p is not None for p in parsed)
    px = sum(p.H * p.W for p in parsed if p is not None)
    arms = {"pil_full_decode": decode_image, "native_parse_coeffs": parse_jpeg_coeffs}
    res = {(k, t): [] for k in arms for t in (1, threads)}
    with ThreadPoolExecutor(threads) as ex:
        for fn in arms.values():  # warm-up
            list(map(fn, files))
        for _ in range(a.rounds):
            for name, fn in arms.items():
                t0 = time.perf_counter()
                for f in files:
                    fn(f)
                res[(name, 1)].append((time.perf_counter() - t0) / len(files))
                t0 = time.perf_counter()
                list(ex.map(fn, files))
                res[(name, threads)].append((time.perf_counter() - t0) / len(files))
    print(f"corpus: {len(files)} JPEGs of tools/http_load.py:corpus(png_every=0), {sum(map(len, files)) / len(files) / 1e3:.1f} KB "
          f"and {px / max(accepted, 1) / 1e3:.0f} kpixel on average; accepted by the native parser: {accepted}/{len(files)}")
    print(f"host CPUs: {os.cpu_count()}; rounds: {a.rounds}; wall ms per image, median (min)")
    print(f"{'arm':<22}{'1 thread':>18}{f'{threads} threads':>18}")
    for name in arms:
        cells = [f"{statistics.median(res[(name, t)]) * 1e3:.3f} ({min(res[(name, t)]) * 1e3:.3f})" for t in (1, threads)]
        print(f"{name:<22}{cells[0]:>18}{cells[1]:>18}")
    for t in (1, threads):
        r = statistics.median(res[("native_parse_coeffs", t)]) / statistics.median(res[("pil_full_decode", t)])
        print(f"native parse / PIL decode at {t} thread(s): {r:.2f}")


if __name__ == "__main__":
    main()
