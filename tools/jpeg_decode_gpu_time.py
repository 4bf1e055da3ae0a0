"""hipEvent times of the GPU JPEG decode launches for one corpus batch, next to the same slot's H2D copy
and resize launch, for both decode paths (PIL pixels staged / coefficients staged and decoded on the device).

    python tools/jpeg_decode_gpu_time.py [--images 32] [--rounds 20] [--out FILE]

Per round the two paths are staged alternately through one StagingRing; `h2d` is ev_h2d0 -> ev_h2d1 of the
slot, `decode+resize` is ev_comp0 -> an event recorded right after stage() returns. The decode launch pair
and the resize launch are then re-issued alone on the staged slot between events of their own. Also prints
the bytes each path uploads and ships over the front-end socket per request.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from http_load import corpus

    from deconv_api_amd.codec import JpegCoeffs, read_data_url
    from deconv_api_amd.ops import native
    from deconv_api_amd.runtime.staging import StagingRing, _layout

    dev = torch.device("cuda", 0)
    urls = [u for u, _ in corpus(a.images, png_every=0)]
    pix = [read_data_url(u) for u in urls]
    coef = [read_data_url(u, coeffs=True) for u in urls]
    assert all(isinstance(c, JpegCoeffs) for c in coef), "a corpus image fell back to PIL"
    n = len(urls)
    ring = StagingRing(dev, slots=1, max_images=n)
    out = {k: torch.empty(n, 224, 224, 8, dtype=torch.bfloat16, device=dev) for k in ("pil", "gpu")}
    lib = native.lib()
    t = {k: [] for k in ("pil h2d", "pil resize (in stage)", "gpu h2d", "gpu decode+resize (in stage)",
                         "gpu decode alone", "gpu resize alone")}

    def ev():
        return torch.cuda.Event(enable_timing=True)

    with torch.cuda.stream(ring.compute_stream):
        for r in range(a.rounds + 2):
            rec = r >= 2  # two warm-up rounds
            for key, imgs in (("pil", pix), ("gpu", coef)):
                st = ring.stage(imgs, out[key])
                e1 = ev()
                e1.record()
                extra = []
                if key == "gpu":
                    i, nj = st.slot, n
                    e = [ev() for _ in range(4)]
                    e[0].record()
                    lib.jpeg_dec_batch(ring.dev[i], ring.jtab_dev[i, :nj], ring.jtab_host[i, :nj])
                    e[1].record()
                    e[2].record()
                    lib.resize_batch(ring.dev[i], ring.tab_dev[i, :n], out[key][:n], ring.dev[i].numel())
                    e[3].record()
                    extra = e
                torch.cuda.synchronize()
                if rec:
                    t[f"{key} h2d"].append(st.ev_h2d0.elapsed_time(st.ev_h2d1))
                    t["pil resize (in stage)" if key == "pil" else "gpu decode+resize (in stage)"].append(
                        st.ev_comp0.elapsed_time(e1))
                    if extra:
                        t["gpu decode alone"].append(extra[0].elapsed_time(extra[1]))
                        t["gpu resize alone"].append(extra[2].elapsed_time(extra[3]))
    assert torch.equal(out["pil"], out["gpu"]), "the two paths staged different network inputs"
    up_pil = _layout(pix, 224, 224)[4]
    _, _, _, _, up_gpu, end_gpu = _layout(coef, 224, 224)
    sock_pil = sum(p.size for p in pix) / n
    sock_gpu = sum(c.coef.nbytes + c.qt.nbytes + 4 for c in coef) / n
    lines = [f"{n}-image batch of tools/http_load.py:corpus(png_every=0) on {torch.cuda.get_device_name(dev)}; "
             f"{a.rounds} rounds, paths alternating; ms, median (min)",
             "the two paths staged bit-identical network inputs: True"]
    for k, v in t.items():
        lines.append(f"  {k:<32}{statistics.median(v):8.3f} ({min(v):.3f})")
    lines.append(f"upload per batch:      pil {up_pil / 1e6:.2f} MB   gpu {up_gpu / 1e6:.2f} MB "
                 f"(+ {(end_gpu - up_gpu) / 1e6:.2f} MB device-only planes and RGB)")
    lines.append(f"socket payload / req:  pil {sock_pil / 1e3:.1f} KB   gpu {sock_gpu / 1e3:.1f} KB "
                 "(coefficients are 3 B/px at 4:2:0, as RGB is, plus MCU padding)")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
