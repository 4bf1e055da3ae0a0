"""GPU JPEG decode: quantized DCT coefficients (codec.JpegCoeffs, from the native entropy decoder
csrc/jpeg_dec.cpp) -> RGB bytes bit-identical to ``PIL.Image.open(...).convert("RGB")``.

Device tensors go to the HIP kernels (csrc/jpeg_dec_gpu.hip); the CPU path is a vectorised numpy
reference of the same three integer steps (libjpeg's islow IDCT, "fancy" chroma upsampling over the
real chroma extent, its YCbCr -> RGB constants) and the oracle of the kernel tests.

``plan_batch`` / ``fill_batch`` lay a batch out in one byte blob the way the kernels read it; the
staging ring (runtime/staging.py) uses them on its pinned slot, ``jpeg_coeffs_to_rgb`` on a blob of its own.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

K444, K422, K420, KGREY = 0, 1, 2, 3
TAB_FIELDS = 12  # int32 per image: coef, rgb, H, W, kind, qt, plane, first block, first item, 3 spare
QT_BYTES = 384   # three uint16 [64] quantizers per image, column-major like the blocks


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def geometry(H: int, W: int, kind: int):
    """(hs, vs, mcux, mcuy, luma blocks, blocks per chroma component) of an image."""
    hs = 2 if kind in (K422, K420) else 1
    vs = 2 if kind == K420 else 1
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    return hs, vs, mcux, mcuy, mcux * mcuy * hs * vs, mcux * mcuy


def total_blocks(H: int, W: int, kind: int) -> int:
    *_, nY, nC = geometry(H, W, kind)
    return nY + (0 if kind == KGREY else 2 * nC)


def check_coeffs(c) -> None:
    """A JpegCoeffs that did not come from the native parser (a socket, a test) must still be
    consistent: the kernels index the coefficient array by its header."""
    if not (1 <= c.H <= 65535 and 1 <= c.W <= 65535 and c.kind in (K444, K422, K420, KGREY)):
        raise ValueError("JpegCoeffs: bad size or sampling kind")
    ncomp = 1 if c.kind == KGREY else 3
    if c.ncomp != ncomp or c.qt.dtype != np.uint16 or c.qt.shape != (ncomp, 64):
        raise ValueError("JpegCoeffs: quantizers do not match the component count")
    if c.coef.dtype != np.int16 or c.coef.ndim != 1 or c.coef.size != 64 * total_blocks(c.H, c.W, c.kind):
        raise ValueError("JpegCoeffs: coefficient array does not match the header")


# ------------------------------------------------------------------ CPU reference
def _idct_pass(c):
    """One 1-D pass of libjpeg's jidctint.c on axis -1 (eight inputs), before the descale."""
    c = [c[..., k] for k in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) * 8192, (c[0] - c[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-1)


def idct_gain() -> int:
    """Largest |weight| of one input in one output of a pass (csrc/jpeg_dec.cpp quotes it: <= 11400)."""
    return int(np.abs(_idct_pass(np.eye(8, dtype=np.int64))).max())


def _plane(blocks: np.ndarray, qt: np.ndarray, bh: int, bw: int) -> np.ndarray:
    """int16 [bh * bw, 64] column-major blocks -> uint8 [bh * 8, bw * 8] samples."""
    x = blocks.reshape(bh, bw, 8, 8).astype(np.int64) * qt.reshape(8, 8).T.astype(np.int64)  # [.., col, row]
    ws = (_idct_pass(x) + (1 << 10)) >> 11            # pass 1 along the rows of a column: [.., col, r]
    out = (_idct_pass(ws.transpose(0, 1, 3, 2)) + (1 << 17)) >> 18  # pass 2 along the columns of a row: [.., r, c]
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1_fancy(c: np.ndarray) -> np.ndarray:
    """[h, cw] -> [h, 2 cw] (jdsample.c h2v1_fancy_upsample; plain replication for cw <= 2)."""
    c = c.astype(np.int32)
    cw = c.shape[1]
    out = np.empty((c.shape[0], 2 * cw), np.int32)
    if cw <= 2:
        out[:, 0::2] = c
        out[:, 1::2] = c
        return out
    out[:, 0::2] = (3 * c + np.concatenate([c[:, :1], c[:, :-1]], 1) + 1) >> 2
    out[:, 1::2] = (3 * c + np.concatenate([c[:, 1:], c[:, -1:]], 1) + 2) >> 2
    out[:, 0] = c[:, 0]
    out[:, -1] = c[:, -1]
    return out


def _h2v2_fancy(c: np.ndarray) -> np.ndarray:
    """[ch, cw] -> [2 ch, 2 cw] (jdsample.c h2v2_fancy_upsample; plain replication for cw <= 2)."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    out = np.empty((2 * ch, 2 * cw), np.int32)
    if cw <= 2:
        for dy in (0, 1):
            for dx in (0, 1):
                out[dy::2, dx::2] = c
        return out
    up = np.concatenate([c[:1], c[:-1]], 0)
    dn = np.concatenate([c[1:], c[-1:]], 0)
    for dy, far in ((0, up), (1, dn)):
        s = 3 * c + far
        ev = (3 * s + np.concatenate([s[:, :1], s[:, :-1]], 1) + 8) >> 4
        od = (3 * s + np.concatenate([s[:, 1:], s[:, -1:]], 1) + 7) >> 4
        ev[:, 0] = (4 * s[:, 0] + 8) >> 4
        od[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[dy::2, 0::2] = ev
        out[dy::2, 1::2] = od
    return out


def decode_ref(c) -> np.ndarray:
    """JpegCoeffs -> uint8 [H, W, 3] on the host (the reference of the kernels)."""
    check_coeffs(c)
    H, W = c.H, c.W
    hs, vs, mcux, mcuy, nY, nC = geometry(H, W, c.kind)
    blocks = c.coef.reshape(-1, 64)
    Y = _plane(blocks[:nY], c.qt[0], mcuy * vs, mcux * hs)[:H, :W].astype(np.int32)
    if c.kind == KGREY:
        return np.repeat(Y.astype(np.uint8)[..., None], 3, axis=2)
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = []
    for k in (1, 2):
        p = _plane(blocks[nY + (k - 1) * nC: nY + k * nC], c.qt[k], mcuy, mcux)[:ch, :cw]
        if c.kind == K422:
            p = _h2v1_fancy(p)
        elif c.kind == K420:
            p = _h2v2_fancy(p)
        chroma.append(p[:H, :W].astype(np.int32) - 128)
    cb, cr = chroma
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ batch layout for the kernels
def plan_batch(coeffs: Sequence, start: int = 0, rgb_align: int = 16):
    """Lay ``coeffs`` out behind byte ``start`` of a blob: first what the host writes and uploads (per image
    the coefficients, then its quantizers), then the device-only part (the planes of every image, then the RGB
    outputs, each aligned to ``rgb_align``). -> (table int32 [n, TAB_FIELDS], upload_end, end). Offsets are int32: ``end`` < 2^31."""
    n = len(coeffs)
    tab = np.zeros((n, TAB_FIELDS), np.int32)
    off = _round_up(start, 16)
    rows = []
    for c in coeffs:
        check_coeffs(c)
        nb = total_blocks(c.H, c.W, c.kind)
        co = off
        qo = co + nb * 128
        off = _round_up(qo + QT_BYTES, 16)
        rows.append([co, 0, c.H, c.W, c.kind, qo, 0, 0, 0, nb])
    upload_end = off
    blk = item = 0
    for r in rows:  # the planes of every image (whole blocks: the offsets stay 16-byte aligned) ...
        r[6] = off
        off += r[9] * 64
        r[7], r[8] = blk, item
        blk += r[9]
        item += r[2] * ((r[3] + 3) // 4)
    for r in rows:  # ... then the RGB outputs
        r[1] = off = _round_up(off, rgb_align)
        off += r[2] * r[3] * 3
    if off >= 2 ** 31 or blk >= 2 ** 31 - 64 or item >= 2 ** 31 - 512:
        raise ValueError("JPEG decode batch too large for 32-bit offsets")
    for b, r in enumerate(rows):
        tab[b, :9] = r[:9]
    return tab, upload_end, _round_up(off, 16)


def fill_batch(host: np.ndarray, tab: np.ndarray, coeffs: Sequence) -> None:
    """Write the uploaded part of a planned batch into ``host`` (uint8 view of the blob)."""
    for r, c in zip(tab, coeffs):
        co, qo = int(r[0]), int(r[5])
        host[co:co + c.coef.size * 2] = c.coef.view(np.uint8)
        # column-major, like the blocks; one strided copy straight into the blob (this runs on the GPU
        # worker thread for every image). A greyscale image's two spare tables are never read.
        hq = host[qo:qo + 128 * c.ncomp].view(np.uint16).reshape(c.ncomp, 8, 8)
        hq[:] = c.qt.reshape(c.ncomp, 8, 8).transpose(0, 2, 1)


def jpeg_coeffs_to_rgb(coeffs: List, device, rgb_align: int = 16) -> List[torch.Tensor]:
    """A list of JpegCoeffs -> a list of uint8 [H, W, 3] tensors on ``device``. GPU: one upload and the
    two decode launches for the whole list, on the current stream; CPU: the numpy reference."""
    device = torch.device(device)
    if device.type != "cuda":
        return [torch.from_numpy(decode_ref(c)) for c in coeffs]
    if not coeffs:
        return []
    from . import native

    tab, upload_end, end = plan_batch(coeffs, 0, rgb_align)
    host = np.zeros(upload_end, np.uint8)
    fill_batch(host, tab, coeffs)
    blob = torch.empty(end, dtype=torch.uint8, device=device)
    blob[:upload_end].copy_(torch.from_numpy(host))
    tab_t = torch.from_numpy(tab)
    native.lib().jpeg_dec_batch(blob, tab_t.to(device), tab_t)
    return [blob[int(r[1]): int(r[1]) + c.size].view(c.H, c.W, 3) for r, c in zip(tab, coeffs)]
