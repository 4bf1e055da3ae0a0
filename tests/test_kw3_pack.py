"""The packed KW3 B image (ops/conv.py kw3_pack): the bytes the KW3 / KW3P kernels' B stages hold, built at
weight-load time. Checked against an element-by-element loop written from the layout's definition
(docs/KERNELS.md, round 7), not from the packer's tensor indexing."""
import pytest
import torch

from deconv_api_amd.ops.conv import ConvWeights, kw3_pack, kw3_packable, kw3_unpack


def _swz(row):
    return ((row >> 2) & 1) << 1


def _pack_loop(w_gemm, C):
    """piece[step = cc*3 + kh][kw][rb], 512 elements each; lane l of a piece = 8 elements of row
    rb*16 + (l >> 2) at column (kh*3 + kw)*C + cc*32 + 8*((l & 3) ^ swz(l >> 2))."""
    ocpad = w_gemm.shape[0]
    rbs = ocpad // 16
    out = torch.empty(ocpad * 9 * C, dtype=w_gemm.dtype)
    for step in range(3 * (C // 32)):
        cc, kh = divmod(step, 3)
        for kw in range(3):
            for rb in range(rbs):
                piece = (step * 3 + kw) * rbs + rb
                for lane in range(64):
                    row = rb * 16 + (lane >> 2)
                    col = (kh * 3 + kw) * C + cc * 32 + 8 * ((lane & 3) ^ _swz(lane >> 2))
                    out[piece * 512 + lane * 8: piece * 512 + lane * 8 + 8] = w_gemm[row, col: col + 8]
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ocpad,C", [(128, 32), (256, 96), (512, 64)])
def test_kw3_pack_matches_definition(ocpad, C, dt):
    g = torch.Generator().manual_seed(ocpad + C)
    kpad = -(-9 * C // 64) * 64
    # distinct values per element wherever the format allows (a permutation error cannot cancel), K padding
    # filled with a value the image must not contain
    w = torch.randn(ocpad, kpad, generator=g).to(dt)
    w[:, 9 * C:] = 777.0
    img = kw3_pack(w, C)
    assert img.dtype == dt and img.is_contiguous() and img.numel() == ocpad * 9 * C
    assert torch.equal(img.view(torch.int16), _pack_loop(w, C).view(torch.int16))
    assert not bool((img == 777.0).any())
    back = kw3_unpack(img, ocpad, C)
    assert torch.equal(back.view(torch.int16), w[:, : 9 * C].contiguous().view(torch.int16))


def test_kw3_pack_subtile_is_contiguous():
    """A tile's (step, kw) sub-tile is the BN*64 bytes at piece (step*3 + kw)*(OCpad/16) + n0/16, whatever BN."""
    ocpad, C = 256, 64
    w = torch.arange(ocpad * 9 * C, dtype=torch.float32).reshape(ocpad, 9 * C).to(torch.int16)
    img = kw3_pack(w, C)
    for bn, n0, step, kw in ((256, 0, 4, 1), (128, 128, 5, 2), (128, 0, 0, 0)):
        cc, kh = divmod(step, 3)
        p = (step * 3 + kw) * (ocpad // 16) + n0 // 16
        sub = img[p * 512: p * 512 + bn * 32].reshape(bn, 4, 8)  # LDS rows of 64 B: [row][chunk slot][8]
        for row in (0, 5, 17, bn - 1):
            for slot in range(4):
                col = (kh * 3 + kw) * C + cc * 32 + 8 * (slot ^ _swz(row))
                assert torch.equal(sub[row, slot], w[n0 + row, col: col + 8]), (bn, n0, step, kw, row, slot)


@pytest.mark.parametrize("kh,kw,cin,ocpad,kind", [(3, 3, 8, 128, "fwd"), (3, 3, 16, 256, "fwd"), (3, 3, 64, 64, "fwd"),
                                                  (1, 1, 64, 128, "fwd"), (3, 1, 64, 128, "fwd"),
                                                  (3, 3, 64, 128, "transpose")])
def test_kw3_ineligible_shapes(kh, kw, cin, ocpad, kind):
    assert not kw3_packable(kh, kw, cin, ocpad, kind)
    assert kw3_packable(3, 3, 64, 128)


def test_conv_weights_cpu_has_no_image():
    """to_device packs on the GPU only (next to w_gemm); a CPU ConvWeights carries neither."""
    cw = ConvWeights(torch.randn(128, 32, 3, 3), None).to_device("cpu")
    assert cw.w_gemm is None and cw.w_kw3 is None
