"""Occlusion sensitivity maps on VGG16 (Zeiler & Fergus section 4.2; the deconvnet of engine/deconvnet.py is the
other half of that paper): where in the image does the evidence for a layer's strongest filters lie?

Per image: the P + 1 occluded variants (ops/occlusion.py) go through ``DeconvNet.forward`` as ONE batch, the
regime the tuned forward is built for (fused stem, KW3P, pool epilogues; no conv kernel is touched). The score of
a variant is the selection score of ``find_top_filters``: the channel sum of a conv / pool target, the unit's
value of a flatten / dense target. The filters are the four ``POST /`` would reconstruct (``select_filters`` on
the unoccluded variant 0, per image; -1 = fewer than four positive filters). Drops become per-pixel heat maps and
a 2 x 2 true-RGB mosaic (no channel reversal: an extension, not reference parity).

Images of a batch run one after another, eagerly (no hipGraph)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..ops.occlusion import occlusion_grid
from ..utils import tracing
from .deconvnet import DeconvNet

DEFAULT_PATCH = 32
DEFAULT_STRIDE = 16


@dataclass
class OcclusionResult:
    scores: torch.Tensor  # fp32 [B, P + 1, 4]: the selected filters' score of every variant (0 where filter -1)
    filters: torch.Tensor  # int32 [B, 4] (-1 = no positive filter: zero heat, black tile)
    heat: torch.Tensor  # fp32 [B, 4, S, S]
    mosaic: torch.Tensor  # u8 RGB [B, 2 S, 2 S, 3]


class Occlusion:
    def __init__(self, net: DeconvNet):
        self.net = net

    def variant_scores(self, xv: torch.Tensor, layer: str) -> torch.Tensor:
        """fp32 [V, C] scores of a batch of variants: one ``DeconvNet.forward`` call."""
        out = self.net.forward(xv, layer).out
        return ops.channel_sum(out) if out.dim() == 4 else out.float().contiguous()

    def run(self, x0: torch.Tensor, layer: str, patch: int = DEFAULT_PATCH, stride: int = DEFAULT_STRIDE) -> OcclusionResult:
        """x0: preprocessed [B, S, S, 8] (the 16-bit network input on the GPU, fp32 on the CPU)."""
        self.net._check_layer(layer)  # UnknownLayerError
        if x0.dim() != 4 or x0.shape[1] != x0.shape[2] or x0.shape[3] != 8:
            raise ValueError(f"expected the network-input layout [B, S, S, 8], got {tuple(x0.shape)}")
        B, S = x0.shape[:2]
        V = len(occlusion_grid(S, patch, stride)) ** 2 + 1  # ValueError outside the definition
        scores, filters, heats, mosaics = [], [], [], []
        for b in range(B):
            xb = x0[b:b + 1].contiguous()
            with tracing.range_("occ.variants"):
                xv = ops.occlude_variants(xb, patch, stride)
            with tracing.range_("occ.forward"):
                sc = self.variant_scores(xv, layer).view(1, V, -1)
            with tracing.range_("occ.maps"):
                idx, _ = ops.topk_positive(sc[:, 0], 4)  # = DeconvNet.select_filters(out[:1], 4, "per_image")
                heat, part = ops.occlusion_heat(sc, idx, S, patch, stride)
                mosaics.append(ops.occlusion_overlay(heat, part, idx, xb))
            sel = torch.gather(sc, 2, idx.long().clamp_min(0).view(1, 1, 4).expand(1, V, 4))
            scores.append(sel * (idx >= 0).view(1, 1, 4))
            filters.append(idx)
            heats.append(heat)
        return OcclusionResult(torch.cat(scores), torch.cat(filters), torch.cat(heats), torch.cat(mosaics))
