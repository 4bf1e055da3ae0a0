"""Activation maps on VGG16 (Zeiler & Fergus figure 7 (b); the third view of a filter next to the deconvnet projection
of engine/deconvnet.py and the occlusion sensitivity of engine/occlusion.py): where in the image does a layer's
strongest filter fire?

One ``DeconvNet.forward`` for the whole batch, the regime the tuned forward is built for (no conv kernel is
touched), then per image the four filters ``POST /`` would reconstruct (``select_filters``, per image; -1 = fewer
than four positive filters), their feature maps upsampled bilinearly to the input (ops/actmap.py) and the 2 x 2
true-RGB mosaic of ``ops.occlusion_overlay`` (red tint with weight 0.6 heat / max heat; a conv target's map is
post-ReLU, a pool target's the pooled map: never negative). Only conv and pool targets have a feature map.

Eager (no hipGraph), like engine/occlusion.py."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..utils import tracing
from .deconvnet import DeconvNet

SPATIAL_KINDS = ("conv", "pool")


@dataclass
class ActivationResult:
    filters: torch.Tensor  # int32 [B, 4] (-1 = no positive filter: zero heat, black tile)
    sums: torch.Tensor  # fp32 [B, 4] selection scores (the filters' channel sums)
    heat: torch.Tensor  # fp32 [B, 4, S, S]
    mosaic: torch.Tensor  # u8 RGB [B, 2 S, 2 S, 3]


class ActivationMaps:
    def __init__(self, net: DeconvNet):
        self.net = net

    def spatial_layers(self):
        """The layers that have a feature map: the conv and pool layers."""
        return [s.name for s in self.net.specs[1:] if s.kind in SPATIAL_KINDS]

    def check_layer(self, layer: str) -> None:
        """UnknownLayerError, or ValueError for a flatten / dense layer; before any compute."""
        i = self.net._check_layer(layer)
        if self.net.specs[i].kind not in SPATIAL_KINDS:
            raise ValueError(f"layer {layer!r} has no feature map (activation maps take a conv or pool layer)")

    def run(self, x: torch.Tensor, layer: str) -> ActivationResult:
        """x: preprocessed [B, S, S, 8] (the 16-bit network input on the GPU, fp32 on the CPU)."""
        self.check_layer(layer)
        if x.dim() != 4 or x.shape[1] != x.shape[2] or x.shape[3] != 8:
            raise ValueError(f"expected the network-input layout [B, S, S, 8], got {tuple(x.shape)}")
        S = x.shape[1]
        with tracing.range_("act.forward"):
            out = self.net.forward(x, layer).out
        with tracing.range_("act.maps"):
            idx, sums = self.net.select_filters(out, 4, "per_image")
            heat, part = ops.activation_heat(out, idx, S)
            mosaic = ops.occlusion_overlay(heat, part, idx, x)
        return ActivationResult(idx, sums, heat, mosaic)
