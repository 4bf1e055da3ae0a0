"""Helpers shared by the GPU kernel tests: the route report, the CU count and the tile / split-K override."""
import contextlib

import torch

from deconv_api_amd import ops


def route():
    """The kernel the last conv2d of this thread launched (csrc/bindings.cpp conv_route): a test that
    names a kernel asserts it, so a dispatch threshold or another CU count cannot quietly turn the
    test into one of the kernel's fallback."""
    return ops.native.lib().conv_route()


def is_route(*prefixes):
    r = route()
    assert any(r.startswith(p) for p in prefixes), f"route {r!r}, expected one of {prefixes}"
    return r


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def tune(cfg, ks):
    """Force the LDS-DMA tile config (0: automatic) and split-K factor (0: automatic, 1: none) of every
    conv inside the block. (DV_NO_SPLITK is latched at the process's first DMA conv: a test cannot
    switch it.)"""
    lib = ops.native.lib()
    lib.dma_tune(cfg, ks)
    try:
        yield
    finally:
        lib.dma_tune(0, 0)
