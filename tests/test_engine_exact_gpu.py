"""GPU: the deconvnet ENGINE (engine/deconvnet.py DeconvNet.forward / select_filters / backward / run / _run_split,
with the dense head it drives as 1x1 convs) against the independent fp64 oracle (oracle/deconv_ref.py), bit for bit.

The kernels have exact tests of their own (test_conv_exact_gpu.py, test_conv_routes_exact_gpu.py,
test_deconv_exact_gpu.py, ...); this file holds the code that strings them together to the same standard: the
arguments the engine hands the kernels (code_div / unpool_div = K, which pool's codes, relu_below, the
transposed dense kernels, use_bias=False, the flatten order, the fp16 unit seed and its scale, the stats
hand-over), on every branch that exists only behind ``is_cuda``.

Method (tests/engine_oracle.py): a VGG16 with +-1 weights and calibrated integer biases on integer images, so
that every 16-bit store of the engine is exact in bf16 and fp16 and every fp32 sum is exact in any order;
``deconv_ref.visualize_all_layers`` is then the expected output and every comparison is ``torch.equal``. The
only tolerances: the softmax probabilities (the bound of test_deconv_exact_gpu.py::test_softmax_rows_edges) and
the uint8 mosaic (the bound of test_oracle_engine.py::test_full_vgg16_block1_conv1_cpu). The conditions of the
method are asserted on the oracle alone (``engine_oracle.oracle`` / ``forward``) before a GPU result exists;
``test_conditions`` and ``test_cpu_engine_mosaic`` need no GPU.

Three geometries: ``tall`` (width_div 8 at image 64, where flatten's input is 2 x 2: the flatten and dense targets);
``small`` (width_div 8, image 32, fc 256, 40 classes, B = 2): all 22 layers x {all, max} x
{global, per_image}; ``wide`` (full widths at image 32, fc 4096, 1000 classes, B = 3 different images): the
targets that reach every fused branch, each branch asserted through counting wrappers and ``conv_route()``.
"""
import re

import numpy as np
import pytest
import torch

import engine_oracle as eo
from deconv_api_amd import ops
from deconv_api_amd.engine import deconvnet as dn
from deconv_api_amd.engine.deconvnet import DeconvNet
from exact_helpers import BF, DEV, HF, _same
from gpu_helpers import route as _route

gpu = pytest.mark.gpu
K = eo.K
DTS = {"bf16": BF, "fp16": HF}
MODES = [(m, t) for m in ("all", "max") for t in ("global", "per_image")]
SMALL_LAYERS = [s.name for s in eo.vgg16_specs(**eo.GEOM["small"][0])[1:]]
# wide: every fused branch of the engine (asserted in test_wide_targets) and the 1 x 1-map / dense targets
WIDE = [("block1_conv1", "all"), ("block1_conv2", "all"), ("block1_pool", "all"), ("block2_conv2", "max"),
        ("block3_conv3", "all"), ("block3_pool", "all"), ("block5_conv3", "all"), ("block5_pool", "max"),
        ("flatten", "all"), ("fc1", "max"), ("fc2", "all"), ("predictions", "all")]
# tall (width_div 8 at image 64, B = 2): block5_pool is 2 x 2 there, so flatten's (h, w, c) order and the reshape
# of its down are visible (on the 1 x 1 map of the other two geometries every order is the same)
TALL = ["flatten", "fc1", "fc2", "predictions"]
# run(): (geometry, layer, mode). block1_conv1 has no stats tensor, predictions in fp16 hands the stats over around
# the unit-seed chain, wide block3_pool takes them from the fused tail
RUNS = [("small", "block1_conv1", "all"), ("small", "block3_conv2", "all"), ("small", "block4_pool", "max"),
        ("small", "fc1", "all"), ("small", "predictions", "all"), ("wide", "block3_pool", "all"),
        ("wide", "predictions", "all")]
SPLIT = [("small", "block3_conv3"), ("small", "predictions"), ("wide", "fc2")]

_engines = {}


def _engine(name, dtn):
    if (name, dtn) not in _engines:
        c = eo.case(name)
        _engines[name, dtn] = (DeconvNet(c.model.build(DEV, DTS[dtn])), c.x8.to(DTS[dtn]).to(DEV))
    return _engines[name, dtn]


def _mosaic_close(got_u8, o, b):
    want = eo.mosaic_ref(o, b)
    diff = np.abs(got_u8.astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3, (int(diff.max()), float((diff > 0).mean()))


# ----------------------------------------------------------------------------------------
# conditions (no GPU)
# ----------------------------------------------------------------------------------------

def _all_requests():
    for layer in SMALL_LAYERS:
        for mode, tk in MODES:
            yield "small", layer, mode, tk
    for layer, mode in WIDE:
        yield "wide", layer, mode, "per_image"
    for layer in TALL:
        for mode, tk in MODES:
            yield "tall", layer, mode, tk
    for name, layer, mode in RUNS:
        yield name, layer, mode, "per_image"
    for name, layer in SPLIT:
        yield name, layer, "all", "per_image"


def test_conditions():
    """(a)-(e) for every request of this file (asserted inside ``engine_oracle``), (f) for at least one of each
    geometry and at a conv, a pool and a dense target; the duplicated filters are selected next to each other."""
    tied = set()
    for name in ("small", "wide", "tall"):
        eo.forward(name)
    assert eo.case("tall").specs[-4].out_hw == 2 and eo.case("small").specs[-4].out_hw == 1  # flatten's map
    for name, layer, mode, tk in _all_requests():
        try:
            o = eo.oracle(name, layer, mode, tk)
        except AssertionError as e:
            raise AssertionError(f"{name} {layer} {mode} {tk}: {e}") from e
        if eo.tied_selection(o):
            tied.add((name, layer))
    for name in ("small", "wide"):
        for layer, (t, u) in eo.case(name).dup_of.items():
            assert (name, layer) in tied, f"{name} {layer}: no tied selection sums"
            f = eo.oracle(name, layer, "all", "per_image").filters[0].tolist()
            # (wide fc2: more than four units tie at the top, so the first four by index are selected instead)
            assert (name, layer) == ("wide", "fc2") or (t in f and u in f), (name, layer, f)
            assert not (t in f and u in f) or f.index(t) + 1 == f.index(u), (name, layer, f)
    # max + global at fc1 selects the unit with unequal values first: the images below the batch maximum reconstruct
    # to zero, the others do not
    for name in ("small", "tall"):
        o = eo.oracle(name, "fc1", "max", "global")
        assert int(o.filters[0, 0]) == eo.case(name).uneven
        per_image = o.recon[:, 0].flatten(1).abs().sum(1)
        assert bool((per_image == 0).any()) and bool((per_image > 0).any())
    assert {"block2_conv2", "block4_pool", "fc2", "predictions"} <= {ly for n, ly in tied if n == "small"}


@pytest.mark.parametrize("name,layer,mode", RUNS[:5])
def test_cpu_engine_mosaic(name, layer, mode):
    """The CPU engine (fp32) on this model: reconstructions equal to the oracle's, the mosaic within the bound the
    GPU test uses."""
    c = eo.case(name)
    o = eo.oracle(name, layer, mode, "per_image")
    res = DeconvNet(c.model.build("cpu", torch.float32)).run(c.x8, layer, k=K, mode=mode)
    _same(res.recon, o.recon.float())
    assert torch.equal(res.filters, o.filters)
    for b in range(c.B):
        _mosaic_close(res.mosaic[b].numpy(), o, b)


# ----------------------------------------------------------------------------------------
# forward + selection + backward
# ----------------------------------------------------------------------------------------

def _check_forward(name, eng, st, layer):
    """Target output and every switch code of the forward state against the oracle's forward."""
    outs, codes = eo.forward(name)
    want = outs[layer]
    if layer == "predictions":
        # the softmax_rows bound on what the engine stores; the live units exactly (the chain starts there)
        c = eo.case(name)
        got = st.out.float().cpu().double()
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-7)
        assert torch.equal(got[:, c.live], want[:, c.live])
    else:
        _same(st.out, want.float())
    names = eng.names
    pools = [n for n in names[: names.index(layer) + 1] if n.endswith("_pool")]
    assert sorted(st.codes) == sorted(pools)
    for p in pools:
        assert torch.equal(st.codes[p].cpu(), codes[p]), f"{p}: switch codes differ from the oracle's first-max switches"


def _check_request(name, eng, x, st, layer, mode, tk):
    o = eo.oracle(name, layer, mode, tk)
    idx, val = DeconvNet.select_filters(st.out, K, tk)
    assert torch.equal(idx.cpu(), o.filters), f"{tk}: filters {idx.cpu().tolist()}, oracle {o.filters.tolist()}"
    assert torch.equal(val.cpu().double(), o.sums), f"{tk}: selection sums differ"
    recon = eng.backward(st, idx, mode, tk)
    assert recon.dtype == torch.float32
    _same(recon, o.recon.float())


@gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
@pytest.mark.parametrize("layer", SMALL_LAYERS)
def test_small_targets(native_lib, layer, dtn):
    """Every named layer as target at width_div 8, image 32, B = 2: the forward's output and switch codes, the
    selected filters in the oracle's order, and the reconstructions in modes all / max with batch_topk global
    (the oracle's rule, max over the batch axis included) / per_image (the oracle one image at a time)."""
    eng, x = _engine("small", dtn)
    st = eng.forward(x, layer)
    _check_forward("small", eng, st, layer)
    for mode, tk in MODES:
        _check_request("small", eng, x, st, layer, mode, tk)


@gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
@pytest.mark.parametrize("layer", TALL)
def test_tall_dense_targets(native_lib, layer, dtn):
    """The flatten and dense targets behind a 2 x 2 block5_pool (image 64): the (h, w, c) order of ``flatten`` going
    up and of the reshape going down, in all four request kinds."""
    eng, x = _engine("tall", dtn)
    st = eng.forward(x, layer)
    _check_forward("tall", eng, st, layer)
    for mode, tk in MODES:
        _check_request("tall", eng, x, st, layer, mode, tk)


class _Spy:
    """Counting wrappers around the ops the engine calls (no engine code changes)."""

    def __init__(self, monkeypatch):
        self.stem = self.tail = self.unpool_out = self.unpool_in = 0
        self.dense = []  # (M, K, OC, route) of every 1x1 conv on a 1 x 1 map
        real_stem, real_tail, real_conv = ops.stem_pool, ops.deconv_tail, ops.conv2d

        def stem(*a, **k):
            r = real_stem(*a, **k)
            self.stem += r is not None
            return r

        def tail(*a, **k):
            r = real_tail(*a, **k)
            self.tail += r is not None
            return r

        def conv(x, cw, **k):
            r = real_conv(x, cw, **k)
            self.unpool_out += k.get("unpool_out") is not None
            self.unpool_in += k.get("in_mode") == "unpool"
            if cw.KH == 1 and x.shape[1] == 1 and x.shape[2] == 1:
                self.dense.append((x.shape[0], cw.cin, cw.cout, _route()))
            return r

        monkeypatch.setattr(ops, "stem_pool", stem)
        monkeypatch.setattr(ops, "deconv_tail", tail)
        monkeypatch.setattr(ops, "conv2d", conv)


@gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
@pytest.mark.parametrize("layer,mode", WIDE)
def test_wide_targets(native_lib, monkeypatch, layer, mode, dtn):
    """Full widths (64-channel block1, 512-channel 2 x 2 block5, fc 4096, 1000 classes), B = 3, K = 4, per-image
    selection, with every branch the target is meant to take asserted:
      * bf16: the fused stem (``ops.stem_pool``) from block1_pool on and the fused tail (``ops.deconv_tail``) from
        block2_conv1 on return a result; fp16 takes the unfused launches (in_mode='unpool' at block1) instead;
      * from block3_conv1 on a conv-down writes its unpooled map (``unpool_out``: the consumer has > 64 channels);
      * flatten / dense targets enter block5_conv3.down with in_mode='unpool' and block5_pool's codes;
      * every dense GEMM with 16 or more K tiles reports a split-K route (fc1.up, K = 512 here, has 8: none)."""
    eng, x = _engine("wide", dtn)
    spy = _Spy(monkeypatch)
    st = eng.forward(x, layer)
    _check_forward("wide", eng, st, layer)
    _check_request("wide", eng, x, st, layer, mode, "per_image")
    li, bf = eng.names.index(layer), dtn == "bf16"
    at = eng.names.index
    assert spy.stem == (1 if bf and li >= at("block1_pool") else 0), spy.stem
    assert spy.tail == (1 if bf and li >= at("block2_conv1") else 0), spy.tail
    assert (spy.unpool_out > 0) == (li >= at("block3_conv1")), spy.unpool_out
    dense_target = li >= at("flatten")
    assert spy.unpool_in == int(dense_target) + int(not bf and li >= at("block2_conv1")), spy.unpool_in
    n_dense = max(0, li - at("flatten"))
    assert len(spy.dense) == 2 * n_dense, spy.dense
    for M, kin, kout, r in spy.dense:
        ks = int(re.search(r"ks(\d+)", r).group(1))
        assert r.startswith("dma 64x64 st3") and (ks > 1) == (-(-kin // 64) >= 16), (M, kin, kout, r)
    assert {m for m, *_ in spy.dense} <= {3, 12}


# ----------------------------------------------------------------------------------------
# run(): mosaic + stats, and the stream split
# ----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
@pytest.mark.parametrize("name,layer,mode", RUNS)
def test_run_mosaic(native_lib, name, layer, mode, dtn):
    """``run(mosaic=True)``: reconstructions, filters and sums exact; the uint8 mosaic (made from the final conv's
    / the fused tail's epilogue statistics, from the rescaled reconstructions after a fp16 unit-seed chain, or in
    two passes for block1_conv1) within one grey level on fewer than 1 byte in 1000 of the reference's
    ``deprocess_image(mosaic(...))``."""
    eng, x = _engine(name, dtn)
    o = eo.oracle(name, layer, mode, "per_image")
    res = eng.run(x, layer, k=K, mode=mode)
    _same(res.recon, o.recon.float())
    assert torch.equal(res.filters.cpu(), o.filters) and torch.equal(res.sums.cpu().double(), o.sums)
    mos = res.mosaic.cpu().numpy()
    for b in range(eo.case(name).B):
        _mosaic_close(mos[b], o, b)


@gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
@pytest.mark.parametrize("name,layer", SPLIT)
def test_run_split(native_lib, monkeypatch, name, layer, dtn):
    """``_run_split``: a batch that splits over two streams (1 + 1 images, 2 + 1 for B = 3) equals the unsplit run
    and the oracle, mosaics included."""
    eng, x = _engine(name, dtn)
    o = eo.oracle(name, layer, "all", "per_image")
    whole = eng.run(x, layer, k=K)
    calls = []
    real = eng._run1
    monkeypatch.setattr(eng, "_run1", lambda xp, *a: calls.append(xp.shape[0]) or real(xp, *a))
    monkeypatch.setattr(dn, "DECONV_STREAMS", 2)
    monkeypatch.setattr(dn, "DECONV_SPLIT_MIN", 2)
    res = eng.run(x, layer, k=K)
    torch.cuda.synchronize()
    assert calls == ([1, 1] if x.shape[0] == 2 else [2, 1]), calls
    _same(res.recon, o.recon.float())
    assert torch.equal(res.recon, whole.recon) and torch.equal(res.filters, whole.filters)
    assert torch.equal(res.sums, whole.sums) and torch.equal(res.mosaic, whole.mosaic)
    assert torch.equal(res.filters.cpu(), o.filters)
