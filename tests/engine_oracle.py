"""A VGG16 the fp64 oracle can follow exactly, for tests/test_engine_exact_gpu.py. A plain module, not a conftest.

``case(name)`` builds (once) a ``VGG16`` on ``vgg16_specs(...)`` with integer weights and a batch of integer
images such that every value the engine stores in a 16-bit tensor is an integer (at a ``predictions`` target an
integer times 2^-3) both bf16 and fp16 hold, and every fp32 partial sum is exact in any order. Then
``deconv_ref.visualize_all_layers`` (fp64, untouched) is the expected output of the GPU engine bit for bit.

Construction, layer by layer on the batch itself:
  * every conv channel / dense unit has ``taps`` non-zero weights of magnitude 1, positive with probability
    ``ppos`` (equal sign shares give all-zero reconstructions: ReLU kills every chain);
  * its integer bias is calibrated from the fp64 forward so that the channel's maximum over the batch is the
    layer's cap (convs 12, dense layers 2: the down chains are positively homogeneous in the seed, so their
    intermediates scale with the target layer's cap);
  * ``dup`` layers copy their top-sum filter onto the next index: two selected filters with EQUAL selection sums
    (the stable first-index order of ``topk_positive`` end to end);
  * fc2 holds duplicated unit pairs (j, j'); each of the 8 live ``predictions`` units has weight +1 on the j and
    -1 on the j' of one pair, so its logit is 0 for every image, and bias 0; every other unit has bias -80. The
    fp64 softmax of the live units is then exactly 2^-3 (the others add 992 e^-71 to a sum of 8, far below half
    an ulp), the engine's 16-bit probabilities are 2^-3 whatever the last bits of the kernel's fp32 quotient,
    all eight tie (the first four by index are selected), and the down chain from a live unit starts as
    2^-3 (e_j - e_j') -> ReLU -> 2^-3 e_j: not zero.

``oracle(name, layer, mode, batch_topk)`` runs ``deconv_ref.visualize_all_layers`` with a recording
``build_stack`` around it and asserts the method's conditions (a)-(e) on what the oracle itself computed, before
any GPU result exists; (f) is ``tied_selection``.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
from deconv_api_amd.oracle import deconv_ref
from exact_helpers import _check_ties, _gen, _representable

K = 4
DT = torch.float64
LIVE = 8  # live predictions units: softmax 2^-3 each
OFF_BIAS = -80.0

# taps per filter and cap by the conv's map side ("first": block1_conv1, whose 3 input channels need more taps for
# a reconstruction with 16 distinct values) and for the dense layers. Small maps get more taps (a 3 x 3 tap leaves
# a 2 x 2 map half of the time: sparse chains die there) and smaller caps (more taps, larger down sums).
TAPS = {"first": 6, 64: 3, 32: 3, 16: 2, 8: 2, 4: 3, 2: 3, "fc1": 3, "fc2": 3, "predictions": 3}
CAPS = {64: 16, 32: 16, 16: 12, 8: 12, 4: 8, 2: 4, "fc1": 3, "fc2": 2}
CENTRE_HW = 4
GEOM = {
    # name: (specs arguments, batch, seed, share of positive weights, layers whose top filter is duplicated,
    #        caps / {"taps": ...} that differ from CAPS / TAPS: a seed on the wide 1 x 1 map is one scalar, so its
    #        reconstruction gets its 16 distinct values from more taps in block5, not from a larger cap)
    "small": (dict(width_div=8, image_size=32, fc=256, classes=40), 2, 11, 0.8, ("block2_conv2", "block4_pool"), {}),
    # image 64: block5_pool is 2 x 2, so the (h, w, c) order of flatten and of its down reshape is visible
    "tall": (dict(width_div=8, image_size=64, fc=256, classes=40), 2, 16, 0.8, (), {}),
    "wide": (dict(width_div=1, image_size=32, fc=4096, classes=1000), 3, 12, 0.8, ("block3_conv3",),
             {"taps": {2: 5, "fc1": 4}}),
}


def _sparse(g, groups, cin, cols, taps, ppos, centre):
    """[groups * cin, cols] (row = group * cin + ci; a conv's 9 groups are its kernel positions, a dense layer has
    one) with up to ``taps`` entries of +-1 per column: a +1 on input ci = column mod cin, so that every input
    keeps a positive way down (at the kernel centre with ``centre``, which a 2 x 2 map cannot shift out of), and
    taps - 1 entries anywhere, positive with probability ``ppos`` (fewer where two draws coincide)."""
    rows = groups * cin
    w = torch.zeros(rows, cols, dtype=DT)
    if taps > 1:
        idx = torch.randint(0, rows, (taps - 1, cols), generator=g)
        sgn = torch.where(torch.rand(taps - 1, cols, generator=g) < ppos, 1.0, -1.0).to(DT)
        w.scatter_(0, idx, sgn)
    grp = torch.full((cols,), groups // 2) if centre else torch.randint(0, groups, (cols,), generator=g)
    w[grp * cin + torch.arange(cols) % cin, torch.arange(cols)] = 1.0
    return w


def _dup_top(w2d, b, act):
    """Copy the filter with the largest sum over the batch onto the next index. ``w2d`` [K, out], ``act`` [..., out]."""
    sums = act.reshape(-1, act.shape[-1]).sum(0)
    t = int(sums.argmax())
    u = (t + 1) % w2d.shape[1]
    w2d[:, u] = w2d[:, t]
    b[u] = b[t]
    return t, u


@functools.lru_cache(maxsize=None)
def case(name):
    sargs, B, seed, ppos, dups, caps = GEOM[name]
    taps = {**TAPS, **caps.get("taps", {})}
    caps = {**CAPS, **{k: v for k, v in caps.items() if k != "taps"}}
    specs = vgg16_specs(**sargs)
    g = _gen(seed)
    hw = sargs["image_size"]
    x3 = torch.randint(-3, 4, (B, hw, hw, 3), generator=g).to(DT)
    params, a, pairs, dup_of = {}, x3, [], {}
    for i, s in enumerate(specs):
        if s.kind == "conv":
            w = _sparse(g, 9, s.cin, s.cout, taps["first" if i == 1 else s.out_hw], ppos, s.out_hw <= CENTRE_HW)
            k = w.reshape(3, 3, s.cin, s.cout)
            pre = F.conv2d(a.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
            b = caps[s.out_hw] - pre.amax(dim=(0, 1, 2))
            # a conv whose pool is a dup layer duplicates its own filter: the pooled maps tie too
            nxt = specs[i + 1]
            if s.name in dups or (nxt.kind == "pool" and nxt.name in dups):
                t, u = _dup_top(w, b, (pre + b).relu())
                dup_of[s.name if s.name in dups else nxt.name] = (t, u)
                pre[..., u] = pre[..., t]
            a = (pre + b).relu()
            params[s.name] = (k.float().contiguous(), b.float())
        elif s.kind == "pool":
            N, H, W, C = a.shape
            a = a.reshape(N, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))
        elif s.kind == "flatten":
            a = a.reshape(B, -1)
        elif s.kind == "dense" and s.activation == "relu":
            w = _sparse(g, 1, s.cin, s.cout, taps[s.name], ppos, True)
            pre = a @ w
            b = caps[s.name] - pre.amax(dim=0)
            if s.name == "fc1":
                # one unit that holds cap in some images and cap - 1 in the others, one higher: the largest sum of
                # the layer with UNEQUAL values, so that mode ``max`` with ``global`` must zero the images below
                # the batch maximum (every other top unit holds its cap in all images)
                act = pre + b
                u = int(((act.amax(0) == caps[s.name]) & (act.amin(0) == caps[s.name] - 1)).nonzero()[0])
                b[u] += 1
                uneven = u
            if s.name == "fc2":  # LIVE duplicated pairs (j, j + 1) on even j spread over the layer
                step = (s.cout // LIVE) & ~1
                for p in range(LIVE):
                    j = p * step
                    w[:, j + 1], b[j + 1] = w[:, j], b[j]
                    pairs.append(j)
                # and the top unit next to itself: tied selection sums among the selected four
                pre = a @ w
                t = int((pre + b).relu().sum(0).argmax())
                u = t + 1 if t % 2 == 0 else t - 1
                if min(t, u) not in pairs:  # (a pair already ties)
                    w[:, u], b[u] = w[:, t], b[t]
                dup_of[s.name] = (min(t, u), max(t, u))
                pre = a @ w
            a = (pre + b).relu()
            params[s.name] = (w.float().contiguous(), b.float())
        elif s.kind == "dense":
            w = _sparse(g, 1, s.cin, s.cout, taps[s.name], ppos, True)
            b = torch.full((s.cout,), OFF_BIAS, dtype=DT)
            live = sorted(set(torch.linspace(1, s.cout - 1, LIVE).long().tolist()))  # the last unit is live
            assert len(live) == LIVE
            for n, f in enumerate(live):
                w[:, f] = 0
                w[pairs[n], f], w[pairs[n] + 1, f] = 1.0, -1.0
                b[f] = 0.0
            params[s.name] = (w.float().contiguous(), b.float())
    model = VGG16(params, list(specs))
    x8 = torch.zeros(B, hw, hw, 8)
    x8[..., :3] = x3.float()
    return types.SimpleNamespace(name=name, model=model, specs=specs, x3=x3, x8=x8, B=B, live=live, dup_of=dup_of,
                                 uneven=uneven,
                                 layers=[s.name for s in specs[1:]])


class _Rec:
    """What one oracle run stored: every stack element's up_data and, per chain, every down_data."""

    def __init__(self):
        self.stack = None
        self.downs = []  # (element name, tensor) in call order


def _recording(rec):
    real = deconv_ref.build_stack

    def build(model, layer_name):
        stack = real(model, layer_name)
        rec.stack = stack
        for el in stack:
            down = el.down

            def wrapped(y, el=el, down=down):
                r = down(y)
                rec.downs.append((el.name, r))
                return r

            el.down = wrapped
        return stack

    return real, build


def _oracle_once(c, x3, layer, mode):
    rec = _Rec()
    real, build = _recording(rec)
    deconv_ref.build_stack = build
    try:
        out = deconv_ref.visualize_all_layers(c.model, x3.numpy(), layer, mode, top=K, only_target=True)[layer]
    finally:
        deconv_ref.build_stack = real
    return out, rec


def _abs_bound(c, rec):
    """(b): max |x| times the largest column / row sum of |w| (plus |bias| going up) bounds every partial sum."""
    ups = {el.name: el.up_data for el in rec.stack}
    dmax = {}
    for name, t in rec.downs:
        dmax[name] = max(dmax.get(name, 0.0), float(t.abs().max()))
    prev = rec.stack[0].up_data
    for el in rec.stack[1:]:
        if isinstance(el, (deconv_ref.DConv, deconv_ref.DDense)):
            k, b = c.model.params[el.name]
            w2 = k.reshape(-1, k.shape[-1]).abs().double()
            up = float(prev.abs().max()) * float(w2.sum(0).max()) + float(b.abs().max())
            assert up < 2 ** 24, f"{el.name}: up partial sums not exact in fp32"
        prev = el.up_data
    # a down's input is the down_data of the element above it (or the seed, bounded by the target's up_data)
    names = [el.name for el in rec.stack]
    for i, el in enumerate(rec.stack):
        if isinstance(el, (deconv_ref.DConv, deconv_ref.DDense)):
            k, _ = c.model.params[el.name]
            w2 = k.reshape(-1, k.shape[-1]).abs().double()
            # conv down: output ci sums taps x co -> rows grouped per ci; the row sum over (kh, kw, co) bounds it
            rows = w2.reshape(9, -1, w2.shape[-1]).sum(dim=(0, 2)).max() if isinstance(el, deconv_ref.DConv) else \
                w2.sum(1).max()
            above = names[i + 1] if i + 1 < len(names) else None
            xin = dmax.get(above, float(ups[el.name].abs().max()))
            xin = max(xin, float(ups[el.name].abs().max()))
            assert xin * float(rows) < 2 ** 24, f"{el.name}: down partial sums not exact in fp32"


@functools.lru_cache(maxsize=None)
def forward(name, layer="predictions"):
    """The oracle's forward through ``layer``: {layer: up_data}, {pool: first-max switch codes u8 [B, PH, PW, C]}.
    Asserts (a) for the up outputs and (e) for every pool input."""
    c = case(name)
    stack = deconv_ref.build_stack(c.model, layer)
    stack[0].up(c.x3)
    for i in range(1, len(stack)):
        stack[i].up(stack[i - 1].up_data)
    outs, codes = {}, {}
    names = {s.name for s in c.specs}
    for i, el in enumerate(stack):
        if el.name not in names or i == 0:
            continue
        outs[el.name] = el.up_data
        if not (el.name == "predictions"):
            _representable(el.up_data, f"{el.name} up")
        if isinstance(el, deconv_ref.DPooling):
            xin = stack[i - 1].up_data
            _check_ties(xin.contiguous())
            N, H, W, C = xin.shape
            sw = el.switch.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
            assert bool((sw.sum(-1) == 1).all())
            codes[el.name] = sw.argmax(-1).to(torch.uint8)
    if "predictions" in outs:
        p = outs["predictions"]
        live = p[:, c.live]
        assert torch.equal(live, torch.full_like(live, 2.0 ** -3)), "live fp64 probabilities are not exactly 2^-3"
        rest = p.clone()
        rest[:, c.live] = 0
        assert float(rest.max()) < 1e-28
        for dt in (torch.bfloat16, torch.float16):  # what the engine stores: 2^-3 on the live units
            assert torch.equal(live.to(dt).double(), live)
    return outs, codes


def _tail_z_representable(c, rec):
    """The fused tail (ops.deconv_tail) stores Z = d . W2^T in bf16: d = block1_conv2.down, W2 the 27 (tap, channel)
    rows of block1_conv1.down. Those sums must be representable too."""
    k, _ = c.model.params["block1_conv1"]  # [3, 3, 3, 64]
    w2 = k.reshape(27, k.shape[-1]).double()
    for name, t in rec.downs:
        if name == "block1_conv2":
            _representable(torch.einsum("nhwc,zc->nhwz", t, w2), "tail Z")


@functools.lru_cache(maxsize=None)
def oracle(name, layer, mode, batch_topk):
    """Expected engine result of one request: recon fp64 [B, K, H, W, 3], filters [B, K], sums [B, K], and
    ``max16``, the largest magnitude the chains store in 16 bits. Conditions (a)-(d) asserted."""
    c = case(name)
    runs = [(c.x3, slice(0, c.B))] if batch_topk == "global" else [(c.x3[b:b + 1], slice(b, b + 1)) for b in range(c.B)]
    hw = c.x3.shape[1]
    recon = torch.zeros(c.B, K, hw, hw, 3, dtype=DT)
    filt = torch.zeros(c.B, K, dtype=torch.int32)
    sums = torch.zeros(c.B, K, dtype=DT)
    max16 = 0.0
    for x3, sl in runs:
        out, rec = _oracle_once(c, x3, layer, mode)
        tgt = next(el for el in rec.stack if el.name == layer)
        top = deconv_ref.find_top_filters(tgt.up_data, K)
        assert len(out) == K and len(top) == K, f"(c) {layer}: the oracle selects {len(out)} filters, not {K}"
        for kk, r in enumerate(out):
            r = torch.as_tensor(r).reshape(-1, hw, hw, 3)
            recon[sl, kk] = r
            filt[sl, kk] = top[kk][0]
            sums[sl, kk] = top[kk][1]
        # (a) every 16-bit store: all down_data but the image (block1_conv1's down and the input element's copy
        # of it), which the engine writes in fp32
        for el_name, t in rec.downs:
            if el_name not in (rec.stack[0].name, rec.stack[1].name):
                _representable(t, f"{layer} chain: {el_name}.down")
                max16 = max(max16, float(t.abs().max()))
        _abs_bound(c, rec)
        if name == "wide":
            _tail_z_representable(c, rec)
    assert float(recon.abs().max()) < 2 ** 24
    # (d) on every reconstruction the oracle returns: with ``global`` one [B, H, W, 3] array per filter (in mode
    # ``max`` an image that does not hold the batch maximum reconstructs to zero BY DEFINITION: the engine must
    # reproduce those zeros), with ``per_image`` one [H, W, 3] array per image and filter
    for kk in range(K):
        for r in ([recon[:, kk]] if batch_topk == "global" else [recon[b, kk] for b in range(c.B)]):
            nz = float((r != 0).double().mean())
            if mode == "all":
                assert nz >= 0.10 and r.unique().numel() >= 16, \
                    f"(d) {layer} filter {kk}: {nz:.3f} non-zero, {r.unique().numel()} values"
            else:
                assert nz > 0, f"(d) {layer} filter {kk}: all zero"
    return types.SimpleNamespace(recon=recon, filters=filt, sums=sums, max16=max16)


def tied_selection(o):
    """(f): two of the selected filters of some image have equal selection sums."""
    return any(len(set(row.tolist())) < K for row in o.sums)


def mosaic_ref(o, b):
    """uint8 mosaic of image b as the reference makes it (channels reversed for the RGB encoder)."""
    recs = [o.recon[b, kk].numpy() for kk in range(K)]
    return np.ascontiguousarray(deconv_ref.deprocess_image(deconv_ref.mosaic(recs))[..., ::-1])
