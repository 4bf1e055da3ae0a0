"""GPU: the hand-written autograd nodes that compose the conv and pool kernels (ops/inception.py
_InceptionFn; ops/autograd.py _BottleneckFn, _ConvFn, _ConvResReluFn) against an EXACT oracle.

The method of test_dream_exact_gpu.py, one level up: every operand is a small integer (weights in [-1, 1]
thinned to a few taps per output, integer biases, x in [0, 3], output gradients in [-1, 1]), so every
activation, every gradient and every partial sum of every launch is an integer that fp32 accumulates exactly
in any order and that bf16 and fp16 store exactly. A correct node therefore reproduces a plain fp64
interpreter of the UNFUSED topology (F.conv2d, F.avg_pool2d(count_include_pad=False), F.max_pool2d,
torch.cat, relu; gradients by torch.autograd.grad on the CPU) bit for bit, forward and backward: one wrong
border divisor of the commuted pool branch, one mis-sliced 8-channel group, one mask taken as >= 0, one
contribution written where it should accumulate shows, however small it is next to the rest.

The avg-pool branch divides by 4, 6 and 9 (the kernel multiplies by 1.f / count), so what it averages must
be multiples of 36. They live in dedicated input channels: the last 32 channels ``P`` of x hold 36 * {0..3},
the pool branch's 1x1 unit has +-1 weights on P only (at most two per output), every other unit that reads x
has zero weight on P, and the pool slice of gY is 36 * {-1, 0, 1}.

Every case is built by a cached ``_*_case`` function that draws the operands, computes the reference and
asserts the method's conditions on the reference ALONE: representability of every intermediate (1), partial
sums of every accumulated tensor bounded by 256 (2), fp32 exactness of every conv (3), density (4), ReLU
pre-activations that are exactly 0 and zeros in x (5), tied max-pool windows (6), and that the oracle tells
the listed mutants of the reference apart (7). ``test_conditions`` (no GPU) builds every case of every table.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd.models.inception_v3 import InceptionV3
from deconv_api_amd.ops import autograd as AG
from deconv_api_amd.ops import inception
from exact_helpers import BF, DEV, HF, _dev, _gen, _ints, _recip_exact, _representable, _same, _tap_weights
from gpu_helpers import cus as _cus, route as _route

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
modes = pytest.mark.parametrize("premasked", [False, True], ids=["plain", "premasked"])

NP = 32  # the channels P of x that carry the avg branch's multiples of 36
CIN = [192, 256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048]  # input channels of mixed0 .. mixed10
TAPS = 6  # non-zero taps per output of the block units


def _case(**kw):
    return types.SimpleNamespace(**kw)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _frac(mask):
    return float(mask.double().mean()) if mask.numel() else 0.0


def _differs(a, b):
    return a.shape != b.shape or not torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _net():
    """The topology (branch programs, unit shapes, strides, pads); the cases overwrite the units' weights."""
    return InceptionV3(0)


# ----------------------------------------------------------------------------------------
# the reference: an fp64 interpreter of the unfused branch programs
# ----------------------------------------------------------------------------------------

def _relu_of(mut):
    """ReLU; as the mutant ``ge`` with the derivative 1 at a pre-activation of exactly 0 (a mask taken >= 0)."""
    return (lambda t: t * (t >= 0)) if "ge" in mut else torch.relu


def _max_last(t):
    """3x3 / 2 max-pool whose gradient goes to the LAST tied maximum of a window (F.max_pool2d: the first)."""
    N, C, H, W = t.shape
    win = F.unfold(t, 3, stride=2).view(N, C, 9, -1)
    top = win.max(dim=2, keepdim=True).values
    last = torch.where(win == top, torch.arange(9).view(1, 1, 9, 1), -1).max(dim=2, keepdim=True).values
    return win.gather(2, last).view(N, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1)


def _interp(prog, Wd, x, mut=(), drop=None):
    """Branch outputs (NCHW, Keras order) of the block ``prog`` = (order, branches) on x (NHWC, fp64) with the
    units Wd[name] = (w, b, stride, pad), and every unit's input, pre-activation and output by name.
    Mutants: ``pad`` (count_include_pad=True), ``ge``, ``last`` (max-pool ties), ``relu_cols`` (the commuted
    pool branch with ReLU on its first 8 columns of T before the average); ``drop``: a unit without gradient."""
    order, br = prog
    relu, nodes = _relu_of(mut), {}

    def conv(n, t):
        w, b, s, p = Wd[n]
        pre = F.conv2d(t, w, b, stride=s, padding=p)
        nodes[n + ".in"], nodes[n + ".pre"] = t, (pre.detach() if n == drop else pre)
        nodes[n] = relu(nodes[n + ".pre"])
        return nodes[n]

    outs = []
    for k in order:
        t = _nchw(x)
        if br[k][0] == "avg" and "relu_cols" in mut:
            w, b, _, _ = Wd[br[k][1]]
            t = F.conv2d(t, w)
            t = F.avg_pool2d(torch.cat([t[:, :8].relu(), t[:, 8:]], 1), 3, 1, 1, count_include_pad=False)
            outs.append(relu(t + b.view(1, -1, 1, 1)))
            continue
        for op in br[k]:
            if op == "avg":
                nodes[k + ".avg"] = t = F.avg_pool2d(t, 3, 1, 1, count_include_pad="pad" in mut)
            elif op == "max":
                t = _max_last(t) if "last" in mut else F.max_pool2d(t, 3, 2, 0)
            elif isinstance(op, tuple):
                t = torch.cat([conv(op[1], t), conv(op[2], t)], 1)
            else:
                t = conv(op, t)
        outs.append(t)
    return outs, nodes


def _conv_bounds(w, a, g):
    """Condition 3 for one conv: sum |a| |w| of its forward (input a) and of its input gradient (output
    gradient g), each bounded by the largest operand times the largest absolute row / column sum of w."""
    fwd = float(a.detach().abs().max()) * float(w.abs().sum(dim=(1, 2, 3)).max())
    bwd = float(g.detach().abs().max()) * float(w.abs().sum(dim=(0, 2, 3)).max())
    assert fwd + 256 < 2 ** 24 and bwd + 256 < 2 ** 24, "partial sums not exact in fp32"


def _zeros_at_relu(pre, what):
    assert _frac(pre == 0) >= 0.02, f"{what}: too few pre-activations are exactly 0"


# ----------------------------------------------------------------------------------------
# 1. Inception blocks
# ----------------------------------------------------------------------------------------

# (block, H, W): non-square maps; the reduction blocks on odd and even maps (parity classes of unequal
# size); mixed4 with a side shorter than its 7-tap kernels
BLOCK_CASES = [(0, 9, 11), (3, 11, 9), (3, 10, 12), (4, 5, 9), (5, 9, 7), (8, 9, 7), (8, 8, 10), (9, 5, 6)]


def _unit_names(ops):
    for op in ops:
        if isinstance(op, tuple):
            yield from op[1:]
        elif op not in ("avg", "max"):
            yield op


def _pool_weights(g, oc, cin):
    """The pool branch's 1x1 unit: +-1 on one or two of the channels P per output, zero elsewhere."""
    w = torch.zeros(oc, cin, 1, 1)
    signs = torch.tensor([[1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, 0.0]])
    for o in range(oc):
        ch = torch.randperm(NP, generator=g)[:2] + (cin - NP)
        w[o, ch, 0, 0] = signs[int(torch.randint(0, 4, (1,), generator=g))]
    return w


def _is_head(shape, stride, pad):
    return tuple(shape[2:]) == (1, 1) and stride == 1 and tuple(pad) == (0, 0)


def _block_grads(c, gY, premasked, mut=(), drop=None):
    """Reference gradient of the block input for the output gradient gY (NHWC): the plain gradient, or
    under the premasked contract the gradient times (x > 0)."""
    xg = c.x.double().requires_grad_(True)
    outs, _ = _interp(c.prog, c.Wd, xg, mut, drop)
    (gx,) = torch.autograd.grad(torch.cat(outs, 1), xg, _nchw(gY.double()))
    if premasked:
        gx = gx * ((c.x >= 0) if "ge" in mut else (c.x > 0))
    return gx


@functools.lru_cache(maxsize=None)
def _block_case(bi, H, W):
    net = _net()
    name, order, br = net.blocks[bi]
    prog = (order, br)
    cin, N = CIN[bi], 2
    g = _gen(1000 * bi + 10 * H + W)
    has_avg = any(ops[0] == "avg" for ops in br.values())
    live = cin - NP if has_avg else cin
    Wt, heads, pool_unit = {}, [], None
    for k in order:
        for j, n in enumerate(_unit_names(br[k])):
            u = net.units[n]
            oc, c_in, kh, kw = u.w.shape
            if br[k][0] == "avg":
                pool_unit = n
                Wt[n] = (_pool_weights(g, oc, c_in), 12 * _ints(g, (oc,), -1, 1), u.stride, u.pad)
            else:
                on_x = j == 0
                assert c_in == cin if on_x else True
                Wt[n] = (_tap_weights(g, oc, c_in, kh, kw, TAPS, live=live if on_x else None), _ints(g, (oc,), -1, 1),
                         u.stride, u.pad)
                if on_x and len(br[k]) > 1 and _is_head(u.w.shape, u.stride, u.pad):
                    heads.append(n)
    x = _ints(g, (N, H, W, cin), 0, 3)
    if has_avg:
        x[..., live:] *= 36
    Wd = {n: (w.double(), b.double(), s, p) for n, (w, b, s, p) in Wt.items()}
    c = _case(bi=bi, name=name, H=H, W=W, prog=prog, Wt=Wt, Wd=Wd, x=x, has_avg=has_avg, live=live, gY={}, gx={})
    members = len(heads) + (pool_unit is not None)
    c.relu_cols = sum(Wt[n][0].shape[0] for n in heads) if members >= 2 else None  # None: no merged head GEMM
    c.b1 = next((br[k][0] for k in order if len(br[k]) == 1 and br[k][0] != "max" and
                 _is_head(Wt[br[k][0]][0].shape, *Wt[br[k][0]][2:])), None) if members >= 2 else None

    # ---- forward: Y, its slices, every intermediate
    xg = x.double().requires_grad_(True)
    outs, nodes = _interp(prog, Wd, xg)
    Y = _nhwc(torch.cat(outs, 1).detach())
    c.Y = Y
    widths = [o.shape[1] for o in outs]
    offs = [sum(widths[:i]) for i in range(len(widths))]
    for n, t in nodes.items():
        # (the unfused average of x is a fraction on the channels that no pool weight reads: never computed)
        _representable(t[:, live:] if n.endswith(".avg") or n == f"{pool_unit}.in" else t, f"{name} {n}")
    _representable(Y, "Y")
    assert _frac(x == 0) >= 0.15, "too few zeros in x"
    for k, o in zip(order, outs):
        assert _frac(o != 0) >= 0.25, f"{name} branch {k}: too few non-zero outputs ({_frac(o != 0):.3f})"
    for n in Wt:
        _zeros_at_relu(nodes[n + ".pre"], f"{name} {n}")
    cnt = F.avg_pool2d(torch.ones(1, 1, H, W), 3, 1, 1, divisor_override=1)
    if has_avg:  # the commuted pool columns of T: x @ W_pool without bias, averaged, then bias (+ ReLU)
        w, b, _, _ = Wt[pool_unit]
        T_pool = F.conv2d(_nchw(x), w)
        _representable(T_pool, "pool columns of T")
        avg = _recip_exact(F.avg_pool2d(T_pool, 3, 1, 1, divisor_override=1), cnt)
        assert torch.equal(avg.double() + b.double().view(1, -1, 1, 1), nodes[pool_unit + ".pre"].detach())
        assert bool((T_pool[:, :8] < 0).any())
    if ["max"] in br.values():
        win = F.unfold(_nchw(x), 3, stride=2).view(N, cin, 9, -1)
        assert _frac((win == win.max(dim=2, keepdim=True).values).sum(dim=2) >= 2) >= 0.05, "too few tied windows"

    # ---- forward mutants
    if has_avg:
        for mut in ("pad", "relu_cols"):
            outs_m, _ = _interp(prog, Wd, x.double(), (mut,))
            assert _differs(_nhwc(torch.cat(outs_m, 1)), Y), f"{name}: the forward oracle misses the mutant {mut}"

    # ---- backward, without and with the premasked contract
    gY0 = _ints(g, Y.shape, -1, 1)
    if has_avg:
        po = offs[[br[k][0] for k in order].index("avg")]
        gY0[..., po:] *= 36
    keys = sorted(nodes)
    Ycat = torch.cat(outs, 1)
    for pm in (False, True):
        gY = gY0 * (Y > 0) if pm else gY0
        xmask = (x > 0) if pm else torch.ones_like(x, dtype=torch.bool)
        grads = torch.autograd.grad(Ycat, [xg] + [nodes[k] for k in keys], _nchw(gY.double()), retain_graph=True)
        gx_plain, gn = grads[0], dict(zip(keys, grads[1:]))
        gx = gx_plain * xmask
        c.gY[pm], c.gx[pm] = gY, gx
        assert torch.equal(gx, _block_grads(c, gY, pm))
        _representable(gx, "gx")
        _representable(gx_plain, "gx before the x mask")
        for n, t in gn.items():
            _representable(t, f"{name} gradient of {n}")
        for n, (w, b, s, p) in Wd.items():
            _conv_bounds(w, nodes[n + ".in"], gn[n + ".pre"])
        # each branch's own contribution to gx; the partial sums of gx in any order
        total = torch.zeros_like(gx)
        for k, o, off, wd in zip(order, outs, offs, widths):
            (cb,) = torch.autograd.grad(o, xg, _nchw(gY.double())[:, off:off + wd], retain_graph=True)
            _representable(cb, f"{name} contribution of {k}")
            total += cb.abs()
            sup = torch.zeros_like(x, dtype=torch.bool)
            first = br[k][0]
            strided = first == "max" or (isinstance(first, str) and first != "avg" and Wt[first][2] > 1)
            rows, cols = (((H - 3) // 2) * 2 + 3, ((W - 3) // 2) * 2 + 3) if strided else (H, W)
            sup[:, :rows, :cols, live:] = first == "avg"
            sup[:, :rows, :cols, :live] = first != "avg"
            assert _frac(cb[sup & xmask] != 0) >= 0.02, f"{name} contribution of {k} too sparse"
            assert _differs((gx_plain - cb) * xmask, gx), f"{name}: the oracle misses the dropped branch {k}"
        assert float(total.max()) <= 256, "partial sums of gx not representable"
        assert _frac(gx[xmask] != 0) >= 0.15, "too few non-zero gradients"
        # G_T: the heads' columns are the gradients of their pre-activations (checked above); the pool
        # columns are the avg-pool gradient of the pool unit's pre-activation gradient
        if has_avg:
            gp = gn[pool_unit + ".pre"]
            _recip_exact(gp, cnt)
            t0 = torch.zeros_like(gp, requires_grad=True)
            (gt,) = torch.autograd.grad(F.avg_pool2d(t0, 3, 1, 1, count_include_pad=False), t0, gp)
            _representable(gt, "pool columns of G_T")
            assert torch.equal(gt, gt.round())
        # a split pair's two input gradients accumulate into one gi
        pairs = [op for ops in br.values() for op in ops if isinstance(op, tuple)]
        for _, a, b2 in pairs:
            inp = nodes[a + ".in"]
            parts = [torch.autograd.grad(nodes[n + ".pre"], inp, gn[n + ".pre"], retain_graph=True)[0] for n in (a, b2)]
            for t in parts:
                _representable(t, f"{name} split gradient")
            assert float((parts[0].abs() + parts[1].abs()).max()) <= 256, "partial sums of a split's gi"
        # ---- backward mutants
        muts = [((m,), None) for m, on in (("pad", has_avg), ("ge", True), ("last", ["max"] in br.values())) if on]
        muts += [((), b2) for _, _, b2 in pairs]
        for mut, drop in muts:
            assert _differs(_block_grads(c, gY, pm, mut, drop), gx), f"{name}: the oracle misses the mutant {mut} {drop}"
        for off, wd in zip(offs, widths):  # one branch's slice of gY read 8 channels further on
            gYs = gY.clone()
            gYs[..., off:off + wd] = torch.roll(gY, -8, dims=3)[..., off:off + wd]
            (gs,) = torch.autograd.grad(Ycat, xg, _nchw(gYs.double()), retain_graph=True)
            assert _differs(gs * xmask, gx), f"{name}: the oracle misses a slice shifted by 8 channels at {off}"
    del c.Wd  # (the fp64 copies served the conditions; the GPU tests build their units from Wt)
    return c


# (block, H, W, variant): ``direct`` / ``subpixel`` force the two strided-dgrad forms of the reduction
# blocks, ``no_b1`` keeps the b1 branch out of the merged head GEMM
BLOCK_RUNS = [(bi, H, W, v) for bi, H, W in BLOCK_CASES
              for v in (("default", "direct", "subpixel") if bi in (3, 8) else
                        ("default", "no_b1") if bi in (0, 4, 9) else ("default",))]


@gpu
@dtypes
@modes
@pytest.mark.parametrize("bi,H,W,variant", BLOCK_RUNS, ids=[f"mixed{b}-{h}x{w}-{v}" for b, h, w, v in BLOCK_RUNS])
def test_exact_inception_block(native_lib, monkeypatch, bi, H, W, variant, premasked, dt):
    """_InceptionFn forward and backward: the merged head GEMM with relu_cols, b1 through out2 / split_col
    into its concat slice (and on its own GEMM), the commuted pool branch, level-ordered conv groups,
    first-write / accumulate order into gx with the x mask fused into the last contribution, the G_T dgrad
    GEMM and both strided-dgrad forms, bit for bit against the fp64 interpreter."""
    c = _block_case(bi, H, W)
    if variant in ("direct", "subpixel"):
        monkeypatch.setattr(AG, "STRIDED_DIRECT_FLOPS", 1e30 if variant == "direct" else 0.0)
    if variant == "no_b1":
        monkeypatch.setattr(inception, "MERGE_B1", False)
    net = _net()
    blk = net.iblocks[bi]
    for n, (w, b, _, _) in c.Wt.items():
        u = net.units[n]
        u.w, u.b = w.clone(), b.clone()
        u.build(DEV, dt)
    blk.build(DEV, dt)
    if c.relu_cols is None:
        assert blk.merge is None and blk.merge_b1 is None
    else:
        assert blk.merge is not None and blk.merge[2] == c.relu_cols
        if c.b1 is None or variant == "no_b1":
            assert blk.merge_b1 is None
        else:
            n1 = c.Wt[c.b1][0].shape[0]
            assert blk.merge_b1 is not None and blk.merge_b1[1] == n1 and blk.merge_b1[3] == n1 + c.relu_cols
    xd = _dev(c.x, dt).requires_grad_(True)
    if premasked:
        with AG.premasked_grads():
            Y = blk(AG.tag_relu_output(xd))
    else:
        Y = blk(xd)
    assert Y.dtype == dt and AG._is_relu_out(Y)
    if variant in ("direct", "subpixel"):
        strided = [net.units[n] for n in c.Wt if net.units[n].stride > 1]
        assert strided and all(AG.strided_direct(u, Y, (H, W)) == (variant == "direct") for u in strided)
    _same(Y, c.Y)
    (gx,) = torch.autograd.grad(Y, xd, _dev(c.gY[premasked], dt))
    assert gx.dtype == dt
    _same(gx, c.gx[premasked])


# ----------------------------------------------------------------------------------------
# 2. ResNet bottleneck
# ----------------------------------------------------------------------------------------

BNECK_CASES = [(1, False), (1, True), (2, True)]  # (stride, projection shortcut)


def _bneck_units(g, cin, width, cout, stride, proj, taps=(6, 6, 4, 3)):
    """(w, b, stride, pad, relu) of c1, c2, c3 and the shortcut (None: identity)."""
    mk = lambda ci, co, k, s, relu, t: (_tap_weights(g, co, ci, k, k, t), _ints(g, (co,), -1, 1), s, k // 2, relu)  # noqa: E731
    return [mk(cin, width, 1, stride, True, taps[0]), mk(width, width, 3, 1, True, taps[1]),
            mk(width, cout, 1, 1, False, taps[2]), mk(cin, cout, 1, stride, False, taps[3]) if proj else None]


def _bneck_graph(blocks, x, mut=()):
    """fp64 chain of unfused bottlenecks y = relu(c3(relu(c2(relu(c1(t))))) + shortcut(t)) on x (NHWC)."""
    relu, nodes = _relu_of(mut), {}
    conv = lambda t, u: F.conv2d(t, u[0].double(), u[1].double(), stride=u[2], padding=u[3])  # noqa: E731
    t = _nchw(x)
    for i, (c1, c2, c3, sh) in enumerate(blocks):
        nd = {"in": t}
        nd["p1"] = conv(t, c1)
        nd["y1"] = relu(nd["p1"])
        nd["p2"] = conv(nd["y1"], c2)
        nd["y2"] = relu(nd["p2"])
        nd["sc"] = t if sh is None else conv(t, sh)
        nd["p3"] = conv(nd["y2"], c3) + nd["sc"]
        nd["y"] = t = relu(nd["p3"])
        nodes.update({f"{i}.{k}": v for k, v in nd.items()})
    return t, nodes


def _bneck_check(blocks, x, g):
    """Reference and conditions of a chain of bottlenecks; returns y (NHWC), gy and gx for both contracts."""
    xg = x.double().requires_grad_(True)
    y, nodes = _bneck_graph(blocks, xg)
    for n, t in nodes.items():
        _representable(t, n)
    assert _frac(x == 0) >= 0.15, "too few zeros in x"
    assert _frac(y != 0) >= 0.25, "too few non-zero outputs"
    for i in range(len(blocks)):
        for p in ("p1", "p2", "p3"):
            _zeros_at_relu(nodes[f"{i}.{p}"], f"block {i} {p}")
    stride = blocks[0][0][2]
    sup = torch.zeros_like(x, dtype=torch.bool)
    sup[:, ::stride, ::stride] = True
    yd = _nhwc(y.detach())
    gy0 = _ints(g, yd.shape, -1, 1)
    keys = sorted(nodes)
    out = _case(y=yd, gy={}, gx={})
    for pm in (False, True):
        gy = gy0 * (yd > 0) if pm else gy0
        xmask = (x > 0) if pm else torch.ones_like(x, dtype=torch.bool)
        grads = torch.autograd.grad(y, [xg] + [nodes[k] for k in keys], _nchw(gy.double()), retain_graph=True)
        gx_plain, gn = grads[0], dict(zip(keys, grads[1:]))
        gx = gx_plain * xmask
        _representable(gx, "gx")
        _representable(gx_plain, "gx before the x mask")
        for n, t in gn.items():
            _representable(t, f"gradient of {n}")
        for i, (c1, c2, c3, sh) in enumerate(blocks):
            for u, a, gr in ((c1, "in", "p1"), (c2, "y1", "p2"), (c3, "y2", "p3")) + (((sh, "in", "p3"),) if sh else ()):
                _conv_bounds(u[0], nodes[f"{i}.{a}"], gn[f"{i}.{gr}"])
            # the block's input gradient (E at the strided pixels): c1's part plus the shortcut's, accumulated
            inp = nodes[f"{i}.in"]
            (part,) = torch.autograd.grad(nodes[f"{i}.p1"], inp, gn[f"{i}.p1"], retain_graph=True)
            full = gx_plain if i == 0 else gn[f"{i}.in"]
            full = _nchw(full) if i == 0 else full
            _representable(part, "c1's part of the input gradient")
            assert float((part.abs() + (full - part).abs()).max()) <= 256, "partial sums of the input gradient"
            assert bool(part.any()) and bool((full - part).any())
        assert _frac(gx[sup & xmask] != 0) >= 0.15, "too few non-zero gradients"
        xq = x.double().requires_grad_(True)
        ym, _ = _bneck_graph(blocks, xq, ("ge",))
        (gm,) = torch.autograd.grad(ym, xq, _nchw(gy.double()))
        assert _differs(gm, gx), "the oracle misses masks taken as >= 0"
        out.gy[pm], out.gx[pm] = gy, gx
    return out


@functools.lru_cache(maxsize=None)
def _bneck_case(stride, proj):
    g = _gen(40 + 10 * stride + proj)
    units = _bneck_units(g, 64, 16, 64, stride, proj)
    x = _ints(g, (2, 8, 10, 64), 0, 3)
    c = _bneck_check([units], x, g)
    c.units, c.x = units, x
    return c


def _chain_m(G):
    """Rows as test_conv_routes_exact_gpu.py _pw_m sizes them for the 256-column convs (the ones that write
    and read the mask handed from block to block): about 2.25 128 x 128 tiles per CU with an M tail."""
    tiles_m = 9 * G // (4 * 2) + 1
    Wd = ((tiles_m - 1) * 128 + 64) // 61
    M = 61 * Wd
    assert 2 * G < -(-M // 128) * 2 < 4 * G and M % 128 != 0
    return 61, Wd


@functools.lru_cache(maxsize=None)
def _chain_case(G):
    g = _gen(77)
    blocks = [_bneck_units(g, 256, 64, 256, 1, False, taps=(6, 6, 2, 0)) for _ in range(2)]
    H, Wd = _chain_m(G)
    x = _ints(g, (1, H, Wd, 256), 0, 3)
    c = _bneck_check(blocks, x, g)
    c.blocks, c.x = blocks, x
    return c


def _cu_count():
    """The CU count that sizes the chain case: the device's, or an MI355X's 256 where there is no GPU."""
    return _cus() if torch.cuda.is_available() else 256


def _build_units(units, dt):
    return [None if u is None else AG.ConvUnit(f"c{i}", u[0], u[1], u[2], (u[3], u[3]), relu=u[4]).build(DEV, dt)
            for i, u in enumerate(units)]


@gpu
@dtypes
@modes
@pytest.mark.parametrize("stride,proj", BNECK_CASES)
def test_exact_bottleneck(native_lib, stride, proj, premasked, dt):
    """_BottleneckFn at cin 64 / width 16 / out 64 on an 8 x 10 map: identity and projection shortcuts, and
    the stride-2 block whose two 1x1 input gradients accumulate into one E before subpixel_scatter."""
    c = _bneck_case(stride, proj)
    units = _build_units(c.units, dt)
    if stride == 2:
        assert AG._pw_strided(units[0]) and AG._pw_strided(units[3])
    xd = _dev(c.x, dt).requires_grad_(True)
    if premasked:
        with AG.premasked_grads():
            y = AG.bottleneck(AG.tag_relu_output(xd), *units)
    else:
        y = AG.bottleneck(xd, *units)
    assert y.dtype == dt and AG._is_relu_out(y)
    _same(y, c.y)
    (gx,) = torch.autograd.grad(y, xd, _dev(c.gy[premasked], dt))
    _same(gx, c.gx[premasked])


@gpu
@dtypes
@pytest.mark.parametrize("bits", [True, False], ids=["bits", "nobits"])
def test_exact_bottleneck_chain(native_lib, monkeypatch, bits, dt):
    """Two chained identity bottlenecks (cin 256 / width 64, premasked) on a map that puts the 256-column
    1x1 convs on the persistent kernel: the second block's input gradient masked by the first block's 1-bit
    mask, and by its 16-bit output (RELU_BITS off), each against the CPU reference."""
    c = _chain_case(_cus())
    monkeypatch.setattr(AG, "RELU_BITS", bits)
    blocks = [_build_units(u, dt) for u in c.blocks]
    xd = _dev(c.x, dt).requires_grad_(True)
    with AG.premasked_grads():
        y = AG.bottleneck(AG.tag_relu_output(xd), *blocks[0])
        assert _route() == "pw 128x128", _route()
        assert (getattr(y, "_dv_bits", None) is not None) == bits
        z = AG.bottleneck(y, *blocks[1])
    _same(z, c.y)
    (gx,) = torch.autograd.grad(z, xd, _dev(c.gy[True], dt))
    assert _route() == "pw 128x128", _route()
    _same(gx, c.gx[True])


# ----------------------------------------------------------------------------------------
# 3. conv units
# ----------------------------------------------------------------------------------------

# (k, stride, pad, cin, cout)
CONV_GEOMS = [(3, 2, 0, 32, 64), (3, 2, 1, 32, 64), (1, 2, 0, 64, 128), (5, 1, 2, 48, 64)]
CONV_CASES = [geom + (relu,) for geom in CONV_GEOMS for relu in (False, True)]


@functools.lru_cache(maxsize=None)
def _conv_case(k, s, p, cin, cout, relu):
    g = _gen(100 * k + 10 * s + p + cin + relu)
    w, b = _tap_weights(g, cout, cin, k, k, 8), _ints(g, (cout,), -1, 1)
    x = _ints(g, (2, 9, 11, cin), 0, 3)
    c = _case(w=w, b=b, x=x, gy={}, gx={})
    assert _frac(x == 0) >= 0.15

    def run(gy, pm, mut=()):
        xg = x.double().requires_grad_(True)
        pre = F.conv2d(_nchw(xg), w.double(), b.double(), stride=s, padding=p)
        y = _relu_of(mut)(pre) if relu else pre
        if gy is None:
            return pre.detach(), _nhwc(y.detach())
        (gx,) = torch.autograd.grad(y, xg, _nchw(gy.double()))
        return gx * ((x >= 0) if "ge" in mut else (x > 0)) if pm else gx

    pre, c.y = run(None, False)
    _representable(c.y)
    assert _frac(c.y != 0) >= 0.25
    if relu:
        _zeros_at_relu(pre, "conv unit")
    ones = torch.ones(1, 1, 9, 11, requires_grad=True)
    (cov,) = torch.autograd.grad(F.conv2d(ones, torch.ones(1, 1, k, k), stride=s, padding=p).sum(), ones)
    cov = (cov > 0).view(1, 9, 11, 1).expand_as(x)
    gy0 = _ints(g, c.y.shape, -1, 1)
    for pm in (False, True):
        gy = gy0 * (c.y > 0) if (pm and relu) else gy0
        gx = run(gy, pm)
        _representable(gx, "gx")
        _representable(run(gy, False), "gx before the x mask")
        _conv_bounds(w, x, gy)
        assert _frac(gx[cov & ((x > 0) if pm else (x >= 0))] != 0) >= 0.15, "too few non-zero gradients"
        if relu or pm:
            assert _differs(run(gy, pm, ("ge",)), gx), "the oracle misses masks taken as >= 0"
        c.gy[pm], c.gx[pm] = gy, gx
    return c


@gpu
@dtypes
@modes
@pytest.mark.parametrize("k,s,p,cin,cout,relu", CONV_CASES)
def test_exact_conv_unit(native_lib, k, s, p, cin, cout, relu, premasked, dt):
    """_ConvFn forward and backward through ConvUnit on a 9 x 11 map: the sub-pixel input gradients of
    3x3 / 2 (pad 0 and 1) and 1x1 / 2 convs and a stride-1 5x5, with and without the unit's ReLU, the
    A-operand mask outside the premasked contract and the x mask inside it."""
    c = _conv_case(k, s, p, cin, cout, relu)
    u = AG.ConvUnit("u", c.w, c.b, s, (p, p), relu=relu).build(DEV, dt)
    xd = _dev(c.x, dt).requires_grad_(True)
    if premasked:
        with AG.premasked_grads():
            y = u(AG.tag_relu_output(xd))
    else:
        y = u(xd)
    assert y.dtype == dt and AG._is_relu_out(y) == relu
    _same(y, c.y)
    (gx,) = torch.autograd.grad(y, xd, _dev(c.gy[premasked], dt))
    assert gx.dtype == dt
    _same(gx, c.gx[premasked])


RES_CASES = [(1, 64, 64), (3, 32, 64)]  # (k, cin, cout)


@functools.lru_cache(maxsize=None)
def _res_case(k, cin, cout):
    g = _gen(300 + k + cin)
    w, b = _tap_weights(g, cout, cin, k, k, 8), _ints(g, (cout,), -1, 1)
    x, sc = _ints(g, (2, 9, 11, cin), 0, 3), _ints(g, (2, 9, 11, cout), -2, 2)
    c = _case(w=w, b=b, x=x, sc=sc)

    def run(gy, mut=()):
        xg, sg = x.double().requires_grad_(True), sc.double().requires_grad_(True)
        pre = F.conv2d(_nchw(xg), w.double(), b.double(), padding=k // 2) + _nchw(sg)
        y = _relu_of(mut)(pre)
        return (pre.detach(), _nhwc(y.detach())) if gy is None else torch.autograd.grad(y, [xg, sg], _nchw(gy.double()))

    pre, c.y = run(None)
    _representable(c.y)
    assert _frac(c.y != 0) >= 0.25
    _zeros_at_relu(pre, "conv_res_relu")
    c.gy = _ints(g, c.y.shape, -1, 1)
    c.gx, c.gsc = run(c.gy)
    _representable(c.gx, "gx")
    _conv_bounds(w, x, c.gy)
    assert _frac(c.gx != 0) >= 0.15 and _frac(c.gsc != 0) >= 0.15
    gxm, gsm = run(c.gy, ("ge",))
    assert _differs(gxm, c.gx) and _differs(gsm, c.gsc), "the oracle misses masks taken as >= 0"
    return c


@gpu
@dtypes
@pytest.mark.parametrize("k,cin,cout", RES_CASES)
def test_exact_conv_res_relu(native_lib, k, cin, cout, dt):
    """_ConvResReluFn: ReLU(conv(x) + bias + sc) in one epilogue; backward, the masked gradient is the
    shortcut's gradient and the operand of the conv's input gradient."""
    c = _res_case(k, cin, cout)
    u = AG.ConvUnit("u", c.w, c.b, 1, (k // 2, k // 2), relu=False).build(DEV, dt)
    xd, sd = _dev(c.x, dt).requires_grad_(True), _dev(c.sc, dt).requires_grad_(True)
    y = AG.conv_res_relu(xd, sd, u)
    assert y.dtype == dt
    _same(y, c.y)
    gx, gs = torch.autograd.grad(y, [xd, sd], _dev(c.gy, dt))
    _same(gx, c.gx)
    _same(gs, c.gsc)


# ----------------------------------------------------------------------------------------
# the conditions of every case, on the CPU alone
# ----------------------------------------------------------------------------------------

CASE_TABLES = {
    "inception_block": (_block_case, BLOCK_CASES),
    "bottleneck": (_bneck_case, BNECK_CASES),
    "bottleneck_chain": (lambda: _chain_case(_cu_count()), [()]),
    "conv_unit": (_conv_case, CONV_CASES),
    "conv_res_relu": (_res_case, RES_CASES),
}


@pytest.mark.parametrize("table", sorted(CASE_TABLES))
def test_conditions(table):
    """Every case of every table: operands, fp64 reference and the method's conditions 1 - 7 (asserted inside
    the case builders, for bf16 and fp16), without a GPU."""
    build, cases = CASE_TABLES[table]
    assert cases
    for case in cases:
        try:
            build(*case)
        except AssertionError as e:
            raise AssertionError(f"{table} case {case}: {e}") from e
