"""Exact-oracle tests of the guided DeepDream matching kernel (csrc/dream_guide.hip: guide_match, through the
binding and through ops.autograd.guide_core / guide_tap), in the style of test_dream_exact_gpu.py.

Operands are small non-negative integers times a Bernoulli keep mask (post-ReLU-like), so every score
sum_c a[p][c] y[q][c] is an integer below 2^24: exact in fp32 under ANY summation order, the MFMA's included.
The winner (lowest q among the maxima, numpy's argmax), the integer loss and the gradient
addend + scale[n] y[q*] (a > 0) with power-of-two scales are then exactly representable in bf16 and fp16, and the
kernel must equal the CPU reference bit for bit. The conditions that make this hold (and that make the cases
worth running: many distinct winners, many ties in the tie-heavy table) are asserted on the reference alone in
``test_conditions``, without a GPU."""
import functools
import types

import numpy as np
import pytest
import torch

from deconv_api_amd.ops import autograd as AG
from exact_helpers import BF, DEV, HF, _dev, _gen, _ints, _same

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = -77.0
GUARD = 64  # 16-bit / fp32 elements of sentinel on either side of an output (keeps 16-B alignment)

# (N, H, W, C, Q, b): Q below, at and across the 16-row MFMA tile and the 64-row pass, position tails (core sizes
# that are no multiple of 16), more positions than one block's four waves take at once, b = 0, the models' largest C
CASES = [(2, 7, 6, 32, 5, 2), (2, 9, 11, 64, 16, 2), (3, 8, 8, 96, 37, 2), (2, 12, 9, 288, 144, 2),
         (1, 21, 19, 32, 130, 2), (2, 5, 5, 768, 17, 0), (2, 6, 7, 1024, 33, 1)]
TABLES = {"wide": (3, 0.5), "ties": (1, 0.4)}  # values 0..hi, keep probability (ties: + repeated guide rows)
GMODES = ("own", "perm", "shared")  # G = N with gidx = identity / a permutation; G = 1
PARTS = (1, 3, 32)


def _operand(g, shape, hi, keep):
    return _ints(g, shape, 0, hi) * (torch.rand(shape, generator=g) < keep)


@functools.lru_cache(maxsize=None)
def _case(N, H, W, C, Q, b, table, gmode):
    hi, keep = TABLES[table]
    g = _gen(1000 * N + 100 * H + 10 * W + C + Q + b + 7 * len(table) + len(gmode))
    G = 1 if gmode == "shared" else N
    a = _operand(g, (N, H, W, C), hi, keep)
    y = _operand(g, (G, Q, C), hi, keep)
    if table == "ties":
        # with many channels two independent rows rarely score alike (8 - 20 % of the positions tie at C >= 288),
        # so four guide rows in ten repeat another row, anywhere in the table: their scores tie exactly, across
        # registers, lane groups, 16-row tiles and 64-row passes, and the lowest q has to win
        dup = torch.rand(Q, generator=g) < 0.4
        src = torch.randint(0, Q, (Q,), generator=g)
        y[:, dup] = y.clone()[:, src[dup]]
    if gmode == "own":
        gidx = list(range(N))
    elif gmode == "perm":
        gidx = [(n + 1) % N for n in range(N)] if N > 1 else [0]
    else:
        gidx = [0] * N
    scale = torch.tensor([0.5, 0.25, 0.125])[:N].clone()
    addend = _ints(g, (N, H, W, C), -4, 4)
    core = torch.zeros(N, H, W, 1, dtype=torch.bool)
    core[:, b:H - b, b:W - b] = True
    Hc, Wc = H - 2 * b, W - 2 * b
    # the naive reference, in numpy: scores in fp64, argmax = FIRST maximum
    s = np.einsum("npc,nqc->npq", a[:, b:H - b, b:W - b].reshape(N, Hc * Wc, C).double().numpy(),
                  y[gidx].double().numpy())
    win = s.argmax(axis=2)
    best = np.take_along_axis(s, win[..., None], axis=2)[..., 0]
    loss = torch.from_numpy(best.sum(axis=1))
    rows = torch.stack([y[gidx[n]][torch.from_numpy(win[n])] for n in range(N)])  # [N, Pc, C]
    term = torch.zeros(N, H, W, C)
    term[:, b:H - b, b:W - b] = (scale.view(N, 1, 1) * rows).view(N, Hc, Wc, C)
    grads = {False: term, True: term * (a > 0)}
    # ---- the method's conditions, on the reference alone
    assert float(s.max()) < 2 ** 24 and float(loss.max()) < 2 ** 24, "scores / loss not exact in fp32"
    for m in (False, True):
        for out in (grads[m], addend + grads[m]):
            for dt in (BF, HF):
                assert torch.equal(out.to(dt).double(), out.double()), "reference not representable"
    assert bool((grads[True] != grads[False]).any()), "the mask changes nothing"
    assert float(loss.min()) > 0
    assert not bool((addend + term == SENTINEL).any())
    if Q >= 16:
        assert len(np.unique(win)) >= 8, f"only {len(np.unique(win))} distinct winners"
    tied = float(((s == best[..., None]).sum(axis=2) >= 2).mean())
    if table == "ties":
        assert tied >= 0.25, f"only {tied:.2f} of the positions tie"
    return types.SimpleNamespace(a=a, y=y, gidx=gidx, G=G, scale=scale, addend=addend, core=core, loss=loss,
                                 grads=grads, win=win, tied=tied)


def _guarded(shape, dtype):
    """A sentinel-filled tensor of ``shape`` in the middle of a larger sentinel-filled buffer -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf):
    return bool((buf[:GUARD].float() == SENTINEL).all()) and bool((buf[-GUARD:].float() == SENTINEL).all())


@gpu
@dtypes
@pytest.mark.parametrize("gmode", GMODES)
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("N,H,W,C,Q,b", CASES)
def test_exact_guide_match(native_lib, N, H, W, C, Q, b, table, gmode, dt):
    """guide_match through the binding, mask on and off, with and without an addend, 1 / 3 / 32 partials: gx bit
    for bit (border included: the addend's bits, or exactly 0), the integer loss, every gx element written,
    nothing written around gx / part, no input changed, and the forward-only call gives the same partials."""
    c = _case(N, H, W, C, Q, b, table, gmode)
    a, y, scale = _dev(c.a, dt), _dev(c.y, dt), c.scale.to(DEV)
    gidx = AG.guide_index(c.gidx, c.G, DEV)
    add = _dev(c.addend, dt)
    ins = [t.clone() for t in (a, y, scale, gidx, add)]
    border = ~c.core.expand(N, H, W, C).to(DEV)
    for mask in (False, True):
        for addend in (None, add):
            want = c.grads[mask] if addend is None else c.addend + c.grads[mask]
            for P in PARTS:
                gx, gbuf = _guarded((N, H, W, C), dt)
                part, pbuf = _guarded((N, P), torch.float32)
                native_lib.guide_match(a, y, gidx, scale, gx, b, addend, part, mask)
                _same(gx, want)
                if addend is None:
                    assert not bool(gx[border].float().any())
                else:
                    assert torch.equal(gx[border].view(torch.int16), add[border].view(torch.int16))
                assert torch.equal(part.double().sum(1).cpu(), c.loss), (P, part.tolist(), c.loss.tolist())
                assert _guards_intact(gbuf) and _guards_intact(pbuf)
                fwd, fbuf = _guarded((N, P), torch.float32)
                native_lib.guide_match(a, y, gidx, scale, None, b, None, fwd, mask)
                assert torch.equal(fwd, part) and _guards_intact(fbuf), "forward-only partials differ"
            # gradient only (no partials)
            gx, gbuf = _guarded((N, H, W, C), dt)
            native_lib.guide_match(a, y, gidx, scale, gx, b, addend, None, mask)
            _same(gx, want)
            assert _guards_intact(gbuf)
    for t, t0 in zip((a, y, scale, gidx, add), ins):
        assert torch.equal(t, t0), "an input changed"


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,C,Q,b", CASES)
def test_exact_guide_core_and_tap(native_lib, N, H, W, C, Q, b, dt):
    """ops.autograd.guide_core (loss and its gradient, masked exactly when the activation carries the ReLU
    tag) and guide_tap (identity; upstream gradient + loss term in one launch, loss partials on the side)."""
    c = _case(N, H, W, C, Q, b, "ties", "perm")
    y, scale = _dev(c.y, dt), c.scale.to(DEV)
    gidx = AG.guide_index(c.gidx, c.G, DEV)
    for relu in (False, True):
        a = AG.tag_relu_output(_dev(c.a, dt), relu).requires_grad_(True)
        loss = AG.guide_core(a, y, gidx, b)
        assert loss.dtype == torch.float32 and torch.equal(loss.double().cpu(), c.loss)
        (ga,) = torch.autograd.grad(loss, a, scale)
        _same(ga, c.grads[relu])
        part = torch.full((N, 5), SENTINEL, dtype=torch.float32, device=DEV)
        out = AG.guide_tap(a, y, gidx, scale, b, part)
        assert AG._is_relu_out(out) == relu and torch.equal(out.detach(), a.detach())
        (gt,) = torch.autograd.grad(out, a, _dev(c.addend, dt))
        _same(gt, c.addend + c.grads[relu])
        assert torch.equal(part.double().sum(1).cpu(), c.loss)


@gpu
def test_guide_match_refuses_bad_arguments(native_lib):
    """The binding refuses, before any launch: C % 32 != 0, an empty core, more partials than the grid has
    blocks for, a gidx of the wrong dtype or length, y of another dtype or channel count, nothing to write."""
    a = torch.zeros(2, 6, 6, 32, dtype=BF, device=DEV)
    y = torch.zeros(2, 5, 32, dtype=BF, device=DEV)
    gidx = AG.guide_index([0, 1], 2, DEV)
    scale = torch.ones(2, device=DEV)
    gx, part = torch.full_like(a, SENTINEL), torch.full((2, 4), SENTINEL, device=DEV)
    bad = [
        dict(a=torch.zeros(2, 6, 6, 48, dtype=BF, device=DEV), y=torch.zeros(2, 5, 48, dtype=BF, device=DEV),
             gx=torch.zeros(2, 6, 6, 48, dtype=BF, device=DEV)),
        dict(b=3),
        dict(part=torch.zeros(2, 33, device=DEV)),
        dict(gidx=gidx.long()),
        dict(gidx=gidx[:1]),
        dict(y=y.to(HF)),
        dict(y=torch.zeros(2, 5, 64, dtype=BF, device=DEV)),
        dict(gx=None, part=None),
        dict(scale=scale[:1]),
    ]
    for kw in bad:
        args = dict(a=a, y=y, gidx=gidx, scale=scale, gx=gx, b=2, addend=None, part=part, mask=True)
        args.update(kw)
        with pytest.raises(RuntimeError, match="guide_match"):
            native_lib.guide_match(**args)
    torch.cuda.synchronize()
    assert bool((gx.float() == SENTINEL).all()) and bool((part == SENTINEL).all())
    with pytest.raises(ValueError):
        AG.guide_index([0, 2], 2, "cpu")


@pytest.mark.parametrize("table", sorted(TABLES))
def test_conditions(table):
    """Every case of the table, every guide mode: generator, numpy reference and the method's conditions
    (asserted inside the case builder, for bf16 and fp16), without a GPU. The tie-heavy table must tie at
    >= 25 % of the core positions; the wide one carries no tie condition."""
    for case in CASES:
        for gmode in GMODES:
            try:
                _case(*case, table, gmode)
            except AssertionError as e:
                raise AssertionError(f"{table} case {case} {gmode}: {e}") from e


def test_cpu_guide_core_is_the_oracle():
    """The CPU form of guide_core equals the numpy reference: the loss exactly, and autograd's gradient is the
    gathered (unmasked) winner rows - the lowest q on a tie."""
    for case in CASES[:5]:
        c = _case(*case, "ties", "perm")
        b = case[5]
        a = c.a.clone().requires_grad_(True)
        loss = AG.guide_core(a, c.y, AG.guide_index(c.gidx, c.G, "cpu"), b)
        assert torch.equal(loss.double(), c.loss)
        (ga,) = torch.autograd.grad(loss, a, c.scale)
        _same(ga, c.grads[False])
