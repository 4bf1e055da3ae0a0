"""Guided DeepDream through the serving layers (CPU engine): POST /deepdream's ``guide`` field, its 400s, the
front-end relay (serve/frontend.py RemoteDream -> serve/ingest.py -> DreamService) and ``cli dream --guide``."""
from __future__ import annotations

import asyncio
import base64
import io
import json
import os
import subprocess
import sys
import tempfile
import threading
from urllib.parse import quote_plus, unquote

import numpy as np
import pytest
from PIL import Image

from deconv_api_amd.api.app import create_app
from deconv_api_amd.config import Config
from deconv_api_amd.serve import ingest as I
from deconv_api_amd.serve.dream_service import DreamService
from deconv_api_amd.serve.frontend import RemoteDream

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _png(h, w, seed) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, format="PNG")
    return buf.getvalue()


def _url(png: bytes) -> str:
    return "data:image/png;base64," + base64.b64encode(png).decode()


FILE, GUIDE = _png(80, 80, 1), _png(60, 90, 2)


@pytest.fixture(scope="module")
def svc():
    ds = DreamService(Config.from_env(device="cpu", hip_graphs=False, dream_window_ms=0.0, dream_tile=128))
    yield ds
    ds.close()


@pytest.fixture(scope="module")
def client(svc):
    from fastapi.testclient import TestClient

    with TestClient(create_app(None, svc.cfg, dream_service=svc)) as c:
        yield c


def _dream(c, **fields):
    body = "&".join(f"{k}={quote_plus(v)}" for k, v in fields.items()).encode()
    return c.post("/deepdream", content=body, headers={"content-type": "application/x-www-form-urlencoded"})


def _jpeg(url: str) -> bytes:
    assert url.startswith("data:image/")
    return base64.b64decode(unquote(url.split(",", 1)[1]))


@pytest.fixture(scope="module")
def answers(client):
    """The route's answers for FILE, unguided and guided (1 octave, 1 step), shared by the tests below."""
    plain = _dream(client, file=_url(FILE), octaves="1", steps="1")
    guided = _dream(client, file=_url(FILE), octaves="1", steps="1", guide=_url(GUIDE))
    assert plain.status_code == 200 and guided.status_code == 200, (plain.text[:300], guided.text[:300])
    return plain.json(), guided.json()


def test_route_guide_changes_the_answer(client, answers):
    plain, guided = answers
    assert _jpeg(plain) != _jpeg(guided)
    with Image.open(io.BytesIO(_jpeg(guided))) as im:
        assert im.size == (80, 80)
    other = _dream(client, file=_url(FILE), octaves="1", steps="1", guide=_url(_png(70, 70, 3)))
    assert other.status_code == 200 and _jpeg(other.json()) != _jpeg(guided)
    again = _dream(client, file=_url(FILE), octaves="1", steps="1", guide=_url(GUIDE))
    assert again.json() == guided  # deterministic, and guided / unguided requests do not share a batch


def test_route_bad_guide_is_400(client):
    r = _dream(client, file=_url(FILE), octaves="1", steps="1", guide="data:image/png;base64,AAAA")
    assert r.status_code == 400 and r.json()["detail"]
    r = _dream(client, file=_url(FILE), octaves="1", steps="1", guide="not a data url")
    assert r.status_code == 400


def test_route_guided_tiled_request_is_400(client, svc):
    """A side above dream_tile (128 here) would run the tiled engine, which takes no guide; without a guide the
    same image is served."""
    big = _url(_png(100, 140, 4))
    r = _dream(client, file=big, octaves="1", steps="1", guide=_url(GUIDE))
    assert r.status_code == 400 and "tiled" in r.json()["detail"]
    with pytest.raises(ValueError, match="tiled"):
        svc.run_batch([svc.prepare(np.zeros((100, 140, 3), np.uint8), 1)], "inception_v3", 1, 1,
                      [svc.prepare_guide(np.zeros((50, 50, 3), np.uint8))])

    class _Runner:  # a multi-rank service: guided dreams are refused before anything is queued
        world = 2

        class info:
            device = "cpu"

    multi = DreamService(svc.cfg, runner=_Runner())
    with pytest.raises(ValueError, match="multi-rank"):
        asyncio.run(multi.dream(_url(FILE), "inception_v3", 1, 1, guide=_url(GUIDE)))


def test_guided_requests_batch_apart_and_pad_with_the_last_guide(svc):
    """Same-shape guided requests run as ONE batch with their guides stacked (3 requests -> padded to 4 by
    repeating the last image and guide); each answer equals the request served alone."""
    ds = DreamService(Config.from_env(device="cpu", hip_graphs=False, dream_window_ms=300.0, dream_max_batch=4))
    try:
        files = [_url(_png(80, 80, 10 + i)) for i in range(3)]
        guides = [_url(_png(64, 64, 20 + i)) for i in range(3)]

        async def go():
            return await asyncio.gather(*[ds.dream(f, "inception_v3", 1, 1, guide=g) for f, g in zip(files, guides)],
                                        ds.dream(files[0], "inception_v3", 1, 1))

        outs = asyncio.run(go())
        assert sorted(ds.batches) == [1, 3]
        alone = asyncio.run(ds.dream(files[1], "inception_v3", 1, 1, guide=guides[1]))
        a, b = np.asarray(Image.open(io.BytesIO(_jpeg(outs[1])))), np.asarray(Image.open(io.BytesIO(_jpeg(alone))))
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 2  # (batch-size-dependent CPU conv rounding)
        assert _jpeg(outs[0]) != _jpeg(outs[3])
    finally:
        ds.close()


@pytest.fixture()
def relay(svc):
    d = tempfile.mkdtemp(prefix="dv-guide-test-")
    path = os.path.join(d, "s.sock")

    class _Deconv:  # the owner's deconv service is not used here
        cfg = svc.cfg

    srv = I.IngestServer(path, _Deconv(), dream=svc)
    cli = I.IngestClient(path, connect_timeout=10)
    yield cli
    cli.close()
    srv.close()
    os.rmdir(d)


def test_frontend_relay_carries_the_guide(relay, svc, answers):
    """The same requests through a front end (RemoteDream over the ingest socket to a CPU owner) give the direct
    route's bytes; an old-style header (no guide_len) is still an unguided request; a header whose guide_len
    exceeds the body is refused."""
    plain, guided = answers
    from fastapi.testclient import TestClient

    with TestClient(create_app(None, svc.cfg, dream_service=RemoteDream(relay, svc.cfg))) as c:
        r = _dream(c, file=_url(FILE), octaves="1", steps="1", guide=_url(GUIDE))
        assert r.status_code == 200 and r.json() == guided
        r = _dream(c, file=_url(FILE), octaves="1", steps="1")
        assert r.status_code == 200 and r.json() == plain
        r = _dream(c, file=_url(FILE), octaves="1", steps="1", guide="data:image/png;base64,AAAA")
        assert r.status_code == 400  # the owner's 400, relayed

    def call(body):
        ev, box = threading.Event(), {}

        def cb(st, data):
            box["r"] = (st, data)
            ev.set()

        relay.send(I.DREAM, cb, payload=body)
        assert ev.wait(120)
        return box["r"]

    old = json.dumps({"model": "inception_v3", "octaves": 1, "steps": 1}).encode() + b"\n" + _url(FILE).encode()
    st, data = call(old)
    assert st == 200 and data.decode() == plain
    g = _url(GUIDE).encode()
    new = json.dumps({"model": "inception_v3", "octaves": 1, "steps": 1, "guide_len": len(g)}).encode() + b"\n" + \
        _url(FILE).encode() + g
    st, data = call(new)
    assert st == 200 and data.decode() == guided
    bad = json.dumps({"model": "inception_v3", "octaves": 1, "steps": 1, "guide_len": 10 ** 9}).encode() + b"\n" + g
    st, data = call(bad)
    assert st == 400


@pytest.mark.timeout(600)
def test_cli_dream_guide_writes_the_routes_bytes(tmp_path, answers):
    plain, guided = answers
    f, g = tmp_path / "f.png", tmp_path / "g.png"
    f.write_bytes(FILE)
    g.write_bytes(GUIDE)
    env = dict(os.environ, DV_DEVICE="cpu", DV_HIP_GRAPHS="0", DV_LOG_JSON="0", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "deconv_api_amd.cli", "dream", str(f), "--octaves", "1", "--steps", "1",
                        "--guide", str(g), "--out-dir", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    got = (tmp_path / "out" / "f_dream_inception_v3.jpg").read_bytes()
    assert got == _jpeg(guided) and got != _jpeg(plain)
