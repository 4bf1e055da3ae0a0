"""``lap_levels`` through the serving layers (CPU engine): POST /deepdream's form field and its 400s, the batching
key, the front-end relay's header (serve/frontend.py RemoteDream -> serve/ingest.py -> DreamService) and
``cli dream --lap-levels``."""
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
    """The route's answers for FILE, plain and with lap_levels=2 (1 octave, 1 step), shared by the tests below."""
    plain = _dream(client, file=_url(FILE), octaves="1", steps="1")
    lap = _dream(client, file=_url(FILE), octaves="1", steps="1", lap_levels="2")
    assert plain.status_code == 200 and lap.status_code == 200, (plain.text[:300], lap.text[:300])
    return plain.json(), lap.json()


class _Recorder:
    """A dream service that records how the route calls it."""

    def __init__(self):
        self.calls = []

    async def dream(self, *args, **kw):
        self.calls.append((args, kw))
        return "data:image/jpeg;base64,AAAA"


def test_route_passes_lap_levels_only_when_set(svc):
    """Absent or 0: the call of today, positional arguments and no keyword (with a guide: ``guide`` alone);
    otherwise ``lap_levels`` as a keyword next to it."""
    from fastapi.testclient import TestClient

    rec = _Recorder()
    with TestClient(create_app(None, svc.cfg, dream_service=rec)) as c:
        f, g = _url(FILE), _url(GUIDE)
        assert _dream(c, file=f, octaves="2", steps="3").status_code == 200
        assert _dream(c, file=f, octaves="2", steps="3", lap_levels="0").status_code == 200
        assert _dream(c, file=f, octaves="2", steps="3", guide=g).status_code == 200
        assert _dream(c, file=f, octaves="2", steps="3", lap_levels="4").status_code == 200
        assert _dream(c, file=f, octaves="2", steps="3", lap_levels="5", guide=g).status_code == 200
        base = (f, "inception_v3", 2, 3)
        assert rec.calls == [(base, {}), (base, {}), (base, {"guide": g}), (base, {"lap_levels": 4}),
                             (base, {"lap_levels": 5, "guide": g})]
        n = len(rec.calls)
        for bad in ("abc", "6", "-1", "1.5"):
            r = _dream(c, file=f, octaves="1", steps="1", lap_levels=bad)
            assert r.status_code == 400 and r.json()["detail"], bad
        assert len(rec.calls) == n, "a refused request reached the service"


def test_route_lap_levels_changes_the_answer_and_reaches_run_batch(client, svc, answers, monkeypatch):
    plain, lap = answers
    assert _jpeg(plain) != _jpeg(lap)
    with Image.open(io.BytesIO(_jpeg(lap))) as im:
        assert im.size == (80, 80)
    seen = []
    real = svc.run_batch

    def spy(*args, **kw):
        seen.append((len(args), dict(kw)))
        return real(*args, **kw)

    monkeypatch.setattr(svc, "run_batch", spy)
    again = _dream(client, file=_url(FILE), octaves="1", steps="1", lap_levels="2")
    assert again.status_code == 200 and again.json() == lap  # deterministic
    other = _dream(client, file=_url(FILE), octaves="1", steps="1", lap_levels="3")
    assert other.status_code == 200 and _jpeg(other.json()) != _jpeg(lap)
    assert _dream(client, file=_url(FILE), octaves="1", steps="1").json() == plain  # and the setting does not stick
    assert seen == [(5, {"lap_levels": 2}), (5, {"lap_levels": 3}), (5, {})]
    for bad in ("abc", "6", "-1"):
        assert _dream(client, file=_url(FILE), octaves="1", steps="1", lap_levels=bad).status_code == 400
    assert len(seen) == 3


def test_service_validates_and_refuses_tiled_and_multi_rank(client, svc):
    for bad in (6, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="lap_levels"):
            svc.validate("inception_v3", 1, 1, bad)
        with pytest.raises(ValueError, match="lap_levels"):
            asyncio.run(svc.dream(_url(FILE), "inception_v3", 1, 1, lap_levels=bad))
    # a side above dream_tile (128 here) would run the tiled engine; without lap_levels the same image is served
    big = _url(_png(100, 140, 4))
    r = _dream(client, file=big, octaves="1", steps="1", lap_levels="2")
    assert r.status_code == 400 and "tiled" in r.json()["detail"]
    with pytest.raises(ValueError, match="tiled"):
        svc.run_batch([svc.prepare(np.zeros((100, 140, 3), np.uint8), 1)], "inception_v3", 1, 1, lap_levels=2)

    class _Runner:  # a multi-rank service: refused before anything is queued
        world = 2

        class info:
            device = "cpu"

    multi = DreamService(svc.cfg, runner=_Runner())
    with pytest.raises(ValueError, match="multi-rank"):
        asyncio.run(multi.dream(_url(FILE), "inception_v3", 1, 1, lap_levels=2))


def test_requests_with_different_lap_levels_batch_apart():
    """Same shape, lap_levels 2, 2, 0 and 3 inside one window: three batches (sizes 2, 1, 1), and a batched answer
    equals the request served alone."""
    ds = DreamService(Config.from_env(device="cpu", hip_graphs=False, dream_window_ms=300.0, dream_max_batch=4))
    try:
        files = [_url(_png(80, 80, 10 + i)) for i in range(4)]

        async def go():
            return await asyncio.gather(*[ds.dream(f, "inception_v3", 1, 1, lap_levels=n)
                                          for f, n in zip(files, (2, 2, 0, 3))])

        outs = asyncio.run(go())
        assert sorted(ds.batches) == [1, 1, 2]
        alone = asyncio.run(ds.dream(files[1], "inception_v3", 1, 1, lap_levels=2))
        a, b = np.asarray(Image.open(io.BytesIO(_jpeg(outs[1])))), np.asarray(Image.open(io.BytesIO(_jpeg(alone))))
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 2  # (batch-size-dependent CPU conv rounding)
        plain = asyncio.run(ds.dream(files[0], "inception_v3", 1, 1))
        assert _jpeg(plain) != _jpeg(outs[0])
    finally:
        ds.close()


@pytest.fixture()
def relay(svc):
    d = tempfile.mkdtemp(prefix="dv-lap-test-")
    path = os.path.join(d, "s.sock")

    class _Deconv:  # the owner's deconv service is not used here
        cfg = svc.cfg

    srv = I.IngestServer(path, _Deconv(), dream=svc)
    cli = I.IngestClient(path, connect_timeout=10)
    yield cli
    cli.close()
    srv.close()
    os.rmdir(d)


def test_frontend_relay_carries_lap_levels(relay, svc, answers):
    """Through a front end the answers are the direct route's bytes; the header carries ``lap_levels`` only when it
    is not 0, a header without it is a plain request, and a bad value is refused."""
    plain, lap = answers
    from fastapi.testclient import TestClient

    sent = []
    real = relay.send

    def send(kind, cb, payload=b""):
        sent.append(json.loads(payload.partition(b"\n")[0]))
        return real(kind, cb, payload=payload)

    relay.send = send
    try:
        with TestClient(create_app(None, svc.cfg, dream_service=RemoteDream(relay, svc.cfg))) as c:
            r = _dream(c, file=_url(FILE), octaves="1", steps="1", lap_levels="2")
            assert r.status_code == 200 and r.json() == lap
            r = _dream(c, file=_url(FILE), octaves="1", steps="1")
            assert r.status_code == 200 and r.json() == plain
            r = _dream(c, file=_url(FILE), octaves="1", steps="1", lap_levels="0")
            assert r.status_code == 200 and r.json() == plain
    finally:
        relay.send = real
    assert sent == [{"model": "inception_v3", "octaves": 1, "steps": 1, "lap_levels": 2},
                    {"model": "inception_v3", "octaves": 1, "steps": 1}, {"model": "inception_v3", "octaves": 1, "steps": 1}]

    def call(head):
        ev, box = threading.Event(), {}

        def cb(st, data):
            box["r"] = (st, data)
            ev.set()

        relay.send(I.DREAM, cb, payload=json.dumps(head).encode() + b"\n" + _url(FILE).encode())
        assert ev.wait(120)
        return box["r"]

    base = {"model": "inception_v3", "octaves": 1, "steps": 1}
    st, data = call(dict(base, lap_levels=2))
    assert st == 200 and data.decode() == lap
    st, data = call(dict(base, lap_levels=0))
    assert st == 200 and data.decode() == plain
    for bad in (6, -1, "2", 1.5, None, True):
        st, data = call(dict(base, lap_levels=bad))
        assert st == 400, bad


@pytest.mark.timeout(600)
def test_cli_dream_lap_levels_writes_the_routes_bytes(tmp_path, answers):
    plain, lap = answers
    f = tmp_path / "f.png"
    f.write_bytes(FILE)
    env = dict(os.environ, DV_DEVICE="cpu", DV_HIP_GRAPHS="0", DV_LOG_JSON="0", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "deconv_api_amd.cli", "dream", str(f), "--octaves", "1", "--steps", "1",
                        "--lap-levels", "2", "--out-dir", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    got = (tmp_path / "out" / "f_dream_inception_v3.jpg").read_bytes()
    assert got == _jpeg(lap) and got != _jpeg(plain)
