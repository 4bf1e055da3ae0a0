"""POST /occlusion through the serving layers (CPU engine, the 5-variant grid patch = stride = 112): the route and
its 4xx answers, the batching service, the front-end relay (ingest kind 7), ``cli occlusion`` and the refusal of a
multi-rank (rank-0 sharding) service."""
from __future__ import annotations

import asyncio
import base64
import io
import os
import subprocess
import sys
import tempfile
import threading
from urllib.parse import unquote

import numpy as np
import pytest
import torch
from PIL import Image

from deconv_api_amd.api.app import create_app
from deconv_api_amd.api.forms import encode_multipart
from deconv_api_amd.codec import DATA_URL_PREFIX, encode_data_url, make_data_url, parse_result_data_url
from deconv_api_amd.config import Config
from deconv_api_amd.engine.deconvnet import DeconvNet
from deconv_api_amd.engine.occlusion import Occlusion
from deconv_api_amd.models.vgg16 import VGG16
from deconv_api_amd.serve import ingest as I
from deconv_api_amd.serve.frontend import RemoteService
from deconv_api_amd.serve.service import DeconvService

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER = "block1_conv2"
IMG = np.random.default_rng(11).integers(0, 256, (60, 90, 3), dtype=np.uint8)
FILE = make_data_url(IMG, "PNG")
GRID = {"patch": "112", "stride": "112"}


@pytest.fixture(scope="module")
def svc():
    cfg = Config.from_env(device="cpu", hip_graphs=False, batch_timeout_ms=1.0, codec_workers=2)
    s = DeconvService(cfg, engine=DeconvNet(VGG16.random(cfg.seed, include_top=False).build("cpu", torch.float32)))
    yield s
    s.close()


@pytest.fixture(scope="module")
def client(svc):
    from fastapi.testclient import TestClient

    with TestClient(create_app(svc, svc.cfg)) as c:
        yield c


@pytest.fixture(scope="module")
def answer(client):
    r = client.post("/occlusion", data={"file": FILE, "layer": LAYER, **GRID})
    assert r.status_code == 200 and r.headers["content-type"].startswith("application/json"), r.text[:300]
    return r.json()


def _jpeg(url: str) -> bytes:
    assert isinstance(url, str) and url.startswith(DATA_URL_PREFIX)
    payload = url[len(DATA_URL_PREFIX):]
    assert "+" not in payload and "=" not in payload
    return base64.b64decode(unquote(payload))


def test_route_answers_a_448_jpeg_for_both_body_types(client, svc, answer):
    with Image.open(io.BytesIO(_jpeg(answer))) as im:
        assert im.format == "JPEG" and im.size == (448, 448)
        got = np.asarray(im.convert("RGB")).astype(int)
    body, ct = encode_multipart({"file": FILE, "layer": LAYER, **GRID})
    r = client.post("/occlusion", content=body, headers={"content-type": ct})
    assert r.status_code == 200 and r.json() == answer
    # the JPEG of the engine's mosaic of the same image: true RGB, no channel reversal
    want = Occlusion(svc.engine).run(svc.preprocess([IMG]), LAYER, 112, 112).mosaic[0].numpy()
    assert np.array_equal(parse_result_data_url(answer), parse_result_data_url(encode_data_url(want, svc.cfg.jpeg_quality)))
    assert np.abs(got - want[..., ::-1]).mean() > np.abs(got - want).mean()
    assert np.array_equal(svc.run_occlusion(LAYER, IMG, 112, 112)[0], want)


def test_route_errors(client, svc):
    n = svc.batches
    r = client.post("/occlusion", data={"layer": LAYER})
    assert r.status_code == 422 and r.json()["detail"][0] == {"loc": ["body", "file"], "msg": "field required",
                                                              "type": "value_error.missing"}
    r = client.post("/occlusion", data={"file": FILE})
    assert r.status_code == 422 and r.json()["detail"][0]["loc"] == ["body", "layer"]
    for layer in ("nope", "input_1", "fc1"):  # (fc1: this model has no classifier head)
        r = client.post("/occlusion", data={"file": FILE, "layer": layer, **GRID})
        assert r.status_code == 400 and r.json()["detail"], layer
    bad = [{"patch": "abc"}, {"patch": "32.5"}, {"stride": "1e1"}, {"stride": "x"},
           {"patch": "7", "stride": "4"}, {"patch": "113", "stride": "16"}, {"patch": "32", "stride": "33"},
           {"patch": "32", "stride": "3"}, {"patch": "16", "stride": "12"}, {"patch": "-32"},
           {"patch": "99999999999999999999"}]
    for f in bad:
        r = client.post("/occlusion", data={"file": FILE, "layer": LAYER, **f})
        assert r.status_code == 400 and r.json()["detail"], f
    for f in ("no-comma-here", "data:image/png;base64," + base64.b64encode(b"junk").decode()):
        r = client.post("/occlusion", data={"file": f, "layer": LAYER, **GRID})
        assert r.status_code == 400, f
    assert svc.batches == n, "a refused request reached the engine"


def test_openapi_lists_the_route(client):
    spec = client.get("/openapi.json").json()
    body = spec["paths"]["/occlusion"]["post"]["requestBody"]["content"]
    for ct in ("application/x-www-form-urlencoded", "multipart/form-data"):
        assert sorted(body[ct]["schema"]["required"]) == ["file", "layer"]
        assert set(body[ct]["schema"]["properties"]) == {"file", "layer", "patch", "stride"}


def test_post_root_is_unchanged_around_an_occlusion_request(client, answer):
    before = client.post("/", data={"file": FILE, "layer": LAYER})
    occ = client.post("/occlusion", data={"file": FILE, "layer": LAYER, **GRID})
    after = client.post("/", data={"file": FILE, "layer": LAYER})
    assert before.status_code == 200 and after.status_code == 200 and occ.status_code == 200
    assert before.content == after.content and occ.json() == answer and occ.content != before.content


def test_occlusion_jobs_are_never_grouped(svc):
    """Two occlusion requests and two deconv requests of one layer queued together: the occlusion jobs run as one
    engine call each."""
    seen = []
    real_o, real_b = svc.launch_occlusion, svc.launch_batch
    svc.launch_occlusion = lambda layer, image, *a: (seen.append(("occ", 1)), real_o(layer, image, *a))[1]
    svc.launch_batch = lambda layer, images: (seen.append(("deconv", len(images))), real_b(layer, images))[1]
    try:
        async def go():
            return await asyncio.gather(svc.occlusion(FILE, LAYER, 112, 112), svc.deconv(FILE, LAYER),
                                        svc.occlusion(FILE, LAYER, 112, 112), svc.deconv(FILE, LAYER))

        outs = asyncio.run(go())
    finally:
        svc.launch_occlusion, svc.launch_batch = real_o, real_b
    assert outs[0] == outs[2] and outs[1] == outs[3] and outs[0] != outs[1]
    assert sorted(s for k, s in seen if k == "occ") == [1, 1] and sum(s for k, s in seen if k == "deconv") == 2


@pytest.fixture()
def relay(svc):
    d = tempfile.mkdtemp(prefix="dv-occ-test-")
    path = os.path.join(d, "s.sock")
    srv = I.IngestServer(path, svc)
    cli = I.IngestClient(path, connect_timeout=10)
    yield cli
    cli.close()
    srv.close()
    os.rmdir(d)


def _raw(cli, kind, **kw):
    ev, box = threading.Event(), {}

    def cb(st, data):
        box["r"] = (st, data)
        ev.set()

    cli.send(kind, cb, **kw)
    assert ev.wait(120)
    return box["r"]


def test_frontend_relay_returns_the_same_bytes(relay, svc, answer, client):
    from fastapi.testclient import TestClient

    assert I.OCCLUSION == 7
    remote = RemoteService(relay, svc.cfg)
    try:
        assert remote.has_occlusion
        with TestClient(create_app(remote, svc.cfg)) as c:
            r = c.post("/occlusion", data={"file": FILE, "layer": LAYER, **GRID})
            assert r.status_code == 200 and r.json() == answer
            assert c.post("/", data={"file": FILE, "layer": LAYER}).content == \
                client.post("/", data={"file": FILE, "layer": LAYER}).content
            assert c.post("/occlusion", data={"file": FILE, "layer": "nope", **GRID}).status_code == 400
            assert c.post("/occlusion", data={"file": FILE, "layer": LAYER, "patch": "7"}).status_code == 400
    finally:
        remote.close()
    # the owner's own checks: a frame whose patch / stride lie outside the definition is answered 400
    st, msg = _raw(relay, I.OCCLUSION, layer=LAYER, h=IMG.shape[0], w=IMG.shape[1], payload=(I.OCC_HEAD.pack(7, 4), IMG))
    assert st == 400 and b"patch" in msg
    # a kind the owner does not know: 400, and the connection still serves the next request
    st, msg = _raw(relay, 9, layer=LAYER, h=2, w=2, payload=b"x" * 12)
    assert st == 400 and msg == b"unknown request kind"
    st, data = _raw(relay, I.OCCLUSION, layer=LAYER, h=IMG.shape[0], w=IMG.shape[1],
                    payload=(I.OCC_HEAD.pack(112, 112), IMG))
    assert st == 200 and data.decode() == answer


def test_frontend_does_not_send_kind_7_to_an_owner_without_it(relay, svc):
    remote = RemoteService(relay, svc.cfg)
    try:
        remote.has_occlusion = False
        with pytest.raises(Exception) as e:
            asyncio.run(remote.occlusion(FILE, LAYER, 112, 112))
        assert getattr(e.value, "status", None) == 400
    finally:
        remote.close()


def test_multi_rank_runner_is_refused(svc):
    class _Runner:  # a rank-0 sharding runner: never reached
        world = 2
        graphs = None
        degraded = False
        last_error = None

        class info:
            device = "cpu"

        def ping(self):
            pass

    from fastapi.testclient import TestClient

    multi = DeconvService(svc.cfg, engine=svc.engine, runner=_Runner())
    try:
        with TestClient(create_app(multi, svc.cfg)) as c:
            r = c.post("/occlusion", data={"file": FILE, "layer": LAYER, **GRID})
            assert r.status_code == 400 and r.json()["detail"] == "occlusion is served by a one-GPU owner"
        with pytest.raises(ValueError, match="one-GPU owner"):
            multi.submit(LAYER, IMG, lambda v, e: None, occ=(112, 112))
    finally:
        multi.close()


@pytest.mark.timeout(600)
def test_cli_occlusion_writes_the_routes_bytes(tmp_path, answer):
    f = tmp_path / "f.png"
    Image.fromarray(IMG).save(f)
    env = dict(os.environ, DV_DEVICE="cpu", DV_HIP_GRAPHS="0", DV_LOG_JSON="0", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "deconv_api_amd.cli", "occlusion", str(f), *args, "--out-dir",
                               str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)

    r = cli("--layer", LAYER, "--patch", "112", "--stride", "112")
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "out" / f"f_occlusion_{LAYER}.jpg").read_bytes() == _jpeg(answer)
    r = cli("--layer", LAYER, "--patch", "7")
    assert r.returncode == 2 and r.stderr.startswith("error:"), r.stderr[-500:]
    r = cli("--layer", "nope")
    assert r.returncode == 2 and r.stderr.startswith("error: unknown layer"), r.stderr[-500:]
