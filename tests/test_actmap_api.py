"""POST /activations through the serving layers (CPU engine): the route and its 4xx answers, the batching service (a
layer's activation jobs share one forward), the front-end relay (ingest kind 8), ``cli activations`` and the refusal of
a multi-rank (rank-0 sharding) service."""
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
from deconv_api_amd.engine.activations import ActivationMaps
from deconv_api_amd.engine.deconvnet import DeconvNet
from deconv_api_amd.models.vgg16 import VGG16
from deconv_api_amd.serve import ingest as I
from deconv_api_amd.serve.frontend import RemoteService
from deconv_api_amd.serve.service import DeconvService, _Job

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER = "block1_conv2"
IMG = np.random.default_rng(11).integers(0, 256, (60, 90, 3), dtype=np.uint8)
IMGS = [IMG, IMG[::-1].copy(), IMG[:, ::-1].copy()]
FILE = make_data_url(IMG, "PNG")
GRID = {"patch": "112", "stride": "112"}
_INFO = (I.STATUS, I.METRICS, I.LAYERS)  # info requests: not counted where a test records what a front end sends


@pytest.fixture(scope="module")
def svc():
    cfg = Config.from_env(device="cpu", hip_graphs=False, batch_timeout_ms=1.0, codec_workers=2)
    s = DeconvService(cfg, engine=DeconvNet(VGG16.random(cfg.seed).build("cpu", torch.float32)))
    yield s
    s.close()


@pytest.fixture(scope="module")
def client(svc):
    from fastapi.testclient import TestClient

    with TestClient(create_app(svc, svc.cfg)) as c:
        yield c


@pytest.fixture(scope="module")
def answer(client):
    r = client.post("/activations", data={"file": FILE, "layer": LAYER})
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
    body, ct = encode_multipart({"file": FILE, "layer": LAYER})
    r = client.post("/activations", content=body, headers={"content-type": ct})
    assert r.status_code == 200 and r.json() == answer
    # the JPEG of the engine's mosaic of the same image: true RGB, no channel reversal
    want = ActivationMaps(svc.engine).run(svc.preprocess([IMG]), LAYER).mosaic[0].numpy()
    assert np.array_equal(parse_result_data_url(answer), parse_result_data_url(encode_data_url(want, svc.cfg.jpeg_quality)))
    assert np.abs(got - want[..., ::-1]).mean() > np.abs(got - want).mean()
    assert np.array_equal(svc.run_activations(LAYER, [IMG])[0], want)


def test_route_errors(client, svc):
    n = svc.batches
    r = client.post("/activations", data={"layer": LAYER})
    assert r.status_code == 422 and r.json()["detail"][0] == {"loc": ["body", "file"], "msg": "field required",
                                                              "type": "value_error.missing"}
    r = client.post("/activations", data={"file": FILE})
    assert r.status_code == 422 and r.json()["detail"][0]["loc"] == ["body", "layer"]
    for layer in ("nope", "input_1", "flatten", "fc1", "predictions"):
        r = client.post("/activations", data={"file": FILE, "layer": layer})
        assert r.status_code == 400 and r.json()["detail"], layer
    assert "has no feature map" in client.post("/activations", data={"file": FILE, "layer": "fc1"}).json()["detail"]
    for f in ("no-comma-here", "data:image/png;base64," + base64.b64encode(b"junk").decode()):
        r = client.post("/activations", data={"file": f, "layer": LAYER})
        assert r.status_code == 400, f
    assert svc.batches == n, "a refused request reached the engine"


def test_openapi_lists_the_route(client):
    spec = client.get("/openapi.json").json()
    body = spec["paths"]["/activations"]["post"]["requestBody"]["content"]
    for ct in ("application/x-www-form-urlencoded", "multipart/form-data"):
        assert sorted(body[ct]["schema"]["required"]) == ["file", "layer"]
        assert set(body[ct]["schema"]["properties"]) == {"file", "layer"}


def test_other_routes_are_unchanged_around_an_activation_request(client, answer):
    post = lambda route, **kw: client.post(route, data={"file": FILE, "layer": LAYER, **kw})  # noqa: E731
    before, occ_before = post("/"), post("/occlusion", **GRID)
    act = post("/activations")
    after, occ_after = post("/"), post("/occlusion", **GRID)
    assert all(r.status_code == 200 for r in (before, occ_before, act, after, occ_after))
    assert before.content == after.content and occ_before.content == occ_after.content
    assert act.json() == answer and act.content != before.content and act.content != occ_before.content


def _queue_together(svc, specs):
    """Put jobs (layer, image, act) on the service's queue in ONE step, so the worker collects them together; returns
    each job's result and the engine calls made as (kind, batch size)."""
    seen, done, box = [], threading.Event(), {}
    real_a, real_b = svc.launch_activations, svc.launch_batch
    svc.launch_activations = lambda layer, images: (seen.append(("act", len(images))), real_a(layer, images))[1]
    svc.launch_batch = lambda layer, images: (seen.append(("deconv", len(images))), real_b(layer, images))[1]

    def deliver(n):
        def cb(value, exc):
            box[n] = (value, exc)
            if len(box) == len(specs):
                done.set()
        return cb

    jobs = [_Job(layer, img, deliver(n), act=act) for n, (layer, img, act) in enumerate(specs)]
    try:
        with svc.q.mutex:  # queue.Queue's own lock: the worker's get() sees all of them or none
            svc.q.queue.extend(jobs)
            svc.q.unfinished_tasks += len(jobs)
            svc.q.not_empty.notify()
        assert done.wait(300)
    finally:
        svc.launch_activations, svc.launch_batch = real_a, real_b
    assert all(box[n][1] is None for n in box), box
    return [box[n][0] for n in range(len(specs))], seen


def _pixels(v, svc):
    return parse_result_data_url(v if isinstance(v, str) else encode_data_url(v, svc.cfg.jpeg_quality))


def test_activation_jobs_of_one_layer_are_one_group(svc, answer):
    outs, seen = _queue_together(svc, [(LAYER, img, True) for img in IMGS])
    assert seen == [("act", 3)]
    # every request gets its own image's picture, the one a lone request gets
    assert np.array_equal(_pixels(outs[0], svc), parse_result_data_url(answer))
    want = ActivationMaps(svc.engine).run(svc.preprocess(IMGS), LAYER).mosaic.numpy()
    for n in range(3):
        assert np.array_equal(_pixels(outs[n], svc), _pixels(want[n], svc))
    assert not np.array_equal(_pixels(outs[0], svc), _pixels(outs[1], svc))


def test_deconv_and_activation_jobs_are_never_mixed(svc, client, answer):
    outs, seen = _queue_together(svc, [(LAYER, IMG, False), (LAYER, IMG, True), ("block1_conv1", IMG, True)])
    assert sorted(seen) == [("act", 1), ("act", 1), ("deconv", 1)]
    assert np.array_equal(_pixels(outs[1], svc), parse_result_data_url(answer))
    deconv = client.post("/", data={"file": FILE, "layer": LAYER}).json()
    assert np.array_equal(_pixels(outs[0], svc), parse_result_data_url(deconv))


@pytest.fixture()
def relay(svc):
    d = tempfile.mkdtemp(prefix="dv-act-test-")
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
    import json

    from fastapi.testclient import TestClient

    assert I.ACTIVATIONS == 8
    st, body = relay.call(I.LAYERS)
    assert st == 200 and json.loads(body)["activations"] == ActivationMaps(svc.engine).spatial_layers()
    assert LAYER in json.loads(body)["activations"] and "fc1" not in json.loads(body)["activations"]
    remote = RemoteService(relay, svc.cfg)
    try:
        assert remote.activation_layers == ActivationMaps(svc.engine).spatial_layers()
        sent = []
        real = relay.send
        relay.send = lambda kind, *a, **kw: (sent.append(kind) if kind not in _INFO else None, real(kind, *a, **kw))[1]
        try:
            with TestClient(create_app(remote, svc.cfg)) as c:
                r = c.post("/activations", data={"file": FILE, "layer": LAYER})
                assert r.status_code == 200 and r.json() == answer
                assert sent == [I.ACTIVATIONS]
                assert c.post("/", data={"file": FILE, "layer": LAYER}).content == \
                    client.post("/", data={"file": FILE, "layer": LAYER}).content
                n = len(sent)
                for layer in ("nope", "fc1", "predictions", "flatten"):  # 400 before anything is sent
                    r = c.post("/activations", data={"file": FILE, "layer": layer})
                    assert r.status_code == 400 and r.json()["detail"], layer
                assert len(sent) == n
        finally:
            relay.send = real
    finally:
        remote.close()
    # the owner's own checks: a frame for a dense layer is answered 400
    st, msg = _raw(relay, I.ACTIVATIONS, layer="fc1", h=IMG.shape[0], w=IMG.shape[1], payload=IMG)
    assert st == 400 and b"has no feature map" in msg
    # a kind the owner does not know: 400, and the connection still serves the next request
    st, msg = _raw(relay, 9, layer=LAYER, h=2, w=2, payload=b"x" * 12)
    assert st == 400 and msg == b"unknown request kind"
    st, data = _raw(relay, I.ACTIVATIONS, layer=LAYER, h=IMG.shape[0], w=IMG.shape[1], payload=IMG)
    assert st == 200 and data.decode() == answer


def test_frontend_does_not_send_kind_8_to_an_owner_without_it(relay, svc):
    remote = RemoteService(relay, svc.cfg)
    try:
        remote.activation_layers = None  # what an owner that does not announce the key leaves
        sent = []
        real = relay.send
        relay.send = lambda kind, *a, **kw: (sent.append(kind) if kind not in _INFO else None, real(kind, *a, **kw))[1]
        try:
            with pytest.raises(Exception) as e:
                asyncio.run(remote.activations(FILE, LAYER))
        finally:
            relay.send = real
        assert getattr(e.value, "status", None) == 400 and sent == []
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
            r = c.post("/activations", data={"file": FILE, "layer": LAYER})
            assert r.status_code == 400 and r.json()["detail"] == "activations are served by a one-GPU owner"
        with pytest.raises(ValueError, match="one-GPU owner"):
            multi.submit(LAYER, IMG, lambda v, e: None, act=True)
    finally:
        multi.close()


@pytest.mark.timeout(600)
def test_cli_activations_writes_the_routes_bytes(tmp_path, answer):
    f, g = tmp_path / "f.png", tmp_path / "g.png"
    Image.fromarray(IMG).save(f)
    Image.fromarray(IMGS[1]).save(g)
    env = dict(os.environ, DV_DEVICE="cpu", DV_HIP_GRAPHS="0", DV_LOG_JSON="0", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "deconv_api_amd.cli", "activations", *args, "--out-dir",
                               str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)

    r = cli(str(f), str(g), "--layer", LAYER)  # two images: one batch
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "out" / f"f_activations_{LAYER}.jpg").read_bytes() == _jpeg(answer)
    assert (tmp_path / "out" / f"g_activations_{LAYER}.jpg").read_bytes() != _jpeg(answer)
    r = cli(str(f), "--layer", "fc1")
    assert r.returncode == 2 and r.stderr.startswith("error:") and "has no feature map" in r.stderr, r.stderr[-500:]
    r = cli(str(f), "--layer", "nope")
    assert r.returncode == 2 and r.stderr.startswith("error: unknown layer"), r.stderr[-500:]
