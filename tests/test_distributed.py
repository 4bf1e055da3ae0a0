"""CPU multi-process (gloo, world_size 2/3/4) tests of the data-parallel path: weight broadcast
bit-equality, all-gather order, ragged shard padding, and sharded deconvnet == single process."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from deconv_api_amd.parallel import dist as pdist

    return pdist.init(backend="gloo", device_type="cpu")


def _worker_collectives(rank, world, port, q):
    try:
        from deconv_api_amd.models.vgg16 import VGG16
        from deconv_api_amd.parallel import dist as pdist

        info = _init(rank, world, port)
        m = VGG16.random(0 if rank == 0 else 99, include_top=False)
        sd = pdist.broadcast_state(m.state_dict(), info, bucket_bytes=8 << 20)
        ref = VGG16.random(0, include_top=False).state_dict()
        same = all(torch.equal(sd[k], ref[k]) for k in ref)
        x = torch.full((2, 3), float(rank))
        g = pdist.all_gather_rows(x, info)
        order = g[:, 0].tolist()
        mx = pdist.all_reduce_max(float(rank) * 1.5, info)
        q.put((rank, same, order, mx))
        pdist.shutdown()
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None, None))


def _run(fn, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=fn, args=(r, world, port, q, *args)) for r in range(world)]
    for p in ps:
        p.start()
    out = [q.get(timeout=300) for _ in range(world)]
    for p in ps:
        p.join(timeout=60)
    return sorted(out, key=lambda t: t[0])


@pytest.mark.parametrize("world", [2, 3, 4])
def test_broadcast_gather(world):
    res = _run(_worker_collectives, world)
    for rank, same, order, mx in res:
        assert same is True, same
        assert order == [float(r) for r in range(world) for _ in range(2)]
        assert mx == 1.5 * (world - 1)


def _worker_sharded(rank, world, port, q):
    try:
        from deconv_api_amd.engine.deconvnet import DeconvNet
        from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
        from deconv_api_amd.parallel.sharded import ShardedRunner

        info = _init(rank, world, port)
        specs = vgg16_specs(width_div=8, image_size=32, fc=64, classes=10)
        eng = DeconvNet(VGG16.random(0, specs=specs).build("cpu", torch.float32))
        runner = ShardedRunner(eng, info, image_size=32)
        if rank == 0:
            rng = np.random.default_rng(0)
            imgs = [rng.integers(0, 256, (30 + i, 28, 3), dtype=np.uint8) for i in range(5)]  # ragged: 5 over 2
            out = runner.run("block3_conv2", imgs)
            out2 = runner.run("block1_pool", imgs[:1])
            runner.stop()
            single = ShardedRunner(eng, type(info)(), image_size=32)
            want = single._local("block3_conv2", imgs).numpy()
            q.put((rank, out.shape, bool(np.array_equal(out, want)), out2.shape))
        else:
            n = runner.follow()
            q.put((rank, n, None, None))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc(), None, None))


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_deconv_matches_single(world):
    """5 ragged images over 2 or 4 ranks (shards 3/2 and 2/1/1/1), then a 1-image batch (empty shards)."""
    res = _run(_worker_sharded, world)
    r0 = res[0]
    assert r0[1] == (5, 64, 64, 3), r0
    assert r0[2] is True
    assert r0[3] == (1, 64, 64, 3)
    for r in res[1:]:
        assert r[1] == 2, r  # every follower served both batches


def _worker_failover(rank, world, port, q, dead_rank):
    try:
        os.environ["DV_FAULT"] = f"exit@2/rank={dead_rank}"  # that rank dies when its 2nd batch arrives
        from deconv_api_amd.engine.deconvnet import DeconvNet
        from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
        from deconv_api_amd.parallel.sharded import ShardedRunner

        info = _init(rank, world, port)
        specs = vgg16_specs(width_div=8, image_size=32, fc=64, classes=10)
        eng = DeconvNet(VGG16.random(0, specs=specs).build("cpu", torch.float32))
        runner = ShardedRunner(eng, info, image_size=32, hb_timeout=1.0)
        if rank == 0:
            rng = np.random.default_rng(1)
            imgs = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8) for _ in range(5)]
            a = runner.run("block2_conv1", imgs)      # sharded over every rank
            w1 = runner.world
            b = runner.run("block2_conv1", imgs)      # dead_rank exits mid-batch -> re-form, recompute
            w2 = runner.world
            c = runner.run("block2_conv1", imgs[:3])  # on the survivors
            single = ShardedRunner(eng, type(info)(), image_size=32)
            want = single._local("block2_conv1", imgs).numpy()
            want_c = single._local("block2_conv1", imgs[:3]).numpy()
            # the service's /ready reports the re-formed world
            from deconv_api_amd.serve.service import DeconvService

            svc = DeconvService(engine=eng, runner=runner)
            st = svc.status()
            svc.close()
            runner.stop()
            q.put((rank, bool(np.array_equal(a, want)), bool(np.array_equal(b, want)),
                   bool(np.array_equal(c, want_c)), (w1, w2, runner.world, st["world"], runner.reforms)))
        else:
            n = runner.follow()
            q.put((rank, "follower returned", n, runner.world, None))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None))


@pytest.mark.parametrize("world,dead", [(2, 1), (3, 2), (3, 1)])
def test_follower_failure_reforms_group(world, dead):
    """A follower dies during its 2nd batch: rank 0 detects it at the next ack (stale heartbeat),
    the survivors re-form the process group (renumbered), the batch is recomputed on them and
    equals the single-process result; /ready reports the new world."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker_failover, args=(r, world, port, q, dead)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world - 1):  # the dead rank reports nothing
        r = q.get(timeout=300)
        res[r[0]] = r
    for p in ps:
        p.join(timeout=60)
    assert 0 in res, res
    r0 = res[0]
    assert r0[1] is True and r0[2] is True and r0[3] is True, r0
    assert r0[4] == (world, world - 1, world - 1, world - 1, 1), r0
    assert ps[dead].exitcode == 17
    for r in range(1, world):
        if r != dead:
            # batch 1, batch 2 recomputed after the re-form, batch 3 (the aborted try does not count)
            assert res[r][1] == "follower returned" and res[r][2] == 3 and res[r][3] == world - 1, res[r]


def test_fault_spec_parse():
    from deconv_api_amd.utils.faults import FaultInjector, InjectedFault, parse

    fs = parse("raise@2,hang@3:0.01/rank=0,exit@9/rank=4")
    assert [(f.action, f.batch, f.rank) for f in fs] == [("raise", 2, None), ("hang", 3, 0), ("exit", 9, 4)]
    inj = FaultInjector(fs, rank=0)
    inj.on_batch()
    with pytest.raises(InjectedFault):
        inj.on_batch()
    inj.on_batch()  # hang 10 ms
    with pytest.raises(ValueError):
        parse("explode@1")


def _worker_bench(rank, world, port, q):
    try:
        _init(rank, world, port)
        import bench
        from deconv_api_amd.parallel import dist as pdist

        # bench.main() initializes its own group from the env; tear ours down first
        pdist.shutdown()
        line = bench.main(["--device", "cpu", "--tiny", "--batch", "3", "--steps", "3", "--warmup", "1",
                           "--gpus", str(world)])
        q.put((rank, line))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc()))


def test_bench_rehearsal_dp2():
    """bench.py's distributed path (weight broadcast, async double-buffered all-gather, max-over-
    ranks timing, JSON contract) on gloo with world_size 2."""
    res = _run(_worker_bench, 2)
    for rank, line in res:
        assert isinstance(line, dict), line
        assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 6 and line["steps"] == 3
        assert line["config"]["parallelism"] == "dp2" and line["value"] > 0 and line["scaling"] == "weak"
        for k in ("metric", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "warmup"):
            assert k in line


def test_bench_dump_outputs_rehearsal(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last timed step's filters and a seeded sample of its mosaics as
    float32 .npy files; the same arguments give the same inputs, sample and (on the CPU engine,
    which is deterministic) the same arrays; --full is accepted and --steps sets the timed steps."""
    import numpy as np

    import bench

    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DV_FORCE_PG", "TORCHELASTIC_RUN_ID"):
        monkeypatch.delenv(v, raising=False)
    B = bench.DUMP_IMAGES + 3  # more images than the dump keeps: the sampling path
    base = ["--device", "cpu", "--tiny", "--batch", str(B), "--steps", "2", "--warmup", "1"]
    runs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        line = bench.main(base + extra + ["--dump-outputs", str(tmp_path / name)])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["n_gpus"] == 1
        runs.append({p.stem: np.load(p) for p in sorted((tmp_path / name).glob("*.npy"))})
    a, b = runs
    assert sorted(a) == ["filters", "mosaic", "mosaic_index"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["filters"].shape == (B, 4) and a["mosaic"].shape == (bench.DUMP_IMAGES, 64, 64, 3)
    idx = a["mosaic_index"]
    assert idx.shape == (bench.DUMP_IMAGES,) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < B
    assert a["mosaic"].min() >= 0 and a["mosaic"].max() <= 255 and a["mosaic"].std() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_shard_sizes():
    from deconv_api_amd.parallel.dist import shard_counts, shard_sizes

    assert shard_sizes(2048, 8) == [256] * 8
    assert shard_sizes(5, 2) == [3, 3]
    assert shard_counts(5, 2) == [3, 2]
    assert sum(shard_counts(7, 4)) == 7


def _tiled_dream(world, rank, info=None):
    from deconv_api_amd.engine.deepdream import RESNET_LAYERS, DreamSettings, TiledDeepDream
    from deconv_api_amd.models.resnet50 import ResNet50

    torch.manual_seed(0)
    net = ResNet50(0).build("cpu")
    s = DreamSettings(layers=dict(RESNET_LAYERS), octaves=1, iterations=2, max_loss=None)
    x = torch.rand(3, 192, 192, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1
    return TiledDeepDream(net, s, tile=96, info=info, seed=5).gradient_ascent(x)


def _worker_tiled(rank, world, port, q):
    try:
        info = _init(rank, world, port)
        out = _tiled_dream(world, rank, info)
        q.put((rank, out.numpy(), None, None))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e), None, None))


def test_tiled_dream_units_across_ranks():
    """12 (tile, image) units over 3 ranks (uneven: some tiles split their images across ranks)
    give the single-process result, identically on every rank."""
    from deconv_api_amd.engine.deepdream import TiledDeepDream

    assert TiledDeepDream._my_units(None, 3, 4, 5, 1) == [(0, 1), (2, 0), (3, 2)]
    assert TiledDeepDream._axis_tiles(731, 512) == (366, [(0, 0, 366), (365, 366, 731)])
    ref = _tiled_dream(1, 0).numpy()
    outs = _run(_worker_tiled, 3)
    for r, out, _, _ in outs:
        assert not isinstance(out, str), out
        assert np.array_equal(out, outs[0][1])  # every rank applies the same update
        # vs one process: the per-image tile batches differ (3 images vs 1), so fp32 CPU conv
        # rounding differs at the 1e-9 level and can flip a ReLU/max-pool tie; the normalized
        # step (0.01) bounds the effect
        d = np.abs(out - ref)
        assert d.mean() < 1e-4 and d.max() < 2e-2, (d.mean(), d.max())


def _worker_inflight(rank, world, port, q, fault):
    try:
        if fault:
            os.environ["DV_FAULT"] = fault
        from deconv_api_amd.engine.deconvnet import DeconvNet
        from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
        from deconv_api_amd.parallel.sharded import ShardedRunner

        info = _init(rank, world, port)
        specs = vgg16_specs(width_div=8, image_size=32, fc=64, classes=10)
        eng = DeconvNet(VGG16.random(0, specs=specs).build("cpu", torch.float32))
        runner = ShardedRunner(eng, info, image_size=32, hb_timeout=1.0)
        if rank == 0:
            rng = np.random.default_rng(3)
            sets = [[rng.integers(0, 256, (32 + i, 30, 3), dtype=np.uint8) for i in range(n)] for n in (5, 4, 3, 6)]
            layers = ["block2_conv1", "block3_conv2", "block1_pool", "block2_conv1"]
            # launch i+1 before finishing i (the service worker's order): two batches in flight
            outs = [None] * 4
            prev = runner.launch(layers[0], sets[0])
            for i in range(1, 4):
                cur = runner.launch(layers[i], sets[i])
                outs[i - 1] = runner.finish(prev)
                prev = cur
            outs[3] = runner.finish(prev)
            single = ShardedRunner(eng, type(info)(), image_size=32)
            same = [bool(np.array_equal(o, single._local(l, s).numpy())) for o, l, s in zip(outs, layers, sets)]
            world_after = runner.world
            runner.stop()
            q.put((rank, same, world_after, runner.reforms))
        else:
            n = runner.follow()
            q.put((rank, "follower returned", n, runner.world))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc(), None, None))


@pytest.mark.parametrize("fault", ["", "exit_ready@2/rank=2", "exit_done@3/rank=1"])
def test_two_batches_in_flight(fault):
    """Rank 0 launches batch i+1 before gathering batch i (world 3): every batch equals the single-
    process result bit for bit. With a fault, a follower dies in one of the windows between its ack
    and the collective (after acking 'ready' of its 2nd run / 'done' of its 3rd): rank 0 detects it
    inside the polled collective, the survivors re-form, and every batch launched on the old group is
    recomputed on the new one."""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker_inflight, args=(r, world, port, q, fault)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world - (1 if fault else 0)):
        r = q.get(timeout=300)
        res[r[0]] = r
    for p in ps:
        p.join(timeout=60)
    assert 0 in res, res
    r0 = res[0]
    assert isinstance(r0[1], list), r0
    assert r0[1] == [True] * 4, r0
    if fault:
        dead = int(fault.split("rank=")[1])
        assert ps[dead].exitcode == 17
        assert r0[2] == world - 1 and r0[3] == 1, r0
    else:
        assert r0[2] == world and r0[3] == 0, r0
        assert all(res[r][2] == 4 for r in range(1, world)), res


def _worker_dream_service(rank, world, port, q):
    try:
        from deconv_api_amd.config import Config
        from deconv_api_amd.engine.deconvnet import DeconvNet
        from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
        from deconv_api_amd.parallel.sharded import ShardedRunner

        info = _init(rank, world, port)
        cfg = Config(device="cpu", dream_tile=96, seed=4, hip_graphs=False)
        specs = vgg16_specs(width_div=8, image_size=32, fc=64, classes=10)
        eng = DeconvNet(VGG16.random(0, specs=specs).build("cpu", torch.float32))
        runner = ShardedRunner(eng, info, image_size=32, cfg=cfg)
        if rank == 0:
            from deconv_api_amd.serve.dream_service import DreamService

            rng = np.random.default_rng(2)
            img = torch.from_numpy(rng.integers(0, 256, (160, 176, 3), dtype=np.uint8))
            ds = DreamService(cfg, runner=runner)
            got = ds.run_batch([img], "resnet50", 1, 2)  # 2 x 2 tiles of <= 96 px over 2 ranks
            imgs = [rng.integers(0, 256, (30, 28, 3), dtype=np.uint8) for _ in range(3)]
            mos = runner.run("block2_conv1", imgs)  # the deconv service keeps working on the same group
            st = ds.status()
            runner.stop()
            single = DreamService(cfg)  # one process: the same image tiled locally (side > 96)
            want = single.run_batch([img], "resnet50", 1, 2)
            want_mos = ShardedRunner(eng, type(info)(), image_size=32)._local("block2_conv1", imgs).numpy()
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            q.put((rank, got.shape, int(d.max()), float(d.mean()), st["world"], bool(np.array_equal(mos, want_mos))))
        else:
            n = runner.follow()
            q.put((rank, "follower returned", n, None, None, None))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def test_deepdream_service_tiled_across_ranks():
    """POST /deepdream's batch on a 2-rank group: rank 0 broadcasts the image, both ranks run their
    (tile, image) units with the per-step pack all-gather, rank 0 answers; equals the single-process
    tiled result up to CPU conv rounding (the units sit in different batches), the deconv command
    stream keeps working on the same group, and the dream service reports the world."""
    res = _run(_worker_dream_service, 2)
    r0 = res[0]
    assert r0[1] == (1, 160, 176, 3), r0
    assert r0[2] <= 3 and r0[3] < 0.05, r0  # uint8 output: at most a few levels apart, rarely
    assert r0[4] == 2 and r0[5] is True, r0
    assert res[1][1] == "follower returned" and res[1][2] == 1, res[1]


def _worker_dream_fault(rank, world, port, q, fault, interleave):
    """rank 0 dreams (2 octaves) on a world-3 group; ``fault`` kills a follower inside an octave;
    ``interleave``: a deconv batch is submitted from another thread while the dream runs."""
    try:
        if fault:
            os.environ["DV_FAULT"] = fault
        import threading
        import time

        from deconv_api_amd.config import Config
        from deconv_api_amd.engine.deconvnet import DeconvNet
        from deconv_api_amd.models.vgg16 import VGG16, vgg16_specs
        from deconv_api_amd.parallel.sharded import ShardedRunner

        info = _init(rank, world, port)
        cfg = Config(device="cpu", dream_tile=96, seed=4, hip_graphs=False)
        specs = vgg16_specs(width_div=8, image_size=32, fc=64, classes=10)
        eng = DeconvNet(VGG16.random(0, specs=specs).build("cpu", torch.float32))
        runner = ShardedRunner(eng, info, image_size=32, cfg=cfg, hb_timeout=1.0)
        if rank == 0:
            rng = np.random.default_rng(2)
            img = torch.from_numpy(rng.integers(0, 256, (1, 160, 176, 3), dtype=np.uint8))
            imgs = [rng.integers(0, 256, (30, 28, 3), dtype=np.uint8) for _ in range(3)]
            octaves = 3 if interleave is True else 2
            t = {}
            stop_ping = threading.Event()
            if interleave == "ping":  # the service's idle liveness check, running beside the dream

                def pinger():
                    while not stop_ping.is_set():
                        runner.ping()
                        time.sleep(0.05)

                pth = threading.Thread(target=pinger)
                pth.start()
            if interleave is True:
                res = {}

                def deconv():
                    while runner._did == 0:  # the dream has started (its setup command is out)
                        time.sleep(0.01)
                    res["mos"] = runner.run("block2_conv1", imgs)
                    t["deconv_done"] = time.time()

                th = threading.Thread(target=deconv)
                th.start()
            t0 = time.time()
            got = runner.dream(img, "resnet50", octaves, 2)
            t["dream_done"] = time.time()
            t["dream_s"] = t["dream_done"] - t0
            stop_ping.set()
            if interleave == "ping":
                pth.join()
            mos_ok = None
            if interleave is True:
                th.join()
                want_mos = ShardedRunner(eng, type(info)(), image_size=32)._local("block2_conv1", imgs).numpy()
                mos_ok = bool(np.array_equal(res["mos"], want_mos)) and t["deconv_done"] < t["dream_done"]
            world_after, reforms, restarts = runner.world, runner.reforms, runner.dream_restarts
            runner.stop()
            from deconv_api_amd.serve.dream_service import DreamService

            want = DreamService(cfg).run_batch([img[0]], "resnet50", octaves, 2)  # one process
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            q.put((rank, (int(d.max()), float(d.mean())), world_after, reforms, restarts, mos_ok, t["dream_s"]))
        else:
            n = runner.follow()
            q.put((rank, "follower returned", n, None, None, None, None))
        from deconv_api_amd.parallel import dist as pdist

        pdist.shutdown()
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None, None))


@pytest.mark.parametrize("fault,interleave", [("exit_octave@2/rank=2", False), ("", True),
                                             ("exit_octave@2/rank=2", "ping")])
def test_dream_fault_and_interleave(fault, interleave):
    """Multi-rank /deepdream (world 3, one command per octave, every collective polled):
    * a follower killed inside the dream's 2nd octave: rank 0 detects it (the octave's polled
      collectives / heartbeats), the survivors re-form, and the dream restarts and completes on
      world 2, equal to the one-process dream up to rounding;
    * no fault: a deconv batch submitted while a 3-octave dream runs completes BEFORE the dream
      (the FIFO command lock is released between octaves) and equals the single-process result;
    * the same fault with the service's ``ping()`` polling beside the dream: whichever of the two
      detects the loss re-forms the group exactly once (ping takes the command lock and re-forms
      through ``_reform``, which drops the dream's per-world tiled state), and the restarted dream
      is equal to the one-process dream."""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker_dream_fault, args=(r, world, port, q, fault, interleave)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in range(world - (1 if fault else 0)):
        r = q.get(timeout=600)
        res[r[0]] = r
    for p in ps:
        p.join(timeout=60)
    assert 0 in res, res
    r0 = res[0]
    assert isinstance(r0[1], tuple), r0
    dmax, dmean = r0[1]
    assert dmax <= 3 and dmean < 0.05, r0  # uint8: a few levels apart, rarely (CPU conv batch rounding)
    if fault:
        assert ps[2].exitcode == 17
        assert r0[2] == 2 and r0[3] == 1 and r0[4] == 1, r0
    else:
        assert r0[2] == 3 and r0[3] == 0 and r0[4] == 0, r0
        assert r0[5] is True, r0
        assert all(res[r][1] == "follower returned" for r in (1, 2)), res
