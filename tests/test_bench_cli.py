"""bench.py contract checks that need no GPU: defaults, the JSON keys the driver reads, and the loud failure
without a device (the hot path has no CPU fallback, so neither has the benchmark)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_defaults_and_workload_constants():
    assert (bench.WIDTH, bench.HEIGHT, bench.BATCH) == (3840, 2160, 64)      # BASELINE.json configs[2]
    assert bench.BYTES_PER_PIXEL == 5 and bench.HBM_PEAK_GBPS == 8000.0
    assert set(bench.ORDERS) == {"bggr", "rggb", "grbg", "gbrg"}


def test_distinct_gpu_check_refuses_ranks_that_share_a_card():
    """the N > 1 line must prove what it ran on -- distinct (host, PCI bus id) pairs are counted, and
    ranks that share a card are refused unless --share-gpu says it is meant."""
    ids = [{"rank": r, "device": r, "pci_bus_id": "0000:%02x:00.0" % (0x10 + r), "host": "n0"} for r in range(8)]
    assert bench.check_distinct_gpus(ids, 8, False) == (8, None)
    two = [dict(ids[0]), dict(ids[0], rank=1)]
    n, err = bench.check_distinct_gpus(two, 2, False)
    assert n == 1 and "only 1 distinct GPUs" in err and "0000:10:00.0" in err and "--share-gpu" in err
    assert bench.check_distinct_gpus(two, 2, True) == (1, None)
    # the same bus id on two hosts is two cards; a runtime that reports no bus id falls back to the ordinal
    assert bench.check_distinct_gpus([dict(ids[0]), dict(ids[0], host="n1")], 2, False) == (2, None)
    anon = [{"rank": 0, "device": 0, "pci_bus_id": None, "host": "n0"}, {"rank": 1, "device": 1, "pci_bus_id": None, "host": "n0"}]
    assert bench.check_distinct_gpus(anon, 2, False) == (2, None)
    assert bench.PLAN_SOURCES == ("default", "measured", "cached", "set")
    # a runtime that reports one bus id for every card: ranks with distinct ordinals under ONE device mask are trusted
    # (a false refusal would cost the 8-GPU run); the same ordinal twice (--share-gpu's case) is still refused
    same = [dict(ids[0], rank=r, device=r, visible_devices="") for r in range(8)]
    assert bench.check_distinct_gpus(same, 8, False) == (8, None)
    n, err = bench.check_distinct_gpus([dict(ids[0], visible_devices=""), dict(ids[0], rank=1, visible_devices="")], 2, False)
    assert n == 1 and err
    twice = [dict(ids[0], rank=r, device=r, visible_devices="0,0||") for r in range(2)]        # one card listed twice
    n, err = bench.check_distinct_gpus(twice, 2, False)
    assert n == 1 and err
    # one device per rank through per-rank masks (every ordinal 0): the bus ids decide
    masked = [dict(ids[r], device=0, visible_devices=str(r)) for r in range(4)]
    assert bench.check_distinct_gpus(masked, 4, False) == (4, None)
    n, err = bench.check_distinct_gpus([dict(ids[0], device=0, visible_devices="0"), dict(ids[0], rank=1, device=0, visible_devices="0")], 2, False)
    assert n == 1 and err


def test_gpu_identity_degrades_quietly_without_a_device(pkg):
    """The identity record of a rank is best effort beyond the ordinal: no device, no bus id -- and no exception."""
    if pkg.device_count() > 0:
        import pytest
        pytest.skip("a GPU is visible")
    ident = bench.gpu_identity(pkg, 0, 3)
    assert ident["rank"] == 3 and ident["device"] == 0 and ident["pci_bus_id"] is None and ident["host"]
    assert pkg.device_pci_bus_id(0) is None and pkg.device_pci_bus_id(-1) is None
    assert bench.check_distinct_gpus([ident, dict(ident, rank=4, device=1)], 2, False) == (2, None)


def test_without_a_gpu_the_benchmark_refuses(pkg):
    if pkg.device_count() > 0:
        import pytest
        pytest.skip("a GPU is visible")
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode != 0
    assert "no MI355X visible" in (res.stderr + res.stdout)
    assert "{" not in res.stdout           # no JSON line is fabricated


def test_profiled_traffic_is_labelled_with_its_box_and_build():
    """`roofline.traffic` is null unless the run itself was profiled; the committed PMC figure travels as
    `traffic_profiled` with the plan, the box serial and the build hash it was measured on."""
    import json
    h = bench.build_hash()
    assert len(h) == 12 and int(h, 16) >= 0
    with open(os.path.join(ROOT, "profiles", "traffic_latest.json")) as f:
        t = json.load(f)
    assert {"plans", "box_serial", "build", "algorithmic_bytes_per_launch"} <= set(t)
    geo = t.get("by_geometry_and_plan", {})
    for band, plan in ((1, "band1"), (544, "chunk"), (0, "identity")):
        tp = bench.profiled_traffic(band)
        key = "3840x2160x64/%s" % plan
        plans_fresher = t.get("build") == h and t.get("by_geometry_build") != h and plan in t["plans"]
        if key in geo and not plans_fresher:    # keyed by geometry AND plan (VERDICT r02 #6b)
            assert tp["key"] == key and tp["bytes"] == geo[key]["hbm_bytes_per_launch"]
            assert tp["box_serial"] == t.get("by_geometry_box_serial") and tp["build"] == t.get("by_geometry_build")
            assert tp["build_matches_this_run"] == (t.get("by_geometry_build") == h)
            assert 1.0 <= tp["bytes"] / geo[key]["algorithmic_bytes_per_launch"] < 1.2
        else:                            # ... unless the per-plan pass of the bench batch is the one taken on this build
            assert tp["plan"] == plan and tp["bytes"] == t["plans"][plan]["hbm_bytes_per_launch"]
            assert 1.0 <= tp["bytes"] / t["algorithmic_bytes_per_launch"] < 1.2
            assert tp["build_matches_this_run"] == (t.get("build") == h)
    # other geometries carry their own entries: generic sensor geometries, 8K, 1080p
    assert any(k.startswith("4056x3040x32/") for k in geo) and any(k.startswith("7680x4320x64/") for k in geo)


def test_stock_element_leg_times_a_pipeline_or_says_why_not(tmp_path, monkeypatch):
    """SURVEY 8(d) / VERDICT r02 #6a: the literal ORC element is timed through filesrc ! bayer2rgb ! fakesink when a
    stock plugin is installed; in this image none is, so the leg says so -- and the pipeline timer itself is
    exercised on `identity`, the element it subtracts."""
    import numpy as np
    leg = bench.stock_element_leg(sample_frames=2)
    assert leg["installed"] is False and "note" in leg          # no gst-plugins-bad (nor liborc) in this image
    tools = bench._gst_tools()
    if tools is None:
        import pytest
        pytest.skip("no GStreamer tools")
    launch, inspect, env = tools
    w, h, n = 640, 480, 6
    path = str(tmp_path / "frames.raw")
    np.zeros((n, h, w), np.uint8).tofile(path)
    el = bench.time_pipeline(launch, env, "identity", w, h, n, path, repeats=1)
    assert el is not None and 0 < el < 60
    assert bench.time_pipeline(launch, env, "no_such_element_xyz", w, h, n, path, repeats=1) is None


def test_cpu_baseline_has_the_simd_leg_and_uses_every_core(monkeypatch):
    """SURVEY 8(d) / BASELINE.md section 4: an ORC-equivalent SIMD leg on one core and an all-cores leg whose thread
    count is the host's core count (VERDICT r01 missing #1), next to the scalar port and the reference's C path."""
    monkeypatch.setattr(bench, "WIDTH", 256)
    monkeypatch.setattr(bench, "HEIGHT", 64)
    cb = bench.cpu_baseline(budget_s=0.5, sample_frames=4)
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["unit"] == "Mpix/s"
    assert cb["simd_1core"]["best"] in ("sse2", "avx2") and cb["value"] == cb["simd_1core"][cb["simd_1core"]["best"]]["value"]
    assert cb["scalar_1core"]["cores"] == 1 and cb["scalar_1core"]["value"] > 0
    ncores = len(os.sched_getaffinity(0))
    assert cb["all_cores"]["cores"] == ncores == cb["all_cores"]["host_cores"]
    assert cb["all_cores"]["jobs"] >= min(2 * ncores, 4 * 64)       # at least two jobs per core (bounded by the rows)
    if cb["reference_c_path"] is not None:
        assert cb["reference_c_path"]["kind"] == "reference" and cb["reference_c_path"]["cores"] == 1


def test_dump_sample_is_fixed_and_bounded():
    """--dump-outputs: the sampled byte positions are the same in every run (two builds are compared output for
    output), distinct, in range and sorted; the three arrays of the bench batch stay within 64 MB as float32."""
    import numpy as np
    total = bench.BATCH * bench.HEIGHT * 4 * bench.WIDTH
    a, b = bench.dump_sample_index(total), bench.dump_sample_index(total)
    assert np.array_equal(a, b) and a[0] >= 0 and a[-1] < total and (np.diff(a) > 0).all()
    assert len(a) > 0.99 * bench.DUMP_SAMPLE
    rows = bench.BATCH * 2 * bench.DUMP_BORDER_ROWS * 4 * bench.WIDTH
    cols = bench.BATCH * bench.HEIGHT * 2 * 4 * bench.DUMP_BORDER_COLS
    assert 4 * (len(a) + rows + cols) <= 64e6


def test_dump_outputs_writes_float32_copies_of_the_batch(tmp_path):
    """dump_outputs() on a host tensor: every array is float32 and holds exactly the bytes of the batch it names."""
    import numpy as np
    import torch
    frames, height, row_bytes = 3, 7, 48
    batch = np.random.default_rng(1).integers(0, 256, (frames, height, row_bytes), dtype=np.uint8)
    names = bench.dump_outputs(str(tmp_path), torch.from_numpy(batch.reshape(-1).copy()), frames, height, row_bytes)
    assert names == ["bgrx_border_cols", "bgrx_border_rows", "bgrx_sample"]
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["bgrx_sample"], batch.reshape(-1)[bench.dump_sample_index(batch.size)])
    rows = [0, 1, height - 2, height - 1]
    cols = list(range(8)) + list(range(row_bytes - 8, row_bytes))
    assert np.array_equal(got["bgrx_border_rows"], batch[:, rows, :])
    assert np.array_equal(got["bgrx_border_cols"], batch[:, :, cols])


def test_dump_outputs_is_refused_in_stream_mode(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "stream", "--dump-outputs",
                          str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--dump-outputs" in res.stderr and "{" not in res.stdout
