#!/usr/bin/env python3
"""bench.py -- bayer2rgb Mpix/s @4K on MI355X, with the HBM roofline and the CPU baseline beside it.

Contract (driver):  python bench.py --gpus N --steps K --warmup W
  N > 1 is launched by the driver as `python -m torch.distributed.run --nproc-per-node N ... bench.py
  --gpus N ...`, one rank per GPU; barriers and the max-over-ranks run over RCCL (gloo only if the RCCL
  communicator cannot be brought up).  Rank 0 prints ONE JSON line.

Workload = BASELINE.json configs[2]: 3840x2160, batch = 64 frames per GPU, all four Bayer orders
(step i converts the batch as order ORDERS[i % 4] -> BGRx; the kernel is the same for all four, only
its v_perm selectors / row-type swap differ).  A "step" is one pass of the hot path over one batch:
ONE kernel launch through the C ABI (mibayer_process_device) on frames already resident in HBM.
Frames are sharded round-robin over ranks (global frame g -> rank g % N), no collective on the data
path; per-GPU work is fixed as N grows ("weak").

The JSON line also carries
  roofline     achieved algorithmic GB/s of the kernel (5 B/pixel: 1 read + 4 written) from HIP
               events on the launch stream over the timed region, against the 8 TB/s HBM3E peak.
A plain run does only that: set-up (incl. the measured plan selection), pre-warm, W warm-up steps, the K
timed steps, the optional --dump-outputs, the line.  --full adds everything else, after the timed region:
  parity       a spot check of the batch against the CPU oracle (config.parity, per_gpu[].parity);
  host_path    the PCIe-inclusive host path, three arms (rank 0, N == 1 only);
  roofline.traffic  HBM bytes per launch measured by a rocprofv3 PMC child of this script (N == 1 only);
  cpu_baseline the CPU oracle (a port of the reference algorithm, oracle/) timed on this box's host
               cores on a bounded sample of the same frames (rank 0, N == 1 only).
The oracle is imported here ONLY for that baseline leg and the parity spot check.

--dump-outputs DIR writes what the last timed step computed (rank 0's BGRx batch) as float32 .npy files:
a fixed, seeded sample of the batch and the border rows / columns of every frame (dump_outputs()).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTH, HEIGHT, BATCH = 3840, 2160, 64
ORDERS = ("bggr", "rggb", "grbg", "gbrg")
FORMAT = "BGRx"
SEED = 2                         # config 3 uses seed 2
BYTES_PER_PIXEL = 5              # algorithmic: 1 B mosaic read + 4 B RGBx written
HBM_PEAK_GBPS = 8000.0           # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
PLAN_SOURCES = ("default", "measured", "cached", "set")      # MIBAYER_PLAN_*


# ----------------------------------------------------------------------------------------------
# distributed harness (also exercised on CPU with gloo, tests/test_sharding.py)
# ----------------------------------------------------------------------------------------------

def shard_frames(total_frames, world_size, rank):
    """Round-robin frame -> rank map of the north star: global frame g runs on rank g % N."""
    return list(range(rank, total_frames, world_size))


def timed_region(step_fn, steps, warmup, sync_fn, dist=None, info=None):
    """W untimed warm-up steps, then exactly K steps bracketed by barrier + device sync on both
    sides.  Returns the MAX over ranks of the elapsed seconds.  `info` (a dict) receives `barrier_ms`: the wall time
    of the closing barrier on this rank (it sits inside the timed region, as the contract asks, so a slow control
    plane shows up in `value`; this is how much)."""
    for i in range(warmup):
        step_fn(i)
    sync_fn()
    if dist is not None:
        dist.barrier()
    sync_fn()
    t0 = time.perf_counter()
    for i in range(steps):
        step_fn(warmup + i)
    sync_fn()
    tb = time.perf_counter()
    if dist is not None:
        dist.barrier()
    sync_fn()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    if info is not None:
        info["barrier_ms"] = (t1 - tb) * 1e3 if dist is not None else 0.0
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def aggregate_mpix_per_s(pixels_per_step_per_rank, world_size, steps, elapsed_s):
    return pixels_per_step_per_rank * world_size * steps / elapsed_s / 1e6


# ----------------------------------------------------------------------------------------------
# CPU baseline (oracle) -- reported beside the GPU number, never the thing optimised
# ----------------------------------------------------------------------------------------------

def _gst_tools():
    """(gst-launch-1.0, gst-inspect-1.0, env) of the GStreamer this box has, or None."""
    import shutil
    prefix = os.environ.get("GST_PREFIX", "/opt/conda")
    for bindir in (os.path.join(prefix, "bin"), "/usr/bin", "/usr/local/bin"):
        launch, inspect = os.path.join(bindir, "gst-launch-1.0"), os.path.join(bindir, "gst-inspect-1.0")
        if os.path.exists(launch) and os.path.exists(inspect):
            env = dict(os.environ)
            if bindir.startswith(prefix):       # a conda GStreamer does not find its own plugins by default
                env.setdefault("GST_PLUGIN_SYSTEM_PATH_1_0", os.path.join(prefix, "lib", "gstreamer-1.0"))
                env.setdefault("GST_PLUGIN_SCANNER", os.path.join(prefix, "libexec", "gstreamer-1.0",
                                                                   "gst-plugin-scanner"))
            env["GST_REGISTRY"] = os.path.join(os.environ.get("TMPDIR", "/tmp"), "mibayer_bench_gst_registry.bin")
            env.pop("GST_PLUGIN_PATH_1_0", None)    # never this repository's own plugin
            env.pop("GST_PLUGIN_PATH", None)
            return launch, inspect, env
    if shutil.which("gst-launch-1.0") and shutil.which("gst-inspect-1.0"):
        return shutil.which("gst-launch-1.0"), shutil.which("gst-inspect-1.0"), dict(os.environ)
    return None


def time_pipeline(launch, env, element, width, height, frames, path, repeats=2, timeout=120):
    """Wall seconds of `filesrc ! video/x-bayer ! <element> ! fakesink` over `frames` frames of `path`, best of
    `repeats` (the file stays in the page cache); None if the pipeline fails."""
    caps = "video/x-bayer,format=rggb,width=%d,height=%d,framerate=30/1" % (width, height)
    cmd = [launch, "-q", "filesrc", "location=" + path, "blocksize=%d" % (((width + 3) & ~3) * height), "!",
           caps, "!"] + element.split() + ["!", "fakesink", "sync=false"]
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        el = time.perf_counter() - t0
        if res.returncode != 0:
            return None
        best = el if best is None else min(best, el)
    return best


def stock_element_leg(sample_frames=24, budget_s=20.0):
    """SURVEY.md section 8(d) / BASELINE.md section 4: where a STOCK gst-plugins-bad `bayer2rgb` -- the literal ORC
    element, not this repository's -- is installed on the box, it is timed through
    `filesrc ! video/x-bayer ! bayer2rgb ! fakesink` (call site gstbayer2rgb.c:456-487) on the same synthetic 4K
    frames, with the same pipeline around `identity` subtracted (file read, caps, buffer hand-over), as in SURVEY.md
    section 6.  This image ships GStreamer 1.14 without gst-plugins-bad and without liborc, and the reference cannot
    travel to the GPU box, so there the leg reports that nothing is installed."""
    tools = _gst_tools()
    if tools is None:
        return {"installed": False, "note": "no GStreamer tools on this box"}
    launch, inspect, env = tools
    try:
        res = subprocess.run([inspect, "bayer2rgb"], env=env, capture_output=True, text=True, timeout=60)
    except Exception as exc:       # noqa: BLE001
        return {"installed": False, "note": "gst-inspect-1.0 failed: %s" % str(exc)[:100]}
    if res.returncode != 0:
        return {"installed": False, "note": "no stock gst-plugins-bad bayer plugin (nor liborc) on this box "
                                            "(gst-inspect-1.0 bayer2rgb finds nothing outside this repository)"}
    where = [ln.split()[-1] for ln in res.stdout.splitlines() if ln.strip().startswith("Filename")]
    if where and os.path.abspath(where[0]).startswith(ROOT):
        return {"installed": False, "note": "the only bayer2rgb in the registry is this repository's own"}
    import numpy as np
    import __graft_entry__ as entry
    oracle = entry.load_oracle()
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "mibayer_bench_stock_%d.raw" % os.getpid())
    try:
        oracle.fill_synthetic(WIDTH, HEIGHT, sample_frames, SEED).tofile(path)
        base = time_pipeline(launch, env, "identity", WIDTH, HEIGHT, sample_frames, path)
        conv = time_pipeline(launch, env, "bayer2rgb ! video/x-raw,format=%s" % FORMAT, WIDTH, HEIGHT, sample_frames,
                             path, timeout=max(60, int(budget_s * 6)))
    finally:
        try:
            os.remove(path)
        except OSError:
            pass
    if base is None or conv is None or conv <= base:
        return {"installed": True, "path": where[0] if where else None,
                "note": "present, but the timing pipeline did not run (identity %r s, bayer2rgb %r s)" % (base, conv)}
    return {"installed": True, "path": where[0] if where else None, "cores": 1, "kind": "reference",
            "value": round(WIDTH * HEIGHT * sample_frames / (conv - base) / 1e6, 1), "unit": "Mpix/s",
            "pipeline_seconds": round(conv, 3), "identity_pipeline_seconds": round(base, 3),
            "note": "stock ORC element through filesrc ! bayer2rgb ! fakesink, %d 4K frames (seed %d), identity "
                    "pipeline subtracted, best of 2; single-threaded per stream" % (sample_frames, SEED)}


def cpu_baseline(budget_s=12.0, sample_frames=32):
    """Four legs on this box's host cores, all on the same 32 frames, all byte-identical restatements of the
    reference path (tests/test_oracle.py):
      simd_1core       the two ORC programs as the pavgb / punpck sequences they compile to (oracle/bayer2rgb_simd.c,
                       SSE2 as ORC's x86-64 backend of the 1.19 era emits, and AVX2 where the CPU has it), one
                       thread -- what one reference element does per stream; this is `value`;
      scalar_1core     the plain-C restatement (gcc -O3 auto-vectorised), one thread;
      all_cores        the best SIMD form on EVERY host core (frames x row bands = jobs >= 2 per core);
      reference_c_path the reference's own compiled row kernels (oracle/_ref, its -DDISABLE_ORC C path), one thread.
    """
    import numpy as np
    import __graft_entry__ as entry
    oracle = entry.load_oracle()
    ncores = os.cpu_count() or 1
    try:
        ncores = len(os.sched_getaffinity(0)) or ncores
    except (AttributeError, OSError):
        pass
    src = oracle.fill_synthetic(WIDTH, HEIGHT, sample_frames, SEED)
    dst = np.empty((sample_frames, HEIGHT, 4 * WIDTH), np.uint8)
    r, g, b = oracle.LAYOUTS[FORMAT]
    # all cores: frames x row bands, at least two jobs per core
    nbands_all = max(1, -(-2 * ncores // sample_frames))
    # page-in with the job -> thread map of the all-cores leg: every output page is first touched (and so placed,
    # on a multi-socket host) by the thread that writes it later
    oracle.bayer2rgb_batch_bands(src, WIDTH, "rggb", r, g, b, nbands_all, ncores, "own", dst)

    def run(mode, nthreads, nbands, budget, repeat=1):
        reps, t0 = 0, time.perf_counter()
        while True:
            oracle.bayer2rgb_batch_bands(src, WIDTH, ORDERS[reps % 4], r, g, b, nbands, nthreads, mode, dst,
                                         repeat=repeat)
            reps += repeat
            el = time.perf_counter() - t0
            if el >= budget:
                return WIDTH * HEIGHT * sample_frames * reps / el / 1e6, reps, el

    share = budget_s / 5.0
    isas = oracle.simd_isas()
    simd = {}
    for isa in isas:
        v, reps, el = run(isa, 1, 1, share / len(isas) * 1.5)
        simd[isa] = {"value": round(v, 1), "passes": reps, "seconds": round(el, 2)}
    best_isa = max(simd, key=lambda k: simd[k]["value"])
    vs, repss, els = run("own", 1, 1, share)
    # every core: one quick pass sizes `repeat` so that a call lasts ~0.25 s and creating / joining `ncores` threads
    # is not what is being timed
    nbands = nbands_all
    t0 = time.perf_counter()
    oracle.bayer2rgb_batch_bands(src, WIDTH, "rggb", r, g, b, nbands, ncores, best_isa, dst)
    one = max(time.perf_counter() - t0, 1e-4)
    vn, repsn, eln = run(best_isa, ncores, nbands, share * 1.5, repeat=max(1, min(200, int(0.25 / one))))
    ref = None
    if oracle.have_ref_rows():
        # the reference's own compiled row kernels (gstbayerorc-dist.c, -DDISABLE_ORC = its C backup path)
        # under the restated frame driver; prebuilt in the build container, travels as a binary
        vr, repsr, elr = run("ref", 1, 1, share)
        ref = {"value": round(vr, 1), "cores": 1, "kind": "reference", "passes": repsr,
               "note": "oracle/_ref row kernels = reference gstbayerorc-dist.c built -DDISABLE_ORC -O2 (the "
                       "reference's no-ORC C path, not the ORC JIT), restated frame driver"}
    return {
        "value": simd[best_isa]["value"], "unit": "Mpix/s", "cores": 1, "kind": "port",
        "sample": "%d of the %d 4K frames (seed %d, frames 0-%d) -> %s, all 4 orders cycled, %d passes in %.1f s; "
                  "ORC-equivalent %s row kernels (oracle/bayer2rgb_simd.c: avgub = pavgb, mergebw/mergewl = "
                  "punpck, gstbayerorc.orc:3-19, 43-92) under the restated frame driver, 1 thread (the reference "
                  "element is single-threaded per stream)" % (
                      sample_frames, BATCH, SEED, sample_frames - 1, FORMAT, simd[best_isa]["passes"],
                      simd[best_isa]["seconds"], best_isa.upper()),
        "simd_1core": dict(simd, best=best_isa, cores=1),
        "scalar_1core": {"value": round(vs, 1), "cores": 1, "passes": repss,
                         "note": "oracle/bayer2rgb_oracle.c, plain C, gcc -O3 auto-vectorised"},
        "all_cores": {"value": round(vn, 1), "cores": ncores, "host_cores": ncores, "passes": repsn,
                      "isa": best_isa, "jobs": sample_frames * nbands,
                      "note": "pthreads, %d frames x %d row bands = %d jobs round-robin over %d threads (every "
                              "host core), several passes per thread creation, output pages first touched by the "
                              "thread that writes them" % (sample_frames, nbands, sample_frames * nbands, ncores)},
        "reference_c_path": ref,
        "stock_orc_element": stock_element_leg(),
    }


# ----------------------------------------------------------------------------------------------
# GPU benchmark
# ----------------------------------------------------------------------------------------------

def parity_spot_check(pkg, ctxs, d_src, d_dst, rank, world, stream):
    """Frame 0 and the last frame of this rank's batch, order rggb, against the oracle."""
    import numpy as np
    import torch
    import __graft_entry__ as entry
    oracle = entry.load_oracle()
    ctx = ctxs["rggb"]
    ctx.process_device(d_src.data_ptr(), d_dst.data_ptr(), BATCH, stream=stream)
    torch.cuda.synchronize()
    r, g, b = oracle.LAYOUTS[FORMAT]
    for local in (0, BATCH - 1):
        gframe = rank + local * world
        src = oracle.fill_synthetic(WIDTH, HEIGHT, 1, SEED, first_frame=gframe)[0]
        want = oracle.bayer2rgb(src, WIDTH, "rggb", r, g, b).reshape(-1)
        got = d_dst[local * ctx.dst_bytes:(local + 1) * ctx.dst_bytes].cpu().numpy()
        if not np.array_equal(got, want):
            raise AssertionError("bench parity check failed: rank %d local frame %d differs from "
                                 "the oracle in %d bytes" % (rank, local, int((got != want).sum())))
    return "bit-exact vs oracle on frames %d and %d of the batch (rggb->%s)" % (0, BATCH - 1, FORMAT)


DUMP_SEED = 20261016             # fixes the sampled byte positions of --dump-outputs
DUMP_SAMPLE = 6 << 20            # sampled bytes of the batch (float32: 24 MiB)
DUMP_BORDER_ROWS = 2             # rows at the top and at the bottom of every frame
DUMP_BORDER_COLS = 2             # pixels at the left and at the right edge of every row


def dump_sample_index(total_bytes, n=DUMP_SAMPLE, seed=DUMP_SEED):
    """Sorted, distinct byte offsets into the output batch: the same for every run of the same geometry."""
    import numpy as np
    return np.unique(np.random.default_rng(seed).integers(0, total_bytes, n, dtype=np.int64))


def dump_outputs(out_dir, d_dst, frames, height, row_bytes):
    """The BGRx batch the last timed step wrote (d_dst: uint8 device tensor, frames x height x row_bytes), as float32
    arrays in out_dir: bgrx_sample.npy (the bytes at dump_sample_index(), in index order) and bgrx_border_rows.npy /
    bgrx_border_cols.npy (frames x rows x row_bytes, frames x height x bytes: the demosaic's edge cases).  The whole
    batch is 2 GB; these are about 50 MB."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    idx = torch.from_numpy(dump_sample_index(d_dst.numel())).to(d_dst.device)
    batch = d_dst.view(frames, height, row_bytes)
    rows = list(range(DUMP_BORDER_ROWS)) + list(range(height - DUMP_BORDER_ROWS, height))
    cols = list(range(4 * DUMP_BORDER_COLS)) + list(range(row_bytes - 4 * DUMP_BORDER_COLS, row_bytes))
    arrays = {"bgrx_sample": d_dst[idx],
              "bgrx_border_rows": batch[:, rows, :],
              "bgrx_border_cols": batch[:, :, cols]}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.to(torch.float32).cpu().numpy())
    return sorted(arrays)


def sched_snapshot():
    """Where a stall of the host path could come from on the HOST side: per thread of this process the time spent
    runnable but not running (/proc/self/task/*/schedstat, second field, ns), the cgroup's CFS-quota throttling
    (cpu.stat) and the system's CPU pressure (/proc/pressure/cpu `some total`, us).  Best effort: {} where /proc says
    nothing."""
    snap = {"threads": {}, "throttled_ms": None, "psi_some_ms": None}
    try:
        for tid in os.listdir("/proc/self/task"):
            try:
                with open("/proc/self/task/%s/schedstat" % tid) as f:
                    run_ns, wait_ns = f.read().split()[:2]
                with open("/proc/self/task/%s/comm" % tid) as f:
                    comm = f.read().strip()
                snap["threads"][tid] = (int(wait_ns), comm)
            except (OSError, ValueError):
                pass
    except OSError:
        pass
    for path, key, scale in (("/sys/fs/cgroup/cpu.stat", "throttled_usec", 1e-3),
                             ("/sys/fs/cgroup/cpu/cpu.stat", "throttled_time", 1e-6)):
        try:
            with open(path) as f:
                for ln in f:
                    if ln.split()[0] == key:
                        snap["throttled_ms"] = int(ln.split()[1]) * scale
        except (OSError, IndexError, ValueError):
            pass
    try:
        with open("/proc/pressure/cpu") as f:
            for ln in f:
                if ln.startswith("some"):
                    snap["psi_some_ms"] = int(ln.split("total=")[1]) * 1e-3
    except (OSError, IndexError, ValueError):
        pass
    return snap


def sched_delta(before, after):
    """What changed between two sched_snapshot()s: the thread that waited longest for a CPU (ms, name), CFS throttling
    and CPU pressure during the interval."""
    worst, who = 0.0, None
    for tid, (wait_ns, comm) in after["threads"].items():
        d = (wait_ns - before["threads"].get(tid, (0, comm))[0]) * 1e-6
        if d > worst:
            worst, who = d, comm

    def diff(key):
        return None if after[key] is None or before[key] is None else round(after[key] - before[key], 2)
    return {"max_thread_runqueue_wait_ms": round(worst, 2), "thread": who, "threads": len(after["threads"]),
            "cgroup_throttled_ms": diff("throttled_ms"), "cpu_pressure_some_ms": diff("psi_some_ms")}


def host_path_rate(pkg, device, frames=240, inflight=3, flags=0, graph_mode=None, stats=None):
    """PCIe-inclusive rate of the host path (hipHostMalloc-pinned buffers, async ring).  flags=FLAG_HIPGRAPH: the
    compute-queue segment of every slot (wait for the upload -> kernel -> signal the download) is a captured graph,
    one hipGraphLaunch per frame, the copies stay on the copy queues; graph_mode="chain": the A/B arm that puts the
    whole H2D -> kernel -> D2H chain of a slot into one graph on the slot's own queue (MIBAYER_FLAG_HIPGRAPH_CHAIN).
    `stats` (a dict) receives the host CPU the timed frames cost (mibayer_get_host_stats), the per-frame latency
    (submit -> mibayer_wait returns) and completion-interval distribution, the mean interval of every tenth of the run
    (a slow PHASE -- clocks, a neighbour on the link -- shows as a step in it; a slow STATE as a flat line at twice the
    usual figure) and where the pinned blocks live relative to the card (VERDICT r05 Weak 3: a 24-frame arm halved in 2
    of 8 recorded runs and nothing in the record said why).
    Returns (Mpix/s, seconds)."""
    import ctypes
    import numpy as np
    L = pkg.lib()
    if graph_mode == "chain":
        flags |= pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN
    with pkg.Context(WIDTH, HEIGHT, "rggb", FORMAT, device=device, inflight=inflight, flags=flags) as ctx:
        srcs, dsts = [], []
        for _ in range(inflight):
            # pinned staging on the NUMA node next to THIS rank's GPU (on a two-socket 8-GPU node half the ranks
            # would otherwise copy across the socket link)
            ps = L.mibayer_host_alloc_near(device, ctx.src_bytes)
            pd = L.mibayer_host_alloc_near(device, ctx.dst_bytes)
            s = np.ctypeslib.as_array(ctypes.cast(ps, ctypes.POINTER(ctypes.c_uint8)), (ctx.src_bytes,))
            d = np.ctypeslib.as_array(ctypes.cast(pd, ctypes.POINTER(ctypes.c_uint8)), (ctx.dst_bytes,))
            s[:] = 0x55
            srcs.append((ps, s))
            dsts.append((pd, d))
        for phase in ("warm", "timed"):
            n = 2 * inflight if phase == "warm" else frames
            before = ctx.host_stats()
            sched0 = sched_snapshot()
            t_submit, t_done = {}, []
            t0 = time.perf_counter()
            for i in range(n):
                if ctx.pending() == inflight:
                    tag = ctx.wait()
                    now = time.perf_counter()
                    t_done.append((now, now - t_submit[tag]))
                t_submit[i + 1] = time.perf_counter()
                ctx.submit(srcs[i % inflight][1], dsts[i % inflight][1], tag=i + 1)
            while ctx.pending():
                tag = ctx.wait()
                now = time.perf_counter()
                t_done.append((now, now - t_submit[tag]))
            el = time.perf_counter() - t0
            sched1 = sched_snapshot()
        if stats is not None:
            after = ctx.host_stats()
            gaps = np.diff(np.array([t for t, _ in t_done])) * 1e6
            lat = np.array([l for _, l in t_done]) * 1e6
            stats.update({"submit_cpu_us_per_frame": round((after["submit_cpu_ms"] - before["submit_cpu_ms"]) * 1e3 / frames, 1),
                          "wait_cpu_us_per_frame": round((after["wait_cpu_ms"] - before["wait_cpu_ms"]) * 1e3 / frames, 1),
                          "wait_wall_us_per_frame": round((after["wait_wall_ms"] - before["wait_wall_ms"]) * 1e3 / frames, 1),
                          "polls_per_frame": round((after["polls"] - before["polls"]) / frames, 1),
                          "naps_per_frame": round((after["naps"] - before["naps"]) / frames, 1),
                          "latency_us": {"p50": round(float(np.percentile(lat, 50)), 1),
                                         "p99": round(float(np.percentile(lat, 99)), 1), "max": round(float(lat.max()), 1)},
                          "completion_interval_us": {"p50": round(float(np.percentile(gaps, 50)), 1),
                                                     "p99": round(float(np.percentile(gaps, 99)), 1),
                                                     "max": round(float(gaps.max()), 1)},
                          "interval_by_tenth_of_run_us": [round(float(x.mean())) for x in np.array_split(gaps, 10)],
                          # host side of a stall: did a thread of this process (the HSA runtime's signal thread, say)
                          # wait for a CPU, was the cgroup throttled, was the machine short of CPUs
                          "sched": sched_delta(sched0, sched1),
                          "placement": {"device_numa_node": L.mibayer_device_numa_node(device),
                                        "pinned_src_nodes": [L.mibayer_host_numa_node(ps) for ps, _ in srcs],
                                        "pinned_dst_nodes": [L.mibayer_host_numa_node(pd) for pd, _ in dsts],
                                        "cpu": ctypes.CDLL(None).sched_getcpu()}})
        for (ps, _), (pd, _) in zip(srcs, dsts):
            L.mibayer_host_free(ps)
            L.mibayer_host_free(pd)
    return WIDTH * HEIGHT * frames / el / 1e6, el


HOST_PATH_FRAMES = 240


def host_path_note(pkg, device):
    host_path_rate(pkg, device, 24, 3, 0)       # first touch of the copy queues and the PCIe link: not measured
    cpu, gcpu = {}, {}
    plain, _ = host_path_rate(pkg, device, HOST_PATH_FRAMES, 3, 0, stats=cpu)
    graph, _ = host_path_rate(pkg, device, HOST_PATH_FRAMES, 3, pkg.FLAG_HIPGRAPH, stats=gcpu)
    chain, _ = host_path_rate(pkg, device, HOST_PATH_FRAMES // 2, 3, pkg.FLAG_HIPGRAPH, "chain")
    return {"value": round(max(plain, graph), 1), "unit": "Mpix/s", "streams_and_events": round(plain, 1),
            "hipgraph_captured_launch": round(graph, 1), "hipgraph_whole_chain_per_slot": round(chain, 1),
            "frames_per_arm": HOST_PATH_FRAMES,
            "host_cpu": cpu,
            "hipgraph_arm": {k: gcpu[k] for k in ("latency_us", "completion_interval_us", "interval_by_tenth_of_run_us",
                                                  "sched")},
            "note": "host->host incl. H2D + D2H over PCIe, hipHostMalloc-pinned buffers, 3 frames in flight, %d 4K "
                    "frames per arm; bound by PCIe (5 B/pixel over a Gen5 x16 link), not HBM; never `value`; host_cpu = "
                    "CPU time of the submitting / waiting thread per frame, latency (submit -> wait returns) and "
                    "completion intervals (streams+events arm = the element's default mode)" % HOST_PATH_FRAMES}


def build_hash():
    """First 12 hex digits of the sha256 over the kernel sources: ties a profiled traffic figure to a build."""
    import hashlib
    h = hashlib.sha256()
    for name in ("mibayer_kernels.hip", "mibayer_internal.h", "mibayer_abi.hip"):
        with open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:12]


def profiled_traffic(band, variant_name=None):
    """The PMC-measured HBM bytes per launch of the geometry and block order this run used, from the last profiled
    pass (profiles/traffic_latest.json, keyed "<W>x<H>x<N>/<plan>"; tools/summarize_geometry_counters.py): NOT a
    measurement of this run, hence not `traffic`."""
    path = os.path.join(ROOT, "profiles", "traffic_latest.json")
    try:
        with open(path) as f:
            t = json.load(f)
        plan = "band1" if band == 1 else ("chunk" if band > 1 else "identity")
        key = "%dx%dx%d/%s" % (WIDTH, HEIGHT, BATCH, plan)
        entry = (t.get("by_geometry_and_plan") or {}).get(key)
        if t.get("build") == build_hash() and t.get("by_geometry_build") != build_hash() and plan in (t.get("plans") or {}):
            entry = None        # the per-plan pass of the bench batch was taken on THIS build, the per-geometry one was not
        if entry is not None:
            return {"bytes": entry["hbm_bytes_per_launch"], "read_bytes": entry.get("read_bytes"),
                    "write_bytes": entry.get("write_bytes"), "key": key, "kernel": entry.get("kernel"),
                    "box_serial": t.get("by_geometry_box_serial"), "build": t.get("by_geometry_build"),
                    "build_matches_this_run": t.get("by_geometry_build") == build_hash(),
                    "file": "profiles/traffic_latest.json", "source": t.get("by_geometry_source")}
        entry = t["plans"][plan]
        return {"bytes": entry["hbm_bytes_per_launch"], "read_bytes": entry.get("read_bytes"),
                "write_bytes": entry.get("write_bytes"), "plan": plan, "box_serial": t.get("box_serial"),
                "build": t.get("build"), "build_matches_this_run": t.get("build") == build_hash(),
                "file": "profiles/traffic_latest.json", "source": t.get("source")}
    except Exception:       # noqa: BLE001 -- no profile committed yet
        return None


def parse_pmc_csv(path, counter, kernel_substr="bayer2rgb", last=8):
    """rocprofv3 `--pmc <counter> --output-format csv` counter_collection file -> (kernel name, mean counter value over
    the last `last` dispatches of kernels whose name contains `kernel_substr`, dispatches used); (None, None, 0) when
    the file holds no such row."""
    import csv
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if r.get("Counter_Name") == counter and kernel_substr in r.get("Kernel_Name", ""):
                rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"], float(r["Counter_Value"])))
    if not rows:
        return None, None, 0
    # one row per dispatch (a counter may be reported per dimension: sum those of one dispatch)
    per = {}
    for did, name, val in rows:
        per.setdefault(did, [name, 0.0])[1] += val
    ids = sorted(per)[-last:]
    return per[ids[-1]][0], sum(per[i][1] for i in ids) / len(ids), len(ids)


# gfx950 corrections of MI355X_MICROARCH.md "HBM": FETCH_SIZE (KiB) reports half of a wide coalesced streaming read
# -> x2; WRITE_SIZE (KiB) was calibrated 1:1 on a known byte count in this access pattern (tools/hbm_probe.hip,
# profiles/r02_summary.md, r03_summary.md)
PMC_TO_BYTES = {"FETCH_SIZE": 1024.0 * 2.0, "WRITE_SIZE": 1024.0}


def find_rocprofv3():
    import shutil
    return shutil.which("rocprofv3") or (
        "/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)


def measure_traffic(plan, launches=8, timeout_s=120.0):
    """HBM bytes per launch of the plan this run just timed, measured IN this run: bench.py re-launches itself as a
    small child (`--traffic-pass`: the same 64-frame 4K batch, the same kernel plan, `launches` launches, no torch)
    under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and again under `--pmc WRITE_SIZE` (separate passes; they do
    not fit one), after the timed region.  plan = (variant name, band override, store alignment).  Returns the
    `roofline.traffic` object, or (None, reason)."""
    import shutil
    import tempfile
    rocprof = find_rocprofv3()
    if rocprof is None:
        return None, "rocprofv3 not on PATH"
    if "rocprofiler" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ):
        return None, "this run is itself profiled (rocprofv3 wraps it): no nested profiler"
    t_start = time.perf_counter()
    tmp = tempfile.mkdtemp(prefix="mibayer_traffic_", dir=os.environ.get("TMPDIR", "/tmp"))
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK",
                        "LOCAL_WORLD_SIZE", "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
    env["TMPDIR"] = tmp
    got, kernel, used, child = {}, None, 0, None
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out_dir = os.path.join(tmp, counter)
            cmd = [rocprof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out_dir, "-o", "t",
                   "--", sys.executable, os.path.abspath(__file__), "--traffic-pass", "%s:%d:%d" % plan,
                   "--traffic-launches", str(launches)]
            left = timeout_s - (time.perf_counter() - t_start)
            if left < 5:
                return None, "traffic pass ran out of its %.0f s budget before the %s pass" % (timeout_s, counter)
            try:
                res = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=left)
            except subprocess.TimeoutExpired:
                return None, "rocprofv3 --pmc %s did not finish within %.0f s" % (counter, left)
            if res.returncode != 0:
                return None, "rocprofv3 --pmc %s exited %d: %s" % (counter, res.returncode,
                                                                  (res.stderr or res.stdout)[-200:].replace("\n", " "))
            for line in res.stdout.splitlines():
                if line.startswith("{") and "traffic_pass" in line:
                    child = json.loads(line)
            files = []
            for root, _, names in os.walk(out_dir):
                files += [os.path.join(root, n) for n in names if n.endswith("counter_collection.csv")]
            if not files:
                return None, "rocprofv3 --pmc %s wrote no counter_collection.csv" % counter
            kernel, mean, used = parse_pmc_csv(files[0], counter, last=launches)
            if mean is None:
                return None, "no bayer2rgb dispatch in the %s pass" % counter
            got[counter] = mean * PMC_TO_BYTES[counter]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    alg = BYTES_PER_PIXEL * WIDTH * HEIGHT * BATCH
    read, write = got["FETCH_SIZE"], got["WRITE_SIZE"]
    return {"read": round(read), "write": round(write), "total": round(read + write),
            "ratio": round((read + write) / alg, 4), "read_ratio": round(read / (WIDTH * HEIGHT * BATCH), 4),
            "write_ratio": round(write / (4 * WIDTH * HEIGHT * BATCH), 4), "unit": "bytes per launch",
            "kernel": kernel, "launches_averaged": used, "plan": "%s/band %d/align %d" % plan,
            "child_kernel_variant": (child or {}).get("kernel_variant"),
            "seconds": round(time.perf_counter() - t_start, 1),
            "method": "this run re-launched itself under rocprofv3 --kernel-trace --pmc FETCH_SIZE and --pmc "
                      "WRITE_SIZE (separate passes) after the timed region, same batch and plan; FETCH_SIZE KiB x 2 "
                      "(gfx950 correction), WRITE_SIZE KiB x 1"}, None


def traffic_child(args):
    """The profiled child of measure_traffic(): the bench workload under one explicit plan, no torch, no timing claims."""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    vname, band, align = args.traffic_pass.rsplit(":", 2)
    names = pkg.variant_names()
    ctxs = {o: pkg.Context(WIDTH, HEIGHT, o, FORMAT, device=0) for o in ORDERS}
    for c in ctxs.values():
        c.set_plan(names.index(vname), int(band), int(align))
    ctx0 = ctxs[ORDERS[0]]
    d_src = ctx0.device_alloc(BATCH * ctx0.src_bytes)
    d_dst = ctx0.device_alloc(BATCH * ctx0.dst_bytes)
    ctx0.fill_synthetic(d_src, BATCH, SEED)
    ctx0.sync()
    for i in range(2 + args.traffic_launches):
        c = ctxs[ORDERS[i % 4]]
        c.process_device(d_src, d_dst, BATCH, stream=ctx0.stream)
    ctx0.sync()
    print(json.dumps({"traffic_pass": args.traffic_pass, "kernel_variant": ctx0.variant_name,
                      "launch_plan": ctx0.launch_geometry(BATCH), "launches": args.traffic_launches}), flush=True)
    ctx0.device_free(d_src)
    ctx0.device_free(d_dst)
    for c in ctxs.values():
        c.close()


class ShmBarrier:
    """Barrier over a counter in /dev/shm for ranks of ONE host: what carries the two barriers of the timed region when
    the plane is gloo -- the fallback of an RCCL group that did not come up, or --backend gloo.  A gloo barrier of eight
    ranks costs 10-13 ms (profiles/r05_eight_ranks_one_gpu.json: barrier_ms 12.87) against a timed region of 8 ms, so a
    fallback more than halved `value` while saying loudly that it had happened (VERDICT r05 Weak 8); this one costs
    tens of microseconds.  Sense-reversing: a rank takes the file lock, counts itself in, and either opens the next
    generation (the last one in) or spins on the generation word.  The file is created by rank 0 and announced over
    the gloo group before anybody uses it; ranks of several hosts keep the gloo barrier."""

    def __init__(self, dist_mod, rank, world):
        import mmap
        import struct
        self._struct, self._world = struct, world
        hosts = [None] * world
        dist_mod.all_gather_object(hosts, os.uname().nodename)
        if len(set(hosts)) != 1:
            raise RuntimeError("ranks on %d hosts" % len(set(hosts)))
        path = [None]
        if rank == 0:
            path[0] = "/dev/shm/mibayer_bench_barrier_%d_%s" % (os.getpid(), os.environ.get("MASTER_PORT", "0"))
            with open(path[0], "wb") as f:
                f.write(b"\0" * 16)
        dist_mod.broadcast_object_list(path, src=0)
        self.path, self._owner = path[0], rank == 0
        self._f = open(self.path, "r+b")
        self._m = mmap.mmap(self._f.fileno(), 16)
        dist_mod.barrier()              # everybody has it mapped before anybody counts

    def wait(self, timeout_s=120.0):
        import fcntl
        fcntl.flock(self._f, fcntl.LOCK_EX)
        count, gen = self._struct.unpack_from("qq", self._m, 0)
        count += 1
        if count == self._world:
            self._struct.pack_into("qq", self._m, 0, 0, gen + 1)
        else:
            self._struct.pack_into("q", self._m, 0, count)
        fcntl.flock(self._f, fcntl.LOCK_UN)
        if count == self._world:
            return
        t0 = time.perf_counter()
        while self._struct.unpack_from("q", self._m, 8)[0] == gen:
            if time.perf_counter() - t0 > timeout_s:
                raise RuntimeError("shared-memory barrier timed out after %.0f s (a rank died?)" % timeout_s)

    def close(self):
        try:
            self._m.close()
            self._f.close()
            if self._owner:
                os.unlink(self.path)
        except OSError:
            pass


class ControlPlane:
    """Barrier and max-over-ranks for the timed region: the only communication of this bench (the data path has no
    collective).  Same small surface as the torch.distributed module, bound to one process group."""

    def __init__(self, dist_mod, group, backend, device, fallback_reason=None, rccl_nranks=None, shm=None):
        self._d, self._g, self._backend, self._device = dist_mod, group, backend, device
        self.ReduceOp = dist_mod.ReduceOp
        self.fallback_reason = fallback_reason      # RCCL was asked for and did not come up: why
        self._shm = shm                             # ShmBarrier: carries barrier() when the plane is gloo on one host
        self.barrier_transport = "rccl" if backend == "nccl" else ("shm" if shm is not None else "gloo")
        # what a sum-of-ones all-reduce on DEVICE tensors over the RCCL group returned when the plane was brought up
        # (= the number of ranks RCCL itself saw); None when the plane is not RCCL
        self.rccl_nranks = rccl_nranks

    def max_over_ranks(self, value):
        """MAX of one float over the ranks, on the plane's own transport (a device tensor over RCCL)."""
        import torch
        t = torch.tensor([value], dtype=torch.float64, device="cuda" if self._backend == "nccl" else "cpu")
        self.all_reduce(t, op=self.ReduceOp.MAX)
        return float(t.item())

    def get_backend(self):
        return self._backend

    def barrier(self):
        if self._backend == "nccl":
            self._d.barrier(group=self._g, device_ids=[self._device])
        elif self._shm is not None:
            self._shm.wait()
        else:
            self._d.barrier(group=self._g)

    def all_reduce(self, t, op):
        self._d.all_reduce(t, op=op, group=self._g)

    def gather_objects(self, obj):
        """One small host object per rank, for the per-GPU breakdown of the JSON line; always over the gloo bootstrap
        group (the default group), whatever carries the barriers."""
        out = [None] * self._d.get_world_size()
        self._d.all_gather_object(out, obj)
        return out

    def destroy_process_group(self):
        if self._shm is not None:
            self._shm.close()
        self._d.destroy_process_group()


def setup_distributed(args):
    """(world, rank, device ordinal, control plane or None).  One rank per GPU; the ranks bootstrap over gloo and
    then bring up an RCCL ("nccl") group for the barriers and the max-reduction.  If the RCCL communicator cannot be
    brought up (e.g. --share-gpu puts two ranks on one GPU) the gloo group carries them instead -- the measured
    region does not depend on it, and the JSON line says so at top level (`control_plane`, `control_plane_fallback`).
    --backend gloo skips RCCL.  --force-dist: a single rank goes through exactly the same bring-up (world size 1),
    so the RCCL branch is exercised on a one-GPU box."""
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no MI355X visible; the bayer2rgb path has no CPU fallback")
    device = local_rank % torch.cuda.device_count() if args.share_gpu else local_rank
    torch.cuda.set_device(device)
    plane = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:         # --force-dist outside a launcher
            import socket
            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
        dist_mod.init_process_group("gloo", rank=rank, world_size=world)

        def gloo_plane(why=None):
            # the barriers of a gloo plane go over shared memory when every rank is on this host (they are: --nnodes=1)
            try:
                shm = ShmBarrier(dist_mod, rank, world)
            except Exception as exc:    # noqa: BLE001 -- several hosts, no /dev/shm: the gloo barrier does
                sys.stderr.write("bench.py rank %d: no shared-memory barrier (%s); gloo barriers\n" % (rank, exc))
                shm = None
            return ControlPlane(dist_mod, None, "gloo", device, fallback_reason=why, shm=shm)
        plane = None
        if args.backend == "nccl":
            try:
                group = dist_mod.new_group(backend="nccl")
                probe = torch.ones(1, device="cuda")
                dist_mod.all_reduce(probe, group=group)
                torch.cuda.synchronize()
                if int(probe.item()) != world:
                    raise RuntimeError("all_reduce over RCCL returned %r for %d ranks" % (probe.item(), world))
                plane = ControlPlane(dist_mod, group, "nccl", device, rccl_nranks=int(probe.item()))
                plane.barrier()                     # the very call of the timed region, once outside it
                torch.cuda.synchronize()
            except Exception as exc:        # noqa: BLE001 -- any RCCL bring-up failure: keep the gloo plane, loudly
                why = "%s: %s" % (type(exc).__name__, str(exc)[:200])
                sys.stderr.write("bench.py rank %d: RCCL CONTROL PLANE UNAVAILABLE (%s); barriers and the "
                                 "max-reduction run over gloo\n" % (rank, why))
                plane = gloo_plane(why)
        if plane is None:
            plane = gloo_plane()
    return world, rank, device, plane


def gpu_identity(pkg, device, rank):
    """What this rank runs on, by hardware identity rather than by ordinal: PCI bus id of the HIP device, its NUMA
    node, the name and CU count the runtime reports.  Gathered into `per_gpu` so that the N > 1 line answers "did the
    ranks sit on N distinct GPUs" by itself."""
    ident = {"rank": rank, "device": device, "pci_bus_id": pkg.device_pci_bus_id(device),
             "numa_node": pkg.lib().mibayer_device_numa_node(device), "host": os.uname().nodename,
             # what this rank's ordinals are relative to (two ranks with the same mask and different ordinals sit on
             # different cards whatever the bus ids say)
             "visible_devices": "|".join(os.environ.get(k, "") for k in
                                         ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"))}
    try:
        import torch
        prop = torch.cuda.get_device_properties(device)
        ident["name"] = prop.name
        ident["compute_units"] = prop.multi_processor_count
        uuid = getattr(prop, "uuid", None)
        if uuid is not None:
            ident["uuid"] = str(uuid)
    except Exception:       # noqa: BLE001 -- identity is best effort beyond the bus id
        pass
    return ident


def check_distinct_gpus(identities, world, share_gpu):
    """(distinct_gpus, error or None) over the ranks' (host, PCI bus id) pairs.  Two ranks on one card halve each
    other's numbers silently, so that is refused unless --share-gpu (a testing mode) says it is meant."""
    def key(i):
        if i.get("pci_bus_id") or i.get("uuid"):
            return (i.get("host"), i.get("pci_bus_id"), i.get("uuid"))
        return (i.get("host"), "ordinal-%s" % i.get("device"), None)
    keys = [key(i) for i in identities]
    # a runtime that reports ONE bus id for several cards (some virtualised set-ups) must not stop a real multi-GPU run:
    # ranks of one host that share one visible-device mask and have different ordinals are on different cards
    by_ordinal = [(i.get("host"), i.get("visible_devices"), i.get("device")) for i in identities]

    def mask_is_plain(i):           # no card listed twice in a device mask (HIP_VISIBLE_DEVICES=0,0 is two ordinals, one card)
        return all(len(part.split(",")) == len(set(part.split(","))) for part in (i.get("visible_devices") or "").split("|"))
    distinct = len(set(keys))
    if distinct < world and len(set(by_ordinal)) == world and all(mask_is_plain(i) for i in identities):
        sys.stderr.write("bench.py: the runtime reports %d distinct bus ids / uuids for %d ranks with distinct ordinals "
                         "under one device mask; trusting the ordinals\n" % (distinct, world))
        distinct = world
    if distinct < world and not share_gpu:
        dup = sorted(set(k for k in keys if keys.count(k) > 1), key=str)
        return distinct, ("bench.py: %d ranks but only %d distinct GPUs (shared: %s); pass --share-gpu if that is "
                          "intended" % (world, distinct, ", ".join("%s/%s" % (k[0], k[1] or k[2]) for k in dup)))
    return distinct, None


def pin_to_device_node(pkg, device):
    """Host-fed ranks run on the CPUs of the NUMA node next to their GPU (best effort; returns the node or -1)."""
    try:
        node = pkg.lib().mibayer_device_numa_node(device)
        if node < 0:
            return -1
        cpus = set()
        with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
            for part in f.read().strip().split(","):
                a, _, b = part.partition("-")
                cpus.update(range(int(a), int(b or a) + 1))
        cpus &= set(os.sched_getaffinity(0))
        if cpus:
            os.sched_setaffinity(0, cpus)
        return node
    except (OSError, ValueError, AttributeError):
        return -1


def run_stream(args):
    """BASELINE.json configs[4]: 3840x2160 steady-state stream, pinned double-buffered H2D/D2H + hipGraph launch,
    1000 frames sharded round-robin over the ranks.  PCIe/host-DRAM-bound by construction."""
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    world, rank, local_rank, dist = setup_distributed(args)
    ident = gpu_identity(pkg, local_rank, rank)
    identities = dist.gather_objects(ident) if dist is not None else [ident]
    distinct_gpus, dup_error = check_distinct_gpus(identities, world, args.share_gpu)
    if dup_error:
        if dist is not None:
            dist.destroy_process_group()
        raise SystemExit(dup_error)
    node = pin_to_device_node(pkg, local_rank)
    total = 1000
    mine = len(shard_frames(total, world, rank))
    def timed(flags, graph_mode=None):
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        _, e = host_path_rate(pkg, local_rank, mine, 2, flags, graph_mode)
        if dist is not None:
            t = torch.tensor([e], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e = float(t.item())
        return e

    timed(0)                                     # clocks, page tables, first-touch of the pinned buffers
    el_streams = timed(0)
    el_chain = timed(pkg.FLAG_HIPGRAPH, "chain")
    el_graph = timed(pkg.FLAG_HIPGRAPH)
    el = el_streams if args.no_graph else el_graph
    # parity after the timed loops: one synthetic frame of this rank's share through the same host path
    oracle = entry.load_oracle()
    gframe = rank
    one = oracle.fill_synthetic(WIDTH, HEIGHT, 1, SEED, first_frame=gframe)[0]
    r, g, b = oracle.LAYOUTS[FORMAT]
    with pkg.Context(WIDTH, HEIGHT, "rggb", FORMAT, device=local_rank, inflight=2,
                     flags=0 if args.no_graph else pkg.FLAG_HIPGRAPH) as pctx:
        got = pctx.process_host(one)
    if not (got == oracle.bayer2rgb(one, WIDTH, "rggb", r, g, b)).all():
        raise AssertionError("bench stream parity check failed on rank %d" % rank)
    parity = "bit-exact vs oracle on global frame %d (rggb->%s, host path)" % (gframe, FORMAT)
    per_gpu = None
    if dist is not None:
        per_gpu = dist.gather_objects(dict(ident, pinned_to_numa_node=node, frames=mine, parity=parity))
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        px = WIDTH * HEIGHT * total
        print(json.dumps({
            "metric": "bayer2rgb Mpix/s @4K (host-fed stream incl. PCIe)", "value": round(px / el / 1e6, 1),
            "unit": "Mpix/s", "n_gpus": world, "steps": total, "warmup": 4, "ms_per_step": round(el / total * 1e3, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8",
            "data": "synthetic constant frames in pinned host memory",
            "config": {"workload": "3840x2160 stream, 1000 frames round-robin over ranks, pinned double-buffered "
                                   "H2D/D2H, %s (BASELINE.json configs[4])"
                                   % ("streams+events" if args.no_graph else
                                      "hipGraph-captured launch: one hipGraphLaunch per frame replays the slot's "
                                      "compute-queue segment (wait for the upload, kernel, signal the download), "
                                      "the copies stay on the copy queues")},
            "per_gpu": per_gpu, "parity": parity,
            "control_plane": dist.get_backend() if dist is not None else "single process",
            "control_plane_fallback": (dist.fallback_reason if dist is not None else None),
        # what carried the two barriers of the timed region: rccl, or -- a gloo plane on one host -- shared memory
        "barrier_transport": (dist.barrier_transport if dist is not None else None),
            "barrier_transport": (dist.barrier_transport if dist is not None else None),
            "rccl_nranks": dist.rccl_nranks if dist is not None else None, "distinct_gpus": distinct_gpus,
            "mechanisms": {"streams_and_events_3_queues": round(px / el_streams / 1e6, 1),
                           "hipgraph_captured_launch": round(px / el_graph / 1e6, 1),
                           "hipgraph_whole_chain_per_slot": round(px / el_chain / 1e6, 1)},
            "roofline": {"bound": "pcie", "achieved": round(4 * px / el / 1e9, 2), "peak": 63.0 * world,
                         "unit": "GB/s", "frac": round(4 * px / el / 1e9 / (63.0 * world), 4), "traffic": None,
                         "note": "binding direction = D2H, 4 B/pixel, against PCIe Gen5 x16 63 GB/s per GPU (spec); the "
                                 "1 B/pixel H2D runs concurrently on the other direction"}}),
              flush=True)


def run(args):
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()

    if pkg.device_count() < 1:
        raise SystemExit("bench.py: no MI355X visible; the bayer2rgb path has no CPU fallback")
    world, rank, local_rank, dist = setup_distributed(args)
    ident = gpu_identity(pkg, local_rank, rank)
    identities = dist.gather_objects(ident) if dist is not None else [ident]
    distinct_gpus, dup_error = check_distinct_gpus(identities, world, args.share_gpu)
    if dup_error:               # every rank sees the same list: all of them leave
        if dist is not None:
            dist.destroy_process_group()
        raise SystemExit(dup_error)

    variant = args.variant
    ctxs = {o: pkg.Context(WIDTH, HEIGHT, o, FORMAT, device=local_rank, variant=variant) for o in ORDERS}
    ctx0 = ctxs[ORDERS[0]]
    # one side stream for every launch of the run; the HIP events below are recorded on it
    tstream = torch.cuda.Stream()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    d_src = torch.empty(BATCH * ctx0.src_bytes, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty(BATCH * ctx0.dst_bytes, dtype=torch.uint8, device="cuda")
    # synthetic frames generated in HBM: this rank's i-th frame is global frame rank + i*world
    for i, gframe in enumerate(shard_frames(BATCH * world, world, rank)):
        ctx0.fill_synthetic(d_src.data_ptr() + i * ctx0.src_bytes, 1, SEED, first_frame=gframe,
                            stream=stream)
    torch.cuda.synchronize()
    # measured launch-plan selection (product API mibayer_autotune), once per stream context, outside
    # the timed region: MI355X boxes differ in which block->tile order streams best
    tune = {}
    if args.plan:
        # an explicit plan (the profiled twin of a bench line: tools/evidence_pass.sh pins the plan the unprofiled run
        # reported, so that the rocprofv3 --stats table's dominant kernel IS that run's kernel)
        vname, band, align = args.plan.rsplit(":", 2)
        for c in ctxs.values():
            c.set_plan(pkg.variant_names().index(vname), int(band), int(align))
        tune[ORDERS[0]] = "pinned by --plan %s" % args.plan
    elif not args.no_autotune:
        tune[ORDERS[0]] = ctx0.autotune(d_src.data_ptr(), d_dst.data_ptr(), BATCH)
        for o in ORDERS[1:]:        # same geometry, same kernel: one plan for all four orders
            ctxs[o].copy_plan_from(ctx0)

    def launch(i):
        ctxs[ORDERS[i % 4]].process_device(d_src.data_ptr(), d_dst.data_ptr(), BATCH, stream=stream)

    # Time-based pre-warm, untimed and stated in the JSON line: an MI355X that has been idle (context set-up,
    # the host side of the autotune report, rendezvous) needs tens of milliseconds of work to reach its
    # sustained clocks, and W = 5 steps are only 2 ms of it.  Launches of the very kernel of the timed region,
    # in chunks, until the wall clock says `--prewarm-ms` have passed with the GPU busy.  Nothing between
    # here and the timed region lets the GPU idle: the W warm-up steps follow back to back.
    prewarm_launches, t0 = 0, time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
        for _ in range(16):
            launch(prewarm_launches)
            prewarm_launches += 1
        tstream.synchronize()
    prewarm_ms = (time.perf_counter() - t0) * 1e3

    # HIP events on the launch stream: one before every timed step and one after the last, so the line
    # carries the per-step distribution beside the mean
    step_events = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] \
        if not args.no_step_events else None
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    first_timed = args.warmup

    def step(i):
        k = i - first_timed
        if step_events is not None and k >= 0:
            step_events[k].record()
        elif k == 0:
            ev0.record()
        launch(i)
        if k == args.steps - 1:
            (step_events[args.steps] if step_events is not None else ev1).record()

    tinfo = {}
    elapsed = timed_region(step, args.steps, args.warmup, torch.cuda.synchronize, dist, tinfo)
    if args.dump_outputs and rank == 0:
        # before anything else launches on d_dst: it holds what the last timed step wrote
        dump_outputs(args.dump_outputs, d_dst, BATCH, HEIGHT, ctx0.dst_bytes // HEIGHT)
    if step_events is not None:
        kernel_ms = step_events[0].elapsed_time(step_events[args.steps]) / args.steps
        per_step = sorted(step_events[k].elapsed_time(step_events[k + 1]) for k in range(args.steps))
    else:
        kernel_ms = ev0.elapsed_time(ev1) / args.steps       # HIP events on the launch stream
        per_step = None
    pixels = WIDTH * HEIGHT * BATCH
    value = aggregate_mpix_per_s(pixels, world, args.steps, elapsed)
    achieved = BYTES_PER_PIXEL * pixels / (kernel_ms * 1e-3) / 1e9
    # what the control plane cost: the slowest rank's kernel time alone, and the slowest closing barrier
    kernel_ms_max = dist.max_over_ranks(kernel_ms) if dist is not None else kernel_ms
    barrier_ms = dist.max_over_ranks(tinfo.get("barrier_ms", 0.0)) if dist is not None else 0.0
    # parity AFTER the timed region (host-side oracle work and 33 MB downloads would idle the GPU before it)
    parity = parity_spot_check(pkg, ctxs, d_src, d_dst, rank, world, stream) if args.full else None

    def pct(q):
        return per_step[min(len(per_step) - 1, int(q * len(per_step)))]

    result = {
        "metric": "bayer2rgb Mpix/s @4K (device-resident batch)",
        "value": round(value, 1), "unit": "Mpix/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8",
        "data": "synthetic (counter-based PRNG frames generated in HBM, seed %d)" % SEED,
        "prewarm_ms": round(prewarm_ms, 1), "prewarm_launches": prewarm_launches,
        # the control plane of the timed region, where a fallback or a slow barrier cannot hide: what carried the
        # barriers / max-reduction, the wall time of the closing barrier (slowest rank; it is inside `value`), and
        # the aggregate rate from the slowest rank's HIP-event kernel time alone (no barrier, no host)
        "control_plane": dist.get_backend() if dist is not None else "single process",
        "control_plane_fallback": (dist.fallback_reason if dist is not None else None),
        # what carried the two barriers of the timed region: rccl, or -- a gloo plane on one host -- shared memory
        "barrier_transport": (dist.barrier_transport if dist is not None else None),
        "barrier_ms": round(barrier_ms, 4),
        "value_kernel_only": round(pixels * world / (kernel_ms_max * 1e-3) / 1e6, 1),
        # hardware identity of the run: ranks RCCL itself counted (sum-of-ones all-reduce on device tensors; null
        # when the plane is not RCCL) and distinct (host, PCI bus id) pairs over the ranks -- both must equal n_gpus
        "rccl_nranks": dist.rccl_nranks if dist is not None else None,
        "distinct_gpus": distinct_gpus,
        "config": {"workload": "3840x2160 x 64 frames per GPU, bggr/rggb/grbg/gbrg -> BGRx cycled per step "
                               "(BASELINE.json configs[2]), one launch per step, frames sharded round-robin "
                               "over ranks, no collective",
                   "kernel_variant": ctx0.variant_name, "launch_plan": ctx0.launch_geometry(BATCH),
                   "plan_source": PLAN_SOURCES[ctx0.get_plan_for(BATCH)[3]],
                   "plan": "%s:%d:%d" % ((pkg.variant_names()[ctx0.get_plan_for(BATCH)[0]],)
                                         + tuple(ctx0.get_plan_for(BATCH)[1:3])),
                   "autotune": tune.get(ORDERS[0], "off"), "parity": parity,
                   "control_plane": dist.get_backend() if dist is not None else "single process"},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
                     "kernel_ms": round(kernel_ms, 4),
                     "algorithmic_bytes_per_launch": BYTES_PER_PIXEL * pixels},
    }
    if per_step is not None:
        med = pct(0.5)
        result["roofline"]["kernel_ms_per_step"] = {
            "median": round(med, 4), "p10": round(pct(0.1), 4), "p90": round(pct(0.9), 4),
            "min": round(per_step[0], 4), "max": round(per_step[-1], 4),
            "frac_at_median": round(BYTES_PER_PIXEL * pixels / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
    # `traffic` is a measurement of THIS run or null: PMC counters need a rocprofv3 wrapper around the process, so
    # the unwrapped bench line says null and carries the last profiled figure under its own name, with the
    # plan, the box and the build it was taken on (tools/summarize_profiles.py writes the file)
    # The host-path note runs BEFORE the traffic pass (round 6).  For some tens of milliseconds after a process that
    # collected PMC counters has left the GPU, whatever runs there can lose ONE interval of 18.5-19.9 ms in which the
    # device completes nothing (caught six times in profiles/r06_host_path_bimodal.md, never without the PMC child, never
    # in host scheduling: no thread of this process waited for a CPU meanwhile) -- that, inside a 15-ms arm right behind
    # the child, was the "5.7 Gpix/s" of the default host mode in two records of rounds 4-5.  --host-path-after-traffic
    # restores the old order (the reproducer).
    if args.full and rank == 0 and world == 1 and not args.no_host_path and not args.host_path_after_traffic:
        for c in ctxs.values():
            c.sync()
        result["host_path"] = host_path_note(pkg, local_rank)
    if args.full and rank == 0 and world == 1 and not args.no_traffic:
        # measured in THIS run: a profiled child of this very script, same batch, same plan, after the timed region
        torch.cuda.synchronize()
        vid, band, align = ctx0.get_plan()
        traffic, why = measure_traffic((pkg.variant_names()[vid], band, align), args.traffic_launches,
                                       args.traffic_seconds)
        result["roofline"]["traffic"] = traffic
        if traffic is None:
            result["roofline"]["traffic_note"] = why
    if result["roofline"]["traffic"] is None:
        # ONE traffic figure per record: only when nothing was measured in this run does the last
        # committed figure travel, under its own name, with the box and the build it was taken on
        result["roofline"]["traffic_profiled"] = profiled_traffic(ctx0.launch_geometry(BATCH)["band"],
                                                                  ctx0.variant_name)
    if dist is not None:
        # per-GPU breakdown (SURVEY.md section 5 "metrics"): `roofline` above is rank 0's kernel, this is every rank's
        mine = dict(ident, kernel_ms=round(kernel_ms, 4), frac=round(achieved / HBM_PEAK_GBPS, 4),
                    kernel_variant=ctx0.variant_name, band=ctx0.launch_geometry(BATCH)["band"],
                    plan_source=PLAN_SOURCES[ctx0.get_plan_for(BATCH)[3]], parity=parity)
        result["per_gpu"] = dist.gather_objects(mine)
    if args.full and rank == 0 and world == 1:
        if not args.no_host_path and args.host_path_after_traffic:
            for c in ctxs.values():
                c.sync()
            result["host_path"] = host_path_note(pkg, local_rank)
        if not args.no_cpu:
            result["cpu_baseline"] = cpu_baseline(args.cpu_seconds)
    for c in ctxs.values():
        c.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--variant", type=int, default=int(os.environ.get("MIBAYER_VARIANT", "0")))
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run the parity spot check, the host-path note, the in-run PMC "
                         "traffic pass and the CPU baseline (each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed as float32 .npy files into DIR")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-host-path", action="store_true")
    ap.add_argument("--host-path-after-traffic", action="store_true",
                    help="reproducer: run the host-path note behind the PMC child, as rounds 1-5 did")
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--plan", default=None, metavar="VARIANT:BAND:ALIGN",
                    help="pin the launch plan (as config.plan of an earlier line reports it) instead of measuring it")
    ap.add_argument("--prewarm-ms", type=float, default=150.0,
                    help="untimed time-based GPU pre-warm before the W warm-up steps (reported as prewarm_ms)")
    ap.add_argument("--no-step-events", action="store_true",
                    help="two HIP events around the timed region instead of one per step")
    ap.add_argument("--no-traffic", action="store_true",
                    help="skip the rocprofv3 PMC pass that fills roofline.traffic (N == 1 only)")
    ap.add_argument("--traffic-launches", type=int, default=8)
    ap.add_argument("--traffic-seconds", type=float, default=120.0, help="budget of the whole traffic pass")
    ap.add_argument("--traffic-pass", default=None, metavar="VARIANT:BAND:ALIGN",
                    help="internal: the profiled child of the traffic pass")
    ap.add_argument("--force-dist", action="store_true",
                    help="N == 1: bring the process groups up exactly as at N > 1 (gloo bootstrap + RCCL group of "
                         "one rank) and run the barriers / max-reduction of the timed region over them")
    ap.add_argument("--mode", choices=("batch", "stream"), default="batch",
                    help="batch = the headline device-resident metric (default); stream = configs[4] host-fed stream")
    ap.add_argument("--no-graph", action="store_true", help="stream mode: streams+events instead of hipGraph")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl",
                    help="torch.distributed backend for the barrier / max-reduce (nccl = RCCL)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="testing only: ranks share the visible GPUs (use with --backend gloo on a 1-GPU box)")
    args = ap.parse_args()
    if args.dump_outputs and args.mode != "batch":
        ap.error("--dump-outputs dumps the batch of the device-resident mode (--mode batch)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # convenience: self-launch one rank per GPU the way the driver does
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", os.environ.get("MASTER_PORT", "29533"), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    if args.traffic_pass:
        traffic_child(args)
    elif args.mode == "stream":
        run_stream(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
