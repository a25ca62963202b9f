"""GPU tests of the inverse direction's geometry (rgb2bayer_flat_kernel, rgb2bayer_kernel; launch_flat,
launch_rgb2bayer, launch_rgb2bayer_list and the c->inverse arm of launch_frames): every item seam, list launches, frame
pitches, base pointers off the 16-byte grid, all 24 selectors, the launch shapes of the lab build and the banded host
path -- byte for byte against the NumPy restatement of the reference loop (oracle/bayer2rgb_np.rgb2bayer), with the
destination inside a prefilled allocation so that every byte a launch must not write is looked at.  The tables are
tests/r2b_cases.py; tests/test_r2b_cases.py shows without a GPU what they reach.

Every device case asserts four things: (a) columns [0, w) equal the model; (b) columns [w, ROUND_UP_4 (w)) are zero;
(c) columns [ROUND_UP_4 (w), dst_stride), the gaps between frames and both guards keep the fill; (d) nothing else -- the
whole allocation is compared with what it must hold.

What the tables are, where one might expect otherwise.  With two items per group (PX = 8) every item count is even,
so the seam tables of those shapes sit one GROUP (two items) under and over a block, not one item.  The banded host
path runs each of its four launch shapes under both band counts: eight contexts of 17 MB.  The tile kernel runs the
flat kernel's whole width sweep (27 widths x 3 heights, rows of one, two and three tiles) under each of the four block
orders, with default strides, and its row-seam cases with default pitches.  Whether a launch takes the VEC = 16 or the
VEC = 4 arm cannot be seen in bytes when width % 4 == 0 (both issue the same 16-byte loads): the pitch and pointer
cases run both arms, but the rule that chooses between them is restated in tests/r2b_cases.py only.

Every test counts the contexts it opens and asserts the number, so that a table that shrinks is noticed here too."""
import numpy as np
import pytest

import r2b_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0x3C
SLACK = 64                      # bytes behind the last source frame, inside its allocation
COUNT = {"contexts": 0, "launches": 0}
NAMES = ("the fill (row padding, gap or guard) was written", "pixels differ", "padding columns are not zero")


def reset_count():
    COUNT["contexts"] = COUNT["launches"] = 0


def counted(contexts):
    """the running test opened as many contexts as its tables have cases (printed with -s)"""
    print("contexts opened: %(contexts)d, conversions started: %(launches)d" % COUNT)
    assert COUNT["contexts"] == contexts, (COUNT, contexts)


def open_ctx(pkg, g, order, triple, **kw):
    COUNT["contexts"] += 1
    ctx = pkg.Context(g.w, g.h, order, triple, src_stride=g.src_stride, dst_stride=g.dst_stride,
                      flags=pkg.FLAG_RGB2BAYER, **kw)
    r = rc.resolved(g)
    assert (ctx.src_stride, ctx.dst_stride) == (r.src_stride, r.dst_stride)
    return ctx


def must_hold(total, starts, wants, w, h, dst_stride):
    """what an allocation of `total` bytes of fill holds once the frames at `starts` have been converted, and which of
    (c), (a), (b) every byte belongs to"""
    exp = np.full(total, FILL, np.uint8)
    kind = np.zeros(total, np.uint8)
    block = np.full((h, dst_stride), FILL, np.uint8)
    kinds = np.zeros((h, dst_stride), np.uint8)
    kinds[:, :w] = 1
    kinds[:, w:rc.round_up_4(w)] = 2
    for lo, want in zip(starts, wants):
        block[:, :rc.round_up_4(w)] = 0
        block[:, :w] = want
        exp[lo:lo + block.size] = block.reshape(-1)
        kind[lo:lo + block.size] = kinds.reshape(-1)
    return exp, kind


def differences(out, exp, kind, lo):
    bad = np.flatnonzero(out != exp)
    parts = []
    for k, name in enumerate(NAMES):
        b = bad[kind[bad] == k]
        if len(b):
            parts.append("%s: %d bytes, first at byte %d of the destination (got %d, want %d)" % (
                name, len(b), b[0] - lo, out[b[0]], exp[b[0]]))
    return "; ".join(parts)


def convert_batch(ctx, g, frames, wants):
    """one mibayer_process_device launch over the frames of g: the destination lies GUARD bytes inside a prefilled
    allocation, the source allocation has SLACK behind the last frame and junk between the frames, the base pointers
    sit g.src_off / g.dst_off bytes off the allocations' alignment.  Returns what is wrong ("" = nothing)"""
    r = rc.resolved(g)
    src = np.random.default_rng(7).integers(0, 256, (r.n, r.src_pitch), np.uint8)
    for f, frame in enumerate(frames):
        src[f, :ctx.src_bytes] = frame.reshape(-1)
    lo = GUARD + r.dst_off
    total = lo + r.n * r.dst_pitch + GUARD
    d_src = ctx.device_alloc(r.src_off + src.size + SLACK)
    d_dst = ctx.device_alloc(total)
    try:
        ctx.to_device(d_src + r.src_off, src)
        ctx.to_device(d_dst, np.full(total, FILL, np.uint8))
        COUNT["launches"] += 1
        ctx.process_device(d_src + r.src_off, d_dst + lo, r.n, r.src_pitch, r.dst_pitch)
        ctx.sync()
        out = ctx.from_device(d_dst, total)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    exp, kind = must_hold(total, [lo + f * r.dst_pitch for f in range(r.n)], wants, r.w, r.h, r.dst_stride)
    return differences(out, exp, kind, lo)


def convert_list(ctx, g, frames, wants, src_offs=None, dst_offs=None):
    """one mibayer_process_device_list call over separately allocated frames, every destination guarded on its own;
    frame k's pointers sit src_offs[k] / dst_offs[k] bytes off the grid.  Each output is compared with its own
    frame's model"""
    n = len(frames)
    src_offs = src_offs or [0] * n
    dst_offs = dst_offs or [0] * n
    total = GUARD + 16 + ctx.dst_bytes + GUARD
    srcs = [ctx.device_alloc(16 + ctx.src_bytes + SLACK) for _ in range(n)]
    dsts = [ctx.device_alloc(total) for _ in range(n)]
    fill = np.full(total, FILL, np.uint8)
    try:
        for k in range(n):
            ctx.to_device(srcs[k] + src_offs[k], frames[k])
            ctx.to_device(dsts[k], fill)
        COUNT["launches"] += 1
        ctx.process_device_list([s + o for s, o in zip(srcs, src_offs)], [d + GUARD + o for d, o in zip(dsts, dst_offs)])
        ctx.sync()
        outs = [ctx.from_device(d, total) for d in dsts]
    finally:
        for d in srcs + dsts:
            ctx.device_free(d)
    wrong = []
    for k in range(n):
        lo = GUARD + dst_offs[k]
        exp, kind = must_hold(total, [lo], [wants[k]], g.w, g.h, ctx.dst_stride)
        msg = differences(outs[k], exp, kind, lo)
        if msg:
            wrong.append("list frame %d of %d: %s" % (k, n, msg))
    return "; ".join(wrong[:3])


def convert_reversed_batch_as_list(ctx, g, frames, wants):
    """the frames of one batch handed over as a list in reverse order: a wrong table index gives wrong bytes"""
    n = len(frames)
    total = GUARD + n * ctx.dst_bytes + GUARD
    d_src = ctx.device_alloc(n * ctx.src_bytes + SLACK)
    d_dst = ctx.device_alloc(total)
    try:
        ctx.to_device(d_src, np.stack([f.reshape(-1) for f in frames]))
        ctx.to_device(d_dst, np.full(total, FILL, np.uint8))
        COUNT["launches"] += 1
        ctx.process_device_list([d_src + k * ctx.src_bytes for k in reversed(range(n))],
                                [d_dst + GUARD + k * ctx.dst_bytes for k in reversed(range(n))])
        ctx.sync()
        out = ctx.from_device(d_dst, total)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    exp, kind = must_hold(total, [GUARD + k * ctx.dst_bytes for k in range(n)], wants, g.w, g.h, ctx.dst_stride)
    return differences(out, exp, kind, GUARD)


def run_batches(pkg, cases, key, bad, tag=""):
    """every case through one launch of its own, orders and offset triples going round with the case index"""
    for i, g in enumerate(cases):
        order, triple = rc.rotate(i + key)
        frames = rc.frames((key, i), g)
        wants = [rc.expect(f, g.w, order, triple) for f in frames]
        with open_ctx(pkg, g, order, triple) as ctx:
            msg = convert_batch(ctx, g, frames, wants)
        if msg:
            bad.append((tag, tuple(g), "w %% 4 = %d" % (g.w % 4), order, triple, msg))


def run_lists(pkg, g, key, bad, sizes=rc.LIST_SIZES, off_grid=True, all_dst_off=0, tag=""):
    """the list launches of one frame geometry through one context: the sizes; one source, then one destination, at
    + 4 in the first and in the second chunk; a batch in reverse order.  all_dst_off: every destination that far off"""
    n_max = max(sizes + (33,))
    order, triple = rc.rotate(key)
    frames = rc.frames((key, 1000), g._replace(n=n_max))
    wants = [rc.expect(f, g.w, order, triple) for f in frames]
    with open_ctx(pkg, g, order, triple) as ctx:
        for n in sizes:
            msg = convert_list(ctx, g, frames[:n], wants[:n], dst_offs=[all_dst_off] * n)
            if msg:
                bad.append((tag, "list of %d" % n, tuple(g), order, triple, msg))
        if off_grid:
            for k in rc.LIST_OFFSET_FRAMES:
                offs = [4 * (f == k) for f in range(33)]
                for which, kw in (("source", dict(src_offs=offs, dst_offs=[all_dst_off] * 33)),
                                  ("destination", dict(dst_offs=[(all_dst_off + o) % 8 for o in offs]))):
                    msg = convert_list(ctx, g, frames[:33], wants[:33], **kw)
                    if msg:
                        bad.append((tag, "list of 33, %s %d at + 4" % (which, k), tuple(g), order, triple, msg))
            msg = convert_reversed_batch_as_list(ctx, g, frames[:33], wants[:33])
            if msg:
                bad.append((tag, "batch of 33 as a reversed list", tuple(g), order, triple, msg))


# -- A. width x height ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strides", ["padded", "default"])
def test_every_width_residue_at_heights_1_2_3(gpu_pkg, strides):
    reset_count()
    cases = rc.sweep_cases()
    assert [g.w for g in cases[::3]] == list(rc.WIDTHS)
    if strides == "padded":
        cases = [rc.padded(g) for g in cases]
    bad = []
    run_batches(gpu_pkg, cases, 1 if strides == "padded" else 2, bad, strides)
    counted(3 * len(rc.WIDTHS))
    assert not bad, bad


# -- B. item seams ----------------------------------------------------------------------------------------------------

def test_item_seams_of_the_production_shape(gpu_pkg):
    reset_count()
    bad = []
    run_batches(gpu_pkg, rc.seam_cases(rc.PRODUCTION), 3, bad, "seam")
    run_batches(gpu_pkg, list(rc.ODD_BATCHES), 4, bad, "odd heights")
    counted(6 + len(rc.ODD_BATCHES))
    assert not bad, bad


# -- C. frame pitches -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 1])
def test_frame_pitches(gpu_pkg, n):
    reset_count()
    bad = []
    run_batches(gpu_pkg, rc.pitch_cases(n), 5 + n, bad, "pitch")
    counted(2 * len(rc.SRC_PITCH_EXTRA) * len(rc.DST_PITCH_EXTRA))
    assert not bad, bad


# -- D. base pointers -------------------------------------------------------------------------------------------------

def test_base_pointers_off_the_16_byte_grid(gpu_pkg):
    reset_count()
    bad = []
    cases = [g._replace(src_off=s, dst_off=d) for g in rc.ALIGN_FRAMES for s, d in rc.ALIGN_OFFSETS]
    run_batches(gpu_pkg, cases, 9, bad, "alignment")
    run_batches(gpu_pkg, [g for g, _ in rc.VEC16_CASES.values()], 10, bad, "vec16 predicates")
    counted(2 * len(rc.ALIGN_OFFSETS) + len(rc.VEC16_CASES))
    assert not bad, bad


# -- E. lists -----------------------------------------------------------------------------------------------------------

def test_list_launches(gpu_pkg):
    reset_count()
    bad = []
    run_lists(gpu_pkg, rc.list_frame(rc.PRODUCTION), 11, bad, off_grid=False, tag="partial items")
    run_lists(gpu_pkg, rc.geometry(rc.LIST_ALIGNED_WIDTH, 3), 12, bad, tag="w % 4 == 0")
    counted(2)
    assert not bad, bad


# -- F. selectors -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", rc.SELECTOR_SIZES, ids=["6x3", "1x1"])
def test_every_offset_triple_and_order(gpu_pkg, g):
    reset_count()
    bad = []
    frame = rc.frames((13,), g)[0]
    for order in rc.ORDERS:
        for triple in rc.TRIPLES:
            want = rc.expect(frame, g.w, order, triple)
            with open_ctx(gpu_pkg, g, order, triple) as ctx:
                msg = convert_batch(ctx, g, [frame], [want])
                COUNT["launches"] += 1
                host = ctx.process_host(frame)
            if msg:
                bad.append(("device", order, triple, msg))
            if not (np.array_equal(host[:, :g.w], want) and (host[:, g.w:] == 0).all()):
                bad.append(("host", order, triple, host.tolist(), want.tolist()))
    counted(len(rc.ORDERS) * len(rc.TRIPLES))
    assert not bad, bad


# -- G. the launch shapes of the lab build --------------------------------------------------------------------------------

def lab_knobs(monkeypatch, shape=None, rows=None, band=None, host_bands=None):
    """the launch shape of the contexts opened from now on (MIBAYER_R2B_*, read when a context is made)"""
    if shape is not None:
        monkeypatch.setenv("MIBAYER_R2B_FLAT", str(shape.K))
        monkeypatch.setenv("MIBAYER_R2B_PX", str(shape.PX))
        monkeypatch.setenv("MIBAYER_R2B_LDNT", str(shape.LD))
    else:
        monkeypatch.setenv("MIBAYER_R2B_FLAT", "0")
        monkeypatch.setenv("MIBAYER_R2B_ROWS", str(rows))
    for name, v in (("MIBAYER_XCD_BAND", band), ("MIBAYER_HOST_BANDS", host_bands)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


@pytest.mark.parametrize("shape", rc.LAB_SHAPES, ids=rc.shape_id)
def test_lab_flat_shapes_seams_and_lists(gpu_lab_pkg, shape, monkeypatch):
    reset_count()
    lab_knobs(monkeypatch, shape)
    key = 20 + rc.LAB_SHAPES.index(shape)
    bad = []
    run_batches(gpu_lab_pkg, rc.seam_cases(shape), key, bad, "seam")
    run_batches(gpu_lab_pkg, list(rc.ODD_BATCHES), key + 40, bad, "odd heights")
    run_lists(gpu_lab_pkg, rc.list_frame(shape), key + 80, bad, tag="list")
    if shape.PX == 8:
        run_batches(gpu_lab_pkg, list(rc.PX8_CASES.values()), key + 120, bad, "two items per group and its fall-backs")
        run_lists(gpu_lab_pkg, rc.list_frame(shape), key + 160, bad, all_dst_off=4, tag="list, destinations at 4 mod 8")
    counted(6 + len(rc.ODD_BATCHES) + 1 + (len(rc.PX8_CASES) + 1 if shape.PX == 8 else 0))
    assert not bad, bad


@pytest.mark.parametrize("R", rc.TILE_ROWS)
def test_lab_tile_kernel(gpu_lab_pkg, R, monkeypatch):
    reset_count()
    bad = []
    for band in rc.TILE_BANDS:
        lab_knobs(monkeypatch, rows=R, band=band)
        run_batches(gpu_lab_pkg, rc.sweep_cases() + rc.tile_cases(R), 200 + R, bad, "band %d" % band)
    # a list has no frame table in this kernel: 17 frames go frame by frame, to the same bytes
    lab_knobs(monkeypatch, rows=R)
    run_lists(gpu_lab_pkg, rc.geometry(1026, 3), 300 + R, bad, sizes=(17,), off_grid=False, tag="list")
    counted(len(rc.TILE_BANDS) * (3 * len(rc.WIDTHS) + len(rc.tile_cases(R))) + 1)
    assert not bad, bad


# -- H. the banded host path ----------------------------------------------------------------------------------------------

BANDED = {"tile_rows_2": (None, 2, rc.BANDED_FRAME), "tile_rows_16": (None, 16, rc.BANDED_FRAME),
          "flat_K2_PX4": (rc.Shape(2, 4, 1), None, rc.BANDED_FRAME),
          "flat_K1_PX8": (rc.Shape(1, 8, 1), None, rc.BANDED_FRAME_PX8)}
_banded_frames = {}


def banded_frame(g):
    if g.w not in _banded_frames:
        _banded_frames[g.w] = rc.frames((14,), g)[0]
    return _banded_frames[g.w]


@pytest.mark.parametrize("host_bands", rc.HOST_BANDS)
@pytest.mark.parametrize("name", list(BANDED))
def test_lab_banded_host_path(gpu_lab_pkg, name, host_bands, monkeypatch):
    reset_count()
    shape, rows, g = BANDED[name]
    lab_knobs(monkeypatch, shape, rows, host_bands=host_bands)
    assert rc.host_bands(host_bands, rc.resolved(g).src_pitch, g.h) == host_bands
    order, triple = rc.rotate(list(BANDED).index(name) + 7 * host_bands)
    src = banded_frame(g)
    want = rc.expect(src, g.w, order, triple)
    stride = rc.round_up_4(g.w)
    with open_ctx(gpu_lab_pkg, g, order, triple, inflight=2) as ctx:
        for _ in range(2):
            COUNT["launches"] += 1
            got = ctx.process_host(src)
            assert np.array_equal(got[:, :g.w], want), (name, host_bands, order, triple)
        outs = [np.full((g.h, stride), FILL, np.uint8) for _ in range(2)]
        for i, o in enumerate(outs):
            COUNT["launches"] += 1
            ctx.submit(src, o, tag=i + 1)
        assert [ctx.wait(), ctx.wait()] == [1, 2]
        for o in outs:
            assert np.array_equal(o[:, :g.w], want), (name, host_bands, order, triple, "queued")
    counted(1)
