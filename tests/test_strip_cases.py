"""The case tables of tests/strip_cases.py reach what they are meant to reach -- asserted from the tables and the NumPy
models alone, so that the GPU tests built on them (tests/test_gpu_strip_geometry.py) cannot go vacuous when a table is
edited."""
import numpy as np
import pytest

import colour_model as cm
import mhc_model as mm
import strip_cases as sc


# -- the tables ----------------------------------------------------------------------------------------------------

def test_arms_are_the_seven_kernels_and_the_eight_colour_arms():
    plain = {sc.strip_index(a) for a in sc.PLAIN_ARMS}
    every = {(m, i, o) for m in (False, True) for i in (False, True) for o in (False, True)}
    assert len(sc.PLAIN_ARMS) == 7 and plain == every - {(False, True, False)}      # the null entry of kStripKernels
    assert not any(a.colour for a in sc.PLAIN_ARMS)
    assert len(sc.COLOUR_ARMS) == 8 and {sc.strip_index(a) for a in sc.COLOUR_ARMS} == every
    assert all(a.colour for a in sc.COLOUR_ARMS)
    assert len({a.name for a in sc.ARMS}) == 15
    assert all(a.bits in (0, 10, 12, 14, 16) for a in sc.ARMS)


def test_widths_cover_every_residue_and_both_seams():
    assert all(w % 2 == 0 and w >= 4 for w in sc.WIDTHS)
    assert {w % 16 for w in sc.WIDTHS} == set(range(0, 16, 2))
    # ... all of them inside one wave too, where no seam is involved
    assert {w % 16 for w in sc.WIDTHS if w <= 4 * sc.STRIP_GROUPS - 8} == set(range(0, 16, 2))
    ends = {(g["lane"], g["full"]) for g in map(sc.last_group, sc.WIDTHS) if g["lane"] == 63}
    ends |= {(g["lane"], g["full"]) for g in map(sc.last_group, sc.WIDTHS) if g["wave"] >= 1}
    for lane in (63, 0, 1, 2, 3):
        assert (lane, True) in ends and (lane, False) in ends, lane
    # residues 10 and 12 (the tail and a full last group in lane & 3 == 2) behind the first and the second seam
    for wave in (1, 2):
        behind = {w % 16 for w in sc.WIDTHS if sc.last_group(w)["wave"] == wave}
        assert {10, 12} <= behind, wave
    assert {w % 16 for w in sc.SWEEP_WIDTHS} == {10, 12}
    assert all(sc.last_group(w)["wave"] == 1 for w in sc.SWEEP_WIDTHS)
    assert {w % 16 for w in sc.ALIGN_WIDTHS} == set(range(0, 16, 2)) and set(sc.ALIGN_WIDTHS) <= set(sc.WIDTHS)


def test_heights_cover_the_chunk_edges():
    assert all(h >= 3 for h in sc.HEIGHTS)
    for chunks in (1, 2):       # one short of `chunks` chunks, exactly, one and two rows over
        for r in (-1, 0, 1, 2):
            assert chunks * sc.STRIP_ROWS + r in sc.HEIGHTS, (chunks, r)
    assert {h % sc.STRIP_ROWS for h in sc.HEIGHTS} >= {15, 0, 1, 2}
    assert {h % 2 for h in sc.HEIGHTS} == {0, 1}
    assert sc.SWEEP_HEIGHT in sc.HEIGHTS and sc.SWEEP_HEIGHT > sc.STRIP_ROWS


@pytest.mark.parametrize("arm", sc.ARMS, ids=lambda a: a.name)
def test_every_arm_sees_every_order_layout_and_byte_order(arm):
    cases = sc.geometry_cases(arm)
    assert {c.w for c in cases if c.h == sc.SWEEP_HEIGHT} >= set(sc.WIDTHS)
    for w in sc.SWEEP_WIDTHS:
        assert {c.h for c in cases if c.w == w} >= set(sc.HEIGHTS)
    assert {c.order for c in cases} == set(sc.ORDERS)
    assert {c.layout for c in cases} == set(sc.LAYOUT16 if arm.out16 else sc.LAYOUT8)
    assert {c.sbe for c in cases} == ({False, True} if arm.bits else {False})
    assert {c.dbe for c in cases} == ({False, True} if arm.out16 else {False})
    # the residues 10 and 12 meet more than one order and layout
    for r in (10, 12):
        assert len({c.order for c in cases if c.w % 16 == r}) >= 2 and len({c.layout for c in cases if c.w % 16 == r}) >= 2
    align = sc.alignment_cases(arm)
    assert {c.w % 16 for c in align} == set(range(0, 16, 2))
    assert len({c.order for c in align}) == 4 and len({c.layout for c in align}) >= 2


# -- section B: the value extremes ---------------------------------------------------------------------------------

def test_extreme_cases_cover_the_arms_and_depths():
    cases = sc.extreme_cases()
    plain = [a for a in cases if not a.colour]
    assert {sc.strip_index(a) for a in plain} == {sc.strip_index(a) for a in sc.PLAIN_ARMS}
    assert {sc.depth_of(a.bits) for a in plain} == {8, 10, 16}
    for index in {sc.strip_index(a) for a in sc.PLAIN_ARMS if a.bits}:      # every 16-bit-word kernel at 10 and at 16
        assert {a.bits for a in plain if sc.strip_index(a) == index} == {10, 16}
    colour = [a for a in cases if a.colour]
    assert {sc.strip_index(a) for a in colour} == {sc.strip_index(a) for a in sc.COLOUR_ARMS}
    assert {sc.depth_of(a.bits) for a in colour} == {8, 10, 16}
    assert len({a.name for a in cases}) == len(cases)


def test_frame_builders():
    w, h = sc.PLANE_SIZE
    planes = sc.plane_frames(w, h, 10)
    assert len(planes) == sc.MAX_LIST == 16
    corners = {tuple(int(v) for v in (p[0, 0], p[0, 1], p[1, 0], p[1, 1])) for p in planes}
    assert len(corners) == 16 and all(set(c) <= {0, 1023} for c in corners)
    for p in planes:
        assert np.array_equal(p, np.tile(p[:2, :2], (h // 2, w // 2)))
    w, h = sc.PATTERN_SIZE
    pats = sc.pattern_frames(w, h, 16)
    assert len(pats) == 9 and not pats[0].any() and (pats[1] == 65535).all()
    assert pats[2][0, :4].tolist() == [0, 65535, 0, 65535] and pats[3][0, :4].tolist() == [0, 0, 65535, 65535]
    assert pats[4][:4, 0].tolist() == [0, 65535, 0, 65535] and pats[5][:4, 0].tolist() == [0, 0, 65535, 65535]
    assert pats[6].sum() == 65535 == pats[6][0, 0] and pats[7].sum() == 65535 == pats[7][h - 1, w - 1]
    assert pats[8].sum() == 18 * 65535 and pats[8][5, 6] == pats[8][11, 21] == 65535 and (5 + 6 + 11 + 21) % 2 == 1
    # deep frames carry junk above the depth, and the models do not see it
    rng = np.random.default_rng(1)
    buf = sc.frame_bytes(planes[5], 10, rng)
    words = buf.view("<u2")
    assert (words >> 10).any() and np.array_equal(words & 1023, planes[5])
    buf8 = sc.frame_bytes(sc.plane_frames(22, 4, 8)[9], 0, rng)
    assert buf8.shape == (4, 24) and (buf8[:, 22:] == 0x5A).all()


@pytest.mark.parametrize("depth", [8, 16])
def test_plane_frames_recorded_clamp_counts(depth):
    """the 16 plane frames at 26 x 18: 9360 of the 22464 MHC outputs are 0 and 9360 are vmax"""
    vmax = (1 << depth) - 1
    out = np.stack([mm.native_rgb(S, "rggb", depth) for S in sc.plane_frames(26, 18, depth)])
    assert out.size == 22464
    assert int((out == 0).sum()) == 9360 and int((out == vmax).sum()) == 9360


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("method", ["bilinear", "mhc"])
def test_extreme_frames_reach_both_ends(method, depth):
    vmax = (1 << depth) - 1
    arm = sc.Arm("x", method, 0 if depth == 8 else depth, True, False)
    sets = (sc.plane_frames(*sc.PLANE_SIZE, depth), sc.pattern_frames(*sc.PATTERN_SIZE, depth))
    for frames in sets:
        out = np.stack([sc.native_rgb(arm, S, "grbg") for S in frames])
        assert (out == 0).any() and (out == vmax).any()
        if method == "bilinear":
            # the packed average with one half at its maximum next to a half at 0, both ways round
            flat = np.concatenate([S.reshape(-1) for S in frames])
            pairs = set(zip(flat[:-1:2].tolist(), flat[1::2].tolist()))
            assert {(0, vmax), (vmax, 0), (vmax, vmax), (0, 0)} <= pairs
    if method == "mhc":
        # every MHC filter leaves the range on both sides before the clamp.  Constant planes cannot do that to F_G and
        # F_diag (there they reduce to 8 (b + c) and 16 d): the pattern frames do, the 3x3 blocks on the upper side
        for k in (mm.F_G, mm.F_ROW, mm.F_COL, mm.F_DIAG):
            raw = [(mm.correlate(S, k) + 8) >> 4 for S in sets[1]]
            assert min(r.min() for r in raw) < 0 and max(r.max() for r in raw) > vmax
        for k in (mm.F_ROW, mm.F_COL):
            raw = [(mm.correlate(S, k) + 8) >> 4 for S in sets[0]]
            assert min(r.min() for r in raw) < 0 and max(r.max() for r in raw) > vmax
    # ... and at every kind of site of the mosaic: the plane frames drive each 2x2 position to both clamps
    if method == "mhc":
        w, h = sc.PLANE_SIZE
        out = np.stack([mm.native_rgb(S, "grbg", depth) for S in sc.plane_frames(w, h, depth)])
        for ys in (0, 1):
            for xs in (0, 1):
                for ch in range(3):
                    sub = out[:, 2 + ys:h - 2:2, 2 + xs:w - 2:2, ch]
                    assert (sub == 0).any() and (sub == vmax).any(), (ys, xs, ch)


# -- section C: the colour stage at the ends of its ranges -----------------------------------------------------------

def stage_internals(rgb, depth, stage):
    """the header's formula once more, keeping what cm.stage drops: the matrix sums, the curve's index and fraction,
    the interpolation before its cap"""
    c = np.maximum(rgb.astype(np.int64) - np.asarray(stage.black, np.int64), 0)
    acc = (c[..., None, :] * np.asarray(stage.matrix, np.int64).reshape(3, 3)).sum(axis=-1)
    c2 = np.clip((acc + 2048) >> 12, 0, (1 << depth) - 1)
    t = c2 << (16 - depth)
    out = {"c": c, "acc": acc, "i": t >> 8, "f": t & 255}
    if stage.tone is not None:
        tone = np.asarray(stage.tone, np.int64)
        out["o"] = (tone[t >> 8] * (256 - (t & 255)) + tone[(t >> 8) + 1] * (t & 255) + 128) >> 8
    return out


def stage_inputs(method, bits):
    rng = np.random.default_rng(1000 + bits)
    arm = sc.Arm("x", method, bits, True, True)
    return [sc.native_rgb(arm, S, "gbrg") for S in sc.stage_frames(rng, bits)]


@pytest.mark.parametrize("bits", [b for b, _, _ in sc.STAGE_IO])
@pytest.mark.parametrize("method", ["bilinear", "mhc"])
def test_colour_stages_reach_their_edges(method, bits):
    depth = sc.depth_of(bits)
    vmax = (1 << depth) - 1
    random_rgb, max_rgb = stage_inputs(method, bits)
    assert (max_rgb == vmax).all()
    stages = {s.name: s for s in sc.colour_stages(depth)}
    assert len(stages) == (8 if depth == 16 else 9)
    for s in stages.values():   # every one is inside the ranges mibayer_set_colour accepts
        assert all(0 <= b <= 65535 for b in s.black) and all(-65535 <= m <= 65535 for m in s.matrix)
        assert s.tone is None or (len(s.tone) == 257 and all(0 <= v <= 65536 for v in s.tone))
    # +-65535: a sum below 0 and one above vmax both occur, and both clamps take a good part of a random frame
    x = stage_internals(random_rgb, depth, stages["pm65535"])
    assert x["acc"].min() < 0 and ((x["acc"] + 2048) >> 12).max() > vmax
    got = cm.stage(random_rgb, depth, stages["pm65535"].black, stages["pm65535"].matrix, None, True)
    assert (got == 0).mean() > 0.25 and (got == vmax << (16 - depth)).mean() > 0.25
    if depth == 16:
        assert 0.30 < (got == 0).mean() < 0.37 and 0.55 < (got == 65535).mean() < 0.70
        # the sum that passes 2^32, with a low part (m & 4095) that carries into the high one
        x = stage_internals(max_rgb, depth, stages["gain16"])
        assert x["acc"].max() == 65535 * 65538 > 1 << 32
        assert all(m & 4095 for m in sc.MATRIX_GAIN16[:2]) and all(m & 1 for m in sc.MATRIX_PM65535[:3])
    # a black level at and above the range leaves nothing
    for name in ("black_vmax", "black_vmax_plus_1"):
        if name in stages:
            assert not stage_internals(random_rgb, depth, stages[name])["c"].any()
            assert not stage_internals(max_rgb, depth, stages[name])["c"].any()
    assert ("black_vmax_plus_1" in stages) == (depth < 16)
    # the curves: the 65535 cap is hit, the last segment is used (with a fraction where the depth has one), the table
    # entry 65536 is read, and a curve that falls is followed down
    for name in ("tone_flat_top", "tone_step", "tone_non_monotonic"):
        x = stage_internals(np.concatenate([random_rgb, max_rgb]), depth, stages[name])
        assert (x["i"] == 255).any()
        if depth > 8:
            assert ((x["i"] == 255) & (x["f"] > 0)).any(), name
        if name != "tone_non_monotonic":
            assert x["o"].max() == 65536, name          # above the cap before it is applied
    tone = np.asarray(sc.TONE_NON_MONOTONIC)
    assert (np.diff(tone) < 0).any() and tone[256] == 65536 and tone.max() <= 65536
    assert sc.TONE_STEP[127] == 0 and sc.TONE_STEP[128] == 65536
    assert set(sc.TONE_FLAT_TOP[200:]) == {65536} and sc.TONE_FLAT_TOP[199] < 65536
    x = stage_internals(random_rgb, depth, stages["tone_step"])
    if depth > 8:
        assert ((x["i"] == 127) & (x["f"] > 0)).any()   # inside the step itself
    # junk in the table of a stage without a curve: out of the table's range, so a kernel that looked would show it
    junk = stages["no_tone_junk_table"]
    assert junk.tone is None and max(junk.junk) > 65536 and len(junk.junk) == 257
    # the model's own output for every stage: defined, in range
    for s in stages.values():
        for out16 in (False, True):
            got = cm.stage(random_rgb, depth, s.black, s.matrix, s.tone, out16)
            assert got.min() >= 0 and got.max() <= (65535 if out16 else 255), s.name


def test_linear_tone_is_the_librarys_definition():
    assert sc.LINEAR_TONE[0] == 0 and sc.LINEAR_TONE[256] == 65536 and len(sc.LINEAR_TONE) == 257
    rgb = np.arange(3 * 1024).reshape(1, 1024, 3) % 1024
    for out16 in (False, True):
        assert np.array_equal(cm.stage(rgb, 10, tone=sc.LINEAR_TONE, out16=out16), cm.stage(rgb, 10, out16=out16))
