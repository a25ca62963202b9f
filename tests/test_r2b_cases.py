"""The case tables of tests/r2b_cases.py reach what they are meant to reach -- asserted from the tables, the mirror of
the launch decisions and the NumPy restatement alone, so that the GPU tests built on them
(tests/test_gpu_r2b_geometry.py) cannot go vacuous when a table is edited."""
import numpy as np
import pytest

import r2b_cases as rc

ALL_SHAPES = (rc.PRODUCTION,) + rc.LAB_SHAPES


def test_constants_and_shapes():
    assert rc.PRODUCTION in rc.LAB_SHAPES and len(rc.LAB_SHAPES) == 20 == len(set(rc.LAB_SHAPES))
    assert {s.K for s in rc.LAB_SHAPES} == {1, 2, 3, 4, 8} and {s.PX for s in rc.LAB_SHAPES} == {4, 8}
    assert rc.launch(rc.PRODUCTION, rc.geometry(4, 1)).per_block == 512 == 8 * rc.WAVE_ITEMS
    assert len(rc.TRIPLES) == 24 == len(set(rc.TRIPLES)) and all(len(set(t)) == 3 for t in rc.TRIPLES)
    assert {rc.rotate(i) for i in range(96)} == {(o, t) for o in rc.ORDERS for t in rc.TRIPLES}
    assert rc.BAND_UNIT % max(rc.TILE_ROWS) == 0


def test_widths_hold_every_residue_at_every_place():
    for widths in (rc.WIDTHS_ITEM + (4,), rc.WIDTHS_WAVE, rc.WIDTHS_TILE, rc.WIDTHS_BLOCK):
        assert {w % 4 for w in widths} == {0, 1, 2, 3}, widths
    assert rc.WIDTHS_ITEM == (1, 2, 3) and {rc.out_dwords(w) for w in rc.WIDTHS_ITEM} == {1}
    # every residue on both sides of the wave, of the tile and of the production block, bar the full last item below it
    for widths, seam in ((rc.WIDTHS_WAVE, rc.WAVE_ITEMS), (rc.WIDTHS_TILE, rc.TILE_DWORDS),
                         (rc.WIDTHS_BLOCK, rc.launch(rc.PRODUCTION, rc.geometry(4, 1)).per_block)):
        below = {w % 4 for w in widths if rc.out_dwords(w) == seam}
        above = {w % 4 for w in widths if rc.out_dwords(w) == seam + 1}
        assert below >= {0, 2, 3} and above >= {1, 2, 3}, (seam, below, above)
    assert {rc.tile(2, w, 3, 1).tiles_x for w in rc.WIDTHS_TILE} == {1, 2}
    assert rc.tile(2, 1024, 3, 1).tiles_x == 1 and rc.tile(2, 1025, 3, 1) == rc.Tile(2, 2, 0, 1)
    sweep = rc.sweep_cases()
    assert len(sweep) == len(rc.WIDTHS) * 3 and {g.h for g in sweep} == {1, 2, 3}
    for g in sweep:
        p = rc.resolved(rc.padded(g))
        assert p.src_stride == 4 * g.w + 12 and p.dst_stride == rc.round_up_4(g.w) + 12
        assert (g.w % 4 or p.src_stride % 16 == 12) and not rc.launch(rc.PRODUCTION, p).vec16
        assert p.dst_stride % 8 == (4 if rc.out_dwords(g.w) % 2 == 0 else 0)


@pytest.mark.parametrize("shape", rc.LAB_SHAPES, ids=rc.shape_id)
def test_seam_tables_sit_one_step_under_on_and_over_one_and_two_blocks(shape):
    steps = rc.seam_steps(shape)
    assert steps == ((-1, 0, 1) if shape.PX == 4 else (-2, 0, 2))
    seen = []
    for g in rc.seam_cases(shape):
        L = rc.launch(shape, g)
        assert L.px == shape.PX and not L.fallback, (g, L)         # the shape holds: no fall-back moves the seam
        assert L.per_block == 256 * shape.K * shape.PX // 4
        near = round(L.items / L.per_block)
        seen.append((near, L.items - near * L.per_block))
        assert L.blocks == near + (L.items > near * L.per_block)
    assert seen == [(b, s) for b in (1, 2) for s in steps]
    if shape.PX == 4:
        assert {g.w % 4 for g in rc.seam_cases(shape)} == {0, 1, 2, 3}
    assert any(g.n > 1 for g in rc.seam_cases(shape))      # (odd heights: ODD_BATCHES; a prime count has one frame)


def test_odd_batches_put_frame_ends_and_group_seams_inside_blocks():
    s = rc.PRODUCTION
    assert {g.n for g in rc.ODD_BATCHES} == {2, 3, 4, 5} and all(g.h % 2 for g in rc.ODD_BATCHES)
    # a block that holds a frame boundary between two frames of odd height: row parity is y & 1, not row & 1
    assert all(any(len(rc.block_frames(s, g, b)) >= 2 for b in range(rc.launch(s, g).blocks)) for g in rc.ODD_BATCHES)
    assert rc.block_frames(s, rc.geometry(50, 3, 4), 0) == [0, 1, 2, 3]
    rows, frames, parities = False, False, False
    for g in rc.ODD_BATCHES:
        for t in (0, 100, 255):
            groups = [k for k in rc.group_items(s, g, 0, t) if k]
            pos = [rc.item_position(k[0], g.w, g.h) for k in groups]
            if len(pos) == 2:
                rows |= pos[0][0] == pos[1][0] and pos[0][1] != pos[1][1]
                frames |= pos[0][0] != pos[1][0]
                # the two groups of a thread differ in y & 1 although their batch rows have one parity
                r0, r1 = (k[0] // rc.out_dwords(g.w) for k in groups)
                parities |= (r0 & 1) == (r1 & 1) and (pos[0][1] & 1) != (pos[1][1] & 1)
    assert rows and frames and parities
    # a partial item inside a batch, behind a wave seam: width 259
    assert rc.item_position(64, 259, 5) == (0, 0, 64, True) and rc.item_position(65, 259, 5) == (0, 1, 0, False)


def test_px8_cases_are_one_fall_back_reason_each():
    s = rc.Shape(1, 8, 1)
    assert list(rc.PX8_CASES) == ["none", "odd_dwords", "dst_stride", "dst8", "vec16"]
    for name, g in rc.PX8_CASES.items():
        L = rc.launch(s, g)
        assert L.fallback == (() if name == "none" else (name,)), (name, L)
        assert L.px == (8 if name == "none" else 4) and L.per_block == 256 * L.px // 4
        assert rc.launch(rc.PRODUCTION, g).px == 4
        r = rc.resolved(g)
        # what validate () and mibayer_process_device accept
        assert r.src_stride >= 4 * g.w and r.dst_stride >= rc.round_up_4(g.w) and not (r.src_stride | r.dst_stride) & 3
        assert r.src_pitch >= r.src_stride * g.h and r.dst_pitch >= r.dst_stride * g.h
        assert not (r.src_pitch | r.dst_pitch | r.src_off | r.dst_off) & 3
    # kept on an odd out_dwords, the second item of a row's last group would lie in the next row: the case leaves room
    # for it inside the frame on both sides
    r = rc.resolved(rc.PX8_CASES["odd_dwords"])
    assert r.src_stride >= 16 * (rc.out_dwords(r.w) + 1) and r.dst_stride >= 4 * (rc.out_dwords(r.w) + 1)


def test_vec16_cases_flip_each_predicate_alone():
    terms = {name: rc.vec16_terms(g) for name, (g, _) in rc.VEC16_CASES.items()}
    assert all(terms[name] == want for name, (_, want) in rc.VEC16_CASES.items())
    for k in range(3):
        assert {t[k] for t in terms.values()} == {True, False}
        assert any(not t[k] and all(t[:k] + t[k + 1:]) for t in terms.values())
    assert rc.launch(rc.PRODUCTION, rc.VEC16_CASES["all"][0]).vec16
    g, _ = rc.VEC16_CASES["pitch_of_one_frame"]
    assert g.n == 1 and rc.resolved(g).src_pitch % 16 == 4 and rc.launch(rc.PRODUCTION, g).vec16
    g, _ = rc.VEC16_CASES["pitch"]
    assert g.n > 1 and rc.resolved(g).src_pitch % 16 == 4 and not rc.launch(rc.PRODUCTION, g).vec16


def test_pitch_and_alignment_cases():
    for n in (3, 1):
        cases = rc.pitch_cases(n)
        assert len(cases) == 18 and {g.w % 4 for g in cases} == {0, 3}
        for g in cases:
            base = rc.resolved(rc.geometry(g.w, g.h, n))
            assert (g.src_pitch - base.src_pitch, g.dst_pitch - base.dst_pitch) in [
                (s, d) for s in (4, 16, 20) for d in (4, 8, 12)]
        by = lambda w: {(g.src_pitch % 16 == 0, g.dst_pitch % 8 == 0) for g in cases if g.w == w}       # noqa: E731
        assert by(1024) == {(a, b) for a in (True, False) for b in (True, False)}
        assert {rc.launch(rc.PRODUCTION, g).vec16 for g in cases if g.w == 1024} == ({True, False} if n > 1 else {True})
        assert not any(rc.launch(rc.PRODUCTION, g).vec16 for g in cases if g.w == 1023)
    assert [rc.launch(rc.PRODUCTION, g).blocks for g in rc.PITCH_FRAMES] == [5, 5]
    a, b = rc.ALIGN_FRAMES
    assert a.w % 4 == 0 and b.w % 4 == 3 and rc.launch(rc.PRODUCTION, a).items == 520
    assert set(rc.ALIGN_OFFSETS) == {(s, d) for s in (0, 4, 8, 12) for d in (0, 4)}
    assert {rc.launch(rc.PRODUCTION, a._replace(src_off=s)).vec16 for s in (4, 8, 12)} == {False}
    assert {rc.dst8(a._replace(dst_off=d)) for d in (0, 4)} == {True, False}


@pytest.mark.parametrize("shape", rc.LAB_SHAPES, ids=rc.shape_id)
def test_list_frames_end_in_a_partial_block(shape):
    g = rc.list_frame(shape)
    L = rc.launch(shape, g._replace(n=33), is_list=True)
    assert L.px == shape.PX and L.blocks >= 2 and L.items % L.per_block and L.items == g.h * 258
    assert (g.w % 4 != 0) == (shape.PX == 4) and not rc.list_goes_frame_by_frame(shape.K, g.w, g.h)


def test_list_sizes_chunks_and_off_grid_frames():
    assert rc.LIST_SIZES == (1, 2, 16, 17, 33)
    assert [rc.list_chunks(n) for n in rc.LIST_SIZES] == [[1], [2], [16], [16, 1], [16, 16, 1]]
    assert [k // rc.MAX_LIST for k in rc.LIST_OFFSET_FRAMES] == [0, 1]
    g = rc.geometry(rc.LIST_ALIGNED_WIDTH, 3, 16)
    for k in rc.LIST_OFFSET_FRAMES:
        offs = [4 * (f == k % 16) for f in range(16)]
        assert sum(o != 0 for o in offs) == 1
        assert not rc.launch(rc.PRODUCTION, g._replace(src_off=offs), is_list=True).vec16
        assert rc.launch(rc.PRODUCTION, g._replace(dst_off=offs), is_list=True).vec16
        assert not rc.dst8(g._replace(dst_off=offs), is_list=True) and rc.dst8(g._replace(src_off=offs), is_list=True)
        assert rc.launch(rc.Shape(1, 8, 1), g._replace(dst_off=offs), is_list=True).fallback == ("dst8",)
    assert rc.launch(rc.Shape(1, 8, 1), g, is_list=True).px == 8
    # a list under the tile kernel goes frame by frame
    assert rc.list_goes_frame_by_frame(0, 1030, 3) and not rc.list_goes_frame_by_frame(2, 1030, 3)


@pytest.mark.parametrize("R", rc.TILE_ROWS)
def test_tile_cases_reach_the_row_seams_the_walk_and_the_one_dword_tile(R):
    cases = rc.tile_cases(R)
    assert {(g.n * g.h) % R for g in cases} >= {R - 1, 0, 1}
    assert rc.tile(R, 5, 1, 40).walk == R - 1 and rc.geometry(5, 1, 40) in cases
    # frames of 3 rows: more than one step of the walk once a block has 8 rows
    assert rc.tile(R, 1026, 3, 5) == rc.Tile(2, -(-15 // R), {2: 1, 4: 1, 8: 2, 16: 4}[R], 1)
    assert all(rc.tile(R, g.w, g.h, g.n).last_tile_dwords == 1 for g in cases if g.w == 1026)
    # the width sweep is the flat kernel's: a row of one, two and three tiles, a full middle tile (tx = 1 of 3), and
    # a last tile of one dword behind one tile and behind two
    sweep = [rc.tile(R, g.w, g.h, g.n) for g in rc.sweep_cases()]
    assert {t.tiles_x for t in sweep} == {1, 2, 3} and rc.TILE_BANDS == (-1, 0, 1, 3)
    assert {t.tiles_x for t in sweep if t.last_tile_dwords == 1} == {1, 2, 3}
    assert rc.tile(R, 2048, 3, 1)[::3] == (2, 256) and rc.tile(R, 2049, 3, 1)[::3] == (3, 1)
    # the only walk the suite had: one 1 x 1 frame, no step at all
    assert rc.tile(R, 1, 1, 1).walk == 0


def test_banded_frames_band():
    for g in (rc.BANDED_FRAME, rc.BANDED_FRAME_PX8):
        r = rc.resolved(g)
        assert r.src_pitch >= rc.BAND_MIN_BYTES and g.h % 2 == 1 and g.h % rc.BAND_UNIT
        assert [rc.host_bands(b, r.src_pitch, g.h) for b in rc.HOST_BANDS] == [3, 8]
    g = rc.BANDED_FRAME
    assert rc.out_dwords(g.w) == 257 and rc.tile(2, g.w, g.h, 1).last_tile_dwords == 1
    assert rc.host_bands(3, 4 * 1024 * 4095, 4095) == 1        # one row less of 1024 pixels is not banded
    assert rc.launch(rc.Shape(1, 8, 1), rc.BANDED_FRAME_PX8).px == 8
    assert rc.launch(rc.Shape(1, 8, 1), rc.BANDED_FRAME).fallback == ("odd_dwords", "dst_stride", "dst8")


def table_frames():
    """every frame geometry (w, h, src_stride) of the tables, once, the two 17 MB banded frames included"""
    seen = {}
    tables = [rc.sweep_cases(), [rc.padded(g) for g in rc.sweep_cases()], rc.ODD_BATCHES, rc.PX8_CASES.values(),
              [g for g, _ in rc.VEC16_CASES.values()], rc.SELECTOR_SIZES, rc.pitch_cases(3), rc.ALIGN_FRAMES,
              [rc.geometry(rc.LIST_ALIGNED_WIDTH, 3), rc.geometry(1026, 3), rc.BANDED_FRAME, rc.BANDED_FRAME_PX8]]
    tables += [rc.seam_cases(s) + [rc.list_frame(s)] for s in ALL_SHAPES] + [rc.tile_cases(R) for R in rc.TILE_ROWS]
    for g in (g for t in tables for g in t):
        seen[(g.w, g.h, rc.resolved(g).src_stride)] = g._replace(n=1, src_pitch=0, dst_pitch=0)
    return list(seen.values())


def test_numpy_expectation_equals_the_c_oracle_for_every_triple_and_order(oracle):
    """... and, for the ARGB offsets (1, 2, 3), the reference's own compiled transform where oracle/_ref was built"""
    live = oracle.have_ref_frame()
    frames = table_frames()
    assert rc.BANDED_FRAME in frames and rc.BANDED_FRAME_PX8 in frames
    for g in frames:
        frame = rc.frames((1,), g)[0]
        for order in rc.ORDERS:
            for t in rc.TRIPLES:
                want = oracle.rgb2bayer(frame, g.w, order, *t)[:, :g.w]
                assert np.array_equal(rc.expect(frame, g.w, order, t), want), (g, order, t)
            if live:
                want = oracle.ref_frame_rgb2bayer(frame, g.w, order)[:, :g.w]
                assert np.array_equal(rc.expect(frame, g.w, order, (1, 2, 3)), want), (g, order)


def test_frames_of_a_batch_differ():
    g = rc.geometry(6, 3, 5)
    fs = rc.frames((3,), g)
    assert len(fs) == 5 and len({f.tobytes() for f in fs}) == 5 and fs[0].shape == (3, 24)
    assert all(np.array_equal(a, b) for a, b in zip(fs, rc.frames((3,), g)))
    wants = {rc.expect(f, 6, "gbrg", (1, 2, 3)).tobytes() for f in fs}
    assert len(wants) == 5
