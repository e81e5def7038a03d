"""The dense FAST row walk (csrc/orbfe_fast_body.inc) at every length of its last block of eight steps.

The walk keeps FM_PF raw rows in flight and runs whole blocks of eight steps without an exit: the steps a run lacks to a multiple
of eight are padding steps in front of step 0.  How many there are depends on `nsteps mod 8`, with nsteps = rows + 7 in the
cell-row form (k_fast_map_u, ROWS_FAST >= 24) and rows + 8 in the generic form (k_fast_map), so the cases below are chosen to
reach all eight residues in both forms; test_cases_reach_every_block_remainder (no GPU) checks that they do, per run and per
wave, and that no fetch of the walk reads a row the one-row-ahead walk did not read.  The GPU test compares candidates (set and
order), keypoint bit patterns and descriptors with the oracle."""
import numpy as np
import pytest

from test_gpu_extract import assert_same_output
from test_gpu_launch_options import (BATCH, DeviceBatch, check_frame, extractor, fast_runs, fast_work, frame,
                                     level_geometry, ref)

CASE_SHAPES = ("odd", "tiny", "narrow")
ROWS_CELL = (24, 25, 40, 64, 100)   # cell-row form: runs of whole cell rows
ROWS_GENERIC = (8, 9, 13, 16, 23)   # generic form: balanced blocks of at most that many rows
DEPTHS = (1, 2, 3, 4)               # every FM_PF the kernel can be built with


def wave_rows(shape, rows_fast):
    """rows the walk of every wave of the dense lane list covers (the common run length of a cell-row wave, the longest run of a
    generic one): the packing of test_gpu_launch_options.fast_work, which the GPU suite holds against the plan's own counts"""
    cellrows = rows_fast >= 24
    stream = []
    for lvl, L in enumerate(level_geometry(shape)):
        ncol = (L["ix1"] - 16 + 3) // 4
        for ys, nr in fast_runs(L, rows_fast):
            stream += [(lvl, 16 + 4 * c, ys, nr) for c in range(ncol)]

    def same_strip(a, b):
        return a[0] == b[0] and a[2] == b[2] and b[1] == a[1] + 4

    i, out = 0, []
    while i < len(stream):
        first = stream[i]
        lanes = [stream[i - 1][3]] if i > 0 and same_strip(stream[i - 1], stream[i]) else []
        while i < len(stream) and stream[i][0] == first[0] and (not cellrows or stream[i][3] == first[3]) and len(lanes) < 64:
            if len(lanes) == 63 and i + 1 < len(stream) and same_strip(stream[i], stream[i + 1]):
                lanes.append(stream[i][3])
                break
            lanes.append(stream[i][3])
            i += 1
        out.append(max(lanes + [first[3] if cellrows else 0]))
    return out


def walk_fetch_steps(nsteps, depth):
    """the step whose row every fetch of the walk asks for, in order: `depth` fetches in front of the loop, then one per step
    s = -pad .. nsteps - 1 for the row of step s + depth, the step clamped to [0, nsteps] on the scalar side"""
    pad = (8 - nsteps % 8) % 8
    clamp = lambda s: min(max(s, 0), nsteps)   # noqa: E731
    return [clamp(i - pad) for i in range(depth)] + [clamp(s + depth) for s in range(-pad, nsteps)]


def test_cases_reach_every_block_remainder(oracle):
    for rows_set, extra, first_row in ((ROWS_CELL, 7, -3), (ROWS_GENERIC, 8, -4)):
        per_run, per_wave, shortest = set(), set(), 1 << 30
        for shape in CASE_SHAPES:
            for r in rows_set:
                assert (r >= 24) == (extra == 7)
                waves = wave_rows(shape, r)
                assert (sum(n + 8 for n in waves), len(waves)) == fast_work(shape, r), (shape, r)
                per_wave |= {(n + extra) % 8 for n in waves}
                for L in level_geometry(shape):
                    for ys, nrows in fast_runs(L, r):
                        nsteps = nrows + extra
                        per_run.add(nsteps % 8)
                        shortest = min(shortest, nrows)
                        # today's walk: steps 0 .. nsteps - 1, each fetching the row of the next step; the last one reads
                        # row ys + nrows + 4, which lies inside the level (the generic form clamps to the last row besides)
                        last_row = ys + first_row + nsteps
                        assert last_row == ys + nrows + 4 and last_row <= L["h"] - 1, (shape, r, ys, nrows)
                        for d in DEPTHS:
                            steps = walk_fetch_steps(nsteps, d)
                            assert len(steps) % 8 == d % 8 and min(steps) == 0, (shape, r, nrows, d)
                            assert ys + first_row + max(steps) <= last_row, (shape, r, ys, nrows, d)
                            # every step's row is fetched, in order, before the step consumes it
                            pad = (8 - nsteps % 8) % 8
                            assert steps[pad:pad + nsteps] == list(range(nsteps)), (shape, r, nrows, d)
        assert per_run == set(range(8)), (extra, sorted(per_run))
        assert per_wave == set(range(8)), (extra, sorted(per_wave))
        # cell rows: no run shorter than 21 rows; generic: down to a run of one row (nsteps = 9: barely more than one block)
        assert shortest == (21 if extra == 7 else 1), (extra, shortest)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_fast", ROWS_CELL + ROWS_GENERIC)
def test_dense_fast_walk_at_every_block_remainder(oracle, rows_fast):
    """A 9-frame device batch and a single-frame handle, dense FAST modes 0 and 1.  The per-level candidates are checked on the
    first frame and on the last frame of the batch: its last level's last run, the short one, is the end of the launch."""
    for shape in CASE_SHAPES:
        single = extractor(shape, 1, options={"rows_fast": rows_fast})
        batch = extractor(shape, BATCH, options={"rows_fast": rows_fast})
        frames = np.stack([frame(shape, i) for i in range(BATCH)])
        refs = [ref(oracle, shape, i) for i in range(BATCH)]
        for mode in (0, 1):
            label = (shape, rows_fast, mode)
            single.set_fast_mode(mode)
            batch.set_fast_mode(mode)
            gk, gd = single(frames[BATCH - 1])
            check_frame(single, 0, refs[BATCH - 1], label + ("single",), stages=("cand",))
            assert_same_output(gk, gd, refs[BATCH - 1].kps, refs[BATCH - 1].desc)
            db = DeviceBatch(batch, frames)
            for b in range(BATCH):
                assert_same_output(*db.output(b), refs[b].kps, refs[b].desc)
            for b in (0, BATCH - 1):
                check_frame(batch, b, refs[b], label + ("batch", b), stages=("cand",))
        for e in (single, batch):   # the plan the calls ran is the one the coverage test reasons about
            got = e.work_counts()
            assert (got["fast_row_steps_per_frame"], got["fast_waves_per_frame"]) == fast_work(shape, rows_fast), (shape, got)
