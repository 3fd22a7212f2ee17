"""CPU: the parts of the video surface that never touch a GPU -- the encode planner (which frame is a keyframe, where blocks and runs
start and end), the container's run segmentation and validity checks, the lane scheduler, the padded mask rows."""
import threading
import time

import numpy as np
import pytest

from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container as C
from new_bloom_filter_repo_amd.container import is_keyframe, plan_range
from new_bloom_filter_repo_amd.dist import halo_start
from new_bloom_filter_repo_amd.video_compressor import _LanePool


def _brute_force_keys(first_index, start, stop, I, inter_frames):
    """The rule, restated: without inter-frames every frame is a keyframe; else the multiples of the interval and the frames whose
    predecessor was not handed in."""
    keys = []
    for t in range(start, stop):
        if not inter_frames:
            keys.append(t)
        elif t % I == 0:
            keys.append(t)
        elif t == first_index:
            keys.append(t)
    return keys


def test_plan_range_partitions_every_range():
    """Every frame of [start, stop) is either a fixed keyframe or the coded (non-first) frame of exactly one block, never both; a fixed
    keyframe that lies inside a block (not as its first frame) is one of that block's run starts, and nothing else is; blocks read only
    frames that were handed in and are never longer than block_frames."""
    cases = 0
    for I in (1, 3, 5, 30):
        for bf in (2, 5, 7, 60):
            for stop in range(0, 41):
                for start in range(0, stop + 1):
                    for first in {start, halo_start(start, I)}:
                        for inter in (True, False):
                            fixed, blocks = plan_range(first, start, stop, I, bf, inter)
                            what = (first, start, stop, I, bf, inter)
                            assert fixed == _brute_force_keys(first, start, stop, I, inter), what
                            assert fixed == [t for t in range(start, stop) if is_keyframe(t, first, I, inter)], what
                            if not inter:
                                assert blocks == [], what
                            covered = {}                                      # frame -> blocks in which it is a non-first frame
                            for b, (lo, end, starts) in enumerate(blocks):
                                assert first <= lo and lo + 1 < end <= stop and end - lo <= bf, what
                                assert lo + 1 >= start, what                  # only the predecessor may lie in front of the range (the halo frame)
                                assert starts == [u - lo for u in range(lo + 1, end) if u in fixed], what
                                assert lo + 1 not in fixed, what              # a block begins with a frame to code
                                for u in range(lo + 1, end):
                                    covered.setdefault(u, []).append(b)
                            assert all(len(bs) == 1 for bs in covered.values()), what
                            coded = {u for u in covered if u not in fixed}
                            assert coded | set(fixed) == set(range(start, stop)) and not coded & set(fixed), what
                            cases += 1
    assert cases > 20000


def test_plan_range_pinned_plans():
    # the clip of tests/test_gpu_surface.py: 41 frames, interval 5, blocks of 7
    fixed, blocks = plan_range(0, 0, 41, 5, 7, True)
    assert fixed == [0, 5, 10, 15, 20, 25, 30, 35, 40]
    assert blocks == [(0, 7, [5]), (6, 13, [4]), (12, 19, [3]), (18, 25, [2]), (25, 32, [5]), (31, 38, [4]), (37, 41, [3])]
    # a shard that starts inside a GOP, with its halo frame: frames 7 and 8 hang off frame 6, which is only read
    assert plan_range(6, 7, 12, 3, 60, True) == ([9], [(6, 12, [3])])
    # the same shard without the halo frame: its first frame has no predecessor and becomes a keyframe
    assert plan_range(7, 7, 12, 3, 60, True) == ([7, 9], [(7, 12, [2])])
    # blocks of two frames are single pairs; a block never begins with a keyframe
    assert plan_range(0, 0, 7, 4, 2, True) == ([0, 4], [(0, 2, []), (1, 3, []), (2, 4, []), (4, 6, []), (5, 7, [])])
    # all keyframes: no blocks
    assert plan_range(0, 2, 6, 3, 7, False) == ([2, 3, 4, 5], [])
    assert plan_range(0, 0, 4, 1, 7, True) == ([0, 1, 2, 3], [])


def test_inter_runs_and_checks():
    K, I, KR, IR = C.KEY, C.INTER, C.KEY_RICE, C.INTER_RICE
    assert (K, I, KR, IR) == (1, 2, 3, 4) and C.KEYS == (1, 3) and C.INTERS == (2, 4)
    assert C.inter_runs([]) == []
    assert C.inter_runs([K, K, KR]) == []                                     # keyframes only
    assert C.inter_runs([K, I, I, I]) == [(0, 1, 4)]                          # a trailing run
    assert C.inter_runs([K, KR, IR, K, KR, K, I]) == [(1, 2, 3), (5, 6, 7)]   # back-to-back keyframes of both types: the run hangs off the last
    assert C.inter_runs([KR, I, IR, IR, I, K, IR]) == [(0, 1, 5), (5, 6, 7)]  # types 2 and 4 in one run
    assert C.inter_runs([K, I, K, I, K]) == [(0, 1, 2), (2, 3, 4)]
    for ok in ([K], [KR, IR], [K, I, IR, KR]):
        C.check_types(ok)
    with pytest.raises(ValueError, match="unknown record type 5"):
        C.check_types([K, I, 5])
    with pytest.raises(ValueError, match="unknown record type 0"):
        C.check_types([0])
    for bad in ([I, K], [IR], [IR, K, I]):
        with pytest.raises(ValueError, match="inter-frame without a preceding keyframe"):
            C.check_types(bad)
    from new_bloom_filter_repo_amd import sample_codec
    assert (sample_codec.KEY_RICE, sample_codec.INTER_RICE) == (KR, IR)       # still exported where they used to live


class _FakeLane:
    def __init__(self, name):
        self.name = name
        self.users = 0


@pytest.mark.parametrize("nlanes", [1, 2, 3])
def test_lane_pool_schedules_jobs_over_lanes(nlanes):
    lanes = [_FakeLane(i) for i in range(nlanes)]
    pool = _LanePool(lanes)
    lock = threading.Lock()
    state = {"in_flight": 0, "max_in_flight": 0}
    threads, before_take = set(), []

    def fn(job, take):
        before_take.append(job)                                               # work in front of the acquisition holds no lane
        with take() as lane:
            with lock:
                assert lane in lanes
                lane.users += 1
                assert lane.users == 1, "two jobs on one lane"
                state["in_flight"] += 1
                state["max_in_flight"] = max(state["max_in_flight"], state["in_flight"])
                threads.add(threading.get_ident())
            time.sleep(0.002 * (job % 3))
            with lock:
                lane.users -= 1
                state["in_flight"] -= 1
        return job * job
    jobs = list(range(17))
    assert pool.map(jobs, fn) == [j * j for j in jobs]                        # results in job order
    assert sorted(before_take) == jobs
    assert 1 <= state["max_in_flight"] <= nlanes
    assert pool.free.qsize() == nlanes
    if nlanes == 1:
        assert threads == {threading.get_ident()} and before_take == jobs     # one lane: every job on the calling thread, in order
    else:
        assert threading.get_ident() not in threads and len(threads) <= nlanes
    assert pool.map([], fn) == []


@pytest.mark.parametrize("nlanes", [1, 2, 3])
def test_lane_pool_exception_reaches_the_caller_and_returns_the_lanes(nlanes):
    lanes = [_FakeLane(i) for i in range(nlanes)]
    pool = _LanePool(lanes)

    def fn(job, take):
        with take() as lane:
            assert lane in lanes
            if job == 4:
                raise KeyError("job 4")
        return job
    with pytest.raises(KeyError, match="job 4"):
        pool.map(list(range(9)), fn)
    assert pool.free.qsize() == nlanes                                        # every lane is back
    assert sorted(pool.free.get_nowait().name for _ in range(nlanes)) == list(range(nlanes))


def test_mask_rows_matches_the_written_out_idiom():
    rng = np.random.default_rng(5)
    for n in (1, 7, 9, 63, 64, 65, 1000, 96 * 64 + 3):
        nb = (n + 7) // 8
        stride = nat.packed_stride(n)
        masks = [np.packbits(rng.integers(0, 2, n, dtype=np.uint8)),                         # exactly ceil(n/8) bytes
                 rng.integers(0, 256, nb + 11, dtype=np.uint8),                              # a longer row: the tail is not copied
                 list(np.packbits(rng.integers(0, 2, n, dtype=np.uint8))),                   # not an array
                 rng.integers(0, 256, stride + 8, dtype=np.uint8)]
        rows = nat.mask_rows(masks, n)
        assert rows.shape == (len(masks), stride) and rows.dtype == np.uint8 and rows.flags.c_contiguous
        for m, got in zip(masks, rows):
            row = np.zeros(stride, dtype=np.uint8)
            row[:(n + 7) // 8] = np.asarray(m, dtype=np.uint8)[:(n + 7) // 8]
            assert np.array_equal(got, row)
        assert nat.mask_rows(np.stack([masks[0], masks[0]]), n).shape == (2, stride)         # a 2-D array of rows
    assert nat.mask_rows([], 100).shape == (0, nat.packed_stride(100))


def test_frame_geometry():
    assert nat.frame_geometry(np.zeros((4, 6), np.uint8)) == (4, 6, 1, 1)
    assert nat.frame_geometry(np.zeros((4, 6, 3), np.uint16)) == (4, 6, 3, 2)
    assert nat.frame_geometry(np.zeros((2, 5, 4), np.uint8)) == (2, 5, 4, 1)
