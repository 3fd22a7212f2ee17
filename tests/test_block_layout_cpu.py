"""tests/block_layout.py on the CPU: the far layouts of the block-stage sweep hold what they claim (nothing overlaps, every far offset
passes the 2^31 or 2^32 it is meant to pass, every alias is the 32-bit truncation it stands for and lies inside the allocation), and the
lane sweep's clips are not vacuous on the reference -- so a seed that is never reaches the GPU test."""
import numpy as np
import pytest

import block_layout as bl
from lookahead_ref import lookahead_ref
from near_lossless_ref import hold_ref

# (item bytes) of every far case of the sweep: 799x11 and 128x64 frames of u8 C=3, u16 C=4, u16 C=1, planar u8 luma; 70 000 digest bytes;
# the pan search's 320x180 u8 C=3 frames; the roll's 64x16 pixels of 4 bytes and 67x33 pixels of 3 bytes
FRAME_BYTES = [799 * 11 * 3, 799 * 11 * 8, 799 * 11 * 2, 799 * 11, 128 * 64 * 3, 128 * 64, 70000, 320 * 180 * 3, 64 * 16 * 4, 67 * 33 * 3,
               bl.ITEM_MAX]
ROW_BYTES = [(799 * 11 + 63) // 64 * 8, 128 * 64 // 8, bl.ROW_MAX]


def disjoint(regions):
    return all(a[1] <= b[0] for a, b in zip(regions, regions[1:])) and all(lo < hi for lo, hi in regions)


@pytest.mark.parametrize("nbytes", FRAME_BYTES)
def test_far_frames(nbytes):
    fb = bl.far_frames(nbytes)
    assert fb.base == 1 << 31 and fb.stride == (1 << 31) + (1 << 20) and fb.base % 16 == 0 and fb.stride % 16 == 0
    assert fb.items == [1 << 31, (1 << 32) + (1 << 20), (1 << 32) + (1 << 31) + (1 << 21)]
    assert fb.stride >= 1 << 31 and 2 * fb.stride >= 1 << 32, "frame 1 passes 2^31, frame 2 passes 2^32"
    assert fb.aliases == [[], [1 << 20], [(1 << 31) + (1 << 21)]]
    assert fb.decoys == [(1 << 20, 1), ((1 << 31) + (1 << 21), 2)]
    check_aliases(fb)
    assert fb.nbytes == fb.items[2] + nbytes + bl.WINDOW and fb.nbytes < 7 << 30
    assert len(fb.windows) == 10 and all(hi - lo == bl.WINDOW for lo, hi in fb.windows), "64 KiB on each side of 3 frames and 2 decoys"


@pytest.mark.parametrize("nbytes", ROW_BYTES)
def test_far_mask_rows(nbytes):
    mb = bl.far_masks(nbytes)
    assert mb.base == 0 and mb.stride == (1 << 32) + (1 << 16) and mb.stride % 16 == 0 and nbytes % 8 == 0
    assert mb.items == [0, (1 << 32) + (1 << 16)] and mb.stride >= 1 << 32
    assert mb.aliases == [[], [1 << 16]] and mb.decoys == [(1 << 16, 1)]
    check_aliases(mb)
    assert mb.nbytes == mb.items[1] + nbytes + bl.WINDOW and mb.nbytes < 5 << 30
    # row 0 starts the allocation and the decoy follows it inside 64 KiB: one window between them, cut to the gap
    assert mb.windows == [(nbytes, 1 << 16), ((1 << 16) + nbytes, (2 << 16) + nbytes), (mb.items[1] - bl.WINDOW, mb.items[1]),
                          (mb.items[1] + nbytes, mb.nbytes)]


def check_aliases(fb):
    regions = fb.regions()
    assert disjoint(regions), "no two of {items, decoys, windows} overlap"
    assert regions[0][0] >= 0 and regions[-1][1] == fb.nbytes
    for f, item in enumerate(fb.items):
        off = item - fb.base
        assert off == f * fb.stride
        unsigned, signed = bl.truncations(off)
        assert unsigned == off % (1 << 32) and signed == (unsigned ^ (1 << 31)) - (1 << 31)
        for t in (unsigned, signed):
            place = fb.base + t
            if t == off:
                continue                                           # the offset fits: no alias
            assert place in fb.aliases[f] and (place, f) in fb.decoys
            assert 0 <= place and place + fb.item_bytes <= fb.nbytes, "the alias lies inside the allocation"
        if f:
            assert fb.aliases[f], "every far item has a decoy"
    # every item and every decoy has poison directly in front of it (except at the allocation's start) and directly behind it
    edges_lo, edges_hi = {lo for lo, _ in fb.windows}, {hi for _, hi in fb.windows}
    for o in fb.items + [o for o, _ in fb.decoys]:
        assert o == 0 or o in edges_hi
        assert o + fb.item_bytes in edges_lo


def test_layout_refuses_what_it_cannot_guard():
    with pytest.raises(ValueError):
        bl.FarBlock(bl.ITEM_MAX + 1, 3, bl.FRAME_BASE, bl.FRAME_STRIDE)
    with pytest.raises(ValueError):
        bl.FarBlock(4096, 2, 0, 1 << 31)                       # signed truncation of frame 1 lands in front of the allocation
    with pytest.raises(ValueError):
        bl.FarBlock(4096, 3, 0, (1 << 32) + 1024)               # frame 1's alias overlaps frame 0
    assert bl.truncations(0x1_8000_0010) == (0x8000_0010, 0x8000_0010 - (1 << 32)) and bl.truncations(5) == (5, 5)


class HostBlock:
    """A stand-in for a device block of nbytes that keeps only the bytes that were written."""

    class _Ctx:
        def sync(self):
            pass

    def __init__(self, nbytes):
        self.nbytes, self.ctx, self.ptr, self.parts = nbytes, self._Ctx(), 0, {}

    def fill(self, offset, value, nbytes):
        self.parts[offset] = np.full(nbytes, value, np.uint8)

    def upload(self, arr, offset=0):
        assert offset + arr.nbytes <= self.nbytes
        self.parts[offset] = np.array(arr, dtype=np.uint8).reshape(-1)

    def download(self, nbytes, offset=0):
        return self.parts[offset][:nbytes].copy()


def test_place_and_untouched_see_a_written_decoy_and_a_written_window():
    assert bl.far_frames_nbytes() == bl.far_frames(bl.ITEM_MAX).nbytes < 7 << 30 and bl.far_masks_nbytes() < 5 << 30
    for lay, buf in ((bl.far_frames(70000), HostBlock(bl.far_frames_nbytes())), (bl.far_masks(1104), HostBlock(bl.far_masks_nbytes()))):
        rng = np.random.default_rng(lay.count)
        items = [rng.integers(0, 256, lay.item_bytes, dtype=np.uint8) for _ in range(lay.count)]
        decoys = [rng.integers(0, 256, lay.item_bytes, dtype=np.uint8) for _ in lay.decoys]
        lay.place(buf, items, decoys)
        assert sorted(buf.parts) == [lo for lo, _ in lay.regions()], "only the items, decoys and windows are touched"
        assert sum(p.nbytes for p in buf.parts.values()) < 2 << 20
        got = lay.untouched(buf, decoys)
        assert all(np.array_equal(g, i) for g, i in zip(got, items))
        buf.parts[lay.decoys[-1][0]][7] ^= 1
        with pytest.raises(AssertionError, match="decoy"):
            lay.untouched(buf, decoys)
        buf.parts[lay.decoys[-1][0]][7] ^= 1
        buf.parts[lay.windows[1][0]][0] = 0
        with pytest.raises(AssertionError, match="window"):
            lay.untouched(buf, decoys)


def test_lane_shape_of_the_sweep():
    hold, la = bl.LaneShape(bl.LANE_N, bl.HOLD_LANE_PIXELS), bl.LaneShape(bl.LANE_N, bl.LOOKAHEAD_LANE_PIXELS)
    assert (hold.full_workgroups, hold.last_lanes, hold.tail()) == (2, 37, (8784, 8789)), "2 full workgroups, 37 lanes, 5 tail pixels"
    assert (la.full_workgroups, la.last_lanes, la.tail()) == (4, 74, (8784, 8789)), "4 full workgroups, 74 lanes, 5 tail pixels"
    assert hold.workgroup(2) == (8192, 8784) and la.workgroup(2) == (4096, 6144) and la.workgroup(4) == (8192, 8784)
    assert -(-bl.LANE_N // bl.WG_THREADS) == 35, "the per-pixel kernels take 35 workgroups"


@pytest.mark.parametrize("dtype,C", bl.LANE_CASES, ids=bl.LANE_IDS)
def test_lane_clips_are_not_vacuous(dtype, C):
    x = bl.lane_clip(dtype, C)
    assert x.shape == (7, 11, 799, C) and x.dtype == dtype
    for e in bl.lane_errors(dtype):
        assert bl.lane_non_vacuous(x, hold_ref(x, bl.LANE_STARTS, e), bl.HOLD_LANE_PIXELS), ("hold", e)
        assert bl.lane_non_vacuous(x, lookahead_ref(x, bl.LANE_STARTS, e)[0], bl.LOOKAHEAD_LANE_PIXELS), ("lookahead", e)
    assert bl.cut_non_vacuous(x, 1)


# ------------------------------------------------------------------ the keyframe quantiser's far frames and its shared-scratch sequence
@pytest.mark.parametrize("dtype,C,bounds", bl.FAR_KEYQUANT_CASES, ids=bl.FAR_KEYQUANT_IDS)
def test_far_keyquant_frames_pass_2_31_and_2_32_and_their_decoys_matter(dtype, C, bounds):
    x, decoys, want, streams = bl.far_keyquant_case(dtype, C, bounds)
    assert x[0].nbytes in FRAME_BYTES, "test_far_frames checks this layout"
    lay = bl.far_frames(x[0].nbytes)
    offsets = [lay.items[f] - lay.base for f in bl.FAR_KEYQUANT_LISTED]
    assert offsets[0] >= 1 << 31 and offsets[1] >= 1 << 32, "frame_index[f] * frame_stride of the listed frames"
    assert all(lay.aliases[f] for f in bl.FAR_KEYQUANT_LISTED) and 0 not in bl.FAR_KEYQUANT_LISTED
    assert bl.far_keyquant_decoys_matter(x, decoys, want, streams, bounds)
    assert 0 in bounds or C == 3, "one of the cases has an exact channel"


def test_the_keyquant_sequence_shrinks_and_grows_in_count_and_in_frame_size():
    sizes = [bl.keyquant_step_sizes(bl.KEYQUANT_STEPS[i]) for i in bl.KEYQUANT_ORDER if i < len(bl.KEYQUANT_STEPS)]
    for what in range(3):                        # the count of listed frames, a frame's samples, the samples in the shared u buffer
        seq = [s[what] for s in sizes]
        ups, downs = [b > a for a, b in zip(seq, seq[1:])], [b < a for a, b in zip(seq, seq[1:])]
        assert any(ups) and any(downs) and downs.index(True) < len(ups) - 1 - ups[::-1].index(True), (what, seq)
    order = bl.KEYQUANT_ORDER
    assert set(order) == set(range(6)) and all(a != b for a, b in zip(order, order[1:])), "every step, none twice in a row"
    # every near-encode call is followed, somewhere, directly by each of the three stages that share its u buffer
    assert {b for a, b in zip(order, order[1:]) if a < 3 and b >= 3} == {3, 4, 5}
