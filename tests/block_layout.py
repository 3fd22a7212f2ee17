"""Where the block-stage sweep (tests/test_gpu_block_stage_sweep.py) puts its frames -- a helper, not a test.  Pure numpy / ctypes: the
device is only touched through the DeviceBuffer a caller hands in.

LaneShape says which pixels of a frame the lane kernels' workgroups and the per-pixel tail own.  FarBlock lays a few items (frames, or
packed mask rows) out inside ONE large allocation so that every 64-bit byte offset a stage forms -- f * stride -- has a 32-bit truncation
that lands on a DECOY inside the same allocation: an item of the same shape with other content, between two poisoned windows.  A kernel
that truncates then reads or writes a decoy, the test sees a wrong answer or a changed decoy, and nothing outside the allocation is
touched.  Only the items, decoys and windows are ever uploaded, filled or downloaded."""
import numpy as np

WG_THREADS = 256            # csrc/rbf_device.h: the lane kernels' workgroup
WINDOW = 1 << 16
POISON = 0xA5
ITEM_MAX = 1 << 20
ROW_MAX = 1 << 15                                                  # a far mask row: its decoy sits 2^16 behind row 0
FRAME_BASE, FRAME_STRIDE = 1 << 31, (1 << 31) + (1 << 20)
MASK_BASE, MASK_STRIDE = 0, (1 << 32) + (1 << 16)


class LaneShape:
    """A frame of n pixels under a lane kernel whose lanes own `lane_pixels` pixels each: the pixel ranges of its workgroups and of the
    per-pixel tail behind the last whole lane."""

    def __init__(self, n, lane_pixels):
        self.n, self.lane_pixels = int(n), int(lane_pixels)
        self.lanes = self.n // self.lane_pixels
        self.first_tail = self.lanes * self.lane_pixels
        self.workgroups = -(-self.lanes // WG_THREADS)
        self.full_workgroups = self.lanes // WG_THREADS
        self.last_lanes = self.lanes - self.full_workgroups * WG_THREADS         # lanes of the partly filled workgroup (0: none)

    def workgroup(self, w):
        """The pixels [lo, hi) of lane workgroup w."""
        per = WG_THREADS * self.lane_pixels
        return min(w * per, self.first_tail), min((w + 1) * per, self.first_tail)

    def tail(self):
        return self.first_tail, self.n


def truncations(offset):
    """What a 64-bit byte offset becomes when a kernel keeps 32 bits of it: (read unsigned, read signed)."""
    lo = int(offset) & 0xFFFFFFFF
    return lo, lo - (1 << 32) if lo >> 31 else lo


class FarBlock:
    """`count` items of item_bytes each at base + f * stride inside one allocation of nbytes.

    items      the allocation offsets of the items
    aliases    per item: the allocation offsets base + t for the 32-bit truncations t of f * stride that differ from f * stride
    decoys     [(allocation offset, the item it stands in for)], one per distinct alias
    windows    [(lo, hi)] poisoned guard ranges: WINDOW bytes on each side of every item and decoy, cut short where they meet the
               allocation's start or a neighbouring item / decoy, and merged where two of them touch -- so no two regions overlap
    """

    def __init__(self, item_bytes, count, base, stride, window=WINDOW):
        self.item_bytes, self.count, self.base, self.stride, self.window = int(item_bytes), int(count), int(base), int(stride), int(window)
        if not 0 < self.item_bytes <= ITEM_MAX:
            raise ValueError("an item of %d bytes: 1 .. %d" % (self.item_bytes, ITEM_MAX))
        self.items = [self.base + f * self.stride for f in range(self.count)]
        self.aliases = []
        for f in range(self.count):
            off = f * self.stride
            self.aliases.append(sorted({self.base + t for t in truncations(off) if t != off}))
        seen = {}
        for f, al in enumerate(self.aliases):
            for a in al:
                if a in seen:
                    raise ValueError("items %d and %d alias to the same place" % (seen[a], f))
                seen[a] = f
        self.decoys = sorted(seen.items())
        solid = sorted([(o, o + self.item_bytes) for o in self.items] + [(o, o + self.item_bytes) for o, _ in self.decoys])
        if solid[0][0] < 0:
            raise ValueError("an alias in front of the allocation: %d" % solid[0][0])
        for (a0, a1), (b0, b1) in zip(solid, solid[1:]):
            if b0 < a1:
                raise ValueError("an item and a decoy overlap: [%d, %d) and [%d, %d)" % (a0, a1, b0, b1))
        self.nbytes = solid[-1][1] + self.window
        raw = []
        for i, (lo, hi) in enumerate(solid):
            floor = solid[i - 1][1] if i else 0
            ceil = solid[i + 1][0] if i + 1 < len(solid) else self.nbytes
            raw.append((max(lo - self.window, floor), lo))
            raw.append((hi, min(hi + self.window, ceil)))
        self.windows = []
        for lo, hi in sorted(w for w in raw if w[1] > w[0]):
            if self.windows and lo <= self.windows[-1][1]:
                self.windows[-1] = (self.windows[-1][0], max(hi, self.windows[-1][1]))
            else:
                self.windows.append((lo, hi))

    def regions(self):
        """Every (lo, hi) the test touches: items, decoys, windows -- sorted."""
        return sorted([(o, o + self.item_bytes) for o in self.items] + [(o, o + self.item_bytes) for o, _ in self.decoys] + self.windows)

    # ------------------------------------------------------------------ the device side (buf: a DeviceBuffer of self.nbytes)
    def place(self, buf, items, decoys):
        """Upload the items and the decoys (arrays of item_bytes each, decoys in self.decoys' order) and fill every window with POISON."""
        from new_bloom_filter_repo_amd import _native as nat
        assert buf.nbytes >= self.nbytes and len(items) == self.count and len(decoys) == len(self.decoys)
        for lo, hi in self.windows:
            if hasattr(buf, "fill"):                              # (the CPU test's stand-in for a device block)
                buf.fill(lo, POISON, hi - lo)
            else:
                nat.check(nat.lib().rbf_memset(buf.ctx.handle, buf.ptr + lo, POISON, hi - lo))
        for off, a in list(zip(self.items, items)) + [(o, d) for (o, _), d in zip(self.decoys, decoys)]:
            raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            assert raw.nbytes == self.item_bytes
            buf.upload(raw, off)
        buf.ctx.sync()

    def fetch(self, buf):
        """(the items' bytes, the decoys' bytes, the windows' bytes) as they are on the device now."""
        buf.ctx.sync()
        return ([buf.download(self.item_bytes, o) for o in self.items], [buf.download(self.item_bytes, o) for o, _ in self.decoys],
                [buf.download(hi - lo, lo) for lo, hi in self.windows])

    def untouched(self, buf, decoys):
        """Assert that every decoy still holds what was placed and every window is POISON; returns the items' bytes."""
        got, dec, win = self.fetch(buf)
        for (off, f), d, want in zip(self.decoys, dec, decoys):
            assert np.array_equal(d, np.ascontiguousarray(want).reshape(-1).view(np.uint8)), "the decoy of item %d at %#x was written" % (f, off)
        for (lo, hi), w in zip(self.windows, win):
            assert (w == POISON).all(), "the window [%#x, %#x) was written" % (lo, hi)
        return got


def far_frames(frame_bytes, count=3):
    """The sweep's frame layout: base 2^31, stride 2^31 + 2^20 (frame 1's offset truncates, signed, to allocation offset 2^20; frame 2's,
    signed or unsigned, to base + 2^21)."""
    return FarBlock(frame_bytes, count, FRAME_BASE, FRAME_STRIDE)


def far_frames_nbytes():
    """An allocation that holds the far frames of every size up to ITEM_MAX."""
    return far_frames(ITEM_MAX).nbytes


def far_masks_nbytes():
    return far_masks(ROW_MAX).nbytes


def far_masks(row_bytes, count=2):
    """The sweep's mask-row layout: base 0, stride 2^32 + 2^16 (row 1's offset truncates to 2^16)."""
    return FarBlock(row_bytes, count, MASK_BASE, MASK_STRIDE)


# ------------------------------------------------------------------ the lane sweep's clip (Part A of the sweep)
LANE_W, LANE_H, LANE_F, LANE_STARTS = 799, 11, 7, [3]
LANE_N = LANE_W * LANE_H                                         # 8789 pixels
HOLD_LANE_PIXELS, LOOKAHEAD_LANE_PIXELS, CUT_LANE_PIXELS = 16, 8, 16
LANE_CASES = [(dt, C) for dt in (np.uint8, np.uint16) for C in (1, 2, 3, 4)]
LANE_IDS = ["%s_c%d" % (np.dtype(dt).name, C) for dt, C in LANE_CASES]
# (dtype name, C) -> a seed other than the default 7000 + 10 * sample bytes + C, where that one is vacuous: with four samples to a pixel the
# default clips leave none of the five tail pixels held-and-moved at max_error = 1 (test_block_layout_cpu.py checks every seed)
LANE_SEEDS = {("uint8", 4): 7100, ("uint16", 4): 7100}


def lane_errors(dtype):
    return (1, 7) + ((0x7FFF,) if np.dtype(dtype).itemsize == 2 else ())


def lane_clip(dtype, C):
    """The sweep's input of one (dtype, C): F = 7 frames of 799x11 from near_lossless_ref.random_clip."""
    from near_lossless_ref import random_clip
    seed = LANE_SEEDS.get((np.dtype(dtype).name, C), 7000 + 10 * np.dtype(dtype).itemsize + C)
    return random_clip(seed, LANE_F, LANE_H, LANE_W, C, dtype)


def changed_pixels(x, y):
    """bool (F, n): the pixels of every frame in which y differs from x in some sample."""
    d = np.asarray(x) != np.asarray(y)
    if d.ndim == 4:
        d = d.any(axis=-1)
    return d.reshape(len(d), -1)


def lane_non_vacuous(x, y, lane_pixels):
    """The sweep's condition on a reference output y of the input x: over the 7 frames, the third lane workgroup holds a pixel that changed
    and one that did not, and so do the tail pixels behind the last whole lane."""
    shape = LaneShape(LANE_N, lane_pixels)
    assert shape.workgroups >= 3 and shape.tail()[1] - shape.tail()[0] == 5
    ch = changed_pixels(x, y)
    for lo, hi in (shape.workgroup(2), shape.tail()):
        part = ch[:, lo:hi]
        if not (part.any() and not part.all()):
            return False
    return True


def cut_non_vacuous(x, tolerance):
    """The same for the cut statistics, which write no frame: over the pairs, the third lane workgroup holds a moving pixel and a still one,
    and the tail a moving one (every pixel counts in intra_bits whatever it does)."""
    shape = LaneShape(LANE_N, CUT_LANE_PIXELS)
    x = np.asarray(x).astype(np.int64)
    moving = (np.abs(x[1:] - x[:-1]) > tolerance).any(axis=-1).reshape(len(x) - 1, -1)
    (lo, hi), (t0, t1) = shape.workgroup(2), shape.tail()
    return bool(moving[:, lo:hi].any() and not moving[:, lo:hi].all() and moving[:, t0:t1].any())
