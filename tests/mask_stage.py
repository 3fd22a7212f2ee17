"""What the mask-stage sweep (tests/test_gpu_mask_stage_sweep.py, tests/test_mask_stage_cpu.py) runs and what it expects -- a helper, not
a test.  Plain numpy; the device is only touched through the buffers a caller hands in.

  reference  ref_masks: A1 and the all-channel paragraph of include/rbf.h in int64 numpy, written from that text and not from the kernels.
  clips      one_hot_clip (one byte of one lane's tile changes per pair), value grids (every (a, b) of 8-bit samples, the int16 rule's edge
             values of 16-bit ones in every pixel slot of a lane), count_clip (every pair another count; 0 and the full frame among them).
  tables     KERNELS (the eight instantiations of the GOP mask kernels), KNOBS, the thresholds, the chunk and ticket shapes.
  mutants    MUTANTS: the wrong rules a kernel could have.  tests/test_mask_stage_cpu.py shows that each differs from the true rule on a
             case the GPU sweep runs.
"""
import collections

import numpy as np

POISON = 0xA5
GUARD = 512
SEG = 1024                                                        # pixels of a segment: one wave of the GOP mask kernels
WG_WAVES = 4
MASK_TICKETS = 64
MASK_MAX_CHUNKS = 256
INT32_MAX = 0x7FFFFFFF

# name, sample bytes, pixel bytes, mask_channels (1 = the luma rule)
Kernel = collections.namedtuple("Kernel", "name sample_bytes pixel_bytes mask_channels")
KERNELS = [
    Kernel("u8_px1_luma", 1, 1, 1), Kernel("u8_px3_luma", 1, 3, 1), Kernel("u16_px2_luma", 2, 2, 1), Kernel("u16_px6_luma", 2, 6, 1),
    Kernel("u8_px3_all", 1, 3, 3), Kernel("u8_px4_all", 1, 4, 4), Kernel("u16_px6_all", 2, 6, 3), Kernel("u16_px8_all", 2, 8, 4),
]
KERNEL_IDS = [k.name for k in KERNELS]
KNOBS = [0, 4, 1]                                                 # rbf_ctx_force_generic: fast | per-pixel bits in the fast kernel | generic kernel
KNOB_IDS = ["fast", "generic_bits", "generic_kernel"]
XORS = [0x01, 0x80, 0x40]
THR_U8 = [-1, 0, 1, 127, 128, 254, 255, 256]
THR_U16 = [-1, 0, 1, 0x7FFE, 0x7FFF, 0x8000, INT32_MAX]


def dtype_of(sample_bytes):
    return np.uint8 if sample_bytes == 1 else np.dtype("<u2")


def samples_per_pixel(kernel):
    return kernel.pixel_bytes // kernel.sample_bytes


def knobs_of(kernel):
    """The all-channel kernels have no per-pixel threshold path: knob bit 2 changes nothing for them."""
    return KNOBS if kernel.mask_channels == 1 else [0, 1]


def thresholds_of(kernel):
    if kernel.mask_channels != 1:
        return [0]
    return THR_U8 if kernel.sample_bytes == 1 else THR_U16


def packed_stride(nbits):
    return (int(nbits) + 63) // 64 * 8


# ------------------------------------------------------------------ the reference
def pair_bits(prev, curr, thr, mask_channels):
    """One pair: prev, curr (n, C) unsigned samples -> bool [n].  include/rbf.h, A1: bit = abs_int16(prev - curr) > thr with numpy's int16
    wrap (the difference is taken mod 2^16 and read as int16; the absolute value of -32768 stays -32768).  All-channel: any of the first
    mask_channels samples differs, an exact comparison."""
    a, b = prev.astype(np.int64), curr.astype(np.int64)
    if mask_channels >= 2:
        return (a[:, :mask_channels] != b[:, :mask_channels]).any(-1)
    d = (a[:, 0] - b[:, 0]) % 65536
    d = np.where(d >= 32768, d - 65536, d)                        # read as int16
    ad = np.where(d < 0, -d, d)
    ad = np.where(ad >= 32768, ad - 65536, ad)                    # -(-32768) wraps to -32768
    return ad > int(thr)


def skipped_pairs(nframes, run_starts):
    """Pair t - 1 is not coded when frame t starts a run (run_starts: the frame indices, frame 0 never counts)."""
    return sorted({int(t) - 1 for t in (run_starts or ()) if 1 <= int(t) < nframes})


def ref_masks(frames, layout, thr, mask_channels=1, run_starts=None):
    """frames (F, n, C) unsigned samples (or (F, H, W, C)); layout: anything with the frame's pixel count as `.n`, or None; thr: one
    threshold or one per pair.  Returns (rows uint8 [F - 1, ceil(n / 64) * 8], MSB-first, pad bits 0; ones int64 [F - 1]).  A skipped pair
    is a zero row and a zero count."""
    frames = np.asarray(frames)
    F = frames.shape[0]
    frames = frames.reshape(F, -1, frames.shape[-1])
    n = frames.shape[1]
    assert layout is None or layout.n == n
    thrs = [int(thr)] * (F - 1) if np.isscalar(thr) else [int(t) for t in thr]
    assert len(thrs) == F - 1
    skip = set(skipped_pairs(F, run_starts))
    rows, ones = np.zeros((F - 1, packed_stride(n)), np.uint8), np.zeros(F - 1, np.int64)
    for f in range(F - 1):
        if f in skip:
            continue
        bits = pair_bits(frames[f], frames[f + 1], thrs[f], mask_channels)
        rows[f, :(n + 7) // 8] = np.packbits(bits)
        ones[f] = int(bits.sum())
    return rows, ones


# ------------------------------------------------------------------ clips
def as_samples(raw, kernel):
    """(F, n * pixel_bytes) bytes -> (F, n, C) samples."""
    F = raw.shape[0]
    return np.ascontiguousarray(raw).view(dtype_of(kernel.sample_bytes)).reshape(F, -1, samples_per_pixel(kernel))


def one_hot_clip(sample_bytes, pixel_bytes, xor_value, seed=7):
    """16 * pixel_bytes + 1 frames of 64x32 (two segments) as samples (F, 2048, C): frame t + 1 is frame t with ONE byte XOR-ed -- byte
    t mod (16 * pixel_bytes) of the 16-pixel tile of lane (7 t + 3) mod 64 in segment t mod 2."""
    T, n = 16 * pixel_bytes, 2 * SEG
    rng = np.random.default_rng(seed + 16 * pixel_bytes + sample_bytes)
    raw = np.empty((T + 1, n * pixel_bytes), np.uint8)
    raw[0] = rng.integers(0, 256, n * pixel_bytes, dtype=np.uint8)
    for t in range(T):
        raw[t + 1] = raw[t]
        at = ((t % 2) * SEG + ((7 * t + 3) % 64) * 16) * pixel_bytes + t % T
        raw[t + 1, at] ^= xor_value
    return as_samples(raw, Kernel("", sample_bytes, pixel_bytes, 0))


def one_hot_byte(t, pixel_bytes):
    """(pixel index, byte of the pixel) that pair t of a one-hot clip changes."""
    b = t % (16 * pixel_bytes)
    return (t % 2) * SEG + ((7 * t + 3) % 64) * 16 + b // pixel_bytes, b % pixel_bytes


def u8_grid():
    """Two planes of 256 x 256 samples in which every (a, b) occurs once."""
    i = np.arange(65536)
    return (i >> 8).astype(np.uint8), (i & 255).astype(np.uint8)


U16_EDGES = [0, 1, 0x7FFE, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF]


def u16_values(seed=16):
    rng = np.random.default_rng(seed)
    vals = U16_EDGES + [int(v) for v in rng.integers(0, 65536, 24)]
    assert len(vals) == 32
    return np.array(vals, dtype="<u2")


def u16_grid():
    """Two planes of 16384 samples: the 1024 pairs of u16_values, 16 times, repetition r rotated by r -- pixel i holds pair (i + r) mod
    1024, so pair p sits in pixel slot (p - r) mod 16 of its lane: every pair in every slot."""
    v = u16_values()
    i = np.arange(16 * 1024)
    p = (i + i // 1024) % 1024
    return v[p // 32], v[p % 32]


def grid_clip(kernel, position=None, pairs=1):
    """The value grid of the kernel's sample type as frames (F, n, C).  position None: for every sample position c in turn the frames
    A_c, B_c (2 C frames; the grid in sample c, the other samples held at a constant): the pairs (A_c, B_c) are the grid, the pairs between
    them cross from one position to the next and are held against the reference like any other.  position c, pairs P: the frames A, B, A,
    B ... (P + 1 of them) with the grid in sample c: a pair for every threshold of a per-pair table."""
    a, b = u8_grid() if kernel.sample_bytes == 1 else u16_grid()
    C, dt = samples_per_pixel(kernel), dtype_of(kernel.sample_bytes)
    const = 0x5A if kernel.sample_bytes == 1 else 0x815A

    def frame(plane, c):
        fr = np.full((plane.size, C), const, dt)
        fr[:, c] = plane
        return fr
    if position is None:
        return np.stack([frame(pl, c) for c in range(C) for pl in (a, b)])
    return np.stack([frame(b if t % 2 else a, position) for t in range(pairs + 1)])


def counts_of(P, n):
    """P distinct counts in [0, n].  From two pairs on: n and n - 1 on the neighbouring pairs (2s, 2s + 1) -- every wave but the one with
    the unchanged pixel then files 1024 | 1024 << 16, both halves of a packed tally word at their maximum -- and from three on 0 on the
    even pair behind them (the last pair when there is none: P = 3)."""
    step = max(1, min(11, (n - 8) // max(P, 1)))
    c = [3 + step * i for i in range(P)]
    assert c[-1] < n - 1
    if P == 1:
        return [n]
    e = 2 * ((P - 2) // 4)
    c[e], c[e + 1] = n, n - 1
    if P >= 3:
        c[e + 2 if e + 2 < P else P - 1] = 0
    assert len(set(c)) == P
    return c


def count_clip(P, kernel, n, seed=3, xor_value=0x40):
    """P + 1 frames (F, n, C): pair i changes exactly counts_of(P, n)[i] pixels, at places drawn from seed + i.  The luma kernels' change
    is xor_value on the luma's low byte (a difference of 64: above every threshold of count_thresholds), the all-channel kernels' on
    byte i mod pixel_bytes of the pixel."""
    counts = counts_of(P, n)
    rng = np.random.default_rng(seed)
    raw = np.empty((P + 1, n, kernel.pixel_bytes), np.uint8)
    raw[0] = rng.integers(0, 256, (n, kernel.pixel_bytes), dtype=np.uint8)
    for i, c in enumerate(counts):
        raw[i + 1] = raw[i]
        where = np.random.default_rng(seed * 1000 + i).permutation(n)[:c]
        raw[i + 1, where, 0 if kernel.mask_channels == 1 else i % kernel.pixel_bytes] ^= xor_value
    return as_samples(raw.reshape(P + 1, -1), kernel), counts


def count_thresholds(P):
    """A per-pair table for a count clip of the luma kernels: every entry below the clip's difference of 64, neighbours differ."""
    return [(7 * i) % 64 for i in range(P)]


CHUNK_PAIRS = [1, 2, 3, 4, 5, 31, 64, 65, 129, 130, 257, 299]
CHUNK_KNOBS = [0, 1, 2, 3, 4, 5, 7, 16, 31]                        # rbf_ctx_force_generic bits 8..12; 0 = auto
CHUNK_KERNELS = [KERNELS[0], KERNELS[7]]


def run_patterns(nframes):
    """{name: run-start frames} of the chunk sweep."""
    F = nframes
    return {"none": [], "every_2nd": list(range(2, F, 2)), "adjacent": [t for t in (F // 2, F // 2 + 1) if 1 <= t < F],
            "at_frame_1": [1] if F > 2 else [], "at_last": [F - 1] if F > 2 else []}


# name: (frames, run starts, entries of the chunk table at one pair per chunk).  A keyframe every second frame makes pair 2 j a coded
# entry and pair 2 j + 1 a skip entry: 2 k + 1 frames give 2 k entries, one more frame one more coded entry.
TABLE_PATTERNS = {
    "table255": (256, list(range(2, 256, 2)), 255),
    "table256": (257, list(range(2, 257, 2)), 256),
    "table257": (258, list(range(2, 258, 2)), 257),
}


def skip_bytes(nframes, run_starts):
    s = np.zeros(nframes - 1, np.uint8)
    s[skipped_pairs(nframes, run_starts)] = 1
    return s


# ------------------------------------------------------------------ tickets: the grid of the fused finish
# name: (W, H, frames, chunks knob, nwg claimed).  nwg = ceil(W H / 1024 / 4) * chunks; `wide`: a chunk of more than 64 pairs.
Ticket = collections.namedtuple("Ticket", "W H frames chunks nwg wide")
TICKETS = [
    Ticket(64, 32, 3, 1, 1, False),
    Ticket(64, 32, 5, 2, 2, False),
    Ticket(64, 128, 67, 1, 2, True),                              # two workgroups, one chunk of 66 pairs
    Ticket(192, 192, 8, 7, 63, False),
    Ticket(336, 256, 196, 3, 63, True),                           # 21 workgroups x 3 chunks of 65 pairs
    Ticket(256, 256, 5, 4, 64, False),
    Ticket(208, 256, 6, 5, 65, False),
    Ticket(1016, 512, 3, 1, 127, False),
    Ticket(512, 256, 5, 4, 128, False),
    Ticket(344, 512, 4, 3, 129, False),
    Ticket(1024, 1024, 5, 4, 1024, False),
]
TICKET_IDS = ["%dx%dx%d_c%d_nwg%d%s" % (t.W, t.H, t.frames, t.chunks, t.nwg, "_wide" if t.wide else "") for t in TICKETS]
SEQUENCE = [4, 0, 6]                                              # TICKETS of the back-to-back rounds on one context: nwg 63, 1, 65


def ticket_groups(nwg):
    """(workgroups on each first-level counter, first-level counters in use): what `mine` and `groups` of the fused tail must come to."""
    mine = [(nwg + MASK_TICKETS - 1 - i) // MASK_TICKETS for i in range(MASK_TICKETS)]
    return mine, min(nwg, MASK_TICKETS)


def ticket_clip(t, seed=0):
    """Planar 8-bit frames (F, n, 1) of a ticket shape: pair i changes a share of the pixels that cycles through coded, static,
    passthrough (>= P_STAR) and sparse."""
    n = t.W * t.H
    rng = np.random.default_rng(1000 + seed + t.nwg + t.frames)
    dens = [0.0889, 0.0, 0.4, 0.02, 0.2, 0.00005]
    fr = np.empty((t.frames, n), np.uint8)
    fr[0] = rng.integers(0, 256, n, dtype=np.uint8)
    for i in range(t.frames - 1):
        fr[i + 1] = fr[i] ^ (rng.random(n) < dens[i % len(dens)]).astype(np.uint8)
    return fr.reshape(t.frames, n, 1)


# ------------------------------------------------------------------ handoff and layouts
HANDOFF_SIZES = [(33, 31), (32, 32), (41, 25), (1087, 1), (64, 17), (1089, 1), (3071, 1), (5185, 1)]
# how a clip lies in memory: bytes in front of frame 0, bytes between frames, bytes behind a row, pixel stride (0 = the pixel's own bytes),
# bytes a mask row is longer than ceil(n / 64) * 8
Placement = collections.namedtuple("Placement", "base frame_pad row_pad pixel_stride mask_extra")


def placements(kernel):
    sb = kernel.sample_bytes
    odd = [2, 4] if kernel.pixel_bytes == 1 else [4, 8] if kernel.pixel_bytes == 2 else []
    out = [Placement(0, 0, 0, 0, 0), Placement(sb, 0, 0, 0, 8), Placement(8, 0, 0, 0, 24), Placement(0, sb, 0, 0, 0), Placement(0, 16, 0, 0, 8),
           Placement(0, 0, 2 * sb, 0, 0), Placement(0, 0, 16, 0, 24), Placement(8, 16, 16, 0, 8), Placement(16, 16, 0, 0, 24)]
    out += [Placement(0, 0, 0, ps, 0) for ps in odd] + [Placement(sb, sb, 2 * sb, ps, 8) for ps in odd]
    return out


def takes_fast_path(kernel, pl, n, pairs):
    """residual_mask_impl's choice (csrc/rbf_api.hip), for the frame's whole segments: flat rows, a pixel stride a fast instantiation
    knows, frames 16-byte aligned and 16-byte apart, the pair counters within 48 KiB of LDS."""
    ps = pl.pixel_stride or kernel.pixel_bytes
    return (pl.row_pad == 0 and ps == kernel.pixel_bytes and pl.base % 16 == 0 and pairs * 4 <= 48 * 1024 and n >= SEG and
            (n * ps + pl.frame_pad) % 16 == 0)


def place(samples, W, H, pl, seed=5):
    """samples (F, n, C) -> (raw bytes of the whole block incl. pl.base, frame stride, row pitch, pixel stride).  Every byte that is not
    a sample of the clip is random and differs from frame to frame: a kernel that reads one takes it for a change."""
    F, n, C = samples.shape
    sb = samples.dtype.itemsize
    px = C * sb
    ps = pl.pixel_stride or px
    pitch = W * ps + pl.row_pad
    fstride = H * pitch + pl.frame_pad
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, pl.base + F * fstride, dtype=np.uint8)
    body = samples.reshape(F, H, W, C).view(np.uint8).reshape(F, H, W, px)
    for f in range(F):
        fr = raw[pl.base + f * fstride:pl.base + f * fstride + H * pitch].reshape(H, pitch)
        fr[:, :W * ps].reshape(H, W, ps)[:, :, :px] = body[f]
    return raw, fstride, pitch, ps


def handoff_clip(kernel, n, frames=4, seed=11):
    """Random frames (F, n, C) in which about a third of the pixels change per pair, a few by 0x8000 alone (16-bit)."""
    rng = np.random.default_rng(seed + n + kernel.pixel_bytes)
    C, dt = samples_per_pixel(kernel), dtype_of(kernel.sample_bytes)
    fr = np.empty((frames, n, C), dt)
    fr[0] = rng.integers(0, 1 << (8 * kernel.sample_bytes), (n, C))
    for f in range(1, frames):
        fr[f] = fr[f - 1]
        ch = rng.random((n, C)) < 0.12
        fr[f][ch] ^= rng.integers(1, 8, (n, C)).astype(dt)[ch]
        if kernel.sample_bytes == 2:
            fr[f][rng.random((n, C)) < 0.03] ^= 0x8000
    return fr


# ------------------------------------------------------------------ blocks between guards
class Block:
    """`nrows` rows of `stride` bytes behind a base of 0 or 8 bytes, between two poisoned guards, as tests/bloom_rows.py lays its roles out;
    here the rows are poisoned as well, and untouched(raw, used) holds everything outside the first `used` bytes of each row."""

    def __init__(self, nrows, stride, base=0):
        self.nrows, self.stride, self.base = int(nrows), int(stride), int(base)
        self.first = GUARD + self.base
        self.nbytes = self.first + self.nrows * self.stride + GUARD

    def image(self):
        return np.full(self.nbytes, POISON, np.uint8)

    def place(self, buf):
        buf.upload(self.image())
        return buf.ptr + self.first

    def rows(self, raw):
        return raw[self.first:self.first + self.nrows * self.stride].reshape(self.nrows, self.stride)

    def untouched(self, raw, used):
        assert raw.nbytes == self.nbytes
        return bool((raw[:self.first] == POISON).all() and (raw[self.first + self.nrows * self.stride:] == POISON).all() and
                    (self.rows(raw)[:, used:] == POISON).all())


# ------------------------------------------------------------------ chunks, as the planner's table gives them
def uniform_chunks(pairs, ppc):
    """[(first pair, pairs, skipped)] of a table with count == 0."""
    return [(f0, min(ppc, pairs - f0), False) for f0 in range(0, pairs, ppc)]


# ------------------------------------------------------------------ wrong rules a kernel could have
def _luma_ad(prev, curr, exact=False):
    a, b = prev.astype(np.int64), curr.astype(np.int64)
    if exact:
        return np.abs(a - b)
    d = (a - b) % 65536
    d = np.where(d >= 32768, d - 65536, d)
    ad = np.where(d < 0, -d, d)
    return np.where(ad >= 32768, ad - 65536, ad)


def _bytes_of(fr):
    return np.ascontiguousarray(fr).view(np.uint8).reshape(fr.shape[0], -1)


def mutant_masks(name, frames, kernel, thr, run_starts=None, chunks=None):
    """ref_masks under the wrong rule `name` (a key of MUTANTS).  chunks: [(first pair, pairs, skipped)], what the chunk and tally rules
    refer to."""
    frames = np.asarray(frames)
    F, n = frames.shape[0], frames.shape[1]
    mc, sb, px = kernel.mask_channels, kernel.sample_bytes, kernel.pixel_bytes
    thrs = [int(thr)] * (F - 1) if np.isscalar(thr) else [int(t) for t in thr]
    skip = set(skipped_pairs(F, run_starts))
    if name == "skipped_pair_diffed":
        skip = set()
    rows, ones = np.zeros((F - 1, packed_stride(n)), np.uint8), np.zeros(F - 1, np.int64)
    for f in range(F - 1):
        if f in skip:
            continue
        prev, curr = frames[f], frames[f + 1]
        if name.startswith("byte_"):
            k = int(name.split("_")[1])
            pb, cb = _bytes_of(prev), _bytes_of(curr)
            if k >= px:
                bits = pair_bits(prev, curr, thrs[f], mc)
            elif mc >= 2 or k < sb:                               # a byte the rule reads: left out
                cb = cb.copy()
                cb[:, k] = pb[:, k]
                bits = pair_bits(prev, cb.view(prev.dtype).reshape(prev.shape), thrs[f], mc)
            else:                                                 # a byte the luma rule does not read: taken in
                bits = pair_bits(prev, curr, thrs[f], mc) | (pb[:, k] != cb[:, k])
        elif name == "exact_for_int16" and mc == 1:
            bits = _luma_ad(prev[:, 0], curr[:, 0], exact=True) > thrs[f]
        elif name == "int16_for_exact" and mc >= 2:
            bits = (_luma_ad(prev[:, :mc], curr[:, :mc]) > 0).any(-1)
        elif name == "ge_for_gt" and mc == 1:
            bits = _luma_ad(prev[:, 0], curr[:, 0]) >= thrs[f]
        else:
            bits = pair_bits(prev, curr, thrs[f], mc)
        rows[f, :(n + 7) // 8] = np.packbits(bits, bitorder="little" if name == "lsb_first" else "big")
        ones[f] = int(bits.sum())
    return chunk_mutant(name, rows, ones, chunks)


def chunk_mutant(name, rows, true_ones, chunks):
    """The chunk and tally rules on the true rows (nullable) and counts of a clip; chunks: [(first pair, pairs, skipped)]."""
    true_ones = np.asarray(true_ones, np.int64)
    ones = true_ones.copy()
    rows = None if rows is None else rows.copy()
    for f0, cnt, skipped in chunks or ():
        if skipped:
            continue
        if name == "chunk_first_pair_dropped" and f0 > 0:         # (chunk 0's first pair is every kernel's first pair: no edge)
            ones[f0] = 0
            if rows is not None:
                rows[f0] = 0
        if name == "chunk_first_pair_twice" and f0 > 0:
            ones[f0] = 2 * true_ones[f0]
        if name == "tally_halves_swapped":
            for s in range(cnt // 2):
                ones[f0 + 2 * s], ones[f0 + 2 * s + 1] = true_ones[f0 + 2 * s + 1], true_ones[f0 + 2 * s]
        if name == "tally_not_flushed" and cnt > 128:             # the lane slots are written again: the later pair's count lands on the earlier
            for j in range(cnt):
                ones[f0 + j] = true_ones[f0 + list(range(j, cnt, 128))[-1]] if j < 128 else 0
    return rows, ones


BIT_MUTANTS = ["lsb_first", "exact_for_int16", "int16_for_exact", "ge_for_gt"] + ["byte_%d_wrong" % k for k in range(8)]
CHUNK_MUTANTS = ["chunk_first_pair_dropped", "chunk_first_pair_twice", "tally_halves_swapped", "tally_not_flushed", "skipped_pair_diffed"]
MUTANTS = BIT_MUTANTS + CHUNK_MUTANTS


def mutant_applies(name, kernel):
    if name.startswith("byte_"):
        return int(name.split("_")[1]) < kernel.pixel_bytes
    if name == "ge_for_gt":
        return kernel.mask_channels == 1
    if name == "exact_for_int16":
        return kernel.mask_channels == 1 and kernel.sample_bytes == 2      # (8-bit differences stay within int16: the two rules are one)
    if name == "int16_for_exact":
        return kernel.mask_channels >= 2 and kernel.sample_bytes == 2      # (8-bit samples never reach 0x8000: the two rules are one)
    return True
