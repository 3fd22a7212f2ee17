"""Case tables, input builders and plain references of tests/test_gpu_value_key_sweep.py (the gather / scatter kernels, the batch gather, the
per-index and the string-key filter surface).  numpy only; the filter references take the C oracle (the `oracle` fixture's module) as an
argument.  Nothing here imports the HIP library; tests/test_value_key_ref_cpu.py proves on the CPU that these inputs are not vacuous.

Layout rules of every case (the GPU file applies them): a buffer the device writes is pre-filled with SENTINEL and carries at least SLACK
bytes behind its last legal byte; mask rows sit packed_stride(n) + ROW_GAP bytes apart with GAP_BYTE in between (a wrong row stride reads set
bits); the pad bits of a row's last word are zero, as the ABI asks."""
import math
from collections import namedtuple

import numpy as np

SENTINEL, SLACK = 0xEE, 64
ROW_GAP, GAP_BYTE = 64, 0xFF
SEG = 1024                                     # pixels of one segment of the mask scan
SCAN_ROUND = 1024                              # segments one round of the scan covers
H, W = 131, 67                                 # n = 8777: 9 segments, a ragged last word, a ragged last segment
BIG_H, BIG_W = 1031, 1021                      # n = 1 052 651: 1028 segments, so the scan carries into a second round
SMALL_H, SMALL_W, SMALL_F = 7, 9, 301          # 300 pairs of 63 pixels

U32_MAX = (1 << 32) - 1


def packed_stride(nbits):
    """Bytes of a packed row of nbits: whole 64-bit words (restated here so that this module needs nothing of the package)."""
    return (int(nbits) + 63) // 64 * 8


def segments(n):
    return (n + SEG - 1) // SEG


# ------------------------------------------------------------------ frames inside padded byte buffers
class Layout(namedtuple("Layout", "kind dtype C H W pixel_stride row_pitch")):
    @property
    def sb(self):
        return np.dtype(self.dtype).itemsize

    @property
    def n(self):
        return self.H * self.W

    @property
    def nbytes(self):
        return self.H * self.row_pitch

    @property
    def flat(self):
        return self.row_pitch == self.W * self.pixel_stride


LAYOUT_KINDS = ("flat", "rows", "pixels")


def layout(kind, dtype, C, h=H, w=W):
    """flat | rows: six bytes behind every row | pixels: one unused sample behind every pixel's channels, and the six bytes."""
    sb = np.dtype(dtype).itemsize
    ps = (C + 1) * sb if kind == "pixels" else C * sb
    return Layout(kind, np.dtype(dtype), C, h, w, ps, w * ps + (0 if kind == "flat" else 6))


VALUE_CASES = [(dt, C, kind) for dt in (np.uint8, np.uint16) for C in (1, 2, 3, 4) for kind in LAYOUT_KINDS]
VALUE_IDS = ["u%dc%d-%s" % (8 * np.dtype(dt).itemsize, C, kind) for dt, C, kind in VALUE_CASES]
BATCH_CASES = [(dt, C, kind) for dt, C, kind in VALUE_CASES if kind != "pixels"]
BATCH_IDS = ["u%dc%d-%s" % (8 * np.dtype(dt).itemsize, C, kind) for dt, C, kind in BATCH_CASES]
CAPACITY_CASE = (np.uint8, 3, "rows")


def samples(buf, lay, base=0):
    """The (H, W, C) samples of the frame that starts at byte `base` of buf: a view, so writing through it writes the buffer."""
    body = buf[base:base + lay.nbytes].view(lay.dtype)
    return np.lib.stride_tricks.as_strided(body, (lay.H, lay.W, lay.C), (lay.row_pitch, lay.pixel_stride, lay.sb))


def frame_bytes(lay, seed):
    """A frame buffer whose every byte is random: row padding and the samples past `channels` hold data too."""
    return np.random.default_rng(seed).integers(0, 256, lay.nbytes, dtype=np.uint8)


def sample_byte_map(lay):
    """True at the bytes of the buffer that belong to a pixel's first C samples."""
    m = np.zeros(lay.nbytes, dtype=bool)
    pixel_bytes(m, lay)[...] = True
    return m


def pixel_bytes(arr, lay):
    """(H, W, C * sample bytes) view of a one-byte-per-byte array of the frame buffer's length: the bytes of every pixel's first C samples."""
    assert arr.itemsize == 1 and len(arr) == lay.nbytes
    return np.lib.stride_tricks.as_strided(arr, (lay.H, lay.W, lay.C * lay.sb), (lay.row_pitch, lay.pixel_stride, 1))


MASK_NAMES = ("empty", "full", "first", "last", "p07", "p90", "seg3_empty_seg4_full")


def mask_set(n, seed):
    """The masks of MASK_NAMES as bool vectors of n pixels."""
    rng = np.random.default_rng(seed)
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[n - 1] = True, True
    segs = rng.random(n) < 0.07
    segs[3 * SEG:4 * SEG] = False
    segs[4 * SEG:5 * SEG] = True
    return dict(zip(MASK_NAMES, (np.zeros(n, bool), np.ones(n, bool), first, last, rng.random(n) < 0.07, rng.random(n) < 0.90, segs)))


def big_masks(n, seed):
    rng = np.random.default_rng(seed)
    return {"p07": rng.random(n) < 0.07, "full": np.ones(n, bool)}


def mask_block(masks, n):
    """(bytes, row stride): the packed rows as the device reads them, GAP_BYTE between and behind them."""
    stride = packed_stride(n) + ROW_GAP
    blk = np.full(len(masks) * stride, GAP_BYTE, dtype=np.uint8)
    for r, m in enumerate(masks):
        assert len(m) == n
        row = np.zeros(packed_stride(n), dtype=np.uint8)
        pk = np.packbits(np.asarray(m, dtype=np.uint8))
        row[:len(pk)] = pk
        blk[r * stride:r * stride + len(row)] = row
    return blk, stride


def gather_ref(buf, lay, mask, base=0):
    """frame[mask] in raster order: count * C samples."""
    return np.ascontiguousarray(samples(buf, lay, base)[np.asarray(mask, bool).reshape(lay.H, lay.W)]).reshape(-1)


def scatter_values(buf, lay, mask, seed):
    """Random values for the masked pixels that differ from the frame's at every sample."""
    have = gather_ref(buf, lay, mask)
    vals = np.random.default_rng(seed).integers(0, 1 << (8 * lay.sb), have.shape, dtype=np.uint64).astype(lay.dtype)
    vals[vals == have] += lay.dtype.type(1)
    return vals


def scatter_ref(buf, lay, mask, values):
    """A copy of the whole byte buffer with the masked pixels' first C samples replaced."""
    out = buf.copy()
    samples(out, lay)[np.asarray(mask, bool).reshape(lay.H, lay.W)] = values.reshape(-1, lay.C)
    return out


# ------------------------------------------------------------------ the batch gather
Clip = namedtuple("Clip", "lay F frame_stride block masks")
BatchRef = namedtuple("BatchRef", "values offsets uncovered")
CHROMA_PIXELS = 40


def make_clip(lay, F, masks, seed, frame_gap=0):
    rng = np.random.default_rng(seed)
    stride = lay.nbytes + frame_gap
    return Clip(lay, F, stride, rng.integers(0, 256, F * stride, dtype=np.uint8), masks)


def sweep_clip(dtype, C, kind, seed=4100):
    """Five frames of 131x67: pairs 0..2 between random frames under the masks 7 % | empty | full; frame 4 is frame 3 with sample 0 changed
    at about a tenth of the pixels -- pair 3's mask is exactly that difference -- and with the LAST channel changed at 40 further pixels,
    which the mask therefore misses (for C = 1 the last channel is sample 0 itself: still 40 changed pixels outside the mask).  Row
    padding, the gap between padded frames and the samples past `channels` are random in every frame."""
    lay = layout(kind, dtype, C)
    rng = np.random.default_rng(seed + 10 * C + lay.sb)
    clip = make_clip(lay, 5, None, seed + 1000 + 10 * C + lay.sb, frame_gap=0 if lay.flat else 16)
    s3, s4 = samples(clip.block, lay, 3 * clip.frame_stride), samples(clip.block, lay, 4 * clip.frame_stride)
    s4[...] = s3
    luma = rng.random((lay.H, lay.W)) < 0.10
    chroma = np.zeros(lay.n, bool)
    chroma[rng.choice(np.flatnonzero(~luma.reshape(-1)), CHROMA_PIXELS, replace=False)] = True
    s4[luma, 0] += lay.dtype.type(1)
    s4[chroma.reshape(lay.H, lay.W), C - 1] += lay.dtype.type(1)
    masks = [rng.random(lay.n) < 0.07, np.zeros(lay.n, bool), np.ones(lay.n, bool), luma.reshape(-1).copy()]
    return clip._replace(masks=masks)


def small_clip(seed=4300):
    """301 frames of 9x7, u8, C = 2: random frames, random masks of mixed density, every seventh one empty."""
    lay = layout("flat", np.uint8, 2, SMALL_H, SMALL_W)
    rng = np.random.default_rng(seed)
    masks = [np.zeros(lay.n, bool) if f % 7 == 3 else rng.random(lay.n) < rng.choice([0.05, 0.5, 0.95]) for f in range(SMALL_F - 1)]
    return make_clip(lay, SMALL_F, masks, seed + 1)


def big_clip(seed=4400):
    lay = layout("flat", np.uint8, 1, BIG_H, BIG_W)
    return make_clip(lay, 3, list(big_masks(lay.n, seed).values()), seed + 1)


def batch_ref(clip):
    """Per-pair gathers from frame f + 1, concatenated | exclusive scan of the counts with the total appended | per pair, the pixels that
    differ in some channel and are not in the mask."""
    lay, vals, counts, unc = clip.lay, [], [], []
    for f, mask in enumerate(clip.masks):
        a, b = samples(clip.block, lay, f * clip.frame_stride), samples(clip.block, lay, (f + 1) * clip.frame_stride)
        m2 = np.asarray(mask, bool).reshape(lay.H, lay.W)
        vals.append(gather_ref(clip.block, lay, mask, (f + 1) * clip.frame_stride))
        counts.append(int(m2.sum()))
        unc.append(int(((a != b).any(-1) & ~m2).sum()))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return BatchRef(np.concatenate(vals), offsets, np.array(unc, dtype=np.uint64))


def capacities(offsets):
    """The capacity cuts of the issue, in pixels, by name.  Pair 1 of the sweep clip is empty, so offsets[1] == offsets[2] is a boundary
    that two pairs share; pair 2 is the full mask."""
    off = [int(o) for o in offsets]
    total = off[-1]
    return {"zero": 0, "one": 1, "total": total, "total-1": total - 1, "boundary": off[1], "boundary+1": off[1] + 1,
            "mid-pair-2": (off[2] + off[3]) // 2, "end-of-pair-2": off[3]}


# ------------------------------------------------------------------ filters: shared pieces
SEEDS_VIDEO = (0x12345678, 0x87654321, 999)
SEEDS_WIDE = (1 << 32, (1 << 64) - 1, (1 << 63) + 5)
INDEX_SEEDS = (SEEDS_VIDEO, SEEDS_WIDE)
KEY_SEEDS = ((0, 1, 3), SEEDS_VIDEO, ((1 << 32) - 1, 1 << 32, (1 << 64) - 1))


def filter_bytes(m):
    """Legal bytes of an m-bit filter on the device: whole 32-bit words."""
    return (int(m) + 31) // 32 * 4


def pack_filter(bits):
    """Byte-per-bit oracle filter -> the device's bytes (numpy.packbits order, zero-padded to whole 32-bit words)."""
    out = np.zeros(filter_bytes(len(bits)), dtype=np.uint8)
    pk = np.packbits(np.asarray(bits, dtype=np.uint8))
    out[:len(pk)] = pk
    return out


def set_positions(packed):
    """Sorted positions of the set bits of a packed filter (cheap on a large, almost empty one)."""
    packed = np.asarray(packed, dtype=np.uint8)
    body = len(packed) // 8 * 8
    words = np.flatnonzero(packed[:body].view(np.uint64))
    at = np.concatenate([(words[:, None] * 8 + np.arange(8)).reshape(-1), np.arange(body, len(packed))]).astype(np.int64)
    at = at[packed[at] != 0]
    bits = np.unpackbits(packed[at]).reshape(-1, 8)
    return (at[:, None] * 8 + np.arange(8))[bits == 1]


def index_positions(orc, i, m, k_star, seeds):
    """The probe positions of index i, from the oracle's primitives (for filters too long for a byte-per-bit array)."""
    fk, pa = math.floor(k_star), k_star - math.floor(k_star)
    h1, h2 = orc.hash_index(i, seeds[0]), orc.hash_index(i, seeds[1])
    cnt = fk + (1 if orc.normalize(orc.hash_index(i, seeds[2])) < pa else 0)
    return [orc.position(h1, h2, j, m) for j in range(cnt)]


# ------------------------------------------------------------------ C: the per-index surface
LONG_N = 8192 * 256 + 77                       # one more than the 8192 workgroups of 256 threads cover in one trip
LONG_M, LONG_K, LONG_DENSITY = 1500007, 2.3, 0.2
LONG_DUPLICATES, LONG_EXTRA = 1000, 64
GRID_LIMIT = 8192 * 256

SHORT_M = (1, 2, 31, 32, 33, 63, 64, 65, 1000003, 1 << 30, (1 << 30) + 1)
SHORT_K = (0.5, 1.0, 2.3, 64.0, 64.5)
BYTE_PER_BIT_MAX = 1 << 24                     # longer filters are compared by set positions

LongCase = namedtuple("LongCase", "mask insert query filt verdicts extra filt_or verdicts_or")
_cache = {}


def long_case(orc):
    """The long list: a mask of LONG_N positions; `insert` = its set positions shuffled, with 1000 duplicates; `query` = a shuffled
    permutation of all positions; the oracle's filter (orc_compress) and its verdict for every position (orc_decompress with an all-ones
    witness), once as built and once with LONG_EXTRA bits OR-ed in that the insert does not set."""
    if "long" not in _cache:
        rng = np.random.default_rng(5100)
        mask = (rng.random(LONG_N) < LONG_DENSITY).astype(np.uint8)
        ones = np.flatnonzero(mask).astype(np.uint32)
        insert = np.concatenate([rng.permutation(ones), rng.choice(ones, LONG_DUPLICATES)]).astype(np.uint32)
        query = rng.permutation(LONG_N).astype(np.uint32)
        filt, scratch = np.zeros(LONG_M, dtype=np.uint8), np.zeros(LONG_N, dtype=np.uint8)
        orc.lib().orc_compress(orc._ptr(mask), LONG_N, LONG_M, LONG_K, orc._seeds(SEEDS_VIDEO), orc._ptr(filt), orc._ptr(scratch))
        extra = np.sort(rng.choice(np.flatnonzero(filt == 0), LONG_EXTRA, replace=False))
        filt_or = filt.copy()
        filt_or[extra] = 1
        witness = np.ones(LONG_N, dtype=np.uint8)
        verdicts = orc.decompress(filt, witness, LONG_N, LONG_K, SEEDS_VIDEO)
        verdicts_or = orc.decompress(filt_or, witness, LONG_N, LONG_K, SEEDS_VIDEO)
        _cache["long"] = LongCase(mask, insert, query, filt, verdicts, extra, filt_or, verdicts_or)
    return _cache["long"]


DIGIT_EDGES = [v for p in range(1, 10) for v in (10 ** p - 1, 10 ** p)]      # both sides of every change of the key length


def short_lists(seed=5200):
    """Index lists by name.  One index cannot be both 0 and 2^32 - 1, so count 1 comes twice; the longer lists hold both, every change of
    the decimal key's length, and random 32-bit indices."""
    rng = np.random.default_rng(seed)
    lists = {"1-zero": np.array([0], np.uint32), "1-max": np.array([U32_MAX], np.uint32)}
    for count in (255, 256, 257):
        rest = rng.integers(0, 1 << 32, count - 2 - len(DIGIT_EDGES), dtype=np.uint64)
        fixed = np.array([0, U32_MAX] + DIGIT_EDGES, dtype=np.uint64)
        lists[str(count)] = rng.permutation(np.concatenate([fixed, rest])).astype(np.uint32)
    return lists


def short_queries(lst, seed=5300):
    """The list itself and 300 indices that are (almost surely) not in it, neighbours of its members included, shuffled."""
    rng = np.random.default_rng(seed + len(lst))
    near = (lst[:50].astype(np.uint64) + 1) % (1 << 32)
    return rng.permutation(np.concatenate([lst.astype(np.uint64), near, rng.integers(0, 1 << 32, 300 - len(near), dtype=np.uint64)])).astype(np.uint32)


def short_ref(orc, m, k_star, seeds, lst, queries):
    """(packed filter, verdicts) of the oracle's add_index / check_index; m <= BYTE_PER_BIT_MAX."""
    f = orc.RationalFilter(m, k_star, seeds)
    for i in lst:
        f.add_index(int(i))
    return pack_filter(f.bit_array), np.array([f.check_index(int(i)) for i in queries], dtype=np.uint8)


def short_ref_positions(orc, m, k_star, seeds, lst, queries):
    """(sorted set positions, verdicts) for a filter too long for a byte-per-bit array."""
    want = set()
    for i in lst:
        want.update(index_positions(orc, int(i), m, k_star, seeds))
    verdicts = np.array([all(p in want for p in index_positions(orc, int(i), m, k_star, seeds)) for i in queries], dtype=np.uint8)
    return np.array(sorted(want), dtype=np.int64), verdicts


# ------------------------------------------------------------------ D: the string-key surface
KEY_LENGTHS = range(0, 132)                    # four full 32-byte stripes and every mix of the 8-, 4- and 1-byte tails
KEYS_PER_LENGTH = 3
KEY_K, KEY_M = 2.5, (2003, 1000003, 16777259)  # 2003: the filter at which three keys per length fill 20..60 %
KEY_M_LARGE = 16777259
STANDARD_K = (1, 2, 7, 64)
BLOB_TAIL, TAIL_BYTE = 64, 0xA5


def _keys_of_lengths(lengths, rng):
    keys = []
    for n in lengths:
        for j in range(KEYS_PER_LENGTH):
            b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            if n and j < 2:
                b[0], b[-1] = (0x00, 0xFF) if j == 0 else (0xFF, 0x00)
                if n == 1:
                    b[0] = 0x00 if j == 0 else 0xFF
            keys.append(bytes(b))
    return keys


def key_sets(seed=5400):
    """(inserted, others): three keys of every length 0..131 in a shuffled order that keeps an empty key away from both ends, and as many
    keys that are not inserted (lengths 4..135: the shortest keys are too few to find fresh ones among them)."""
    rng = np.random.default_rng(seed)
    keys = _keys_of_lengths(KEY_LENGTHS, rng)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    for end in (0, len(keys) - 1):
        if len(keys[end]) == 0:
            swap = next(i for i in range(1, len(keys) - 1) if len(keys[i]))
            keys[end], keys[swap] = keys[swap], keys[end]
    have = set(keys)
    others = [k for k in _keys_of_lengths([n if n >= 4 else 132 + n for n in KEY_LENGTHS], rng) if k not in have]
    return keys, others


def key_queries(keys, others, seed=5500):
    """Every inserted key and every other one, shuffled: (keys, inserted flag of each)."""
    rng = np.random.default_rng(seed)
    allk = keys + others
    order = rng.permutation(len(allk))
    return [allk[i] for i in order], np.array([i < len(keys) for i in order])


def key_blob(keys):
    """(bytes, offsets): the keys back to back, a run of TAIL_BYTE behind the last one; offsets has len(keys) + 1 entries."""
    offsets = np.zeros(len(keys) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(k) for k in keys])
    blob = np.frombuffer(b"".join(keys) + bytes([TAIL_BYTE]) * BLOB_TAIL, dtype=np.uint8).copy()
    return blob, offsets


def decimal_blob(indices):
    """key_blob of str(i) for every index, without a Python loop over the keys."""
    v = np.asarray(indices, dtype=np.uint64).copy()
    lens = np.ones(len(v), dtype=np.int64)
    for p in range(1, 20):
        lens += v >= np.uint64(10 ** p)
    offsets = np.zeros(len(v) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(lens)
    blob = np.full(int(offsets[-1]) + BLOB_TAIL, TAIL_BYTE, dtype=np.uint8)
    ends = offsets[1:].astype(np.int64)
    for d in range(1, int(lens.max()) + 1):
        sel = lens >= d
        blob[ends[sel] - d] = (48 + v[sel] % np.uint64(10)).astype(np.uint8)
        v //= np.uint64(10)
    return blob, offsets


def rational_key_ref(orc, m, k_star, seeds, keys, queries):
    """(byte-per-bit filter, verdicts) of orc_add_key / orc_check_key; ctypes passes the length, so zero bytes are part of the key."""
    L, bits, sd = orc.lib(), np.zeros(m, dtype=np.uint8), orc._seeds(seeds)
    for k in keys:
        L.orc_add_key(orc._ptr(bits), m, k_star, sd, k, len(k))
    return bits, np.array([L.orc_check_key(orc._ptr(bits), m, k_star, sd, k, len(k)) for k in queries], dtype=np.uint8)


def standard_key_ref(orc, m, k, keys, queries):
    L, bits = orc.lib(), np.zeros(m, dtype=np.uint8)
    for key in keys:
        L.orc_std_add_key(orc._ptr(bits), m, k, key, len(key))
    return bits, np.array([L.orc_std_check_key(orc._ptr(bits), m, k, key, len(key)) for key in queries], dtype=np.uint8)
