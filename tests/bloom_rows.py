"""Where the Bloom row sweep (tests/test_gpu_bloom_row_sweep.py) puts the rows of rbf_bloom_encode_batch, rbf_bloom_decode_batch,
rbf_pack_records and the output side of rbf_encode_runs, and what it expects in them -- a helper, not a test.  Plain numpy / ctypes; the
device is only touched through the buffers a caller hands in.

  batches   six masks per frame size (DENSITIES: two filters in the FP64 range, two below it, one frame the reference passes through,
            one more in the range) and what the C oracle makes of them: mask -> optimal_params -> filter, witness, counts.  Computed once
            per process (batch), whatever layout or knob the device then runs.
  layouts   LAYOUTS: per role (mask rows, filter rows, witness rows, stats, ones, the record) a stride kind and a base, chosen so that every
            role sees every value and every ordered pair of roles sees (plain, odd).  Block lays a role out as GUARD | rows | GUARD.
  mutants   MUTANTS: the row-address rules a kernel could have by mistake.  tests/test_bloom_rows_cpu.py shows that each of them fetches
            other bytes than the true rule wherever it forms another address.
  kernels   KERNELS: what the launch planner decides for (knob, batch), in the `decision` notation of tests/c/plan_cases.cpp; the CPU test
            holds the table against the planner itself.
"""
import collections
import ctypes

import numpy as np

from new_bloom_filter_repo_amd import params as P
from plan_boundaries import random_mask

POISON = 0xA5
GUARD = 512                                                       # a multiple of 16: `base` alone decides a block's alignment
MAX_BATCH = 128                                                   # csrc/rbf_geometry.h: frames of one launch sequence
SIZES = [(512, 256), (509, 257)]                                  # n = 131072: whole segments | n = 130813: n % 64 = 61
SIZE_IDS = ["512x256", "509x257"]
DENSITIES = (0.0889, 0.2, 0.05, 0.01, 0.4, 0.0889)                # 0.4 >= P_STAR: m = 0
PASSTHROUGH = 4
MANY = (799, 11, 130)                                             # more than MAX_BATCH rows: the second chunk starts at row 128
F64_MIN = 1 << 15                                                 # csrc/rbf_geometry.h F64MOD_M_MIN: smaller filters take the Barrett kernels
STATS = 4                                                         # RBF_STATS_PER_FRAME

# rbf_ctx_force_generic arguments of the sweep, and what the planner makes of the two six-frame batches under each (both sizes alike):
# (the batch is split over the two families, decision of the undivided batch or of its Barrett half, decision of its FP64 half), a
# decision being fast_insert.query.double_buffer.insert_tab.two_phase.probe_image.insert_tiles.query_tiles with query 0 k_query, 1
# k_query_lds / k_query_u64 (probe_image), 2 k_query_tiled, 3 k_query_s64t.  `known`: the entry knows the masks' counts (rbf_encode_runs).
KNOBS = [0, 8, 2 | 8, 1, 16 << 16, 32 << 16, (32 << 16) | (1 << 14), (32 << 16) | 128]
KNOB_IDS = ["default", "barrett", "single_buffer", "generic", "tile16", "tile32", "tile32_hashed", "tile32_insert_tab"]
KERNELS = {
    0: (True, "1.1.1.0.0.0.1.1", "1.1.0.1.0.1.1.1"),              # k_insert_lds + k_query_lds x2 | k_insert_tab (whole) + k_query_u64
    8: (False, "1.1.1.0.0.0.1.1", None),                          # k_insert_lds + k_query_lds, two buffers
    2 | 8: (False, "1.1.0.0.0.0.1.1", None),                      # ... one buffer
    1: (False, "0.0.0.0.0.0.0.0", None),                          # k_insert + k_query in global memory
    16 << 16: (True, "1.2.0.0.0.0.1.1", "1.3.0.1.0.1.2.2"),       # k_insert_lds + k_query_tiled | k_insert_tab over two tiles + k_query_s64t
    32 << 16: (True, "1.2.0.0.0.0.1.1", "1.3.0.1.0.1.1.1"),       # ... | one tile
    (32 << 16) | (1 << 14): (True, "1.2.0.0.0.0.1.1", "1.3.0.1.0.1.1.1"),
    (32 << 16) | 128: (True, "1.2.0.0.0.0.1.1", "1.3.0.1.0.1.1.1"),
}
KERNELS_KNOWN = dict(KERNELS)
KERNELS_KNOWN[16 << 16] = (True, "1.2.0.0.0.0.1.1", "1.3.0.1.1.1.2.2")    # counts known: k_insert_positions + k_insert_records


def packed_stride(nbits):
    return (int(nbits) + 63) // 64 * 8


# ------------------------------------------------------------------ what the oracle makes of a mask
Frame = collections.namedtuple("Frame", "mask ones k m floor_k T filter filter_ones witness_bits witness")


def padded(bits):
    """numpy.packbits of a bit vector, zero-padded to whole 64-bit words."""
    row = np.zeros(packed_stride(len(bits)), np.uint8)
    pk = np.packbits(np.asarray(bits, np.uint8))
    row[:pk.size] = pk
    return row


def expect_frame(oracle, mask):
    """mask (uint8 [n] of 0 / 1) -> Frame: the reference's geometry (oracle.optimal_params, the passthrough rules of oracle.compress), the C
    oracle's filter and witness as the device packs them (zero-padded to 64-bit words), the integer parameters the C ABI takes."""
    mask = np.ascontiguousarray(mask, np.uint8)
    n, ones = len(mask), int(mask.sum())
    p = np.uint64(ones) / n
    k, l = oracle.optimal_params(n, p)
    none = np.zeros(0, np.uint8)
    if p >= oracle.P_STAR or l == 0 or l >= n:
        return Frame(mask, ones, 0.0, 0, 0, 0, none, 0, 0, none)
    bits, witness = np.zeros(l, np.uint8), np.zeros(n, np.uint8)
    vp = ctypes.c_void_p
    w = int(oracle.lib().orc_compress(vp(mask.ctypes.data), n, l, float(k), (ctypes.c_uint64 * 3)(*P.SEEDS_VIDEO), vp(bits.ctypes.data),
                                      vp(witness.ctypes.data)))
    floor_k, T = P.activation_threshold(k)
    return Frame(mask, ones, k, int(l), int(floor_k), int(T), padded(bits), int(bits.sum()), w, padded(witness[:w]))


_BATCHES = {}


def batch(oracle, W, H, count=len(DENSITIES)):
    """The `count` Frames of a W x H batch: densities cycle through DENSITIES, mask j from seed 100 W + j.  Cached: shared by every test."""
    key = (W, H, count)
    if key not in _BATCHES:
        _BATCHES[key] = [expect_frame(oracle, random_mask(100 * W + j, W * H, DENSITIES[j % len(DENSITIES)])) for j in range(count)]
    return _BATCHES[key]


def mask_row(fr):
    return padded(fr.mask)


def plist(frames):
    return [(fr.m, fr.floor_k, fr.T) for fr in frames]


def stats_rows(frames):
    out = np.zeros((len(frames), STATS), np.uint64)
    for f, fr in enumerate(frames):
        out[f, 0], out[f, 1] = fr.witness_bits, fr.filter_ones
    return out


def minimal_strides(frames):
    """(mask, filter, witness, tight witness): the strides BloomEngine itself uses -- encode takes packed_stride(n) for the witness rows,
    decode the `tight` one, max ceil(bits / 64) * 8, which is below ceil(n / 64) * 8."""
    n = len(frames[0].mask)
    return (packed_stride(n), max(packed_stride(fr.m) for fr in frames), packed_stride(n),
            max([packed_stride(fr.witness_bits) for fr in frames] + [8]))


def record_bytes(frames, skipped=()):
    """The record rbf_pack_records owes for a batch, byte for byte (include/rbf.h): k travels as given."""
    n, F = len(frames[0].mask), len(frames)
    head = np.zeros(4 + 8 * F, "<u8")
    head[0], head[1] = 0x3130434552464252, F
    off, payload = head.nbytes, []
    for f, fr in enumerate(frames):
        if f in skipped:                                          # a pair across a keyframe: a header row without payload
            first = wit = np.zeros(0, np.uint8)
            head[4 + 8 * f:12 + 8 * f] = [0, 0xFFFFFFFF, 0, 0, 0, 0, off, off]
        else:
            first, wit = fr.filter if fr.m else mask_row(fr), fr.witness
            head[4 + 8 * f:12 + 8 * f] = [fr.m, fr.floor_k, fr.T, np.float64(fr.k).view("<u8"), fr.witness_bits, fr.filter_ones, off, off + first.nbytes]
        payload += [first, wit]
        off += first.nbytes + wit.nbytes
    head[2] = off
    return np.concatenate([head.view(np.uint8)] + payload)


# ------------------------------------------------------------------ layouts
Rows = collections.namedtuple("Rows", "kind base")
Layout = collections.namedtuple("Layout", "name masks filters witnesses stats ones record")
STRIDE_KINDS = ("min", "plus8", "wide")
BASES = (0, 8)
ROW_ROLES = ("masks", "filters", "witnesses")
ROLES = ROW_ROLES + ("stats", "ones", "record")


def stride_of(kind, minimal):
    """min: the minimal stride | plus8: one word more, which flips the stride between 0 and 8 mod 16 | wide: rounded up to 16, then 4096 +
    16 more -- rows more than a page apart, every row 16-byte aligned when the base is."""
    return {"min": minimal, "plus8": minimal + 8, "wide": (minimal + 15) // 16 * 16 + 4096 + 16}[kind]


PLAIN = Rows("min", 0)
# Layout 0 is BloomEngine's own (the control).  Role r is odd -- a stride that is not minimal, or a base of 8 -- in three of the layouts
# 1..7, no two roles in the same three: for every ordered pair of roles one layout has the first plain and the second odd.
LAYOUTS = [
    Layout("engine", PLAIN, PLAIN, PLAIN, 0, 0, 0),
    Layout("m+8@8_s8_o8", Rows("plus8", 8), PLAIN, PLAIN, 8, 8, 0),
    Layout("f+8_wwide@8_o8", PLAIN, Rows("plus8", 0), Rows("wide", 8), 0, 8, 0),
    Layout("mwide_fwide@8_r8", Rows("wide", 0), Rows("wide", 8), PLAIN, 0, 0, 8),
    Layout("w+8_s8_r8", PLAIN, PLAIN, Rows("plus8", 0), 8, 0, 8),
    Layout("m@8_w@8", Rows("min", 8), PLAIN, Rows("min", 8), 0, 0, 0),
    Layout("f@8_s8", PLAIN, Rows("min", 8), PLAIN, 8, 0, 0),
    Layout("o8_r8", PLAIN, PLAIN, PLAIN, 0, 8, 8),
]
LAYOUT_IDS = [lay.name for lay in LAYOUTS]


def is_odd(lay, role):
    v = getattr(lay, role)
    return v != PLAIN if role in ROW_ROLES else v != 0


def decode_witness_kind(lay):
    """The witness rows a decode reads: where the layout leaves them minimal, the engine's own tight stride."""
    return "tight" if lay.witnesses.kind == "min" else lay.witnesses.kind


class Block:
    """`nrows` rows of `stride` bytes behind a base of 0 or 8 bytes, between two guards: GUARD | base | rows | GUARD.  A role's whole
    block, built on the host (image), uploaded, downloaded and taken apart again (row, guards)."""

    def __init__(self, nrows, stride, base=0, guard=GUARD):
        self.nrows, self.stride, self.base, self.guard = int(nrows), int(stride), int(base), int(guard)
        self.first = self.guard + self.base
        self.nbytes = self.first + self.nrows * self.stride + self.guard

    def offset(self, f):
        return self.first + f * self.stride

    def image(self, payloads=()):
        """The block as bytes: POISON everywhere, payloads[f] (at most a stride long) at the start of row f."""
        raw = np.full(self.nbytes, POISON, np.uint8)
        for f, p in enumerate(payloads):
            p = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
            assert f < self.nrows and p.nbytes <= self.stride
            raw[self.offset(f):self.offset(f) + p.nbytes] = p
        return raw

    def row(self, raw, f, nbytes=None):
        assert 0 <= f < self.nrows
        return raw[self.offset(f):self.offset(f) + (self.stride if nbytes is None else nbytes)]

    def guards(self, raw):
        assert raw.nbytes == self.nbytes
        return raw[:self.first], raw[self.first + self.nrows * self.stride:]

    def guards_are_poison(self, raw):
        return all((g == POISON).all() for g in self.guards(raw))

    # the device side: buf is a DeviceBuffer (or the CPU test's stand-in) of self.nbytes
    def place(self, buf, payloads=()):
        buf.upload(self.image(payloads))
        return buf.ptr + self.first

    def fetch(self, buf):
        return buf.download(self.nbytes)


def row_blocks(lay, frames, decode=False):
    """{role: Block} of the three row roles of a batch under a layout."""
    ms, fs, ws, tight = minimal_strides(frames)
    wkind = decode_witness_kind(lay) if decode else lay.witnesses.kind
    F = len(frames)
    return {"masks": Block(F, stride_of(lay.masks.kind, ms), lay.masks.base),
            "filters": Block(F, stride_of(lay.filters.kind, fs), lay.filters.base),
            "witnesses": Block(F, tight if wkind == "tight" else stride_of(wkind, ws), lay.witnesses.base)}


def reduce_takes_vectors(block):
    """k_filter_reduce's choice (insert_fast, csrc/rbf_api.hip): 16-byte accesses iff the stride is whole quads and the base is aligned."""
    return (block.stride // 4) % 4 == 0 and block.base % 16 == 0


# ------------------------------------------------------------------ row-address rules a kernel could have by mistake
# offset of row f from the aligned start of the rows' allocation (Block: GUARD; FarBlock: 0), given the caller's base and byte stride
TRUE_RULE = lambda base, stride, f: base + f * stride                                             # noqa: E731
MUTANTS = {
    "stride_in_32_bits": lambda base, stride, f: base + ((f * stride) & 0xFFFFFFFF),      # the stride, or its product with f, kept in 32 bits
    "bytes_taken_as_dwords": lambda base, stride, f: base + f * stride * 4,
    "dwords_taken_as_bytes": lambda base, stride, f: base + f * (stride // 4),
    "base_ignored": lambda base, stride, f: f * stride,
    "stride_rounded_to_16": lambda base, stride, f: base + f * ((stride + 15) // 16 * 16),
}


def mutant_fetch(block, raw, rule, nbytes):
    """What a reader with `rule` takes for each row of a placed Block: nbytes from its address, None where that leaves the block."""
    out = []
    for f in range(block.nrows):
        at = block.guard + rule(block.base, block.stride, f)
        out.append(raw[at:at + nbytes].copy() if 0 <= at and at + nbytes <= raw.nbytes else None)
    return out


def mutant_verdict(block, raw, name, nbytes):
    """None: the mutant forms the true addresses under this layout | True: it fetches other bytes for some row | False: it would pass."""
    if all(MUTANTS[name](block.base, block.stride, f) == TRUE_RULE(block.base, block.stride, f) for f in range(block.nrows)):
        return None
    true, got = mutant_fetch(block, raw, TRUE_RULE, nbytes), mutant_fetch(block, raw, MUTANTS[name], nbytes)
    return any(g is None or not np.array_equal(g, t) for g, t in zip(got, true))


def ones_in(row, nbytes):
    return int(np.unpackbits(row[:nbytes]).sum())


# ------------------------------------------------------------------ far rows (tests/block_layout.py)
def far_layout(which, row_bytes):
    """FarBlock of the sweep's two far places: `rows` -- base 0, stride 2^32 + 2^16, two rows | `frames` -- base 2^31, stride 2^31 + 2^20,
    three rows."""
    import block_layout as bl
    return bl.far_masks(row_bytes) if which == "rows" else bl.far_frames(row_bytes)


FAR_PLACES = {"rows": 2, "frames": 3}                             # rows a place holds = frames of the batch run there
# Frames of the 509x257 batch at a far place, and the frames whose rows are the decoys (one per far row, in FarBlock.decoys' order): every
# decoy is another valid row of the same kind.  FAR_CODED: the far rows belong to coded frames (what encode and decode read and write);
# FAR_PASSTHROUGH: to the frame the reference passes through, the only kind whose mask row rbf_pack_records reads.
FAR_CODED = {"rows": [4, 0], "frames": [4, 0, 1]}
FAR_PASSTHROUGH = {"rows": [0, 4], "frames": [0, 4, 4]}
FAR_DECOYS = {"rows": [5], "frames": [5, 2]}


# Mask strides whose LOW 32 bits are smaller than a row: two rows in the `rows` allocation, no decoy -- kept in 32 bits, row 1's offset
# lands inside row 0, which holds another mask.  k_insert_tab / k_insert_positions stage a row's bytes under a 32-bit bound made from
# the stride: taken from its low half, that bound was 0 and 8 here, and the filter was built from what LDS happened to hold.
WRAPPING_STRIDES = [1 << 32, (1 << 32) + 8]


def encoded_with(oracle, mask, fr):
    """(filter row, witness bits, witness row) of `mask` under frame fr's geometry: what an encode gives that reads another mask row."""
    n = len(fr.mask)
    bits, witness = np.zeros(fr.m, np.uint8), np.zeros(n, np.uint8)
    vp = ctypes.c_void_p
    mask = np.ascontiguousarray(mask, np.uint8)
    w = int(oracle.lib().orc_compress(vp(mask.ctypes.data), n, fr.m, float(fr.k), (ctypes.c_uint64 * 3)(*P.SEEDS_VIDEO), vp(bits.ctypes.data),
                                      vp(witness.ctypes.data)))
    return padded(bits), w, padded(witness[:w])


def far_rows(frames, role, nbytes):
    """The rows of `role` of some frames, each nbytes long (zero behind its payload)."""
    out = []
    for fr in frames:
        p = {"masks": mask_row(fr), "filters": fr.filter, "witnesses": fr.witness}[role]
        row = np.zeros(nbytes, np.uint8)
        row[:min(p.nbytes, nbytes)] = p[:nbytes]
        out.append(row)
    return out


def far_row_bytes(frames, role):
    ms, fs, ws, tight = minimal_strides(frames)
    return {"masks": ms, "filters": fs, "witnesses": ws}[role]


def decoded(oracle, fr, filter_row, witness_row):
    """The mask the reference's decompress gives for frame fr's geometry from these packed rows."""
    n = len(fr.mask)
    bits = np.ascontiguousarray(np.unpackbits(filter_row)[:fr.m])
    wit = np.zeros(n, np.uint8)
    have = np.unpackbits(witness_row)[:n]
    wit[:len(have)] = have
    out = np.zeros(n, np.uint8)
    vp = ctypes.c_void_p
    oracle.lib().orc_decompress(vp(bits.ctypes.data), fr.m, vp(wit.ctypes.data), n, float(fr.k), (ctypes.c_uint64 * 3)(*P.SEEDS_VIDEO), vp(out.ctypes.data))
    return out


# ------------------------------------------------------------------ one context, shrinking and growing (part C)
# (W, H, frames, rbf_ctx_force_generic argument); then the first again
SEQUENCE = [(512, 256, 6, 0), (799, 11, 6, 0), (322, 181, 6, 1), (509, 257, 3, 0)]
SEQUENCE_ORDER = [0, 1, 2, 3, 0]


# ------------------------------------------------------------------ the runs entry's clip
RUN_DENSITIES = [[0.0889, 0.2], [0.05, 0.4, 0.01]]                # seven frames, six pairs, pair 2 lies across the second keyframe
RUN_SKIPPED = 2
RUN_CASES = [(1, True), (1, False), (3, False)]                   # (mask_channels, planar luma)
RUN_IDS = ["luma_planar", "luma_interleaved", "all_interleaved"]

_RUNS = {}


def runs_clip(oracle, W, H, mc):
    """(frames (7, H, W, 3) uint8, run_starts, Frames of the six pairs -- the skipped pair's from an all-zero mask)."""
    key = (W, H, mc)
    if key not in _RUNS:
        from test_gpu_runs import make_runs
        frames, starts = make_runs(60 + W, W, H, RUN_DENSITIES)
        assert starts == [RUN_SKIPPED + 1]
        want = []
        for f in range(len(frames) - 1):
            if f == RUN_SKIPPED:
                mask = np.zeros(W * H, np.uint8)
            elif mc == 1:
                mask = oracle.residual_mask(np.ascontiguousarray(frames[f][..., 0]), np.ascontiguousarray(frames[f + 1][..., 0]), 0.0).reshape(-1)
            else:
                mask = (frames[f] != frames[f + 1]).any(-1).reshape(-1).astype(np.uint8)
            want.append(expect_frame(oracle, mask))
        _RUNS[key] = (frames, starts, want)
    return _RUNS[key]
