"""The video container, its record types and the layout of a stream: which frames are keyframes, where the encoder's blocks and the
decoder's runs start and end, and the bound frame of a near-lossless call (no GPU; numpy only in bounds_frame).

All-keyframe streams are written exactly as the reference does -- 'BFVC' | <I frames | (<I len | record)*
(improved_video_compressor.py:398-406) -- so either implementation reads them.  Streams with any other record use magic 'BFV2' and prefix
every record with a type byte, following the type-byte precedent of VideoFrameCompressor.compress_frame (:1053):
  1 = keyframe (zlib, FixedVideoCompressor), 2 = inter-frame (Bloom record, values in zlib-9),
  3, 4 = the same two roles with the GPU sample codec in place of zlib-9 (sample_codec.py has their layout),
  5 = the frame digests of all the records in front of it (integrity.py has the layout): optional, only as the LAST record.  It is no
      frame: split_trailer takes it off, and everything else in this module sees the frame records only.
"""
import struct

KEY, INTER, KEY_RICE, INTER_RICE = 1, 2, 3, 4
KEYS, INTERS = (KEY, KEY_RICE), (INTER, INTER_RICE)
DIGESTS = 5


def write(records):
    """The container bytes of [(type, record)]."""
    all_key = all(ty == KEY for ty, _ in records)
    out = [b"BFVC" if all_key else b"BFV2", struct.pack("<I", len(records))]
    for ty, rec in records:
        body = rec if all_key else struct.pack("<B", ty) + rec
        out += [struct.pack("<I", len(body)), body]
    return b"".join(out)


def size(records):
    """len(write(records)) without building it."""
    extra = 0 if all(ty == KEY for ty, _ in records) else 1
    return 8 + sum(4 + extra + len(rec) for _, rec in records)


def parse(blob):
    """[(type, record)] of a container."""
    magic = blob[:4]
    if magic not in (b"BFVC", b"BFV2"):
        raise ValueError(f"Invalid file format: {magic}")
    (count,) = struct.unpack_from("<I", blob, 4)
    off, records = 8, []
    for _ in range(count):
        (length,) = struct.unpack_from("<I", blob, off)
        body = blob[off + 4: off + 4 + length]
        off += 4 + length
        records.append((KEY, body) if magic == b"BFVC" else (body[0], body[1:]))
    return records


def split_trailer(records):
    """(frame records, digests): the digests of a container's DIGESTS record, one per frame record, or None when it has none.  A plain
    ValueError -- never an integrity error, which speaks of frames -- when the trailer is not the last record, is there twice, does not
    cover exactly the frame records in front of it, or is damaged (integrity.parse_trailer)."""
    at = [i for i, (ty, _) in enumerate(records) if ty == DIGESTS]
    if not at:
        return list(records), None
    if len(at) > 1:
        raise ValueError("%d digest trailers (records %s): a container has at most one" % (len(at), at))
    if at[0] != len(records) - 1:
        raise ValueError("the digest trailer is record %d of %d: it may only be the last" % (at[0], len(records)))
    from .integrity import parse_trailer
    digests = parse_trailer(records[-1][1])
    if len(digests) != len(records) - 1:
        raise ValueError("the digest trailer covers %d frames, the container holds %d" % (len(digests), len(records) - 1))
    return list(records[:-1]), digests


def check_types(types):
    """ValueError unless every type is known and the stream starts with a keyframe."""
    for ty in types:
        if ty not in KEYS + INTERS:
            raise ValueError(f"unknown record type {ty}")
    if types and types[0] in INTERS:
        raise ValueError("inter-frame without a preceding keyframe")


def inter_runs(types):
    """The maximal runs of inter-frame records of a checked stream: [(index of the keyframe in front, first record, end)]."""
    runs, i = [], 0
    while i < len(types):
        if types[i] in KEYS:
            i += 1
            continue
        j = i
        while j < len(types) and types[j] in INTERS:
            j += 1
        runs.append((i - 1, i, j))
        i = j
    return runs


def is_keyframe(t, first_index, keyframe_interval, inter_frames=True):
    """The keyframe rule for global frame t of a call whose first frame is global frame first_index: t % keyframe_interval == 0, or no
    inter-frames at all, or the frame's predecessor is not among the frames handed in."""
    return not inter_frames or t % keyframe_interval == 0 or t - 1 < first_index


def plan_range(first_index, start, stop, keyframe_interval, block_frames, inter_frames):
    """What encode_range does with the frames [start, stop) of a call whose frames begin at global index first_index: (fixed_keys, blocks).
    fixed_keys: the frames the rule makes keyframes, ascending.  blocks: [(first frame read, end, run starts)] -- a block reads the frames
    lo .. end-1 (at most block_frames, several GOPs), codes every frame but the first against its predecessor, and its run starts (indices
    into the block) are the keyframes inside it, which start a new run."""
    fixed = [t for t in range(start, stop) if is_keyframe(t, first_index, keyframe_interval, inter_frames)]
    blocks = []
    t = start
    while t < stop:
        if is_keyframe(t, first_index, keyframe_interval, inter_frames):
            t += 1
            continue
        end = min(stop, t - 1 + block_frames)                            # the block reads frames t-1 .. end-1
        blocks.append((t - 1, end, [u - (t - 1) for u in range(t, end) if is_keyframe(u, first_index, keyframe_interval)]))      # keyframes inside the block: new runs
        t = end
    return fixed, blocks


def blocks_off_keyframes(blocks, first_index, keyframe_interval):
    """The blocks of a plan_range() plan whose first frame -- the one a block reads but does not code -- is NOT a keyframe of the stream.
    A near-lossless call (max_error > 0) needs this list to be empty: a block's frames are held against the block's own first frame, so a
    block that starts inside a run would need the held state of the block in front of it, which lives in another lane's coder."""
    return [b for b in blocks if not is_keyframe(b[0], first_index, keyframe_interval)]


def bounds_frame(error_bounds, shape=None, dtype=None):
    """The BOUND FRAME of a near-lossless call with a bound per sample: an array of exactly a frame's `shape` ((H, W) or (H, W, C)) and
    `dtype` (uint8 / uint16) whose entry is the largest error its sample may be coded with -- the only form the layers below the surface
    see (GopCoder(error_bounds=...), rbf_temporal_hold_runs_map).  error_bounds is one of
      a sequence of C non-negative integers          one bound per channel (C = 1 for (H, W) frames)
      an integer array of shape (H, W)               one bound per pixel, for all of its samples
      an integer array of shape (H, W, C)            one bound per sample
    ValueError for anything else: a str, a scalar, floats, bools, negative values, values that do not fit the sample width, a shape that
    does not fit the frames.  shape=None: only what can be said without a frame is checked (the constructors do that) and the bounds come
    back as an int64 array.  (The one function of this module that needs numpy; no native library.)"""
    import numpy as np
    if isinstance(error_bounds, (str, bytes, bytearray)) or np.ndim(error_bounds) == 0:
        raise ValueError("error_bounds must be a sequence of per-channel bounds or an (H, W) / (H, W, C) integer array, got %r" % (error_bounds,))
    if isinstance(error_bounds, (list, tuple)) and any(isinstance(v, (bool, np.bool_)) for v in error_bounds):
        raise ValueError("error_bounds must be integers, got a bool in %r" % (error_bounds,))
    try:
        e = np.asarray(error_bounds)
    except ValueError:
        raise ValueError("error_bounds is not a rectangular array") from None
    if e.dtype.kind not in "iu":
        raise ValueError("error_bounds must be integers, got dtype %s" % e.dtype)
    if not 1 <= e.ndim <= 3 or e.size == 0:
        raise ValueError("error_bounds must have one, two or three dimensions, got shape %r" % (e.shape,))
    e = e.astype(np.int64) if e.dtype != np.uint64 else e
    if int(e.min()) < 0:
        raise ValueError("error_bounds must be non-negative, got %d" % int(e.min()))
    if shape is None:
        return e
    shape, dtype = tuple(int(s) for s in shape), np.dtype(dtype)
    if dtype not in (np.uint8, np.uint16) or len(shape) not in (2, 3):
        raise ValueError("a bound frame is an (H, W) or (H, W, C) frame of uint8 or uint16, got %r of %s" % (shape, dtype))
    top = int(np.iinfo(dtype).max)
    if int(e.max()) > top:
        raise ValueError("error_bounds %d does not fit a %d-bit sample" % (int(e.max()), 8 * dtype.itemsize))
    C = shape[2] if len(shape) == 3 else 1
    if e.ndim == 1:
        if e.shape[0] != C:
            raise ValueError("error_bounds has %d per-channel bounds, the frames have %d channel(s)" % (e.shape[0], C))
        e = e if len(shape) == 3 else e[0]
    elif e.shape == shape[:2] and len(shape) == 3:
        e = e[:, :, None]
    elif e.shape != shape:
        raise ValueError("error_bounds of shape %r does not fit frames of shape %r" % (e.shape, shape))
    out = np.empty(shape, dtype=dtype)
    out[...] = e
    return out


def uniform_bound(bound_frame):
    """d when every entry of the bound frame equals d, else None: such a frame is today's max_error=d, and the surface codes it through
    the scalar calls -- the container is byte for byte that of max_error=d."""
    flat = bound_frame.reshape(-1)
    d = int(flat[0])
    return d if bool((flat == flat[0]).all()) else None


def cut_frames(stats, run_starts=()):
    """The scene-cut rule on the statistics of a block (GopCoder.cut_stats: one row (moving, inter_bits, intra_bits) per pair, row j - 1
    for frame j of the block): frame j is a cut iff inter_bits + moving > intra_bits -- coding it against its predecessor, at one mask bit
    per moving pixel, would cost more than coding it on its own.  Integers only, no tunable constant.  Returns the block indices j >= 1,
    ascending, that are cuts and not run starts (keyframes of the stream) already."""
    known = {int(t) for t in run_starts}
    cuts = []
    for j, row in enumerate(stats, start=1):
        moving, inter, intra = (int(v) for v in row)
        if inter + moving > intra and j not in known:
            cuts.append(j)
    return cuts
