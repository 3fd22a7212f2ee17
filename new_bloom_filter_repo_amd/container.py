"""The video container, its record types and the layout of a stream: which frames are keyframes, where the encoder's blocks and the
decoder's runs start and end, and the bound frame of a near-lossless call (no GPU; numpy only in bounds_frame).

All-keyframe streams are written exactly as the reference does -- 'BFVC' | <I frames | (<I len | record)*
(improved_video_compressor.py:398-406) -- so either implementation reads them.  Streams with any other record use magic 'BFV2' and prefix
every record with a type byte, following the type-byte precedent of VideoFrameCompressor.compress_frame (:1053):
  1 = keyframe (zlib, FixedVideoCompressor), 2 = inter-frame (Bloom record, values in zlib-9),
  3, 4 = the same two roles with the GPU sample codec in place of zlib-9 (sample_codec.py has their layout),
  5 = the frame digests of all the records in front of it (integrity.py has the layout): optional, only as the LAST record.  It is no
      frame: split_trailer takes it off, and everything else in this module sees the frame records only.
  6 = the pan table (build_pans has the layout): optional, behind the last frame record and in front of a digest trailer.  It is no frame
      either: split_tables takes it off.
  7 = a keyframe within a bound per channel (bounded_keyframes=True; sample_codec.py has its layout).  KEYS stays the pair of exact
      keyframe types; KEY_TYPES names every keyframe type, and is what the stream checks below go by.
"""
import struct

KEY, INTER, KEY_RICE, INTER_RICE = 1, 2, 3, 4
KEYS, INTERS = (KEY, KEY_RICE), (INTER, INTER_RICE)
DIGESTS = 5
PANS = 6
PANS_VERSION = 1
KEY_NEAR = 7
KEY_TYPES = KEYS + (KEY_NEAR,)


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
    """[(type, record)] of a container.  A plain ValueError for bytes that are not a whole container: another magic, a header, a length
    field or a body that is cut short, a count that the bytes cannot hold, a 'BFV2' record without its type byte, or bytes behind the
    last record.  The message names the record."""
    magic = bytes(blob[:4])
    if magic not in (b"BFVC", b"BFV2"):
        raise ValueError(f"Invalid file format: {magic}")
    if len(blob) < 8:
        raise ValueError("container of %d bytes is cut short in its header" % len(blob))
    (count,) = struct.unpack_from("<I", blob, 4)
    if count > (len(blob) - 8) // 4:
        raise ValueError("container declares %d records, its %d bytes cannot hold them" % (count, len(blob)))
    off, records = 8, []
    for i in range(count):
        if off + 4 > len(blob):
            raise ValueError("record %d of %d: the container ends in front of or inside its length field" % (i, count))
        (length,) = struct.unpack_from("<I", blob, off)
        if off + 4 + length > len(blob):
            raise ValueError("record %d of %d declares %d bytes, the container has %d left" % (i, count, length, len(blob) - off - 4))
        body = blob[off + 4: off + 4 + length]
        off += 4 + length
        if magic == b"BFV2" and not length:
            raise ValueError("record %d of %d is empty: a record starts with its type byte" % (i, count))
        records.append((KEY, body) if magic == b"BFVC" else (body[0], body[1:]))
    if off != len(blob):
        where = "record %d, the last of the %d the container declares" % (count - 1, count) if count else "the header of a container that declares no record"
        raise ValueError("%d bytes behind %s" % (len(blob) - off, where))
    return records


def build_pans(entries):
    """The body of the PANS record: '<B' version = 1 | 3 zero bytes | '<I' count | count x ('<I' record index, '<I' ox, '<I' oy) | '<Q' FD1
    (rbf_frame_digest_host) of all preceding body bytes.  entries: {record index: (ox, oy)} or [(record index, ox, oy)] -- the cumulative
    offsets of the inter-frame records whose stabilised frame is not the frame itself ((ox, oy) != (0, 0), 0 <= ox < W, 0 <= oy < H):
    the record codes S(p) = F((p + (ox, oy)) mod (W, H)), a decoder rolls the rebuilt frame back.  Written ascending by record index."""
    from .integrity import frame_digest
    rows = sorted((int(i), int(ox), int(oy)) for i, (ox, oy) in entries.items()) if isinstance(entries, dict) else [tuple(int(v) for v in e) for e in entries]
    body = struct.pack("<B3xI", PANS_VERSION, len(rows)) + b"".join(struct.pack("<III", *row) for row in rows)
    return body + struct.pack("<Q", frame_digest(body))


def parse_pans(body):
    """[(record index, ox, oy)] of a PANS record body; a plain ValueError for anything that is not a whole, undamaged version-1 table
    whose entries ascend by record index and carry a non-zero offset (what the table's own bytes can say: split_tables checks the
    entries against the container's records)."""
    from .integrity import frame_digest
    body = bytes(body)
    if len(body) < 16:
        raise ValueError("pan table: its %d bytes are shorter than a table's header and checksum" % len(body))
    version, z0, z1, z2, count = struct.unpack_from("<BBBBI", body, 0)
    if version != PANS_VERSION:
        raise ValueError("pan table version %d is unknown (this reader knows %d)" % (version, PANS_VERSION))
    if z0 or z1 or z2:
        raise ValueError("pan table: reserved bytes are not zero")
    if len(body) != 8 + 12 * count + 8:
        raise ValueError("pan table of %d bytes does not hold the %d entries it declares" % (len(body), count))
    (stored,) = struct.unpack_from("<Q", body, len(body) - 8)
    if stored != frame_digest(body[:-8]):
        raise ValueError("pan table is damaged: its own checksum does not match")
    rows = [struct.unpack_from("<III", body, 8 + 12 * j) for j in range(count)]
    if not rows:
        raise ValueError("pan table without entries: a container without pans carries no table")
    for a, b in zip(rows, rows[1:]):
        if b[0] <= a[0]:
            raise ValueError("pan table: record index %d after %d, the entries must ascend" % (b[0], a[0]))
    for i, ox, oy in rows:
        if ox == 0 and oy == 0:
            raise ValueError("pan table: record %d has offset (0, 0), which is no entry" % i)
    return rows


def split_tables(records, frame_shape=None):
    """(frame records, pans, digests) of a container's records: split_trailer, and the PANS record taken off as well.  pans: {record index:
    (ox, oy)}, empty without a table.  A plain ValueError when the table is there twice, does not stand directly behind the last frame
    record (in front of a digest trailer, if there is one), is damaged (parse_pans), or names a record that is no inter-frame.
    frame_shape: (H, W) of the frames when the caller knows it -- an offset outside 0 <= ox < W, 0 <= oy < H is then refused too
    (check_pans does that for a caller who learns the shape later)."""
    at = [i for i, (ty, _) in enumerate(records) if ty == PANS]
    if not at:
        frames, digests = split_trailer(records)
        return frames, {}, digests
    if len(at) > 1:
        raise ValueError("%d pan tables (records %s): a container has at most one" % (len(at), at))
    rest = list(records[:at[0]]) + list(records[at[0] + 1:])
    frames, digests = split_trailer(rest)
    if at[0] != len(frames):
        raise ValueError("the pan table is record %d, behind %d frame records: it stands directly behind the last frame record" % (at[0], len(frames)))
    pans = {}
    try:
        rows = parse_pans(records[at[0]][1])
    except ValueError as e:
        raise ValueError("record %d: %s" % (at[0], e)) from None
    for i, ox, oy in rows:
        if i >= len(frames) or frames[i][0] not in INTERS:
            raise ValueError("pan table: record %d is no inter-frame record" % i)
        pans[i] = (ox, oy)
    if frame_shape is not None:
        check_pans(pans, frame_shape)
    return frames, pans, digests


def check_pans(pans, frame_shape):
    """ValueError unless every offset of a pan table fits frames of frame_shape = (H, W, ...)."""
    H, W = int(frame_shape[0]), int(frame_shape[1])
    for i, (ox, oy) in sorted(pans.items()):
        if not (0 <= ox < W and 0 <= oy < H):
            raise ValueError("pan table: record %d has offset (%d, %d) outside a frame of %dx%d" % (i, ox, oy, W, H))


def pan_offsets(stats, run_starts, W, H):
    """The pan rule and the accumulation on the rows of a block (GopCoder.align_pans: one row per pair, row j - 1 for frame j of the block,
    fields dx, dy, moving_zero, moving_best -- include/rbf.h, rbf_pan_search): pair j adopts v_j = (dx, dy) iff moving_best < moving_zero,
    else v_j = 0 -- integers, no tunable constant; c_0 = 0 and c_j = 0 at every run start, else c_j = c_{j-1} + v_j, reduced to
    0 <= ox < W, 0 <= oy < H.  Returns (offsets, adopted): offsets[j] = (ox, oy) for every frame j of the block, adopted = [(j, dx, dy)]
    for the pairs that adopted a shift, ascending."""
    starts = {int(t) for t in run_starts or ()}
    offsets, adopted = [(0, 0)], []
    for j, row in enumerate(stats, start=1):
        if j in starts:
            offsets.append((0, 0))
            continue
        dx, dy = int(row["dx"]), int(row["dy"])
        ox, oy = offsets[-1]
        if (dx or dy) and int(row["moving_best"]) < int(row["moving_zero"]):
            adopted.append((j, dx, dy))
            ox, oy = (ox + dx) % int(W), (oy + dy) % int(H)
        offsets.append((ox, oy))
    return offsets, adopted


def stat_tolerance(max_error, bounds_min, hold_mode, sample_bytes):
    """The scalar tolerance a block is looked at with (GopCoder.cut_stats, align_pans) before any hold rewrites it -- a pixel the hold
    will keep still is not moving: max_error, or the SMALLEST entry of the bound frame (bounds_min; None without one), doubled for
    hold_mode="lookahead" and clamped to the sample range."""
    tol = int(max_error if bounds_min is None else bounds_min)
    return min(tol if hold_mode == "first" else 2 * tol, (1 << (8 * sample_bytes)) - 1)


def sweep_candidates(cap):
    """The bounds a target_psnr call tries for every run (GopCoder.hold_sweep takes at most eight): 1..cap when cap <= 8, else the
    distinct values of round(cap * i / 8), i = 1..8 -- ascending, the last one is cap.  cap: max_error, 1..255."""
    cap = int(cap)
    if not 1 <= cap <= 255:
        raise ValueError("the sweep's ceiling must be in 1..255, got %r" % (cap,))
    if cap <= 8:
        return list(range(1, cap + 1))
    return sorted({int(round(cap * i / 8)) for i in range(1, 9)})


def sse_budget(target_psnr, bits, samples):
    """The largest sum of squared errors `samples` samples of `bits` bits may carry at a PSNR of at least target_psnr dB (peak
    2^bits - 1): floor(samples * peak^2 / 10^(target_psnr / 10)).  The one place that forms it."""
    peak = (1 << int(bits)) - 1
    tenths = float(target_psnr) / 10.0
    return 0 if tenths > 300.0 else int(int(samples) * peak * peak / 10.0 ** tenths)     # (10^300: no clip's sse reaches it)


def choose_bound(rows, candidates, budget):
    """The bound of one run under a target: the LARGEST candidate whose sse (rows: the run's GopCoder.hold_sweep rows, one per
    candidate) is within `budget` -- whether or not sse grows with the bound -- and 0, the exact run, when none is."""
    for row, d in reversed(list(zip(rows, candidates))):
        if int(row["sse"]) <= budget:
            return int(d)
    return 0


def rebase_cuts(offsets, cuts, starts, W, H):
    """A scene cut is a keyframe, coded from the caller's array, so its run starts at offset 0 like every other: (new offsets, rel) for
    a block whose frames were rolled by `offsets` (pan_offsets) and in which the frames `cuts` then became run starts (starts: all the
    run starts, cuts included).  The cut frame and the frames that hang off it -- up to the next run start -- are rolled back by the cut
    frame's offset: rel[f] is what to roll frame f by now (GopCoder.roll_frames; (0, 0) outside the cuts' runs), new offsets[f] the
    frame's offset after that, reduced to 0 <= ox < W, 0 <= oy < H."""
    new, rel = list(offsets), [(0, 0)] * len(offsets)
    for j in cuts:
        cx, cy = offsets[j]
        end = min([t for t in starts if t > j] + [len(offsets)])
        for f in range(j, end):
            rel[f] = (-cx, -cy)
            new[f] = ((offsets[f][0] - cx) % W, (offsets[f][1] - cy) % H)
    return new, rel


def fallback_pairs(skipped, uncovered, offsets, near):
    """Which pairs of a coded block are NOT written as inter-frames: [bool] per pair, pair f being frame f + 1 of the block.  skipped[f]:
    the pair stands in front of a run start (the frame is a keyframe anyway); uncovered[f]: pixels of it changed that its mask cannot
    say (a luma mask, chroma moved alone), so the frame falls back to an exact keyframe.  In a near-lossless block (near) and in a run
    that carries a non-zero pan offset (offsets: the frames' cumulative offsets, or None) the rest of the run goes with it: its records
    continue the HELD or STABILISED frames, not the exact keyframe a decoder will have.
    near and pan_range both need mask_channels="all", whose uncovered counts are all zero on frames of two or more channels, so colour
    clips never reach that propagation.  Single-channel frames do: their one sample goes through the luma rule whatever mask_channels
    says, and at 16 bits that rule does not mark a change of exactly 0x8000 (the int16 wrap).  A near-lossless or panned
    run of 16-bit grey frames with such a pixel falls back from that frame on (tests/surface_cases.py has such clips)."""
    pairs = len(skipped)
    panned = [False] * pairs                     # pair f belongs to a run that carries a non-zero offset
    if offsets is not None:
        run_bounds = sorted({0} | {f + 1 for f in range(pairs) if skipped[f]}) + [pairs + 1]
        for lo, hi in zip(run_bounds, run_bounds[1:]):
            if any(offsets[t] != (0, 0) for t in range(lo, hi)):
                panned[lo:hi - 1] = [True] * (hi - 1 - lo)
    out, broken = [], False                      # broken: a frame of this run fell back, and the rest of the run goes with it
    for f in range(pairs):
        falls = not skipped[f] and (bool(int(uncovered[f])) or broken)
        broken = falls and (bool(near) or panned[f])
        out.append(bool(skipped[f]) or falls)
    return out


def split_trailer(records):
    """(frame records, digests): the digests of a container's DIGESTS record, one per frame record, or None when it has none.  A plain
    ValueError -- never an integrity error, which speaks of frames -- when the trailer is not the last record, is there twice, does not
    cover exactly the frame records in front of it, or is damaged (integrity.parse_trailer).  (A container with a pan table: split_tables.)"""
    at = [i for i, (ty, _) in enumerate(records) if ty == DIGESTS]
    if not at:
        return list(records), None
    if len(at) > 1:
        raise ValueError("%d digest trailers (records %s): a container has at most one" % (len(at), at))
    if at[0] != len(records) - 1:
        raise ValueError("the digest trailer is record %d of %d: it may only be the last" % (at[0], len(records)))
    from .integrity import parse_trailer
    try:
        digests = parse_trailer(records[-1][1])
    except ValueError as e:
        raise ValueError("record %d: %s" % (at[0], e)) from None
    if len(digests) != len(records) - 1:
        raise ValueError("record %d: the digest trailer covers %d frames, the container holds %d" % (at[0], len(digests), len(records) - 1))
    return list(records[:-1]), digests


def check_types(types):
    """ValueError, naming the record, unless every type is known and the stream starts with a keyframe."""
    for i, ty in enumerate(types):
        if ty not in KEY_TYPES + INTERS:
            raise ValueError(f"record {i}: unknown record type {ty}")
    if types and types[0] in INTERS:
        raise ValueError("record 0: inter-frame without a preceding keyframe")


def inter_runs(types):
    """The maximal runs of inter-frame records of a checked stream: [(index of the keyframe in front, first record, end)]."""
    runs, i = [], 0
    while i < len(types):
        if types[i] in KEY_TYPES:
            i += 1
            continue
        j = i
        while j < len(types) and types[j] in INTERS:
            j += 1
        runs.append((i - 1, i, j))
        i = j
    return runs


def read_span(types, start=0, stop=None, step=1):
    """What a reader of the frames range(start, stop, step) of a checked stream has to decode, from the record types alone: (keys, runs).
    keys: the keyframe records that are wanted themselves, ascending (lone keyframes and keyframes in front of a run alike).  runs:
    [(keyframe record, first record, end, positions)] for every run of inter_runs(types) that holds a wanted frame -- `end` is one past
    the LAST record the reader needs, not the run's end, and positions are the wanted records as offsets from the run's first record.
    Runs and keyframes without a wanted frame do not appear.  stop None or past the end: the end of the stream.  ValueError for
    step < 1, start < 0, or a span that is empty after clamping."""
    count = len(types)
    for name, v in (("start", start), ("step", step)) + ((("stop", stop),) if stop is not None else ()):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    start, step = int(start), int(step)
    stop = count if stop is None else min(int(stop), count)
    if step < 1:
        raise ValueError("step must be >= 1, got %d" % step)
    if start < 0:
        raise ValueError("start must be >= 0, got %d" % start)
    if start >= stop:
        raise ValueError("no frame in [%d, %d) of a stream of %d frames" % (start, stop, count))
    wanted = range(start, stop, step)
    keys = [i for i in wanted if types[i] in KEY_TYPES]
    runs = []
    for k, lo, hi in inter_runs(types):
        first = start if start >= lo else lo + (start - lo) % step           # the first wanted record at or behind lo
        inside = list(range(first, min(hi, stop), step))
        if inside:
            runs.append((k, lo, inside[-1] + 1, [i - lo for i in inside]))
    return keys, runs


def span_records(keys, runs):
    """How many records a reader of read_span's (keys, runs) decodes: every run's keyframe and its records up to the last one needed,
    and the wanted keyframes that front no such run."""
    fronts = {k for k, _, _, _ in runs}
    return len(fronts | set(keys)) + sum(end - lo for _, lo, end, _ in runs)


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
