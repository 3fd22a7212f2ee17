"""Damaged containers: small containers built on the host, a list of named damages, and a host-only twin of the decoder -- the cases and
the reference of tests/test_damaged_containers_cpu.py and tests/test_gpu_damaged_containers.py; a helper, not a test.

  containers  13 frames, a keyframe every 6 (records 0, 6 and 12 are keyframes: two runs), 67 x 33 x 3 at 8 bits and 37 x 9 x 3 at 16 bits,
              a luma mask and an all-channel mask, each with and without a digest trailer.  They are written HERE, not by the product:
              type-1 records by zlib, type-2 records from the C oracle's compress, the trailer from the numpy FD1.  Every container holds
              a Bloom-coded inter-frame (witness_bits > 0) and a passthrough one.  The record types of the GPU sample codec (3, 4, 7) and
              the pan table (6) have no host encoder in this tree; their damages are not in this file (DESIGN.md 7 says so).
  damages     `damages(container)`: named cases -- every field of every record type at 0, its value - 1, + 1, its maximum and with bit 31
              (its top bit) set; every record cut at every field boundary and one byte either side; a record made empty; records dropped,
              doubled and swapped; the count field +- 1; a bit flipped in the first, the last and a seeded middle byte of every payload.
  twin        `twin_decode(records)`: Refused(record index) or the frames and, with a trailer, the frames whose digest is not the stored
              one.  zlib for type 1; the record's fields, the pass set of tests/foreign_decode.py's reference and a numpy scatter for type
              2; integrity.frame_digest for the trailer.  The rules it restates are the ones DESIGN.md 6 gives a reader of a container."""
import collections
import struct
import zlib

import numpy as np

import re

import bloom_params as bp
import foreign_decode as fd
import near_key_ref as nk
import sample_codec_ref as ref
from new_bloom_filter_repo_amd import container, integrity
from new_bloom_filter_repo_amd import params as P
from new_bloom_filter_repo_amd import sample_codec as sc
from new_bloom_filter_repo_amd.frame_codec import build_record, parse_record

KEY, INTER, KEY_RICE, INTER_RICE, DIGESTS, PANS, KEY_NEAR = 1, 2, 3, 4, 5, 6, 7
KEYS, INTERS = (KEY, KEY_RICE, KEY_NEAR), (INTER, INTER_RICE)
NEAR_BOUNDS = (2, 3, 3)
PAN_OFFSETS = {7: (2, 1), 8: (2, 1), 9: (4, 2), 10: (4, 2), 11: (5, 2)}     # record -> cumulative (ox, oy): the second run is panned
T, INTERVAL = 13, 6
SHAPES = {"u8": (33, 67, np.uint8), "u16": (9, 37, np.uint16)}
PASSTHROUGH_FRAME = 3                                              # the frame whose mask is too dense for a filter
Container = collections.namedtuple("Container", "name frames records blob coded passthrough")


class Refused(Exception):
    """The twin's verdict on a container a decoder must refuse: `record` is the index in the stream of the record that cannot be decoded."""

    def __init__(self, record, why=""):
        self.record = int(record)
        super().__init__("record %d: %s" % (record, why))


# ------------------------------------------------------------------ the clips and the host encoder
def clip(kind, seed=5100):
    H, W, dtype = SHAPES[kind]
    rng = np.random.default_rng(seed + H)
    top = int(np.iinfo(dtype).max)
    frames = [rng.integers(0, top + 1, (H, W, 3)).astype(dtype)]
    for t in range(1, T):
        f = frames[-1].copy()
        moving = rng.random((H, W)) < (0.5 if t == PASSTHROUGH_FRAME else 0.08)
        step = rng.integers(1, 0x7FFF if top > 255 else 256, (H, W, 3)).astype(dtype)     # (16 bits: never a change of exactly 0x8000)
        f[moving] = (f[moving] + step[moving]).astype(dtype)
        chroma = (rng.random((H, W)) < 0.02) & ~moving             # pixels whose chroma moves alone: the all-channel mask says them
        f[chroma, 1] ^= 1
        frames.append(f)
    return frames


def luma_mask(a, b):
    ya, yb = a[..., 0].astype(np.int64), b[..., 0].astype(np.int64)
    return ((ya ^ yb) & 0x7FFF) != 0 if a.dtype.itemsize == 2 else ya != yb


def key_record(frame):
    z = zlib.compress(frame.tobytes(), 9)
    return struct.pack("<III", frame.shape[0], frame.shape[1], frame.dtype.itemsize) + struct.pack("<I", len(z)) + z + b"\0"


def inter_record(oracle, prev, cur, channels):
    mask = (luma_mask(prev, cur) if channels == "luma" else (prev != cur).any(axis=2)).reshape(-1).astype(np.uint8)
    bitmap, witness, p, n, _ = oracle.compress(mask)
    k = oracle.optimal_params(n, p)[0] if len(witness) else 0
    values = cur.reshape(n, -1)[mask.astype(bool)].reshape(-1)
    return bytes([cur.dtype.itemsize]) + build_record("f64", p, n, k, len(bitmap), np.packbits(bitmap).tobytes(), len(witness),
                                                      np.packbits(np.array(witness, np.uint8)).tobytes(), len(values), zlib.compress(values.tobytes(), 9))


def rice_inter_record(oracle, prev, cur):
    """A type-4 record: type 2's bytes with the sample stream of the pair's residuals at the all-channel mask in the value field."""
    mask = (prev != cur).any(axis=2).reshape(-1).astype(np.uint8)
    bits = 8 * cur.dtype.itemsize
    bitmap, witness, p, n, _ = oracle.compress(mask)
    k = oracle.optimal_params(n, p)[0] if len(witness) else 0
    stream = ref.encode(ref.inter_u(prev, cur, mask, bits), bits)
    return bytes([cur.dtype.itemsize]) + build_record("f64", p, n, k, len(bitmap), np.packbits(bitmap).tobytes(), len(witness),
                                                      np.packbits(np.array(witness, np.uint8)).tobytes(), int(mask.sum()) * cur.shape[2], stream)


def build_rice(oracle, which, digests):
    """The two rice containers, written on the host from the numpy sample codec (tests/sample_codec_ref.py, tests/near_key_ref.py):
      rice_pan    8 bits, type-3 keyframes, type-4 inter-frames, the second run panned: a pan table (type 6) in front of the trailer.
                  The records code the stabilised frames; the frames of the container are those rolled back.
      rice_near   16 bits, type-7 keyframes within NEAR_BOUNDS, type-4 inter-frames that continue the quantised keyframe (what a look-ahead
                  hold leaves of a clip is the encoder's business: a container shows only the records)."""
    name = "%s%s" % (which, "_digests" if digests else "")
    if name in _CONTAINERS:
        return _CONTAINERS[name]
    src = clip("u8" if which == "rice_pan" else "u16")
    bits = 8 * src[0].dtype.itemsize
    coded, records = [], []
    for t, f in enumerate(src):
        if t % INTERVAL == 0:
            if which == "rice_pan":
                coded.append(f)
                records.append((KEY_RICE, sc.key_record(f, ref.encode(ref.intra_u(f, bits), bits))))
            else:
                y, rec = nk.record(f, NEAR_BOUNDS)
                coded.append(y)
                records.append((KEY_NEAR, rec))
        else:
            cur = coded[-1].copy()
            moved = (f != src[t - 1]).any(axis=2)
            cur[moved] = f[moved]
            records.append((INTER_RICE, rice_inter_record(oracle, coded[-1], cur)))
            coded.append(cur)
    frames = list(coded)
    if which == "rice_pan":
        frames = [np.roll(f, (PAN_OFFSETS[t][1], PAN_OFFSETS[t][0]), axis=(0, 1)) if t in PAN_OFFSETS else f for t, f in enumerate(coded)]
        records.append((PANS, container.build_pans(PAN_OFFSETS)))
    if digests:
        records.append((DIGESTS, integrity.build_trailer([integrity.frame_digest(f) for f in coded])))     # (of the frames the records code)
    wit = lambda r: parse_record("f64", r[1:])["witness_bits"]
    _CONTAINERS[name] = Container(name, frames, records, container.write(records), [i for i, (ty, r) in enumerate(records) if ty == INTER_RICE and wit(r) > 0],
                                  [i for i, (ty, r) in enumerate(records) if ty == INTER_RICE and wit(r) == 0])
    return _CONTAINERS[name]


_CONTAINERS = {}
CONFIGS = [(kind, channels, digests) for kind in ("u8", "u16") for channels in ("luma", "all") for digests in (False, True)]


def name_of(kind, channels, digests):
    return "%s_%s%s" % (kind, channels, "_digests" if digests else "")


def build(oracle, kind, channels, digests):
    """The container of a configuration.  With a luma mask the chroma-only pixels of the clip are taken out first: a luma mask cannot say
    them, and this encoder has no fallback."""
    name = name_of(kind, channels, digests)
    if name in _CONTAINERS:
        return _CONTAINERS[name]
    frames = clip(kind)
    if channels == "luma":
        for t in range(1, T):
            same = ~luma_mask(frames[t - 1], frames[t])
            frames[t][same] = frames[t - 1][same]
    records = []
    for t, f in enumerate(frames):
        records.append((KEY, key_record(f)) if t % INTERVAL == 0 else (INTER, inter_record(oracle, frames[t - 1], f, channels)))
    if digests:
        records.append((DIGESTS, integrity.build_trailer([integrity.frame_digest(f) for f in frames])))
    coded = [i for i, (ty, r) in enumerate(records) if ty == INTER and parse_record("f64", r[1:])["witness_bits"] > 0]
    passthrough = [i for i, (ty, r) in enumerate(records) if ty == INTER and parse_record("f64", r[1:])["witness_bits"] == 0]
    _CONTAINERS[name] = Container(name, frames, records, container.write(records), coded, passthrough)
    return _CONTAINERS[name]


# ------------------------------------------------------------------ the twin
def _hashes(oracle):
    return bp.hashes(oracle, fd.SEEDS)


def _key_frame(rec):
    h, w, item = struct.unpack_from("<III", rec, 0)
    (size,) = struct.unpack_from("<I", rec, 12)
    raw = zlib.decompress(bytes(rec[16:16 + size]))
    dtype = {1: np.uint8, 2: np.uint16}.get(item, np.float32)
    gray = h * w * item
    if gray == 0:
        raise ValueError("an empty frame")
    a = np.frombuffer(raw, dtype=dtype)
    if len(raw) > gray and len(raw) % gray == 0 and len(raw) // gray > 4:
        raise ValueError("more than four samples per pixel")
    frame = a.reshape(h, w, len(raw) // gray) if len(raw) > gray and len(raw) % gray == 0 else a.reshape(h, w)
    if len(rec) != 16 + size + 1 or rec[16 + size] != 0:          # (these containers carry no planes: the byte behind the frame is 0)
        raise ValueError("has_yuv")
    return frame


def _inter_frame(oracle, rec, prev):
    """The frame a type-2 record makes of `prev`; ValueError and friends where a decoder must refuse it."""
    mask, d = _inter_mask(oracle, rec, prev)
    n, ch = mask.size, prev.shape[2] if prev.ndim == 3 else 1
    raw = zlib.decompress(d["values_z"])
    if len(raw) != d["value_count"] * prev.dtype.itemsize:
        raise ValueError("value count")
    values = np.frombuffer(raw, dtype=prev.dtype)
    out = prev.copy()
    if len(values) != int(mask.sum()) * ch:
        if ch == 1:
            raise ValueError("values do not fit the mask")
        return out                                                 # a colour frame is left as it was
    out.reshape(n, -1)[mask] = values.reshape(-1, ch)
    return out


def _inter_mask(oracle, rec, prev):
    """(mask bool [n], the record's fields) of a type-2 or type-4 record behind `prev`."""
    if len(rec) < 1 or rec[0] != prev.dtype.itemsize or rec[0] not in (1, 2):
        raise ValueError("sample width")
    d = parse_record("f64", rec[1:])
    H, W = prev.shape[:2]
    n, ch = H * W, prev.shape[2] if prev.ndim == 3 else 1
    if d["n"] != n or len(d["bitmap"]) != (d["bitmap_bits"] + 7) // 8 or len(d["witness"]) != (d["witness_bits"] + 7) // 8:
        raise ValueError("n or byte counts")
    k, m = d["k"], d["bitmap_bits"]
    if not np.isfinite(k) or k < 0 or k >= 65:
        raise ValueError("k")                                      # (of a passthrough record too, which reads it no further)
    if d["witness_bits"] > 0:
        if m < 1:
            raise ValueError("m")
        floor_k, thr = P.activation_threshold(k)
        passes = bp.passing(_hashes(oracle), np.unpackbits(d["bitmap"])[:m], m, int(floor_k), int(thr), np.arange(n))
        mask = fd.reference_mask(passes, d["witness"], len(d["witness"])).astype(bool)
    else:
        if d["bitmap_bits"] != n:
            raise ValueError("a passthrough bitmap is the mask")
        mask = np.unpackbits(d["bitmap"])[:n].astype(bool)
    return mask, d


_STREAMS = {}


def _stream_u(buf, count, bits):
    """The u values of a sample stream of `count` `bits`-bit samples, read as rbf_rice_decode reads it: the header and the table as
    rice_parse checks them, every chunk's codes inside its declared words, fewer than 32 bits left behind the last code and all of them 0."""
    buf = bytes(buf)
    key = (buf, count, bits)
    if key in _STREAMS:
        if _STREAMS[key] is None:
            raise ValueError("corrupt sample stream")
        return _STREAMS[key]
    _STREAMS[key] = None
    if len(buf) < 8 or len(buf) % 4:
        raise ValueError("stream length")
    n, b = struct.unpack_from("<IB", buf, 0)
    if n != count or b != bits or any(buf[5:8]):
        raise ValueError("stream head")
    c = -(-n // ref.CHUNK)
    hdr = (8 + 3 * c + 3) // 4 * 4
    if hdr > len(buf) or any(buf[8 + 3 * c:hdr]):
        raise ValueError("stream table")
    ks = list(buf[8:8 + c])
    words = [int(x) for x in np.frombuffer(buf, dtype="<u2", count=c, offset=8 + c)]
    for ci in range(c):
        nc = min(ref.CHUNK, n - ci * ref.CHUNK)
        if ks[ci] > bits or not 1 <= words[ci] <= (nc * bits + 31) // 32:
            raise ValueError("chunk table")
    if hdr + 4 * sum(words) != len(buf):
        raise ValueError("table against length")
    out, off, mask = np.empty(n, dtype=np.int64), hdr, (1 << bits) - 1
    for ci in range(c):
        nw, k = words[ci], ks[ci]
        val = int.from_bytes(buf[off:off + 4 * nw], "little")
        off += 4 * nw
        pos = 0
        for i in range(ci * ref.CHUNK, min(n, ci * ref.CHUNK + ref.CHUNK)):
            if k >= bits:
                u, pos = (val >> pos) & mask, pos + bits
            else:
                q = 0
                while q < ref.ESC and (val >> (pos + q)) & 1:
                    q += 1
                if q < ref.ESC:
                    u, pos = (q << k) | ((val >> (pos + q + 1)) & ((1 << k) - 1)), pos + q + 1 + k
                else:
                    u, pos = (val >> (pos + ref.ESC)) & mask, pos + ref.ESC + bits
            if pos > 32 * nw:
                raise ValueError("a code runs past its chunk's words")
            out[i] = u
        if 32 * nw - pos >= 32 or val >> pos:
            raise ValueError("words or set bits behind the last code")
    _STREAMS[key] = out
    return out


def _rice_key_frame(rec, near):
    """(frame, yuv) of a type-3 record, or of a type-7 one."""
    rec = bytes(rec)
    if near:
        h, w, item, channels, yuv, d, s = nk.parse(rec)
    else:
        if len(rec) < 14 + 8:
            raise ValueError("truncated")
        h, w, item, channels, yuv = struct.unpack_from("<IIIBB", rec, 0)
        d, s = None, rec[14:]
    if item not in (1, 2) or channels > 4 or yuv > 1 or h == 0 or w == 0:
        raise ValueError("head")
    n = max(1, channels)
    bits, dtype = 8 * item, (np.uint8 if item == 1 else np.uint16)
    shape = (h, w) if channels == 0 else (h, w, channels)
    u = _stream_u(s, h * w * n, bits)
    frame = nk.rebuild(u, shape, dtype, d) if near else ref.rebuild_scan(ref.from_u(u, bits), shape, bits).astype(dtype)
    return frame, bool(yuv)


def _rice_inter_frame(oracle, rec, prev):
    """_inter_frame for a type-4 record: residuals added at the mask's pixels; a stream that does not fit its mask is refused."""
    mask, d = _inter_mask(oracle, rec, prev)
    ch = prev.shape[2] if prev.ndim == 3 else 1
    bits = 8 * prev.dtype.itemsize
    u = _stream_u(d["values_z"], d["value_count"], bits)
    if d["value_count"] != int(mask.sum()) * ch:
        raise ValueError("residuals do not fit the mask")
    out = prev.copy()
    flat = out.reshape(mask.size, -1)
    flat[mask] = ((flat[mask].astype(np.int64) + ref.from_u(u, bits).reshape(-1, ch)) & ((1 << bits) - 1)).astype(prev.dtype)
    return out


def _pans(body, records, shape):
    """{record: (ox, oy)} of a pan table body against the frame records in front of it."""
    body = bytes(body)
    if len(body) < 16:
        raise ValueError("short")
    version, z0, z1, z2, count = struct.unpack_from("<BBBBI", body, 0)
    if version != 1 or z0 or z1 or z2 or len(body) != 8 + 12 * count + 8 or count == 0:
        raise ValueError("pan table head")
    if struct.unpack_from("<Q", body, len(body) - 8)[0] != integrity.frame_digest(body[:-8]):
        raise ValueError("pan table checksum")
    rows = [struct.unpack_from("<III", body, 8 + 12 * j) for j in range(count)]
    out = {}
    for j, (i, ox, oy) in enumerate(rows):
        if (j and i <= rows[j - 1][0]) or (ox == 0 and oy == 0) or i >= len(records) or records[i][0] not in INTERS:
            raise ValueError("pan entry")
        out[i] = (ox, oy)
    return out


def _trailer(body):
    body = bytes(body)
    version, algo, zero, count = struct.unpack_from("<BBHI", body, 0)
    if (version, algo, zero) != (1, 1, 0) or len(body) != 8 + 8 * count + 8:
        raise ValueError("trailer head")
    if struct.unpack_from("<Q", body, len(body) - 8)[0] != integrity.frame_digest(body[:-8]):
        raise ValueError("trailer checksum")
    return list(struct.unpack_from("<%dQ" % count, body, 8))


Decoded = collections.namedtuple("Decoded", "frames bad yuv")        # yuv: per frame, whether a decoder wraps it as a YUVFrame
_ERRORS = (ValueError, struct.error, zlib.error, IndexError, OverflowError, TypeError)


def twin_decode(oracle, records):
    """Decoded(frames, bad) -- bad: the frames whose digest is not the stored one, ascending, None without a trailer -- or raises Refused."""
    records = list(records)
    stored = None
    at = [i for i, (ty, _) in enumerate(records) if ty == DIGESTS]
    if at:
        if len(at) > 1 or at[0] != len(records) - 1:
            raise Refused(at[0], "a trailer is the last record, once")
        try:
            stored = _trailer(records[-1][1])
        except _ERRORS as e:
            raise Refused(at[0], str(e))
        records = records[:-1]
    pan_body, pan_at = None, [i for i, (ty, _) in enumerate(records) if ty == PANS]
    if pan_at:
        if len(pan_at) > 1 or pan_at[0] != len(records) - 1:
            raise Refused(pan_at[0], "a pan table stands directly behind the last frame record, once")
        pan_body, records = records[-1][1], records[:-1]
    if stored is not None and len(stored) != len(records):
        raise Refused(at[0], "the trailer covers other frames")
    if not records:
        raise Refused(0, "no frames")
    pans = {}
    if pan_body is not None:
        try:
            pans = _pans(pan_body, records, None)
        except _ERRORS as e:
            raise Refused(pan_at[0], str(e))
    for i, (ty, _) in enumerate(records):
        if ty not in KEYS + INTERS:
            raise Refused(i, "unknown type %d" % ty)
    if records[0][0] in INTERS:
        raise Refused(0, "an inter-frame without a keyframe")
    coded, yuv = [], []
    for i, (ty, rec) in enumerate(records):
        try:
            if ty == KEY:
                coded.append(_key_frame(rec))
                yuv.append(False)
            elif ty in (KEY_RICE, KEY_NEAR):
                f, y = _rice_key_frame(rec, ty == KEY_NEAR)
                coded.append(f)
                yuv.append(y)
            else:
                coded.append(_inter_frame(oracle, rec, coded[-1]) if ty == INTER else _rice_inter_frame(oracle, rec, coded[-1]))
                yuv.append(yuv[-1])
            if i in pans and not (pans[i][0] < coded[-1].shape[1] and pans[i][1] < coded[-1].shape[0]):
                raise ValueError("a pan offset outside the frame")
        except _ERRORS as e:
            raise Refused(i, str(e))
    frames = [np.roll(f, (pans[i][1], pans[i][0]), axis=(0, 1)) if i in pans else f for i, f in enumerate(coded)]
    bad = None if stored is None else [i for i, f in enumerate(coded) if integrity.frame_digest(f) != stored[i]]     # (the digests describe the coded frames)
    return Decoded(frames, bad, yuv)


def names_record(message, record):
    """Does the text name the record: `record R` or a range `records A..B` that holds it."""
    for a, b in re.findall(r"records? (\d+)(?:\.\.(\d+))?", message):
        if int(a) <= record <= int(b or a):
            return True
    return False


# ------------------------------------------------------------------ damages
Damage = collections.namedtuple("Damage", "name record kind blob")  # record: the record it is aimed at (None: the container's own framing); kind: a benign kind it may be, or None


def _fields(ty, rec):
    """[(name, offset, width)] of a record's fixed fields and [(name, offset, length)] of its payloads."""
    if ty == KEY:
        (size,) = struct.unpack_from("<I", rec, 12)
        return [("h", 0, 4), ("w", 4, 4), ("itemsize", 8, 4), ("zsize", 12, 4), ("has_yuv", 16 + size, 1)], [("zlib", 16, size)]
    if ty == DIGESTS:
        count = struct.unpack_from("<I", rec, 4)[0]
        return [("version", 0, 1), ("algo", 1, 1), ("reserved", 2, 2), ("count", 4, 4), ("checksum", 8 + 8 * count, 8)], [("digest0", 8, 8), ("digest_last", 8 * count, 8)]
    if ty in (KEY_RICE, KEY_NEAR):
        fields = [("h", 0, 4), ("w", 4, 4), ("itemsize", 8, 4), ("channels", 12, 1), ("yuv", 13, 1)]
        s0 = 14
        if ty == KEY_NEAR:
            nb = rec[15]
            fields += [("version", 14, 1), ("bound_count", 15, 1), ("bound0", 16, 2), ("bound_last", 14 + 2 * nb, 2)]
            s0 = (16 + 2 * nb + 3) // 4 * 4
        sf, sp = _stream_fields(rec, s0)
        return fields + sf, sp
    if ty == PANS:
        count = struct.unpack_from("<I", rec, 4)[0]
        return [("version", 0, 1), ("reserved", 1, 3), ("count", 4, 4), ("entry0_record", 8, 4), ("entry0_ox", 12, 4), ("entry0_oy", 16, 4),
                ("checksum", 8 + 12 * count, 8)], [("pan_entry", 8 + 12 * (count - 1), 12)]
    fields = [("width_byte", 0, 1), ("p", 1, 4), ("n", 5, 4), ("k", 9, 8), ("bitmap_bits", 17, 4), ("witness_bits", 21, 4), ("bitmap_size", 25, 4)]
    bsize = struct.unpack_from("<I", rec, 25)[0]
    off = 29 + bsize
    wsize = struct.unpack_from("<I", rec, off)[0]
    fields.append(("witness_size", off, 4))
    voff = off + 4 + wsize
    vsize = struct.unpack_from("<I", rec, voff)[0]
    fields += [("values_size", voff, 4), ("value_count", voff + 4, 4)]
    payloads = [("filter", 29, bsize)] + ([("witness", off + 4, wsize)] if wsize else [])
    if ty == INTER_RICE:
        sf, sp = _stream_fields(rec, voff + 8)
        return fields + sf, payloads + sp
    return fields, payloads + [("values", voff + 8, vsize)]


def _stream_fields(rec, s0):
    """The fields and payloads of the sample stream that starts at byte s0 of a record: N, B, the reserved bytes; the Rice table and
    the Rice payload."""
    n = struct.unpack_from("<I", rec, s0)[0]
    c = -(-n // ref.CHUNK)
    hdr = (8 + 3 * c + 3) // 4 * 4
    return [("stream_n", s0, 4), ("stream_bits", s0 + 4, 1), ("stream_reserved", s0 + 5, 3)], \
        [("rice_table", s0 + 8, 3 * c), ("rice_payload", s0 + hdr, len(rec) - s0 - hdr)]


K_VALUES = [("zero", 0.0), ("minus1", None), ("plus1", None), ("inf", float("inf")), ("nan", float("nan")), ("negative", -1.0), ("k64_5", 64.5),
            ("k65", 65.0), ("past32", 2.0 ** 32 + 3.5)]


def _with(records, i, rec):
    out = list(records)
    out[i] = (out[i][0], bytes(rec))
    return container.write(out)


def record_damages(records, i, tag):
    """The damages of record i: fields, cuts, bit flips."""
    ty, rec = records[i]
    rec = bytes(rec)
    fields, payloads = _fields(ty, rec)
    out = []

    def add(name, new, kind=None):
        if bytes(new) != rec and not any(d.name == "%s.%s" % (tag, name) for d in out):
            out.append(Damage("%s.%s" % (tag, name), i, kind, _with(records, i, new)))
    if ty == KEY:                                                  # the one head that still inflates to its byte count: another frame of the same bytes
        add("hw=swapped", rec[4:8] + rec[0:4] + rec[8:])
    for name, off, width in fields:
        if name == "k":
            (k,) = struct.unpack_from("<d", rec, off)
            for label, v in K_VALUES:
                v = k - 1 if label == "minus1" else k + 1 if label == "plus1" else v
                add("k=%s" % label, rec[:off] + struct.pack("<d", v) + rec[off + 8:], "unread_k" if tag.endswith("passthrough") else None)
            continue
        v = int.from_bytes(rec[off:off + width], "little")
        top = (1 << (8 * width)) - 1
        for label, nv in (("0", 0), ("-1", (v - 1) & top), ("+1", (v + 1) & top), ("max", top), ("topbit", v | (1 << (8 * width - 1)))):
            kind = "p" if name == "p" else "pad_or_unconsumed" if name == "witness_bits" and label in ("-1", "+1") else None
            add("%s=%s" % (name, label), rec[:off] + nv.to_bytes(width, "little") + rec[off + width:], kind)
    bounds = sorted({off for _, off, _ in fields} | {off + w for _, off, w in fields} | {off + ln for _, off, ln in payloads})
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut < len(rec):
                add("cut@%d" % cut, rec[:cut])
    rng = np.random.default_rng(len(rec))
    for name, off, ln in payloads:
        if ln == 0:
            continue
        for label, at in (("first", off), ("last", off + ln - 1), ("middle", off + int(rng.integers(0, ln)))):
            for bit in ((0, 7) if label == "last" else (int(rng.integers(0, 8)),)):     # the last byte: both ends, one of them may be a pad bit
                new = bytearray(rec)
                new[at] ^= 1 << bit
                add("%s.flip_%s_bit%d" % (name, label, bit), new, "pad_or_unconsumed" if name in ("filter", "witness") else None)
    return out


def framing_damages(c):
    """Damages of the container's own framing and of its list of records."""
    blob, recs = c.blob, c.records
    n = len(recs)
    out = []

    def add(name, new, record=None):
        out.append(Damage("container." + name, record, None, bytes(new)))
    for cut in (0, 3, 4, 6, 8, 10, 12, 13):
        add("cut@%d" % cut, blob[:cut])
    add("cut_last_byte", blob[:-1], n - 1)
    add("trailing_byte", blob + b"\0")
    add("count-1", blob[:4] + struct.pack("<I", n - 1) + blob[8:])
    add("count+1", blob[:4] + struct.pack("<I", n + 1) + blob[8:])
    add("count=max", blob[:4] + struct.pack("<I", 0xFFFFFFFF) + blob[8:])
    add("record0_length+1", blob[:8] + struct.pack("<I", struct.unpack_from("<I", blob, 8)[0] + 1) + blob[12:], 0)
    add("record0_length=topbit", blob[:8] + struct.pack("<I", struct.unpack_from("<I", blob, 8)[0] | 0x80000000) + blob[12:], 0)
    first_inter = c.coded[0]
    for i in (0, first_inter, n - 1):
        add("record%d_empty" % i, container.write(recs[:i] + [(recs[i][0], b"")] + recs[i + 1:]), i)
        add("record%d_zero_length" % i, _zero_length(recs, i), i)
    add("drop_key0", container.write(recs[1:]), 0)
    add("drop_key6", container.write(recs[:6] + recs[7:]), 6)
    add("drop_inter", container.write(recs[:first_inter] + recs[first_inter + 1:]), first_inter)
    add("double_inter", container.write(recs[:first_inter + 1] + recs[first_inter:]), first_inter + 1)
    add("double_key6", container.write(recs[:7] + recs[6:]), 7)
    add("swap_inters", container.write(recs[:1] + [recs[2], recs[1]] + recs[3:]), 1)
    add("swap_key_and_inter", container.write([recs[1], recs[0]] + recs[2:]), 0)
    add("type_of_inter=9", container.write(recs[:first_inter] + [(9, recs[first_inter][1])] + recs[first_inter + 1:]), first_inter)
    if recs[-1][0] == DIGESTS:
        add("double_trailer", container.write(recs + [recs[-1]]), n - 1)
        add("trailer_first", container.write([recs[-1]] + recs[:-1]), 0)
    return out


def _zero_length(recs, i):
    """The container with record i's length field 0 and no body at all (not even the type byte)."""
    out = [b"BFV2", struct.pack("<I", len(recs))]
    for j, (ty, rec) in enumerate(recs):
        body = b"" if j == i else struct.pack("<B", ty) + rec
        out += [struct.pack("<I", len(body)), body]
    return b"".join(out)


def damages(c, full=True):
    """Every damage of a container.  full=False: the list of records (dropped, doubled, swapped, emptied) and the FIELDS of one coded
    inter-frame and of one keyframe only -- the other configurations differ from the full one in sample width, mask and trailer, which those reach; the
    cuts and the bit flips walk the same parsers in every configuration."""
    recs = c.records
    if c.name.startswith("rice"):
        kinds = {ty: i for i, (ty, _) in enumerate(recs)}           # the last record of every type: no run hangs off the last keyframe
        groups = [("rice_key" if c.name.startswith("rice_pan") else "near_key", 12), ("rice_coded", c.coded[-1])]
        if full:
            groups += [("rice_passthrough", c.passthrough[0])] + ([("pans", kinds[PANS])] if PANS in kinds else [])
        return [d for tag, i in groups for d in record_damages(recs, i, tag) if full or "=" in d.name]
    if not full:
        return [d for d in framing_damages(c) if "cut@" not in d.name] + \
            [d for i, tag in ((c.coded[-1], "coded"), (12, "key")) for d in record_damages(recs, i, tag) if "=" in d.name]
    out = framing_damages(c)
    out += record_damages(recs, c.coded[0], "coded")
    out += record_damages(recs, 12, "key")                      # the last keyframe: no run hangs off it, so a frame it still decodes to is returned
    out += record_damages(recs, c.passthrough[0], "passthrough")
    if recs[-1][0] == DIGESTS:
        out += record_damages(recs, len(recs) - 1, "trailer")
    return out


FULL = ("u8_luma_digests", "rice_pan_digests", "rice_near_digests")
RICE_CONFIGS = [("rice_pan", True), ("rice_pan", False), ("rice_near", True), ("rice_near", False)]
# the configurations whose damages are cases: the full list on one, the reduced list on one of every sample width, mask and trailer
CASE_CONFIGS = [("u8", "luma", True), ("u8", "luma", False), ("u8", "all", False), ("u16", "luma", False), ("u16", "all", True)]


def all_cases(oracle):
    """[(Container, Damage)] of every configuration."""
    out = []
    for cfg in CASE_CONFIGS:
        c = build(oracle, *cfg)
        out += [(c, d) for d in damages(c, c.name in FULL)]
    for cfg in RICE_CONFIGS:
        c = build_rice(oracle, *cfg)
        out += [(c, d) for d in damages(c, c.name in FULL)]
    return out


# ------------------------------------------------------------------ classification
def classify(oracle, c, dmg):
    """("refused", record index or None) | ("other", Decoded) | ("benign", Decoded) -- by container.parse and the twin alone."""
    try:
        records = container.parse(dmg.blob)
    except ValueError:
        return "refused", None
    try:
        got = twin_decode(oracle, records)
    except Refused as e:
        return "refused", e.record
    same = not any(got.yuv) and len(got.frames) == len(c.frames) and all(f.shape == g.shape and f.dtype == g.dtype and np.array_equal(f, g) for f, g in zip(got.frames, c.frames))
    return ("benign" if same else "other"), got
