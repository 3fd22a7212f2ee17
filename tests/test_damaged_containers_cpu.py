"""tests/damaged_containers.py on the CPU: the host-built containers are what they claim, the twin decodes them to their frames, every
damage is classified by the product's parsers and the twin alone -- refused, decodes to other frames, or benign --, every benign case is
of a named kind and is proven to be, every record type has cases in the other two classes, and every refusal that the parsers can see
without a device is a plain ValueError that names its record.  Plus the parsers' own promises (container.parse, parse_record,
decompress_frame, params.filter_params, _native.params_array) on the inputs that used to raise something else."""
import collections
import struct
import zlib

import numpy as np
import pytest

import damaged_containers as dc
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd import params as P
from new_bloom_filter_repo_amd.frame_codec import FixedVideoCompressor, parse_record
from new_bloom_filter_repo_amd.sample_codec import parse_key_record, parse_near_key_record
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor, _inter_record, _naming
import bloom_params as bp
import foreign_decode as fd

# p: the density, which no decoder reads | pad bits behind bitmap_bits / witness_bits, and witness bits that no pass consumes | the k of
# a passthrough record: its bitmap is the mask, so its k is as informational as its p (a range check apart, which refuses inf, nan, < 0).
# A flipped FILTER bit is benign only where the pass set provably stays what it was (_proven_benign: no position's verdict depends on it)
BENIGN_KINDS = ("p", "pad_or_unconsumed", "unread_k")


@pytest.fixture(scope="module")
def cases(oracle):
    return dc.all_cases(oracle)


@pytest.fixture(scope="module")
def classes(oracle, cases):
    return [dc.classify(oracle, c, d) for c, d in cases]


def test_the_containers_are_what_they_claim(oracle):
    for cfg in dc.CONFIGS:
        c = dc.build(oracle, *cfg)
        types = [ty for ty, _ in c.records]
        assert types[:13] == [1, 2, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2, 1] and (types[13:] == [5]) == cfg[2]
        assert c.coded and c.passthrough == [dc.PASSTHROUGH_FRAME], "a Bloom-coded inter-frame and a passthrough one"
        assert container.parse(c.blob) == [(ty, bytes(r)) for ty, r in c.records]
        H, W, dtype = dc.SHAPES[cfg[0]]
        assert all(f.shape == (H, W, 3) and f.dtype == dtype for f in c.frames)
        got = dc.twin_decode(oracle, c.records)
        assert all(np.array_equal(a, b) for a, b in zip(got.frames, c.frames)) and len(got.frames) == 13
        assert got.bad == ([] if cfg[2] else None)
        chroma_alone = any(((a != b).any(axis=2) & ~dc.luma_mask(a, b)).any() for a, b in zip(c.frames, c.frames[1:]))
        assert chroma_alone == (cfg[1] == "all"), "the all-channel mask has something to say that the luma mask cannot"


def test_the_count_of_cases(cases):
    assert 300 <= len(cases) <= 2000, len(cases)
    names = [(c.name, d.name) for c, d in cases]
    assert len(set(names)) == len(names)
    full = [d.name for c, d in cases if c.name in dc.FULL]
    for group in ("container.", "key.", "coded.", "passthrough.", "trailer."):
        assert sum(n.startswith(group) for n in full) >= 20, group
    for what in ("cut@", "=0", "=-1", "=+1", "=max", "=topbit", "flip_first", "flip_last", "flip_middle", "_empty", "drop_", "double_", "swap_", "count-1", "count+1"):
        assert any(what in n for n in full), what


def _proven_benign(oracle, c, d):
    """The claim behind a benign verdict, from the bytes: which field or bit differs, and why no decoder may care."""
    good = parse_record("f64", bytes(c.records[d.record][1])[1:])
    bad = parse_record("f64", bytes(container.parse(d.blob)[d.record][1])[1:])
    differs = [k for k in good if (bytes(good[k]) != bytes(bad[k]) if isinstance(good[k], (np.ndarray, bytes)) else (good[k] != bad[k] and not (good[k] != good[k])))]
    if d.kind == "p":
        return differs in (["p"], [])                             # (a NaN p compares unequal to itself: nothing else differs)
    if d.kind == "unread_k":
        return differs == ["k"] and good["witness_bits"] == 0 and 0 <= bad["k"] < 65
    if differs == ["witness_bits"]:                                # the field moved inside its last byte: the line between the witness and its pad bits
        return (good["witness_bits"] + 7) // 8 == (bad["witness_bits"] + 7) // 8
    if differs == ["bitmap"]:
        at = int(np.flatnonzero(np.unpackbits(good["bitmap"]) != np.unpackbits(bad["bitmap"]))[0])
        if at >= good["bitmap_bits"]:                              # a pad bit behind bitmap_bits
            return True
        # a filter bit: benign only where every position whose verdict changes lies behind the last position that passes either way and
        # reads a pad bit of the witness -- no consumed witness bit moves, and the new passes read zeros
        if not good["witness_bits"]:
            return False
        h, m, n = bp.hashes(oracle, fd.SEEDS), good["bitmap_bits"], good["n"]
        floor_k, T = P.activation_threshold(good["k"])
        a, b = (bp.passing(h, np.unpackbits(x["bitmap"])[:m], m, int(floor_k), int(T), np.arange(n)) for x in (good, bad))
        changed, both = np.flatnonzero(a != b), np.flatnonzero(a & b)
        if not len(changed):                                       # a filter bit on which no position's verdict depends: the pass set is the same
            return True
        return changed[0] > both[-1] and int(a.sum()) >= good["witness_bits"] and not a[changed].any()
    if differs == ["witness"]:
        at = int(np.flatnonzero(np.unpackbits(good["witness"]) != np.unpackbits(bad["witness"]))[0])
        return at >= good["witness_bits"]                          # a pad bit behind witness_bits: an encoder's witness is as long as the pass count
    return False


def test_every_case_is_classified_and_every_benign_one_is_of_a_named_kind(oracle, cases, classes):
    per_type = collections.defaultdict(collections.Counter)
    counts = collections.Counter()
    for (c, d), (cls, what) in zip(cases, classes):
        counts[cls] += 1
        group = d.name.split(".")[0]
        per_type[group][cls] += 1
        if cls == "benign":
            assert d.kind in BENIGN_KINDS and _proven_benign(oracle, c, d), (c.name, d.name, "benign, and of no named kind")
    assert counts["refused"] > counts["other"] > 0 and counts["benign"] > 0, counts
    for group in ("key", "coded", "passthrough", "container", "rice_key", "near_key", "rice_coded", "rice_passthrough"):
        assert per_type[group]["refused"] and per_type[group]["other"], (group, per_type[group])
    # a trailer and a pan table are covered by their own checksums: no damage of one decodes to other frames -- a damaged digest or pan
    # ENTRY is refused like any other byte of them
    for group in ("trailer", "pans"):
        assert per_type[group]["refused"] and not per_type[group]["other"] and not per_type[group]["benign"], group


def test_other_frames_are_caught_by_a_trailer(oracle, cases, classes):
    """With frame_digests the container proves itself: a damage that still decodes, to other frames, shows in the twin's
    list of frames whose digest is not the stored one -- from the damaged frame to the end of its run."""
    seen = 0
    for (c, d), (cls, what) in zip(cases, classes):
        if cls != "other" or what.bad is None:
            continue
        differing = [i for i, (f, g) in enumerate(zip(what.frames, c.frames)) if f.shape != g.shape or not np.array_equal(f, g) or what.yuv[i]]
        if d.name == "key.hw=swapped" or ".yuv=" in d.name:
            # FOUND HERE, and left as it is: FD1 is defined over a frame's bytes, not its geometry or its wrapper.  A keyframe
            # head that reads the same bytes as W x H instead of H x W, or a yuv byte of 1 (the frame comes back as a YUVFrame), decodes
            # to another frame with the stored digest.
            assert differing == [12] and what.bad == [] and what.frames[12].tobytes() == c.frames[12].tobytes()
            continue
        if len(what.frames) == len(c.frames):
            assert what.bad == differing and differing, (c.name, d.name)
            if c.name.startswith("rice_pan"):                      # (rolled frames: a coded frame that differs is a frame that differs)
                pass
            ends = [6, 12, 13]
            assert differing == list(range(differing[0], min(e for e in ends if e > differing[0]))), (c.name, d.name, differing)
            seen += 1
    assert seen >= 10


def _product_refuses(c, d, record):
    """What the product's own parsers say without a device: container.parse, split_tables, check_types, and per record decompress_frame /
    _inter_record against the GOOD frame in front of it.  Returns the message, or None when the parsers see nothing."""
    try:
        records = container.parse(d.blob)
        frames, _, _ = container.split_tables(records)
        container.check_types([ty for ty, _ in frames])
    except ValueError as e:
        assert type(e) is ValueError
        return str(e)
    keys = FixedVideoCompressor(verbose=False)
    if record is not None and record < len(frames):
        ty, rec = frames[record]
        try:                                                       # the decoder's own route to the parsers: _naming puts the index in, not this test
            if ty in dc.KEYS:
                with _naming(record):
                    {dc.KEY: keys.decompress_frame, dc.KEY_RICE: parse_key_record, dc.KEY_NEAR: parse_near_key_record}[ty](rec)
            else:
                prev = c.frames[min(record, len(c.frames)) - 1]
                ImprovedVideoCompressor._parse_run(prev, [rec], [ty], first=record)
        except ValueError as e:
            assert type(e) is ValueError
            return str(e)
    return None


def test_refusals_are_plain_value_errors_from_the_products_parsers(oracle, cases, classes):
    """Every refused case, here on the CPU: the parsers raise ValueError and nothing else.  What only a decode can see -- a value stream
    that does not inflate, a value count that does not fit the decoded mask of a single-channel frame -- is counted, not skipped: the
    GPU tier holds it."""
    seen = collections.Counter()
    for (c, d), (cls, what) in zip(cases, classes):
        if cls != "refused":
            continue
        msg = _product_refuses(c, d, what)
        group = d.name.split(".")[0]
        if msg is None:
            bad = container.parse(d.blob)[what]
            assert bad[0] in dc.INTERS + (dc.KEY_RICE, dc.KEY_NEAR), (c.name, d.name, "a refusal the parsers do not see lies in a value field or a sample stream")
            seen["decode"] += 1
        else:
            seen["parsers"] += 1
            assert what is None or "record" in msg, (c.name, d.name, msg)
            # the text names the record the twin refuses.  Not held for a changed LIST of records (more than one record may be the first to
            # fail) nor for the pan table, whose entries' errors name the record an entry points at
            if what is not None and group not in ("container", "pans"):
                assert dc.names_record(msg, what), (c.name, d.name, what, msg)
                seen["named"] += 1
    assert seen["parsers"] > seen["decode"] > 0 and seen["named"] > 500, seen


# ------------------------------------------------------------------ the parsers' own promises
def test_container_parse_refuses_what_is_no_whole_container(oracle):
    c = dc.build(oracle, "u8", "luma", False)
    blob = c.blob
    for cut in (0, 3, 4, 6, 8, 10, 12, 13, len(blob) - 1):
        with pytest.raises(ValueError):
            container.parse(blob[:cut])
    for bad in (blob + b"\0", blob[:4] + struct.pack("<I", 14) + blob[8:], blob[:4] + struct.pack("<I", 0xFFFFFFFF) + blob[8:],
                blob[:4] + struct.pack("<I", 12) + blob[8:], dc._zero_length(c.records, 1)):
        with pytest.raises(ValueError) as e:
            container.parse(bad)
        assert type(e.value) is ValueError
    with pytest.raises(ValueError, match="record 1 of 13 is empty"):
        container.parse(dc._zero_length(c.records, 1))
    with pytest.raises(ValueError, match="record 0 of 13 declares"):
        container.parse(blob[:8] + struct.pack("<I", 1 << 31) + blob[12:])
    assert container.parse(b"BFVC" + struct.pack("<I", 0)) == []


def test_parse_record_refuses_every_cut_and_every_wrong_byte_count(oracle):
    c = dc.build(oracle, "u8", "luma", False)
    rec = bytes(c.records[c.coded[0]][1])[1:]
    good = parse_record("f64", rec)
    assert len(good["bitmap"]) == (good["bitmap_bits"] + 7) // 8 and len(good["witness"]) == (good["witness_bits"] + 7) // 8
    for cut in range(len(rec)):
        with pytest.raises(ValueError) as e:
            parse_record("f64", rec[:cut])
        assert type(e.value) is ValueError, cut
    with pytest.raises(ValueError):
        parse_record("f64", rec + b"\0")
    for off in (24, 28 + len(good["bitmap"])):                     # the two byte counts
        for v in (0, 1 << 31, 0xFFFFFFFF):
            with pytest.raises(ValueError):
                parse_record("f64", rec[:off] + struct.pack("<I", v) + rec[off + 4:])
    ref = parse_record("reference", rec[:8] + struct.pack("<f", good["k"]) + rec[16:])
    assert ref["bitmap_bits"] == good["bitmap_bits"] and bytes(ref["values_z"]) == bytes(good["values_z"])


def test_decompress_frame_refuses_cut_and_flipped_records(oracle):
    c = dc.build(oracle, "u8", "luma", False)
    rec = bytes(c.records[0][1])
    keys = FixedVideoCompressor(verbose=False)
    assert np.array_equal(keys.decompress_frame(rec), c.frames[0])
    rng = np.random.default_rng(9)
    for cut in sorted({0, 3, 4, 11, 12, 15, 16, 17, len(rec) - 2, len(rec) - 1} | {int(x) for x in rng.integers(0, len(rec), 20)}):
        with pytest.raises(ValueError) as e:
            keys.decompress_frame(rec[:cut])
        assert type(e.value) is ValueError, cut
    for at in [int(x) for x in rng.integers(16, len(rec) - 1, 40)]:
        bad = bytearray(rec)
        bad[at] ^= 1 << int(rng.integers(0, 8))
        try:
            got = keys.decompress_frame(bytes(bad))
        except ValueError as e:
            assert type(e) is ValueError
        else:                                                      # zlib's own checksum: a flip that inflates at all inflates to the frame
            assert np.array_equal(got, c.frames[0])


def test_filter_params_and_params_array_refuse_what_the_abi_cannot_take():
    for k in (float("inf"), float("-inf"), float("nan"), 2.0 ** 32 + 3.5, 65.0, -0.5, np.float64("inf"), np.float32("nan")):
        with pytest.raises(ValueError):
            P.filter_params(k, 100)
    for l in (-1, 1 << 32, (1 << 32) + 1):
        with pytest.raises(ValueError):
            P.filter_params(2.5, l)
    assert P.filter_params(64.5, 100)[:2] == (100, 64) and P.filter_params(0, 0) == (0, 0, 0) and P.filter_params(2.0, (1 << 32) - 1)[0] == (1 << 32) - 1
    for row in (((1 << 32) + 1, 1, 0), (100, (1 << 32) + 3, 0), (100, 1, 1 << 64), (-1, 1, 0)):
        with pytest.raises(ValueError):
            nat.params_array([(100, 1, 0), row])
    arr = nat.params_array([((1 << 32) - 1, 64, (1 << 64) - 1)])
    assert (arr[0].m, arr[0].floor_k, arr[0].threshold) == ((1 << 32) - 1, 64, (1 << 64) - 1)


def test_a_passthrough_mask_loses_its_pad_bits_before_it_reaches_a_device(oracle):
    """The scatter walks every set bit of a mask's last word: a pad bit behind bit n of a passthrough bitmap would be a pixel past the
    frame.  _inter_record clears them (n = 2211: five pad bits)."""
    c = dc.build(oracle, "u8", "luma", False)
    i = c.passthrough[0]
    rec = bytearray(c.records[i][1])
    d = _inter_record(bytes(rec), 2211, np.uint8, False)
    at = 1 + 28 + len(d["bitmap"]) - 1                            # the bitmap's last byte
    rec[at] |= 0x1F
    got = _inter_record(bytes(rec), 2211, np.uint8, False)
    assert np.array_equal(got["bitmap"], d["bitmap"]) and not (got["bitmap"][-1] & 0x1F)
    for n_bits in (2210, 2212, 0):
        bad = bytes(rec[:18]) + struct.pack("<I", n_bits) + bytes(rec[22:])
        with pytest.raises(ValueError):
            _inter_record(bad, 2211, np.uint8, False)
    with pytest.raises(ValueError):
        _inter_record(bytes([2]) + bytes(rec[1:]), 2211, np.uint8, False)
    assert zlib.decompress(d["values_z"])


def test_whatever_a_record_raises_comes_out_as_a_value_error_that_names_it():
    from new_bloom_filter_repo_amd.integrity import IntegrityError
    from new_bloom_filter_repo_amd.video_compressor import _naming
    for exc, first, last, want in ((struct.error("x"), 3, None, "record 3: x"), (ValueError("record 5: y"), 3, None, "record 5: y"),
                                   (ValueError("y"), None, None, "y"), (zlib.error("z"), None, None, "z"), (IndexError("i"), 1, 1, "record 1: i"),
                                   (OverflowError("o"), 0, 5, "records 0..5: o"),
                                   (nat.RbfError(nat.RBF_ERANGE, "floor_k 70 > 64"), 2, 4, "records 2..4: librbf_hip error -34: floor_k 70 > 64")):
        with pytest.raises(ValueError) as e:
            with _naming(first, last):
                raise exc
        assert type(e.value) is ValueError and str(e.value) == want
    with pytest.raises(nat.RbfError):                              # the device's own trouble is no property of the record
        with _naming(1):
            raise nat.RbfError(nat.RBF_ENOMEM, "out of memory")
    with pytest.raises(IntegrityError):
        with _naming(1):
            raise IntegrityError(4, 1, 2, key_record=0)
