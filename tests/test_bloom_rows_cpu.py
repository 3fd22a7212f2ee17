"""tests/bloom_rows.py on the CPU: the placement helper round-trips, the layout set covers what the GPU sweep (tests/
test_gpu_bloom_row_sweep.py) claims, the batches reach both kernel families, the planner sends every (knob, batch) where KERNELS says,
every decoy matters, and every mutant row-address rule fetches other bytes than the true one wherever it forms another address -- so a
kernel with that mistake cannot pass the sweep."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import block_layout as bl
import bloom_rows as br
import plan_boundaries as pb
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd.dist import unpack_device_record
from test_block_layout_cpu import HostBlock


class HostBuffer:
    """A stand-in for a DeviceBuffer: the bytes a Block uploads, at address 4096."""

    def __init__(self, nbytes):
        self.ptr, self.raw = 4096, np.zeros(nbytes, np.uint8)

    def upload(self, arr, offset=0):
        self.raw[offset:offset + arr.nbytes] = arr

    def download(self, nbytes, offset=0):
        return self.raw[offset:offset + nbytes].copy()


# ------------------------------------------------------------------ the placement helper
def test_a_block_round_trips_and_shows_a_written_guard():
    rng = np.random.default_rng(1)
    for stride, base in ((24, 0), (24, 8), (4128, 8)):
        blk = br.Block(3, stride, base)
        assert blk.nbytes == 2 * br.GUARD + base + 3 * stride and [blk.offset(f) for f in range(3)] == [br.GUARD + base + f * stride for f in range(3)]
        rows = [rng.integers(0, 256, k, dtype=np.uint8) for k in (24, 16, 8)]
        buf = HostBuffer(blk.nbytes)
        assert blk.place(buf, rows) == buf.ptr + br.GUARD + base
        raw = blk.fetch(buf)
        assert blk.guards_are_poison(raw)
        for f, r in enumerate(rows):
            assert np.array_equal(blk.row(raw, f, r.nbytes), r) and (blk.row(raw, f)[r.nbytes:] == br.POISON).all()
        for at in (0, blk.first - 1, blk.first + 3 * stride, blk.nbytes - 1):       # in front of the rows (the base included) and behind them
            buf.raw[at] ^= 1
            assert not blk.guards_are_poison(blk.fetch(buf)), at
            buf.raw[at] ^= 1
        buf.raw[blk.first] ^= 1                                    # a row's own byte is no guard
        assert blk.guards_are_poison(blk.fetch(buf))


# ------------------------------------------------------------------ the layout set
def test_the_layouts_cover_every_value_and_every_ordered_pair_of_roles():
    L = br.LAYOUTS
    assert len(L) == 8 and len(set(br.LAYOUT_IDS)) == 8
    assert L[0] == br.Layout("engine", br.PLAIN, br.PLAIN, br.PLAIN, 0, 0, 0) and not any(br.is_odd(L[0], r) for r in br.ROLES)
    for role in br.ROW_ROLES:
        assert {getattr(lay, role).kind for lay in L} == set(br.STRIDE_KINDS), role
        assert {getattr(lay, role).base for lay in L} == set(br.BASES), role
    for role in ("stats", "ones", "record"):
        assert {getattr(lay, role) for lay in L} == set(br.BASES), role
    for a, b in itertools.permutations(br.ROLES, 2):
        assert any(not br.is_odd(lay, a) and br.is_odd(lay, b) for lay in L), "no layout has %s plain and %s odd" % (a, b)
    assert {br.decode_witness_kind(lay) for lay in L} == {"tight", "plus8", "wide"} and br.decode_witness_kind(L[0]) == "tight"
    assert br.stride_of("min", 4856) == 4856 and br.stride_of("plus8", 4856) == 4864 and br.stride_of("wide", 4856) == 4864 + 4096 + 16


@pytest.mark.parametrize("W,H", br.SIZES, ids=br.SIZE_IDS)
def test_the_batches_reach_both_families_and_both_paths_of_the_reduce_kernel(oracle, W, H):
    n = W * H
    frames = br.batch(oracle, W, H)
    assert n % 64 == (0 if W == 512 else 61)
    ms = [fr.m for fr in frames]
    assert all(ms[f] >= br.F64_MIN for f in (0, 1, 5)) and all(2 <= ms[f] < br.F64_MIN for f in (2, 3)) and ms[br.PASSTHROUGH] == 0, ms
    assert frames[br.PASSTHROUGH].ones >= oracle.P_STAR * n
    # the parameters are the library's own host planner's
    par = (nat.FilterParams * 6)()
    ones = (ctypes.c_uint64 * 6)(*[fr.ones for fr in frames])
    ks = (ctypes.c_double * 6)()
    assert nat.lib().rbf_plan_batch(n, ones, 6, 1, par, ks) == 0
    for f, fr in enumerate(frames):
        assert par[f].m == fr.m and (not fr.m or (par[f].floor_k, par[f].threshold, ks[f]) == (fr.floor_k, fr.T, fr.k)), f
        assert 0 < fr.witness_bits < n or not fr.m
    mask_s, filt_s, wit_s, tight = br.minimal_strides(frames)
    assert (mask_s, wit_s) == (nat.packed_stride(n), nat.packed_stride(n)) and filt_s == max(nat.packed_stride(m) for m in ms)
    assert 8 <= tight < nat.packed_stride(n), "the decode's own witness stride is below ceil(n / 64) * 8"
    assert {nat.packed_stride(m) % 16 for m in ms if m} == {0, 8}, "the batch's own filter rows end on both residues"
    # k_filter_reduce: the scalar path and the vector path, the second with an aligned and a far-apart stride
    paths = {(br.reduce_takes_vectors(br.row_blocks(lay, frames)["filters"]), lay.filters.kind) for lay in br.LAYOUTS}
    assert filt_s % 16 == 8 and paths >= {(False, "min"), (True, "plus8"), (False, "wide")}, paths
    # the last mask word's pad bits are zero, and the witness rows are zero behind their last bit
    for fr in frames:
        assert not np.unpackbits(br.mask_row(fr))[n:].any() and not np.unpackbits(fr.witness)[fr.witness_bits:].any()
        assert fr.filter.nbytes == nat.packed_stride(fr.m) and fr.witness.nbytes == nat.packed_stride(fr.witness_bits)


def test_more_rows_than_one_launch_sequence_takes(oracle):
    W, H, F = br.MANY
    frames = br.batch(oracle, W, H, F)
    assert F == br.MAX_BATCH + 2 and all(fr.m for fr in frames[br.MAX_BATCH:]), "the second chunk's two rows are coded"
    assert sum(1 for fr in frames if not fr.m) == 21, "passthrough rows in the first chunk"
    assert len({fr.mask.tobytes() for fr in frames}) == F, "no two rows alike: a chunk that starts at the wrong row shows"


# ------------------------------------------------------------------ which kernels a (knob, batch) lands on
@pytest.fixture(scope="module")
def plan_cases(tmp_path_factory):
    if pb.GXX is None:
        pytest.skip("g++ not found: tests/c/plan_cases.cpp is built with a plain host compiler")
    return pb.build_plan_cases(tmp_path_factory.mktemp("bloom_rows_plan"))


@pytest.mark.parametrize("known", [0, 1], ids=["counts_unknown", "counts_known"])
@pytest.mark.parametrize("W,H", br.SIZES, ids=br.SIZE_IDS)
def test_the_planner_sends_every_knob_where_the_table_says(oracle, plan_cases, W, H, known):
    assert br.KNOBS == list(br.KERNELS) == list(br.KERNELS_KNOWN) and len(br.KNOB_IDS) == len(br.KNOBS)
    ms = [fr.m for fr in br.batch(oracle, W, H)]
    text = "".join("batch %d %d %d %d %d %s\n" % (W * H, pb.CUS, knob, known, len(ms), " ".join(map(str, ms))) for knob in br.KNOBS)
    out = subprocess.run([plan_cases], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    at = 0
    for knob in br.KNOBS:
        split, first, second = (br.KERNELS_KNOWN if known else br.KERNELS)[knob]
        head = dict(f.split("=") for f in lines[at][1:])
        assert lines[at][0] == "batch" and head["mixed"] == "1"
        got = {ln[0]: dict(f.split("=") for f in ln[1:])["decision"] for ln in lines[at + 1:at + 4]}
        at += 4
        # encode and decode take the same road (the decode never knows the counts: its FP64 half is the counts-unknown one)
        assert (head["encode_split"], head["decode_split"]) == (str(int(split)),) * 2, (hex(knob), head)
        if split:
            assert (got["small"], got["big"]) == (first, second), (hex(knob), got)
        else:
            assert got["plan"] == first, (hex(knob), got)
    assert at == len(lines)
    # between them the knobs reach every insert kernel and every query kernel
    table = (br.KERNELS_KNOWN if known else br.KERNELS).values()
    decisions = [d.split(".") for _, a, b in table for d in (a, b) if d]
    assert {d[1] for d in decisions} == {"0", "1", "2", "3"} and {(d[0], d[3], d[4]) for d in decisions} >= {("0", "0", "0"), ("1", "0", "0"), ("1", "1", "0")}
    assert (("1", "1", "1") in {(d[0], d[3], d[4]) for d in decisions}) == bool(known)


# ------------------------------------------------------------------ mutant address rules
def placed(block, rows):
    buf = HostBuffer(block.nbytes)
    block.place(buf, rows)
    return block.fetch(buf)


@pytest.mark.parametrize("W,H", br.SIZES, ids=br.SIZE_IDS)
def test_every_mutant_address_rule_fetches_other_bytes(oracle, W, H):
    frames = br.batch(oracle, W, H)
    payload = {"masks": [br.mask_row(fr) for fr in frames], "filters": [fr.filter for fr in frames], "witnesses": [fr.witness for fr in frames]}
    caught = set()
    for lay in br.LAYOUTS:
        for decode in (False, True):
            blocks = br.row_blocks(lay, frames, decode)
            for role in br.ROW_ROLES:
                raw = placed(blocks[role], payload[role])
                for name in br.MUTANTS:
                    v = br.mutant_verdict(blocks[role], raw, name, 8)
                    assert v is not False, "%s: a reader of the %s rows with %s would pass" % (lay.name, role, name)
                    if v:
                        caught.add((role, name))
    near = [m for m in br.MUTANTS if m != "stride_in_32_bits"]      # (a near stride fits 32 bits: the far rows catch that one, below)
    assert caught == {(role, m) for role in br.ROW_ROLES for m in near}, "every mistake is caught for every role by some layout"


@pytest.mark.parametrize("place", sorted(br.FAR_PLACES))
def test_a_far_offset_kept_in_32_bits_lands_on_a_decoy(oracle, place):
    frames = br.batch(oracle, *br.SIZES[1])
    for role in br.ROW_ROLES:
        nbytes = br.far_row_bytes(frames, role)
        lay = br.far_layout(place, nbytes)
        assert lay.count == br.FAR_PLACES[place] == len(br.FAR_CODED[place]) and len(lay.decoys) == len(br.FAR_DECOYS[place]) and nbytes <= bl.ROW_MAX
        rows = br.far_rows([frames[f] for f in br.FAR_CODED[place]], role, nbytes)
        decoys = br.far_rows([frames[f] for f in br.FAR_DECOYS[place]], role, nbytes)
        buf = HostBlock(bl.far_masks_nbytes() if place == "rows" else bl.far_frames_nbytes())
        lay.place(buf, rows, decoys)
        differs = 0
        for f in range(lay.count):
            true, mutant = br.TRUE_RULE(lay.base, lay.stride, f), br.MUTANTS["stride_in_32_bits"](lay.base, lay.stride, f)
            assert true == lay.items[f]
            if mutant != true:
                assert mutant in [o for o, _ in lay.decoys], "the truncated address is a decoy's"
                assert not np.array_equal(buf.download(nbytes, mutant), buf.download(nbytes, true))
                differs += 1
        assert differs >= 1 and lay.stride * (lay.count - 1) >= 1 << 32


def test_a_stride_with_nearly_empty_low_32_bits_wraps_into_row_0(oracle):
    frames = br.batch(oracle, *br.SIZES[1])
    rows = br.far_rows([frames[f] for f in br.FAR_CODED["rows"]], "masks", br.far_row_bytes(frames, "masks"))
    nb = rows[0].nbytes
    for stride in br.WRAPPING_STRIDES:
        assert stride % 8 == 0 and stride >= 1 << 32 and (stride & 0xFFFFFFFF) < (frames[0].mask.size + 7) // 8, "legal, and its low half is shorter than a row"
        at = br.MUTANTS["stride_in_32_bits"](0, stride, 1)
        assert at + 8 <= nb and not np.array_equal(rows[0][at:at + nb - at], rows[1][:nb - at]), "row 1's truncated address holds other bytes"
        assert stride + nb + (1 << 16) <= bl.far_masks_nbytes()


@pytest.mark.parametrize("W,H", br.SIZES, ids=br.SIZE_IDS)
def test_a_reader_of_the_whole_stride_counts_other_ones(oracle, W, H):
    n = W * H
    frames = br.batch(oracle, W, H)
    seen = 0
    for lay in br.LAYOUTS:
        blk = br.row_blocks(lay, frames)["masks"]
        raw = placed(blk, [br.mask_row(fr) for fr in frames])
        for f, fr in enumerate(frames):
            assert br.ones_in(blk.row(raw, f), (n + 7) // 8) == fr.ones
            if blk.stride > nat.packed_stride(n):
                assert br.ones_in(blk.row(raw, f), blk.stride) != fr.ones, "the poison behind the payload counts"
                seen += 1
    assert seen == 6 * sum(1 for lay in br.LAYOUTS if lay.masks.kind != "min")


# ------------------------------------------------------------------ far rows: every decoy matters
@pytest.mark.parametrize("place", sorted(br.FAR_PLACES))
def test_every_decoy_of_an_input_role_changes_the_expected_output(oracle, place):
    frames = br.batch(oracle, *br.SIZES[1])
    coded, through, decoys = br.FAR_CODED[place], br.FAR_PASSTHROUGH[place], br.FAR_DECOYS[place]
    assert all(frames[f].m for f in coded[1:]) and all(frames[f].m for f in decoys) and not any(frames[f].m for f in through[1:])
    for f, d in zip(coded[1:], decoys):                            # far row j stands at coded[j], its decoy holds frame decoys[j - 1]'s row
        fr, other = frames[f], frames[d]
        # encode reads the decoy mask: another filter and another witness
        filt, bits, wit = br.encoded_with(oracle, other.mask, fr)
        assert not np.array_equal(filt, fr.filter) and (bits, wit.tobytes()) != (fr.witness_bits, fr.witness.tobytes())
        # decode reads the decoy filter, or the decoy witness: another mask
        fs, ws = br.far_row_bytes(frames, "filters"), br.far_row_bytes(frames, "witnesses")
        own_f, own_w = br.far_rows([fr], "filters", fs)[0], br.far_rows([fr], "witnesses", ws)[0]
        dec_f, dec_w = br.far_rows([other], "filters", fs)[0], br.far_rows([other], "witnesses", ws)[0]
        assert np.array_equal(br.decoded(oracle, fr, own_f, own_w), fr.mask)
        assert not np.array_equal(br.decoded(oracle, fr, dec_f, own_w), fr.mask) and not np.array_equal(br.decoded(oracle, fr, own_f, dec_w), fr.mask)
        # pack copies the decoy row: other record bytes
        assert not np.array_equal(dec_f[:fr.filter.nbytes], fr.filter) and not np.array_equal(dec_w[:fr.witness.nbytes], fr.witness)
    for f, d in zip(through[1:], decoys):                          # pack reads the mask row of the frame that is passed through
        assert not np.array_equal(br.mask_row(frames[d]), br.mask_row(frames[f]))


# ------------------------------------------------------------------ the record and the sequence
@pytest.mark.parametrize("W,H", br.SIZES, ids=br.SIZE_IDS)
def test_the_expected_record_parses_back_to_the_rows(oracle, W, H):
    frames = br.batch(oracle, W, H)
    for skipped in ((), (2,)):
        rows = unpack_device_record(br.record_bytes(frames, skipped), W * H)
        assert len(rows) == 6
        for f, (g, fr) in enumerate(zip(rows, frames)):
            if f in skipped:
                assert g.get("skipped") and g["witness_bits"] == 0 and "filter" not in g and "mask" not in g
                continue
            assert (g["l"], g["floor_k"], g["threshold"], g["k"], g["witness_bits"], g["filter_ones"]) == (fr.m, fr.floor_k, fr.T, fr.k, fr.witness_bits, fr.filter_ones)
            assert np.array_equal(g["witness"], fr.witness[:(fr.witness_bits + 7) // 8])
            assert np.array_equal(g["filter"], fr.filter[:(fr.m + 7) // 8]) if fr.m else np.array_equal(g["mask"], br.mask_row(fr)[:(W * H + 7) // 8])


def test_the_sequence_shrinks_grows_and_changes_family(oracle):
    steps = [br.SEQUENCE[i] for i in br.SEQUENCE_ORDER]
    assert br.SEQUENCE_ORDER[0] == br.SEQUENCE_ORDER[-1] and len(set(br.SEQUENCE_ORDER)) == len(br.SEQUENCE)
    pixels, counts = [W * H for W, H, _, _ in steps], [F for _, _, F, _ in steps]
    for seq in (pixels, counts):
        assert any(b < a for a, b in zip(seq, seq[1:])) and any(b > a for a, b in zip(seq, seq[1:])), seq
    assert [g for _, _, _, g in br.SEQUENCE] == [0, 0, 1, 0], "one step on the generic kernels between LDS ones"
    largest = [max(fr.m for fr in br.batch(oracle, W, H, F)) for W, H, F, _ in steps]
    assert any(m >= br.F64_MIN for m in largest) and any(m < br.F64_MIN for m in largest), "probe images and partial filters shrink and grow"
