"""Pan alignment without a GPU: the reference (pan_ref.py) by hand, the tie-break, the rule and the accumulation (container.pan_offsets), the
pan table's round trip and every refusal, the keyword's validation, the additive C ABI entries, the new kernels' resources, and the
properties of the clips the GPU tests rely on."""
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pan_ref
from conftest import REPO
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.integrity import build_trailer
from new_bloom_filter_repo_amd.synthetic import make_camera_gop, make_panning_gop
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor


def row(dx, dy, mz, mb):
    r = np.zeros((), dtype=nat.PAN_ROW)
    r["dx"], r["dy"], r["moving_zero"], r["moving_best"] = dx, dy, mz, mb
    return r


def test_reference_by_hand_on_5x4():
    """W = 5, H = 4, R = 1: the grid is x in {1}, y in {1}: one point (8 > W - 2).  prev(1, 1) = 7; cur holds 7 at (2, 1) only."""
    prev = np.zeros((4, 5), dtype=np.uint8)
    cur = np.full((4, 5), 100, dtype=np.uint8)
    prev[1, 1] = 7
    cur[1, 2] = 7
    xs, ys = pan_ref.grid_points(5, 4, 1)
    assert list(xs) == [1] and list(ys) == [1]
    t = pan_ref.sad_table(prev, cur, 1)
    assert len(t) == 9 and t[(1, 0)] == 0 and all(v == 93 for k, v in t.items() if k != (1, 0))
    assert pan_ref.pick(t) == (1, 0)
    # moving: cyclic.  cur rolled by (1, 0): new(x, y) = cur(x + 1, y): the 7 lands on (1, 1), where prev holds 7; every other pixel is 100 vs 0
    assert np.array_equal(pan_ref.roll(cur, 1, 0)[1], [100, 7, 100, 100, 100])
    assert pan_ref.moving(prev, cur, (1, 0)) == 19 and pan_ref.moving(prev, cur, (0, 0)) == 20
    assert pan_ref.moving(prev, cur, (1, 0), tolerance=100) == 0 and pan_ref.moving(prev, cur, (1, 0), tolerance=99) == 19
    # 16 bits: the true absolute difference, not the int16 wrap
    a, b = np.zeros((4, 5), dtype=np.uint16), np.full((4, 5), 0x8000, dtype=np.uint16)
    assert pan_ref.sad_table(a, b, 1)[(0, 0)] == 0x8000 and pan_ref.moving(a, b, (0, 0), tolerance=0x7FFF) == 20


def test_tie_break_order():
    t = {(dx, dy): 5 for dx in range(-2, 3) for dy in range(-2, 3)}
    assert pan_ref.pick(t) == (0, 0)                                  # (0, 0) wins every tie
    del t[(0, 0)]
    assert pan_ref.pick(t) == (-1, 0)                                 # |dx|+|dy| = 1: |dy| = 0 first, then dx ascending
    del t[(-1, 0)], t[(1, 0)]
    assert pan_ref.pick(t) == (0, -1)                                 # then dy ascending
    del t[(0, -1)], t[(0, 1)]
    assert pan_ref.pick(t) == (-2, 0)                                 # |dx|+|dy| = 2, |dy| = 0
    t[(2, 2)] = 4
    assert pan_ref.pick(t) == (2, 2)                                  # the SAD comes first
    flat = [np.full((20, 24, 3), 9, dtype=np.uint8)] * 2
    assert pan_ref.stat_rows(flat, 4) == [dict(dx=0, dy=0, sad_zero=0, sad_best=0, moving_zero=0, moving_best=0)]       # constant frames


def test_rule_and_accumulation_across_run_starts():
    rows = [row(3, -2, 100, 10), row(1, 1, 50, 50), row(-4, 0, 9, 8), row(0, 0, 0, 0), row(2, 2, 7, 1), row(0, 0, 5, 5), row(5, 5, 1, 0)]
    offs, adopted = container.pan_offsets(rows, [4], 10, 8)
    #  frame:  0       1       2 (tie: not adopted)  3         4 (run start)  5       6       7
    assert offs == [(0, 0), (3, 6), (3, 6), (9, 6), (0, 0), (2, 2), (2, 2), (7, 7)]
    assert adopted == [(1, 3, -2), (3, -4, 0), (5, 2, 2), (7, 5, 5)]
    as_dicts = [{k: int(r[k]) for k in r.dtype.names} for r in rows]
    assert pan_ref.offsets(as_dicts[:3] + [dict(as_dicts[3])] + as_dicts[4:], [4], 10, 8) == (offs, adopted)
    assert container.pan_offsets([row(-1, -1, 5, 4)] * 3, (), 2, 2) == ([(0, 0), (1, 1), (0, 0), (1, 1)], [(1, -1, -1), (2, -1, -1), (3, -1, -1)])
    assert container.pan_offsets([], (), 4, 4) == ([(0, 0)], [])


def records_of(types):
    return [(ty, b"rec%d" % i) for i, ty in enumerate(types)]


def test_pan_table_round_trip_and_refusals():
    K, I = container.KEY, container.INTER
    entries = {1: (3, 0), 2: (95, 63), 4: (0, 1)}
    body = container.build_pans(entries)
    assert body == pan_ref.build_table([(1, 3, 0), (2, 95, 63), (4, 0, 1)])
    assert container.parse_pans(body) == pan_ref.parse_table(body) == [(1, 3, 0), (2, 95, 63), (4, 0, 1)]
    frames = records_of([K, I, I, K, I])
    digests = [11, 22, 33, 44, 55]
    recs = frames + [(container.PANS, body), (container.DIGESTS, build_trailer(digests))]
    blob = container.write(recs)
    assert container.split_tables(container.parse(blob)) == (frames, entries, digests)
    assert container.split_tables(container.parse(blob), (64, 96, 3)) == (frames, entries, digests)
    assert container.split_tables(frames + [(container.PANS, body)]) == (frames, entries, None)
    # without a table: today's handling, by both functions
    assert container.split_tables(frames + [recs[-1]]) == (frames, {}, digests) and container.split_tables(frames) == (frames, {}, None)
    assert container.split_trailer(frames + [recs[-1]]) == (frames, digests) and container.split_trailer(frames) == (frames, None)
    container.check_types([ty for ty, _ in container.split_tables(recs)[0]])
    with pytest.raises(ValueError, match="unknown record type 6"):
        container.check_types([K, container.PANS])

    def refused(records, what, **kw):
        with pytest.raises(ValueError, match=what):
            container.split_tables(records, **kw)

    def resum(b):
        return b[:-8] + struct.pack("<Q", pan_ref.fd1(b[:-8]))
    for at in (0, 5, 9, 13, len(body) - 1):                          # one flipped byte anywhere: the table's own digest
        bad = bytearray(body)
        bad[at] ^= 0x40
        refused(frames + [(container.PANS, bytes(bad))], "damaged|version|reserved|does not hold")
    refused(frames + [(container.PANS, container.build_pans({3: (1, 1)}))], "record 3 is no inter-frame")
    refused(frames + [(container.PANS, container.build_pans({7: (1, 1)}))], "record 7 is no inter-frame")
    refused(frames + [(container.PANS, resum(body[:8] + body[20:32] + body[8:20] + body[32:]))], "must ascend")
    refused(frames + [(container.PANS, resum(body[:8] + body[8:20] + body[8:20] + body[32:]))], "must ascend")
    refused(frames + [(container.PANS, container.build_pans([(1, 0, 0)]))], r"offset \(0, 0\)")
    refused(frames + [(container.PANS, container.build_pans({}))], "without entries")
    refused(frames + [(container.PANS, container.build_pans({1: (96, 0)}))], "outside a frame", frame_shape=(64, 96, 3))
    refused(frames + [(container.PANS, container.build_pans({1: (0, 64)}))], "outside a frame", frame_shape=(64, 96, 3))
    refused(frames + [(container.PANS, body), (container.PANS, body)], "2 pan tables")
    refused(frames[:3] + [(container.PANS, body)] + frames[3:], "directly behind the last frame record")
    refused(frames + [recs[-1], (container.PANS, body)], "directly behind the last frame record|only be the last")
    refused(frames + [(container.PANS, body[:10])], "shorter than")
    refused(frames + [(container.PANS, resum(b"\x02" + body[1:]))], "version 2 is unknown")
    refused(frames + [(container.PANS, resum(body[:1] + b"\x01" + body[2:]))], "reserved")
    refused(frames + [(container.PANS, resum(body[:4] + struct.pack("<I", 2) + body[8:]))], "does not hold the 2 entries")


def test_offsets_are_checked_against_the_frame_shape():
    container.check_pans({1: (3, 0), 2: (95, 63), 4: (0, 1)}, (64, 96, 3))
    with pytest.raises(ValueError, match="record 2"):
        container.check_pans({1: (3, 0), 2: (95, 63)}, (63, 96))


def test_keyword_refusals():
    ok = dict(pan_range=4, mask_channels="all", inter_frames=True, keyframe_interval=6)
    comp = ImprovedVideoCompressor(**ok)
    assert comp.pan_range == 4 and comp.last_pans == []
    assert ImprovedVideoCompressor().pan_range == 0
    for bad in (-1, 33, 1.0, "4", True, None):
        with pytest.raises(ValueError, match="pan_range must be an integer in 0..32"):
            ImprovedVideoCompressor(**dict(ok, pan_range=bad))
    for kw, what in ((dict(gop_batching=False), "needs gop_batching=True"), (dict(inter_frames=False), "acts on inter-frames"),
                     (dict(keyframe_interval=1), "acts on inter-frames"), (dict(mask_channels="luma"), "needs mask_channels='all'")):
        with pytest.raises(ValueError, match=what):
            ImprovedVideoCompressor(**dict(ok, **kw))
    per_pixel = np.zeros((8, 8), dtype=np.int64)
    per_pixel[3, 3] = 2
    with pytest.raises(ValueError, match="differ from pixel to pixel"):
        ImprovedVideoCompressor(**dict(ok, error_bounds=per_pixel))
    with pytest.raises(ValueError, match="differ from pixel to pixel"):
        ImprovedVideoCompressor(**dict(ok, error_bounds=np.stack([per_pixel] * 3, axis=2)))
    ImprovedVideoCompressor(**dict(ok, error_bounds=[1, 2, 2]))                     # per-channel bounds are fine
    ImprovedVideoCompressor(**dict(ok, error_bounds=np.full((8, 8, 3), 2)))         # ... and so is a map that says the same everywhere
    # blocks that start at keyframes: refused before anything touches a device
    frames = [np.zeros((20, 24, 3), dtype=np.uint8)] * 12
    with pytest.raises(ValueError, match="pan_range=4: the block that starts at frame 4 does not start at a keyframe"):
        ImprovedVideoCompressor(**dict(ok, block_frames=5)).encode_range(frames, 0, 0, 12)
    with pytest.raises(ValueError, match="does not start at a keyframe"):
        ImprovedVideoCompressor(**ok).encode_range(frames, 0, 3, 12)
    assert "pan_range=0" in inspect.signature(ImprovedVideoCompressor.__init__).__str__()


def test_header_declares_both_entries_additively():
    hdr = open(os.path.join(REPO, "include", "rbf.h")).read()
    assert re.search(r"#define\s+RBF_ABI_VERSION\s+4\b", hdr)
    clean = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(rbf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", clean))
    assert protos["rbf_pan_search"].count(",") + 1 == 12 == len(nat._PROTOS["rbf_pan_search"][1])
    assert protos["rbf_roll_frames"].count(",") + 1 == 8 == len(nat._PROTOS["rbf_roll_frames"][1])
    assert "rbf_pan_stat" in hdr and nat.PAN_ROW.itemsize == 40 and nat.PAN_ROW.names == ("dx", "dy", "sad_zero", "sad_best", "moving_zero", "moving_best")
    assert "RBF_K_PAN" not in hdr and "RBF_K_ROLL" not in hdr          # untimed, like rbf_cut_stats: the id count stays
    lib = nat.lib()
    assert hasattr(lib, "rbf_pan_search") and hasattr(lib, "rbf_roll_frames")


def test_pan_kernels_do_not_spill():
    out = subprocess.run(["python", os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True, check=True).stdout
    rows = {ln[:84].strip(): ln[84:].split() for ln in out.splitlines() if not ln.startswith("#") and not ln.startswith("kernel ")}
    for k in ("k_pan_sad<unsigned char, 8>", "k_pan_sad<unsigned char, 16>", "k_pan_sad<unsigned char, 32>", "k_pan_sad<unsigned short, 8>",
              "k_pan_sad<unsigned short, 16>", "k_pan_sad<unsigned short, 32>", "k_pan_pick", "k_pan_moving<unsigned char, 1>",
              "k_pan_moving<unsigned char, 3>", "k_pan_moving<unsigned char, 4>", "k_pan_moving<unsigned short, 1>", "k_pan_moving<unsigned short, 3>",
              "k_pan_moving<unsigned short, 4>", "k_pan_moving_reduce", "k_roll_frames", "k_roll_frames_bytes"):
        hits = [n for n in rows if n == k]
        assert hits, (k, sorted(rows))
        vgprs, _, scratch, spills, waves = rows[k][:5]
        assert scratch == "0" and spills == "0" and int(waves) >= 2, (k, rows[k])


def test_sad_tile_fits_two_workgroups_per_cu():
    """rbf_kernels_pan.h: a tile of 16 x 8 grid points with a halo of R, rows padded to an odd number of dwords, plus 128 grid samples."""
    for R in (1, 8, 32):
        for sb in (1, 2):
            pitch = 4 * ((((8 * 16 + 2 * R) * sb + 3) // 4) | 1)
            assert pitch * (8 * 8 + 2 * R) + 16 * 8 * 4 <= 64 * 1024


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(96, 64, 4, 12), (320, 180, 8, 8)])
@pytest.mark.parametrize("noise", [(0, 0), (1, 2)])
def test_reference_finds_every_planted_shift(shape, dtype, noise):
    """What the GPU tests rely on: on the planted clips the reference finds every shift, every planted pair passes the rule, and the
    aligned pair's mask falls from about n to under 0.15 n -- so "the container is smaller" (test_gpu_pan.py) is not luck."""
    W, H, R, F = shape
    frames, shifts = pan_ref.planted_clip(W, H, R, dtype, sensor_noise=noise[0], nframes=F)
    rows = pan_ref.stat_rows(frames, R, tolerance=noise[1])
    assert [(r["dx"], r["dy"]) for r in rows] == shifts
    n = W * H
    for r, v in zip(rows, shifts):
        assert r["moving_best"] < 0.15 * n, r
        if v != (0, 0):
            assert r["moving_best"] < r["moving_zero"], r
            if abs(v[0]) == R:                                       # a corner of the range: unaligned, about every pixel moves
                assert r["moving_zero"] > 0.6 * n, r
        else:
            assert r["moving_best"] == r["moving_zero"] and r["sad_best"] == r["sad_zero"]
    stab, offs, adopted, _ = pan_ref.stabilise(frames, R, tolerance=noise[1], run_starts=[6] if F == 12 else [])
    assert adopted == [(j, dx, dy) for j, (dx, dy) in enumerate(shifts, start=1) if (dx, dy) != (0, 0) and not (F == 12 and j == 6)]
    for j in range(1, F):                                            # the identity: pair j of the stabilised block differs in moving(v_j) pixels
        if F == 12 and j == 6:
            continue
        d = np.abs(stab[j].astype(np.int64) - stab[j - 1].astype(np.int64)) > noise[1]
        assert int(d.any(axis=2).sum()) == rows[j - 1]["moving_best"]


@pytest.mark.parametrize("noise", [0, 1, 2])
def test_static_noisy_clips_adopt_nothing(noise):
    for seed in (3, 4, 5):
        frames = make_camera_gop(seed, 96, 64, 4, sensor_noise=noise)
        rows = pan_ref.stat_rows(frames, 4, tolerance=2 * noise)
        offs, adopted = pan_ref.offsets(rows, [], 96, 64)
        assert adopted == [] and offs == [(0, 0)] * 4, rows


def test_make_panning_gop():
    frames, shifts = make_panning_gop(7, 64, 48, 40, (3, -2), return_shifts=True)
    assert len(frames) == 40 and frames[0].shape == (48, 64, 3) and frames[0].dtype == np.uint8
    assert set(shifts) == {(-3, 2), (3, -2), (-3, -2), (3, 2)} or set(shifts) >= {(-3, 2), (3, -2)}     # back and forth: the signs flip
    assert make_panning_gop(7, 64, 48, 3, [(0, 0), (2, 1)], dtype=np.uint16)[2].dtype == np.uint16
    with pytest.raises(ValueError, match="velocities"):
        make_panning_gop(7, 64, 48, 4, [(1, 1)] * 2)
    # a window that does not move is the canvas's centre: the scene of make_camera_gop, cropped
    still = make_panning_gop(9, 40, 32, 3, (0, 0))
    canvas = make_camera_gop(9, 40 + 12, 32 + 10, 3)
    assert all(np.array_equal(s, c[5:37, 6:46]) for s, c in zip(still, canvas))
    # the existing generators return the bytes they did (test_near_lossless_cpu.py pins make_camera_gop's digests)


def test_a_fallen_back_frame_of_a_rolled_run_is_digested_from_the_callers_array():
    """Its record codes the caller's frame; the block holds that frame rolled by the run's offset, so the block's digest is not the
    frame's.  (Reached by 16-bit single-channel clips, whose mask is blind to a change of 0x8000: tests/surface_cases.py, EXTRA.)"""
    from concurrent.futures import ThreadPoolExecutor
    from new_bloom_filter_repo_amd.integrity import frame_digest_host
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor, _BlockRecords, _RangeRecords
    frames = [np.full((8, 12), 1000 * t + 7, dtype=np.uint16) for t in range(4)]
    comp = ImprovedVideoCompressor(keyframe_interval=4, block_frames=4, inter_frames=True, mask_channels="all", pan_range=2, frame_digests=True)
    with ThreadPoolExecutor(2) as pool:
        book = _RangeRecords(comp, frames, 0, 0, 4, pool)
        coded = pool.submit(lambda: b"record")
        block_digests = [11, 22, 33, 44]         # (of the rolled block: right for the frames the records code, wrong for a frame coded from the caller's array)
        book.take_block((0, 4, []), _BlockRecords([coded, None, None], digests=block_digests, pan_offsets=[(0, 0), (2, 1), (4, 2), (0, 0)]))
        got = [d if isinstance(d, int) else d.result() for d in (book.digests[u] for u in range(4))]
    assert got[:2] == [11, 22], "the keyframe and the coded inter-frame: the block's digests"
    assert got[2] == frame_digest_host(frames[2]) != 33, "fell back under a non-zero offset: the caller's frame"
    assert got[3] == 44, "fell back at offset (0, 0): the block holds the caller's frame"
    assert book.pan_table == {1: (2, 1)}
