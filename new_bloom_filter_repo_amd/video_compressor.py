"""ImprovedVideoCompressor -- the product surface (improved_video_compressor.py:309-669), with the
inter-frame route the reference never wired in: frame t is a keyframe iff t % keyframe_interval == 0
(zlib, FixedVideoCompressor); every other frame is coded as a luma residual mask against frame t-1
through the GPU Bloom path (VideoFrameCompressor).

Losslessness is kept unconditional, as the reference promises ("True Lossless"): an inter-frame is
only emitted when applying its record to frame t-1 reproduces frame t bit for bit (the luma mask at
threshold 0 must cover every changed pixel); otherwise that frame falls back to a keyframe.  mask_channels="all" codes the
mask of every pixel in which any sample changed instead, which covers every change by construction.

Container and record types: container.py.  sample_codec="rice" writes types 3 and 4 instead of 1 and 2: the same two roles with the GPU
sample codec (sample_codec.py) in place of zlib-9.  frame_digests=True appends a type-5 record: one digest per frame (integrity.py), which
decompress_video checks against what it rebuilt.  bounded_keyframes=True writes type 7 where a near-lossless call would write type 3: the
keyframe within the bound, quantised in the block it is resident in (rbf_kernels_keyquant.h).
"""
import contextlib
import os
import queue
import struct
import threading
import time
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import container
from . import params as P
from ._native import frame_geometry
from .container import DIGESTS, INTER, INTER_RICE, KEY, KEY_NEAR, KEY_RICE, KEY_TYPES, PANS, is_keyframe, plan_range
from .frame_codec import FixedVideoCompressor, VideoFrameCompressor, YUVFrame, build_record, frame_data, parse_record
from .integrity import IntegrityError, build_trailer, digests_device, frame_digest_host
from .sample_codec import key_format, key_record, near_key_record, parse_key_record, parse_near_key_record, stream_info
from .surface_options import check_blocks, check_options

_POPCOUNT8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)   # numpy 1.x has no bitwise_count


def _popcount(packed):
    """Set bits of a packed uint8 vector."""
    if hasattr(np, "bitwise_count"):             # numpy >= 2: whole 64-bit words
        body = packed[:packed.size // 8 * 8]
        words = body.view(np.uint64) if body.ctypes.data % 8 == 0 else np.frombuffer(body.tobytes(), dtype=np.uint64)
        return int(np.bitwise_count(words).sum(dtype=np.int64)) + int(np.bitwise_count(packed[body.size:]).sum(dtype=np.int64))
    return int(_POPCOUNT8[packed].sum(dtype=np.int64))


def _as_block(data):
    """The frames of a block as ONE contiguous (F, H, W[, C]) array for the upload: a zero-copy view when the caller's frames already lie
    back to back in memory (slices of one decoded clip), a stacked copy otherwise."""
    a = data[0]
    if all(d.flags.c_contiguous for d in data):
        base, nb = a.ctypes.data, a.nbytes
        if nb and all(d.ctypes.data == base + i * nb for i, d in enumerate(data)):
            import ctypes
            raw = np.ctypeslib.as_array((ctypes.c_uint8 * (nb * len(data))).from_address(base))      # (the frames in `data` keep the memory alive)
            return raw.view(a.dtype).reshape((len(data),) + a.shape)
    return np.stack(data)


class _Lane:
    """One GPU lane of the plugin surface: a library context (= one HIP stream) with the GOP coders and the decode engine that live on
    it.  Consecutive blocks of a video alternate over the lanes, each block driven by its own host thread (the C ABI's copies are
    synchronous and ctypes drops the GIL), so block b+1 uploads while block b encodes and block b-1 downloads."""

    def __init__(self, ctx, owned):
        self.ctx, self.owned = ctx, owned
        self.coders = {}
        self.engine = None
        self.samples = None
        self.scratch = None

    def digests(self, ptr, stride, nframes, frame_bytes):
        """integrity.digests_device on this lane, into a block the lane keeps (no allocation per chunk of a run)."""
        if self.scratch is None:
            from ._native import BufferCache
            self.scratch = BufferCache(self.ctx)
        return digests_device(self.ctx, ptr, stride, nframes, frame_bytes, out=self.scratch.get("digests", 8 * nframes))

    def coder(self, spec):
        """The lane's GopCoder(**spec), kept.  A compressor has one bound frame per frame shape and dtype (its _bound_frames), so that
        pair stands for the frame in the key."""
        from .gop import GopCoder
        E = spec.error_bounds
        key = spec._replace(error_bounds=None if E is None else (E.shape, E.dtype.str))
        c = self.coders.get(key)
        if c is None:
            if len(self.coders) >= 2:            # a stream has at most two block sizes (full blocks and its tail)
                for old in self.coders.values():
                    old.close()
                self.coders = {}
            c = self.coders[key] = GopCoder(self.ctx, **spec._asdict())
        return c

    def decode_engine(self):
        from .engine import BloomEngine
        if self.engine is None:
            self.engine = BloomEngine(self.ctx)
        return self.engine

    def sample_coder(self):
        from .sample_codec import SampleCoder
        if self.samples is None:
            self.samples = SampleCoder(self.ctx)
        return self.samples

    def release(self):
        for c in self.coders.values():
            c.close()
        self.coders = {}
        for name in ("engine", "samples", "scratch"):
            if getattr(self, name) is not None:
                getattr(self, name).close()
                setattr(self, name, None)

    def close(self):
        self.release()
        if self.owned:
            self.ctx.close()


class _LanePool:
    """The jobs of one call spread over its lanes: `free` holds the lanes no job is using."""

    def __init__(self, lanes):
        self.lanes = list(lanes)
        self.free = queue.Queue()
        for lane in self.lanes:
            self.free.put(lane)

    @contextlib.contextmanager
    def take(self):
        """`with pool.take() as lane:` -- waits for a free lane and returns it whatever happens inside."""
        lane = self.free.get()
        try:
            yield lane
        finally:
            self.free.put(lane)

    def map(self, jobs, fn):
        """[fn(job, self.take) for job in jobs]: fn holds a lane for the part of its work that needs one.  One lane: the jobs run in order on
        the calling thread; more: on len(lanes) threads, started in order.  An exception in a job reaches the caller."""
        if len(self.lanes) == 1:
            return [fn(job, self.take) for job in jobs]
        with ThreadPoolExecutor(len(self.lanes)) as gpu_pool:
            return list(gpu_pool.map(lambda job: fn(job, self.take), jobs))


_CoderSpec = namedtuple("_CoderSpec", "width height nframes channels sample_bytes mask_channels max_error hold_mode error_bounds keep_originals")      # GopCoder's keywords


class _BlockRecords:
    """What _encode_block returns for a block the GPU coded."""

    def __init__(self, pairs=(), digests=None, cuts=(), pan_offsets=None, pans=(), quality=None, near_keys=None, run_bounds=()):
        self.pairs = list(pairs)                 # per pair: the future of its inter-frame record, or None (needs a keyframe, or is one)
        self.digests = digests                   # frame_digests=True: uint64 per frame of the block, or None
        self.cuts = tuple(cuts)                  # scene_cuts=True: the block indices the cut rule made run starts
        self.pan_offsets = pan_offsets           # pan_range > 0: the frames' cumulative offsets (ox, oy) in the block, or None
        self.pans = pans                         # ... and [(block index, dx, dy)] of the pairs that adopted a shift
        self.quality = quality                   # quality_report=True: GopCoder.error_stats() of the block, a row per frame
        self.near_keys = near_keys or {}         # bounded_keyframes=True: block index of a run first -> its type-7 record
        self.run_bounds = list(run_bounds)       # target_psnr: (block index of a run's first frame, its bound, sse, updates) per run


def _union_seconds(intervals):
    """Total length of the union of (t0, t1) intervals."""
    total, end = 0.0, None
    for t0, t1 in sorted(intervals):
        if end is None or t0 > end:
            total += t1 - t0
            end = t1
        elif t1 > end:
            total += t1 - end
            end = t1
    return total


def _close_timing(tm, t_all, busy):
    """The totals of a last_timing dict: `busy` holds the (start, end) times of the lanes' GPU work since t_all."""
    tm["total"] = time.perf_counter() - t_all
    tm["gpu_busy"] = _union_seconds(busy)                                    # wall time during which at least one lane had a copy or a kernel in flight
    tm["gpu_busy_frac"] = tm["gpu_busy"] / tm["total"] if tm["total"] > 0 else 0.0


def _inter_record(r, n, dtype, rice):
    """The fields of an inter-frame record (type 2, or rice: type 4) behind a frame of n pixels and `dtype` samples, checked before any of
    them reaches the device: the sample-width byte, n, the byte counts (parse_record), and
      a coded record (witness_bits > 0)   a filter of at least one bit, and a k* and a length the C ABI takes (params.filter_params);
      a passthrough one                    its bitmap IS the mask: bitmap_bits == n.  The pad bits behind bit n of its last byte are
                                           cleared here -- the scatter walks every set bit of the mask's last word.
    ValueError otherwise."""
    if len(r) < 1 or r[0] not in (1, 2) or r[0] != np.dtype(dtype).itemsize:
        raise ValueError("inter-frame record: sample-width byte %s behind a frame of %d-byte samples" % (r[0] if len(r) else "missing", np.dtype(dtype).itemsize))
    d = parse_record("f64", r[1:])
    if d["n"] != n:
        raise ValueError("inter-frame record of %d pixels after a frame of %d" % (d["n"], n))
    d["dtype"] = np.uint8 if r[0] == 1 else np.uint16
    d["rice"] = bool(rice)
    P.filter_params(d["k"], d["bitmap_bits"])                     # (k* and the length in range: of a passthrough record too)
    if d["witness_bits"] > 0:
        if d["bitmap_bits"] < 1:
            raise ValueError("inter-frame record: %d witness bits and no filter" % d["witness_bits"])
    else:
        if d["bitmap_bits"] != n:
            raise ValueError("inter-frame record without witness: its bitmap of %d bits is no mask of %d pixels" % (d["bitmap_bits"], n))
        if n % 8:
            mask = d["bitmap"].copy()
            mask[-1] &= (0xFF << (8 - n % 8)) & 0xFF
            d["bitmap"] = mask
    if d["rice"]:
        cnt, bits, size = stream_info(d["values_z"])
        if (cnt, bits, size) != (d["value_count"], 8 * np.dtype(dtype).itemsize, len(d["values_z"])):
            raise ValueError("type-4 record: its sample stream (%d %d-bit samples, %d bytes) does not match the record" % (cnt, bits, size))
    return d


_RECORD_ERRORS = (ValueError, struct.error, zlib.error, IndexError, OverflowError)


@contextlib.contextmanager
def _naming(first, last=None):
    """Whatever the bytes of the records first .. last make a decoder raise comes out as a plain ValueError that names them by their
    index in the stream (first None: the caller has no index; the error still comes out plain).  An IntegrityError speaks of a frame
    already; an RbfError that is no refusal of an argument (RBF_EINVAL, RBF_ERANGE) is the device's and passes."""
    from ._native import RBF_EINVAL, RBF_ERANGE, RbfError
    try:
        yield
    except IntegrityError:
        raise
    except _RECORD_ERRORS + (RbfError,) as e:
        if isinstance(e, RbfError) and e.code not in (RBF_EINVAL, RBF_ERANGE):
            raise                                # the device's own trouble, not the record's
        named = first is None or (type(e) is ValueError and str(e).startswith("record"))
        if named and type(e) is ValueError:
            raise
        where = "" if named else ("record %d: " % first if last is None or last == first else "records %d..%d: " % (first, last))
        raise ValueError("%s%s" % (where, e)) from None


def _run_offsets(pan_table, lo, hi):
    """The cumulative pan offsets of the records lo .. hi-1 of a container, or None when none of them is rolled."""
    offs = [pan_table.get(i, (0, 0)) for i in range(lo, hi)]
    return offs if any(o != (0, 0) for o in offs) else None


class _DigestLog:
    """The digests decompress_video takes of the frames it rebuilds, against the stored ones.  expected: the container's digests, or None
    when there is nothing to check -- then nothing is taken."""

    def __init__(self, expected):
        self.expected, self.checking = expected, expected is not None
        self.got, self.device = {}, {}           # record index -> (digest of the rebuilt frame, "device" | "host"); first record index -> the list a lane fills

    def sink(self, first):
        """A list for the device digests of the records first, first + 1, ..., or None when not checking."""
        return self.device.setdefault(first, []) if self.checking else None

    def host(self, first, frames):
        """Digest `frames`, the frames of the records first, first + 1, ..., with the host twin."""
        if self.checking:
            for i, f in enumerate(frames):
                self.got[first + i] = (frame_digest_host(frame_data(f)), "host")

    def summary(self, nframes):
        """(last_integrity, last_bad_frames) of a call that rebuilt nframes frames."""
        self.got.update({first + i: (int(v), "device") for first, values in self.device.items() for i, v in enumerate(values)})
        where = [w for _, w in self.got.values()]
        integrity = {"frames": nframes, "checked": len(self.got), "device": where.count("device"), "host": where.count("host")}
        return integrity, [i for i in sorted(self.got) if self.got[i][0] != self.expected[i]]


class _RangeRecords:
    """The bookkeeping of one encode_range call: what becomes of every frame of [start, stop) -- its record, or the job that makes it,
    its digest, its row of the quality report, its pan offset -- and the call's cuts and pans.  comp: the compressor; pool: the executor
    of the host's zlib-9 and digest jobs.
      records    frame -> (type, record)
      pending    frame -> (type, the future of its record; KEY: the callable that joins it)
      gpu_keys   sample_codec="rice": the keyframes coded as type-3 records on the lanes, at the end
      digests    frame -> its digest, or the future of the host twin's
      quality    quality_report: frame -> its row of the block it was coded in
      pan_table  pan_range: index into the range's records -> the frame's cumulative offset, if not (0, 0)
      scene_cuts, pans   the cut frames; (frame, dx, dy) of the adopted pairs"""

    def __init__(self, comp, frames, first_index, start, stop, pool):
        self.comp, self.frames, self.first_index, self.start, self.stop, self.pool = comp, frames, first_index, start, stop, pool
        self.inter_type = INTER_RICE if comp.sample_codec == "rice" else INTER
        self.records, self.pending, self.digests, self.quality, self.pan_table = {}, {}, {}, {}, {}
        self.gpu_keys, self.scene_cuts, self.pans, self.run_bounds = set(), [], [], []

    def key(self, t):
        """Frame t is a keyframe: on a lane later (a type-3 record can carry it) or in zlib-9 on the host threads from now on."""
        if t in self.pending or t in self.gpu_keys:
            return
        frame = self.frames[t - self.first_index]
        if self.comp.sample_codec == "rice" and key_format(frame) is not None:
            self.gpu_keys.add(t)
        else:
            self.pending[t] = (KEY, self.comp.compressor.compress_frame_jobs(frame, self.pool.submit))

    def near_key(self, u, got, j):
        """Frame u is a run first of a block: True when the block delivered its type-7 record (bounded_keyframes: the block holds the
        quantised frame Y, and the inter-frames behind it hang off Y), which is filed -- the frame no longer goes through gpu_keys, and
        its row of the quality report is the block's, like its digest.  Two blocks that hold the same keyframe deliver the same bytes."""
        rec = got.near_keys.get(j)
        if rec is None or not self.start <= u < self.stop:
            return rec is not None
        self.gpu_keys.discard(u)
        self.records.setdefault(u, (KEY_NEAR, rec))
        if got.quality is not None:
            self.quality.setdefault(u, got.quality[j])
        return True

    def digest_of(self, u, block_digests=None, j=0):
        """Frame u's digest: entry j of its block's (taken on the GPU from the resident frames), else the host twin's of the caller's array."""
        if not self.comp.frame_digests or u in self.digests or not self.start <= u < self.stop:
            return
        if block_digests is not None:
            self.digests[u] = int(block_digests[j])
        else:
            self.digests[u] = self.pool.submit(frame_digest_host, frame_data(self.frames[u - self.first_index]))

    def take_block(self, block, inter):
        """File the frames of `block` = (lo, end, run starts) of the plan; inter: what _encode_block made of it, or None -- not
        batchable, or gop_batching=False: frame by frame, here.
        The block's digests describe its frames AFTER the hold.  The hold never writes a run's first frame (rbf_kernels_hold.h: "frame
        first[y] is never written"), so the block's first frame and the keyframes inside it -- the run starts handed to the coder -- still
        are the caller's originals, which is what their keyframe records code: their digests are taken from the block too.  Not so a
        frame that falls back to a keyframe with max_error > 0, or in a run the alignment rolled: its record codes the original, the
        block holds the held or rolled frame -- the host twin digests the original."""
        comp, start, stop = self.comp, self.start, self.stop
        lo, end, _ = block
        seg = self.frames[lo - self.first_index:end - self.first_index]      # predecessor + the frames lo+1..end-1
        got = inter if inter is not None else _BlockRecords()
        cut = set(got.cuts)                      # a cut frame is a run start of its block like a rule keyframe
        self.scene_cuts += [lo + j for j in sorted(cut) if start <= lo + j < stop]
        self.pans += [(lo + j, dx, dy) for j, dx, dy in got.pans if start <= lo + j < stop]
        self.run_bounds += [(lo + j, d, sse, updates) for j, d, sse, updates in got.run_bounds if start <= lo + j < stop]
        self.near_key(lo, got, 0)
        self.digest_of(lo, got.digests, 0)
        for j in range(1, len(seg)):
            u = lo + j
            if is_keyframe(u, self.first_index, comp.keyframe_interval) or j in cut:
                if not self.near_key(u, got, j):
                    self.key(u)
                self.digest_of(u, got.digests, j)
                continue
            if inter is None:
                self.digest_of(u)
                rec = comp._encode_inter(seg[j - 1], seg[j])
                if rec is not None:
                    self.records[u] = (self.inter_type, rec)
                    continue
            elif inter.pairs[j - 1] is not None:
                self.pending[u] = (self.inter_type, inter.pairs[j - 1])
                self.digest_of(u, got.digests, j)
                if got.pan_offsets is not None and got.pan_offsets[j] != (0, 0) and start <= u < stop:
                    self.pan_table[u - start] = got.pan_offsets[j]
                if got.quality is not None:
                    self.quality[u] = got.quality[j]
                continue
            self.key(u)
            rolled = got.pan_offsets is not None and got.pan_offsets[j] != (0, 0)     # (the block holds the frame rolled: the record codes the caller's)
            self.digest_of(u, None if comp._near or rolled else got.digests, j)

    def finish(self, release, tm, busy):
        """Code the type-3 keyframes, wait for the host threads, set the compressor's last_* attributes; the range's [(type, record)]."""
        comp, frames, first_index, start, stop = self.comp, self.frames, self.first_index, self.start, self.stop
        if self.gpu_keys:
            t_key = time.perf_counter()
            for u, rec in comp._encode_keys_rice(frames, first_index, sorted(self.gpu_keys - set(self.records)), busy).items():
                self.records[u] = (KEY_RICE, rec)
            if release:
                comp._release_lanes()
            tm["gpu_phase"] += time.perf_counter() - t_key
        t_wait = time.perf_counter()
        for u, (ty, fut) in self.pending.items():
            self.records[u] = (ty, fut() if ty == KEY else fut.result())
        tm["zlib_wait"] = time.perf_counter() - t_wait                       # what the host threads' zlib-9 still owed after the last block left the GPU
        comp.last_digests = [d if isinstance(d, int) else int(d.result()) for d in (self.digests[u] for u in range(start, stop))] if comp.frame_digests else None
        comp.last_scene_cuts, comp.last_pans, comp.last_pan_offsets = sorted(self.scene_cuts), sorted(self.pans), self.pan_table
        comp.last_run_bounds = sorted(self.run_bounds)
        comp.last_quality = comp._quality_dicts(frames, first_index, start, stop, self.quality) if comp.quality_report else None
        return [self.records[u] for u in range(start, stop)]


class ImprovedVideoCompressor:
    def __init__(self, noise_tolerance=10.0, keyframe_interval=30, min_diff_threshold=3.0,
                 max_diff_threshold=30.0, bloom_threshold_modifier=1.0, batch_size=30,
                 num_threads=None, use_direct_yuv=False, verbose=False, ctx=None, inter_frames=None,
                 gop_batching=True, block_frames=None, gpu_lanes=2, mask_channels="luma", sample_codec="zlib", max_error=0,
                 frame_digests=False, verify_digests=True, hold_mode="first", scene_cuts=False, error_bounds=None, quality_report=False,
                 pan_range=0, target_psnr=None, bounded_keyframes=False):
        """Reference signature (improved_video_compressor.py:318-327) plus seventeen keyword-only extras:
        ctx (library context), gop_batching (False: one set of C-ABI calls per inter-frame instead of one
        per block; both write the same bytes), block_frames (consecutive frames handed to the GPU in ONE
        rbf_encode_runs launch sequence -- several GOPs, cut at the keyframes; default 2 GOPs, at most 128
        frames), gpu_lanes (contexts = HIP streams the blocks alternate over, each block on its own host
        thread: upload, encode and download of neighbouring blocks overlap; 1 = one block at a time) and
        inter_frames -- None (default): YUV input is coded with
        Bloom inter-frames ('BFV2' container, which the reference's decompress_video rejects), anything
        else as keyframes; False: always the reference's all-keyframe 'BFVC' container, readable by the
        reference; True: inter-frames for every colour space (lossless fallback to keyframes per frame).
        mask_channels: "luma" (default) -- an inter-frame's mask is the luma residual mask, and a frame in which some pixel changed in
        chroma but not in luma falls back to a keyframe; "all" -- the mask marks every pixel in which any sample changed (the all-channel
        mask kernel), so every inter-frame the GPU can batch is coded as one.  Both write records today's decoder reads: a fresh default
        compressor decompresses either container.
        sample_codec: "zlib" (default) -- keyframes and changed values in zlib-9, the record formats' own; "rice" -- both through the GPU
        sample codec (sample_codec.py: records 3 and 4, 'BFV2' only, so not with inter_frames=False); frames a type-3 record cannot carry
        stay zlib keyframes.  decompress_video reads either with any settings.
        max_error: 0 (default) -- lossless.  A positive integer -- near-lossless: every decoded sample is within max_error of the original
        and every keyframe is exact.  Inside a run (a keyframe and the inter-frames that hang off it) a pixel is held at its last coded value
        while every one of its samples stays within max_error of it, and is updated as a whole otherwise (GopCoder(max_error=...): the
        bounded-error temporal hold on the GPU); the held frames are then coded exactly, in today's records -- a fresh default compressor
        decodes the container.  What it buys: on footage with sensor noise the exact mask is almost all ones, the held one is the moving
        pixels.  Needs mask_channels="all", inter-frames, gop_batching=True, and blocks that start at keyframes (encode_range raises
        otherwise: block_frames a multiple of keyframe_interval, a range that starts on a keyframe).  A block the GPU cannot batch is
        coded exactly, which satisfies the bound.  The reference's noise_tolerance / min_diff_threshold / max_diff_threshold stay
        accepted and unused.
        hold_mode: "first" (default) -- the rule above: a pixel is held while it stays within max_error of the value it was last coded
        with, so sensor noise of +-a needs max_error >= 2a before the masks get sparse.  "lookahead" (needs max_error > 0) -- a pixel's
        segment lasts while the windows [x - max_error, x + max_error] of its frames still intersect (GopCoder(hold_mode="lookahead"):
        the look-ahead hold on the GPU), so max_error = a is enough; the same bound, exact keyframes and records, never more updates.
        frame_digests: False (default) -- the container is today's, byte for byte.  True -- compress_video appends a type-5 record with one
        FD1 digest per frame (integrity.py; the container is then always 'BFV2'): of the frame the decoder must rebuild, so with
        max_error > 0 of the HELD frame.  Frames coded from a resident block are digested there, on the GPU, in one launch sequence per
        block; frames that reach the container from the caller's arrays (keyframes, the frame-by-frame route) by the host twin.
        verify_digests: True (default) -- decompress_video checks a container's digests, inter-frames on the GPU from the block they are
        rebuilt in, and raises IntegrityError at the first frame (in stream order) that does not match; False -- the trailer is parsed and
        ignored.  A container without one decodes as ever.  last_integrity says how many frames were checked, and where.
        scene_cuts: False (default) -- frame t is a keyframe iff t % keyframe_interval == 0, whatever is in it; the container is today's,
        byte for byte.  True -- a frame that is cheaper coded on its own than against its predecessor (a scene cut: its mask would be all
        ones and its "changed values" the difference of two unrelated pictures) becomes a keyframe as well.  The decision is made on the GPU
        from the block's resident frames right after their upload (GopCoder.cut_stats: rbf_cut_stats, one pass that reads every frame
        once; container.cut_frames: inter_bits + moving > intra_bits, integers, no tunable constant) and the cut frames join the block's
        run starts, so the hold, the mask stage and the Bloom kernels treat them exactly like the rule's keyframes.  With max_error > 0 a
        pixel the hold will keep still is not counted as moving (tolerance max_error for hold_mode="first", 2 * max_error for
        "lookahead"), and a cut frame is exact like every keyframe.  The keyframe rule itself is unchanged, and decompress_video derives
        its runs from the record types: a fresh default compressor decodes the container.  Needs a resident block to look at: not with
        gop_batching=False, inter_frames=False or keyframe_interval=1; a block the GPU cannot batch is coded as without the keyword.
        last_scene_cuts lists the cut frames (global indices, ascending) of the last encode_range.
        error_bounds: None (default), or the near-lossless mode with a bound PER SAMPLE in place of the one number max_error (not both):
        a sequence of C non-negative integers (one bound per channel: chroma tolerates more than luma), an integer array of shape (H, W)
        (one bound per pixel: 0 inside a region that must stay exact, any value at a known bad pixel) or one of shape (H, W, C).
        container.bounds_frame expands it to a bound frame when the first block's shape is known (a shape that does not fit the frames
        raises before anything is uploaded); the hold kernels read that frame (GopCoder(error_bounds=...)), everything behind them codes
        the held block exactly, as with max_error: every decoded sample is within ITS bound, keyframes and pixels whose bounds are 0 are
        exact, a fresh default compressor decodes.  hold_mode applies as above, and what max_error > 0 needs is needed here.  A bound
        frame whose entries all equal d is coded as max_error=d, byte for byte.  With scene_cuts the cut statistic stays scalar: its
        tolerance is the SMALLEST entry of the bound frame (doubled for "lookahead") -- a smaller tolerance only counts more pixels as
        moving, so a frame may become a keyframe that a map-aware statistic would have kept as an inter-frame: that can cost bytes,
        never correctness.
        quality_report: False (default) -- nothing is copied or launched.  True -- last_quality holds one dict per frame of the last
        encode_range, aligned with its records: max_abs_error, mse, psnr (peak 2^B - 1; inf for an exact frame), changed_samples,
        over_bound (samples further from the original than their bound: 0).  Measured on the GPU from the block each frame was coded in
        (GopCoder(keep_originals=True).error_stats(): a device copy of the uploaded block against the held one).  The decoder rebuilds
        the held block exactly -- with frame_digests the container proves it -- so this is the quality of the decoded clip, for one
        more read of the block and no decode.  A frame that reaches the container from the caller's array (keyframes, exact fallbacks)
        reports zeros.  Works with max_error=d and with a lossless call too.
        pan_range: 0 (default) -- nothing is launched and the container is today's, byte for byte.  R in 1..32 -- pan alignment: while the
        camera pans, every pixel differs from the one at its position a frame earlier, the mask is all ones and the Bloom stage never
        runs.  Right after a block's upload the GPU finds every pair's global integer shift within +-R pixels (GopCoder.align_pans:
        rbf_pan_search, SAD on a luma grid; include/rbf.h has the definitions), a pair adopts it iff fewer pixels move with it than
        without (container.pan_offsets: integers, no tunable constant), and every frame is rolled cyclically by its run's cumulative
        offset (rbf_roll_frames) -- a bijection: nothing is lost, and the pixels that wrap around are the newly revealed content, coded
        as changed pixels.  Cut statistic, hold, mask stage, Bloom kernels, sample codec and digests then see a still block and are the
        code they are; the offsets travel in a type-6 record (container.build_pans) that is written only when some pair adopted a
        shift, so a clip without a pan gets today's bytes.  decompress_video rolls every rebuilt frame back on the device; a fresh
        default compressor decodes.  The model is integer translation only: a sub-pixel pan leaves edge residue, which a near-lossless
        hold absorbs in part and a lossless call codes; nothing is interpolated.  Keyframes, scene cuts included, always have offset 0.
        Needs gop_batching=True, inter-frames, keyframe_interval > 1, mask_channels="all" and blocks that start at keyframes (as
        max_error > 0 does); not with error_bounds that differ from pixel to pixel (the bound map would no longer sit on the pixels it
        was drawn for; per-channel bounds are fine).  A block whose frames are not larger than 2R in both directions is coded as
        without the keyword.  last_pans lists (global frame index, dx, dy) for every pair of the last encode_range that adopted a shift.
        target_psnr: None (default) -- the bound is max_error, for every run; nothing is launched and the container is today's, byte for
        byte.  T, a finite positive number of dB -- the caller names the quality to keep instead of the bound, and max_error = cap >= 1
        becomes the bound's CEILING.  After a block's upload, pan alignment and cut detection -- the runs are final, the block is still
        -- ONE pass over the block (GopCoder.hold_sweep: rbf_hold_sweep) measures what each candidate bound
        (container.sweep_candidates: 1..cap, or eight values up to a cap above 8) would do to each run under hold_mode's rule, and every
        run gets the largest candidate whose sum of squared errors fits its budget (container.choose_bound; container.sse_budget:
        floor(N (2^B - 1)^2 / 10^(T / 10)), N the samples of all the run's frames), or 0 -- exact -- when none does.  The hold then
        runs with a bound per run (GopCoder.set_run_bounds) and everything behind it is the code it is: a clean run takes the cap while
        a noisy one stays tight.  So every run's PSNR over all samples of all its frames is >= T, every sample is within cap of the
        original, keyframes are exact, and -- the records carry no bound -- a fresh default compressor decodes the container.  A T
        that every run meets at the cap writes the bytes of max_error=cap; a T no candidate meets writes the lossless
        mask_channels="all" container.  A block the GPU cannot batch is coded exactly, as with max_error.  Needs max_error in 1..255,
        block_frames <= 128 (the sweep takes 128 runs of up to 128 frames) and everything max_error > 0 needs; not with error_bounds (the sweep is scalar) and not with bounded_keyframes (the
        keyframe would be quantised before the sweep could see what the hold hangs off).  Combines with scene_cuts, pan_range,
        frame_digests, quality_report, hold_mode and sample_codec as max_error does.  The cut statistic keeps the CAP's tolerance: a
        run that ends up with a smaller bound moves more than the statistic assumed and may miss a cut -- that costs bytes, never
        correctness.  last_run_bounds lists (global index of the run's first frame, its bound, sse, updates) for every run of the
        last encode_range; compress_video's result carries it as "run_bounds" next to "target_psnr".
        bounded_keyframes: False (default) -- keyframes are exact, nothing is launched and the container is today's, byte for byte.
        True -- every keyframe that is a run first of a batched block (rule keyframes and scene cuts alike) is coded within the bound
        instead of exactly: a closed-loop quantiser inside the keyframe predictor (GopCoder.quantise_run_starts:
        rbf_rice_encode_intra_near, include/rbf.h has the rule) rewrites the frame in its block before the hold runs, so the
        inter-frames that hang off it are held against the value a decoder will have, and the frame travels in a type-7 record
        (container.KEY_NEAR: the per-channel bounds and a sample stream of the quantised residuals).  On noisy footage the exact
        keyframes are the larger part of a near-lossless container; this takes 30-40 % off them.  The inter-frames are then held against
        a keyframe that is up to d away from the original: the look-ahead hold absorbs that (the container shrinks), the first-value hold
        does not when the noise is half the bound (the container can grow) -- use it with hold_mode="lookahead".  Needs sample_codec="rice" and a
        near-lossless bound -- max_error > 0 or per-channel error_bounds that are not all zero; not error_bounds arrays of two or
        more dimensions (a decoder would need the map) -- and with it everything max_error > 0 needs.  Combines with scene_cuts,
        hold_mode, frame_digests, quality_report (a keyframe's row is then its block's, no longer zeros) and pan_range.  A keyframe
        that never sits in a batched block -- an unbatchable shape, a keyframe outside any block, a frame no type-3 record could carry,
        the exact fallback of a near-lossless run -- stays an exact record, which satisfies the bound.  A fresh default compressor
        decodes the container.
        What the last call left behind: last_compressed_frames -- [(type, record bytes)] of compress_video; of encode_range last_digests,
        last_quality, last_scene_cuts and last_pans as above, and last_pan_offsets -- {index into its records: (ox, oy)}, what the
        type-6 record says; of decompress_video last_integrity -- {"frames", "checked", "device", "host"} -- and last_bad_frames -- the
        frames whose digest did not match (on_mismatch="collect"); of either last_timing -- seconds per stage (bench.py's e2e_surface
        leg; profile_stages=True synchronises between the stages of a block so that it can tell them apart)."""
        o = self._options = check_options(keyframe_interval, inter_frames, gop_batching, block_frames, gpu_lanes, mask_channels, sample_codec,
                                          max_error, frame_digests, verify_digests, hold_mode, scene_cuts, error_bounds, quality_report, pan_range,
                                          target_psnr, bounded_keyframes)
        self.bounded_keyframes, self.target_psnr = o.bounded_keyframes, o.target_psnr
        self.pan_range, self.error_bounds, self.quality_report, self.scene_cuts = o.pan_range, o.error_bounds, o.quality_report, o.scene_cuts
        self.max_error, self.hold_mode, self._near = o.max_error, o.hold_mode, o.near
        self.frame_digests, self.verify_digests = o.frame_digests, o.verify_digests
        self.sample_codec, self.mask_channels, self.inter_frames = o.sample_codec, o.mask_channels, o.inter_frames
        self.keyframe_interval, self.gop_batching, self.block_frames, self.gpu_lanes = o.keyframe_interval, o.gop_batching, o.block_frames, o.gpu_lanes
        self.noise_tolerance, self.min_diff_threshold, self.max_diff_threshold = noise_tolerance, min_diff_threshold, max_diff_threshold
        self.bloom_threshold_modifier, self.batch_size = bloom_threshold_modifier, batch_size
        self.num_threads = max(1, num_threads or min(64, os.cpu_count() or 1))     # zlib of keyframes / changed values
        self.use_direct_yuv, self.verbose = use_direct_yuv, verbose
        self.chain_chunk_frames = 64             # frames per device-side rebuild chunk of a run (engine.rebuild_chain)
        self.last_pans, self.last_pan_offsets, self.last_scene_cuts, self.last_run_bounds = [], {}, [], []
        self.last_quality = self.last_digests = self.last_integrity = self.last_bad_frames = self.last_compressed_frames = self.last_timing = None
        self.last_read = None
        self.profile_stages = False
        self.compressor = FixedVideoCompressor(verbose=verbose)
        self._bound_frames = {}                  # (frame shape, dtype) -> (the bound frame, its uniform value or None)
        self._ctx, self._inter, self._lanes = ctx, None, []
        self._tm_lock = threading.Lock()

    def close(self):
        """Return the device memory this compressor holds (the lanes' GOP coders and contexts, the inter-frame codec's
        scratch).  Also happens when the object is dropped; the compressor stays usable afterwards."""
        for lane in self._lanes:
            lane.close()
        self._lanes = []
        if self._inter is not None:
            self._inter.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def inter(self):
        if self._inter is None:
            self._inter = VideoFrameCompressor(keyframe_interval=self.keyframe_interval, use_direct_yuv=True,
                                               verbose=False, ctx=self._ctx, mask_channels=self.mask_channels)
        return self._inter

    def _get_lanes(self, count):
        """`count` lanes: lane 0 is the caller's context (or the process default), the others are contexts of their own on the same device."""
        from . import _native as nat
        if not self._lanes:
            self._lanes.append(_Lane(self._ctx or nat.default_context(), False))
        while len(self._lanes) < count:
            self._lanes.append(_Lane(nat.Context(self._lanes[0].ctx.device), True))
        return self._lanes[:count]

    def _on_lanes(self, jobs, fn):
        """The results of fn(job, take) in job order, the jobs alternating over min(gpu_lanes, len(jobs)) lanes (_LanePool.map)."""
        return _LanePool(self._get_lanes(min(self.gpu_lanes, len(jobs)))).map(jobs, fn)

    def _release_lanes(self):
        for lane in self._lanes:
            lane.release()

    def _tm_add(self, **kw):
        tm = self.last_timing
        if tm is None:
            return
        with self._tm_lock:
            for name, dt in kw.items():
                tm[name] = tm.get(name, 0.0) + dt

    # ------------------------------------------------------------------ encode
    def _encode_inter(self, prev, curr):
        """Record bytes for frame `curr` against `prev`, or None when a keyframe is needed."""
        a, b = frame_data(prev), frame_data(curr)
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (np.uint8, np.uint16) or (a.ndim == 3 and not 3 <= a.shape[2] <= 4):
            return None
        mask, values, _ = self.inter._calculate_frame_diff(a, b, threshold=0.0)
        if self.mask_channels != "all" or a.ndim == 2:     # (the all-channel mask marks every change by construction)
            changed = (a != b)
            if changed.ndim == 3:
                changed = changed.any(axis=2)
            if np.any(changed & (mask == 0)):    # chroma moved where luma did not: not representable
                return None
        if self.sample_codec == "rice":
            record = self._inter_record_rice(mask, a, b)
        else:
            record, _ = self.inter._compress_frame_differences(mask, values)
        return struct.pack("<B", b.dtype.itemsize) + record

    def _inter_record_rice(self, mask, a, b):
        """_compress_frame_differences with the pair's sample stream (on lane 0) in the value field: the bytes _encode_block writes."""
        flat = np.asarray(mask).reshape(-1)
        bitmap, witness, p, n, _ = self.inter.bloom_compressor.compress(flat)
        k, _l = self.inter.bloom_compressor._calculate_optimal_params(n, p)
        ones = int(np.count_nonzero(flat))
        stream = self._get_lanes(1)[0].sample_coder().encode_pair(a, b, np.packbits(flat.astype(np.uint8)), ones)
        _, _, C, _ = frame_geometry(b)
        return build_record(self.inter.wire_format, p, n, k, len(bitmap), np.packbits(bitmap).tobytes(), len(witness),
                            np.packbits(np.array(witness, dtype=np.uint8)).tobytes(), ones * C, stream)

    @staticmethod
    def _block_geometry(seg):
        """(a, H, W, C, sb) of a block of frames -- its first frame's array and _native.frame_geometry of it -- or, as a str, the reason
        the GPU cannot take the block in one piece."""
        data = [frame_data(f) for f in seg]
        a = data[0]
        if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] < 3):
            return "frames of %s with shape %r" % (a.dtype, a.shape)
        if any(d.shape != a.shape or d.dtype != a.dtype for d in data[1:]):
            return "mixed shapes or dtypes"
        return (a,) + tuple(frame_geometry(a))

    def _coder_spec(self, a, nframes):
        """The GopCoder keywords for a block of `nframes` frames like `a`."""
        H, W, C, sb = frame_geometry(a)
        mc = C if self.mask_channels == "all" and C >= 2 else 1      # all-channel mask: every change is covered, no uncovered pass
        max_error, hold_mode, bounds = self.max_error, self.hold_mode, None
        if self.error_bounds is not None:
            bounds, d = self._bound_frame(a)
            if d is not None:                    # one value everywhere: today's scalar calls, today's bytes
                max_error, hold_mode, bounds = d, self.hold_mode if d else "first", None
        return _CoderSpec(W, H, nframes, C, sb, mc, max_error, hold_mode, bounds, self.quality_report)

    def _prepare_block(self, coder, block, run_starts, tol):
        """Upload `block` into the coder and make it what the hold and the mask stage are to see: aligned (pan_range: GopCoder.align_pans),
        looked at for cuts (scene_cuts: GopCoder.cut_stats, container.cut_frames -- the cuts join the run starts) and, where a cut carries
        an offset, re-based (container.rebase_cuts).  tol: container.stat_tolerance -- the block is looked at before any hold rewrites
        it, and a pixel the hold will keep still is not moving.  With target_psnr the runs, final by then, get their bounds
        (_choose_run_bounds) last of all.  Returns (run starts, offsets, adopted, cuts, times, run bounds): the frames' cumulative
        offsets (ox, oy) or None, the pairs [(j, dx, dy)] that adopted a shift, the cut frames, when the upload, the alignment and the
        cut statistic were done (time.perf_counter), and [(first frame, bound, sse, updates)] per run, [] without a target."""
        coder.load_frames(block)                 # (synchronous: the frames are pageable host memory)
        t_up = time.perf_counter()
        starts, offsets, adopted, cuts = list(run_starts), None, [], []
        if self.pan_range and coder.W > 2 * self.pan_range and coder.H > 2 * self.pan_range:
            offsets, _, adopted = coder.align_pans(self.pan_range, tolerance=tol)     # everything below sees the stabilised block
        t_pan = time.perf_counter()
        if self.scene_cuts:
            cuts = container.cut_frames(coder.cut_stats(tolerance=tol), run_starts)
            if cuts:
                starts = sorted(set(run_starts) | set(cuts))
                coder.set_run_starts(starts)
                if offsets is not None and any(offsets[j] != (0, 0) for j in cuts):
                    offsets, rel = container.rebase_cuts(offsets, cuts, starts, coder.W, coder.H)
                    coder.roll_frames(rel)
                adopted = [row for row in adopted if row[0] not in cuts]      # (the pair in front of a cut is not coded)
        t_cut = time.perf_counter()
        run_bounds = self._choose_run_bounds(coder) if self.target_psnr is not None else []
        return starts, offsets, adopted, cuts, (t_up, t_pan, t_cut), run_bounds

    def _choose_run_bounds(self, coder):
        """target_psnr: sweep the resident block, still and with its final runs (GopCoder.hold_sweep: every candidate of
        container.sweep_candidates(max_error) for every run in ONE read of the block), give every run the largest candidate whose sse
        fits the run's budget (container.choose_bound, container.sse_budget over all samples of all the run's frames) and hand the
        bounds to the coder (set_run_bounds).  Returns [(first frame of the run in the block, bound, sse, updates)]; a run that stays
        exact reports sse 0 and its exact update count (one more sweep, candidate 0, only when there is such a run)."""
        candidates = container.sweep_candidates(self.max_error)
        rows, runs = coder.hold_sweep(candidates), coder.runs()
        per_frame = coder.W * coder.H * coder.C
        bounds = [container.choose_bound(rows[r], candidates, container.sse_budget(self.target_psnr, 8 * coder.sb, (b - a) * per_frame))
                  for r, (a, b) in enumerate(runs)]
        exact = coder.hold_sweep([0]) if not all(bounds) else None
        coder.set_run_bounds(bounds)
        out = []
        for r, ((a, _), d) in enumerate(zip(runs, bounds)):
            row = rows[r][candidates.index(d)] if d else exact[r][0]
            out.append((a, d, int(row["sse"]), int(row["updates"])))
        return out

    @staticmethod
    def _pair_jobs(res, values, fallback, pool, n, C, itemsize, rice):
        """The record of every pair of a coded block as a future of `pool` (the value field's zlib-9 runs there), None where fallback[f]
        says the pair is not coded as an inter-frame.  res: GopCoder.results_packed(); values: per pair the changed values, or (rice)
        the pair's sample stream.  The filter and the witness were built with the k rbf_plan_batch computed in C: the record carries
        THAT value (the decoder derives floor_k and T from it), so a last-ulp difference to the Python twin is harmless."""
        jobs = []
        for f, r in enumerate(res):
            if fallback[f]:
                jobs.append(None)
                continue
            p = np.uint64(r["ones"]) / n
            if r["l"]:
                k = r["k"]
                parts = (r["l"], r["filter"], r["witness_bits"], r["witness"])
            else:                                # the reference passes the mask itself through (:215-225)
                k, _l = P.optimal_params(n, p)
                parts = (n, r["mask"], 0, b"")
            vals = values[f]
            if rice:
                def job(p=p, k=k, parts=parts, stream=vals, count=r["ones"] * C):
                    return struct.pack("<B", itemsize) + build_record("f64", p, n, k, *parts, count, stream)
            else:
                def job(p=p, k=k, parts=parts, vals=vals):
                    vz = zlib.compress(vals, level=9)
                    return struct.pack("<B", vals.dtype.itemsize) + build_record("f64", p, n, k, *parts, len(vals), vz)      # (VideoFrameCompressor's default wire format)
            jobs.append(pool.submit(job))
        return jobs

    def _encode_block(self, seg, pool, run_starts=(), lane=None, busy=None):
        """Inter-frame records of one block of consecutive frames in one pass over the GPU: seg[0] is only read (a keyframe, or a
        shard's halo frame), every other frame is coded against its predecessor -- except the frames named in `run_starts` (indices
        into seg), which are keyframes of the stream: they start a new run and the pair in front of them is not coded.  One upload,
        ONE rbf_encode_runs launch sequence for all the runs, ONE exact-size download of the packed record (rbf_pack_records), one
        batched gather of the changed values (luma mask: with the count of changes it cannot carry); zlib runs in `pool`.  With
        frame_digests the block's frames are digested where they lie, after the hold (GopCoder.frame_digests): the result's `digests`.
        With scene_cuts and pan_range the block is looked at right after its upload (_prepare_block): the result's `cuts`,
        `pan_offsets` and `pans`.
        lane: the context and coders to use (default: lane 0); busy: list that receives the (start, end) time of this block's GPU work.
        Returns a _BlockRecords -- pairs: a future / None per pair (None = needs a keyframe, or is one) --, or None when the block
        cannot be batched (_block_geometry)."""
        t0 = time.perf_counter()
        geometry = self._block_geometry(seg)
        if isinstance(geometry, str):
            return None
        a, H, W, C, sb = geometry
        if C > 4:                                # rbf_gather_values_batch carries at most 4 samples per pixel
            return _BlockRecords([None] * (len(seg) - 1))
        if lane is None:
            lane = self._get_lanes(1)[0]
        spec = self._coder_spec(a, len(seg))
        coder = lane.coder(spec)
        coder.set_run_starts(list(run_starts))
        block = _as_block([frame_data(f) for f in seg])
        tol = container.stat_tolerance(spec.max_error, None if spec.error_bounds is None else spec.error_bounds.min(), spec.hold_mode, sb)
        t1 = time.perf_counter()
        _, offsets, adopted, cuts, (t_up, t_pan, t_cut), run_bounds = self._prepare_block(coder, block, run_starts, tol)
        t_q = time.perf_counter()
        near_keys = {}
        if self.bounded_keyframes:               # the run firsts become their quantised selves before the hold looks at them
            firsts = [j for j in [0] + sorted(set(run_starts) | set(cuts)) if key_format(seg[j]) is not None]
            bounds = coder.key_bounds()
            near_keys = {j: near_key_record(seg[j], bounds, stream)
                         for j, stream in coder.quantise_run_starts(lane.sample_coder(), firsts).items()}
        t2 = time.perf_counter()
        if self.bounded_keyframes:
            self._tm_add(key_quantise=t2 - t_q)
        coder.encode()
        if self.profile_stages:
            lane.ctx.sync()
        t3 = time.perf_counter()
        res = coder.results_packed()
        block_digests = coder.frame_digests() if self.frame_digests else None
        block_quality = coder.error_stats() if self.quality_report else None
        t4 = time.perf_counter()
        rice = self.sample_codec == "rice"
        if spec.mask_channels == 1:
            values, uncovered = coder.gather_values(check_uncovered=True)
        else:
            values, uncovered = None if rice else coder.gather_values(check_uncovered=False), [0] * (len(seg) - 1)
        if rice:                                 # the value fields: every pair's residual stream in one launch sequence
            values = coder.rice_streams([r["ones"] for r in res], lane.sample_coder())
        t5 = time.perf_counter()
        self._tm_add(stack=t1 - t0, upload=t_up - t1, gpu_encode=t3 - t2, download_rows=t4 - t3, value_gather=t5 - t4)
        if self.scene_cuts:
            self._tm_add(cut_stats=t_cut - t_pan)   # (one launch sequence, a wait and 24 bytes per pair)
        if self.target_psnr is not None:
            self._tm_add(hold_sweep=t_q - t_cut)
        if self.pan_range:
            self._tm_add(pan_align=t_pan - t_up)
        if busy is not None:
            busy.append((t1, t5))
        fallback = container.fallback_pairs([bool(r.get("skipped")) for r in res], uncovered, offsets, self._near)
        return _BlockRecords(self._pair_jobs(res, values, fallback, pool, H * W, C, a.dtype.itemsize, rice),
                             block_digests, cuts, offsets, adopted, block_quality, near_keys, run_bounds)

    def encode_range(self, frames, first_index, start, stop, inter_frames=True, release=True):
        """[(type, record)] for the frames with global indices [start, stop); frames[i] is global frame
        first_index + i (a shard passes its halo frame too, dist.halo_start).  Frame t is a keyframe iff
        t % keyframe_interval == 0 -- or, with scene_cuts, a cut (self.last_scene_cuts) --; the inter-frames are coded in blocks of up to `block_frames` consecutive frames --
        several GOPs per block, ONE launch sequence on the GPU per block, cut at the keyframes (plan_range).  The blocks alternate over
        `gpu_lanes` contexts, each block on its own host thread; the host's zlib-9 (keyframes: four jobs each; changed values:
        one job per frame) runs on `num_threads` threads under all of it.  release: return the lanes' device memory as soon as the last
        block has left the GPU (False: keep the coders for the next call of the same geometry).
        frame_digests=True: self.last_digests holds one digest per returned record (of the frame a decoder rebuilds from it), else None.
        The keyframes the rule fixes in advance go to the host threads FIRST: their zlib-9 (the longest single jobs, ~0.2 s for a 1080p
        frame, plus its three planes) then runs under the GPU's blocks instead of behind the last one."""
        I = self.keyframe_interval
        self.last_timing = tm = {}
        t_all = time.perf_counter()
        busy = []
        fixed_keys, blocks = plan_range(first_index, start, stop, I, self.block_frames, inter_frames)
        if blocks:
            if self._near and self.error_bounds is not None and self.gop_batching:     # a bound frame that does not fit the clip: before any upload
                a = frame_data(frames[blocks[0][0] - first_index])
                if a.dtype in (np.uint8, np.uint16) and a.ndim in (2, 3):
                    self._bound_frame(a)
            check_blocks(self._options, blocks, first_index, I)
        in_block = {u for lo, end, _ in blocks for u in range(lo, end)} if self.gop_batching else set()
        with ThreadPoolExecutor(self.num_threads) as pool:
            book = _RangeRecords(self, frames, first_index, start, stop, pool)

            def run_block(block, take):
                lo, end, starts = block
                with take() as lane:
                    return self._encode_block(frames[lo - first_index:end - first_index], pool, starts, lane, busy)
            for t in fixed_keys:
                book.key(t)
                if t not in in_block:            # (a keyframe inside a block is digested there, with the block's other frames)
                    book.digest_of(t)
            results = self._on_lanes(blocks, run_block) if self.gop_batching and blocks else [None] * len(blocks)
            tm["gpu_phase"] = time.perf_counter() - t_all                    # until the last block's values were on the host
            if release:                                                      # the lanes' blocks of frames, masks, filters and witnesses go back while the
                t_rel = time.perf_counter()                                  # host threads still owe their zlib: not kept between videos
                self._release_lanes()
                tm["release"] = time.perf_counter() - t_rel
            for block, inter in zip(blocks, results):
                book.take_block(block, inter)
            records = book.finish(release, tm, busy)
        _close_timing(tm, t_all, busy)
        tm["blocks"], tm["lanes"] = len(blocks), min(self.gpu_lanes, max(1, len(blocks)))
        return records

    def _bound_frame(self, a):
        """(the bound frame of error_bounds for frames like `a`, d if all its entries equal d else None); kept, so that every block of a
        clip hands its coder the same array."""
        key = (a.shape, a.dtype.str)
        if key not in self._bound_frames:
            E = container.bounds_frame(self.error_bounds, a.shape, a.dtype)
            self._bound_frames[key] = (E, container.uniform_bound(E))
        return self._bound_frames[key]

    def _quality_dicts(self, frames, first_index, start, stop, rows):
        """last_quality: frame u's dict from its block's row (rows[u]); a frame coded from the caller's array is exact -- zeros."""
        from ._native import ERROR_ROW
        from .verify import quality_rows
        out = []
        for u in range(start, stop):
            a = frame_data(frames[u - first_index])
            row = rows.get(u)
            out += quality_rows([np.zeros((), dtype=ERROR_ROW) if row is None else row], max(1, a.size), 8 * a.dtype.itemsize)
        return out

    def _encode_keys_rice(self, frames, first_index, ts, busy):
        """Type-3 records of the keyframes with global indices `ts`: batches of up to four frames of one shape, ONE rbf_rice_encode_intra
        each, alternating over the GPU lanes like the blocks.  Returns {t: record}."""
        batches = []
        for t in ts:
            a = frame_data(frames[t - first_index])
            if batches and len(batches[-1][1]) < 4 and batches[-1][0] == (a.shape, a.dtype):
                batches[-1][1].append(t)
            else:
                batches.append(((a.shape, a.dtype), [t]))

        def run(batch, take):
            fs = [frames[t - first_index] for t in batch[1]]
            with take() as lane:
                t0 = time.perf_counter()
                streams = lane.sample_coder().encode_frames(fs)
                busy.append((t0, time.perf_counter()))
            return [key_record(f, s) for f, s in zip(fs, streams)]
        outs = self._on_lanes(batches, run)
        return {t: rec for (_, ts_b), recs in zip(batches, outs) for t, rec in zip(ts_b, recs)}

    def _decode_key_rice(self, rec, lane=None, busy=None, digest_out=None, near=False):
        """A type-3 keyframe (near: a type-7 one) decoded on `lane` (default: lane 0): the frame, or a YUVFrame when the record says so.  digest_out: a list that
        receives the frame's digest, taken on the device where the frame was decoded, before its download."""
        if lane is None:
            lane = self._get_lanes(1)[0]
        t0 = time.perf_counter()
        dev, yuv = self._decode_key_device(rec, lane, None, digest_out, near)
        frame = lane.sample_coder().fetch(dev)
        if busy is not None:
            busy.append((t0, time.perf_counter()))
        return YUVFrame(frame) if yuv else frame

    def compress_video(self, frames, output_path=None, input_color_space="BGR"):
        """improved_video_compressor.py:358-450, same result dict.  Divergence: with inter-frames enabled
        (see the constructor's `inter_frames`; the default for YUV input) the container is 'BFV2', which only
        this package reads; `inter_frames=False` (or keyframe_interval=1) writes the reference's 'BFVC'."""
        if not frames:
            raise ValueError("No frames provided for compression")
        start = time.time()
        yuv = input_color_space.upper() == "YUV"
        if yuv:
            self.use_direct_yuv = True
            for i in range(len(frames)):
                if not hasattr(frames[i], "yuv_info"):
                    frames[i] = self.compressor.add_yuv_info_to_frame(frames[i])
        original_size = sum(f.nbytes for f in frames)
        use_inter = yuv if self.inter_frames is None else bool(self.inter_frames)
        try:
            records = self.encode_range(frames, 0, 0, len(frames), inter_frames=use_inter)
        finally:
            self._release_lanes()                # (an exception in front of encode_range's own release)
        if self.last_pan_offsets:                # the pan table: behind the last frame record, only when some frame is rolled
            records = records + [(PANS, container.build_pans(self.last_pan_offsets))]
        if self.frame_digests:                   # the trailer: one digest per frame record, behind them all
            records = records + [(DIGESTS, build_trailer(self.last_digests))]
        self.last_compressed_frames = records
        keyframes = sum(1 for ty, _ in records if ty in KEY_TYPES)
        if output_path:
            blob = container.write(records)
            os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
            with open(output_path, "wb") as f:
                f.write(blob)
            compressed_size = len(blob)
        else:                                    # the container's size without joining ~1 MB per frame into one bytes object nobody asked for
            compressed_size = container.size(records)
        ratio = compressed_size / original_size
        elapsed = time.time() - start
        results = {"frame_count": len(frames), "original_size": original_size, "compressed_size": compressed_size,
                   "compression_ratio": ratio, "space_savings": 1.0 - ratio, "compression_time": elapsed,
                   "frames_per_second": len(frames) / elapsed if elapsed > 0 else float("inf"),
                   "keyframes": keyframes, "keyframe_ratio": keyframes / len(frames),
                   "output_path": output_path, "color_space": input_color_space, "overall_ratio": ratio}
        if self.max_error:
            results.update(max_error=self.max_error, hold_mode=self.hold_mode)
        if self.error_bounds is not None:
            results.update(error_bounds=True, hold_mode=self.hold_mode)
        if self.target_psnr is not None:
            results.update(target_psnr=self.target_psnr, run_bounds=list(self.last_run_bounds))
        if self.bounded_keyframes:
            results["bounded_keyframes"] = sum(1 for ty, _ in records if ty == KEY_NEAR)
        if self.scene_cuts:
            results["scene_cuts"] = list(self.last_scene_cuts)
        if self.pan_range:
            results["pans"] = list(self.last_pans)
        if self.verbose:
            print("\\nCompression Results:")
            print(f"Original Size: {original_size / (1024 * 1024):.2f} MB")
            print(f"Compressed Size: {compressed_size / (1024 * 1024):.2f} MB")
            print(f"Compression Ratio: {ratio:.4f}")
            print(f"Keyframes: {keyframes} ({results['keyframe_ratio'] * 100:.1f}%)")
        return results

    _container = staticmethod(container.write)
    _container_size = staticmethod(container.size)
    _parse_container = staticmethod(container.parse)

    # ------------------------------------------------------------------ decode
    @staticmethod
    def _load_records(input_path, compressed_frames):
        """(frame records, pan table, stored digests or None) of a container file or of a list of records, checked (container.split_tables,
        check_types): a damaged trailer or pan table is a plain ValueError here, not a damaged frame."""
        records = None
        if input_path and os.path.exists(input_path):
            with open(input_path, "rb") as f:
                records = container.parse(f.read())
        elif compressed_frames:
            records = [r if isinstance(r, tuple) else (KEY, r) for r in compressed_frames]
        if not records:
            raise ValueError("No compressed frames provided")
        records, pan_table, stored = container.split_tables(records)
        if not records:
            raise ValueError("No compressed frames provided")
        container.check_types([ty for ty, _ in records])
        return records, pan_table, stored

    def decompress_video(self, input_path=None, output_path=None, compressed_frames=None, metadata=None, on_mismatch="raise"):
        """The frames of a container (input_path) or of its records (compressed_frames).  A container with a digest trailer is checked
        unless verify_digests=False: every inter-frame on the GPU, from the chain block it is rebuilt in; a type-3 keyframe on the GPU
        where it is decoded; a type-1 keyframe by the host twin on the thread that inflated it.  The first frame, in stream order, whose
        digest is not the stored one raises IntegrityError (on_mismatch="collect": no exception, self.last_bad_frames lists them all --
        verify.verify_container).  self.last_integrity = {"frames", "checked", "device", "host"}.
        Damage: a container whose bytes make a record undecodable raises a plain ValueError whose text names the record's index in
        the stream (IntegrityError is a ValueError and names a frame) -- never struct.error, IndexError, zlib.error, OverflowError, a numpy
        broadcasting error or an RbfError --, no frame comes back that the records do not code, and this object decodes a good container
        bit for bit afterwards ("What a reader does with a damaged container").
        The keyframes are independent of everything else: they are inflated on the host threads while the inter-frame runs go through
        the GPU (type-3 keyframes are decoded on the lanes: by the run that hangs off them, or by a job of their own).  Every run hangs
        off its own keyframe, so the runs are independent too: they alternate over the lanes, each on its own host thread -- the inflate
        and upload of run r+1 under the device-side rebuild and the download of run r."""
        if on_mismatch not in ("raise", "collect"):
            raise ValueError("on_mismatch must be 'raise' or 'collect', got %r" % (on_mismatch,))
        start = time.time()
        t_all = time.perf_counter()
        records, pan_table, stored = self._load_records(input_path, compressed_frames)
        log = _DigestLog(stored if self.verify_digests else None)
        types = [ty for ty, _ in records]
        self.last_timing = tm = {}
        busy = []
        key_pool = ThreadPoolExecutor(self.num_threads)

        def key_job(j, rec):
            with _naming(j):
                frame = self.compressor.decompress_frame(rec)
            return frame, frame_digest_host(frame_data(frame)) if log.checking else None
        keys = {j: key_pool.submit(key_job, j, rec) for j, (ty, rec) in enumerate(records) if ty == KEY}
        runs = container.inter_runs(types)                                   # (index of the keyframe in front, first record, end)
        gkeys, decoded = {}, {}                                              # type-3 keyframes a run's job decoded; first record of a run -> its frames

        def run_job(job, take):
            k, lo, hi = job
            base = keys[k].result()[0] if types[k] == KEY else None          # (waits for the host's inflate without holding a lane)
            with take() as lane:
                if base is None:
                    with _naming(k):
                        base = gkeys[k] = self._decode_key_rice(records[k][1], lane, busy, digest_out=log.sink(k), near=types[k] == KEY_NEAR)
                if lo is None:
                    return None
                return self._decode_run(base, [rec for _, rec in records[lo:hi]], lane, key_pool, busy, types=types[lo:hi],
                                        digests_out=log.sink(lo), offsets=_run_offsets(pan_table, lo, hi), first=lo)
        try:
            bases = {k for k, _, _ in runs}
            jobs = runs + [(j, None, None) for j, ty in enumerate(types) if ty in (KEY_RICE, KEY_NEAR) and j not in bases]     # lone type-3 keyframes: no run
            if self.gop_batching and jobs:
                for (_, lo, _), out in zip(jobs, self._on_lanes(jobs, run_job)):
                    if lo is not None:
                        decoded[lo] = out
            ends = {lo: hi for _, lo, hi in runs}
            frames, i = [], 0
            while i < len(records):
                if i not in ends:                                            # a keyframe
                    if types[i] == KEY:
                        frame, digest = keys[i].result()
                        frames.append(frame)
                        if log.checking:
                            log.got[i] = (digest, "host")
                    else:
                        with _naming(i):
                            frames.append(gkeys[i] if i in gkeys else self._decode_key_rice(records[i][1], digest_out=log.sink(i), near=types[i] == KEY_NEAR))
                    i += 1
                    continue
                if i in decoded:
                    frames += decoded[i]
                else:
                    stabilised = []
                    frames += self._decode_frame_by_frame(frames[-1], records[i:ends[i]], _run_offsets(pan_table, i, ends[i]), stabilised, first=i)
                    log.host(i, stabilised)                                  # (the digests describe the frames the records code)
                i = ends[i]
        finally:
            key_pool.shutdown(wait=True)
            self._release_lanes()
        _close_timing(tm, t_all, busy)
        tm["runs"], tm["lanes"] = len(runs), min(self.gpu_lanes, max(1, len(runs)))
        self.last_integrity, self.last_bad_frames = log.summary(len(frames))
        if self.last_bad_frames and on_mismatch == "raise":
            i = self.last_bad_frames[0]
            raise IntegrityError(i, log.expected[i], log.got[i][0], key_record=max(j for j in range(i + 1) if types[j] in KEY_TYPES))
        if output_path:
            self.save_frames_as_video(frames, output_path)
        if self.verbose:
            print(f"Decompressed {len(frames)} frames in {time.time() - start:.2f} seconds")
        return frames

    def _decode_key_device(self, rec, lane, busy=None, digest_out=None, near=False):
        """_decode_key_rice without the download: (the keyframe as an engine.DeviceFrame of `lane`, valid until the lane's sample coder
        decodes its next frame; whether the record says YUV).  digest_out: as there."""
        d = parse_near_key_record(rec) if near else parse_key_record(rec)
        t0 = time.perf_counter()
        hook = None if digest_out is None else (lambda ptr, nbytes, cnt: digest_out.extend(int(x) for x in lane.digests(ptr, nbytes, cnt, nbytes)))
        dev = lane.sample_coder().decode_frame_device(d["stream"], d["height"], d["width"], d["channels"], d["itemsize"],
                                                      d["bounds"] if near else None, on_decoded=hook)
        if busy is not None:
            busy.append((t0, time.perf_counter()))
        return dev, bool(d["yuv"])

    def read_frames(self, input_path=None, compressed_frames=None, start=0, stop=None, step=1, roi=None, scale=1, on_mismatch="raise"):
        """Part of a container: the views of the frames range(start, stop, step), in order (stop=None: the end; a stop past the end is
        clamped).  roi=(x, y, w, h), None = the whole frame; scale in {1, 2, 4, 8}: every s x s block of the region becomes its mean,
        rounded half up (include/rbf.h, rbf_frame_view_batch, has the rule; view.view_host is its numpy twin).  A YUVFrame clip yields
        YUVFrame views.  With roi=None, scale=1 and the full range the frames are decompress_video's, bit for bit.  ValueError for
        step < 1, start < 0, an empty span, a bad region or a bad scale.
        What is not needed is not decoded (container.read_span plans from the record types alone): type-1 keyframes outside the span
        are not inflated, runs outside it take no lane, and a run stops at its last wanted frame.  What is not wanted is not
        downloaded: inter-frames are viewed in the chain block they are rebuilt in, after the digests and the pan roll-back
        (engine.rebuild_chain), type-3 / type-7 keyframes where they are decoded -- a keyframe a run hangs off goes into the chain block
        device to device and never reaches the host.  A type-1 keyframe that is wanted itself is inflated on the host and viewed by the
        numpy twin, as is everything on the frame-by-frame route (gop_batching=False).  The runs alternate over the lanes as in
        decompress_video.
        A container with a trailer is checked for every frame that is REBUILT (verify_digests, on_mismatch, IntegrityError and
        last_bad_frames as in decompress_video, indices in clip numbering); the trailer's own digest and the pan table are checked whole.
        Damage: a container whose bytes make a record undecodable raises a plain ValueError whose text names the record's index in
        the stream (IntegrityError is a ValueError and names a frame) -- never struct.error, IndexError, zlib.error, OverflowError, a numpy
        broadcasting error or an RbfError --, no view comes back of a frame that the records do not code, and this object decodes a good container
        bit for bit afterwards ("What a reader does with a damaged container").
        self.last_read = {"records", "records_decoded", "frames_rebuilt", "frames_returned", "downloaded_bytes", "view_shape"}:
        downloaded_bytes is the sum over the frame downloads the call made -- the view blocks of the chains and of the decoded
        keyframes (masks and digests are not frames), counted where each download is made.  That holds on the batched route.  On the
        frame-by-frame route (gop_batching=False) whole frames come back one call at a time and the figure is only a tally of the
        type-3 / type-7 keyframes and type-4 frames that did (type-2 frames, rebuilt by scatter_values, are not in it)."""
        from .view import View, check_region, view_host
        if on_mismatch not in ("raise", "collect"):
            raise ValueError("on_mismatch must be 'raise' or 'collect', got %r" % (on_mismatch,))
        check_region(None, scale, 1, 1)                                      # (the scale; the region needs a frame's shape)
        if roi is not None:
            check_region(roi, scale, 1 << 62, 1 << 62)                       # (its form and signs, before anything is decoded)
        t_all = time.perf_counter()
        records, pan_table, stored = self._load_records(input_path, compressed_frames)
        types = [ty for ty, _ in records]
        keys, runs = container.read_span(types, start, stop, step)
        wanted = list(range(int(start), len(types) if stop is None else min(int(stop), len(types)), int(step)))
        log = _DigestLog(stored if self.verify_digests else None)
        view = View(roi, scale)
        self.last_timing = tm = {}
        busy = []
        fronts = {k for k, _, _, _ in runs}
        key_pool = ThreadPoolExecutor(self.num_threads)

        def key_job(j, rec):
            with _naming(j):
                frame = self.compressor.decompress_frame(rec)
            return frame, frame_digest_host(frame_data(frame)) if log.checking else None
        inflated = {j: key_pool.submit(key_job, j, records[j][1]) for j in sorted(fronts | set(keys)) if types[j] == KEY}
        kviews, decoded = {}, {}                                             # wanted type-3 / type-7 keyframes -> their views; first record of a run -> its views

        def wrap(a, yuv):
            return YUVFrame(a) if yuv else a

        def run_job(job, take):
            k, lo, end, pos = job
            base = inflated[k].result()[0] if types[k] == KEY else None      # (waits for the host's inflate without holding a lane)
            with take() as lane:
                yuv = isinstance(base, YUVFrame)
                if base is None:
                    with _naming(k):
                        base, yuv = self._decode_key_device(records[k][1], lane, busy, digest_out=log.sink(k), near=types[k] == KEY_NEAR)
                    if k in keys:
                        kviews[k] = wrap(lane.sample_coder().fetch(base, view), yuv)
                if lo is None:
                    return None
                return self._decode_run(base, [rec for _, rec in records[lo:end]], lane, key_pool, busy, types=types[lo:end],
                                        digests_out=log.sink(lo), offsets=_run_offsets(pan_table, lo, end), view=view.at(pos), yuv=yuv, first=lo)
        try:
            jobs = list(runs) + [(j, None, None, None) for j in keys if types[j] in (KEY_RICE, KEY_NEAR) and j not in fronts]     # lone type-3 keyframes: no run
            if self.gop_batching and jobs:
                for (_, lo, _, _), out in zip(jobs, self._on_lanes(jobs, run_job)):
                    if lo is not None:
                        decoded[lo] = out
            else:
                for k, lo, end, pos in jobs:                                 # frame by frame: whole frames on the host, the twin views them
                    if types[k] == KEY:
                        base = inflated[k].result()[0]
                    else:
                        with _naming(k):
                            base = self._decode_key_rice(records[k][1], digest_out=log.sink(k), near=types[k] == KEY_NEAR)
                        view.downloads.append(base.nbytes)
                        if k in keys:
                            kviews[k] = wrap(view_host(frame_data(base), roi, scale), isinstance(base, YUVFrame))
                    if lo is None:
                        continue
                    stabilised = []
                    whole = self._decode_frame_by_frame(base, records[lo:end], _run_offsets(pan_table, lo, end), stabilised, first=lo)
                    log.host(lo, stabilised)                                 # (the digests describe the frames the records code)
                    view.downloads.append(sum(f.nbytes for (ty, _), f in zip(records[lo:end], whole) if ty == INTER_RICE))
                    decoded[lo] = [wrap(view_host(frame_data(whole[p]), roi, scale), isinstance(base, YUVFrame)) for p in pos]
            for j, fut in inflated.items():
                frame, digest = fut.result()
                if log.checking:
                    log.got[j] = (digest, "host")
                if j in keys:
                    kviews[j] = wrap(view_host(frame_data(frame), roi, scale), isinstance(frame, YUVFrame))
            at = {lo + p: (lo, q) for _, lo, _, pos in runs for q, p in enumerate(pos)}
            frames = [kviews[i] if i in kviews else decoded[at[i][0]][at[i][1]] for i in wanted]
        finally:
            key_pool.shutdown(wait=True)
            self._release_lanes()
        _close_timing(tm, t_all, busy)
        tm["runs"], tm["lanes"] = len(runs), min(self.gpu_lanes, max(1, len(runs)))
        rebuilt = container.span_records(keys, runs)
        self.last_integrity, self.last_bad_frames = log.summary(rebuilt)
        self.last_read = {"records": len(records), "records_decoded": rebuilt, "frames_rebuilt": rebuilt, "frames_returned": len(frames),
                          "downloaded_bytes": int(sum(view.downloads)), "view_shape": tuple(frame_data(frames[0]).shape)}
        if self.last_bad_frames and on_mismatch == "raise":
            i = self.last_bad_frames[0]
            raise IntegrityError(i, log.expected[i], log.got[i][0], key_record=max(j for j in range(i + 1) if types[j] in KEY_TYPES))
        return frames

    def _decode_frame_by_frame(self, base, records, offsets=None, stabilised_out=None, first=None):
        """The frames of a run of inter-frame records after `base`, one record at a time (gop_batching=False).  offsets: the records'
        cumulative pan offsets (ox, oy), or None -- the records code the STABILISED frames, each is rolled back on the host (np.roll)
        after the next record has been applied to it; stabilised_out: a list that receives the frames as the records code them."""
        frames = []
        for j, (ty, r) in enumerate(records):
            at = None if first is None else first + j
            if ty == INTER_RICE:
                frames += self._decode_run(base, [r], types=[INTER_RICE], first=at)
            else:
                with _naming(at):
                    arr = frame_data(base)
                    n = arr.shape[0] * arr.shape[1]
                    d = self._parse_run(arr, [r], [ty])[0]                       # the checks of the batched route, before anything is decoded
                    values = np.frombuffer(zlib.decompress(d["values_z"]), dtype=d["dtype"])
                    if len(values) != d["value_count"]:
                        raise ValueError("inter-frame record: %d values declared, %d inflated" % (d["value_count"], len(values)))
                    if d["witness_bits"] > 0:                                    # (the witness as the batched route takes it: its whole bytes)
                        mask = self.inter.bloom_compressor.decompress(np.unpackbits(d["bitmap"])[:d["bitmap_bits"]], np.unpackbits(d["witness"]), n, d["k"])
                    else:
                        mask = np.unpackbits(d["bitmap"])[:n]
                    frames.append(self.inter._apply_frame_diff(base, np.asarray(mask, dtype=np.uint8).reshape(arr.shape[:2]), values))
            base = frames[-1]
        if stabilised_out is not None:
            stabilised_out += frames
        if offsets is None:
            return frames
        container.check_pans({(i if first is None else first + i): o for i, o in enumerate(offsets)}, frame_data(base).shape)
        out = []
        for f, (ox, oy) in zip(frames, offsets):
            if (ox, oy) != (0, 0):
                a = np.roll(frame_data(f), (oy, ox), axis=(0, 1))            # F(p) = S((p - c) mod (W, H))
                f = YUVFrame(a) if isinstance(f, YUVFrame) else a
            out.append(f)
        return out

    @staticmethod
    def _parse_run(base_arr, recs, types, first=None):
        """The records of a run after the frame `base_arr`, parsed ("f64" wire format) and checked against it; each dict also carries
        `dtype` (of its values) and `rice` (a type-4 record: its value field is a sample stream).  first: the index of recs[0] in the stream,
        which a ValueError then names (_inter_record has the checks)."""
        n = base_arr.shape[0] * base_arr.shape[1]
        parsed = []
        for j, (ty, r) in enumerate(zip(types, recs)):
            with _naming(None if first is None else first + j):
                parsed.append(_inter_record(r, n, base_arr.dtype, ty == INTER_RICE))
        return parsed

    @staticmethod
    def _fit_values(parsed, masks, vals, n, ch, first=None):
        """Every record's value count against its decoded mask (in place): a type-4 stream that does not fit its mask is an error, so is a
        single-channel type-2 record; a colour frame with a mismatching value count is left untouched."""
        name = lambda i: "" if first is None else "record %d: " % (first + i)
        for i, (m, v) in enumerate(zip(masks, vals)):
            ones = _popcount(np.asarray(m, dtype=np.uint8)[:(n + 7) // 8])
            if parsed[i]["rice"]:                # no reference behaviour to keep: a stream that does not fit its mask is an error
                if parsed[i]["value_count"] != ones * ch:
                    raise ValueError("%stype-4 record: %d residuals for a mask of %d pixels" % (name(i), parsed[i]["value_count"], ones))
                continue
            if len(v) != ones * ch:              # same rule as _apply_frame_diff (:886-903)
                if ch == 1:
                    raise ValueError("%schanged_values does not match the mask" % name(i))
                masks[i], vals[i] = np.zeros((n + 7) // 8, np.uint8), v[:0]      # color: frame left untouched

    def _decode_run(self, base, recs, lane=None, pool=None, busy=None, types=None, digests_out=None, offsets=None, view=None, yuv=None, first=None):
        """A run of inter-frame records after `base`: the masks of all Bloom-coded frames are decoded in
        ONE rbf_bloom_decode_batch, the changed values are inflated in threads, and the frames are
        rebuilt in sequence on the device (engine.apply_chain; type-4 records: SampleCoder.apply_chain).  lane: the context to use
        (default: lane 0); pool: executor for the inflates (default: a temporary one); types: the records' types (default: all type 2);
        digests_out: a list that receives the digest of every rebuilt frame, in order -- taken on the device from the chain block, after
        the rebuild of a chunk and before its download (engine.rebuild_chain's hook).
        offsets: None, or the records' cumulative pan offsets (ox, oy): the records code the stabilised frames S(p) = F((p + c) mod (W, H)),
        so every rebuilt chunk is rolled back on the device (rbf_roll_frames with the negated offsets) after the digest hook and before
        its download -- after its last frame, still stabilised, has been copied into the chain block's slot 0 for the next chunk.
        view (view.View, read_frames): the run's frames stay on the device and the views of the records view.wanted (positions in recs)
        come back instead, taken after the roll-back (engine.rebuild_chain has the hook order); base may then be an engine.DeviceFrame
        of the lane -- a keyframe that was decoded there and never downloaded -- with yuv saying whether the clip's frames are
        YUVFrames.  A viewed run is one stretch of one record type: a run that mixes types 2 and 4 (no compressor writes one) is a
        ValueError here -- decompress_video reads it."""
        from . import _native as nat
        from .engine import DeviceFrame, apply_chain
        if lane is None:
            lane = self._get_lanes(1)[0]
        types = [INTER] * len(recs) if types is None else list(types)
        t0 = time.perf_counter()
        base_arr = base if isinstance(base, DeviceFrame) else frame_data(base)
        yuv = isinstance(base, YUVFrame) if yuv is None else yuv
        H, W, ch, _ = frame_geometry(base_arr)
        n = H * W
        at = lambda j: None if first is None else first + j                  # a record's index in the stream, for the errors
        parsed = self._parse_run(base_arr, recs, types, first)
        if view is not None and any(d["rice"] != parsed[0]["rice"] for d in parsed):
            raise ValueError("a run that mixes record types 2 and 4 cannot be read in part: decompress_video reads it")
        def inflate(d):
            v = np.frombuffer(zlib.decompress(d["values_z"]), dtype=d["dtype"])
            if len(v) != d["value_count"]:
                raise ValueError("inter-frame record: %d values declared, %d inflated" % (d["value_count"], len(v)))
            return v
        own_pool = None
        if pool is None:
            pool = own_pool = ThreadPoolExecutor(self.num_threads)
        val_jobs = [None if d["rice"] else pool.submit(inflate, d) for d in parsed]      # (run under the mask decode below)
        t1 = time.perf_counter()
        coded = [d for d in parsed if d["witness_bits"] > 0]
        if coded:
            plist = [P.filter_params(d["k"], d["bitmap_bits"]) for d in coded]
            with _naming(at(0), at(len(recs) - 1)):
                masks = lane.decode_engine().decode(n, plist, [d["bitmap"] for d in coded], [d["witness"] for d in coded])
            for d, m in zip(coded, masks):
                d["mask"] = m
        t2 = time.perf_counter()
        vals = []
        for i, (j, d) in enumerate(zip(val_jobs, parsed)):
            with _naming(at(i)):
                vals.append(d["values_z"] if j is None else j.result())
        if own_pool is not None:
            own_pool.shutdown()
        t3 = time.perf_counter()
        masks = [d["mask"] if "mask" in d else d["bitmap"][:(n + 7) // 8] for d in parsed]
        self._fit_values(parsed, masks, vals, n, ch, first)
        t4 = time.perf_counter()
        out, prev, i = [], base_arr, 0
        hook = None if digests_out is None else (lambda ptr, fbytes, cnt: digests_out.extend(int(x) for x in lane.digests(ptr, fbytes, cnt, fbytes)))
        chunk = self.chain_chunk_frames
        fbytes, pixel_bytes = base_arr.nbytes, base_arr.nbytes // n
        if offsets is not None:
            container.check_pans({(k if first is None else first + k): o for k, o in enumerate(offsets)}, base_arr.shape)

        def unroll(fb, c0, cnt):
            """rebuild_chain's before_download hook: it runs inside the apply_chain calls below, where `i` is the record of the run the
            stretch in hand starts at."""
            offs = offsets[i + c0:i + c0 + cnt]
            if not any(o != (0, 0) for o in offs):
                return False
            L = nat.lib()
            nat.check(L.rbf_memcpy_d2d(lane.ctx.handle, fb.ptr, fb.ptr + cnt * fbytes, fbytes))          # the next chunk's predecessor: still stabilised
            neg = (nat._i32 * (2 * cnt))(*[-int(v) for o in offs for v in o])
            nat.check(L.rbf_roll_frames(lane.ctx.handle, fb.ptr + fbytes, fbytes, cnt, W, H, pixel_bytes, neg))
            return True
        before = None if offsets is None else unroll
        while i < len(parsed):                   # stretches of one record type: values written (type 2) or residuals added (type 4)
            j = i
            while j < len(parsed) and parsed[j]["rice"] == parsed[i]["rice"]:
                j += 1
            with _naming(at(i), at(j - 1)):              # (a sample stream whose codes do not end inside its words is found on the device: RBF_EINVAL)
                if parsed[i]["rice"]:
                    part = lane.sample_coder().apply_chain(prev, masks[i:j], vals[i:j], chunk_frames=chunk, on_rebuilt=hook, before_download=before, view=view)
                else:
                    part = apply_chain(lane.ctx, prev, masks[i:j], vals[i:j], chunk_frames=chunk, on_rebuilt=hook, before_download=before, view=view)
            out += part
            prev, i = part[-1] if view is None else None, j               # (a viewed run is one stretch: nothing continues it)
            if offsets is not None and i < len(parsed) and offsets[i - 1] != (0, 0):      # the next stretch continues the stabilised frame
                prev = np.ascontiguousarray(np.roll(prev, (-offsets[i - 1][1], -offsets[i - 1][0]), axis=(0, 1)))
        t5 = time.perf_counter()
        self._tm_add(parse=t1 - t0, mask_decode=t2 - t1, inflate_wait=t3 - t2, check=t4 - t3, apply_chain=t5 - t4)
        if busy is not None:
            busy += [(t1, t2), (t4, t5)]
        return [YUVFrame(f) for f in out] if yuv else out

    def verify_lossless(self, original_frames, decompressed_frames):
        return self.compressor.verify_lossless(original_frames, decompressed_frames)

    # ------------------------------------------------------------------ video file I/O (OpenCV, out of scope)
    def save_frames_as_video(self, frames, output_path, fps=30):
        if not frames:
            raise ValueError("No frames provided")
        raise RuntimeError("writing video files needs OpenCV (cv2.VideoWriter, improved_video_compressor.py:525-581), "
                           "which is outside this package's scope; frames are returned as arrays")

    def extract_frames_from_video(self, video_path, max_frames=0, target_fps=None, scale_factor=1.0,
                                  output_color_space="BGR"):
        if not os.path.exists(video_path):
            raise ValueError(f"Video file not found: {video_path}")
        raise RuntimeError("reading video files needs OpenCV (cv2.VideoCapture, improved_video_compressor.py:583-669), "
                           "which is outside this package's scope; pass frames as arrays")
