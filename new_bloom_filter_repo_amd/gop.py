"""GOP-level driver: frames resident in HBM -> residual masks -> (host: filter geometry) ->
Bloom insert + query/witness, one C-ABI call per block of frames: one GOP (rbf_encode_gop) or several GOPs whose keyframes
are marked (rbf_encode_runs: ONE launch sequence for all of them).

Device memory comes from an allocator callback so the same code runs on library-owned buffers
(default) or on torch tensors (bench.py / dist.py pass `torch_allocator`, which lets RCCL move the
results without a copy)."""
import ctypes

import numpy as np

from . import _native as nat
from . import params as P


class _OwnedBlock:
    def __init__(self, buf):
        self.buf, self.ptr, self.nbytes = buf, buf.ptr, buf.nbytes

    def numpy(self, ctx, nbytes=None):
        return self.buf.download(nbytes)


class _TorchBlock:
    def __init__(self, t):
        self.tensor, self.ptr, self.nbytes = t, t.data_ptr(), t.numel() * t.element_size()

    def numpy(self, ctx, nbytes=None):
        a = self.tensor.cpu().numpy().view(np.uint8).reshape(-1)
        return a if nbytes is None else a[:nbytes]


def owned_allocator(ctx):
    return lambda nbytes: _OwnedBlock(ctx.alloc(nbytes))


def torch_allocator(device):
    import torch
    return lambda nbytes: _TorchBlock(torch.zeros((int(nbytes) + 7) // 8, dtype=torch.int64, device=device))


class TorchArena:
    """Carves consecutive 256-byte aligned blocks out of ONE torch tensor, so that a GOP's output
    record (filters | witnesses | stats) is a single contiguous tensor a collective can move."""

    def __init__(self, device, nbytes):
        import torch
        self.tensor = torch.zeros((int(nbytes) + 7) // 8, dtype=torch.int64, device=device)
        self.used = 0

    def __call__(self, nbytes):
        nbytes = (int(nbytes) + 255) // 256 * 256
        assert self.used + nbytes <= self.tensor.numel() * 8, "arena exhausted"
        view = self.tensor[self.used // 8:(self.used + nbytes) // 8]
        self.used += nbytes
        return _TorchBlock(view)


class GopCoder:
    """Encodes the nframes-1 inter-frame residual masks of one GOP of (H, W, C) frames."""

    def __init__(self, ctx, width, height, nframes, channels=3, sample_bytes=1, seeds=P.SEEDS_VIDEO,
                 allocator=None, threshold=0.0, out_allocator=None, frames_block=None, adaptive=None,
                 planar_luma=False, keep_interleaved=True, resident_gops=1, luma_block=None, run_starts=None, mask_channels=1,
                 max_error=0, hold_mode="first", error_bounds=None, keep_originals=False):
        """allocator: device memory source (default: library-owned); out_allocator: separate source for
        the output record (filters, witnesses, stats); frames_block: share another coder's frame buffer.
        threshold=None with adaptive=(noise_tolerance, min_thr, max_thr): per-frame noise-adaptive
        thresholds (improved_video_compressor.py:746-766) -- lossy, like the reference's default.
        planar_luma: keep the GOP's Y planes as one dense block (the reference's YUVFrame carries the same plane,
        fixed_video_compressor.py:292-296) and run the mask stage on it: a third of the interleaved bytes.  The
        interleaved frames are then needed by gather_values() only (keep_interleaved=False: luma alone is resident,
        3x more GOPs per byte of HBM).  resident_gops: room for that many GOPs of frames; encode(gop=g) codes the g-th.
        luma_block: share an existing block of Y planes (like frames_block).
        run_starts: frame indices (within the block of `nframes` frames) that are KEYFRAMES of the caller's stream: each starts a new run,
        and the pair in front of it is not coded (rbf_encode_runs: several GOPs in ONE launch sequence; results() marks those pairs
        `skipped`).  The reference codes frame by frame (improved_video_compressor.py:198-266); batching whole GOPs is this package's.
        mask_channels: 1 (default) = the luma mask; >= 2 = the all-channel mask (rbf_encode_runs_begin_ex): a pixel's bit is 1 when any of
        its first mask_channels samples changed.  Lossless only: threshold 0, no adaptive thresholds, interleaved frames (not planar_luma).
        max_error: 0 (default) = lossless.  > 0 = near-lossless: encode_begin() first runs the bounded-error temporal hold
        (rbf_temporal_hold_runs, same run starts) over the resident GOP and then codes the HELD frames exactly, so every decoded sample is
        within max_error of the original and a run's first frame is exact.  THE RESIDENT BLOCK IS MODIFIED IN PLACE: gather_values() and
        rice_streams() read the held frames (that is what makes the records consistent), and so does every other coder that shares the
        block through frames_block.  The hold is idempotent, so encoding a resident GOP again gives the same rows.  Needs a mask that
        sees every sample (mask_channels == channels, or channels == 1); not with planar_luma, adaptive or a non-zero threshold.
        hold_mode: "first" (default) = that hold: a pixel is kept while its samples stay within max_error of the segment's first value.
        "lookahead" (needs max_error > 0) = the look-ahead hold (rbf_temporal_lookahead_runs): a segment lasts while the windows
        [x - max_error, x + max_error] of its frames intersect, so sensor noise of +-a is held at max_error = a instead of 2a; the same
        bound, the same exact run firsts, never more updates per pixel.  It is NOT idempotent, so the coder runs it ONCE PER load_frames():
        a second encode() of the same resident GOP skips the stage -- the block already is its held sequence -- and returns the same rows.
        (A block shared through frames_block, or filled behind the coder's back, is the caller's to keep track of: mark_loaded().)
        error_bounds: None (default), or a BOUND FRAME (container.bounds_frame: an array of exactly a frame's shape and dtype) -- the
        near-lossless stage with a bound per sample in place of max_error (rbf_temporal_hold_runs_map / rbf_temporal_lookahead_runs_map):
        every decoded sample is within ITS entry of the original, a pixel whose entries are 0 is exact.  The frame is uploaded once per
        coder and serves every block.  Needs what max_error > 0 needs, and not max_error > 0 itself; hold_mode applies as above.
        keep_originals: True = load_frames() also keeps a device copy of the block as it was uploaded (rbf_memcpy_d2d, before any hold),
        which is what error_stats() compares the coded block with.
        """
        from .engine import threshold_floor
        self.mask_channels = int(mask_channels)
        if not 1 <= self.mask_channels <= channels:
            raise ValueError("mask_channels must be 1 (luma) or up to the %d samples of a pixel, got %r" % (channels, mask_channels))
        if self.mask_channels > 1:
            if planar_luma:
                raise ValueError("the all-channel mask reads the interleaved frames: not with planar_luma")
            if threshold is None or adaptive is not None:
                raise ValueError("the all-channel mask is lossless only: no adaptive thresholds")
            if not np.ndim(threshold) == 0 or float(threshold) != 0.0:
                raise ValueError("the all-channel mask is lossless only: threshold must be 0, got %r" % (threshold,))
        if isinstance(max_error, bool) or not isinstance(max_error, (int, np.integer)) or max_error < 0:
            raise ValueError("max_error must be a non-negative integer, got %r" % (max_error,))
        self.max_error = int(max_error)
        if self.max_error >> (8 * sample_bytes):
            raise ValueError("max_error %d does not fit a %d-bit sample" % (self.max_error, 8 * sample_bytes))
        self.error_bounds = None
        if error_bounds is not None:
            if self.max_error:
                raise ValueError("error_bounds and max_error > 0 are two ways to say the bound: give one")
            want = ((height, width) if channels == 1 else (height, width, channels)), np.dtype(np.uint8 if sample_bytes == 1 else np.uint16)
            if not isinstance(error_bounds, np.ndarray) or (error_bounds.shape, error_bounds.dtype) != want:
                raise ValueError("error_bounds must be a bound frame (container.bounds_frame) of shape %r and dtype %s" % want)
            self.error_bounds = np.ascontiguousarray(error_bounds)
        near = "error_bounds" if self.error_bounds is not None else "max_error > 0" if self.max_error else None
        if near:
            if self.mask_channels != channels:
                raise ValueError("%s holds every sample of a pixel: the mask has to see them all (mask_channels == channels = %d, "
                                 "got %d)" % (near, channels, self.mask_channels))
            if planar_luma:
                raise ValueError("%s holds the interleaved frames: not with planar_luma" % near)
            if threshold is None or adaptive is not None:
                raise ValueError("%s codes the held frames exactly: no adaptive thresholds" % near)
            if not np.ndim(threshold) == 0 or float(threshold) != 0.0:
                raise ValueError("%s codes the held frames exactly: threshold must be 0, got %r" % (near, threshold))
        if hold_mode not in ("first", "lookahead"):
            raise ValueError("hold_mode must be 'first' or 'lookahead', got %r" % (hold_mode,))
        if hold_mode == "lookahead" and not near:
            raise ValueError("hold_mode='lookahead' is a near-lossless stage: it needs max_error > 0 or error_bounds")
        self.hold_mode = hold_mode
        self._held = set()                            # look-ahead: the resident GOPs that already are their held sequence
        self._key_streams = {}                        # bounded keyframes: resident GOP -> what quantise_run_starts() made of it
        self.ctx, self.W, self.H, self.F, self.C, self.sb = ctx, width, height, nframes, channels, sample_bytes
        self.n = width * height
        self.pairs = nframes - 1
        self.seeds = nat.Seeds(*[int(s) for s in seeds])
        if threshold is None and adaptive is None:
            raise ValueError("threshold=None needs adaptive=(noise_tolerance, min_thr, max_thr)")
        self.thr = 0 if threshold is None else threshold_floor(threshold)
        self.adaptive = adaptive if threshold is None else None
        self.thr_tab = None
        self.set_run_starts(run_starts)
        base_alloc = allocator or owned_allocator(ctx)
        self._blocks = []

        def alloc(nbytes):                        # remember what this coder allocated, for close()
            b = base_alloc(nbytes)
            self._blocks.append(b)
            return b
        self._alloc = alloc
        self.frame_bytes = self.n * channels * sample_bytes
        self.mask_stride, self.filter_stride, self.witness_stride = self.strides(self.n)
        oalloc = self._out_alloc = out_allocator or alloc
        self.planar_luma, self.keep_interleaved, self.resident_gops = bool(planar_luma), bool(keep_interleaved), int(resident_gops)
        if self.planar_luma and self.adaptive is not None:
            raise ValueError("noise-adaptive thresholds read the interleaved frames: planar_luma needs an explicit threshold")
        self.luma_bytes = self.n * sample_bytes
        self.luma = (luma_block if luma_block is not None else alloc(self.luma_bytes * nframes * self.resident_gops)) if self.planar_luma else None
        if frames_block is not None:
            self.frames = frames_block
        elif self.planar_luma and not self.keep_interleaved:
            self.frames = None
        else:
            self.frames = alloc(self.frame_bytes * nframes * self.resident_gops)
        self.masks, self.ones = alloc(self.mask_stride * self.pairs), alloc(8 * self.pairs)
        self.filters, self.witness = oalloc(self.filter_stride * self.pairs), oalloc(self.witness_stride * self.pairs)
        self.stats = oalloc(8 * nat.STATS_PER_FRAME * self.pairs)
        self.params, self.k = (nat.FilterParams * self.pairs)(), (ctypes.c_double * self.pairs)()
        self.record = None
        self.gop = 0                                  # the resident GOP encode_begin() last coded
        self._values = self._voff = self._uncov = self._cut_stats = self._digests = None      # scratch blocks, allocated on first use
        self.bounds = None                            # the bound frame on the device
        if self.error_bounds is not None:
            self.bounds = alloc(self.frame_bytes)
            nat.check(nat.lib().rbf_memcpy_h2d(ctx.handle, self.bounds.ptr, self.error_bounds.ctypes.data, self.frame_bytes))
        self.keep_originals = bool(keep_originals)
        if self.keep_originals and self.frames is None:
            raise ValueError("keep_originals copies the interleaved frames (keep_interleaved=True)")
        self.originals = alloc(self.frame_bytes * nframes * self.resident_gops) if self.keep_originals else None
        if self.adaptive is not None:
            self.moments = alloc(16 * self.pairs)
            self.noise_plane = None                       # allocated on the first exact fallback

    def set_run_starts(self, run_starts):
        """Name the keyframes inside the block for the following encode() calls (see the constructor): a coder is sized by its frame
        count, not by where its runs start, so one coder serves every block of a stream whatever the keyframe interval."""
        self.run_starts = None
        self.run_bounds = None                        # (bounds are per run: new runs, no bounds)
        self.skipped = [False] * self.pairs
        if run_starts:
            self.run_starts = (ctypes.c_uint8 * self.F)()
            for t in run_starts:
                if not 0 <= int(t) < self.F:
                    raise ValueError("run start %r outside the block of %d frames" % (t, self.F))
                if int(t) > 0:
                    self.run_starts[int(t)] = 1
                    self.skipped[int(t) - 1] = True

    def runs(self):
        """[(first frame, end)] of the block's runs in frame order, a run of one frame included: frame 0 and every run start open one."""
        starts = [0] + [t for t in range(1, self.F) if self.run_starts is not None and self.run_starts[t]]
        return list(zip(starts, starts[1:] + [self.F]))

    def set_run_bounds(self, bounds):
        """A bound PER RUN in place of the one max_error, for the following encode() calls: one integer in 0..max_error per run of runs()
        (the coder's max_error is the ceiling: it is what the coder was checked against and what error_stats() counts over_bound with),
        or None to return to the single max_error.  encode_begin() then calls the scalar hold entry (hold_mode's) once per maximal
        stretch of consecutive runs that share a bound -- with the stretch's first frame, its frame count and its own slice of the run
        starts -- and not at all for a stretch whose bound is 0: those runs are coded exactly.  The records carry no bound, so every
        decoder reads the result.  set_run_starts() forgets the bounds: call it first.  Not with error_bounds."""
        if bounds is None:
            self.run_bounds = None
            return
        if self.bounds is not None or not self.max_error:
            raise ValueError("run bounds replace a scalar max_error > 0 (their ceiling): not with error_bounds, not on a lossless coder")
        bounds = list(bounds)
        if len(bounds) != len(self.runs()):
            raise ValueError("one bound per run: the block has %d runs, got %d bounds" % (len(self.runs()), len(bounds)))
        for d in bounds:
            if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= d <= self.max_error:
                raise ValueError("a run's bound must be an integer in 0..max_error = %d, got %r" % (self.max_error, d))
        self.run_bounds = [int(d) for d in bounds]

    def _hold_stretches(self):
        """[(first frame, end, bound)] of the maximal stretches of consecutive runs that share a non-zero bound (set_run_bounds)."""
        runs, out, i = self.runs(), [], 0
        while i < len(runs):
            j = i
            while j + 1 < len(runs) and self.run_bounds[j + 1] == self.run_bounds[i]:
                j += 1
            if self.run_bounds[i]:
                out.append((runs[i][0], runs[j][1], self.run_bounds[i]))
            i = j + 1
        return out

    def hold_sweep(self, candidates, lookahead=None, gop=0):
        """What every candidate bound would do to every run of resident GOP `gop` (rbf_hold_sweep, include/rbf.h): a structured array
        (_native.SWEEP_ROW) of shape (runs, candidates) -- row [r, i]: sse, updates and max_abs of run r of runs() under the hold with
        max_error = candidates[i], first-value or (lookahead) look-ahead; default: the coder's hold_mode.  candidates: 1..8 strictly
        ascending integers <= 255, 0 allowed as the first.  Read-only, ONE read of the block AS IT IS NOW with the coder's current run
        starts, whatever the number of candidates: call it before any hold has rewritten the block, the caveat of cut_stats().  Blocks
        until the rows are on the host."""
        if self.planar_luma or self.frames is None:
            raise ValueError("the hold sweep reads the interleaved frames: not with planar_luma")
        assert 0 <= gop < self.resident_gops
        cands = [int(d) for d in candidates]
        if any(d < 0 for d in cands):
            raise ValueError("candidates must be non-negative, got %r" % (cands,))
        look = self.hold_mode == "lookahead" if lookahead is None else bool(lookahead)
        rows = np.zeros((len(self.runs()), len(cands)), dtype=nat.SWEEP_ROW)
        nat.check(nat.lib().rbf_hold_sweep(self.ctx.handle, self._block_ptr(self.frames, gop), self.frame_bytes, self.F, self.W, self.H,
                                           self.C, self.sb, self.run_starts, int(look), (ctypes.c_uint32 * max(1, len(cands)))(*cands),
                                           len(cands), rows.ctypes.data))
        return rows

    @staticmethod
    def strides(n):
        """(mask, filter, witness) row strides in bytes for frames of n pixels."""
        fstride = (nat.packed_stride(int(n * 0.32) + 64) + 15) // 16 * 16     # l <= 0.317 n for every density
        return nat.packed_stride(n), fstride, nat.packed_stride(n)

    @staticmethod
    def record_bytes(n, pairs):
        """Bytes a TorchArena needs for the output records (filters | witnesses | stats) of `pairs` frames."""
        _, fs, ws = GopCoder.strides(n)
        r = lambda x: (x + 255) // 256 * 256
        return r(fs * pairs) + r(ws * pairs) + r(8 * nat.STATS_PER_FRAME * pairs)

    def close(self):
        """Free the library-owned blocks this coder allocated (torch-backed blocks die with their tensors)."""
        for b in self._blocks:
            if isinstance(b, _OwnedBlock):
                b.buf.free()
        self._blocks = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _block_ptr(self, block, gop):
        """Where resident GOP `gop` starts in a block of interleaved frames (self.frames, self.originals)."""
        return block.ptr + gop * self.frame_bytes * self.F

    def load_frames(self, frames, gop=0):
        """Upload one GOP of interleaved (F, H, W, C) frames into slot `gop`.  With planar_luma the Y planes are extracted on
        the device (rbf_extract_luma_batch) when the interleaved frames are kept, else on the host (only luma crosses PCIe)."""
        frames = np.ascontiguousarray(frames)
        assert frames.nbytes == self.frame_bytes * self.F, (frames.shape, frames.dtype)
        assert 0 <= gop < self.resident_gops
        self.mark_loaded(gop)
        if self.frames is not None:
            dst = self.frames.ptr + gop * self.frame_bytes * self.F
            nat.check(nat.lib().rbf_memcpy_h2d(self.ctx.handle, dst, frames.ctypes.data, frames.nbytes))
            if self.keep_originals:                   # before any hold rewrites the block
                nat.check(nat.lib().rbf_memcpy_d2d(self.ctx.handle, self.originals.ptr + gop * self.frame_bytes * self.F, dst, frames.nbytes))
            if self.planar_luma:
                nat.check(nat.lib().rbf_extract_luma_batch(self.ctx.handle, dst, self.frame_bytes, self.F, self.W, self.H, self.W * self.C * self.sb,
                                                           self.C * self.sb, self.sb, self.luma.ptr + gop * self.luma_bytes * self.F))
        else:
            self.load_luma(frames.reshape(self.F, self.H, self.W, self.C)[..., 0], gop)

    def mark_loaded(self, gop=0):
        """Slot `gop` holds new input frames (load_frames() calls this; a caller that fills the block some other way does): the next
        encode() of it runs the look-ahead hold again."""
        self._held.discard(gop)
        self._key_streams.pop(gop, None)

    def load_luma(self, planes, gop=0):
        """Upload one GOP of dense (F, H, W) Y planes (planar_luma coders)."""
        assert self.planar_luma and 0 <= gop < self.resident_gops
        planes = np.ascontiguousarray(planes)
        assert planes.nbytes == self.luma_bytes * self.F, (planes.shape, planes.dtype)
        nat.check(nat.lib().rbf_memcpy_h2d(self.ctx.handle, self.luma.ptr + gop * self.luma_bytes * self.F, planes.ctypes.data, planes.nbytes))

    def _noise(self, first, count, moments_ptr, planes_ptr):
        nat.check(nat.lib().rbf_noise_moments_batch(
            self.ctx.handle, self.frames.ptr + first * self.frame_bytes, self.frame_bytes, count, self.W, self.H,
            self.W * self.C * self.sb, self.C * self.sb, self.sb, moments_ptr, planes_ptr))

    def adaptive_floors(self):
        """Integer thresholds of the reference's adaptive rule for frames 1..F-1 (engine.py has the
        reasoning: exact integer moments decide the floor; the float32 replay is the rare fallback)."""
        from .engine import adaptive_threshold, adaptive_threshold_band, threshold_floor
        self._noise(1, self.pairs, self.moments.ptr, None)
        self.ctx.sync()
        moments = self.moments.numpy(self.ctx)[:16 * self.pairs].view(np.int64).reshape(self.pairs, 2)
        floors = []
        for i in range(self.pairs):
            lo, hi = adaptive_threshold_band(self.n, int(moments[i, 0]), int(moments[i, 1]), *self.adaptive)
            if lo != hi:
                if self.noise_plane is None:
                    self.noise_plane = self._alloc(4 * self.n)
                    self.moments1 = self._alloc(16)
                self._noise(1 + i, 1, self.moments1.ptr, self.noise_plane.ptr)
                self.ctx.sync()
                plane = self.noise_plane.numpy(self.ctx)[:4 * self.n].view(np.float32).reshape(self.H, self.W)
                lo = threshold_floor(adaptive_threshold(np.std(plane), *self.adaptive))
            floors.append(lo)
        return floors

    def key_bounds(self):
        """The per-channel bounds of the coder's near-lossless stage: max_error for every channel, or the channels' entries of a bound
        frame that is the same at every pixel.  ValueError for a lossless coder and for bounds that differ from pixel to pixel (a
        decoder of a bounded keyframe would need the map, which its record does not carry)."""
        if self.error_bounds is None:
            d = [self.max_error] * self.C
        else:
            e = self.error_bounds.reshape(-1, self.C)
            if not bool((e == e[0]).all()):
                raise ValueError("bounded keyframes carry one bound per channel: not with error_bounds that differ from pixel to pixel")
            d = [int(v) for v in e[0]]
        if not any(d):
            raise ValueError("bounded keyframes are a near-lossless stage: they need max_error > 0 or error_bounds")
        return d

    def quantise_run_starts(self, sample_coder, frames=None, gop=0):
        """Bounded-error keyframes: quantise the run firsts of resident GOP `gop` IN PLACE within key_bounds() and return {j: the type-7
        sample stream of frame j} (SampleCoder.encode_near: rbf_rice_encode_intra_near, one launch sequence and one exact-size download).
        frames: the block indices to quantise (default: frame 0 and every run start); each has to be a run first -- the hold never
        writes those, so what encode() and everything behind it see of them is Y, and the inter-frames that hang off them are held
        against Y.  Call it after load_frames() (and align_pans / set_run_starts), before encode().  The stage runs ONCE PER
        load_frames(): a second call returns the first call's streams and launches nothing (Y is a fixed point of the rule, so a
        second pass would only repeat the work)."""
        if self.planar_luma or self.frames is None:
            raise ValueError("the keyframe quantiser rewrites the interleaved frames: not with planar_luma")
        assert 0 <= gop < self.resident_gops
        if gop in self._key_streams:
            return self._key_streams[gop]
        firsts = [0] + [t for t in range(1, self.F) if self.run_starts is not None and self.run_starts[t]]
        idx = firsts if frames is None else sorted({int(j) for j in frames})
        if any(j not in firsts for j in idx):
            raise ValueError("frames %r: only run firsts (%r) can be bounded keyframes" % (idx, firsts))
        out = {}
        if idx:
            streams = sample_coder.encode_near(self._block_ptr(self.frames, gop), self.frame_bytes, self.F, idx, self.W, self.H, self.C, self.sb,
                                               self.key_bounds())
            out = dict(zip(idx, streams))
        self._key_streams[gop] = out
        return out

    def encode(self, gop=0):
        """Enqueue one full pass over resident GOP `gop`; returns after the Bloom kernels are enqueued."""
        self.encode_begin(gop)
        self.encode_finish()

    def encode_begin(self, gop=0):
        """First half (rbf_encode_gop_begin): the mask stage of resident GOP `gop` is enqueued; returns without waiting.
        A caller that drives several coders (one context each) begins the next coder's GOP before it finishes this one."""
        if self.adaptive is not None:
            self.thresholds = self.adaptive_floors()
            self.thr_tab = (ctypes.c_int32 * self.pairs)(*self.thresholds)
        self.gop = gop
        if self.planar_luma:                          # dense Y planes: pixel stride = one sample
            src, fstride, pitch, pstride = self.luma.ptr + gop * self.luma_bytes * self.F, self.luma_bytes, self.W * self.sb, self.sb
        else:
            src, fstride, pitch, pstride = self.frames.ptr + gop * self.frame_bytes * self.F, self.frame_bytes, self.W * self.C * self.sb, self.C * self.sb
        geometry = (self.ctx.handle, src, fstride, self.F, self.W, self.H, self.C, self.sb)
        if self.run_bounds is not None:               # a bound per run: the scalar entry, once per stretch of runs that share a bound
            if len(self.run_bounds) != len(self.runs()):
                raise ValueError("the run bounds no longer fit the block's runs: set_run_bounds() after set_run_starts()")
            look = self.hold_mode == "lookahead"
            if not look or gop not in self._held:
                hold = nat.lib().rbf_temporal_lookahead_runs if look else nat.lib().rbf_temporal_hold_runs
                for a, b, d in self._hold_stretches():
                    marks = None if self.run_starts is None else (ctypes.c_uint8 * (b - a))(*self.run_starts[a:b])
                    nat.check(hold(self.ctx.handle, src + a * fstride, fstride, b - a, self.W, self.H, self.C, self.sb, d, marks))
                if look:
                    self._held.add(gop)
        elif (self.max_error or self.bounds is not None) and self.hold_mode == "lookahead":
            if gop not in self._held:                 # not idempotent: once per load_frames(); after that the block IS its held sequence
                if self.bounds is not None:
                    nat.check(nat.lib().rbf_temporal_lookahead_runs_map(*geometry, self.bounds.ptr, self.run_starts))
                else:
                    nat.check(nat.lib().rbf_temporal_lookahead_runs(*geometry, self.max_error, self.run_starts))
                self._held.add(gop)
        elif self.bounds is not None:                 # near-lossless: the block becomes its held sequence, which is then coded exactly
            nat.check(nat.lib().rbf_temporal_hold_runs_map(*geometry, self.bounds.ptr, self.run_starts))
        elif self.max_error:
            nat.check(nat.lib().rbf_temporal_hold_runs(*geometry, self.max_error, self.run_starts))
        nat.check(nat.lib().rbf_encode_runs_begin_ex(
            self.ctx.handle, src, fstride, self.F, self.W, self.H,
            pitch, pstride, self.sb, self.thr, self.thr_tab, self.run_starts, ctypes.byref(self.seeds),
            self.masks.ptr, self.mask_stride, self.ones.ptr,
            self.filters.ptr, self.filter_stride, self.witness.ptr, self.witness_stride, self.stats.ptr, self.mask_channels))

    def encode_ready(self):
        """True once the mask stage's counts have reached the host (encode_finish will not wait)."""
        ready = ctypes.c_int(0)
        nat.check(nat.lib().rbf_encode_gop_poll(self.ctx.handle, ctypes.byref(ready)))
        return bool(ready.value)

    def encode_finish(self):
        """Second half (rbf_encode_gop_finish): waits for the counts, plans the filters (float64, host), enqueues the Bloom kernels."""
        nat.check(nat.lib().rbf_encode_gop_finish(self.ctx.handle, self.params, self.k))

    def pack(self, block=None):
        """Compact this GOP's output rows into one exact-size record on the device (rbf_pack_records);
        returns the block holding it.  `block`: where to put it (default: a block of the worst-case size)."""
        if block is None:
            if self.record is None:
                self.record = self._out_alloc(int(nat.lib().rbf_record_max_bytes(self.pairs, self.n)))
            block = self.record
        nat.check(nat.lib().rbf_pack_records(
            self.ctx.handle, self.pairs, self.n, self.params, self.k, self.masks.ptr, self.mask_stride,
            self.filters.ptr, self.filter_stride, self.witness.ptr, self.witness_stride, self.stats.ptr,
            block.ptr, block.nbytes // 8 * 8))
        return block

    def gather_values(self, check_uncovered=False):
        """A2 for the whole GOP (rbf_gather_values_batch): list of per-pair arrays of the changed pixels'
        samples (all channels, raster order, frame dtype) taken from frame f+1; with check_uncovered also
        the per-pair count of pixels that changed in some channel although their mask bit is 0."""
        self.ctx.sync()
        ones = self.ones.numpy(self.ctx)[:8 * self.pairs].view(np.uint64)
        total = int(ones.sum())
        if self._values is None or self._values.nbytes < max(8, total * self.C * self.sb):
            self._values = self._alloc(max(8, total * self.C * self.sb))
        if self._voff is None:
            self._voff = self._alloc(8 * (self.pairs + 1))
            self._uncov = self._alloc(8 * self.pairs)
        if self.frames is None:
            raise ValueError("gather_values needs the interleaved frames (keep_interleaved=True)")
        nat.check(nat.lib().rbf_gather_values_batch(
            self.ctx.handle, self._block_ptr(self.frames, self.gop), self.frame_bytes, self.F, self.W, self.H, self.W * self.C * self.sb, self.C * self.sb,
            self.sb, self.C, self.masks.ptr, self.mask_stride, self._values.ptr, total, self._voff.ptr,
            self._uncov.ptr if check_uncovered else None))
        self.ctx.sync()
        off = self._voff.numpy(self.ctx)[:8 * (self.pairs + 1)].view(np.uint64)
        assert int(off[-1]) == total, "mask changed since the ones counts were taken"
        dt = np.uint8 if self.sb == 1 else np.uint16
        flat = self._values.numpy(self.ctx)[:total * self.C * self.sb].view(dt)
        vals = [flat[int(off[f]) * self.C:int(off[f + 1]) * self.C].copy() for f in range(self.pairs)]
        if not check_uncovered:
            return vals
        return vals, self._uncov.numpy(self.ctx)[:8 * self.pairs].view(np.uint64).copy()

    def rice_streams(self, ones, codec):
        """The sample-codec streams of every pair (type-4 value fields, sample_codec.py): pair f's residuals of frame f+1 against frame f at
        mask f's '1' pixels, all pairs in ONE rbf_rice_encode_inter launch sequence and one exact-size download.  ones: the masks' set-bit
        counts (results_packed()'s); codec: the SampleCoder of this coder's context.  A skipped pair gets the empty stream."""
        if self.frames is None:
            raise ValueError("rice_streams needs the interleaved frames (keep_interleaved=True)")
        return codec.encode_inter(self._block_ptr(self.frames, self.gop), self.frame_bytes, self.F, self.W, self.H,
                                  self.C, self.sb, self.masks.ptr, self.mask_stride, ones)

    def cut_stats(self, gop=0, tolerance=0):
        """The scene-cut statistics of resident GOP `gop` (rbf_cut_stats, include/rbf.h): a (pairs, 3) uint64 array, row f = (moving,
        inter_bits, intra_bits) of frame f + 1 against frame f; container.cut_frames applies the rule.  Read-only, ONE launch sequence over
        the block AS IT IS NOW and one download of 24 bytes per pair: the surface calls it directly after load_frames(), before any hold
        has rewritten the block -- after an encode() with max_error > 0 it would describe the held frames.  tolerance: a pixel counts as
        moving when a sample differs by more than this from the frame before (what a hold of that bound would keep still is not counted)."""
        if self.frames is None:
            raise ValueError("cut_stats needs the interleaved frames (keep_interleaved=True)")
        assert 0 <= gop < self.resident_gops
        if self.pairs < 1:
            return np.zeros((0, 3), dtype=np.uint64)
        if self._cut_stats is None:
            self._cut_stats = self._alloc(24 * self.pairs)
        nat.check(nat.lib().rbf_cut_stats(self.ctx.handle, self._block_ptr(self.frames, gop), self.frame_bytes, self.F, self.W,
                                          self.H, self.C, self.sb, int(tolerance), self._cut_stats.ptr))
        self.ctx.sync()
        return self._cut_stats.numpy(self.ctx, 24 * self.pairs)[:24 * self.pairs].view(np.uint64).reshape(self.pairs, 3).copy()

    def pan_search(self, pan_range, tolerance=0, gop=0):
        """The pan statistics of resident GOP `gop` (rbf_pan_search, include/rbf.h): a structured array (_native.PAN_ROW) of `pairs` rows
        -- the best integer shift of frame f + 1 against frame f within +-pan_range pixels, its SAD and the SAD of no shift on the luma
        grid, and how many pixels of the whole frame move with and without it (tolerance as in cut_stats).  Read-only on the block AS IT
        IS NOW, with the coder's current run starts (the row in front of one is zeros); blocks until the rows are on the host."""
        if self.planar_luma or self.frames is None:
            raise ValueError("the pan search reads the interleaved frames: not with planar_luma")
        assert 0 <= gop < self.resident_gops
        rows = np.zeros(self.pairs, dtype=nat.PAN_ROW)
        if self.pairs:
            nat.check(nat.lib().rbf_pan_search(self.ctx.handle, self._block_ptr(self.frames, gop), self.frame_bytes, self.F, self.W,
                                               self.H, self.C, self.sb, int(pan_range), int(tolerance), self.run_starts, rows.ctypes.data))
        return rows

    def roll_frames(self, offsets, gop=0):
        """Roll the frames of resident GOP `gop` in place (rbf_roll_frames): frame j becomes new(x, y) = old((x + ox_j) mod W, (y + oy_j)
        mod H) with offsets[j] = (ox_j, oy_j); a frame with a zero offset is not touched.  With keep_originals the originals copy is rolled
        by the same offsets, so that error_stats() still compares like with like."""
        if self.planar_luma or self.frames is None:
            raise ValueError("the roll moves the interleaved frames: not with planar_luma")
        assert len(offsets) == self.F and 0 <= gop < self.resident_gops
        if not any(int(ox) % self.W or int(oy) % self.H for ox, oy in offsets):
            return
        flat = (ctypes.c_int32 * (2 * self.F))(*[int(v) for o in offsets for v in o])
        for block in (self.frames, self.originals):
            if block is not None:
                nat.check(nat.lib().rbf_roll_frames(self.ctx.handle, self._block_ptr(block, gop), self.frame_bytes, self.F, self.W,
                                                    self.H, self.C * self.sb, flat))
        self.mark_loaded(gop)                         # the block holds new input: a look-ahead hold runs after the roll, not before

    def align_pans(self, pan_range, tolerance=0, gop=0):
        """Make resident GOP `gop` still: search every pair's shift (pan_search), apply the rule and accumulate (container.pan_offsets: a
        pair adopts its best shift iff fewer pixels move with it; the offsets add up along a run and start at 0 at every run start) and
        roll every frame by its cumulative offset in place (roll_frames) -- frame j then holds S_j(p) = F_j((p + c_j) mod (W, H)), and pair
        j of the block differs in exactly moving_best (or moving_zero) pixels.  Call it directly after load_frames(), before cut_stats()
        and encode().  Returns (offsets, rows, adopted): the F cumulative offsets (ox, oy), the rows of pan_search, and pan_offsets'
        [(j, dx, dy)] of the pairs that adopted a shift.  Not for a planar_luma coder."""
        from .container import pan_offsets
        rows = self.pan_search(pan_range, tolerance, gop)
        starts = [t for t in range(1, self.F) if self.run_starts is not None and self.run_starts[t]]
        offsets, adopted = pan_offsets(rows, starts, self.W, self.H)
        self.roll_frames(offsets, gop)
        return offsets, rows, adopted

    def error_stats(self):
        """What the resident block of the GOP encode() last coded differs from its originals by (keep_originals=True; rbf_error_stats,
        include/rbf.h): a structured array (_native.ERROR_ROW) of F rows -- sse, differing, over_bound, max_abs per frame, over_bound
        against the coder's bound frame or its max_error.  One read of both blocks, no decode: a decoder rebuilds the resident block
        exactly, so this is the decoded clip's quality.  Valid after encode(); blocks until the rows are on the host."""
        if self.originals is None:
            raise ValueError("error_stats needs the uploaded frames: GopCoder(keep_originals=True)")
        rows = np.zeros(self.F, dtype=nat.ERROR_ROW)
        nat.check(nat.lib().rbf_error_stats(self.ctx.handle, self._block_ptr(self.originals, self.gop), self.frame_bytes,
                                            self._block_ptr(self.frames, self.gop), self.frame_bytes,
                                            self.F, self.W, self.H, self.C, self.sb, None if self.bounds is None else self.bounds.ptr,
                                            self.max_error, rows.ctypes.data))
        return rows

    def frame_digests(self):
        """FD1 of the F resident frames of the GOP encode() last coded (integrity.py): ONE rbf_frame_digest_batch over the block -- bytes the
        hold and the mask stage have just read -- and one download of 8 F bytes; uint64[F].  Call it after encode(): with max_error > 0 the
        block then holds the HELD frames, which are what the records code and a decoder rebuilds.  (A run's first frame is never written
        by the hold, rbf_kernels_hold.h: its digest is its original's.)"""
        if self.frames is None:
            raise ValueError("frame_digests needs the interleaved frames (keep_interleaved=True)")
        from .integrity import digests_device
        if self._digests is None:
            self._digests = self._alloc(8 * self.F)
        return digests_device(self.ctx, self._block_ptr(self.frames, self.gop), self.frame_bytes, self.F,
                              self.frame_bytes, out=self._digests)

    def results_packed(self):
        """What results() returns, through ONE exact-size download: the rows are compacted into a record on the device (rbf_pack_records:
        header + the used bytes of every filter and witness, ~150 KB per 1080p frame instead of ~600 KB of padded rows), the record's
        32-byte header says how many bytes to fetch.  Rows carry `filter` / `witness` (and `mask` only for frames the reference passes
        through uncoded, l == 0) as views of the downloaded record; `ones` comes from the mask stage's counts."""
        from .dist import unpack_device_record, record_used_bytes
        block = self.pack()
        self.ctx.sync()
        used = record_used_bytes(block.numpy(self.ctx, 32))
        raw = block.numpy(self.ctx, (used + 7) // 8 * 8)
        ones = self.ones.numpy(self.ctx)[:8 * self.pairs].view(np.uint64)
        rows = unpack_device_record(raw, self.n, copy=False)
        assert len(rows) == self.pairs
        for f, r in enumerate(rows):
            r["ones"] = int(ones[f])
            if r.get("skipped"):
                assert self.skipped[f] and r["ones"] == 0
        return rows

    def results(self):
        """Download: list of per-frame dicts (mask/filter/witness packed uint8, counts, k, l)."""
        self.ctx.sync()
        def rows(block, stride):                       # blocks may be padded (arena alignment)
            return block.numpy(self.ctx)[:self.pairs * stride].reshape(self.pairs, stride)
        masks = rows(self.masks, self.mask_stride)
        filt = rows(self.filters, self.filter_stride)
        wit = rows(self.witness, self.witness_stride)
        stats = rows(self.stats, 8 * nat.STATS_PER_FRAME).view(np.uint64)
        ones = self.ones.numpy(self.ctx)[:8 * self.pairs].view(np.uint64)
        out = []
        for f in range(self.pairs):
            if self.skipped[f]:                        # the pair across a keyframe: not coded (its mask row is zeros, ones 0)
                assert int(self.params[f].m) == 0 and int(self.params[f].floor_k) == nat.PAIR_SKIPPED and int(ones[f]) == 0
                out.append({"skipped": True, "ones": 0, "k": 0.0, "l": 0, "witness_bits": int(stats[f, 0]), "mask": masks[f, :(self.n + 7) // 8].copy()})
                continue
            m = int(self.params[f].m)
            wb = int(stats[f, 0])
            out.append({"mask": masks[f, :(self.n + 7) // 8].copy(), "ones": int(ones[f]), "k": float(self.k[f]), "l": m,
                        "floor_k": int(self.params[f].floor_k), "threshold": int(self.params[f].threshold),
                        "filter": filt[f, :(m + 7) // 8].copy(), "witness": wit[f, :(wb + 7) // 8].copy(),
                        "witness_bits": wb, "filter_ones": int(stats[f, 1])})
        return out
