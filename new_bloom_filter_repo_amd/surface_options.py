"""The keyword checks of ImprovedVideoCompressor (its docstring is the user documentation): check_options says once what every keyword
must be and what the features that work on a resident block need from the others; check_blocks says what they need from a plan_range()
plan.  Host only: numpy and container.py, no native library.

A _Feature is something that works on the frames of a block while they are resident on the GPU.  needs: what it needs, IN THE ORDER its
refusals are tried -- "gop_batching", "inter_frames" (inter-frames at all: not inter_frames=False, keyframe_interval > 1), "all_channels"
(mask_channels="all"), "keyframe_blocks" (every block of a range starts at a keyframe: check_blocks).  resident / verb / off_keyframe: the
reason phrases of the gop_batching, all_channels and keyframe_blocks refusals."""
from collections import namedtuple

import numpy as np

from . import container

_Feature = namedtuple("_Feature", "needs resident verb off_keyframe")
PAN = _Feature(("gop_batching", "inter_frames", "all_channels", "keyframe_blocks"), "block to align", "rolls",
               "cumulative offset would need the pairs in front of it")
CUTS = _Feature(("gop_batching", "inter_frames"), "block to look at", None, None)
NEAR = _Feature(("all_channels", "inter_frames", "gop_batching", "keyframe_blocks"), "run to hold", "holds",
                "held state would live in another block's coder")
_REFUSALS = {"gop_batching": lambda f, name: "%s needs gop_batching=True: the frame-by-frame route has no resident %s" % (name, f.resident),
             "inter_frames": lambda f, name: "%s acts on inter-frames: not with inter_frames=False or keyframe_interval=1" % name,
             "all_channels": lambda f, name: "%s %s every sample of a pixel: it needs mask_channels='all'" % (name, f.verb)}

Options = namedtuple("Options", "pan_range error_bounds quality_report scene_cuts max_error hold_mode frame_digests verify_digests near "
                                "sample_codec mask_channels inter_frames keyframe_interval gop_batching block_frames gpu_lanes bounded_keyframes target_psnr")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _require(feature, name, have):
    """ValueError for the first of the feature's needs that the call does not meet (have: {need: a function that says whether it does})."""
    for need in feature.needs:
        if need in have and not have[need]():
            raise ValueError(_REFUSALS[need](feature, name))


def check_options(keyframe_interval=30, inter_frames=None, gop_batching=True, block_frames=None, gpu_lanes=2, mask_channels="luma",
                  sample_codec="zlib", max_error=0, frame_digests=False, verify_digests=True, hold_mode="first", scene_cuts=False,
                  error_bounds=None, quality_report=False, pan_range=0, target_psnr=None, bounded_keyframes=False):
    """The checked and normalised keywords of ImprovedVideoCompressor as an Options tuple, or the ValueError of the first refusal.
    `near` is the name the near-lossless stage goes by in messages ("error_bounds", "max_error > 0") or None.  The default block is
    two keyframe intervals (a multiple of the interval: every block of a stream has the same shape), at most 128 frames: small blocks
    start the host's zlib of the changed values early; the GPU's share of a block is a fraction of a millisecond either way."""
    have = {"gop_batching": lambda: bool(gop_batching), "all_channels": lambda: mask_channels == "all",
            "inter_frames": lambda: inter_frames is not False and max(1, int(keyframe_interval)) > 1}
    if not _is_int(pan_range) or not 0 <= pan_range <= 32:
        raise ValueError("pan_range must be an integer in 0..32, got %r" % (pan_range,))
    pan_range = int(pan_range)
    if pan_range:
        _require(PAN, "pan_range=%d" % pan_range, have)
        if error_bounds is not None:
            e = container.bounds_frame(error_bounds)
            if e.ndim >= 2 and not bool((e.reshape((-1,) + e.shape[2:]) == e.reshape((-1,) + e.shape[2:])[0]).all()):
                raise ValueError("pan_range=%d moves the pixels: not with error_bounds that differ from pixel to pixel "
                                 "(per-channel bounds are fine)" % pan_range)
    if error_bounds is not None:
        if _is_int(max_error) and max_error > 0:
            raise ValueError("error_bounds and max_error > 0 are two ways to say the bound: give one")
        container.bounds_frame(error_bounds)     # what can be refused without a frame is refused here
    if scene_cuts:
        _require(CUTS, "scene_cuts=True", have)
    if not _is_int(max_error) or max_error < 0:
        raise ValueError("max_error must be a non-negative integer, got %r" % (max_error,))
    max_error = int(max_error)
    if hold_mode not in ("first", "lookahead"):
        raise ValueError("hold_mode must be 'first' or 'lookahead', got %r" % (hold_mode,))
    if hold_mode == "lookahead" and not max_error and error_bounds is None:
        raise ValueError("hold_mode='lookahead' is a near-lossless stage: it needs max_error > 0 or error_bounds")
    near = "error_bounds" if error_bounds is not None else "max_error > 0" if max_error else None
    if near:
        _require(NEAR, near, have)
    if mask_channels not in ("luma", "all"):
        raise ValueError("mask_channels must be 'luma' or 'all', got %r" % (mask_channels,))
    if sample_codec not in ("zlib", "rice"):
        raise ValueError("sample_codec must be 'zlib' or 'rice', got %r" % (sample_codec,))
    if sample_codec == "rice" and inter_frames is False:
        raise ValueError("sample_codec='rice' writes 'BFV2' records; inter_frames=False asks for 'BFVC', which holds zlib keyframes only")
    if bounded_keyframes:
        if sample_codec != "rice":
            raise ValueError("bounded_keyframes=True writes type-7 records, whose payload is a sample stream: it needs sample_codec='rice'")
        if not near:
            raise ValueError("bounded_keyframes=True codes keyframes within the near-lossless bound: it needs max_error > 0 or error_bounds")
        e = None if error_bounds is None else container.bounds_frame(error_bounds)
        if e is not None and e.ndim >= 2:
            raise ValueError("bounded_keyframes=True: a type-7 record carries one bound per channel, and a decoder would need the map: "
                             "not with error_bounds of shape %r" % (e.shape,))
        if e is not None and not e.any():
            raise ValueError("bounded_keyframes=True needs a bound: error_bounds is all zero")
    if target_psnr is not None:
        if isinstance(target_psnr, bool) or not isinstance(target_psnr, (int, float, np.integer, np.floating)) \
                or not np.isfinite(target_psnr) or not target_psnr > 0:
            raise ValueError("target_psnr must be a finite positive number of dB, got %r" % (target_psnr,))
        if error_bounds is not None:
            raise ValueError("target_psnr picks one scalar bound per run (the sweep is scalar): not with error_bounds")
        if not max_error:
            raise ValueError("target_psnr picks every run's bound from 1..max_error: it needs max_error > 0 as the ceiling")
        if max_error > 255:
            raise ValueError("target_psnr sweeps bounds of at most 255: max_error=%d is above that" % max_error)
        if bounded_keyframes:
            raise ValueError("target_psnr measures the holds against exact keyframes (a keyframe would be quantised before the sweep "
                             "could see what the hold hangs off): not with bounded_keyframes=True")
        target_psnr = float(target_psnr)
    I = max(1, int(keyframe_interval))
    block_frames = max(2, int(block_frames)) if block_frames else min(128, max(2, 2 * I if 2 * I <= 128 else I))
    if target_psnr is not None and block_frames > 128:
        raise ValueError("target_psnr sweeps blocks of at most 128 runs of at most 128 frames: not with block_frames=%d" % block_frames)
    return Options(pan_range, error_bounds, bool(quality_report), bool(scene_cuts), max_error, hold_mode, bool(frame_digests),
                   bool(verify_digests), near, sample_codec, mask_channels, inter_frames, I, bool(gop_batching), block_frames,
                   max(1, int(gpu_lanes)), bool(bounded_keyframes), target_psnr)


def check_blocks(options, blocks, first_index, I):
    """ValueError when a feature of `options` that needs "keyframe_blocks" meets a plan_range() plan with a block that does not start at
    a keyframe (container.blocks_off_keyframes); the near-lossless stage is asked first."""
    off = container.blocks_off_keyframes(blocks, first_index, I)
    if not off:
        return
    for feature, name in ((NEAR, options.near and ("max_error=%d" % options.max_error if options.max_error else "error_bounds")),
                          (PAN, options.pan_range and "pan_range=%d" % options.pan_range)):
        if name and "keyframe_blocks" in feature.needs:
            raise ValueError("%s: the block that starts at frame %d does not start at a keyframe, so its %s; make block_frames (%d) a "
                             "multiple of keyframe_interval (%d) and start the range on a keyframe"
                             % (name, off[0][0], feature.off_keyframe, options.block_frames, I))
