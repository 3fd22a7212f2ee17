"""Synthetic YUV444 frame sequences for tests and bench (no network, no datasets).

Recipe: `rng = np.random.default_rng(seed)`; keyframe of uniform random
samples; every following frame changes a Bernoulli(p) set of pixels -- a non-zero luma
residual plus fresh chroma -- so that with threshold 0 the luma mask marks exactly the
pixels that changed and reconstruction from (mask, values) is exact.

p = P_KSTAR_2_3 makes the reference's parameter rule pick k* = 2.3
(k = log2((1-p) ln^2 2 / p), improved_video_compressor.py:185).
"""
import math

import numpy as np

P_KSTAR_2_3 = 1.0 / (1.0 + 2.0 ** 2.3 / math.log(2.0) ** 2)   # 0.08888997000980829


def next_frame(rng, frame, p, scratch=None):
    """Return a new frame differing from `frame` on a Bernoulli(p) pixel set.  `scratch`: reusable (H, W) float64 array for
    the Bernoulli draws (same stream as rng.random((h, w)); a fresh 16 MB array per frame costs more in page faults than
    everything else here)."""
    h, w = frame.shape[:2]
    bits = 8 * frame.dtype.itemsize
    if scratch is None:
        scratch = np.empty((h, w), dtype=np.float64)
    change = rng.random(out=scratch) < p
    idx = np.flatnonzero(change)                  # raster order = the order boolean-mask assignment uses (same frames, ~10x faster)
    cnt = int(idx.size)
    out = frame.copy()
    flat = out.reshape(-1, out.shape[2])
    if bits == 8:
        resid = rng.integers(1, 256, cnt, dtype=np.uint16)
        flat[idx, 0] = ((flat[idx, 0].astype(np.uint16) + resid) & 0xFF).astype(np.uint8)
    else:
        # residuals in 1..32767: avoids the int16 blind spot |d| == 32768 (np.abs(int16 -32768) < 0)
        resid = rng.integers(1, 32768, cnt, dtype=np.uint32)
        flat[idx, 0] = ((flat[idx, 0].astype(np.uint32) + resid) & 0xFFFF).astype(np.uint16)
    flat[idx, 1] = rng.integers(0, 1 << bits, cnt, dtype=frame.dtype)
    flat[idx, 2] = rng.integers(0, 1 << bits, cnt, dtype=frame.dtype)
    return out


def make_gop(seed, width, height, nframes, p=P_KSTAR_2_3, dtype=np.uint8):
    """nframes interleaved YUV444 frames of shape (H, W, 3)."""
    rng = np.random.default_rng(seed)
    bits = 8 * np.dtype(dtype).itemsize
    frames = [rng.integers(0, 1 << bits, (height, width, 3), dtype=dtype)]
    scratch = np.empty((height, width), dtype=np.float64)
    for _ in range(nframes - 1):
        frames.append(next_frame(rng, frames[-1], p, scratch))
    return frames


def make_clip_shard(seed, width, height, first, stop, interval=30, p=P_KSTAR_2_3, dtype=np.uint8, threads=None):
    """Frames [first, stop) of a long synthetic clip, as an array (stop-first, H, W, 3).  The clip is a sequence
    of independent GOPs of `interval` frames (GOP g = make_gop(seed * 1000 + g, ...)), so any rank can produce
    its shard -- including a halo frame -- without generating the frames before it, and every rank sees the
    same clip."""
    from concurrent.futures import ThreadPoolExecutor
    jobs = []
    g = first // interval
    while g * interval < stop:
        jobs.append((g, max(first, g * interval), min(stop, (g + 1) * interval)))
        g += 1

    def one(job):                                 # the GOPs are independent streams: one thread each (numpy drops the GIL in the big ops)
        g, lo, hi = job
        return make_gop(seed * 1000 + g, width, height, hi - g * interval, p=p, dtype=dtype)[lo - g * interval:]
    with ThreadPoolExecutor(max(1, min(len(jobs), threads or 16))) as pool:
        parts = list(pool.map(one, jobs))
    return np.stack([f for part in parts for f in part])


def make_mask(seed, n, p):
    """Flat 0/1 uint8 vector with Bernoulli(p) ones (the reference's `binary_input`)."""
    return (np.random.default_rng(seed).random(n) < p).astype(np.uint8)


def _rgb_to_yuv444(rgb, bits):
    """BT.601 full-range RGB -> YUV444 with rounding, per pixel: float (..., 3) RGB in the sample range -> integer (..., 3) YUV."""
    mid, top = float(1 << (bits - 1)), (1 << bits) - 1
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u = mid - 0.168736 * r - 0.331264 * g + 0.5 * b
    v = mid + 0.5 * r - 0.418688 * g - 0.081312 * b
    return np.clip(np.rint(np.stack([y, u, v], axis=-1)), 0, top)


def make_panning_gop(seed, width, height, nframes, velocities, moving=0.01, dtype=np.uint8, color_space="YUV", sensor_noise=0,
                     return_shifts=False):
    """nframes (H, W, 3) frames of a panning camera: a width x height window that moves over a larger make_camera_gop canvas (same seed and
    keywords: the scene changes under the window the way it does there).  velocities: one (vx, vy) -- the window moves that many pixels
    per frame -- or a sequence of nframes - 1 of them, one per pair ((0, 0) entries make a static stretch).  The window starts in the
    canvas's centre; the canvas has a margin of max(largest |v|, 15 % of the frame) on every side, so it stays within about 1.3x of the
    frame in each direction, and the path goes back and forth: a component that would leave the margin changes its sign from that pair
    on.  The picture content moves against the window, so the shift that aligns frame f with frame f-1 in the sense of rbf_pan_search
    (include/rbf.h) is (-vx, -vy) of the pair's actual velocity; return_shifts=True returns (frames, shifts) with those shifts,
    shifts[f-1] for frame f."""
    vel = np.asarray(velocities, dtype=np.int64)
    if vel.ndim == 1:
        vel = np.tile(vel, (max(0, nframes - 1), 1))
    if vel.shape != (max(0, nframes - 1), 2):
        raise ValueError("velocities must be one (vx, vy) or nframes - 1 = %d of them, got shape %r" % (nframes - 1, vel.shape))
    top = int(np.abs(vel).max()) if vel.size else 0
    mx, my = max(top, -(-15 * width // 100)), max(top, -(-15 * height // 100))
    canvas = make_camera_gop(seed, width + 2 * mx, height + 2 * my, nframes, moving=moving, dtype=dtype, color_space=color_space,
                             sensor_noise=sensor_noise)
    px, py, sx, sy = mx, my, 1, 1
    frames, shifts = [np.ascontiguousarray(canvas[0][py:py + height, px:px + width])], []
    for f in range(1, nframes):
        vx, vy = int(vel[f - 1, 0]), int(vel[f - 1, 1])
        if not 0 <= px + sx * vx <= 2 * mx:
            sx = -sx
        if not 0 <= py + sy * vy <= 2 * my:
            sy = -sy
        px, py = px + sx * vx, py + sy * vy
        shifts.append((-sx * vx, -sy * vy))
        frames.append(np.ascontiguousarray(canvas[f][py:py + height, px:px + width]))
    return (frames, shifts) if return_shifts else frames


def make_camera_gop(seed, width, height, nframes, moving=0.01, dtype=np.uint8, color_space="YUV", sensor_noise=0):
    """nframes (H, W, 3) frames that change the way camera footage does, unlike make_gop: a smooth RGB texture of which a Bernoulli(moving)
    set of pixels is perturbed by a few levels per channel in every pair, then converted to YUV444 (BT.601, rounded) -- so in every pair
    some pixels change in chroma while their luma stays the same (the luma residual mask misses them).  color_space="BGR" returns the RGB
    frames in B, G, R order before the conversion (channel 0 = B: some pixels change in G or R only).  16-bit: the samples are scaled to 16
    bits over a fixed fine texture, and in every pair a few channel-0 samples change by exactly 0x8000 (the int16 rule's blind spot).
    sensor_noise=a > 0: what a sensor adds to all of that -- every emitted sample of every frame carries independent uniform integer noise
    in [-a, a] (clipped to the sample range; drawn from a generator of its own, so the scene is the one sensor_noise=0 draws up to the
    jumps), so no two frames share a sample for long and the exact mask is almost all ones.  The moving set then jumps further: all three
    RGB channels of a moving pixel move the same way by 2a + 8 .. 2a + 14 levels (luma moves as far, short of clipping at the range's
    ends), which is more than 2a + max_error for every max_error <= 6 -- a near-lossless hold of that bound lets it through; the one pixel
    per pair whose luma is kept moves as it does without noise.  sensor_noise=0 (default) consumes the same random numbers and returns
    the same bytes as before the keyword existed."""
    if color_space not in ("YUV", "BGR"):
        raise ValueError("color_space must be 'YUV' or 'BGR'")
    sensor_noise = int(sensor_noise)
    if sensor_noise < 0:
        raise ValueError("sensor_noise must be >= 0")
    noise_rng = np.random.default_rng([int(seed), 0x5E4501]) if sensor_noise else None
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    bits = 8 * dtype.itemsize
    scale = 257.0 if bits == 16 else 1.0
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    rgb = np.empty((height, width, 3), dtype=np.float64)
    for c in range(3):                           # a few low-frequency waves and a gradient per channel: smooth, no two channels alike
        ph, fx, fy = rng.uniform(0, 2 * np.pi, 3), rng.uniform(0.5, 3.0, 3), rng.uniform(0.5, 3.0, 3)
        wave = sum(np.sin(2 * np.pi * (fx[i] * xx / width + fy[i] * yy / height) + ph[i]) for i in range(3))
        rgb[..., c] = 128.0 + 30.0 * wave + 40.0 * (xx / width - yy / height)
    top = (1 << bits) - 1
    rgb = np.clip(np.rint(rgb), 0, 255) * scale  # the scene, in sample units
    if bits == 16:
        rgb += rng.integers(0, 256, (height, width, 3))          # a fixed sub-level texture of a 16-bit sensor

    def render(x):
        return x if color_space == "BGR" else _rgb_to_yuv444(x, bits)

    cur = render(rgb)
    flip = np.zeros((height, width), dtype=bool)     # 16-bit: channel-0 samples currently offset by 0x8000
    frames = []

    def emit(img):
        f = np.ascontiguousarray(img[..., ::-1] if color_space == "BGR" else img).astype(dtype)
        if bits == 16:
            f[..., 0] ^= (flip * 0x8000).astype(np.uint16)
        if sensor_noise:                         # last: the noise sits on what the sensor sees, the 0x8000 offsets included
            noisy = f.astype(np.int64) + noise_rng.integers(-sensor_noise, sensor_noise + 1, f.shape)
            f = np.clip(noisy, 0, top).astype(dtype)
        frames.append(f)
    emit(cur)
    n = width * height
    for _ in range(nframes - 1):
        idx = np.flatnonzero(rng.random(n) < moving)
        if idx.size == 0:
            idx = rng.integers(0, n, 1)
        ys, xs = np.unravel_index(idx, (height, width))
        if sensor_noise:                                                   # a jump the noise cannot be mistaken for: see the docstring
            d = rng.integers(2 * sensor_noise + 8, 2 * sensor_noise + 15, (idx.size, 3)) * rng.choice((-1, 1), (idx.size, 1))
        else:
            d = rng.integers(-6, 7, (idx.size, 3))
        d[np.all(d == 0, axis=1), 1] = 1                                   # every chosen pixel moves
        d = d * scale
        d[0] = (3, 0, -8) if color_space == "YUV" else (2, -1, 0)          # luma kept, chroma moved -- at least once per pair (BGR: B = RGB[2])
        lv = np.clip(rgb[ys, xs] + d, 0, top)
        if color_space == "YUV":
            old = _rgb_to_yuv444(rgb[ys[0], xs[0]], bits)
            for _ in range(64):                                              # nudge pixel 0 until its Y rounds to the same value
                new = _rgb_to_yuv444(lv[0], bits)
                if new[0] == old[0] and np.any(new[1:] != old[1:]):
                    break
                lv[0] = np.clip(rgb[ys[0], xs[0]] + rng.integers(-8, 9, 3) * np.array([1, 0, 1]), 0, top)
        rgb[ys, xs] = lv
        cur[ys, xs] = render(lv)                     # (emit copies)
        if bits == 16:
            flip.reshape(-1)[rng.integers(0, n, 3)] ^= True
        emit(cur)
    return frames


def add_run_noise(frames, interval, amplitudes, seed=0):
    """Sensor noise whose amplitude varies from run to run: a copy of `frames` (an (F, H, W, C) array or a list of frames, uint8 / uint16)
    in which every sample of run r -- frames r * interval .. (r + 1) * interval - 1 -- carries independent uniform integer noise in
    [-a, a], a = amplitudes[r % len(amplitudes)], clipped to the sample range.  A clean stretch tolerates a large near-lossless bound
    at a given PSNR, a noisy one a small bound: what ImprovedVideoCompressor(target_psnr=...) tells apart.  Returns an array."""
    x = np.stack([np.asarray(f) for f in frames]) if not isinstance(frames, np.ndarray) else frames
    dtype, top = x.dtype, int(np.iinfo(x.dtype).max)
    rng = np.random.default_rng(seed)
    out = x.copy()
    for r, lo in enumerate(range(0, len(x), interval)):
        a = int(amplitudes[r % len(amplitudes)])
        run = x[lo:lo + interval].astype(np.int32)
        out[lo:lo + interval] = np.clip(run + rng.integers(-a, a + 1, run.shape), 0, top).astype(dtype)
    return out
