"""References, layouts and inputs of the frame-preparation sweep (tests/test_gpu_frame_prep_sweep.py) -- a helper, not a test.  Pure numpy,
integer-exact: the 5x5 median residual and its moments (oracle.median_blur5, proven against a brute force by tests/test_adaptive_cpu.py),
BGR to gray (oracle.bgr_to_gray) and luma (sample 0).

Layout places a clip (F, H, W, C) into a byte buffer at a base offset, with a row pitch, a frame stride and a pixel stride of C samples
(the entries read 1 or 3 of them).  Every byte that is not a sample of the clip is noise, so a kernel that ignores the base, the pitch or
the stride reads a wrong sample INSIDE the buffer: a wrong answer, never a fault.  tests/test_frame_prep_cpu.py proves on the CPU that
every such misreading changes luma, gray and moments for every case the GPU sweep runs."""
import functools

import numpy as np

from oracle import oracle as orc

TILE_W, TILE_H = 64, 8                                             # csrc/rbf_kernels_noise.h: NZ_TILE_W, NZ_TILE_H
GUARD = 512
MAX_FRAMES = 65535                                                 # csrc/rbf_api.hip: frame_pass_rules
MAX_NOISE_HEIGHT = TILE_H * 65535                                  # the noise grid's y dimension


# ------------------------------------------------------------------ references
def top_of(dtype):
    return int(np.iinfo(dtype).max)


def median5(plane, mode="edge"):
    """The 13th smallest of every 5x5 window under numpy's padding `mode`: "edge" is the kernel's rule (oracle.median_blur5), "reflect"
    and "constant" (zeros) are what a wrong border rule would compute."""
    plane = np.asarray(plane)
    if mode == "edge":
        return orc.median_blur5(plane)
    padded = np.pad(plane, 2, mode=mode)
    win = np.lib.stride_tricks.sliding_window_view(padded, (5, 5)).reshape(plane.shape + (25,))
    return np.partition(win, 12, axis=-1)[..., 12].astype(plane.dtype)


def median5_signed16(plane):
    """What a network of SIGNED 16-bit min/max selects: the median of the samples read as int16."""
    return median5(np.ascontiguousarray(plane).view(np.int16)).view(np.uint16)


def median_net():
    """The comparator list of csrc/rbf_median_net.h, restated: [(a, b)] -- the minimum goes to wire a, the maximum to wire b."""
    net = []
    p = 1
    while p < 32:
        k = p
        while k >= 1:
            for j in range(k % p, 32 - k, 2 * k):
                for i in range(min(k, 32 - j - k)):
                    if (i + j) // (2 * p) == (i + j + k) // (2 * p) and i + j + k < 25:
                        net.append((i + j, i + j + k))
            k >>= 1
        p <<= 1
    return net


def median5_network(plane, signed_min=False, signed_max=False):
    """Wire 12 of the network over every replicated 5x5 window of a uint16 plane, as a kernel whose packed minimum and / or maximum
    compares SIGNED 16-bit halves would compute it.  With both unsigned it is the median (tests/test_frame_prep_cpu.py checks that)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint16)
    padded = np.pad(plane, 2, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(padded, (5, 5)).reshape(plane.shape + (25,))
    v = [win[..., i].copy() for i in range(25)]

    def pick(a, b, smaller, signed):
        ka, kb = (a.view(np.int16), b.view(np.int16)) if signed else (a, b)
        return np.where((ka <= kb) == smaller, a, b)

    for a, b in median_net():
        v[a], v[b] = pick(v[a], v[b], True, signed_min), pick(v[a], v[b], False, signed_max)
    return v[12]


def residual(plane, mode="edge", median=None):
    plane = np.ascontiguousarray(plane)
    med = median5(plane, mode) if median is None else median(plane)
    return plane.astype(np.int64) - med.astype(np.int64)


def moments_of(d):
    return [int(d.sum()), int((d * d).sum())]


def luma_ref(clip):
    return np.ascontiguousarray(clip[..., 0])


def gray_ref(clip):
    return np.stack([orc.bgr_to_gray(f) for f in clip])


def noise_ref(clip, mode="edge"):
    """(residual planes int64 (F, H, W), moments [[s1, s2]] as Python ints) of sample 0 of every frame."""
    d = np.stack([residual(f[..., 0], mode) for f in clip])
    return d, [moments_of(p) for p in d]


# ------------------------------------------------------------------ layouts
class Layout:
    """Where the samples of a clip (F, H, W, C) of `dtype` lie in a byte buffer: sample c of pixel (x, y) of frame f at
    base + f * frame_stride + y * row_pitch + x * pixel_stride + c * sample_bytes."""

    def __init__(self, shape, dtype, base=0, row_pitch=None, frame_stride=None, name="dense"):
        self.F, self.H, self.W, self.C = (int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.sb = self.dtype.itemsize
        self.pixel_stride = self.C * self.sb
        self.dense_pitch = self.W * self.pixel_stride
        self.row_pitch = self.dense_pitch if row_pitch is None else int(row_pitch)
        self.dense_stride = self.H * self.row_pitch
        self.frame_stride = self.dense_stride if frame_stride is None else int(frame_stride)
        self.base, self.name = int(base), name
        assert self.row_pitch >= self.dense_pitch and self.frame_stride >= self.dense_stride
        self.nbytes = self.base + (self.F - 1) * self.frame_stride + (self.H - 1) * self.row_pitch + self.dense_pitch

    def offsets(self, base=None, row_pitch=None, frame_stride=None):
        """int64 (F, H, W, C): the byte offset of every sample, optionally as a reader with another base, pitch or stride forms it."""
        base = self.base if base is None else base
        pitch = self.row_pitch if row_pitch is None else row_pitch
        stride = self.frame_stride if frame_stride is None else frame_stride
        f, y, x, c = np.ix_(*(np.arange(n, dtype=np.int64) for n in (self.F, self.H, self.W, self.C)))
        return base + f * stride + y * pitch + x * self.pixel_stride + c * self.sb

    def place(self, clip, seed=12345):
        """uint8 [nbytes]: the clip at its places, every other byte from a generator -- no padding byte run repeats its neighbours."""
        clip = np.ascontiguousarray(clip, dtype=self.dtype)
        assert clip.shape == (self.F, self.H, self.W, self.C), (clip.shape, (self.F, self.H, self.W, self.C))
        buf = np.random.default_rng(seed).integers(0, 256, self.nbytes, dtype=np.uint8)
        off = self.offsets()
        raw = clip.reshape(clip.shape + (1,)).view(np.uint8)        # (F, H, W, C, sb), little endian like the device
        for b in range(self.sb):
            buf[off + b] = raw[..., b]
        return buf

    def read(self, buf, **as_if):
        """The clip a reader finds in buf; as_if: base / row_pitch / frame_stride of a reader that ignores the layout's."""
        off = self.offsets(**as_if)
        assert off.min() >= 0 and off.max() + self.sb <= len(buf), "a misreading stays inside the buffer"
        out = np.zeros(off.shape, np.uint32)
        for b in range(self.sb):
            out |= buf[off + b].astype(np.uint32) << (8 * b)
        return out.astype(self.dtype)

    def geometry(self):
        """The C ABI's argument run: frame stride, frames, width, height, row pitch, pixel stride, sample bytes."""
        return self.frame_stride, self.F, self.W, self.H, self.row_pitch, self.pixel_stride, self.sb

    def misreadings(self):
        """[(what, as_if)] for every way this layout differs from the dense one: what a kernel that ignores it would read."""
        out = []
        if self.row_pitch != self.dense_pitch:
            out.append(("dense pitch", dict(row_pitch=self.dense_pitch)))
        if self.frame_stride != self.H * self.row_pitch:
            out.append(("dense frame stride", dict(frame_stride=self.H * self.row_pitch)))
        if self.base:
            out.append(("base 0", dict(base=0)))
        return out


LAYOUT_NAMES = ["dense", "pitch", "stride", "base", "all"]


def make_layout(name, shape, dtype):
    """The sweep's five layouts: dense | row pitch = dense + one pixel + one sample | frame stride = rows + 3 samples | base one sample in |
    all three."""
    F, H, W, C = shape
    sb = np.dtype(dtype).itemsize
    pitched, strided, based = name in ("pitch", "all"), name in ("stride", "all"), name in ("base", "all")
    pitch = W * C * sb + (C * sb + sb if pitched else 0)
    return Layout(shape, dtype, base=sb if based else 0, row_pitch=pitch, frame_stride=H * pitch + (3 * sb if strided else 0), name=name)


# ------------------------------------------------------------------ A: every layout
A_W, A_H, A_F = 131, 19, 3                                         # tile columns 64, 64, 3; tile rows 8, 8, 3; row 18 is the upper half of a pair
A_CASES = [(dt, C, lay) for dt in (np.uint8, np.uint16) for C in (1, 3, 4) for lay in LAYOUT_NAMES]
A_IDS = ["%s_c%d_%s" % (np.dtype(dt).name, C, lay) for dt, C, lay in A_CASES]


def random_clip(seed, F, H, W, C, dtype):
    return np.random.default_rng(seed).integers(0, top_of(dtype) + 1, (F, H, W, C)).astype(dtype)


def a_clip(dtype, C):
    return random_clip(4100 + 10 * np.dtype(dtype).itemsize + C, A_F, A_H, A_W, C, dtype)


# ------------------------------------------------------------------ B: tile edges of the median
EDGE_WS = [1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129]
EDGE_HS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
EDGE_SEED = 1                                                      # test_frame_prep_cpu.py: the first seed under which every border rule matters


def edge_plane(W, H, dtype, seed=EDGE_SEED):
    """A steep ramp in both directions plus noise: the replicated border is not what a reflected or a zero border would show."""
    top = top_of(dtype)
    rng = np.random.default_rng([seed, W, H, np.dtype(dtype).itemsize])
    y, x = np.mgrid[0:H, 0:W]
    ramp = top * (0.05 + 0.45 * x / max(W - 1, 1) + 0.4 * y / max(H - 1, 1))
    return np.clip(np.rint(ramp + rng.normal(0, 0.02 * top, (H, W))), 0, top).astype(dtype)


# ------------------------------------------------------------------ C: orderings the network must get right
def windows_ones(plane01):
    """The number of ones in every replicated 5x5 window of a 0/1 plane."""
    padded = np.pad(np.asarray(plane01, dtype=np.int64), 2, mode="edge")
    return np.lib.stride_tricks.sliding_window_view(padded, (5, 5)).sum(axis=(-1, -2))


@functools.lru_cache(maxsize=None)
def _ordering_planes(dtype_name):
    dtype = np.dtype(dtype_name).type
    top = top_of(dtype)
    rng = np.random.default_rng(5200 + np.dtype(dtype).itemsize)
    shape = (A_H, A_W)

    def two_level(lo, hi, density):
        return np.where(rng.random(shape) < density, hi, lo).astype(dtype)

    def three_level(vals):
        return np.array(vals, dtype=dtype)[rng.integers(0, len(vals), shape)]

    def columns(pattern):
        return np.broadcast_to(np.array(pattern, dtype=dtype)[np.arange(A_W) % 3], shape).copy()

    out = [("zero_top_0.40_0.60", [two_level(0, top, 0.40), two_level(0, top, 0.60)]),
           ("zero_top_0.45_0.55", [two_level(0, top, 0.45), two_level(0, top, 0.55)]),
           ("zero_top_0.50_0.50", [two_level(0, top, 0.50), two_level(0, top, 0.50)]),
           ("v_v1_low_high", [two_level(0, 1, 0.5), two_level(top - 1, top, 0.5)]),
           ("v_v1_mid", [two_level(top // 2, top // 2 + 1, 0.5), two_level(top // 2 - 1, top // 2, 0.45)]),
           ("full_range", [rng.integers(0, top + 1, shape).astype(dtype), rng.integers(0, top + 1, shape).astype(dtype)]),
           ("constant", [np.full(shape, top // 3, dtype), np.full(shape, top, dtype)]),
           ("columns", [columns([top, 0, 0]), columns([0, top, top])])]
    if np.dtype(dtype).itemsize == 2:
        out += [("sign_bit_pair", [two_level(32767, 32768, 0.5), two_level(32767, 32768, 0.42)]),
                ("sign_bit_three", [three_level([0, 32768, 65535]), three_level([0, 32768, 65535])]),
                ("v_v1_byte_carry", [two_level(255, 256, 0.5), two_level(0x7FFF - 0x100, 0x7FFF - 0xFF, 0.5)])]
    return [(name, np.stack(planes)[..., None]) for name, planes in out]


def ordering_planes(dtype):
    """[(name, clip (2, 19, 131, 1))]: two frames to a call."""
    return _ordering_planes(np.dtype(dtype).name)


ORDERING_NAMES = {dt: [name for name, _ in _ordering_planes(dt)] for dt in ("uint8", "uint16")}


# ------------------------------------------------------------------ D: many frames
MANY_F, MANY_W, MANY_H = 300, 5, 3


def many_clips(dtype, C):
    """(300 frames of 5x3, frame f from seed 6300 + f; a second clip of 2 frames for the reused accumulator)."""
    first = np.concatenate([random_clip(6300 + f, 1, MANY_H, MANY_W, C, dtype) for f in range(MANY_F)])
    return first, random_clip(6700 + C, 2, MANY_H, MANY_W, C, dtype)


def many_layout(shape, dtype):
    """Frame stride padded by 3 samples, dense rows."""
    return make_layout("stride", shape, dtype)


# ------------------------------------------------------------------ F: gray extremes
def gray_colours(dtype):
    """(N, 3): the seven corner colours of tests/test_gpu_adaptive.py, the three single-channel maxima, and per channel the two values
    whose weighted product lies closest under and closest at-or-over a half (the rounding term 1 << 14 decides them)."""
    top = top_of(dtype)
    rows = [[0, 0, 0], [top, top, top], [top, 0, 0], [0, top, 0], [0, 0, top], [1, 2, 3], [top - 1, top, top - 2],
            [top, 0, 0], [0, top, 0], [0, 0, top]]
    v = np.arange(top + 1, dtype=np.int64)
    for ch, coef in enumerate((3735, 19235, 9798)):
        frac = (v * coef) % (1 << 15)
        under = int(v[np.argmax(np.where(frac < (1 << 14), frac, -1))])
        over = int(v[np.argmin(np.where(frac >= (1 << 14), frac, 1 << 16))])
        for val in (under, over):
            row = [0, 0, 0]
            row[ch] = val
            rows.append(row)
    return np.array(rows, dtype=dtype)


def gray_without_rounding(frame):
    f = np.asarray(frame).astype(np.uint64)
    return ((f[..., 0] * 3735 + f[..., 1] * 19235 + f[..., 2] * 9798) >> 15).astype(np.asarray(frame).dtype)


def gray_clips(dtype, C):
    """[(name, clip (1, H, W, C))]: the seven corner colours as a 7x1 and as a 1x7 frame, the nine further colours as 9x1 and 1x9; a fourth
    sample, where there is one, is noise."""
    col = gray_colours(dtype)
    if C == 4:
        extra = np.random.default_rng(77).integers(0, top_of(dtype) + 1, (len(col), 1)).astype(dtype)
        col = np.concatenate([col, extra], axis=1)
    out = []
    for part in (col[:7], col[7:]):
        n = len(part)
        out += [("%dx1" % n, part.reshape(1, 1, n, C).copy()), ("1x%d" % n, part.reshape(1, n, 1, C).copy())]
    return out


# ------------------------------------------------------------------ G: the adaptive rule
ADAPTIVE_RULE = (10.0, 3.0, 30.0)                                  # noise tolerance, min, max: the reference's defaults
# (W, H, dtype name) -> the per-frame (seed, sigma) of the clip; frame 0 only stands in front of the first pair.  Found by
# search_adaptive_frames() below: one frame whose band is undecided, the others decided, with at least two thresholds among them.
ADAPTIVE_CLIPS = {
    (131, 19, "uint8"): [(1, 0.5), (2, 1.1), (94, 1.4), (3, 1.7), (4, 0.8)],
    (131, 19, "uint16"): [(1, 0.5), (2, 1.1), (654, 0.7000000000000001), (3, 1.7), (4, 0.8)],
    (200, 72, "uint8"): [(1, 0.5), (2, 1.1), (438, 2.2), (3, 1.7), (4, 0.8)],
    (200, 72, "uint16"): [(1, 0.5), (2, 1.1), (249, 2.2), (3, 1.7), (4, 0.8)],
}


def adaptive_frame(seed, sigma, W, H, dtype):
    """A gentle ramp plus sensor noise of `sigma` levels."""
    top = top_of(dtype)
    rng = np.random.default_rng([seed, W, H, np.dtype(dtype).itemsize])
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.rint(top // 4 + 0.3 * x + 0.2 * y + rng.normal(0, sigma, (H, W))), 0, top).astype(dtype)


def adaptive_clip(W, H, dtype):
    """(F, H, W, 3): luma from ADAPTIVE_CLIPS, two further samples of noise."""
    frames = ADAPTIVE_CLIPS[(W, H, np.dtype(dtype).name)]
    luma = np.stack([adaptive_frame(seed, sigma, W, H, dtype) for seed, sigma in frames])
    rest = np.random.default_rng(W + H).integers(0, top_of(dtype) + 1, luma.shape + (2,)).astype(dtype)
    return np.concatenate([luma[..., None], rest], axis=-1)


def band_of(plane, rule=ADAPTIVE_RULE):
    from new_bloom_filter_repo_amd import engine as E
    s1, s2 = moments_of(residual(plane))
    return E.adaptive_threshold_band(plane.size, s1, s2, *rule)


@functools.lru_cache(maxsize=None)
def _adaptive_case(W, H, dtype_name):
    from new_bloom_filter_repo_amd import engine as E
    clip = adaptive_clip(W, H, np.dtype(dtype_name).type)
    want, bands = [], []
    for f in range(1, len(clip)):
        y = np.ascontiguousarray(clip[f, :, :, 0])
        want.append(E.threshold_floor(orc.adaptive_diff_threshold(y, *ADAPTIVE_RULE)))
        bands.append(band_of(y))
    return clip, want, bands, [f for f, (lo, hi) in enumerate(bands, start=1) if lo != hi]


def adaptive_case(W, H, dtype):
    """(clip, the oracle's floors of frames 1.., their (lo, hi) bands, the frames whose band is undecided)."""
    return _adaptive_case(W, H, np.dtype(dtype).name)


ADAPTIVE_SHAPES = [(131, 19), (200, 72)]
ADAPTIVE_CASES = [(W, H, dt) for W, H in ADAPTIVE_SHAPES for dt in (np.uint8, np.uint16)]
ADAPTIVE_IDS = ["%dx%d_%s" % (W, H, np.dtype(dt).name) for W, H, dt in ADAPTIVE_CASES]


def search_adaptive_frames(W, H, dtype, tries=20000):
    """How ADAPTIVE_CLIPS was found (python tests/frame_prep_ref.py prints it): walk seeds at sigmas 0.4 .. 2.4 until one frame's band is
    undecided, then put it between decided frames of three different sigmas."""
    found = None
    for seed in range(tries):
        sigma = 0.4 + 0.1 * (seed % 21)
        lo, hi = band_of(adaptive_frame(seed, sigma, W, H, dtype))
        if lo != hi:
            found = (seed, sigma)
            break
    assert found, "no undecided frame in %d tries" % tries
    decided = []
    for seed, sigma in ((1, 0.5), (2, 1.1), (3, 1.7), (4, 0.8)):
        while True:
            lo, hi = band_of(adaptive_frame(seed, sigma, W, H, dtype))
            if lo == hi:
                decided.append((seed, sigma))
                break
            seed += 100
    return [decided[0], decided[1], found, decided[2], decided[3]]


if __name__ == "__main__":
    for W, H, dt in ADAPTIVE_CASES:
        print("    (%d, %d, %r): %r," % (W, H, np.dtype(dt).name, search_adaptive_frames(W, H, dt)))
