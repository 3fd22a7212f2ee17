"""The cases of the surface geometry sweep, as data: the composed surface (ImprovedVideoCompressor -> GopCoder -> the C ABI -> container
-> decompress_video) at frame geometries where the block stages leave their lane tiles, mask rows end inside a byte, Rice streams end
inside a chunk and the pan rule's size condition flips -- with holds, look-aheads, pans, cuts, quality reports and keyframe quantisers in
front of them.  test_gpu_surface_geometries.py runs them against surface_twin.py; test_surface_geometries_cpu.py proves on the CPU that
the array covers every legal pair, that every geometry reaches what its row says, and that every case exercises what it turns on.
A test helper: not collected.

Read it top to bottom: GEOMETRIES (each with the reason it is there, and regime(): the rules of include/rbf.h as arithmetic), LAYOUTS,
DEPTHS, PROFILES (fixed keyword sets), legal(), CASES (surface_cases.covering_array over these axes, and EXTRA), SEEDS, REST and clip().

The generator gives 72 cases -- as many as there are pairs of the 12 geometries and the 6 profiles, the two longest axes -- and EXTRA
three more: 75 cases."""
import numpy as np

import surface_cases as sc

T, I, CUT, R = sc.T, sc.I, sc.CUT, sc.R
BLOCK = 2 * I

# (W, H): what the row reaches.  regime() and test_surface_geometries_cpu.py turn every sentence into arithmetic.
GEOMETRIES = {
    (1, 1): "one pixel: density 0 or 1 only, every stream a single sample per channel",
    (5, 3): "15 pixels: below one lane tile at every layout",
    (15, 1): "one row just below a tile; no pixel has one above",
    (16, 1): "one row of exactly one tile; no pixel has one above",
    (1, 15): "every pixel is column 0: the intra predictor is always 'above'",
    (9, 8): "H = 2R at R = 4: not panned",
    (9, 9): "W, H > 2R at R = 4: panned",
    (24, 5): "120 pixels = 7 tiles + 8: tiles and tail where frame bytes % 16 == 0 (u16 grey, u16 yuv/bgr, bgra), per-pixel only where not",
    (37, 9): "333 pixels: under one Rice chunk with 1 and 3 samples (333, 999), a ragged second chunk with 4 (1332)",
    (67, 33): "2211 pixels: frame bytes never a multiple of 16, ragged last mask word, ragged last chunk",
    (72, 29): "2088 pixels = 130 tiles + 8, 2088 % 64 = 40: tiles plus tail, several chunks per stream",
    (1030, 2): "a row longer than 1024 samples and than four 256-sample spans of the keyframe quantiser; too flat to pan",
}
LAYOUTS = {"grey": 1, "yuv": 3, "bgr": 3, "bgra": 4}          # samples per pixel.  bgra: (H, W, 4), handed in as BGR (surface_cases.make_clip)
DEPTHS = {"u8": 1, "u16": 2}                                   # bytes per sample

# profile: (constructor keywords, the near-lossless mode of surface_cases.NEAR whose clip recipe -- noise, lighting step -- it runs on)
PROFILES = {
    "exact_rice": (dict(mask_channels="all", sample_codec="rice", scene_cuts=True, frame_digests=True), "off"),
    "exact_luma_zlib": (dict(mask_channels="luma", sample_codec="zlib", frame_digests=True), "off"),
    "first_key7": (dict(mask_channels="all", sample_codec="rice", max_error=2, bounded_keyframes=True, scene_cuts=True, frame_digests=True,
                        quality_report=True), "first_d2"),
    "look_pan": (dict(mask_channels="all", sample_codec="zlib", max_error=1, hold_mode="lookahead", pan_range=R, scene_cuts=True,
                      frame_digests=True, quality_report=True), "look_d1"),
    "per_channel": (dict(mask_channels="all", sample_codec="rice", error_bounds="PER_CHANNEL", bounded_keyframes=True, scene_cuts=True),
                    "first_122"),
    "map_look": (dict(mask_channels="all", sample_codec="rice", error_bounds="MAP", hold_mode="lookahead", quality_report=True), "map"),
}
PER_CHANNEL = {3: (1, 2, 2), 4: (1, 2, 2, 3)}

AXES = [("geometry", list(GEOMETRIES)), ("layout", list(LAYOUTS)), ("depth", list(DEPTHS)), ("profile", list(PROFILES))]
NAMES = [n for n, _ in AXES]


def regime(W, H, C, sb, R=R):
    """What include/rbf.h says a dense block of W x H pixels of C samples of sb bytes goes through, as numbers.
      per_pixel_only  "Frames whose base and stride are multiples of 16 go through 16-byte accesses, any other sample-aligned layout
                      ... through a per-pixel kernel" (hold, cut statistic, quality report; the digest's <false> instance): the stride of
                      a dense block is the frame's bytes; and "frames of fewer than 16 pixels"
      tiles, tail     "... and the last (width*height) % 16 pixels of a frame through a per-pixel kernel"
      mask_pad_bits   the padding bits in the last byte of a frame's (n + 7) // 8 mask bytes; mask_word_bits: n % 64
      chunks, last    a keyframe's sample stream: "N = H W C, chunks of 1024"; `last` samples in the last one
      panned          "Frames are W x H, with W > 2R and H > 2R" """
    n = W * H
    fb = n * C * sb
    vector = fb % 16 == 0 and n >= 16
    N = n * C
    return dict(pixels=n, frame_bytes=fb, per_pixel_only=not vector, tiles=n // 16 if vector else 0, tail=n % 16 if vector else n,
                mask_pad_bits=-n % 8, mask_word_bits=n % 64, chunks=-(-N // 1024), last=N - 1024 * ((N - 1) // 1024),
                panned=W > 2 * R and H > 2 * R, has_above=H > 1, has_left=W > 1)


def legal(c):
    """None when the assignment can be run, else the reason it is not."""
    if c["layout"] == "bgra" and c["profile"] == "exact_luma_zlib":
        return "the twin's luma rule is not stated for four samples: bgra runs with mask_channels='all' only"
    if c["layout"] == "grey" and c["profile"] == "per_channel":
        return "per-channel bounds do not fit frames of one channel"
    return None


def bound_map(W, H):
    """2 everywhere, the left half -- at least one column -- 0."""
    e = np.full((H, W), 2, dtype=np.int64)
    e[:, :max(1, W // 2)] = 0
    return e


# Beyond the pairs: combinations of three values that reach code no pair of the array does.
#   72 x 29 yuv u16 look_pan   tiles plus tail at 16 bits under the search, the roll (rows of 432 bytes: its 16-byte vectors), the cut statistic
#                              and the look-ahead -- the array's look_pan cases at 67 x 33 and 72 x 29 are 8-bit grey
#   67 x 33 bgra u16 map_look  the only layout whose 67 x 33 frame is a multiple of 8 bytes: the look-ahead's 8-byte tiles with a tail of
#                              2211 % 8 = 3 pixels, under a bound map
#   1030 x 2 bgra u16 first_key7   the longest row the quantiser sees: 4120 samples of 16 bits
EXTRA = [dict(geometry=(72, 29), layout="yuv", depth="u16", profile="look_pan"),
         dict(geometry=(67, 33), layout="bgra", depth="u16", profile="map_look"),
         dict(geometry=(1030, 2), layout="bgra", depth="u16", profile="first_key7")]
CASES = sc.covering_array(AXES, legal) + [dict(c) for c in EXTRA]
for _k, _c in enumerate(CASES):
    _c["gpu_lanes"] = 1 + _k % 3


def case_id(k, c):
    return "%02d-%dx%d-%s-%s-%s-l%d" % ((k,) + c["geometry"] + (c["layout"], c["depth"], c["profile"], c["gpu_lanes"]))


IDS = [case_id(k, c) for k, c in enumerate(CASES)]


def keywords(c):
    """The constructor keywords of a case."""
    W, H = c["geometry"]
    kw = dict(PROFILES[c["profile"]][0], keyframe_interval=I, block_frames=BLOCK, gpu_lanes=c["gpu_lanes"])
    if kw.get("error_bounds") == "PER_CHANNEL":
        kw["error_bounds"] = PER_CHANNEL[LAYOUTS[c["layout"]]]
    elif kw.get("error_bounds") == "MAP":
        kw["error_bounds"] = bound_map(W, H)
    if c["layout"] != "yuv":
        kw["inter_frames"] = True
    return kw


def as_surface_case(c):
    """The case in surface_cases' terms, for the helpers that read a case's layout, dtype, near mode and switches."""
    kw = PROFILES[c["profile"]][0]
    return dict(dtype=c["depth"], layout=c["layout"], mask_channels=kw["mask_channels"], sample_codec=kw["sample_codec"],
                near=PROFILES[c["profile"]][1], scene_cuts=bool(kw.get("scene_cuts")), pan_range=kw.get("pan_range", 0),
                bounded_keyframes=bool(kw.get("bounded_keyframes")), frame_digests=bool(kw.get("frame_digests")),
                quality_report=bool(kw.get("quality_report")), gpu_lanes=c["gpu_lanes"], block_frames=BLOCK, route="whole")


def color_space(c):
    return "YUV" if c["layout"] == "yuv" else "BGR"


def frame_shape(c):
    W, H = c["geometry"]
    return (H, W) if c["layout"] == "grey" else (H, W, LAYOUTS[c["layout"]])


def frame_dtype(c):
    return np.uint8 if c["depth"] == "u8" else np.uint16


# ---- the clips -------------------------------------------------------------------------------------------------------------------------
# surface_cases.SEEDS unless a row says otherwise: {(geometry, clip_name()): (seed, seed)}, chosen so that the conditions of
# test_surface_geometries_cpu.py hold on the twin's output (conditions on the twin, not measurements of the product)
SEEDS = {}
# The camera of the panning clip moves by (2, 1) a frame.  Over a frame the pan rule does not take (W <= 2R or H <= 2R) nothing can follow
# it: the canvas's texture scales with the frame, one row of a frame of 1, 2 or 5 rows is 6 to 20 levels, and EVERY pair is a cut -- none of
# 1500 seeds left 24 x 5 an inter-frame, none of 400 did for 1030 x 2.  So on those rows the camera rests for the pairs REST (two in each
# scene, none at a rule keyframe or the splice); it moves in all the others, where the twin must adopt no shift.
REST = (2, 3, 14, 15)
_clips, _twins = {}, {}


def velocities(W, H):
    v = np.tile(np.array([2, 1]), (T - 1, 1))
    if not (W > 2 * R and H > 2 * R):
        v[[t - 1 for t in REST]] = 0
    return v


def clip_key(c):
    return c["geometry"], sc.clip_name(as_surface_case(c))


def clip(c):
    """The T frames of a case (read-only arrays): the recipes of surface_cases.clip at the row's W x H."""
    key = clip_key(c)
    if key not in _clips:
        (W, H), name = key
        _clips[key] = sc.make_clip(name, W, H, SEEDS.get(key, sc.SEEDS[name[0]]), velocities(W, H))
    return _clips[key]


def twin_of(k, mutant=None):
    import surface_twin
    if (k, mutant) not in _twins:
        _twins[(k, mutant)] = surface_twin.twin(clip(CASES[k]), keywords(CASES[k]), None, mutant)
    return _twins[(k, mutant)]
