"""numpy reference of the scene-cut statistic (rbf_cut_stats, include/rbf.h) and of the rule that reads it -- a helper of the scene-cut
tests, not a test."""
import numpy as np

from new_bloom_filter_repo_amd.synthetic import make_camera_gop


def rice_map(d, bits):
    """The sample codec's mapping of a residual mod 2^bits (sample_codec_ref.to_u)."""
    full = 1 << bits
    d = np.asarray(d, dtype=np.int64) & (full - 1)
    return np.where(d < full // 2, 2 * d, 2 * (full - d) - 1)


def glen(u):
    """2 floor(log2(u + 1)) + 1: the Elias-gamma length of u + 1, exact in integers."""
    v = np.asarray(u, dtype=np.int64) + 1
    log2 = np.zeros(v.shape, dtype=np.int64)
    for s in (16, 8, 4, 2, 1):
        big = (v >> s) > 0
        log2 += np.where(big, s, 0)
        v = np.where(big, v >> s, v)
    return 2 * log2 + 1


def cut_stats(frames, tolerance):
    """(F - 1, 3) uint64: moving, inter_bits, intra_bits of every pair of a block of (F, H, W[, C]) uint8 / uint16 frames."""
    x = np.asarray(frames)
    bits = 8 * x.dtype.itemsize
    if x.ndim == 3:
        x = x[..., None]
    x = x.astype(np.int64)
    out = np.zeros((len(x) - 1, 3), dtype=np.uint64)
    for t in range(1, len(x)):
        moving = (np.abs(x[t] - x[t - 1]) > tolerance).any(axis=-1)
        inter = glen(rice_map(x[t] - x[t - 1], bits)).sum(axis=-1)
        pred = np.zeros_like(x[t])
        pred[:, 1:] = x[t][:, :-1]
        pred[1:, 0] = x[t][:-1, 0]
        intra = glen(rice_map(x[t] - pred, bits))
        out[t - 1] = (int(moving.sum()), int(inter[moving].sum()), int(intra.sum()))
    return out


def cut_frames(stats, run_starts=()):
    """The block indices j >= 1 with inter_bits + moving > intra_bits that are not run starts already."""
    known = {int(t) for t in run_starts}
    return [j + 1 for j, (moving, inter, intra) in enumerate(np.asarray(stats).tolist())
            if int(inter) + int(moving) > int(intra) and j + 1 not in known]


def ratio(row):
    moving, inter, intra = (int(v) for v in row)
    return (inter + moving) / intra


def two_scenes(width=320, height=180, per_scene=6, dtype=np.uint8, sensor_noise=0, seeds=(1, 2)):
    """make_camera_gop(seed, ...) x per_scene of every seed, spliced: one (len(seeds) * per_scene, H, W, 3) array."""
    return np.concatenate([np.stack(make_camera_gop(s, width, height, per_scene, dtype=dtype, sensor_noise=sensor_noise)) for s in seeds])
