"""numpy references of the near-lossless stage with a bound per sample (rbf_temporal_hold_runs_map, rbf_temporal_lookahead_runs_map) and
of the quality report (rbf_error_stats) -- helpers of the error-bounds tests, not tests.  hold_map_ref and lookahead_map_ref are
near_lossless_ref.hold_ref and lookahead_ref.lookahead_ref with int(max_error) replaced by the bound frame E."""
import numpy as np

from near_lossless_ref import all_channel_masks, hold_ref, random_clip      # noqa: F401  (the tests take them from here)
from lookahead_ref import lookahead_ref, update_counts                      # noqa: F401

ROW = np.dtype([("sse", "<u8"), ("differing", "<u8"), ("over_bound", "<u8"), ("max_abs", "<u4"), ("reserved", "<u4")])


def _stack(frames):
    return np.asarray(frames) if isinstance(frames, np.ndarray) else np.stack([np.asarray(f) for f in frames])


def hold_map_ref(frames, run_starts, bounds):
    """hold_ref with a bound per sample: `bounds` has a frame's shape; a pixel keeps its held value while EVERY one of its samples is within
    ITS bound of it, and takes the frame's value, whole, otherwise."""
    x = _stack(frames)
    E = np.asarray(bounds).astype(np.int64)
    assert E.shape == x.shape[1:], (E.shape, x.shape)
    starts = {int(t) for t in (run_starts or ())} | {0}
    y = x.copy()
    for t in range(1, len(x)):
        if t in starts:
            continue
        over = np.abs(x[t].astype(np.int64) - y[t - 1].astype(np.int64)) > E
        upd = over.any(axis=-1, keepdims=True) if x.ndim == 4 else over
        y[t] = np.where(upd, x[t], y[t - 1])
    return y


def lookahead_map_ref(frames, run_starts, bounds):
    """lookahead_ref with a bound per sample: the windows are [x - E, x + E] clamped to the sample range.  Returns (y, starts)."""
    x = _stack(frames)
    E = np.asarray(bounds).astype(np.int64)
    assert E.shape == x.shape[1:], (E.shape, x.shape)
    F, top = len(x), int(np.iinfo(x.dtype).max)
    xs = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    e = E if x.ndim == 4 else E[..., None]
    firsts = sorted({int(t) for t in (run_starts or ())} | {0})
    y = xs.copy()
    starts = np.zeros(xs.shape[:3], dtype=bool)
    for a, b in zip(firsts, firsts[1:] + [F]):
        lo, hi, prev = xs[a].copy(), xs[a].copy(), xs[a].copy()
        first = np.full(xs.shape[1:3], a)

        def close(end, which):
            v = np.clip(prev, lo, hi)
            for t in range(a, end):
                sel = which & (first <= t)
                y[t][sel] = v[sel]
            prev[which] = v[which]

        for t in range(a + 1, b):
            xl, xh = np.maximum(xs[t] - e, 0), np.minimum(xs[t] + e, top)
            nlo, nhi = np.maximum(lo, xl), np.minimum(hi, xh)
            brk = (nlo > nhi).any(axis=-1)
            close(t, brk)
            starts[t] = brk
            first[brk] = t
            lo = np.where(brk[..., None], xl, nlo)
            hi = np.where(brk[..., None], xh, nhi)
        close(b, np.ones_like(first, dtype=bool))
    y = y.astype(x.dtype)
    return (y if x.ndim == 4 else y[..., 0]), starts


def error_stats_ref(a, b, bounds=0):
    """The rows of rbf_error_stats for the blocks a (originals) and b (coded): per frame sse, differing, over_bound, max_abs in exact
    integers.  bounds: an integer, or a bound frame of a frame's shape."""
    a, b = _stack(a), _stack(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    E = np.asarray(bounds).astype(np.int64)
    rows = np.zeros(len(a), dtype=ROW)
    for f in range(len(a)):
        d = np.abs(a[f].astype(np.int64) - b[f].astype(np.int64))
        rows[f] = (int((d * d).sum()), int(np.count_nonzero(d)), int(np.count_nonzero(d > E)),      # (int64: d^2 < 2^32, a frame < 2^31 samples)
                   int(d.max()) if d.size else 0, 0)
    return rows


def test_bounds(shape, dtype, seed=0):
    """The bound frame of the sweeps: random bounds 0..5, a rectangle of zeros (returned as index slices), a stripe of M (the last two
    columns) and, at 16 bits, a few entries of 300."""
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    E = rng.integers(0, 6, shape).astype(dtype)
    H, W = shape[:2]
    if np.dtype(dtype).itemsize == 2:
        E.reshape(-1)[::11] = 300
    E[:, W - 2:] = top
    rect = (slice(H // 4, H // 4 + max(1, H // 2)), slice(W // 4, W // 4 + max(2, W // 3)))
    E[rect] = 0
    return E, rect


test_bounds.__test__ = False
