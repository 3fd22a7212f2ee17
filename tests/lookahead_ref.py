"""numpy reference of the look-ahead temporal hold (rbf_temporal_lookahead_runs) -- a helper of the look-ahead tests, not a test.
Written from the rule in include/rbf.h: greedy interval stabbing per pixel and run."""
import numpy as np


def lookahead_ref(frames, run_starts, max_error):
    """The held sequence of `frames` ((F, H, W) or (F, H, W, C), uint8 / uint16; a list of frames is stacked) and the segment-start bits.

    Frame 0 and every frame named in run_starts start a run and are kept.  Inside a run a pixel stays at the run's first value while
    every sample is within max_error of it (the anchored segment); the first frame that breaks this opens a free segment, which lasts
    while the windows [x - e, x + e] (clamped to the sample range) of its frames intersect in EVERY sample, and whose value is the
    previous segment's value clamped into that intersection; the frame that empties a sample's intersection opens the next segment.
    Returns (y, starts): y a new array like frames, starts a bool (F, H, W) array that is True where a pixel's segment opens (never at
    a run's first frame)."""
    x = np.asarray(frames) if isinstance(frames, np.ndarray) else np.stack([np.asarray(f) for f in frames])
    F, e, top = len(x), int(max_error), int(np.iinfo(x.dtype).max)
    xs = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    firsts = sorted({int(t) for t in (run_starts or ())} | {0})
    y = xs.copy()
    starts = np.zeros(xs.shape[:3], dtype=bool)
    for a, b in zip(firsts, firsts[1:] + [F]):
        lo, hi, prev = xs[a].copy(), xs[a].copy(), xs[a].copy()        # the anchored segment is the free one whose window is the point x_0
        first = np.full(xs.shape[1:3], a)                               # the frame each pixel's open segment began at

        def close(end, which):
            """Pixels `which` end their segment in front of frame `end`: its frames get clamp(prev, lo, hi)."""
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


def update_counts(y, run_starts):
    """How often every pixel changes inside its runs: int (H, W) -- the set bits of the exact all-channel masks, per pixel."""
    y = np.asarray(y)
    ch = y[1:] != y[:-1]
    if y.ndim == 4:
        ch = ch.any(axis=-1)
    for t in run_starts or ():
        if int(t) > 0:
            ch[int(t) - 1] = False
    return ch.sum(axis=0)
