"""numpy reference of the bounded-error temporal hold (rbf_temporal_hold_runs) -- a helper of the near-lossless tests, not a test."""
import numpy as np


def hold_ref(frames, run_starts, max_error):
    """The held sequence of `frames` ((F, H, W) or (F, H, W, C), uint8 / uint16; a list of frames is stacked): frame 0 and every frame
    named in run_starts start a run and are kept; inside a run a pixel keeps its held value while EVERY one of its samples is within
    max_error of it (int64 differences: no wrap), and takes the frame's value, whole, otherwise.  Returns a new array."""
    x = np.asarray(frames) if isinstance(frames, np.ndarray) else np.stack([np.asarray(f) for f in frames])
    starts = {int(t) for t in (run_starts or ())} | {0}
    y = x.copy()
    for t in range(1, len(x)):
        if t in starts:
            continue
        over = np.abs(x[t].astype(np.int64) - y[t - 1].astype(np.int64)) > int(max_error)
        upd = over.any(axis=-1, keepdims=True) if x.ndim == 4 else over
        y[t] = np.where(upd, x[t], y[t - 1])
    return y


def all_channel_masks(y, run_starts):
    """The exact all-channel masks of a block (bool (F-1, H*W): pair f marks the pixels in which frames f and f+1 differ in any sample);
    the pair in front of a run start is all zeros (it is not coded)."""
    y = np.asarray(y)
    ch = y[1:] != y[:-1]
    if y.ndim == 4:
        ch = ch.any(axis=-1)
    ch = ch.reshape(len(y) - 1, -1)
    for t in run_starts or ():
        if int(t) > 0:
            ch[int(t) - 1] = False
    return ch


def random_clip(seed, F, H, W, C, dtype, step=3):
    """A random walk per sample (steps of up to +-step, clipped) with a few large jumps: most samples stay near their held value."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    shape = (H, W) if C == 0 else (H, W, C)
    x = [rng.integers(0, top + 1, shape).astype(np.int64)]
    for _ in range(F - 1):
        nxt = x[-1] + rng.integers(-step, step + 1, shape)
        jump = rng.random(shape) < 0.02
        nxt[jump] = rng.integers(0, top + 1, int(jump.sum()))
        x.append(np.clip(nxt, 0, top))
    return np.stack(x).astype(dtype)
