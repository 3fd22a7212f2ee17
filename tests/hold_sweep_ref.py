"""numpy reference of the hold sweep (rbf_hold_sweep) -- a helper of the hold-sweep tests, not a test.  Built on the holds' own references:
for each candidate hold the clip, then take the rows of the quality report and the mask counts per run."""
import numpy as np

from error_bounds_ref import error_stats_ref
from lookahead_ref import lookahead_ref
from near_lossless_ref import all_channel_masks, hold_ref

ROW = np.dtype([("sse", "<u8"), ("updates", "<u8"), ("max_abs", "<u4"), ("reserved", "<u4")])     # rbf_sweep_row


def run_list(nframes, run_starts):
    """[(first frame, end)] of the runs of a block, a run of one frame included."""
    firsts = sorted({int(t) for t in (run_starts or ())} | {0})
    return list(zip(firsts, firsts[1:] + [nframes]))


def sweep_ref(frames, run_starts, candidates, lookahead):
    """The rows of rbf_hold_sweep: a (runs, candidates) array of ROW.  Row [r, i]: over run r's frames, sse and max_abs of the clip
    against its held sequence under max_error = candidates[i] (hold_ref, or lookahead_ref), and the set bits of the held sequence's
    all-channel masks."""
    x = np.asarray(frames)
    runs = run_list(len(x), run_starts)
    rows = np.zeros((len(runs), len(candidates)), dtype=ROW)
    for i, d in enumerate(candidates):
        y = lookahead_ref(x, run_starts, d)[0] if lookahead else hold_ref(x, run_starts, d)
        err = error_stats_ref(x, y)
        ones = all_channel_masks(y, run_starts).sum(axis=1) if len(x) > 1 else np.zeros(0, dtype=np.int64)
        for r, (a, b) in enumerate(runs):
            rows[r, i] = (int(err["sse"][a:b].sum()), int(ones[a:b - 1].sum()), int(err["max_abs"][a:b].max()), 0)
    return rows


def sweep_closed_form(frames, run_starts, candidates):
    """The look-ahead rows the way the kernel forms them: one forward walk per pixel that never sees a segment's value before the
    segment closes -- per segment its length n and, per sample, the moments S1, S2, the min and the max of d = x - (the segment's
    first sample); on close, with w = value - first sample: sse += S2 - 2 w S1 + n w^2, max_abs = max(dmax - w, w - dmin)."""
    x = np.asarray(frames)
    xs = (x if x.ndim == 4 else x[..., None]).astype(np.int64)
    top = int(np.iinfo(x.dtype).max)
    runs = run_list(len(x), run_starts)
    rows = np.zeros((len(runs), len(candidates)), dtype=ROW)
    for i, e in enumerate(candidates):
        for r, (a, b) in enumerate(runs):
            lo, hi, prev, ref = xs[a].copy(), xs[a].copy(), xs[a].copy(), xs[a].copy()
            s1, s2, dmin, dmax = (np.zeros_like(ref) for _ in range(4))
            n = np.ones(ref.shape[:2], dtype=np.int64)
            sse = updates = worst = 0
            for t in list(range(a + 1, b)) + [None]:
                if t is None:                                   # the run's end closes every segment
                    if b - a < 2:
                        break
                    brk = np.ones(ref.shape[:2], dtype=bool)
                else:
                    xl, xh = np.maximum(xs[t] - e, 0), np.minimum(xs[t] + e, top)
                    nlo, nhi = np.maximum(lo, xl), np.minimum(hi, xh)
                    brk = (nlo > nhi).any(axis=-1)
                    updates += int(brk.sum())
                v = np.clip(prev, lo, hi)
                w = v - ref
                seg = s2 - 2 * w * s1 + n[..., None] * w * w
                assert (np.abs(s1) < 2 ** 31).all() and (s2 < 2 ** 32).all() and (seg >= 0).all(), "the kernel's 32-bit moments"
                sse += int(seg[brk].sum())
                if brk.any():
                    worst = max(worst, int(np.maximum(dmax - w, w - dmin)[brk].max()))
                if t is None:
                    break
                m = brk[..., None]
                prev = np.where(m, v, prev)
                ref = np.where(m, xs[t], ref)
                d = xs[t] - ref
                lo, hi = np.where(m, xl, nlo), np.where(m, xh, nhi)
                s1, s2 = np.where(m, 0, s1 + d), np.where(m, 0, s2 + d * d)
                dmin, dmax = np.where(m, 0, np.minimum(dmin, d)), np.where(m, 0, np.maximum(dmax, d))
                n = np.where(brk, 1, n + 1)
            rows[r, i] = (sse, updates, worst, 0)
    return rows
