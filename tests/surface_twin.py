"""The composed numpy reference of the video surface: what ImprovedVideoCompressor(**keywords) writes for a clip and what a decoder
rebuilds from it, predicted from the per-stage twins (pan_ref, scene_cut_ref, near_key_ref, near_lossless_ref, lookahead_ref,
error_bounds_ref) in the order DESIGN.md and include/rbf.h document.  A test helper: not collected, not part of the package, and nothing
of the package is imported -- the plan, the tolerance rule, the pan rule, the cut rule, the re-base, the fallback rule and the record type
numbers are RESTATED here, so that a change of the product's composition shows as a difference and not as an agreement with itself.

  twin(frames, keywords, shards=None) -> dict
      kinds        the record types in container order: 1 / 3 / 7 keyframes, 2 / 4 inter-frames, then 6 (pan table) and 5 (digest trailer)
      scene_cuts   the cut frames, ascending
      pans         [(t, dx, dy)] of the pairs that adopted a shift
      pan_offsets  {record index: (ox, oy)} of the inter-frames whose stabilised frame is not the frame itself
      decoded      the frames a decoder rebuilds
      coded        the frames the records code (stabilised and held): the digests describe THESE
      digests      FD1 per frame (None without frame_digests)
      quality      error_bounds_ref.ROW per frame (None without quality_report): originals against decoded

`mutant` names one deliberate mistake in the composition (MUTANTS); test_surface_cases_cpu.py proves that each of them changes the
output of a case the GPU file runs -- which is how the sweep is known to fail when the product makes that mistake.  The last two
are told apart by the cases of surface_geometries.py (test_surface_geometries_cpu.py): pan_rule_not_strict takes a frame of H = 2R into
the search, which the C ABI refuses (Refused: the product would raise where the twin codes the clip unpanned), and offsets_mod_swapped
shows only where W != H."""
import numpy as np

import error_bounds_ref as eb
import near_key_ref as nk
import pan_ref
import scene_cut_ref

KEY, INTER, KEY_RICE, INTER_RICE, DIGESTS, PANS, KEY_NEAR = 1, 2, 3, 4, 5, 6, 7

DEFAULTS = dict(keyframe_interval=30, block_frames=None, mask_channels="luma", sample_codec="zlib", max_error=0, hold_mode="first",
                error_bounds=None, scene_cuts=False, pan_range=0, bounded_keyframes=False, frame_digests=False, quality_report=False)
IGNORED = ("gpu_lanes", "inter_frames", "gop_batching", "verify_digests")      # keywords that change no byte of what the twin predicts

MUTANTS = ("hold_before_quantiser", "cuts_before_alignment", "lookahead_tolerance_not_doubled", "tolerance_from_max_bound", "no_rebase",
           "rebase_one_frame_short", "halo_not_quantised", "digest_of_rolled_back_frame", "pan_rule_not_strict", "offsets_mod_swapped")
GEOMETRY_MUTANTS = MUTANTS[-2:]                  # mistakes that no 96 x 64 frame shows: proven on the cases of surface_geometries.py


class Refused(Exception):
    """What a composition ends in when it hands a stage what include/rbf.h says the stage refuses (RBF_EINVAL): no output at all."""


def options(keywords):
    o = dict(DEFAULTS)
    for k, v in keywords.items():
        if k in IGNORED:
            continue
        if k not in o:
            raise KeyError(k)
        o[k] = v
    I = max(1, int(o["keyframe_interval"]))
    o["keyframe_interval"] = I
    o["block_frames"] = max(2, int(o["block_frames"])) if o["block_frames"] else min(128, max(2, 2 * I if 2 * I <= 128 else I))
    return o


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def is_keyframe(t, first_index, I):
    """Global frame t is a keyframe iff t % I == 0, or it is the first frame handed in."""
    return t % I == 0 or t == first_index


def plan(first_index, start, stop, I, block_frames):
    """[(lo, end, run starts)]: a block reads frames lo .. end-1, lo = t - 1 for the first inter-frame t not yet coded, end = min(stop,
    t - 1 + block_frames); its run starts are the keyframes inside it, as indices into the block."""
    blocks, t = [], start
    while t < stop:
        if is_keyframe(t, first_index, I):
            t += 1
            continue
        end = min(stop, t - 1 + block_frames)
        blocks.append((t - 1, end, [u - (t - 1) for u in range(t, end) if is_keyframe(u, first_index, I)]))
        t = end
    return blocks


def halo_start(start, I):
    """The first frame a shard that codes [start, ...) reads."""
    return start if start % I == 0 else start - 1


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def bound_of(o, shape, dtype):
    """(d, E, hold_mode): the scalar bound and None, or None and the bound frame (the frames' shape); (0, None, "first") for a lossless
    call.  A bound frame whose entries all equal d IS max_error=d."""
    if o["error_bounds"] is None:
        return int(o["max_error"]), None, o["hold_mode"]
    e = np.asarray(o["error_bounds"]).astype(np.int64)
    E = np.empty(shape, dtype=np.int64)
    if e.ndim == 1:
        assert e.shape[0] == (shape[2] if len(shape) == 3 else 1), "per-channel bounds that do not fit the frames"
        E[...] = e if len(shape) == 3 else e[0]
    elif e.ndim == 2 and len(shape) == 3:
        E[...] = e[:, :, None]
    else:
        E[...] = e
    assert int(E.max()) <= np.iinfo(dtype).max
    if (E == E.reshape(-1)[0]).all():
        d = int(E.reshape(-1)[0])
        return d, None, o["hold_mode"] if d else "first"
    return None, E, o["hold_mode"]


def tolerance(d, E, hold_mode, dtype, mutant=None):
    """What the block is looked at with before any hold rewrites it: the bound, or the smallest entry of the bound frame; doubled for
    the look-ahead hold; clamped to the sample range."""
    base = d if E is None else int(E.max() if mutant == "tolerance_from_max_bound" else E.min())
    tol = base if hold_mode == "first" or mutant == "lookahead_tolerance_not_doubled" else 2 * base
    return min(tol, int(np.iinfo(dtype).max))


# ---- one block -----------------------------------------------------------------------------------------------------------------------
def luma_mask(a, b):
    """The luma residual mask at threshold 0 ("np.abs(int16 - int16) wraps"): sample 0 differs -- at 16 bits in its low 15
    bits, a change of exactly 0x8000 is not marked."""
    ya, yb = (a if a.ndim == 2 else a[..., 0]).astype(np.int64), (b if b.ndim == 2 else b[..., 0]).astype(np.int64)
    return ((ya ^ yb) & 0x7FFF) != 0 if a.dtype.itemsize == 2 else ya != yb


def block(seg, run_starts, o, mutant=None):
    """The stages of one block of consecutive frames seg (seg[0] is only read) with the rule's run starts.  Returns a dict: `coded` (the
    frames as the records code them), `offsets` ((ox, oy) per frame), `adopted`, `cuts`, `starts` (all run starts) and `falls` (frames
    j >= 1 that are no run start and are still not coded as inter-frames)."""
    x = [np.asarray(f) for f in seg]
    F, (H, W), dtype = len(x), x[0].shape[:2], x[0].dtype
    C = 1 if x[0].ndim == 2 else x[0].shape[2]
    d, E, hold_mode = bound_of(o, x[0].shape, dtype)
    near = bool(o["max_error"]) or o["error_bounds"] is not None
    tol = tolerance(d, E, hold_mode, dtype, mutant)
    starts, R = sorted(int(t) for t in run_starts), int(o["pan_range"])
    # 2. pan
    S, offs, adopted = [f.copy() for f in x], [(0, 0)] * F, []
    panned = bool(R) and (W >= 2 * R and H >= 2 * R if mutant == "pan_rule_not_strict" else W > 2 * R and H > 2 * R)
    if panned and not (W > 2 * R and H > 2 * R):
        raise Refused("rbf_pan_search: width or height <= 2*range")      # (pan_rule_not_strict: where the search has no grid point)
    if panned:
        S, offs, adopted, _ = pan_ref.stabilise(x, R, tol, starts)
        offs = [(int(ox), int(oy)) for ox, oy in offs]
    # 3. cuts, and the re-base of a cut that carries an offset
    cuts = []
    if o["scene_cuts"]:
        looked_at = x if mutant == "cuts_before_alignment" else S
        stats = scene_cut_ref.cut_stats(np.stack(looked_at), tol)
        cuts = [j for j in range(1, F) if int(stats[j - 1][1]) + int(stats[j - 1][0]) > int(stats[j - 1][2]) and j not in starts]
        if cuts:
            starts = sorted(set(starts) | set(cuts))
            if panned and mutant != "no_rebase":
                old = list(offs)
                for j in cuts:
                    cx, cy = old[j]
                    end = min([t for t in starts if t > j] + [F])
                    if mutant == "rebase_one_frame_short":
                        end = max(j + 1, end - 1)
                    for f in range(j, end):
                        S[f] = pan_ref.roll(S[f], -cx, -cy)
                        mx, my = (H, W) if mutant == "offsets_mod_swapped" else (W, H)
                        offs[f] = ((old[f][0] - cx) % mx, (old[f][1] - cy) % my)
            adopted = [row for row in adopted if row[0] not in cuts]
    # 4. bounded keyframes, 5. the hold
    S = np.stack(S)

    def quantise(S, firsts):
        if o["bounded_keyframes"]:
            per_channel = [d] * C if E is None else [int(v) for v in E.reshape(-1, C)[0]]
            for j in firsts:
                S[j] = nk.quantise(S[j], per_channel)[0]
        return S

    def hold(S):
        if not near or (E is None and d == 0):
            return S
        if E is None:
            return eb.hold_ref(S, starts, d) if hold_mode == "first" else eb.lookahead_ref(S, starts, d)[0]
        return eb.hold_map_ref(S, starts, E) if hold_mode == "first" else eb.lookahead_map_ref(S, starts, E)[0]

    if mutant == "hold_before_quantiser":
        S = quantise(hold(S), [0] + starts)
    elif mutant == "halo_not_quantised":
        S = quantise(hold(quantise(S, starts)), [0])
    else:
        S = hold(quantise(S, [0] + starts))
    # 6. fallback: a mask that is the luma mask cannot say every change
    falls, broken = [], False
    luma_only = o["mask_channels"] != "all" or C < 2
    for j in range(1, F):
        if j in starts:
            broken = False
            continue
        changed = S[j] != S[j - 1]
        changed = changed if changed.ndim == 2 else changed.any(axis=2)
        uncovered = luma_only and bool((changed & ~luma_mask(S[j - 1], S[j])).any())
        if uncovered or broken:
            falls.append(j)
            run = [t for t in range(F) if max([0] + [s for s in starts if s <= j]) <= t < min([s for s in starts if s > j] + [F])]
            broken = near or any(offs[t] != (0, 0) for t in run)      # the rest of the run continues frames a decoder will not have
    return dict(coded=S, offsets=offs, adopted=[tuple(int(v) for v in row) for row in adopted], cuts=cuts, starts=starts, falls=falls)


# ---- a range, a clip -----------------------------------------------------------------------------------------------------------------
def encode_range(frames, first_index, start, stop, o, mutant=None):
    """What one call codes of the global frames [start, stop); frames[i] is global frame first_index + i.  Per frame u: kinds[u],
    coded[u], offsets[u]; and the call's cuts and pans."""
    I, rice = o["keyframe_interval"], o["sample_codec"] == "rice"
    exact_key, inter = (KEY_RICE if rice else KEY), (INTER_RICE if rice else INTER)
    at = lambda u: np.asarray(frames[u - first_index])
    kinds, coded, offsets, cuts, pans = {}, {}, {}, [], []
    for u in range(start, stop):
        if is_keyframe(u, first_index, I):       # until a block says otherwise: an exact keyframe, coded from the caller's array
            kinds[u], coded[u], offsets[u] = exact_key, at(u), (0, 0)
    for lo, end, starts in plan(first_index, start, stop, I, o["block_frames"]):
        b = block([at(u) for u in range(lo, end)], starts, o, mutant)
        for j in range(end - lo):
            u = lo + j
            if not start <= u < stop:
                continue
            if j == 0 or j in b["starts"]:
                if o["bounded_keyframes"] and kinds.get(u) != KEY_NEAR:
                    kinds[u], coded[u], offsets[u] = KEY_NEAR, b["coded"][j], (0, 0)
                elif j:
                    kinds[u], coded[u], offsets[u] = exact_key, b["coded"][j], (0, 0)      # (a run first has offset 0: the caller's frame)
                if j in b["cuts"]:
                    cuts.append(u)
            elif j in b["falls"]:
                kinds[u], coded[u], offsets[u] = exact_key, at(u), (0, 0)
            else:
                kinds[u], coded[u], offsets[u] = inter, b["coded"][j], b["offsets"][j]
        pans += [(lo + j, dx, dy) for j, dx, dy in b["adopted"] if start <= lo + j < stop]
    return kinds, coded, offsets, sorted(cuts), sorted(pans)


def twin(frames, keywords, shards=None, mutant=None):
    """The whole surface for one clip: compress_video (shards=None) or encode_range over [(start, stop)] shards, each from its halo frame
    on, put together the way compress_video puts a container together; then the decode."""
    o = options(keywords)
    frames = [np.asarray(f) for f in frames]
    T, I = len(frames), o["keyframe_interval"]
    kinds, coded, offsets, cuts, pans = {}, {}, {}, [], []
    for start, stop in (shards or [(0, T)]):
        first = halo_start(start, I)
        k, c, f, sc, p = encode_range(frames[first:], first, start, stop, o, mutant)
        kinds.update(k), coded.update(c), offsets.update(f)
        cuts += sc
        pans += p
    assert sorted(kinds) == list(range(T))
    pan_offsets = {u: offsets[u] for u in range(T) if offsets[u] != (0, 0)}
    decoded = [pan_ref.roll(coded[u], -offsets[u][0], -offsets[u][1]) if offsets[u] != (0, 0) else np.asarray(coded[u]) for u in range(T)]
    out = dict(kinds=[kinds[u] for u in range(T)] + ([PANS] if pan_offsets else []) + ([DIGESTS] if o["frame_digests"] else []),
               scene_cuts=sorted(cuts), pans=sorted(pans), pan_offsets=pan_offsets, decoded=decoded, coded=[np.asarray(coded[u]) for u in range(T)],
               digests=None, quality=None)
    if o["frame_digests"]:
        described = decoded if mutant == "digest_of_rolled_back_frame" else out["coded"]
        out["digests"] = [pan_ref.fd1(np.ascontiguousarray(f).tobytes()) for f in described]
    if o["quality_report"]:
        d, E, _ = bound_of(o, frames[0].shape, frames[0].dtype)
        out["quality"] = eb.error_stats_ref(np.stack(frames), np.stack(decoded), d if E is None else E)
    return out


def bound_frame(keywords, shape, dtype):
    """The bound every decoded sample is within, as an array of the frames' shape (zeros for a lossless call)."""
    d, E, _ = bound_of(options(keywords), shape, dtype)
    return np.full(shape, d, dtype=np.int64) if E is None else E
