"""The numpy reference of pan alignment (include/rbf.h, "pan alignment"): SAD table, pick, moving count, rule, offsets, roll, and the pan
table's bytes.  Written from the definitions, independent of the library and of container.py: it is the yardstick the CPU and the GPU
tests compare against, and is never compared with itself."""
import struct

import numpy as np

GRID = 8


def luma(frame):
    """Sample 0 of every pixel, as int64."""
    a = np.asarray(frame)
    return (a if a.ndim == 2 else a[..., 0]).astype(np.int64)


def grid_points(W, H, R):
    """(xs, ys) of the grid: x in {R, R+8, ...} < W-R, y in {R, R+8, ...} < H-R."""
    assert W > 2 * R and H > 2 * R
    return np.arange(R, W - R, GRID), np.arange(R, H - R, GRID)


def sad_table(prev, cur, R):
    """{(dx, dy): SAD} for |dx|, |dy| <= R, Python ints."""
    Yp, Yc = luma(prev), luma(cur)
    H, W = Yp.shape
    xs, ys = grid_points(W, H, R)
    ref = Yp[np.ix_(ys, xs)]
    return {(dx, dy): int(np.abs(Yc[np.ix_(ys + dy, xs + dx)] - ref).sum()) for dy in range(-R, R + 1) for dx in range(-R, R + 1)}


def sad_tables(frames, R):
    """The SAD tables of every pair of `frames` at once, int64 (pairs, 2R+1, 2R+1) indexed [pair, dy + R, dx + R]: for every grid point the
    window Yc[y-R:y+R+1, x-R:x+R+1] against Yp[y, x].  sad_table walks the candidates in Python, too slow for the thousands of pairs of
    a clip with every candidate of R = 32 planted; test_block_layout_cpu.py proves the two equal."""
    Y = np.stack([luma(f) for f in frames])
    H, W = Y.shape[1:]
    xs, ys = grid_points(W, H, R)
    out = np.zeros((len(Y) - 1, 2 * R + 1, 2 * R + 1), dtype=np.int64)
    Y = Y.astype(np.int16 if Y.max(initial=0) < 1 << 15 else np.int32)   # (the narrowest type the differences fit: this is memory-bound)
    for y in ys:
        for x in xs:
            out += np.abs(Y[1:, y - R:y + R + 1, x - R:x + R + 1] - Y[:-1, y, x][:, None, None])
    return out


def pick(table):
    """The candidate with the smallest (SAD, |dx|+|dy|, |dy|, dy, dx)."""
    return min(table, key=lambda v: (table[v], abs(v[0]) + abs(v[1]), abs(v[1]), v[1], v[0]))


def roll(frame, ox, oy):
    """new(x, y) = old((x + ox) mod W, (y + oy) mod H)."""
    return np.roll(np.asarray(frame), (-int(oy), -int(ox)), axis=(0, 1))


def moving(prev, cur, v, tolerance=0):
    """Pixels p with a sample where |cur((p + v) mod (W, H))[c] - prev(p)[c]| > tolerance."""
    a, b = np.asarray(prev).astype(np.int64), roll(cur, v[0], v[1]).astype(np.int64)
    d = np.abs(a - b) > tolerance
    return int((d if d.ndim == 2 else d.any(axis=2)).sum())


def stat_rows(frames, R, tolerance=0, run_starts=()):
    """What rbf_pan_search writes: a dict per pair with dx, dy, sad_zero, sad_best, moving_zero, moving_best; zeros in front of a run start."""
    rows = []
    for f in range(1, len(frames)):
        if f in set(run_starts):
            rows.append(dict(dx=0, dy=0, sad_zero=0, sad_best=0, moving_zero=0, moving_best=0))
            continue
        t = sad_table(frames[f - 1], frames[f], R)
        dx, dy = pick(t)
        rows.append(dict(dx=dx, dy=dy, sad_zero=t[(0, 0)], sad_best=t[(dx, dy)], moving_zero=moving(frames[f - 1], frames[f], (0, 0), tolerance),
                         moving_best=moving(frames[f - 1], frames[f], (dx, dy), tolerance)))
    return rows


def offsets(rows, run_starts, W, H):
    """(cumulative offsets per frame, [(j, dx, dy)] adopted): a pair adopts its best shift iff moving_best < moving_zero."""
    out, adopted = [(0, 0)], []
    for j, r in enumerate(rows, start=1):
        if j in set(run_starts):
            out.append((0, 0))
            continue
        ox, oy = out[-1]
        if r["moving_best"] < r["moving_zero"]:
            adopted.append((j, r["dx"], r["dy"]))
            ox, oy = (ox + r["dx"]) % W, (oy + r["dy"]) % H
        out.append((ox, oy))
    return out, adopted


def stabilise(frames, R, tolerance=0, run_starts=()):
    """(stabilised frames, offsets, adopted, rows)."""
    H, W = np.asarray(frames[0]).shape[:2]
    rows = stat_rows(frames, R, tolerance, run_starts)
    offs, adopted = offsets(rows, run_starts, W, H)
    return [roll(f, ox, oy) for f, (ox, oy) in zip(frames, offs)], offs, adopted, rows


def fd1(data):
    """FD1 (include/rbf.h) of a bytes object, in plain Python integers."""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, x: (rotl((acc + x * P2) & M, 31) * P1) & M
    merge = lambda a, b: (((a ^ rnd(0, b)) * P1) + P4) & M

    def aval(h):
        h ^= h >> 33
        h = (h * P2) & M
        h ^= h >> 29
        h = (h * P3) & M
        return h ^ (h >> 32)

    def block(b, seed):
        w = struct.unpack("<512Q", b + bytes(4096 - len(b)))
        acc = [(seed + P5 + l * P1) & M for l in range(64)]
        for r in range(4):
            for h in range(2):
                for l in range(64):
                    acc[l] = rnd(acc[l], w[128 * r + 2 * l + h])
        d = 1
        while d < 64:
            for l in range(0, 64, 2 * d):
                acc[l] = merge(acc[l], acc[l + d])
            d *= 2
        return aval(acc[0])
    b, L = bytes(data), len(data)
    while len(b) > 4096:
        b = b"".join(struct.pack("<Q", block(b[i:i + 4096], i // 4096)) for i in range(0, len(b), 4096))
    return block(b, L)


def build_table(entries):
    """The type-6 record's body for [(record index, ox, oy)], ascending."""
    body = struct.pack("<B3xI", 1, len(entries)) + b"".join(struct.pack("<III", i, ox, oy) for i, ox, oy in entries)
    return body + struct.pack("<Q", fd1(body))


def parse_table(body):
    """[(record index, ox, oy)] of a type-6 body whose checksum holds."""
    version, count = struct.unpack_from("<B3xI", body, 0)
    assert version == 1 and len(body) == 16 + 12 * count and struct.unpack_from("<Q", body, len(body) - 8)[0] == fd1(body[:-8])
    return [struct.unpack_from("<III", body, 8 + 12 * j) for j in range(count)]


# ---- the clips the tests share ----
def planted_clip(width=96, height=64, R=4, dtype=np.uint8, sensor_noise=0, seed=5, channels=3, nframes=12):
    """(frames, shifts): nframes frames of a panning camera whose pairs carry the planted shifts -- the four corners of the range, (0, 0), (1, 0),
    (0, -1) -- twice over the two GOPs of six frames; the pairs in front of frames 0 and 6 are not coded, their shifts are moot."""
    from new_bloom_filter_repo_amd.synthetic import make_panning_gop
    cycle = [(R, R), (-R, -R), (R, -R), (-R, R), (0, 0), (1, 0), (0, -1)]
    shifts = [cycle[i % len(cycle)] for i in range(nframes - 1)]
    frames, got = make_panning_gop(seed, width, height, nframes, [(-dx, -dy) for dx, dy in shifts], dtype=dtype, sensor_noise=sensor_noise,
                                   return_shifts=True)
    assert got == shifts
    if channels == 1:
        frames = [np.ascontiguousarray(f[..., 0]) for f in frames]
    elif channels == 2:
        frames = [np.ascontiguousarray(f[..., :2]) for f in frames]
    elif channels == 4:
        frames = [np.ascontiguousarray(np.concatenate([f, f[..., :1] ^ 0x55], axis=2)) for f in frames]
    return frames, shifts
