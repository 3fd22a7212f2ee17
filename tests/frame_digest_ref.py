"""What the frame-digest tests share: the issue's test pattern and its known answers (from an independent numpy implementation)."""
import numpy as np

KNOWN = {
    0: 0x19044D0607DE195D,
    1: 0x71B883805DCCAF1B,
    4095: 0x43EEB4182D75AFC0,
    4096: 0xA6F7626AE65AAC8B,
    4097: 0x05EF9C7F725155E0,
    6633: 0x1BC7D4C4D0FCFC5A,
    13266: 0x78A90132D34CA223,
    172800: 0x7284D3815C1E4A8C,
    2097152: 0x4EA5EBC3DB0EEB85,               # the largest length with one level under the final block
    2098176: 0x9B86659075CE0444,               # 1024 x 683 x 3: the smallest test shape with two levels
    6220800: 0xE4F7BA5E3659F153,               # a 1080p 8-bit frame: 1519 hashes, then 3, then the final block
}

_cache = {}


def pattern(length, start=0):
    """byte[i] = ((x ^ (x >> 29)) >> 16) & 255 with x = i * 2654435761 mod 2^64, for i in start .. start + length - 1."""
    key = (int(length), int(start))
    if key not in _cache:
        with np.errstate(over="ignore"):
            x = np.arange(start, start + length, dtype=np.uint64) * np.uint64(2654435761)
        out = (((x ^ (x >> np.uint64(29))) >> np.uint64(16)) & np.uint64(255)).astype(np.uint8)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]
