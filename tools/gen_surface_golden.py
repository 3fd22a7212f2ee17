#!/usr/bin/env python3
"""Write (or, with --check, compare) the two fixtures that pin the video surface's behaviour: tests/golden/surface_refusals.json (no GPU)
and tests/golden/surface_containers.json (one GPU).  tests/surface_golden.py has the grid, the clips and the configurations; this tool
only runs them against whatever `new_bloom_filter_repo_amd` the interpreter finds first -- put another checkout's directory in front on
PYTHONPATH to pin or check that one.

Usage: python tools/gen_surface_golden.py [--check] [--only refusals|containers] [--out DIR]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)                            # (behind PYTHONPATH: a checkout named there wins)
sys.path.insert(0, os.path.join(REPO, "tests"))

import surface_golden as sg  # noqa: E402


def refusals():
    from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor
    outcomes, index = sg.refusal_table(ImprovedVideoCompressor)
    return {"grid": sg.grid_description(), "dropped_values": [], "order": "itertools.product over the grid, the last keyword fastest",
            "outcomes": outcomes, "counts": [index.count(sg.SYMBOLS[i]) for i in range(len(outcomes))], "index": index}


def containers():
    doc = {"frames": sg.T, "width": sg.W, "height": sg.H, "keyframe_interval": sg.I, "block_frames": sg.B, "entries": {}}
    for name, _, _, _ in sg.CONFIGS:
        doc["entries"][name] = sg.run_config(name)
    e = doc["entries"]
    for a, b in sg.SAME_BYTES:
        assert e[a]["canonical_sha256"] == e[b]["canonical_sha256"], (a, b)
    p = e["pan_cut_digests_quality"]             # the cut sits inside a panned run: frames in front of it and behind it carry offsets
    assert p["scene_cuts"] == [10] and "9" in p["pan_offsets"] and "11" in p["pan_offsets"], p
    return doc


def extends(what, old, new):
    """Writing over a committed fixture may only ADD to it: a grid that grew by keywords keeps the recorded outcome of every old
    combination (the new keywords at their first value, the default), and every recorded container entry stays as it is.  Returns what
    was compared, for the log; AssertionError otherwise."""
    if what == "containers":
        for name, entry in old["entries"].items():
            assert new["entries"].get(name) == entry, "container entry %r changed" % name
        return "%d recorded entries unchanged, %d new" % (len(old["entries"]), len(new["entries"]) - len(old["entries"]))
    names = [name for name, _ in sg.GRID]        # (product order; the files are written with sorted keys)
    assert set(names) == set(new["grid"]) >= set(old["grid"]) and all(new["grid"][n] == v for n, v in old["grid"].items()), "the grid's old axes changed"
    sizes = [len(new["grid"][n]) for n in names]
    added = [n not in old["grid"] for n in names]
    restricted, stride = [], 1
    strides = []
    for size in reversed(sizes):
        strides.insert(0, stride)
        stride *= size
    import itertools
    for idx in itertools.product(*[range(1 if a else size) for a, size in zip(added, sizes)]):
        restricted.append(new["outcomes"][sg.SYMBOLS.index(new["index"][sum(i * st for i, st in zip(idx, strides))])])
    recorded = [old["outcomes"][sg.SYMBOLS.index(ch)] for ch in old["index"]]
    assert restricted == recorded, "an old combination's outcome changed"
    return "%d recorded outcomes unchanged under %s at their defaults" % (len(recorded), [n for n, a in zip(names, added) if a])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    ap.add_argument("--only", choices=("refusals", "containers"))
    ap.add_argument("--out", help="directory to write to (default: tests/golden)")
    args = ap.parse_args()
    bad = 0
    for what, make, path in (("refusals", refusals, sg.REFUSALS), ("containers", containers, sg.CONTAINERS)):
        if args.only and args.only != what:
            continue
        doc = json.loads(json.dumps(make()))
        if args.check:
            same = doc == sg.load(path)
            print("%s: %s" % (os.path.basename(path), "identical" if same else "DIFFERENT"))
            bad += not same
            continue
        if os.path.exists(path):
            print("%s: %s" % (os.path.basename(path), extends(what, sg.load(path), doc)))
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            path = os.path.join(args.out, os.path.basename(path))
        with open(path, "w", encoding="utf-8") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
