"""Damaged containers through the whole decoder (tests/damaged_containers.py; tests/test_damaged_containers_cpu.py classifies every case on
the CPU and proves the twin on the undamaged containers).  For every damage whose bytes still parse as a container:

  decompress_video, batched and frame by frame, and read_frames over the damaged record's run either return the twin's frames, bit for
  bit, or raise a plain ValueError that names the record the twin refuses -- never struct.error, IndexError, zlib.error, OverflowError,
  a numpy broadcasting error or an RbfError;
  with a trailer, IntegrityError.frame is the first frame whose digest the twin finds wrong, and on_mismatch="collect" lists exactly
  the twin's frames (verify_container too);
  after every refusal and every mismatch the same compressor object decodes the undamaged container bit for bit, at one lane and at two.

No case is sent in the expectation that it faults: DESIGN.md 7 has, per field that reaches a kernel argument, the host or C-ABI check
that bounds what the kernel reads and writes."""
import numpy as np
import pytest

import damaged_containers as dc
from new_bloom_filter_repo_amd import _native as nat
from new_bloom_filter_repo_amd import container
from new_bloom_filter_repo_amd.frame_codec import YUVFrame, frame_data
from new_bloom_filter_repo_amd.integrity import IntegrityError
from new_bloom_filter_repo_amd.verify import verify_container
from new_bloom_filter_repo_amd.video_compressor import ImprovedVideoCompressor

pytestmark = pytest.mark.gpu

GROUPS = [(dc.name_of(*cfg), g) for cfg in dc.CASE_CONFIGS for g in (("container", "key", "coded", "passthrough", "trailer") if dc.name_of(*cfg) in dc.FULL
                                                                      else ("container", "key", "coded"))]
GROUPS += [("rice_pan_digests", g) for g in ("rice_key", "rice_coded", "rice_passthrough", "pans")] + [("rice_pan", g) for g in ("rice_key", "rice_coded")]
GROUPS += [("rice_near_digests", g) for g in ("near_key", "rice_coded", "rice_passthrough")] + [("rice_near", g) for g in ("near_key", "rice_coded")]
CONFIG_NAMES = sorted({c for c, _ in GROUPS})


@pytest.fixture(scope="module")
def cases(oracle):
    out = []
    for c, d in dc.all_cases(oracle):
        try:
            records = container.parse(d.blob)
        except ValueError:
            continue                                               # the CPU tier holds what never parses
        out.append((c, d, records, dc.classify(oracle, c, d)))
    return out


@pytest.fixture(scope="module")
def compressors():
    made = {(lanes, batched): ImprovedVideoCompressor(gpu_lanes=lanes, gop_batching=batched, verbose=False) for lanes in (1, 2) for batched in (True, False)}
    yield made
    for comp in made.values():
        comp.close()


def same_frames(got, want, yuv=None):
    """Shape, dtype and bytes of every frame, and whether it comes back wrapped as a YUVFrame (yuv: per frame; None: none is)."""
    yuv = [False] * len(want) if yuv is None else list(yuv)
    return len(got) == len(want) and all(frame_data(g).shape == w.shape and frame_data(g).dtype == w.dtype and np.array_equal(frame_data(g), w)
                                         and isinstance(g, YUVFrame) == y for g, w, y in zip(got, want, yuv))


def refusal(call, record, what):
    """The call must raise a plain ValueError that names the record."""
    try:
        call()
    except IntegrityError as e:
        raise AssertionError((what, "an IntegrityError where the record cannot be decoded", str(e)))
    except ValueError as e:
        assert type(e) is ValueError and not isinstance(e, nat.RbfError), (what, type(e), str(e))
        assert "record" in str(e), (what, str(e))
        if record is not None:
            assert dc.names_record(str(e), record), (what, record, str(e))
        return
    raise AssertionError((what, "decoded what the twin refuses (record %s)" % record))


def run_span(records, record):
    """(start, stop) of the frames of the run the record lies in, its keyframe included; a keyframe alone: itself."""
    types = [ty for ty, _ in records if ty not in (dc.DIGESTS, dc.PANS)]
    record = min(record, len(types) - 1)
    start = max(i for i in range(record + 1) if types[i] in dc.KEYS) if any(types[i] in dc.KEYS for i in range(record + 1)) else 0
    stop = record + 1
    while stop < len(types) and types[stop] not in dc.KEYS:
        stop += 1
    return start, stop


def hold(comp, c, d, records, verdict, what):
    """One damaged container against one compressor object; returns True when the good container has to be decoded afterwards."""
    cls, twin = verdict
    aimed = d.record if d.record is not None else 0
    if cls == "refused":
        # (a changed LIST of records: more than one record may be the first to fail; a pan entry's error names the record it points at)
        strict = twin if d.name.split(".")[0] not in ("container", "pans") else None
        refusal(lambda: comp.decompress_video(compressed_frames=records), strict, (what, "decompress_video"))
        start, stop = run_span(records, twin)
        refusal(lambda: comp.read_frames(compressed_frames=records, start=start, stop=stop), strict, (what, "read_frames", start, stop))
        return True
    if not twin.bad:
        assert same_frames(comp.decompress_video(compressed_frames=records), twin.frames, twin.yuv), (what, "decompress_video")
        start, stop = run_span(records, aimed)
        assert same_frames(comp.read_frames(compressed_frames=records, start=start, stop=stop), twin.frames[start:stop], twin.yuv[start:stop]), (what, "read_frames")
        return cls != "benign"
    with pytest.raises(IntegrityError) as e:
        comp.decompress_video(compressed_frames=records)
    assert e.value.frame == twin.bad[0], (what, e.value.frame, twin.bad)
    got = comp.decompress_video(compressed_frames=records, on_mismatch="collect")
    assert same_frames(got, twin.frames, twin.yuv) and list(comp.last_bad_frames) == twin.bad, (what, comp.last_bad_frames, twin.bad)
    start, stop = run_span(records, twin.bad[0])
    with pytest.raises(IntegrityError) as e:
        comp.read_frames(compressed_frames=records, start=start, stop=stop)
    assert e.value.frame == twin.bad[0], (what, "read_frames", e.value.frame, twin.bad)
    got = comp.read_frames(compressed_frames=records, start=start, stop=stop, on_mismatch="collect")
    assert same_frames(got, twin.frames[start:stop], twin.yuv[start:stop]) and list(comp.last_bad_frames) == [i for i in twin.bad if start <= i < stop], (what, "read_frames, collect")
    return True


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("config,group", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_a_damaged_container_is_refused_or_decodes_as_the_twin_says(cases, compressors, config, group, lanes):
    mine = [x for x in cases if x[0].name == config and x[1].name.split(".")[0] == group]
    assert mine, "no case of this group parses"
    good = mine[0][0]
    for batched in (True, False):
        comp = compressors[lanes, batched]
        assert same_frames(comp.decompress_video(compressed_frames=good.records), good.frames), "the undamaged container"
        for c, d, records, verdict in mine:
            what = (config, d.name, "lanes=%d" % lanes, "batched" if batched else "frame by frame")
            if hold(comp, c, d, records, verdict, what):
                assert same_frames(comp.decompress_video(compressed_frames=good.records), good.frames), (what, "the good container afterwards")
    assert same_frames(compressors[lanes, True].read_frames(compressed_frames=good.records, start=1, stop=12, step=2), good.frames[1:12:2])


@pytest.mark.parametrize("config", [n for n in CONFIG_NAMES if n.endswith("digests")])
def test_verify_container_lists_the_twins_frames(cases, config):
    """Every case with a trailer whose damage still decodes (verify_container makes a compressor of its own per call)."""
    seen = 0
    for c, d, records, (cls, twin) in cases:
        if c.name == config and cls == "other" and twin.bad is not None:
            report = verify_container(d.blob)
            assert report["bad"] == twin.bad and report["trailer"] == "ok" and report["frames"] == len(twin.frames), (d.name, report)
            seen += 1
    assert seen >= 5, seen


def test_a_record_damaged_outside_the_span_is_not_decoded(cases, compressors):
    """read_frames plans from the record types alone: a refused record in the second run does not keep the first run from being read."""
    comp = compressors[1, True]
    seen = 0
    for c, d, records, (cls, twin) in cases:
        if cls == "refused" and twin is not None and 7 <= twin <= 11 and d.name.split(".")[0] in ("coded", "rice_coded") and [ty for ty, _ in records[:13]] == [ty for ty, _ in c.records[:13]]:
            assert same_frames(comp.read_frames(compressed_frames=records, start=0, stop=6), c.frames[:6]), d.name
            seen += 1
    assert seen >= 20
