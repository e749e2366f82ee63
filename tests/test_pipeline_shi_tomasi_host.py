"""Host side of the Shi-Tomasi re-detect of the device-resident KLT loop (vo_pipeline_config.detector = 1): the oracle
loop's cases (tests/pipeline_shi_tomasi_oracle.py) re-detect where and with the counts the GPU tests rely on; the ctypes
mirror of the configuration's new tail matches include/vo_hip.h; the Python keywords map names to values."""
import ctypes as C
import os
import re

import pytest

import pipeline_shi_tomasi_oracle as sto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_oracle_cases_redetect_where_and_with_the_counts_the_gpu_tests_expect(name):
    """Cases A-D: one re-detect, at the step from frame 2 to frame 3; A gets the detector's cap (300), B, C and D fewer and
    each a different count, which is what _num_features is afterwards (klt.py:114)."""
    _, _, _, _, when, count = sto.CASES[name]
    stream, feats, T, pairs, refs = sto.run_case(name)
    assert feats.length == int(0.83 * sto.N)
    assert pairs[when] == (2, 3)
    assert [r["redetected"] for r in refs] == [1 if k == when else 0 for k in range(len(pairs))]
    r = refs[when]
    assert r["appended"] == count and r["num_features"] == count
    assert r["detection"].shape == (count, 2)
    for k, ref in enumerate(refs):
        assert ref["num_features"] == (sto.N if k < when else count)
    # before the re-detect the limit is 0.8 * 300; the step that re-detects starts below it
    assert refs[when]["n_before"] < 0.8 * sto.N <= refs[when - 1]["n_before"]


def test_a_full_start_state_redetects_later():
    """Fraction 1.0 with (0.01, 8): the tracks last longer, the re-detect comes at the step from frame 5 back to 4."""
    _, _, _, pairs, refs = sto.run_case("A", fraction=1.0)
    when = [k for k, r in enumerate(refs) if r["redetected"]]
    assert when == [5] and pairs[5] == (5, 4)


def _header_config_fields():
    text = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    start = "typedef struct vo_pipeline_config {"
    body = text[text.index(start) + len(start):text.index("} vo_pipeline_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|int64_t|double)\s+(.*)$", decl.strip(), flags=re.S)
        if not m:
            continue
        for name in m.group(2).split(","):
            name = name.strip()
            k = re.match(r"(\w+)\[(\d+)\]$", name)
            fields.append((k.group(1), m.group(1), int(k.group(2))) if k else (name, m.group(1), 1))
    return fields


def test_config_mirror_matches_the_header():
    """Every field of vo_pipeline_config, in order, with the header's type; the new tail -- detector, st_block,
    st_quality, st_min_distance -- at the end, 24 bytes, so that a zeroed tail is the configuration as it was."""
    from vo import _native
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    header = _header_config_fields()
    mirror = _native.PipelineConfig._fields_
    assert [f[0] for f in mirror] == [h[0] for h in header]
    for (name, ctype), (_, htype, count) in zip(mirror, header):
        assert ctype == (ctypes_of[htype] * count if count > 1 else ctypes_of[htype]), name
    assert [h[0] for h in header[-4:]] == ["detector", "st_block", "st_quality", "st_min_distance"]
    P = _native.PipelineConfig
    end_before = P.match_ratio.offset + 8
    assert (P.detector.offset, P.st_block.offset, P.st_quality.offset, P.st_min_distance.offset) == (
        end_before, end_before + 4, end_before + 8, end_before + 16)
    assert C.sizeof(P) == end_before + 24
    z = P()
    assert (z.detector, z.st_block, z.st_quality, z.st_min_distance) == (0, 0, 0.0, 0.0)


class _FakeLib:
    """Stands in for libvo_hip.so under Pipeline.__init__: keeps the configuration it was given."""

    def __init__(self):
        self.cfg = None

    def vo_pipeline_create(self, h, cfg_ref, out):
        from vo import _native
        self.cfg = _native.PipelineConfig.from_buffer_copy(cfg_ref._obj)
        return 0

    def vo_pipeline_feature_cap(self, h):
        return 600

    def vo_pipeline_seed(self, h, pcg):
        return 0

    def vo_pipeline_destroy(self, h):
        return None


class _FakeCtx:
    def __init__(self):
        self._lib, self._h, self._pipelines = _FakeLib(), None, set()

    def _chk(self, rc):
        assert rc == 0


def test_python_keywords_reach_the_configuration():
    import numpy as np
    from vo import _native
    from vo._pipeline import DETECTORS
    assert DETECTORS == {"harris": 0, "shi-tomasi": 1}
    K = np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]])
    ctx = _FakeCtx()
    p = _native.Pipeline(ctx, 240, 320, 4, K, n_keypoints=300)
    c = ctx._lib.cfg
    assert (c.detector, c.st_block, c.st_quality, c.st_min_distance) == (0, 0, 0.0, 0.0) and p.detector == "harris"
    p = _native.Pipeline(ctx, 240, 320, 4, K, n_keypoints=300, detector="shi-tomasi", st_quality=0.02, st_min_distance=14,
                         st_block=5)
    c = ctx._lib.cfg
    assert (c.detector, c.st_block, c.st_quality, c.st_min_distance) == (1, 5, 0.02, 14.0) and p.detector == "shi-tomasi"
    assert c.n_keypoints == 300 and c.tracker_mode == 0
    with pytest.raises(KeyError):
        _native.Pipeline(ctx, 240, 320, 4, K, detector="fast")


def test_drivers_take_the_detector_and_default_to_harris():
    import inspect
    from vo import driver
    for fn in (driver.run_on_device, driver.run_batch_on_device):
        assert inspect.signature(fn).parameters["detector"].default == "harris"
    assert driver._pipeline_kwargs(None, 300, 15, 2, 256, "current")["detector"] == "harris"
    assert driver._pipeline_kwargs(None, 300, 15, 2, 256, "current", "shi-tomasi")["detector"] == "shi-tomasi"
