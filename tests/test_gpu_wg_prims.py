"""The workgroup primitives of airslam_amd/csrc/wg_prims.h alone (Context.debug_wg_prims: one workgroup of 64 / 256 / 1024 threads walking its input in rounds with a
running base, as the production loops do), against numpy.  Integers and key orders only: every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
_S = {}


def _ctx():
    if "ctx" not in _S:
        from airslam_amd import api
        _S["ctx"] = api.Context()
    return _S["ctx"]


def _sizes(threads):
    return sorted({0, 1, 63, 64, 65, threads - 1, threads, threads + 1, 2 * threads + 17})


def _expect(v, keep, threads):
    """what the hook returns for (v, keep), restated with numpy"""
    v64, k = v.astype(np.int64), keep.astype(np.int64)
    first = np.zeros(threads, np.int64)
    first[:min(v.size, threads)] = v64[:threads]
    w = first.reshape(threads // 64, 64)
    return {"scan": np.cumsum(v64) - v64, "pos": np.cumsum(k) - k,
            "totals": np.array([v64.sum(), k.sum(), v64.sum(), v64.max() if v.size else I32.min, v64.min() if v.size else I32.max]),
            "wave": np.stack([w.sum(1), w.max(1), w.min(1)], axis=1)}


def _check(v, keep, threads):
    v, keep = np.asarray(v, np.int32), np.asarray(keep, np.uint8)
    got = _ctx().debug_wg_prims(v, keep, np.zeros((0,), np.uint32), threads)
    for name, want in _expect(v, keep, threads).items():
        assert np.array_equal(got[name].astype(np.int64), want), (name, threads, v.size)


@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_scan_compaction_and_reductions(threads):
    rng = np.random.default_rng(threads)
    for n in _sizes(threads):
        last = np.zeros(n, np.uint8)
        last[-1:] = 1
        for keep in (np.zeros(n, np.uint8), np.ones(n, np.uint8), last, (rng.random(n) < 0.5).astype(np.uint8)):
            for v in (rng.integers(0, 1001, n), np.zeros(n, np.int64)):
                _check(v, keep, threads)


@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_reductions_with_negative_values_and_the_extreme_in_the_last_lane(threads):
    rng = np.random.default_rng(7 * threads)
    for n in (threads, 2 * threads + 17):
        base = rng.integers(-1000, 1001, n)
        _check(base, np.ones(n, np.uint8), threads)
        for at in (threads - 1, n - 1):                        # the last lane of the last wave of the first round / the walk's last entry
            for extreme in (-100000, 100000):
                v = base.copy()
                v[at] = extreme
                _check(v, np.zeros(n, np.uint8), threads)
    _check(np.full(threads, -5), np.ones(threads, np.uint8), threads)      # every value negative: no 0 start value leaks into max


def _keys(rng, dtype, P, pad):
    """seeded keys with duplicates, then `pad` all-ones sentinels"""
    k = rng.integers(0, max(P // 3, 2), P).astype(dtype)
    if dtype == np.uint64:
        k = (k << np.uint64(32)) | rng.integers(0, 4, P).astype(np.uint64)      # both halves take part in the order
    k[P - pad:] = np.iinfo(dtype).max
    return k


@pytest.mark.parametrize("dtype,P,threads", [(np.uint64, 64, 256), (np.uint64, 256, 256), (np.uint64, 4096, 256), (np.uint32, 256, 256), (np.uint32, 8192, 256),
                                             (np.uint64, 1024, 1024)])
def test_sort(dtype, P, threads):
    rng = np.random.default_rng(P + threads)
    for pad in (0, 1, P - 1):
        keys = _keys(rng, dtype, P, pad)
        got = _ctx().debug_wg_prims(np.zeros(0, np.int32), np.zeros(0, np.uint8), keys, threads)["sorted"]
        assert got.dtype == dtype and np.array_equal(got, np.sort(keys)), (P, pad)
