"""The test hooks stage, wait and read back through one stream-ordered holder (HookStage in airslam_amd/csrc/airfe_debug.hip): outside its definition the file makes no
HIP allocation, fill, copy or wait of its own, so where a fill or an upload is ordered is decided in one place; nothing in the file fills on or waits for the null stream
(the context's non-blocking stream does not wait for it: LAB_NOTES.md, the two "second run of the suite failed" entries), and no hook holds a whole context as an
allocation list."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")
HIP_CALLS = ("hipMalloc(", "hipFree(", "hipMemset(", "hipMemsetAsync(", "hipMemcpy(", "hipMemcpyAsync(", "hipMemcpy2D(", "hipMemcpy2DAsync(", "hipStreamSynchronize(",
             "hipDeviceSynchronize(")


def _code(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name calls; only code makes them


def _split_holder(text):
    """(the holder's definition, everything else): `struct HookStage {` to the first `};` at the start of a line"""
    assert text.count("struct HookStage {") == 1
    a = text.index("struct HookStage {")
    b = text.index("\n};", a) + 3
    return text[a:b], text[:a] + text[b:]


def test_hooks_make_no_hip_call_of_their_own():
    holder, rest = _split_holder(_code("airfe_debug.hip"))
    for call in HIP_CALLS:
        assert call not in rest, call
    for call in ("hipMalloc(", "hipFree(", "hipMemsetAsync(", "hipMemcpyAsync(", "hipStreamSynchronize("):      # ... because the holder makes them
        assert call in holder, call


def test_nothing_on_the_null_stream_and_no_old_plumbing():
    text = _code("airfe_debug.hip")
    assert "hipMemset(" not in text
    assert not re.search(r"hipStreamSynchronize\(\s*(nullptr|0|NULL)\s*\)", text)
    assert not re.search(r"Async\([^;]*,\s*(nullptr|0|NULL)\s*\)\s*;", text)      # no fill or copy queued on the null stream either
    for name in ("DbgTmp", "dbg_canary", "dalloc<", "dupload("):
        assert name not in text, name
    assert "(void)hipMemcpy" not in text


def test_no_hook_holds_a_whole_context():
    assert not re.search(r"\bairfe_ctx\s+\w+\s*;", _code("airfe_debug.hip"))


def test_the_matcher_file_keeps_the_two_score_hooks():
    names = re.findall(r"^int (airfe_debug_[a-z0-9_]+)\(", _code("airfe_match.hip"), flags=re.M)
    assert sorted(names) == ["airfe_debug_lightglue_scores", "airfe_debug_superglue_scores"]
    moved = re.findall(r"^int (airfe_debug_[a-z0-9_]+)\(", _code("airfe_debug.hip"), flags=re.M)
    assert {"airfe_debug_lg_filter", "airfe_debug_sg_decode", "airfe_debug_sg_sinkhorn", "airfe_debug_sg_front"} <= set(moved)
