"""The batch-1 frame entries' queue is stated once (frame_match_host in airslam_amd/csrc/airfe_frame.hip): airfe_track_frame and airfe_promote_frame hold their
argument checks and the values they vary, no copy, event, detector or matcher call of their own; the reference upload and the rows-home copy that records
ev_feat are one statement each for them and the keyframe; airfe.hip queues no pipeline."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")
PARENT_LINES = 6703          # airfe*.hip + airfe_host.h of the commit this split was made on (`git show <parent>:<file> | wc -l`, summed)
WG_PRIMS_HOOK_LINES = 70     # + airfe_debug_wg_prims with its one-workgroup kernel (airfe_debug.hip), the one entry point added since: the tree stood at 6702 before it
SG_FRONT_HOOK_LINES = 45     # + airfe_debug_sg_front (airfe_debug.hip); sg_front_dev, the statement it and both SuperGlue forwards call, took airfe_match.hip from 504 to 503 lines


def _code(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name calls; only code makes them


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "airfe*.hip")))


def test_track_and_promote_hold_no_queue_of_their_own():
    text = _code(os.path.join(CSRC, "airfe_frame.hip"))
    for entry in ("int airfe_track_frame(", "int airfe_promote_frame("):
        assert text.count(entry) == 1
        body = text[text.index(entry):]
        body = body[:body.index("} AIRFE_CATCH(")]
        assert "frame_match_host(" in body
        for call in ("hipMemcpyAsync", "hipEventRecord", "detect_dev(", "lightglue_dev(", "fransac_queue("):
            assert call not in body, (entry, call)


def test_feature_event_and_reference_count_are_stated_once():
    text = "".join(_code(s) for s in _sources())
    assert len(re.findall(r"hipEventRecord\(\s*c->ev_feat\b", text)) == 1
    assert len(re.findall(r"c->ref_n\s*=\s*n_ref\b", text)) == 1


def test_airfe_hip_queues_no_pipeline():
    text = _code(os.path.join(CSRC, "airfe.hip"))
    for call in ("detect_dev", "detect_dev2", "lightglue_dev", "superglue_dev", "line_branch_dev", "line_tail_dev", "launch_assign_points_to_lines", "launch_match_lines"):
        assert not re.search(r"\b" + call + r"\s*\(", text), call


def test_host_side_did_not_grow():
    total = 0
    for path in _sources() + [os.path.join(CSRC, "airfe_host.h")]:
        with open(path) as f:
            total += sum(1 for _ in f)
    assert total <= PARENT_LINES + WG_PRIMS_HOOK_LINES + SG_FRONT_HOOK_LINES, total
