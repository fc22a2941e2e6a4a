"""The PLNet line path's launch sequences are stated once (the steps in airslam_amd/csrc/airfe_lines.hip): the test hooks in airfe_debug.hip and the entries in
airfe.hip, airfe_frame.hip and airfe_assoc.hip call the steps production is composed of and hold no launcher call of their own, so a pin on a hook is a pin on production's arguments, buffers and order."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")
LAUNCHERS = ("launch_s0_j2l", "launch_wireframe", "launch_s1_junc_rows", "launch_s1_junc_proj", "launch_s1h_junc_proj", "launch_plnet_s1", "launch_plnet_s1h",
             "launch_line_filter", "launch_junction_scan", "launch_s0_decode", "launch_s0_head_decode")
TWO_FORMS = {"launch_plnet_s1": 2}          # the CHW and the projected form may be two calls inside the one stage-1 step


def _calls(path):
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name launchers; only code calls them
    return {name: len(re.findall(r"\b" + name + r"\s*\(", text)) for name in LAUNCHERS}


def test_hooks_hold_no_line_path_launch():
    for src in ("airfe_debug.hip", "airfe.hip", "airfe_frame.hip", "airfe_assoc.hip"):
        calls = _calls(os.path.join(CSRC, src))
        assert not any(calls.values()), (src, {n: k for n, k in calls.items() if k})


def test_each_line_path_launch_is_stated_once():
    sources = sorted(glob.glob(os.path.join(CSRC, "airfe*.hip")))
    assert len(sources) >= 8
    total = {name: 0 for name in LAUNCHERS}
    for src in sources:
        for name, k in _calls(src).items():
            total[name] += k
    for name, k in total.items():
        assert 1 <= k <= TWO_FORMS.get(name, 1), (name, k)
