"""The host side of the keyframe database (airslam_amd/csrc/airfe_bowdb.h, airfe_bowdb.hip, airfe_bowmap.hip, airfe_junction.hip) states each thing once: the dense
query and every other database launch have one call site, the database's device memory has one owner (DevBlock / reserve / release: no allocation call of its
own), and the default of a `stream` argument is stream_of (airfe_host.h), never spelled out."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")
BOW_HOST = ("airfe_bowdb.h", "airfe_bowdb.hip", "airfe_bowmap.hip", "airfe_junction.hip")
ONCE = ("launch_bowdb_query", "launch_bowdb_select", "launch_loopdet_select", "launch_bowgroup", "launch_covis_build", "launch_covis_segments", "launch_triangulate",
        "launch_junction_keys", "launch_junction_term", "launch_junction_connect")


def _code(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name launchers; only code calls them


def test_each_database_launch_is_stated_once():
    sources = sorted(glob.glob(os.path.join(CSRC, "airfe*.hip")))
    assert len(sources) >= 11 and {"airfe_bowdb.hip", "airfe_bowmap.hip", "airfe_junction.hip"} <= {os.path.basename(s) for s in sources}
    text = "".join(_code(s) for s in sources)
    for name in ONCE:
        assert len(re.findall(r"\b" + name + r"\s*\(", text)) == 1, name


def test_the_database_allocates_through_blocks_only():
    for name in BOW_HOST:
        text = _code(os.path.join(CSRC, name))
        for call in ("hipMalloc", "hipFree"):
            assert not re.search(r"\b" + call + r"\s*\(", text), (name, call)


def test_the_stream_default_is_spelled_out_nowhere():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(sources) >= 40
    for src in sources:
        assert not re.search(r"\?\s*\(\s*hipStream_t\s*\)\s*stream\s*:", _code(src)), os.path.basename(src)
    host = _code(os.path.join(CSRC, "airfe_host.h"))
    assert len(re.findall(r"\bstream_of\s*\(", host)) == 1                   # its definition
    calls = sum(len(re.findall(r"\bstream_of\s*\(", _code(s))) for s in sources) - 1
    assert calls >= 40, calls
