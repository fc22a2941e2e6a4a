"""The kernels' workgroup primitives are written once, in airslam_amd/csrc/wg_prims.h (scan, compaction, reductions, sort), and the helpers the *_core.h headers
share once, in core_common.h (the host/device switch, the count clamp, the NaN facts).  Source text with the comments stripped, as
tests/test_matcher_one_block_cpu.py reads it: a copy of a primitive shows up here as the instruction pattern it cannot be written without."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "airslam_amd", "csrc")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))


def _code(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # comments name calls; only code makes them


def _files_with(pattern):
    return {name for name in SOURCES if re.search(pattern, _code(name))}


def test_the_shuffle_scan_is_written_once():
    assert _files_with(r"__shfl_up") == {"wg_prims.h"}


def test_the_ballot_prefix_is_written_once_outside_the_exempt_kernels():
    # kernels_ext.hip: wf_emit_kernel, wireframe_kernel and the wave-per-line pl_assign_kernel walk runs of 64 per WAVE; kernels_nms512.hip compacts several registers
    assert _files_with(r"1ull << lane") == {"wg_prims.h", "kernels_ext.hip", "kernels_nms512.hip"}


def test_one_host_device_switch():
    assert _files_with(r"#define \w+_HD ") == {"core_common.h"}


def test_one_count_clamp():
    assert _files_with(r"< 0 \? 0 : \(\w+ > ") == {"core_common.h"}


@pytest.mark.parametrize("name", ["jn_scan256", "block_scan256", "block_excl_scan_1024", "bg_block_sum", "jn_sort", "jn_wave_sum", "mg_count", "po_clamp", "prob_n",
                                  "clampi"])
def test_the_private_copies_are_gone(name):
    assert not _files_with(r"\b%s\b" % name)


@pytest.mark.parametrize("name,kernel,calls", [
    ("kernels_pnp.hip", "pnp_gather_kernel", 1), ("kernels_bowgroup.hip", "reloc_gather_kernel", 1), ("kernels_loopdet.hip", "loopdet_select_kernel", 1),
    ("kernels_loopdet.hip", "loopdet_gather_kernel", 1), ("kernels_fransac.hip", "fransac_compact_kernel", 1), ("kernels_covis.hip", "covis_emit_kernel", 1),
    ("kernels_bowdb.hip", "bowdb_select_kernel", 1)])
def test_the_ordered_compactions_call_the_primitive(name, kernel, calls):
    text = _code(name)
    body = text[text.index("void %s(" % kernel):]
    body = body[:body.index("__global__")] if "__global__" in body else body
    assert body.count("block_compact<") == calls
