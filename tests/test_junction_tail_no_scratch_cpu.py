"""Build-time guard for the junction tail's kernels, as tests/test_no_scratch_cpu.py holds the other hot kernels: the line filter that builds the junction list in LDS
and every instantiation of the sampling gather GEMM (both slot layouts, both 2-byte types) compile without scratch; their register and LDS figures are recorded."""
import re

from gpu_common import diag
from test_no_scratch_cpu import _compile

KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs", "AGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def _figures(src):
    out, name = {}, None
    for line in _compile(src)[0].splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def test_junction_tail_kernels_use_no_scratch():
    found = {}
    for src, frag in (("kernels_ext.hip", "line_filter_junc_kernel"), ("kernels_gemmr_sample.hip", "gemmr_gather_kernel_sample")):
        for name, u in _figures(src).items():
            if frag in name:
                found[name] = u
                print(name, u)
                assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    sample = [n for n in found if "gemmr_gather_kernel_sample" in n]
    assert len(sample) == 4 and sum("sample_junc" in n for n in sample) == 2 and len(found) == 5
    # the filter's static LDS: the 512 x 512-bit map and the scan's 16 words; the GEMM's LDS is dynamic (sized by the launcher)
    lf = [u for n, u in found.items() if "line_filter_junc_kernel" in n][0]
    assert lf["LDS Size [bytes/block]"] == 512 * 512 // 8 + 64
    diag("junction_tail_kernel_resources", **{n: str(u) for n, u in found.items()})
